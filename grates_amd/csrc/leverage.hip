// Leverages of observations: out[j] = |U^-T x_j|^2 = x_j^T N^-1 x_j for the columns x_j of X [n][ldx] and the upper triangular
// inverse Ui = U^-1 of the Cholesky factor of N (shg_leverages; no reference counterpart)
//   Z = Ui^T X is formed tile by tile on the fp64 MFMA (v_mfma_f64_16x16x4_f64) and never written: the epilogue squares the
//   accumulators and sums them over the rows of the tile.
// Workgroup = (row tile t of 128 rows of Z, column tile of 128 columns), 4 waves as 2 x 2, wave tile 64 x 64 (16 accumulators),
// BK = 16.  Row p of Z sums over q <= p only, so the K range of row tile t ends with its diagonal block, q < min(n, 128 t + 128):
// half the MFMAs of the full product.  The row tiles are taken from the last (longest) to the first.  Both operands are read along
// their rows (Ui[q][p0 ..] and X[q][j0 ..]: 128 consecutive doubles per k-row, the same thread map for both) and staged k-major,
// so both fragments are "k-row (lane >> 4), element (lane & 15)" reads of a [16][144] image without bank conflicts.  Entries of
// Ui below the diagonal are replaced by zeros while a tile of the diagonal block is staged (they may hold anything, NaN included),
// and so are the k-rows from n on of the last K tile.
// Every tile writes the sums of its 128 rows to partial[t][j]; leverage_sum_kernel adds the row tiles in ascending order.  No
// atomics; the K order is ascending from q = 0 in steps of 4 whatever the column, the epilogue order is fixed by the row alone, so
// out[j] depends on n, Ui and column j only.
// The tile, its K loop and the loads "uniform 64-bit row base + per-lane 32-bit byte offset" are those of mfma_tile.h.
#include "mfma_tile.h"

namespace shg {
namespace {

constexpr int LT = 128;        // rows of Z and columns per workgroup
constexpr int LK = 16;         // K tile
constexpr int LLD = 144;       // k-row of a staged tile: 128 + 16 doubles of padding (the four k-rows of a fragment read fall on distinct banks)

__global__ __launch_bounds__(256, 2) void leverage_kernel(int n, long long cols, const double* __restrict__ Ui, int ldu, const double* __restrict__ X,
                                                           long long ldx, double* __restrict__ partial, long long col_base) {
    extern __shared__ double lds[];                    // [buffer][Ui^T tile | X tile][16][144]: 73.7 KB, two workgroups per CU
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int fr = lane & 15, fk = lane >> 4;
    const int c = tid & 127;                                          // column of both tiles a thread fetches
    const int kh = __builtin_amdgcn_readfirstlane(tid >> 7);          // ... in the k-rows kh, kh + 2, ..., kh + 14 (wave-uniform)

    const int t = (int)(gridDim.y - 1 - blockIdx.y);                  // longest row tiles first
    const int p0 = t * LT;
    const long long j0 = col_base + (long long)blockIdx.x * LT;
    const int kend = min(n, p0 + LT);                                 // q < kend: the diagonal block closes the K range
    const int nt = (kend + LK - 1) / LK;

    // clamped columns stay inside the matrices: what they deliver only reaches rows of Z that the epilogue leaves out and columns
    // that are not stored
    const unsigned u_off = (unsigned)(min(p0 + c, n - 1) - p0) * 8u;
    const unsigned x_off = (unsigned)(min(j0 + c, cols - 1) - j0) * 8u;
    const double* u_base = Ui + p0;
    const double* x_base = X + j0;

    double ureg[8], xreg[8];
    auto fetch = [&](int i) {
        const int k0 = i * LK;
#pragma unroll
        for (int h = 0; h < 8; ++h) {
            const int q = min(k0 + kh + 2 * h, n - 1);                // uniform; only the last K tile can reach n
            ureg[h] = load_uniform_base(u_base + (size_t)q * ldu, u_off);
            xreg[h] = load_uniform_base(x_base + (size_t)q * ldx, x_off);
        }
    };
    double* stage_base = lds + kh * LLD + c;
    auto stage = [&](int buf, int i) {
        const int k0 = i * LK;
        double* As = stage_base + buf * (2 * LK * LLD);
        double* Bs = As + LK * LLD;
        const bool masked = (k0 + LK - 1 > p0) || (k0 + LK > n);      // uniform: tiles of the diagonal block, and the last one
#pragma unroll
        for (int h = 0; h < 8; ++h) {
            double u = ureg[h], x = xreg[h];
            if (masked) {
                const int q = k0 + kh + 2 * h;
                u = (q <= p0 + c && q < n) ? u : 0.0;
                x = q < n ? x : 0.0;
            }
            As[2 * h * LLD] = u;
            Bs[2 * h * LLD] = x;
        }
    };

    double4_t acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = (double4_t){0.0, 0.0, 0.0, 0.0};

    // every fragment is one ds_read_b64 "lane base + immediate" (lds_double_t of mfma_tile.h)
    const lds_double_t* a_frag = (const lds_double_t*)(lds + fk * LLD + wr * 64 + fr);
    const lds_double_t* b_frag = (const lds_double_t*)(lds + LK * LLD + fk * LLD + wc * 64 + fr);
    asm volatile("" : "+v"(a_frag));
    asm volatile("" : "+v"(b_frag));
    auto multiply = [&](int buf) {
        const volatile lds_double_t* Ab = a_frag + buf * (2 * LK * LLD);
        const volatile lds_double_t* Bb = b_frag + buf * (2 * LK * LLD);
        tile_multiply<4, 4 * LLD, 16, 4 * LLD, 16>(Ab, Bb, acc);
    };
    SHG_TILE_PIPELINE(nt, fetch, stage, multiply);

    // ---- epilogue.  C/D layout: column = lane & 15, row = (lane >> 4) + 4 * reg.  A lane sums the squares of its 16 rows of a
    //      column in ascending (a, reg) order, the four lanes of a column close as (s + s^16) + (s + s^16)^32, then wr 0 + wr 1.
    double* red = lds;                                                // [2 wr][128 columns]: every wave is past the last barrier
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double v = (p0 + wr * 64 + a * 16 + fk + 4 * r < n) ? acc[a][b][r] : 0.0;
                s = fma(v, v, s);
            }
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        if (fk == 0) red[wr * LT + wc * 64 + b * 16 + fr] = s;
    }
    __syncthreads();
    if (tid < LT && j0 + tid < cols) partial[(long long)t * cols + j0 + tid] = red[tid] + red[LT + tid];
}

__global__ __launch_bounds__(256) void leverage_sum_kernel(int tiles, long long count, long long cols, const double* __restrict__ partial,
                                                               double* __restrict__ out) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    double s = partial[j];
    for (int t = 1; t < tiles; ++t) s += partial[(long long)t * cols + j];
    out[j] = s;
}

}  // namespace
}  // namespace shg

using namespace shg;

extern "C" int shg_leverages(int n, long long cols, const double* Ui, int ldu, const double* X, long long ldx, double* out, void* stream_) {
    SHG_REQUIRE(n >= 0 && cols >= 0, "shg_leverages: negative size (n %d, cols %lld)", n, cols);
    SHG_REQUIRE(ldu >= n, "shg_leverages: ldu %d below n %d", ldu, n);
    SHG_REQUIRE(ldx >= cols, "shg_leverages: ldx %lld below the %lld columns", ldx, cols);
    const long long kMost = 1LL << 40;
    SHG_REQUIRE((long long)n * ldu <= kMost && (n == 0 || ldx <= kMost / n) && cols <= kMost, "shg_leverages: n %d, ldu %d, ldx %lld is too large",
                n, ldu, ldx);
    if (cols == 0) return SHG_OK;
    SHG_REQUIRE(out != nullptr && ((Ui != nullptr && X != nullptr) || n == 0), "shg_leverages: NULL pointer");
    hipStream_t stream = (hipStream_t)stream_;
    if (n == 0) return zero_fill(out, cols, cols, 1, stream);
    const int tiles = ceil_div(n, LT);
    ScratchLease lease(stream);                       // held until the kernel that adds the row tiles is enqueued
    double* partial = (double*)lease.get(kScratchSplitK, (size_t)tiles * (size_t)cols * sizeof(double));
    if (!partial) return fail(SHG_ERR_NOMEM, "shg_leverages: workspace of %d x %lld doubles", tiles, cols);
    const size_t lds_bytes = (size_t)2 * 2 * LK * LLD * sizeof(double);
    SHG_SET_LDS_ONCE(leverage_kernel, lds_bytes);
    const long long coltiles = ceil_div64(cols, LT);
    const long long kChunk = 1LL << 22;               // column tiles of one launch
    for (long long first = 0; first < coltiles; first += kChunk) {
        const unsigned gx = (unsigned)std::min(kChunk, coltiles - first);
        hipLaunchKernelGGL(leverage_kernel, dim3(gx, (unsigned)tiles), dim3(256), lds_bytes, stream, n, cols, Ui, ldu, X, ldx, partial, first * LT);
        SHG_HIP(hipGetLastError());
    }
    const long long kSumChunk = (1LL << 30);          // columns of one launch of the sum
    for (long long first = 0; first < cols; first += kSumChunk) {
        const long long count = std::min(kSumChunk, cols - first);
        // (a column offset moves all three pointers alike: row tile t of the chunk is at partial + first + t cols)
        hipLaunchKernelGGL(leverage_sum_kernel, dim3((unsigned)ceil_div64(count, 256)), dim3(256), 0, stream, tiles, count, cols, partial + first,
                           out + first);
        SHG_HIP(hipGetLastError());
    }
    return SHG_OK;
}

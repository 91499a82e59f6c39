// Basin covariance C = F S F^T for B <= 64 functionals F [B][n] and a symmetric S [n][n] of which only the upper triangle is read
// (shg_basin_covariance).
//
// With U = the strict upper triangle of S plus half its diagonal, S = U + U^T and C = G + G^T, G = (F U) F^T.  The triangle is cut into
// column blocks of kCovTC columns; column block J holds the rows 0 .. j0 + kCovTC, split into work items of q * kCovTC rows so that
// the launch has about two thousand items of equal length (a whole triangle of column blocks would leave the short ones idle at the
// end).  An item (J, rows k0 .. k1) computes
//   Y^T [c][b] = sum_k U[k][j0 + c] F[b][k]            fp64 MFMA, S and F staged through two LDS stages 16 rows at a time, two chunks in flight
//   P [b'][b]  = sum_c F[b'][j0 + c] Y^T[c][b]         fp64 MFMA on the accumulators of Y^T as they are (their row index is the sum's)
// and writes P to its own slot: every element on or above the diagonal of S is read from memory once, none below it (the
// diagonal block masks them before they are loaded).  The partials are summed in a fixed order by two small kernels (groups of
// items, then the groups), C[b][b'] = G[b][b'] + G[b'][b] with both sums formed identically: C is exactly symmetric and
// repeated calls are bitwise equal.  No atomics.
//
// Fragments of v_mfma_f64_16x16x4f64 (lane l): A[row l & 15][k l >> 4], B[k l >> 4][col l & 15], D[row (l >> 4) + 4 reg][col l & 15].
// Waves split the kCovTC columns (two 16-column tiles each), all RT 16-row tiles of the functionals (RT = ceil(B / 16)).
#include "common.h"

#include <cmath>

namespace shg {

constexpr int kCovTC = 128;            // columns of S per item
constexpr int kCovKC = 16;             // rows of S per LDS chunk
constexpr int kCovItems = 4096;        // aim: at least this many items (4 workgroups on each of 256 CUs, four times over: a short last round)
constexpr int kCovSP = kCovTC + 2;     // LDS row pitch of the S chunk
constexpr int kCovFP = kCovKC + 1;     // LDS row pitch of the F chunk

typedef double cov_double4 __attribute__((ext_vector_type(4)));
typedef double double2_t __attribute__((ext_vector_type(2)));

// item -> (column block J, first row k0): column blocks longest first, then their row pieces in ascending order
__device__ __forceinline__ void cov_item(int item, int nblocks, int n, int q, int& J, int& k0) {
    for (J = nblocks - 1; J > 0; --J) {
        const int height = min((J + 1) * kCovTC, n);
        const int pieces = (height + q * kCovTC - 1) / (q * kCovTC);
        if (item < pieces) break;
        item -= pieces;
    }
    k0 = item * q * kCovTC;
}

template <int RT, bool VEC>
__global__ __launch_bounds__(256) void basin_cov_kernel(int B, int n, int q, const double* __restrict__ F, int ldf, const double* __restrict__ S,
                                                        long long lds, double* __restrict__ partial) {
    constexpr int BP = 16 * RT;
    constexpr int SL_SIZE = kCovKC * kCovSP, FL_SIZE = BP * kCovFP, RED_SIZE = 4 * 16 * BP;
    constexpr int STAGE = SL_SIZE + FL_SIZE;       // one LDS stage: S chunk [kCovKC][kCovSP], F chunk [BP][kCovFP]
    constexpr int LDS = (2 * STAGE > RED_SIZE) ? 2 * STAGE : RED_SIZE;
    constexpr int FE = BP * kCovKC / 256;          // F elements per thread and chunk
    __shared__ __attribute__((aligned(16))) double lds_buf[LDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    const int nblocks = (n + kCovTC - 1) / kCovTC;
    int J, k0;
    cov_item(blockIdx.x, nblocks, n, q, J, k0);
    const int j0 = J * kCovTC;
    const int k1 = min(k0 + q * kCovTC, min(j0 + kCovTC, n));

    // S chunk: pair e of thread t is idx = 256 e + t -> row idx / 64, columns 2 (idx % 64) + 0, 1 (a wave reads 1 KB contiguous); VEC
    // (even lds, 16-byte aligned S) loads a pair whose two elements are both wanted as one 16-byte load
    struct Regs {
        double s[8];
        double f[FE];
    };
    Regs ra, rb;
    auto fetch = [&](Regs& r, int kk) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int idx = 256 * e + tid;
            const int k = kk + idx / (kCovTC / 2), j = j0 + 2 * (idx % (kCovTC / 2));
            double v0 = 0.0, v1 = 0.0;
            if (k < k1) {                            // nothing below the diagonal is loaded
                const double* src = S + (size_t)k * lds + j;
                if (VEC && k <= j && j + 1 < n) {
                    const double2_t v = *reinterpret_cast<const double2_t*>(src);
                    v0 = v.x, v1 = v.y;
                } else {
                    if (k <= j && j < n) v0 = src[0];
                    if (k <= j + 1 && j + 1 < n) v1 = src[1];
                }
                if (k == j) v0 *= 0.5;
                if (k == j + 1) v1 *= 0.5;
            }
            r.s[2 * e] = v0;
            r.s[2 * e + 1] = v1;
        }
#pragma unroll
        for (int e = 0; e < FE; ++e) {
            const int idx = 256 * e + tid;
            const int b = idx / kCovKC, k = kk + idx % kCovKC;
            r.f[e] = (b < B && k < k1) ? F[(size_t)b * ldf + k] : 0.0;
        }
    };
    auto stage = [&](const Regs& r, int buf) {
        double* SL = lds_buf + buf * STAGE;
        double* FL = SL + SL_SIZE;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int idx = 256 * e + tid;
            double* dst = SL + (idx / (kCovTC / 2)) * kCovSP + 2 * (idx % (kCovTC / 2));
            dst[0] = r.s[2 * e];
            dst[1] = r.s[2 * e + 1];
        }
#pragma unroll
        for (int e = 0; e < FE; ++e) {
            const int idx = 256 * e + tid;
            FL[(idx / kCovKC) * kCovFP + idx % kCovKC] = r.f[e];
        }
    };

    cov_double4 acc[2][RT];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int bt = 0; bt < RT; ++bt) acc[ct][bt] = cov_double4{0.0, 0.0, 0.0, 0.0};
    auto compute = [&](int buf) {
        const double* SL = lds_buf + buf * STAGE;
        const double* FL = SL + SL_SIZE;
#pragma unroll
        for (int s = 0; s < kCovKC / 4; ++s) {
            double a[2], bf[RT];
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) a[ct] = SL[(4 * s + lk) * kCovSP + 16 * (wave + 4 * ct) + lr];   // the wave's columns 16 wave .., 64 + 16 wave ..
#pragma unroll
            for (int bt = 0; bt < RT; ++bt) bf[bt] = FL[(16 * bt + lr) * kCovFP + 4 * s + lk];
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int bt = 0; bt < RT; ++bt) acc[ct][bt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ct], bf[bt], acc[ct][bt], 0, 0, 0);
        }
    };
    // Two chunks in flight: chunk c + 1 waits in one register set while chunk c + 2 is requested into the other; chunk c is
    // multiplied from LDS stage c & 1 while chunk c + 1 is written to the other stage -- one barrier per chunk.
    auto step = [&](int kk, int buf, Regs& next, Regs& later) {
        if (kk + 2 * kCovKC < k1) fetch(later, kk + 2 * kCovKC);
        compute(buf);
        if (kk + kCovKC < k1) stage(next, buf ^ 1);
        __syncthreads();
    };
    fetch(ra, k0);
    if (k0 + kCovKC < k1) fetch(rb, k0 + kCovKC);
    stage(ra, 0);
    __syncthreads();
    for (int kk = k0; kk < k1; kk += 2 * kCovKC) {
        step(kk, 0, rb, ra);
        if (kk + kCovKC < k1) step(kk + kCovKC, 1, ra, rb);
    }
                                                   // (the last step ended with a barrier: the LDS now holds the reduction slots RED [wave][16][BP])

    // P [b'][b] = sum_c F[b'][j0 + c] Y^T[c][b]: register s of a Y^T tile is the B fragment of k step s
    double* RED = lds_buf;
    double* out = partial + (size_t)blockIdx.x * BP * BP;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        cov_double4 g[RT];
#pragma unroll
        for (int bt = 0; bt < RT; ++bt) g[bt] = cov_double4{0.0, 0.0, 0.0, 0.0};
        const int brow = 16 * rt + lr;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int j = j0 + 16 * (wave + 4 * ct) + 4 * s + lk;
                const double fa = (brow < B && j < n) ? F[(size_t)brow * ldf + j] : 0.0;
#pragma unroll
                for (int bt = 0; bt < RT; ++bt) g[bt] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa, acc[ct][bt][s], g[bt], 0, 0, 0);
            }
#pragma unroll
        for (int bt = 0; bt < RT; ++bt)
#pragma unroll
            for (int r = 0; r < 4; ++r) RED[(wave * 16 + lk + 4 * r) * BP + 16 * bt + lr] = g[bt][r];
        __syncthreads();
        for (int e = tid; e < 16 * BP; e += 256) {
            const double v = ((RED[e] + RED[16 * BP + e]) + RED[2 * 16 * BP + e]) + RED[3 * 16 * BP + e];
            out[(size_t)(16 * rt) * BP + e] = v;
        }
        __syncthreads();
    }
}

// sums[g][e] = sum of partial[item][e] over the items g * per .. (g + 1) * per - 1, in ascending order
__global__ __launch_bounds__(256) void basin_cov_group_kernel(int items, int per, int bp2, const double* __restrict__ partial, double* __restrict__ sums) {
    const int g = blockIdx.x, e = blockIdx.y * 256 + threadIdx.x;
    if (e >= bp2) return;
    const int i0 = g * per, i1 = min(i0 + per, items);
    double acc = 0.0;
#pragma unroll 8
    for (int i = i0; i < i1; ++i) acc += partial[(size_t)i * bp2 + e];
    sums[(size_t)g * bp2 + e] = acc;
}

// C[b][b'] = G[b][b'] + G[b'][b] with G^T = sum over the groups (ascending) of sums[g]: both entries of a pair from the same two sums
__global__ __launch_bounds__(256) void basin_cov_final_kernel(int B, int bp, int groups, const double* __restrict__ sums, double* __restrict__ C) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= B * B) return;
    const int b = e / B, c = e % B;
    const int lo = min(b, c), hi = max(b, c);
    double x = 0.0, y = 0.0;
#pragma unroll 8
    for (int g = 0; g < groups; ++g) {
        x += sums[(size_t)g * bp * bp + lo * bp + hi];
        y += sums[(size_t)g * bp * bp + hi * bp + lo];
    }
    C[e] = x + y;
}

// items of a launch with pieces of q column blocks' height
static long long cov_item_count(int n, int q) {
    const int nblocks = (n + kCovTC - 1) / kCovTC;
    long long items = 0;
    for (int J = 0; J < nblocks; ++J) {
        const int height = std::min((J + 1) * kCovTC, n);
        items += (height + q * kCovTC - 1) / (q * kCovTC);
    }
    return items;
}

}  // namespace shg

using namespace shg;

extern "C" int shg_basin_covariance(int B, int n, const double* F, int ldf, const double* S, int lds, double* C, void* stream_) {
    SHG_REQUIRE(B >= 1 && B <= 64, "shg_basin_covariance: %d functionals, 1 to 64 are supported", B);
    SHG_REQUIRE(n >= 1, "shg_basin_covariance: n = %d, at least 1 expected", n);
    SHG_REQUIRE(F != nullptr && S != nullptr && C != nullptr, "shg_basin_covariance: NULL pointer");
    SHG_REQUIRE(ldf >= n && lds >= n, "shg_basin_covariance: leading dimensions ldf = %d, lds = %d must be at least n = %d", ldf, lds, n);
    const hipStream_t stream = (hipStream_t)stream_;
    // the longest pieces (fewest items, fewest partials) that still give the launch kCovItems items
    int q = 16;
    while (q > 1 && cov_item_count(n, q) < kCovItems) q /= 2;
    const long long items = cov_item_count(n, q);
    SHG_REQUIRE(items <= 0x7fffffff, "shg_basin_covariance: n = %d is too large", n);
    const int RT = (B + 15) / 16, bp = 16 * RT, bp2 = bp * bp;
    const int per = std::max(1, (int)std::ceil(std::sqrt((double)items)));
    const int groups = (int)((items + per - 1) / per);
    Workspace ws = Workspace::pooled(stream);
    double *partial, *sums;
    if (!ws.alloc(partial, (size_t)items * bp2, sums, (size_t)groups * bp2)) return fail(SHG_ERR_NOMEM, "shg_basin_covariance: workspace allocation failed");
    const bool vec = lds % 2 == 0 && ((uintptr_t)S & 15) == 0;
#define SHG_COV_LAUNCH(RT_)                                                                                                                        \
    do {                                                                                                                                           \
        if (vec) hipLaunchKernelGGL((basin_cov_kernel<RT_, true>), dim3((unsigned)items), dim3(256), 0, stream, B, n, q, F, ldf, S, (long long)lds, partial); \
        else hipLaunchKernelGGL((basin_cov_kernel<RT_, false>), dim3((unsigned)items), dim3(256), 0, stream, B, n, q, F, ldf, S, (long long)lds, partial); \
    } while (0)
    if (RT == 1) SHG_COV_LAUNCH(1); else if (RT == 2) SHG_COV_LAUNCH(2); else if (RT == 3) SHG_COV_LAUNCH(3); else SHG_COV_LAUNCH(4);
#undef SHG_COV_LAUNCH
    hipLaunchKernelGGL(basin_cov_group_kernel, dim3(groups, bp2 / 256), dim3(256), 0, stream, (int)items, per, bp2, (const double*)partial, sums);
    hipLaunchKernelGGL(basin_cov_final_kernel, dim3(ceil_div(B * B, 256)), dim3(256), 0, stream, B, bp, groups, (const double*)sums, C);
    SHG_HIP(hipGetLastError());
    return SHG_OK;
}

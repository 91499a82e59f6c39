// Decorrelation of coloured observation noise with long filters (shg_whiten_rows_long): the definition of shg_whiten_rows,
//
//   y[t] = sum_{k = 0 .. n} h[n][k] x[t - k],   n = min(stage[t], q, t),
//
// for orders up to 4095, where the arcs of a series get their full covariance matrices.  Per channel this
// is the product Y_c = X_c B_c with the banded upper triangular B_c[t'][t] = h_c[n_t][t - t'] for 0 <= t - t' <= n_t and +0.0
// elsewhere, formed tile by tile on the fp64 MFMA (v_mfma_f64_16x16x4_f64).  B is never stored: its tiles are generated from the tap
// table while they are staged.
// Workgroup = (128 rows of one channel: rows c, c + channels, ..., 128 output columns), 4 waves as 2 x 2, wave tile 64 x 64
// (16 accumulators), BK = 16: the tile and the K loop of mfma_tile.h.  The K range of a column tile is its band alone: from the
// smallest t - n_t of its columns to its last column, so the start-up tiles of an arc take fewer steps and a stationary tile
// q + 128 columns of X.
// The tile of X is read along its rows (16 consecutive doubles of 4 rows per wave load) and staged row-major [128][18]: a fragment
// read is "row (lane & 15), k (lane >> 4)", and the row stride of 18 doubles puts the 32 lanes of a ds_read_b64 group on distinct
// banks.  The tile of B is staged k-major [16][144] as in leverage.hip; thread c of a k-row gathers h[n_t][t - t'] of its own column
// t, which is a run of consecutive addresses across the lanes wherever the columns share a tap row (every stationary tile: the row
// h[q] then serves the whole tile from cache) and a gather from the table in the start-up columns of an arc.
// No atomics, one workgroup per output tile, K ascending from the first column of the band in steps of 4: repeated calls are bitwise
// equal.  Zeros of B multiply values of X outside x[t - n .. t], so the columns 0 .. M - 1 of X must be finite; loads are clamped
// to the rows and to the columns 0 .. M - 1 of X and to the tap row of the column, whatever stage holds.
#include "mfma_tile.h"

#include <climits>

#include "whiten_host.h"          // the contract of the call and kWhitenLongMaxOrder

namespace shg {
namespace {

constexpr int WT = 128;        // rows and output columns per workgroup
constexpr int WK = 16;         // K tile
constexpr int WLDA = 18;       // row of the staged tile of X: 16 + 2 doubles of padding (16 rows x 2 k of a fragment read fall on distinct banks)
constexpr int WLDB = 144;      // k-row of the staged tile of B: 128 + 16 doubles of padding
constexpr int WIMG = WT * WLDA + WK * WLDB;      // doubles of one buffer: X tile | B tile

__global__ __launch_bounds__(256, 2) void whiten_long_kernel(long long rpc, int channels, int M, const double* __restrict__ X, long long ldx,
                                                              const int32_t* __restrict__ stage, const double* __restrict__ taps, int q, int skip,
                                                              double* __restrict__ Y, long long ldy, long long item_base) {
    extern __shared__ double lds[];                    // [buffer][X tile [128][18] | B tile [16][144]]: 73.7 KB, two workgroups per CU
    __shared__ int lo_s[4];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int fr = lane & 15, fk = lane >> 4;

    const long long item = item_base + blockIdx.y;                    // row tile-major, then channel
    const int ch = (int)(item % channels);
    const long long r0 = item / channels * WT;                        // first row of the tile among the rows of the channel
    const int t0 = skip + (int)blockIdx.x * WT;                       // first output column: t0 < M
    const int width = min(WT, M - t0);

    // ---- the column of B a thread generates: its lag count n, -1 past M (such a column is all zeros and is not stored)
    const int c = tid & 127;
    const int kh = __builtin_amdgcn_readfirstlane(tid >> 7);          // ... in the k-rows kh, kh + 2, ..., kh + 14 (wave-uniform)
    const bool live = c < width;
    const int tc = t0 + min(c, width - 1);
    const int n = live ? min(min(max(stage[tc], 0), q), tc) : -1;
    const double* hrow = taps + ((size_t)ch * (q + 1) + (size_t)max(n, 0)) * (size_t)(q + 1);

    // first column of the band, relative to t0 (<= 0): the smallest t - n_t of the tile
    int lo = live ? c - n : INT_MAX;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) lo = min(lo, __shfl_xor(lo, m));
    if (lane == 0) lo_s[wave] = lo;
    __syncthreads();
    const int kbeg = __builtin_amdgcn_readfirstlane(min(min(lo_s[0], lo_s[1]), min(lo_s[2], lo_s[3])));      // -t0 <= kbeg <= 0
    const int nt = (width - kbeg + WK - 1) / WK;

    // ---- the rows of X a thread fetches: column ka of the K tile in the rows ra, ra + 16, ..., ra + 112, clamped to the channel's rows
    const int ka = tid & 15, ra = tid >> 4;
    const double* xrow[8];
#pragma unroll
    for (int h = 0; h < 8; ++h) xrow[h] = X + ((long long)ch + (long long)channels * min(r0 + ra + 16 * h, rpc - 1)) * ldx + t0;
    const int klast = M - 1 - t0;                                     // last column of X, relative to t0

    double xreg[8], breg[8];
    auto fetch = [&](int i) {
        const int k0 = kbeg + i * WK;                                 // first column of the K tile, relative to t0
        const int kx = min(k0 + ka, klast);                           // what lies past M - 1 meets zeros of B only
#pragma unroll
        for (int h = 0; h < 8; ++h) xreg[h] = xrow[h][kx];
#pragma unroll
        for (int h = 0; h < 8; ++h) {
            const int d = c - (k0 + kh + 2 * h);                      // the lag of this entry of B
            breg[h] = hrow[min(max(d, 0), max(n, 0))];                // inside the tap row whatever d
        }
    };
    double* a_stage = lds + ra * WLDA + ka;
    double* b_stage = lds + WT * WLDA + kh * WLDB + c;
    auto stage_tiles = [&](int buf, int i) {
        const int k0 = kbeg + i * WK;
        double* As = a_stage + buf * WIMG;
        double* Bs = b_stage + buf * WIMG;
#pragma unroll
        for (int h = 0; h < 8; ++h) {
            const int d = c - (k0 + kh + 2 * h);
            As[16 * h * WLDA] = xreg[h];
            Bs[2 * h * WLDB] = (d >= 0 && d <= n) ? breg[h] : 0.0;
        }
    };

    double4_t acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = (double4_t){0.0, 0.0, 0.0, 0.0};

    // every fragment is one ds_read_b64 "lane base + immediate" (lds_double_t of mfma_tile.h)
    const lds_double_t* a_frag = (const lds_double_t*)(lds + (wr * 64 + fr) * WLDA + fk);
    const lds_double_t* b_frag = (const lds_double_t*)(lds + WT * WLDA + fk * WLDB + wc * 64 + fr);
    asm volatile("" : "+v"(a_frag));
    asm volatile("" : "+v"(b_frag));
    auto multiply = [&](int buf) {
        const volatile lds_double_t* Ab = a_frag + buf * WIMG;
        const volatile lds_double_t* Bb = b_frag + buf * WIMG;
        tile_multiply<4, 4, 16 * WLDA, 4 * WLDB, 16>(Ab, Bb, acc);
    };
    SHG_TILE_PIPELINE(nt, fetch, stage_tiles, multiply);

    // ---- epilogue.  C/D layout: column = lane & 15, row = (lane >> 4) + 4 * reg: a store writes 16 consecutive doubles of 4 rows
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long row = r0 + wr * 64 + a * 16 + fk + 4 * r;
            if (row >= rpc) continue;
            double* y = Y + ((long long)ch + (long long)channels * row) * ldy + (t0 - skip);
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int col = wc * 64 + b * 16 + fr;
                if (col < width) y[col] = acc[a][b][r];
            }
        }
}

}  // namespace
}  // namespace shg

using namespace shg;

extern "C" int shg_whiten_rows_long(long long rows, int channels, int M, const double* X, long long ldx, const int32_t* stage, const double* taps,
                                    int q, int skip, double* Y, long long ldy, void* stream_) {
    char message[256];
    const int status = whiten_check(kWhitenRowsLong, rows, 1, channels, M, X, ldx, stage, taps, q, skip, Y, ldy, message, sizeof(message));
    if (status < 0) return shg::fail(SHG_ERR_INVALID, "%s", message);
    if (status > 0) return SHG_OK;
    const size_t lds_bytes = (size_t)2 * WIMG * sizeof(double);
    SHG_SET_LDS_ONCE(whiten_long_kernel, lds_bytes);
    const long long rpc = rows / channels;
    const long long items = ceil_div64(rpc, WT) * channels;           // (row tile, channel) pairs
    const unsigned coltiles = (unsigned)ceil_div64((long long)M - skip, WT);
    const long long kChunk = 32768;                                   // items of one launch
    for (long long first = 0; first < items; first += kChunk) {
        const unsigned gy = (unsigned)std::min(kChunk, items - first);
        hipLaunchKernelGGL(whiten_long_kernel, dim3(coltiles, gy), dim3(256), lds_bytes, (hipStream_t)stream_, rpc, channels, M, X, ldx, stage, taps, q,
                           skip, Y, ldy, first);
        SHG_HIP(hipGetLastError());
    }
    return SHG_OK;
}

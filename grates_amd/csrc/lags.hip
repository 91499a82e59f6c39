// Lagged products of the rows of a matrix, cut at arc boundaries: of every row with itself (shg_segment_lag_products: the square sums
// per arc, lag 0, and the empirical autocovariance, lags 0 .. q, of post-fit residuals) and of K rows with each
// other (shg_segment_cross_lag_products: the empirical cross-covariance function of the K components, section 4.29).
//
//   S[r][s][k]     = sum over t with seg[s] <= t and t + k < seg[s+1] of X[r][t] X[r][t + k],    k = 0 .. lags
//   S[s][k][c][c'] = sum over t with seg[s] <= t and t + k < seg[s+1] of X[c][t] X[c'][t + k],   k = 0 .. lags
//
// Summation order of an entry, relative to the start of its segment, the same in all three kernels: lane i of 64 runs the chain acc = 0,
// acc = fma(x[t], x'[t + k], acc) over t = start + i, start + i + 64, ... ascending while t + k < end; the 64 chains are added by the
// butterfly acc += acc of lane ^ 32, ^ 16, ^ 8, ^ 4, ^ 2, ^ 1; lane 0 stores.  Nothing in it depends on the row, lags, the other
// segments, the position of the segment in the row or the launch.  The chain of a tile and the choice of its specialisation are written
// once, lag_tile and lag_tile_any, so S[s][k][c][c] of the cross call is bitwise shg_segment_lag_products of row c.
//
// lags = 0 (many rows, bound by memory): segment_squares_kernel, the mapping of arcs.hip: a wave takes one segment of 4 consecutive rows,
// lane <-> column, one coalesced read of X.
// lags > 0 (few rows, every value meets lags + 1 partners): segment_lags_kernel: a workgroup of 4 waves takes one segment of one row in
// tiles of 1024 columns, staged in LDS with the `lags` columns behind them (one read of X from global memory); wave w holds the lags
// w G .. w G + G - 1 in G accumulators per lane, G = lag_group(lags) <= 33, so no lane spills at any lags.  x[t] stays in a register and
// the reads of x[t + k] by consecutive lanes are consecutive doubles of LDS: no bank conflicts, and the chain order costs nothing.
// K <= 6 rows against each other (every value meets K (lags + 1) partners): segment_cross_lags_kernel: the same workgroup takes one
// segment of one pair (c, c'), the first factors of row c and the partners of row c' staged side by side, the same waves and G.
#include "common.h"

#include "lags_device.h"          // segment_range, shared with lags_long.hip
#include "lags_host.h"

namespace shg {

__global__ __launch_bounds__(kLagWaves * 64) void segment_squares_kernel(long long items, long long rows, int M, const double* __restrict__ X,
                                                                         long long ldx, int nseg, const int32_t* __restrict__ seg,
                                                                         double* __restrict__ S) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * kLagWaves;
    for (long long item = (long long)blockIdx.x * kLagWaves + (threadIdx.x >> 6); item < items; item += waves) {    // uniform in a wave
        const long long group = item / nseg;
        const int s = (int)(item - group * nseg);
        const long long r0 = group * kLagRows;
        int start, end;
        segment_range(seg, s, M, lane, start, end);
        const double* x[kLagRows];
#pragma unroll
        for (int i = 0; i < kLagRows; ++i) x[i] = X + min(r0 + i, rows - 1) * ldx;       // a row past the end repeats the last one and is not stored
        double acc[kLagRows];
#pragma unroll
        for (int i = 0; i < kLagRows; ++i) acc[i] = 0.0;
#pragma unroll 4
        for (long long t = (long long)start + lane; t < end; t += 64) {                   // 64 bits: t + 64 may pass 2^31
#pragma unroll
            for (int i = 0; i < kLagRows; ++i) {
                const double xv = x[i][t];
                acc[i] = fma(xv, xv, acc[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < kLagRows; ++i)
#pragma unroll
            for (int mask = 32; mask >= 1; mask >>= 1) acc[i] += __shfl_xor(acc[i], mask);
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < kLagRows; ++i)
                if (r0 + i < rows) S[(r0 + i) * nseg + s] = acc[i];
        }
    }
}

// one tile of a wave: lane i takes the columns i, i + 64, ... of the tile (first factors xa) against their partners k0 + k behind them
// (xb; the same array in segment_lags_kernel).  kEvery: the wave holds all G lags; kInside: no partner of the tile lies past the end of
// the segment (else i + k < staged is t + k < end)
template <int G, bool kEvery, bool kInside>
__device__ inline void lag_tile(const double* xa, const double* xb, int lane, int width, int staged, int k0, int count, double (&acc)[G]) {
    for (int i = lane; i < width; i += 64) {
        const double xv = xa[i];
#pragma unroll
        for (int k = 0; k < G; ++k)
            if ((kEvery || k < count) && (kInside || i + k0 + k < staged)) acc[k] = fma(xv, xb[i + k0 + k], acc[k]);
    }
}

// the tile of a wave that holds lags (count > 0), by the specialisation that its lags and the end of the segment allow
template <int G>
__device__ inline void lag_tile_any(const double* xa, const double* xb, int lane, int width, int staged, int lags, int k0, int count, double (&acc)[G]) {
    const bool inside = staged == width + lags;                  // every partner of the tile is inside the segment
    if (count == G && inside) lag_tile<G, true, true>(xa, xb, lane, width, staged, k0, count, acc);
    else if (count == G) lag_tile<G, true, false>(xa, xb, lane, width, staged, k0, count, acc);
    else if (inside) lag_tile<G, false, true>(xa, xb, lane, width, staged, k0, count, acc);
    else lag_tile<G, false, false>(xa, xb, lane, width, staged, k0, count, acc);
}

template <int G>
__global__ __launch_bounds__(kLagWaves * 64) void segment_lags_kernel(long long items, int M, const double* __restrict__ X, long long ldx, int lags,
                                                                      int nseg, const int32_t* __restrict__ seg, double* __restrict__ S) {
    __shared__ double xs[kLagTile + kLagWaves * kLagMaxGroup];      // columns first .. first + kLagTile + lags of the segment; no index i + k0 + k lies outside
    const int tid = threadIdx.x, lane = tid & 63;
    const int k0 = (tid >> 6) * G;                                   // the first lag of this wave
    const int count = min(G, lags + 1 - k0);                         // it holds the lags k0 .. k0 + count - 1 (none: it only helps to stage)
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const long long row = item / nseg;
        const int s = (int)(item - row * nseg);
        int start, end;
        segment_range(seg, s, M, lane, start, end);
        const double* x = X + row * ldx + start;
        const int length = end - start;
        double acc[G];
#pragma unroll
        for (int k = 0; k < G; ++k) acc[k] = 0.0;
        for (int first = 0; first < length; first += min(kLagTile, length - first)) {
            const int width = min(kLagTile, length - first);        // columns of the tile
            const int staged = min(width + lags, length - first);   // and those behind them that are still in the segment
            __syncthreads();                                         // the previous tile's reads of xs are done
            for (int i = tid; i < staged; i += kLagWaves * 64) xs[i] = x[first + i];
            __syncthreads();
            if (count > 0) lag_tile_any<G>(xs, xs, lane, width, staged, lags, k0, count, acc);
        }
        if (count > 0) {
#pragma unroll
            for (int k = 0; k < G; ++k)
#pragma unroll
                for (int mask = 32; mask >= 1; mask >>= 1) acc[k] += __shfl_xor(acc[k], mask);
            if (lane == 0) {
                double* out = S + (row * nseg + s) * (lags + 1) + k0;
#pragma unroll
                for (int k = 0; k < G; ++k)
                    if (k < count) out[k] = acc[k];
            }
        }
    }
}

template <int G>
static void launch_segment_lags(const LagGeometry& g, int M, const double* X, long long ldx, int lags, int nseg, const int32_t* seg, double* S,
                                hipStream_t stream) {
    hipLaunchKernelGGL((segment_lags_kernel<G>), dim3(g.blocks), dim3(kLagWaves * 64), 0, stream, g.items, M, X, ldx, lags, nseg, seg, S);
}

constexpr int kCrossMaxDim = 6;

template <int G>
__global__ __launch_bounds__(kLagWaves * 64) void segment_cross_lags_kernel(int items, int K, int M, const double* __restrict__ X, long long ldx, int lags,
                                                                            const int32_t* __restrict__ seg, double* __restrict__ S) {
    __shared__ double xa[kLagTile];                                  // columns first .. first + kLagTile of row c of the segment
    __shared__ double xb[kLagTile + kLagWaves * kLagMaxGroup];      // and first .. first + kLagTile + lags of row c'; no index i + k0 + k lies outside
    const int tid = threadIdx.x, lane = tid & 63;
    const int k0 = (tid >> 6) * G;                                   // the first lag of this wave
    const int count = min(G, lags + 1 - k0);                         // it holds the lags k0 .. k0 + count - 1 (none: it only helps to stage)
    for (int item = blockIdx.x; item < items; item += gridDim.x) {
        const int s = item / (K * K);
        const int c = (item - s * K * K) / K, cc = item - (s * K + c) * K;
        int start, end;
        segment_range(seg, s, M, lane, start, end);
        const double* a = X + c * ldx + start;
        const double* b = X + cc * ldx + start;
        const int length = end - start;
        double acc[G];
#pragma unroll
        for (int k = 0; k < G; ++k) acc[k] = 0.0;
        for (int first = 0; first < length; first += min(kLagTile, length - first)) {
            const int width = min(kLagTile, length - first);        // columns of the tile
            const int staged = min(width + lags, length - first);   // and those behind them that are still in the segment
            __syncthreads();                                         // the previous tile's reads of xa / xb are done
            for (int i = tid; i < staged; i += kLagWaves * 64) {
                if (i < width) xa[i] = a[first + i];
                xb[i] = b[first + i];
            }
            __syncthreads();
            if (count > 0) lag_tile_any<G>(xa, xb, lane, width, staged, lags, k0, count, acc);
        }
        if (count > 0) {
#pragma unroll
            for (int k = 0; k < G; ++k)
#pragma unroll
                for (int mask = 32; mask >= 1; mask >>= 1) acc[k] += __shfl_xor(acc[k], mask);
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < G; ++k)
                    if (k < count) S[(((size_t)s * (lags + 1) + k0 + k) * K + c) * K + cc] = acc[k];
            }
        }
    }
}

template <int G>
static void launch_segment_cross_lags(unsigned blocks, int items, int K, int M, const double* X, long long ldx, int lags, const int32_t* seg, double* S,
                                      hipStream_t stream) {
    hipLaunchKernelGGL((segment_cross_lags_kernel<G>), dim3(blocks), dim3(kLagWaves * 64), 0, stream, items, K, M, X, ldx, lags, seg, S);
}

}  // namespace shg

using namespace shg;

extern "C" int shg_segment_lag_products(long long rows, int M, const double* X, long long ldx, int lags, int nseg, const int32_t* seg, double* S,
                                        void* stream_) {
    char message[256];
    const int status = segment_lag_products_check(rows, M, X, ldx, lags, nseg, seg, S, message, sizeof(message));
    if (status < 0) return shg::fail(SHG_ERR_INVALID, "%s", message);
    if (status > 0) return SHG_OK;
    const LagGeometry g = segment_lag_products_geometry(rows, nseg, lags);
    hipStream_t stream = (hipStream_t)stream_;
    switch (g.group) {
        case 0:
            hipLaunchKernelGGL(segment_squares_kernel, dim3(g.blocks), dim3(kLagWaves * 64), 0, stream, g.items, rows, M, X, ldx, nseg, seg, S);
            break;
        case 1: launch_segment_lags<1>(g, M, X, ldx, lags, nseg, seg, S, stream); break;
        case 2: launch_segment_lags<2>(g, M, X, ldx, lags, nseg, seg, S, stream); break;
        case 4: launch_segment_lags<4>(g, M, X, ldx, lags, nseg, seg, S, stream); break;
        case 8: launch_segment_lags<8>(g, M, X, ldx, lags, nseg, seg, S, stream); break;
        case 16: launch_segment_lags<16>(g, M, X, ldx, lags, nseg, seg, S, stream); break;
        default: launch_segment_lags<kLagMaxGroup>(g, M, X, ldx, lags, nseg, seg, S, stream); break;
    }
    SHG_HIP(hipGetLastError());
    return SHG_OK;
}

extern "C" int shg_segment_cross_lag_products(int K, int M, const double* X, long long ldx, int lags, int nseg, const int32_t* seg, double* S,
                                              void* stream_) {
    const char* fn = "shg_segment_cross_lag_products";
    SHG_REQUIRE(M >= 0 && ldx >= 0, "%s: negative size (M %d, ldx %lld)", fn, M, ldx);
    SHG_REQUIRE(K >= 1 && K <= kCrossMaxDim, "%s: dimension K %d outside 1 .. %d", fn, K, kCrossMaxDim);
    SHG_REQUIRE(lags >= 0 && lags <= kLagMax, "%s: lags %d outside 0 .. %d", fn, lags, kLagMax);
    SHG_REQUIRE(nseg >= 0, "%s: nseg %d is negative", fn, nseg);
    SHG_REQUIRE(ldx >= M, "%s: ldx %lld below M %d", fn, ldx, M);
    const long long limit = 1LL << 40;
    SHG_REQUIRE(ldx == 0 || K <= limit / ldx, "%s: %d rows of %lld values of X are too large", fn, K, ldx);
    SHG_REQUIRE(nseg <= (1 << 24), "%s: %d segments of %d x %d x %d values of S are too large", fn, nseg, lags + 1, K, K);
    if (nseg == 0) return SHG_OK;
    SHG_REQUIRE(X && seg && S, "%s: NULL pointer", fn);
    const int items = nseg * K * K;                                 // at most 2^24 x 36
    const unsigned blocks = (unsigned)std::min(items, kLagBlocks);
    hipStream_t stream = (hipStream_t)stream_;
    switch (lag_group(lags)) {
        case 1: launch_segment_cross_lags<1>(blocks, items, K, M, X, ldx, lags, seg, S, stream); break;
        case 2: launch_segment_cross_lags<2>(blocks, items, K, M, X, ldx, lags, seg, S, stream); break;
        case 4: launch_segment_cross_lags<4>(blocks, items, K, M, X, ldx, lags, seg, S, stream); break;
        case 8: launch_segment_cross_lags<8>(blocks, items, K, M, X, ldx, lags, seg, S, stream); break;
        case 16: launch_segment_cross_lags<16>(blocks, items, K, M, X, ldx, lags, seg, S, stream); break;
        default: launch_segment_cross_lags<kLagMaxGroup>(blocks, items, K, M, X, ldx, lags, seg, S, stream); break;
    }
    SHG_HIP(hipGetLastError());
    return SHG_OK;
}

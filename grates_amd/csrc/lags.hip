// Lagged products of the rows of a matrix with themselves, cut at arc boundaries (shg_segment_lag_products): the square sums per arc
// (lag 0) and the empirical autocovariance (lags 0 .. q) of post-fit residuals.
//
//   S[r][s][k] = sum over t with seg[s] <= t and t + k < seg[s+1] of X[r][t] X[r][t + k],   k = 0 .. lags
//
// Summation order of an entry, relative to the start of its segment, the same in both kernels: lane i of 64 runs the chain acc = 0,
// acc = fma(x[t], x[t + k], acc) over t = start + i, start + i + 64, ... ascending while t + k < end; the 64 chains are added by the
// butterfly acc += acc of lane ^ 32, ^ 16, ^ 8, ^ 4, ^ 2, ^ 1; lane 0 stores.  Nothing in it depends on the row, lags, the other
// segments, the position of the segment in the row or the launch.
//
// lags = 0 (many rows, bound by memory): segment_squares_kernel, the mapping of arcs.hip: a wave takes one segment of 4 consecutive rows,
// lane <-> column, one coalesced read of X.
// lags > 0 (few rows, every value meets lags + 1 partners): segment_lags_kernel: a workgroup of 4 waves takes one segment of one row in
// tiles of 1024 columns, staged in LDS with the `lags` columns behind them (one read of X from global memory); wave w holds the lags
// w G .. w G + G - 1 in G accumulators per lane, G = lag_group(lags) <= 33, so no lane spills at any lags.  x[t] stays in a register and
// the reads of x[t + k] by consecutive lanes are consecutive doubles of LDS: no bank conflicts, and the chain order costs nothing.
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

// one tile of a wave: lane i takes the columns i, i + 64, ... of the tile against their partners k0 + k behind them.  kEvery: the wave
// holds all G lags; kInside: no partner of the tile lies past the end of the segment (else i + k < staged is t + k < end)
template <int G, bool kEvery, bool kInside>
__device__ inline void lag_tile(const double* xs, int lane, int width, int staged, int k0, int count, double (&acc)[G]) {
    for (int i = lane; i < width; i += 64) {
        const double xv = xs[i];
#pragma unroll
        for (int k = 0; k < G; ++k)
            if ((kEvery || k < count) && (kInside || i + k0 + k < staged)) acc[k] = fma(xv, xs[i + k0 + k], acc[k]);
    }
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
            if (count > 0) {
                const bool inside = staged == width + lags;          // every partner of the tile is inside the segment
                if (count == G && inside) lag_tile<G, true, true>(xs, lane, width, staged, k0, count, acc);
                else if (count == G) lag_tile<G, true, false>(xs, lane, width, staged, k0, count, acc);
                else if (inside) lag_tile<G, false, true>(xs, lane, width, staged, k0, count, acc);
                else lag_tile<G, false, false>(xs, lane, width, staged, k0, count, acc);
            }
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

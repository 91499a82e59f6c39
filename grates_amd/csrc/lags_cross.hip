// Lagged products between the rows of a matrix, cut at arc boundaries (shg_segment_cross_lag_products): the empirical cross-covariance
// function of the K components of post-fit residuals.
//
//   S[s][k][c][c'] = sum over t with seg[s] <= t and t + k < seg[s+1] of X[c][t] X[c'][t + k],   k = 0 .. lags
//
// The summation order of an entry is that of shg_segment_lag_products (lags.hip), relative to the start of its segment: lane i of 64
// runs the chain acc = 0, acc = fma(x_c[t], x_c'[t + k], acc) over t = start + i, start + i + 64, ... ascending while t + k < end; the 64
// chains are added by the butterfly acc += acc of lane ^ 32, ^ 16, ^ 8, ^ 4, ^ 2, ^ 1; lane 0 stores.  So S[s][k][c][c] is bitwise
// shg_segment_lag_products of row c.
//
// K <= 6 rows, every value meets K (lags + 1) partners: a workgroup of 4 waves takes one segment of one pair (c, c') in tiles of 1024
// columns, the first factors of row c and the partners of row c' with the `lags` columns behind them staged in LDS; wave w holds the lags
// w G .. w G + G - 1 in G accumulators per lane, G = lag_group(lags) as in lags.hip.
#include "common.h"

#include "lags_device.h"          // segment_range, shared with lags.hip and lags_long.hip
#include "lags_host.h"            // the tile, the waves and lag_group of lags.hip

namespace shg {

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
            for (int i = lane; i < width; i += 64) {
                const double xv = xa[i];
#pragma unroll
                for (int k = 0; k < G; ++k)
                    if (k < count && i + k0 + k < staged) acc[k] = fma(xv, xb[i + k0 + k], acc[k]);
            }
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

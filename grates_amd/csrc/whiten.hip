// Decorrelation of coloured observation noise (shg_whiten_rows): the banded lower-triangular W with W^T W = Sigma^-1 of a sequence
// of scalar AR models, applied along the point axis of the rows of a matrix.
//
//   y[t] = sum_{k = 0 .. n} h[n][k] x[t - k],   n = min(stage[t], q, t)
//
// Memory-bound: one read and one write of the matrix, n + 1 FMAs per value.  A workgroup takes a tile of kTile consecutive output
// columns of one row, stages them with the q columns in front of them in LDS (coalesced loads, every value of X is read from global
// memory once per tile), keeps the tap row of the stationary model of the row's channel beside them, and reads the rare start-up tap
// rows (the first q points of an arc) from global memory.  Every output is the same chain of FMAs whatever the tile, the row or the
// call it is computed in.
#include "common.h"

#include "whiten_host.h"          // the contract of the call and kWhitenMaxOrder

namespace shg {

constexpr int kWhitenThreads = 256;
constexpr int kWhitenPerThread = 4;
constexpr int kWhitenTile = kWhitenThreads * kWhitenPerThread;      // output columns of a work item
constexpr int kWhitenBlocks = 256 * 8;                               // 8 workgroups of 4 waves fill a CU: the rest is a grid stride

__global__ __launch_bounds__(kWhitenThreads) void whiten_rows_kernel(long long items, int tiles, int channels, int M, const double* __restrict__ X,
                                                                     long long ldx, const int32_t* __restrict__ stage,
                                                                     const double* __restrict__ taps, int q, int skip, double* __restrict__ Y,
                                                                     long long ldy) {
    __shared__ double xs[kWhitenTile + kWhitenMaxOrder];            // columns t0 - q .. t0 + kWhitenTile of the row
    __shared__ double hs[kWhitenMaxOrder + 1];                      // h[q][0 .. q] of the row's channel
    const int tid = threadIdx.x;
    const int q1 = q + 1;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const long long row = item / tiles;
        const int t0 = skip + (int)(item - row * tiles) * kWhitenTile;                  // first output column of the tile: t0 < M
        const int width = min(kWhitenTile, M - t0);
        const double* x = X + row * ldx;
        const double* h = taps + (size_t)(row % channels) * q1 * q1;
        __syncthreads();                                                                 // the previous item's reads of xs / hs are done
        for (int i = tid; i < width + q; i += kWhitenThreads) {
            const int c = t0 - q + i;                                                    // c < M; never before column 0 of the row
            xs[i] = c >= 0 ? x[c] : 0.0;
        }
        if (tid < q1) hs[tid] = h[(size_t)q * q1 + tid];
        __syncthreads();
        double* y = Y + row * ldy;
#pragma unroll
        for (int j = 0; j < kWhitenPerThread; ++j) {
            const int i = tid + j * kWhitenThreads;
            if (i >= width) break;
            const int t = t0 + i;
            const int n = min(min(max(stage[t], 0), q), t);                              // lags: inside the table and inside the row
            const double* xt = xs + q + i;                                               // xt[-k] = x[t - k]
            double acc;
            if (n == q) {
                acc = hs[0] * xt[0];
                for (int k = 1; k <= q; ++k) acc = fma(hs[k], xt[-k], acc);
            } else {
                const double* hn = h + (size_t)n * q1;
                acc = hn[0] * xt[0];
                for (int k = 1; k <= n; ++k) acc = fma(hn[k], xt[-k], acc);
            }
            y[t - skip] = acc;
        }
    }
}

}  // namespace shg

using namespace shg;

extern "C" int shg_whiten_rows(long long rows, int channels, int M, const double* X, long long ldx, const int32_t* stage, const double* taps, int q,
                               int skip, double* Y, long long ldy, void* stream_) {
    char message[256];
    const int status = whiten_check(kWhitenRows, rows, 1, channels, M, X, ldx, stage, taps, q, skip, Y, ldy, message, sizeof(message));
    if (status < 0) return shg::fail(SHG_ERR_INVALID, "%s", message);
    if (status > 0) return SHG_OK;
    const int tiles = (int)ceil_div64((long long)M - skip, kWhitenTile);
    const long long items = rows * tiles;
    const unsigned blocks = (unsigned)std::min<long long>(items, kWhitenBlocks);
    hipLaunchKernelGGL(whiten_rows_kernel, dim3(blocks), dim3(kWhitenThreads), 0, (hipStream_t)stream_, items, tiles, channels, M, X, ldx, stage, taps, q,
                       skip, Y, ldy);
    SHG_HIP(hipGetLastError());
    return SHG_OK;
}

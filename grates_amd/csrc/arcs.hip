// Products of the rows of a matrix with a basis, cut at arc boundaries (shg_segment_products): what the elimination of arc-wise
// parameters needs of the transposed design matrix.
//
//   S[r][s][j] = sum_{t = seg[s] .. seg[s+1] - 1} X[r][t] Bt[j][r % channels][t]
//
// One pass over X.  A wave takes a work item: one segment of 4 rows of one channel (rows r, r + channels, ...; 2 rows above u = 8, where
// 4 u accumulators no longer leave registers for a second wave), so that every basis value it loads serves all of them; X is read from global memory once, coalesced (lane <-> column), the basis of a block
// comes from cache.  Summation order of an entry, relative to the start of its segment: lane i of 64 runs the chain acc = 0,
// acc = fma(x[t], b[t], acc) over the columns t = start + i, start + i + 64, ... in ascending order; the 64 chains are added by the
// butterfly acc += acc of lane ^ 32, ^ 16, ^ 8, ^ 4, ^ 2, ^ 1 (both partners form the same sum, so every lane ends with the same
// value); lane 0 stores.  Nothing in it depends on the row, the other segments, the position of the segment in the row or the launch.
#include "common.h"

#include "arcs_host.h"

namespace shg {

template <int U, int kRows = segment_rows(U)>
__global__ __launch_bounds__(kSegWaves * 64) void segment_products_kernel(long long items, long long outer, int channels, int M,
                                                                          const double* __restrict__ X, long long ldx,
                                                                          const double* __restrict__ Bt, long long ldb, int nseg,
                                                                          const int32_t* __restrict__ seg, double* __restrict__ S) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * kSegWaves;
    for (long long item = (long long)blockIdx.x * kSegWaves + (threadIdx.x >> 6); item < items; item += waves) {    // uniform in a wave
        const long long group = item / nseg;
        const int s = (int)(item - group * nseg);
        const int c = (int)(group % channels);
        const long long p0 = group / channels * kRows;                           // rows (p0 + i) channels + c, p0 + i < outer
        // the table clamped to 0 .. M and made non-decreasing: start = max of the clamped entries 0 .. s, end = max(start, entry s + 1).
        // segment_range of lags_device.h written out: with the call every kernel of this file compiles to other instructions
        int start = 0;
        for (int i = lane; i <= s; i += 64) start = max(start, min(max(seg[i], 0), M));
#pragma unroll
        for (int mask = 32; mask >= 1; mask >>= 1) start = max(start, __shfl_xor(start, mask));
        const int end = max(start, min(max(seg[s + 1], 0), M));

        const double* x[kRows];
#pragma unroll
        for (int i = 0; i < kRows; ++i) x[i] = X + (min(p0 + i, outer - 1) * channels + c) * ldx;     // a row past the end repeats the last one and is not stored
        const double* b = Bt + (long long)c * ldb;
        const long long bstep = (long long)channels * ldb;
        double acc[kRows][U];
#pragma unroll
        for (int i = 0; i < kRows; ++i)
#pragma unroll
            for (int j = 0; j < U; ++j) acc[i][j] = 0.0;
        constexpr int kUnroll = U <= 4 ? 4 : (U <= 8 ? 2 : 1);                      // loads in flight against registers
#pragma unroll kUnroll
        for (int t = start + lane; t < end; t += 64) {
            double xv[kRows];
#pragma unroll
            for (int i = 0; i < kRows; ++i) xv[i] = x[i][t];
#pragma unroll
            for (int j = 0; j < U; ++j) {
                const double bv = b[j * bstep + t];
#pragma unroll
                for (int i = 0; i < kRows; ++i) acc[i][j] = fma(xv[i], bv, acc[i][j]);
            }
        }
#pragma unroll
        for (int i = 0; i < kRows; ++i)
#pragma unroll
            for (int j = 0; j < U; ++j)
#pragma unroll
                for (int mask = 32; mask >= 1; mask >>= 1) acc[i][j] += __shfl_xor(acc[i][j], mask);
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < kRows; ++i) {
                if (p0 + i >= outer) break;
                double* out = S + (((p0 + i) * channels + c) * nseg + s) * U;
#pragma unroll
                for (int j = 0; j < U; ++j) out[j] = acc[i][j];
            }
        }
    }
}

template <int U>
static void launch_segment_products(const SegmentGeometry& g, long long rows, int channels, int M, const double* X, long long ldx, const double* Bt,
                                    long long ldb, int u, int nseg, const int32_t* seg, double* S, hipStream_t stream) {
    if constexpr (U <= kSegMaxParameters) {
        if (u == U)
            hipLaunchKernelGGL((segment_products_kernel<U>), dim3(g.blocks), dim3(kSegWaves * 64), 0, stream, g.items, rows / channels, channels, M, X, ldx,
                               Bt, ldb, nseg, seg, S);
        else
            launch_segment_products<U + 1>(g, rows, channels, M, X, ldx, Bt, ldb, u, nseg, seg, S, stream);
    }
}

}  // namespace shg

using namespace shg;

extern "C" int shg_segment_products(long long rows, int channels, int M, const double* X, long long ldx, const double* Bt, long long ldb, int u, int nseg,
                                    const int32_t* seg, double* S, void* stream_) {
    char message[256];
    const int status = segment_products_check(rows, channels, M, X, ldx, Bt, ldb, u, nseg, seg, S, message, sizeof(message));
    if (status < 0) return shg::fail(SHG_ERR_INVALID, "%s", message);
    if (status > 0) return SHG_OK;
    launch_segment_products<1>(segment_products_geometry(rows, channels, nseg, u), rows, channels, M, X, ldx, Bt, ldb, u, nseg, seg, S,
                               (hipStream_t)stream_);
    SHG_HIP(hipGetLastError());
    return SHG_OK;
}

// Decorrelation of vector noise (shg_whiten_rows_vector): the block lower-triangular banded W with W^T W = Sigma^-1 of a sequence of
// VAR models of dimension K, applied along the point axis to groups of K rows of a matrix.
//
//   y[c][t] = sum_{k = 0 .. n} sum_{c' = 0 .. K-1} H[n][k][c][c'] x[c'][t - k],   n = min(stage[t], q, t)
//
// K (n + 1) FMAs per value: bound by how operands reach the fp64 VALU, not by memory.  A workgroup takes a tile of kThreads * J
// consecutive output columns of the K rows of one group and stages them with the q columns in front in LDS.  A lane owns J consecutive
// columns of all K rows: K J accumulators.  The K x K taps of a lag of the stationary model are uniform in the wave and come through
// scalar loads; one x[c'][t - k] meets K of them, and the J values a lane needs of row c' at lag k are those of lag k - 1 moved by
// one column, so a lane keeps them in registers and reads one new value from LDS per (k, c'): one LDS read per K J FMAs.  The tile is
// stored in J planes (column i at plane i % J, slot i / J), so that read is consecutive doubles over consecutive lanes.  The rare
// start-up columns (the first q points of an arc) and the ragged end of a row take the tap rows from global memory per lane.  Every
// output is the same chain whatever path, tile, group or call it is computed in: k ascending, c' ascending inside, the first term a
// product and every later one an fma.
#include "common.h"

#include "whiten_host.h"          // the contract of the call, kVectorMaxOrder and the dimensions

namespace shg {

constexpr int kVectorThreads = 256;
constexpr int kVectorBlocks = 256 * 8;                               // workgroups of a launch at most: the rest is a grid stride

// columns of a lane: K J accumulators and K J window values stay in registers, and K times the tile with its halo leaves room for two
// workgroups and more on a CU (K = 3: 27 KB, K = 6: 30 KB)
constexpr int vector_columns(int K) { return K <= 3 ? 4 : 2; }
constexpr int vector_tile(int K) { return kVectorThreads * vector_columns(K); }

template <int K, int J>
struct VectorTile {
    static constexpr int kTile = kVectorThreads * J;
    static constexpr int kSlots = (kTile + kVectorMaxOrder) / J + 16 / J;   // slots of a plane; the 16 / J more spread the planes over the banks of a staged store
    static constexpr int kRow = J * kSlots;                                 // doubles of one component
    __device__ static inline int at(int i) { return (i % J) * kSlots + i / J; }
};

template <int K, int J>
__global__ __launch_bounds__(kVectorThreads) void whiten_vector_kernel(long long items, int tiles, int M, const double* __restrict__ X, long long ldx,
                                                                       const int32_t* __restrict__ stage, const double* __restrict__ taps, int q,
                                                                       int skip, double* __restrict__ Y, long long ldy) {
    typedef VectorTile<K, J> T;
    __shared__ double xs[K * T::kRow];                               // columns t0 - qp .. t0 + kTile of the K rows of the group
    const int tid = threadIdx.x;
    const int q1 = q + 1;
    const int qp = (q + J - 1) / J * J;                              // the halo in whole lanes' worth of columns: qp <= kVectorMaxOrder
    const double* hq = taps + (size_t)q * q1 * (K * K);              // H[q][0 .. q]
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const long long group = item / tiles;
        const int t0 = skip + (int)(item - group * tiles) * T::kTile;                   // first output column of the tile: t0 < M
        const int width = min(T::kTile, M - t0);
        const double* x = X + group * K * ldx;
        __syncthreads();                                                                 // the previous item's reads of xs are done
        for (int i = tid; i < width + qp; i += kVectorThreads) {
            const int col = t0 - qp + i;                                                 // col < M; never before column 0 of a row
            const int slot = T::at(i);
#pragma unroll
            for (int c = 0; c < K; ++c) xs[c * T::kRow + slot] = col >= 0 ? x[c * ldx + col] : 0.0;
        }
        __syncthreads();
        const int i0 = tid * J;                                                          // first of the lane's columns, counted in the tile
        if (i0 >= width) continue;                                                       // (the barriers are above: every thread reaches them)
        int n[J];
        bool stationary = i0 + J <= width;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int t = t0 + min(i0 + j, width - 1);
            n[j] = min(min(max(stage[t], 0), q), t);                                     // lags: inside the table and inside the row
            stationary = stationary && n[j] == q;
        }
        double* y = Y + group * K * ldy + (t0 - skip) + i0;
        if (stationary) {
            double acc[K][J], w[K][J];
            const int base = qp / J + tid;                                               // slot of column i0 + qp of the staged tile
#pragma unroll
            for (int c = 0; c < K; ++c)
#pragma unroll
                for (int j = 0; j < J; ++j) w[c][j] = xs[c * T::kRow + j * T::kSlots + base];
#pragma unroll
            for (int cc = 0; cc < K; ++cc)
#pragma unroll
                for (int c = 0; c < K; ++c) {
                    const double h = hq[c * K + cc];
#pragma unroll
                    for (int j = 0; j < J; ++j) acc[c][j] = cc == 0 ? h * w[cc][j] : fma(h, w[cc][j], acc[c][j]);
                }
            for (int k = 1; k <= q; ++k) {
                const double* hk = hq + (size_t)k * (K * K);
                const int back = qp - k;                                                 // column i0 - k of the tile is staged at back + i0
                const int fresh = (back % J) * T::kSlots + back / J + tid;
#pragma unroll
                for (int cc = 0; cc < K; ++cc) {
#pragma unroll
                    for (int j = J - 1; j > 0; --j) w[cc][j] = w[cc][j - 1];
                    w[cc][0] = xs[cc * T::kRow + fresh];
#pragma unroll
                    for (int c = 0; c < K; ++c) {
                        const double h = hk[c * K + cc];
#pragma unroll
                        for (int j = 0; j < J; ++j) acc[c][j] = fma(h, w[cc][j], acc[c][j]);
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < K; ++c)
#pragma unroll
                for (int j = 0; j < J; ++j) y[c * ldy + j] = acc[c][j];
        } else {
#pragma unroll
            for (int j = 0; j < J; ++j) {
                if (i0 + j >= width) break;
                const int nj = n[j];
                const double* hn = taps + (size_t)nj * q1 * (K * K);                     // H[nj][0 .. nj]
                const int i = qp + i0 + j;                                               // the column in the staged tile: i - k >= qp - q >= 0
                double acc[K];
#pragma unroll
                for (int cc = 0; cc < K; ++cc) {
                    const double xv = xs[cc * T::kRow + T::at(i)];
#pragma unroll
                    for (int c = 0; c < K; ++c) acc[c] = cc == 0 ? hn[c * K + cc] * xv : fma(hn[c * K + cc], xv, acc[c]);
                }
                for (int k = 1; k <= nj; ++k) {
                    const double* hk = hn + (size_t)k * (K * K);
                    const int slot = T::at(i - k);
#pragma unroll
                    for (int cc = 0; cc < K; ++cc) {
                        const double xv = xs[cc * T::kRow + slot];
#pragma unroll
                        for (int c = 0; c < K; ++c) acc[c] = fma(hk[c * K + cc], xv, acc[c]);
                    }
                }
#pragma unroll
                for (int c = 0; c < K; ++c) y[c * ldy + j] = acc[c];
            }
        }
    }
}

template <int K>
static void launch_whiten_vector(long long groups, int M, const double* X, long long ldx, const int32_t* stage, const double* taps, int q, int skip,
                                 double* Y, long long ldy, hipStream_t stream) {
    constexpr int J = vector_columns(K);
    const int tiles = (int)ceil_div64((long long)M - skip, vector_tile(K));
    const long long items = groups * tiles;
    const unsigned blocks = (unsigned)std::min<long long>(items, kVectorBlocks);
    hipLaunchKernelGGL((whiten_vector_kernel<K, J>), dim3(blocks), dim3(kVectorThreads), 0, stream, items, tiles, M, X, ldx, stage, taps, q, skip, Y, ldy);
}

}  // namespace shg

using namespace shg;

extern "C" int shg_whiten_vector_info(int K, int* tile_columns) {
    SHG_REQUIRE(K >= kVectorMinDim && K <= kVectorMaxDim, "shg_whiten_vector_info: dimension K %d outside %d .. %d", K, kVectorMinDim, kVectorMaxDim);
    if (tile_columns) *tile_columns = vector_tile(K);
    return SHG_OK;
}

extern "C" int shg_whiten_rows_vector(long long groups, int K, int M, const double* X, long long ldx, const int32_t* stage, const double* taps, int q,
                                      int skip, double* Y, long long ldy, void* stream_) {
    char message[256];
    const int status = whiten_check(kWhitenRowsVector, groups, K, 1, M, X, ldx, stage, taps, q, skip, Y, ldy, message, sizeof(message));
    if (status < 0) return shg::fail(SHG_ERR_INVALID, "%s", message);
    if (status > 0) return SHG_OK;
    hipStream_t stream = (hipStream_t)stream_;
    switch (K) {
        case 2: launch_whiten_vector<2>(groups, M, X, ldx, stage, taps, q, skip, Y, ldy, stream); break;
        case 3: launch_whiten_vector<3>(groups, M, X, ldx, stage, taps, q, skip, Y, ldy, stream); break;
        case 4: launch_whiten_vector<4>(groups, M, X, ldx, stage, taps, q, skip, Y, ldy, stream); break;
        case 5: launch_whiten_vector<5>(groups, M, X, ldx, stage, taps, q, skip, Y, ldy, stream); break;
        default: launch_whiten_vector<6>(groups, M, X, ldx, stage, taps, q, skip, Y, ldy, stream); break;
    }
    SHG_HIP(hipGetLastError());
    return SHG_OK;
}

// Lagged products of the rows of a matrix with themselves, cut at arc boundaries, for up to 4095 lags on the fp64 MFMA
// (shg_segment_lag_products_long): the definition of shg_segment_lag_products (lags.hip),
//
//   S[r][s][k] = sum over t with seg[s] <= t and t + k < seg[s+1] of X[r][t] X[r][t + k],   k = 0 .. lags <= 4095
//
// Formulation.  Relative to the start of the segment, with zeros outside it,
//
//   A[i][c] = x[c - 16 i],   B[c][j] = x[c + j + k0],   D[i][j] = sum_c A[i][c] B[c][j] = sum_t x[t] x[t + k0 + 16 i + j]:
//
// every entry of a 16 x 16 accumulator of v_mfma_f64_16x16x4_f64 is one complete lag, a tile is the 256 lags k0 .. k0 + 255 in row-major
// order, 16 tiles hold 0 .. 4095, and nothing is discarded.
// Work items.  A segment is cut into chunks of 2048 columns counted from its start, and its last chunk takes what is left, up to 2560
// (a short remainder costs its 240 columns of skew again and keeps one wave busy).  A chunk is one workgroup of 4 waves, which stages
// x[chunk start .. + 2560 + 272 + k0 of the last tile) in LDS once, +0.0 by a select where the segment has ended.  Wave w takes the
// first factors x[t] of quarter w of the chunk (512 columns; a fourth of a chunk above 2048, rounded up to 4) against all their
// partners, in sweeps of at most 4 tiles (4 accumulators = 32 registers) over the columns c = quarter start .. + length + 240 in
// steps of 4.
// Operands.  The A fragment of a step is "row i = lane & 15, column c0 + (lane >> 4)": the rows lie 16 doubles apart, so read from LDS
// the 32 lanes of a ds_read_b64 group would meet 4 banks.  It is not read: A[i][c + 16] = A[i - 1][c], so the fragment of step n + 4 is
// the fragment of step n moved one lane up inside each row of 16 lanes (one DPP row_shr:1 per half) with x[c0 + (lane >> 4)] entering
// at i = 0 -- 4 registers hold the fragments of the steps n mod 4, and the one LDS read per step has 4 distinct addresses (broadcast).
// A value keeps its t on the way through the lanes, so "t inside the quarter" is one select where it enters.  The B fragment is
// "column j = lane & 15, row c0 + (lane >> 4)", x[c0 + k0 + (lane & 15) + (lane >> 4)]: 17 consecutive doubles per 32 lanes, no conflict.
// Sums.  A wave's entry is the chain over its steps in ascending t; the four quarters are added as ((q0 + q1) + q2) + q3 by wave 0
// (through LDS), which writes the chunk's 256 lags per tile to the workspace of the call; a second kernel adds the chunks of a (row,
// segment) in ascending order and writes S.  No atomics.  Nothing in the order of an entry depends on the row, lags (a sweep of fewer
// tiles runs the same chain per tile), the other segments, the position of the segment or the launch; the cut into chunks and quarters
// depends on the length of the segment alone.
// Zeros multiply values of the segment (a first factor outside the quarter, a partner past the end), so those must be finite.
#include "lags_device.h"
#include "lags_long_host.h"

namespace shg {
namespace {

struct LagLongSlot {            // what a workgroup needs of its chunk
    int start, end;             // the segment in the clamped table; start > end: no chunk has this slot
    int first;                  // first column of the chunk, relative to start
    int pad;
};
struct LagLongSegment {         // what the second kernel needs of a segment
    int slot, chunks;           // its chunks have the slots slot .. slot + chunks - 1
};

// one wave per segment: the chunks of segment s get their slots, and every slot from its first one to the first one of segment s + 1
// (segment 0: from slot 0; the last segment: to the last slot) is written, so that no slot is left as it was
__global__ __launch_bounds__(kLagLongWaves * 64) void lag_long_slots_kernel(int M, int nseg, const int32_t* __restrict__ seg, long long slots,
                                                                            LagLongSlot* __restrict__ slot_table,
                                                                            LagLongSegment* __restrict__ segment_table) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * kLagLongWaves;
    for (long long item = (long long)blockIdx.x * kLagLongWaves + (threadIdx.x >> 6); item < nseg; item += waves) {
        const int s = (int)item;
        int start, end;
        segment_range(seg, s, M, lane, start, end);
        const long long own = lag_long_first_slot(start, s);
        const int chunks = lag_long_chunks(end - start);
        const long long from = s == 0 ? 0 : own;
        const long long to = s == nseg - 1 ? slots : lag_long_first_slot(end, s + 1);       // segment s + 1 starts at `end`
        for (long long slot = from + lane; slot < to; slot += 64) {
            const bool used = slot >= own && slot < own + chunks;
            LagLongSlot info;
            info.start = used ? start : 1;
            info.end = used ? end : 0;
            info.first = used ? (int)(slot - own) * kLagLongChunk : 0;
            info.pad = 0;
            slot_table[slot] = info;
        }
        if (lane == 0) {
            LagLongSegment info;
            info.slot = (int)own;
            info.chunks = chunks;
            segment_table[s] = info;
        }
    }
}

// the A fragment of four steps on: every row of 16 lanes moves one lane up, `fresh` enters at its lane 0 (bound_ctrl off: a lane without
// a source keeps the old value, which is `fresh`)
__device__ inline double shift_in(double held, double fresh) {
    const long long hb = __builtin_bit_cast(long long, held), fb = __builtin_bit_cast(long long, fresh);
    const int lo = __builtin_amdgcn_update_dpp((int)fb, (int)hb, 0x111, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(fb >> 32), (int)(hb >> 32), 0x111, 0xF, 0xF, false);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}

typedef double __attribute__((address_space(3))) lds_double_t;

// one sweep of a wave: T tiles from lag k0 on over the quarter that starts at column q0 of the staged values and has `length` columns
template <int T>
__device__ inline void lag_long_sweep(const lds_double_t* xs, int q0, int length, int steps, int k0, int fr, int fk, double4_t (&acc)[T]) {
    const lds_double_t* ap = xs + q0 + fk;                      // x[c0 + (lane >> 4)]: what enters A at row 0
    const lds_double_t* bp = xs + q0 + fk + fr + k0;            // B[c0 + (lane >> 4)][lane & 15] of the first tile
    const int alive = length - fk;                              // the entering value lies in the quarter while 4 n < alive
    double a[4] = {0.0, 0.0, 0.0, 0.0};                         // columns in front of the quarter: zeros
    for (int n = 0; n < steps; n += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int off = 4 * (n + u);
            const double entering = ap[off];
            a[u] = shift_in(a[u], off < alive ? entering : 0.0);
#pragma unroll
            for (int tile = 0; tile < T; ++tile)
                acc[tile] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], bp[off + tile * kLagLongTile], acc[tile], 0, 0, 0);
        }
    }
}

// C/D layout: column j = lane & 15, row i = (lane >> 4) + 4 reg: lag k0 + 16 i + j = k0 + 64 reg + lane
template <int T>
__device__ inline void lag_long_tiles_of(const lds_double_t* xs, double* comb, int wave, int lane, int q0, int length, int steps, int tile0,
                                         double* __restrict__ out) {
    double4_t acc[T];
#pragma unroll
    for (int tile = 0; tile < T; ++tile) acc[tile] = (double4_t){0.0, 0.0, 0.0, 0.0};
    if (steps > 0) lag_long_sweep<T>(xs, q0, length, steps, tile0 * kLagLongTile, lane & 15, lane >> 4, acc);
    if (wave > 0) {
        double* mine = comb + (wave - 1) * kLagLongGroup * kLagLongTile;
#pragma unroll
        for (int tile = 0; tile < T; ++tile)
#pragma unroll
            for (int r = 0; r < 4; ++r) mine[tile * kLagLongTile + 64 * r + lane] = acc[tile][r];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int tile = 0; tile < T; ++tile)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int e = tile * kLagLongTile + 64 * r + lane;
                double v = acc[tile][r];
#pragma unroll
                for (int w = 1; w < kLagLongWaves; ++w) v += comb[(w - 1) * kLagLongGroup * kLagLongTile + e];
                out[tile0 * kLagLongTile + e] = v;
            }
    }
    __syncthreads();                                            // the next sweep writes comb again
}

__global__ __launch_bounds__(kLagLongWaves * 64, 2) void lag_long_kernel(long long items, long long slots, const double* __restrict__ X, long long ldx,
                                                                         int tiles, int staged, const LagLongSlot* __restrict__ slot_table,
                                                                         double* __restrict__ partial) {
    extern __shared__ double lds[];                             // [staged values of x | accumulators of the waves 1 .. 3 of a sweep]: 78.0 KB
    double* comb = lds + (kLagLongLds - (kLagLongWaves - 1) * kLagLongGroup * kLagLongTile);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const lds_double_t* xs = (const lds_double_t*)lds;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const long long row = item / slots;
        const LagLongSlot info = slot_table[item - row * slots];
        if (info.start > info.end) continue;                    // uniform: no chunk has this slot
        const int left = info.end - info.start - info.first;    // columns of the segment from the chunk on: > 0
        const double* x = X + row * ldx + info.start + info.first;
        __syncthreads();                                        // the previous item's reads of the staged values are done
        for (int i = tid; i < staged; i += kLagLongWaves * 64) {
            const double v = x[min(i, left - 1)];               // inside the segment whatever i
            lds[i] = i < left ? v : 0.0;
        }
        __syncthreads();
        const int take = lag_long_take(left);                   // columns of the chunk: the rest of the segment if it is the last one
        const int quarter = lag_long_quarter(take);
        const int q0 = wave * quarter;
        const int length = min(quarter, take - q0);             // <= 0: the chunk ends in front of this quarter
        const int steps = lag_long_steps(length);
        double* out = partial + item * tiles * kLagLongTile;
        int tile0 = 0;
        for (; tile0 + 4 <= tiles; tile0 += 4) lag_long_tiles_of<4>(xs, comb, wave, lane, q0, length, steps, tile0, out);
        if (tiles - tile0 >= 2) {
            lag_long_tiles_of<2>(xs, comb, wave, lane, q0, length, steps, tile0, out);
            tile0 += 2;
        }
        if (tiles - tile0 >= 1) lag_long_tiles_of<1>(xs, comb, wave, lane, q0, length, steps, tile0, out);
    }
}

// S[r][s][k] = the partial sums of the chunks of (r, s) in ascending order; 0 for a segment without columns
__global__ __launch_bounds__(256) void lag_long_sum_kernel(long long entries, long long slots, int lags, int nseg, int tiles,
                                                           const LagLongSegment* __restrict__ segment_table, const double* __restrict__ partial,
                                                           double* __restrict__ S) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    const int each = tiles * kLagLongTile;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < entries; e += stride) {
        const long long pair = e / (lags + 1);
        const int k = (int)(e - pair * (lags + 1));
        const long long row = pair / nseg;
        const LagLongSegment info = segment_table[pair - row * nseg];
        const double* p = partial + (row * slots + info.slot) * each + k;
        double v = 0.0;
        if (info.chunks > 0) v = p[0];
        for (int chunk = 1; chunk < info.chunks; ++chunk) v += p[(long long)chunk * each];
        S[e] = v;
    }
}

}  // namespace
}  // namespace shg

using namespace shg;

extern "C" int shg_segment_lag_long_info(int* chunk, int* tile_lags, int* max_lags) {
    if (chunk) *chunk = kLagLongChunk;
    if (tile_lags) *tile_lags = kLagLongTile;
    if (max_lags) *max_lags = kLagLongMax;
    return SHG_OK;
}

extern "C" int shg_segment_lag_products_long(long long rows, int M, const double* X, long long ldx, int lags, int nseg, const int32_t* seg, double* S,
                                             void* stream_) {
    char message[256];
    const int status = segment_lag_products_long_check(rows, M, X, ldx, lags, nseg, seg, S, message, sizeof(message));
    if (status < 0) return shg::fail(SHG_ERR_INVALID, "%s", message);
    if (status > 0) return SHG_OK;
    const LagLongGeometry g = segment_lag_products_long_geometry(rows, M, nseg, lags);
    hipStream_t stream = (hipStream_t)stream_;
    SHG_SET_LDS_ONCE(lag_long_kernel, g.lds_bytes);
    Workspace ws = Workspace::pooled(stream);
    double* partial;
    LagLongSlot* slot_table;
    LagLongSegment* segment_table;
    if (!ws.alloc(partial, (size_t)g.partials, slot_table, (size_t)g.slots, segment_table, (size_t)nseg))
        return shg::fail(SHG_ERR_NOMEM, "shg_segment_lag_products_long: workspace allocation failed");
    const unsigned slot_blocks = (unsigned)std::min<long long>(ceil_div64(nseg, kLagLongWaves), 1 << 16);
    hipLaunchKernelGGL(lag_long_slots_kernel, dim3(slot_blocks), dim3(kLagLongWaves * 64), 0, stream, M, nseg, seg, g.slots, slot_table, segment_table);
    SHG_HIP(hipGetLastError());
    hipLaunchKernelGGL(lag_long_kernel, dim3(g.blocks), dim3(kLagLongWaves * 64), g.lds_bytes, stream, g.items, g.slots, X, ldx, g.tiles, g.staged,
                       slot_table, partial);
    SHG_HIP(hipGetLastError());
    const long long entries = rows * nseg * (lags + 1);
    const unsigned sum_blocks = (unsigned)std::min<long long>(ceil_div64(entries, 256), 1 << 16);
    hipLaunchKernelGGL(lag_long_sum_kernel, dim3(sum_blocks), dim3(256), 0, stream, entries, g.slots, lags, nseg, g.tiles, segment_table, partial, S);
    SHG_HIP(hipGetLastError());
    return SHG_OK;
}

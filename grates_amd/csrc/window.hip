// Window expansion of a transposed design matrix (shg_window_expand): the adjoint of the window model of the shg_*_points_at calls,
// for parameters that vary in time.
//
//   S[e][r][t] = factors[t][e - slot(t)] * T[r][t]   for slot(t) <= e < slot(t) + W,   +0.0 for every other e < E
//
// slot(t) is constant along runs of columns (run_begin, run_slot).  Bandwidth-bound: one read of T, E writes, no arithmetic worth the
// name.  Lanes run along t, the unit-stride axis of T and of every slot of S; a lane keeps the W factors of its columns in registers,
// walks down the rows, loads a value once and stores its E outputs, each exactly once: the zeros in front of the window, the W
// products, the zeros behind it.  Where the pointers and strides allow, a lane holds two adjacent columns and stores 16 bytes; a pair
// that straddles a run boundary (two slots) and the last column of an odd n are stored 8 bytes at a time.
#include "common.h"

namespace shg {

constexpr int kExpandThreads = 256;
constexpr int kExpandMaxSlots = 16;                                  // W <= E <= 16: the window of the shg_*_points_at calls
constexpr int kExpandBlocks = 256 * 8;                               // workgroups in flight; the rows beyond are a grid stride

// slot of column t: that of the run r with run_begin[r] <= t < run_begin[r + 1] (the host checked the tables: 0 .. n covered, ascending)
__device__ inline int expand_slot(const int32_t* __restrict__ run_begin, const int32_t* __restrict__ run_slot, int runs, int t) {
    int lo = 0, hi = runs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (run_begin[mid] <= t) lo = mid; else hi = mid - 1;
    }
    return run_slot[lo];
}

// the E outputs of one value: y points at S[0][r][t]
__device__ inline void expand_store(double* __restrict__ y, long long slot_stride, int slot, int W, int E, const double (&f)[kExpandMaxSlots], double v) {
    for (int e = 0; e < slot; ++e) y[e * slot_stride] = 0.0;
#pragma unroll
    for (int j = 0; j < kExpandMaxSlots; ++j)
        if (j < W) y[(slot + j) * slot_stride] = f[j] * v;
    for (int e = slot + W; e < E; ++e) y[e * slot_stride] = 0.0;
}

template <int V>                                                     // columns per lane: 2 (16-byte loads and stores) or 1
__global__ __launch_bounds__(kExpandThreads) void window_expand_kernel(long long rows, int n, const double* __restrict__ T, long long ldt,
                                                                       const int32_t* __restrict__ run_begin, const int32_t* __restrict__ run_slot,
                                                                       int runs, const double* __restrict__ factors, int W, int E,
                                                                       double* __restrict__ S, long long lds, long long slot_stride) {
    const long long column = ((long long)blockIdx.x * kExpandThreads + threadIdx.x) * V;
    if (column >= n) return;
    const int t = (int)column;
    const bool two = V == 2 && t + 1 < n;
    const int s0 = expand_slot(run_begin, run_slot, runs, t);
    const int s1 = two ? expand_slot(run_begin, run_slot, runs, t + 1) : s0;
    double f0[kExpandMaxSlots], f1[kExpandMaxSlots];
#pragma unroll
    for (int j = 0; j < kExpandMaxSlots; ++j) {
        f0[j] = j < W ? factors[(size_t)t * W + j] : 0.0;
        f1[j] = two && j < W ? factors[(size_t)(t + 1) * W + j] : 0.0;
    }
    for (long long row = blockIdx.y; row < rows; row += gridDim.y) {
        const double* x = T + row * ldt + t;
        double* y = S + row * lds + t;
        if (V == 2 && two && s0 == s1) {
            const double2 v = *reinterpret_cast<const double2*>(x);
            for (int e = 0; e < s0; ++e) *reinterpret_cast<double2*>(y + e * slot_stride) = make_double2(0.0, 0.0);
#pragma unroll
            for (int j = 0; j < kExpandMaxSlots; ++j)
                if (j < W) *reinterpret_cast<double2*>(y + (s0 + j) * slot_stride) = make_double2(f0[j] * v.x, f1[j] * v.y);
            for (int e = s0 + W; e < E; ++e) *reinterpret_cast<double2*>(y + e * slot_stride) = make_double2(0.0, 0.0);
        } else {
            expand_store(y, slot_stride, s0, W, E, f0, x[0]);
            if (two) expand_store(y + 1, slot_stride, s1, W, E, f1, x[1]);
        }
    }
}

}  // namespace shg

using namespace shg;

extern "C" int shg_window_expand(long long rows, int n, const double* T, long long ldt, const int32_t* run_slot, const int32_t* run_begin, int runs,
                                 const double* factors, int W, int E, double* S, long long lds, long long slot_stride, void* stream_) {
    const char* fn = "shg_window_expand";
    hipStream_t stream = (hipStream_t)stream_;
    SHG_REQUIRE(rows >= 0 && n >= 0 && ldt >= 0 && lds >= 0 && slot_stride >= 0, "%s: negative size (rows %lld, n %d, ldt %lld, lds %lld, slot_stride %lld)",
                fn, rows, n, ldt, lds, slot_stride);
    SHG_REQUIRE(W >= 1 && W <= kExpandMaxSlots, "%s: window of %d fields, expected 1 .. %d", fn, W, kExpandMaxSlots);
    SHG_REQUIRE(E >= W && E <= kExpandMaxSlots, "%s: %d slots, expected W = %d .. %d", fn, E, W, kExpandMaxSlots);
    SHG_REQUIRE(runs >= 0, "%s: negative number of runs %d", fn, runs);
    SHG_REQUIRE(ldt >= n, "%s: ldt %lld below n %d", fn, ldt, n);
    SHG_REQUIRE(lds >= n, "%s: lds %lld below n %d", fn, lds, n);
    const long long limit = 1LL << 40;
    SHG_REQUIRE((ldt == 0 || rows <= limit / ldt) && (lds == 0 || rows <= limit / lds), "%s: %lld rows of %lld (T) and %lld (S) values are too large", fn,
                rows, ldt, lds);
    const long long extent = rows > 0 ? (rows - 1) * lds + n : 0;                        // values of one slot, first to last
    SHG_REQUIRE(slot_stride >= extent, "%s: slot_stride %lld below the %lld values of one slot", fn, slot_stride, extent);
    SHG_REQUIRE(slot_stride <= limit / kExpandMaxSlots, "%s: %d slots of %lld values are too large", fn, E, slot_stride);
    if (rows == 0 || n == 0) return SHG_OK;
    SHG_REQUIRE(T && run_slot && run_begin && factors && S, "%s: NULL pointer", fn);
    // the run tables in full, before the first HIP call: no table content reaches the kernel unchecked
    SHG_REQUIRE(runs >= 1, "%s: no run for %d columns", fn, n);
    SHG_REQUIRE(run_begin[0] == 0, "%s: run_begin[0] is %d, not 0", fn, run_begin[0]);
    for (int r = 0; r < runs; ++r) {
        SHG_REQUIRE(run_begin[r + 1] > run_begin[r] && run_begin[r + 1] <= n, "%s: run_begin must increase strictly up to n %d (run %d: %d, %d)", fn, n, r,
                    run_begin[r], run_begin[r + 1]);
        SHG_REQUIRE(run_slot[r] >= 0 && run_slot[r] <= E - W, "%s: run %d starts at slot %d, outside 0 .. E - W = %d", fn, r, run_slot[r], E - W);
    }
    SHG_REQUIRE(run_begin[runs] == n, "%s: the runs end at column %d, not at n %d", fn, run_begin[runs], n);
    const uintptr_t t0 = (uintptr_t)T, t1 = (uintptr_t)(T + (rows - 1) * ldt + n), s0 = (uintptr_t)S,
                    s1 = (uintptr_t)(S + (E - 1) * slot_stride + extent);
    SHG_REQUIRE(t1 <= s0 || s1 <= t0, "%s: T and S overlap (the call is out of place)", fn);

    std::vector<int32_t> table(run_begin, run_begin + runs + 1);                         // run_begin [runs + 1], then run_slot [runs]
    table.insert(table.end(), run_slot, run_slot + runs);
    Workspace ws = Workspace::plain(stream);
    int32_t* table_d;
    if (!ws.alloc(table_d, table.size())) return fail(SHG_ERR_NOMEM, "%s: workspace allocation failed", fn);
    SHG_HIP(hipMemcpyAsync(table_d, table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    SHG_HIP(hipStreamSynchronize(stream));                                                 // the host table goes out of scope
    const bool wide = n >= 2 && (t0 | s0) % 16 == 0 && ldt % 2 == 0 && lds % 2 == 0 && slot_stride % 2 == 0;
    const int per_lane = wide ? 2 : 1;
    const unsigned gx = (unsigned)ceil_div64(n, (long long)kExpandThreads * per_lane);
    const unsigned gy = (unsigned)std::min<long long>(rows, std::max<long long>(1, kExpandBlocks / gx));
    if (wide)
        hipLaunchKernelGGL(window_expand_kernel<2>, dim3(gx, gy), dim3(kExpandThreads), 0, stream, rows, n, T, ldt, table_d, table_d + runs + 1, runs,
                           factors, W, E, S, lds, slot_stride);
    else
        hipLaunchKernelGGL(window_expand_kernel<1>, dim3(gx, gy), dim3(kExpandThreads), 0, stream, rows, n, T, ldt, table_d, table_d + runs + 1, runs,
                           factors, W, E, S, lds, slot_stride);
    SHG_HIP(hipGetLastError());
    return SHG_OK;
}

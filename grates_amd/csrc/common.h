// Shared declarations of libshg (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <vector>

#include "../../include/shg.h"

namespace shg {

typedef double double4_t __attribute__((ext_vector_type(4)));        // the accumulator of one v_mfma_f64_16x16x4_f64

int fail(int code, const char* fmt, ...);
unsigned hip_failures();      // how many HIP errors fail() has reported so far: device state that a launch leaves behind is suspect when this has moved
// Zero fills as kernels of this library (plan.hip), for the paths that several host threads feed at once (the chains of the
// block-banded smoother, one thread and one stream each): on ROCm 7.2 a 4-byte hipMemsetAsync issued from four threads on
// four streams left 0x80808080 in its target about four runs in five (the pivot flag of blockchol.hip's factorisation; with a
// kernel in its place, never).  rows x cols doubles with leading dimension ld (ld == cols: one contiguous run).
int zero_fill(double* p, long long ld, long long cols, long long rows, hipStream_t stream);
int zero_fill(int* p, hipStream_t stream);
// one triangle of square matrices into contiguous [batch][n][n] storage, zeros on the other side, which is not read (plan.hip)
int triangle_copy(int n, const double* src, int ld, long long stride, int batch, double* dst, bool upper, hipStream_t stream);
// grow-only scratch of a stream (plan.hip), kept until shg_scratch_release(); one slot per buffer that is live at the same time
enum ScratchSlot { kScratchSplitK = 0, kScratchAnaFold = 1, kScratchAnaTransform = 2, kScratchAnaSolution = 3, kScratchAnaFlag = 4,
                   kScratchSeriesIn = 5, kScratchSeriesOut = 6 /* order-major copies of a batch in the reference layout (filters.hip) */,
                   kScratchTriangle = 7 /* zero-filled copies of the triangular operands of shg_gemm_ex (blas.hip) */,
                   kScratchBlocks = 8 /* and up: the workspaces of one block-matrix call (blockchol.hip) */ };
class ScratchLease {          // the scratch buffers of one stream, held while the operations that use them are enqueued (plan.hip)
public:
    explicit ScratchLease(hipStream_t stream);
    ~ScratchLease();
    ScratchLease(const ScratchLease&) = delete;
    ScratchLease& operator=(const ScratchLease&) = delete;
    void* get(int slot, size_t bytes);
    // two more streams of the same device for work that runs beside the leased stream (the look-ahead of blas.hip's
    // factorisation), with the events that order them; created on first use, kept with the scratch buffers
    int side(hipStream_t streams[2], hipEvent_t* to_side, hipEvent_t from_side[2]);
    int event(int i, hipEvent_t* ev);       // further events of the stream (0 .. 7), created on first use
    int sides_apart() const;                // how many of the side streams have a hardware queue of their own (0 .. 2)
private:
    void* owner_;
};
// The block row of a chain continues to the right of its diagonal block A [n x n] with ONE coupling block B [n x nc] (which
// becomes W = U^-T B) above the next diagonal block S [nc x nc] (which becomes the Schur complement S - W^T W).  The panel
// sweep over A simply carries on through B and S: step k solves its 128 rows of B, subtracts their products from the rows of B
// below and from S -- on the side stream, under the leaves, instead of two d^3 products (and their launches) after the sweep.
struct Coupling {
    double* B;
    int ldb, nc;
    long long strideB;
    double* S;
    int lds;
    long long strideS;
    hipEvent_t inverse_done;      // recorded on the side stream behind the last product of the inverse; the caller's stream does
                                  // not wait for it (lookahead_join does)
};

// gemm_tall.hip: C = alpha A B + beta C for tall A [M x K] and at most 240 columns (the dense filter product)
bool gemm_tall_shape(bool ta, bool tb, int M, int N, int K, int batch, bool upper_only, int tri, const double* A, int lda, const double* B, int ldb,
                     const double* C);
int gemm_tall(int M, int N, int K, double alpha, const double* A, int lda, const double* B, int ldb, double beta, double* C, int ldc, hipStream_t stream);

// blas.hip: batched C = alpha op(A) op(B) + beta C; tri: triangular structure of the operands (see GemmExParams::tri)
int gemm_ex(bool ta, bool tb, int M, int N, int K, double alpha, const double* A, int lda, long long strideA, const double* B, int ldb,
            long long strideB, double beta, double* C, int ldc, long long strideC, int batch, bool upper_only, hipStream_t stream);
int gemm_ex_tri(bool ta, bool tb, int M, int N, int K, double alpha, const double* A, int lda, long long strideA, const double* B, int ldb,
                long long strideB, double beta, double* C, int ldc, long long strideC, int batch, bool upper_only, int tri, hipStream_t stream);
// blas.hip: Cholesky factors U (A = U^T U, in place) and their inverses
int factor_invert_batched(int n, double* A, int lda, long long strideA, double* X, int ldx, long long strideX, int batch, int* info,
                          hipStream_t stream);
int potrf_upper(int n, double* A, int lda, double* work, int* info, hipStream_t stream);
int trtri_upper(int n, const double* U, int ldu, double* X, int ldx, double* work, hipStream_t stream);
int potrf_inverse_batch(int n, double* A, int lda, long long strideA, double* X, int ldx, long long strideX, double* work, long long strideW,
                        int* info, int info_stride, int batch, const Coupling* cp, hipStream_t stream);
bool potrf_inverse_carries_coupling(int n, hipStream_t stream);
void potrf_inverse_set_lookahead(int mode);
int potrf_inverse_lookahead_mode();
size_t potrf_inverse_work(int n);

// gemm.hip / covprop.hip: products whose A entries are generated from per-point or per-plan tables
int covprop_build_cs_table(shg_plan* p, hipStream_t stream);
int covprop_rows(shg_plan* p, const double* cov, int Pn, int p_off, int lat0, int lat1, double* partial, hipStream_t stream);
int synth_generic(const double* pkd, int ldp, const double* csr, int ldcs, const int* rslot, long long idiv, long long jmod, int M,
                  const double* X, int K, int N, double* C, hipStream_t stream);
int covprop_generic(const double* pkd, int ldp, const double* csr, int ldcs, const int* rslot, long long idiv, long long jmod,
                    long long row0, int M, const double* cov, int Pn, int p_off, double* partial, double* sigma, shg_plan* prof,
                    hipStream_t stream, bool symmetric, bool transposed_table, const unsigned* csoff = nullptr, int pk_rows = 0, int ldcov = 0);

// plan.hip: recursion factors a_nm / b_nm in packed order-major layout (the reference's expression order)
void recursion_tables(int N, std::vector<double>& a, std::vector<double>& b);

void stream_scratch_release();
hipError_t workspace_alloc(void** ptr, size_t bytes, hipStream_t stream);    // hipMallocAsync from a pool that keeps freed memory cached

#define SHG_HIP(call)                                                                              \
    do {                                                                                           \
        hipError_t _e = (call);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return shg::fail(SHG_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e),   \
                             __FILE__, __LINE__);                                                  \
    } while (0)

#define SHG_REQUIRE(cond, ...)                                                                     \
    do {                                                                                           \
        if (!(cond)) return shg::fail(SHG_ERR_INVALID, __VA_ARGS__);                               \
    } while (0)

// Device array that lives as long as its owner (a plan table): hipMalloc / hipFree.  ensure(n) keeps a buffer of at least n
// elements (grow-only workspaces), assign(n) replaces it by one of exactly n (tables rebuilt when their key changes); after a
// failed allocation the array is empty.
template <typename T>
class DeviceArray {
public:
    DeviceArray() = default;
    DeviceArray(DeviceArray&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    DeviceArray& operator=(DeviceArray&& o) noexcept { std::swap(p_, o.p_); std::swap(n_, o.n_); return *this; }
    ~DeviceArray() { reset(); }
    T* get() const { return p_; }
    size_t size() const { return n_; }
    explicit operator bool() const { return p_ != nullptr; }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        n_ = 0;
    }
    hipError_t ensure(size_t n) { return n <= n_ ? hipSuccess : assign(n); }
    hipError_t assign(size_t n) {
        reset();
        const hipError_t e = hipMalloc((void**)&p_, n * sizeof(T));
        if (e == hipSuccess) n_ = n; else p_ = nullptr;
        return e;
    }
private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

// a table of at least one element filled from the host
template <typename T>
int upload(DeviceArray<T>& dst, const std::vector<T>& src) {
    SHG_HIP(dst.assign(std::max<size_t>(src.size(), 1)));
    if (!src.empty()) SHG_HIP(hipMemcpy(dst.get(), src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return SHG_OK;
}

// Device buffers of one call, allocated on a stream and given back with hipFreeAsync on that stream, in the order of their
// allocation, when the workspace goes out of scope.  pooled(): workspace_alloc; plain(): hipMallocAsync from the pool as it is.
class Workspace {
public:
    static Workspace pooled(hipStream_t stream) { return Workspace(stream, true); }
    static Workspace plain(hipStream_t stream) { return Workspace(stream, false); }
    Workspace(Workspace&& o) noexcept : stream_(o.stream_), pooled_(o.pooled_), bufs_(std::move(o.bufs_)) { o.bufs_.clear(); }
    Workspace& operator=(Workspace&&) = delete;
    ~Workspace() {
        for (void* q : bufs_) (void)hipFreeAsync(q, stream_);
    }
    // alloc(a, na, b, nb, ...): na elements for a, then nb for b, ...; false when one of them fails (the others stay owned)
    template <typename T, typename... More>
    bool alloc(T*& p, size_t n, More&&... more) {
        void* q = nullptr;
        if ((pooled_ ? workspace_alloc(&q, n * sizeof(T), stream_) : hipMallocAsync(&q, n * sizeof(T), stream_)) != hipSuccess) return false;
        bufs_.push_back(q);
        p = static_cast<T*>(q);
        if constexpr (sizeof...(More) > 0) return alloc(std::forward<More>(more)...);
        return true;
    }
private:
    Workspace(hipStream_t stream, bool pooled) : stream_(stream), pooled_(pooled) {}
    hipStream_t stream_;
    bool pooled_;
    std::vector<void*> bufs_;
};

// Knock-out switches for timing experiments (results are wrong with any of them on) exist in -DSHG_EXPERIMENT builds only
// (`make timeline` -> libshg_timeline.so, never loaded by the package): the shipping library reads no environment variable.
#ifdef SHG_EXPERIMENT
#define SHG_DBG(P, bits) ((P).dbg & (bits))
inline int experiment_switches() {
    const char* e = getenv("SHG_DEBUG");
    return e ? atoi(e) : 0;
}
#else
#define SHG_DBG(P, bits) 0
#if (defined(SHG_ROT_X) && SHG_ROT_X) || (defined(SHG_PIPE_X) && SHG_PIPE_X) || (defined(SHG_GEMM_X) && SHG_GEMM_X) || (defined(SHG_ANA_X) && SHG_ANA_X) || (defined(SHG_FILT_X) && SHG_FILT_X) || (defined(SHG_TALL_X) && SHG_TALL_X)
#error "SHG_ROT_X / SHG_GEMM_X / SHG_ANA_X / SHG_FILT_X are timing experiments: build with -DSHG_EXPERIMENT (make timeline)"
#endif
#endif

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per kernel and device instead of in front of every launch: the call goes
// through the runtime's process-wide lock, and a smoother chain issues ~100 launches per epoch from several host threads.
#define SHG_SET_LDS_ONCE(fn, bytes)                                                                                        \
    do {                                                                                                                   \
        static std::atomic<unsigned long long> done_{0};                                                                   \
        int dev_ = 0;                                                                                                      \
        (void)hipGetDevice(&dev_);                                                                                         \
        const unsigned long long bit_ = 1ull << (dev_ & 63);                                                               \
        if (!(done_.load(std::memory_order_acquire) & bit_)) {                                                             \
            SHG_HIP(hipFuncSetAttribute((const void*)(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes)));     \
            done_.fetch_or(bit_, std::memory_order_release);                                                               \
        }                                                                                                                  \
    } while (0)

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline int round_up(int a, int b) { return ceil_div(a, b) * b; }
inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// packed order-major index of (n, m), n >= m:  off(m) + n - m,  off(m) = m (N+1) - m (m-1) / 2
__host__ __device__ inline int order_offset(int N, int m) { return m * (N + 1) - (m * (m - 1)) / 2; }
__host__ __device__ inline int packed_count(int N) { return (N + 1) * (N + 2) / 2; }

// Factors of the derivative map D of the solid harmonics (gravity_points.hip, design.hip), of the input coefficient (n, m): f- goes with
// P_{n+1,m-1} (m >= 1), f0 with P_{n+1,m}, f+ with P_{n+1,m+1}; f- of order 1 and f+ of order 0 carry the reference's extra sqrt(2).
__host__ __device__ inline double d_factor_base(double dn) { return sqrt((2.0 * dn + 1.0) / (2.0 * dn + 3.0)); }
__host__ __device__ inline double d_factor_minus(int n, int m) {
    const double dn = n, dm = m;
    double f = sqrt((dn - dm + 1.0) * (dn - dm + 2.0)) * d_factor_base(dn);
    if (m == 1) f *= sqrt(2.0);
    return f;
}
__host__ __device__ inline double d_factor_zero(int n, int m) {
    const double dn = n, dm = m;
    return sqrt((dn - dm + 1.0) * (dn + dm + 1.0)) * d_factor_base(dn);
}
__host__ __device__ inline double d_factor_plus(int n, int m) {
    const double dn = n, dm = m;
    double f = sqrt((dn + dm + 1.0) * (dn + dm + 2.0)) * d_factor_base(dn);
    if (m == 0) f *= sqrt(2.0);
    return f;
}

// Exchange between the lanes 2q and 2q+1 that turns "4 rows x 1 column per lane" into "2 rows x 2 adjacent columns per lane":
//   even lanes: lo = x (own),                  hi = x of the odd neighbour
//   odd lanes:  lo = y of the even neighbour,  hi = y (own)
// One v_cndmask_b32 with a DPP source (quad_perm [1, 0, 3, 2]) per 32-bit half: the select of the value to send, the DPP move
// and the select of the received value collapse into one instruction.  fp64 MFMAs and VALU instructions of all waves
// of a SIMD share one issue pipe (tools/mfma64_issue.hip), so every VALU instruction saved here is MFMA time.
// `odd` = lane mask of the odd lanes.  All lanes must be active.
__device__ inline void pair_exchange(double x, double y, unsigned long long odd, double& lo, double& hi) {
    const long long xb = __builtin_bit_cast(long long, x), yb = __builtin_bit_cast(long long, y);
    const int x0 = (int)xb, x1 = (int)(xb >> 32), y0 = (int)yb, y1 = (int)(yb >> 32);
    int l0, l1, h0, h1;
    asm volatile(
        "s_nop 1\n\t"                                                   // VALU write -> DPP read of the same VGPR: 2 wait states
        "s_mov_b64 vcc, %[odd]\n\t"
        "v_cndmask_b32_dpp %[h0], %[x0], %[y0], vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"     // odd ? y : x of the neighbour
        "v_cndmask_b32_dpp %[h1], %[x1], %[y1], vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "s_not_b64 vcc, vcc\n\t"
        "v_cndmask_b32_dpp %[l0], %[y0], %[x0], vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"     // even ? x : y of the neighbour
        "v_cndmask_b32_dpp %[l1], %[y1], %[x1], vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf"
        : [l0] "=&v"(l0), [l1] "=&v"(l1), [h0] "=&v"(h0), [h1] "=&v"(h1)
        : [x0] "v"(x0), [x1] "v"(x1), [y0] "v"(y0), [y1] "v"(y1), [odd] "s"(odd)
        : "vcc", "scc");
    lo = __builtin_bit_cast(double, ((long long)l1 << 32) | (unsigned int)l0);
    hi = __builtin_bit_cast(double, ((long long)h1 << 32) | (unsigned int)h0);
}


// value of the lane 8 positions away inside the row of 16 lanes (DPP row_ror:8)
__device__ inline double swap_half_row(double x) {
    const long long bits = __builtin_bit_cast(long long, x);
    const int lo = (int)bits, hi = (int)(bits >> 32);
    const int lo2 = __builtin_amdgcn_update_dpp(0, lo, 0x128, 0xF, 0xF, true);
    const int hi2 = __builtin_amdgcn_update_dpp(0, hi, 0x128, 0xF, 0xF, true);
    return __builtin_bit_cast(double, ((long long)hi2 << 32) | (unsigned int)lo2);
}

constexpr int kRotMaxClasses = 6; // classes r = 0 .. R / 2 of the rotation-folded synthesis kernel, R <= 10
// Order pruning of that kernel (synthesis_rot.hip): one record of kRotLevelInts ints per latitude block,
//   [0] npieces  [1] nslot  [2] nrec  [3] ntrip  [4] first trig piece of the level's stream  [5] first record of its item table
//   [8 ..] cls_nk[kRotMaxClasses]  [14 ..] cls_cnt[kRotMaxClasses]
constexpr int kRotLevelInts = 24;
constexpr int kRotPruneMaxDegree = 128;   // cut-offs are worked out for plans up to this degree (the panel of that kernel fits the LDS up to ~110)
constexpr int kEpochTile = 8;    // epochs handled together by one wave of the Legendre stage
constexpr int kLatTile = 64;     // parallels per wave of the Legendre stage (lane <-> parallel)

}  // namespace shg

// Device-resident tables of one (degree, parallels, kn, meridians) configuration.
struct shg_plan {
    int device = 0;
    int N = 0, nlat = 0, nlon = 0;
    int ldlat = 0;          // nlat rounded up to 64: leading dimension of per-parallel tables / F
    bool sym4 = false;      // 4-fold longitude symmetry path
    int rotR = 0;           // rotations of the meridian set used by the rotation-folded kernel (synthesis_rot.hip): 10, 9, 6, 3 or 0 = not applicable
    std::vector<double> lon_host;   // meridians as given (the trig stream of that kernel is rebuilt when shg_plan_set_rotations changes R)
    shg::DeviceArray<double> rot_trig; // [column tiles][k-steps][64 lanes][2] cos / signed sin stream of that kernel, one per level of rot_level_set
    // order pruning of that kernel: a latitude block near a pole keeps the orders 0 .. level only (synthesis_rot.hip)
    bool order_pruning = true;        // shg_plan_set_order_pruning
    bool half_tile_fold = true;       // shg_plan_set_half_tile_fold
    std::vector<int> rot_levels;      // per latitude block of that kernel: largest order kept (N = everything)
    std::vector<int> rot_level_set;   // the distinct levels, N first, then descending: one layout, trig stream and item table each
    std::vector<int> rot_trig_piece;  // per level: first piece of its trig stream in rot_trig
    std::vector<int> rot_item_rec, rot_item_nrec, rot_item_ntrip;   // per level: first record / records per wave / trips of its item table in itemtab_d
    shg::DeviceArray<int> rot_levtab_d;   // [2][blocks][kRotLevelInts]: the level records of the blocks with pruning on, then off (every block at N)
    bool rot_levtab_valid = false;
    bool sym_ns = false;    // parallels (colatitude and kn rows) symmetric about the equator
    int ngroups = 1;        // 4 (sym4) or 1
    int goff[5] = {0, 0, 0, 0, 0};   // first K slot of each group (multiples of 4), goff[ngroups] = K
    int K = 0;              // total K slots of the longitude stage (multiple of 4)
    int ncol = 0;           // output columns per group: nlon/4 (sym4) or nlon
    int ncoltiles = 0;      // ceil(ncol / 16)
    int chunk = 16;         // epochs per pass

    // device tables
    shg::DeviceArray<double> ct;   // [ldlat] cos(colat)
    shg::DeviceArray<double> st;   // [ldlat] sin(colat)
    shg::DeviceArray<double> pmm;  // [N+1][ldlat] sectorial seeds P_mm(theta_i)
    shg::DeviceArray<double> knT;  // [N+1][ldlat] kn transposed
    shg::DeviceArray<double> arec; // [packed] recursion factor a_nm
    shg::DeviceArray<double> brec; // [packed] recursion factor b_nm
    shg::DeviceArray<double> trig; // [ncoltiles][K][16] cos/sin table, column-tile major
    // 64-row fused kernel: order 0 (constant along a parallel) leaves the K loop and becomes the start value of the cosine /
    // even-order accumulators, when that saves a body of 16 slots (d/o 96: 13 -> 12 bodies).  Slot K_f of the panel holds it.
    bool fold0 = false;
    int goff_f[5] = {0, 0, 0, 0, 0};
    int K_f = 0;
    shg::DeviceArray<double> trig_f; // [ncoltiles][K_f][16]
    shg::DeviceArray<double> lon;    // [nlon]
    shg::DeviceArray<double> colat;  // [nlat]
    // covariance-propagation tables (built lazily)
    shg::DeviceArray<double> pk_deg;      // [nlat][Pfull] kn-scaled P_nm in degree-wise order (nmin = 0)
    shg::DeviceArray<double> cs_slot;     // [2N+1][nlon] cos/sin per slot (0, 1c, 1s, 2c, 2s, ...)
    shg::DeviceArray<int> rslot;          // [Pfull] rank inside its degree of every degree-wise index
    shg::DeviceArray<double> cov_partial; // [column blocks][band rows] partial row sums of the covariance kernel
    shg::DeviceArray<double> cov_pad;     // covariance matrix copied to rows of even length (16-byte aligned rows for the LDS copy of the kernel)
    // workspace
    shg::DeviceArray<double> cpk; // [packed][2][chunk_pad] repacked coefficients of one pass
    shg::DeviceArray<double> F;   // [chunk][K][ldlat] output of the Legendre stage
    int chunk_alloc = 0;
    // fused synthesis path (synthesis_fused.hip)
    shg::DeviceArray<double> pk;  // [packed + 4][ldlat] kn-scaled Legendre table (two-kernel variant), built on first use
    shg::DeviceArray<double> pkf; // [nit][Qtot][64 lanes][2] the same table in MFMA-fragment order (fused kernel), built on first use
    shg::DeviceArray<int> qoff;   // [N+2] first row-octet of every order in the fragment-ordered tables; qoff[N+1] = Qtot
    int Qtot = 0;
    std::vector<int> ns_badmap; // per block of 8 northern parallels: -1, or rank among the blocks whose mirrored parallels get their own table
    int ns_nbad = 0;
    shg::DeviceArray<int> badmap_d;
    shg::DeviceArray<int> octinfo_d; // [Qtot] order | octet-in-order << 8 of every octet of the fragment-ordered tables
    shg::DeviceArray<int> itemtab_d; // work items of the fused kernel's Legendre stage, [8 waves][nrec][4]
    int itemtab_nrec = 0, itemtab_ntrip = 0;
    int itemtab_rot = -1;       // panel slot convention of the work items: 0 = 4-fold kernel, R = rotation-folded kernel
    const double* om_src = nullptr;   // set for the duration of shg_synthesis_om: the coefficient repack reads this order-major series
    int om_N = 0, om_Bpad = 0;
    shg::DeviceArray<int> tickets_d; // ticket queues of the rotation-folded kernel's Legendre stage, one 128-byte line per XCD (synthesis_rot.hip), allocated and zeroed by rot_set_stage_limit
    unsigned tickets_failures = 0;   // hip_failures() when the queues were last zeroed: zeroed again before the first launch after a HIP error
    int stage_limit = 0;        // workgroups that may run their Legendre stage at once (0 = no limit)
    bool stage_limit_set = false;    // by rot_set_stage_limit; until then the first launch of that kernel sets the default (synthesis_rot.hip)
    shg::DeviceArray<int> blockmap_d; // XCD-aware (epoch tile, parallel tile) order of the fused kernel's workgroups
    int blockmap_nbt = 0, blockmap_nit = 0;
    std::vector<char> ns_badrow;    // per northern parallel: mirror image deviates too much to share the northern table
    // two-workgroup fused synthesis (synthesis_fused32.hip): blocks of 4 northern parallels
    shg::DeviceArray<double> pkf32;
    shg::DeviceArray<int> qoff32;
    shg::DeviceArray<int> badmap32_d;
    int Qtot32 = 0, nbad32 = 0;
    int pkf_variant = 0;        // 1 plain fragment order, 2 north-south symmetric fragment order
    shg::DeviceArray<double> cpk4; // repacked coefficients of the whole batch: [ceil(B/4)][Qtot][32][2] (fused) or [ceil(B/8)][packed][2][8]
    int cpk4_variant = 0;       // layout the workspace was last zero-initialised for
    size_t cpk4_zeroed = 0;
    // analysis operator cache (analysis.hip): H[S][N+1][nlat] for the area weights ana_area and min degree ana_nmin
    shg::DeviceArray<double> ana_H;
    shg::DeviceArray<double> ana_Hp; // north-south parity form of the operator [S][2 ceil((N+1)/2)][nlat/2] (analysis.hip), valid when ana_parity
    bool ana_parity = false;
    double ana_parity_defect = -1.0;   // largest dropped entry / largest entry of H when ana_Hp was formed (-1: not formed)
    shg::DeviceArray<double> ana_area; // [nlat][nlon] copy of the area weights the operator was built for (compared on the device per call)
    int ana_nmin = -1;
    bool ana_rowconst = false;  // the weights of the cached operator are constant along every parallel (geographic and Gauss grids)
    shg::DeviceArray<double> ana_trig; // trig table of the fused transform kernel in chunk order [chunk][8 columns][4 groups x MT x 16 orders], zero padded
    int ana_trig_mt = 0;
    int path = 0;               // 0 auto, 1 three-kernel path, 2 fused 4-fold kernel, 5 fused kernel with 32-row panels (two workgroups per CU), 6 rotation-folded fused kernel

    // users of the plan are serialised (PlanGuard): its tables are built lazily and its workspaces are per plan, not per stream
    std::mutex mtx;
    hipStream_t last_stream = nullptr;
    bool used = false;
    hipEvent_t order_event = nullptr;

    // optional per-kernel event timing (shg_plan_profile)
    bool profiling = false;
    unsigned profile_mask = ~0u;            // kinds that are timed while profiling is on
    std::vector<hipEvent_t> prof_events;    // pairs (start, stop)
    std::vector<int> prof_kinds;
    size_t prof_used = 0;                   // number of pairs in use
};

namespace shg {
int plan_alloc_workspace(shg_plan* p);
int fused_chunk_for(const shg_plan* p);
int build_pk_table(shg_plan* p, hipStream_t stream);
int build_pkf_table(shg_plan* p, bool ns, int rotR, hipStream_t stream);
int build_blockmap(shg_plan* p, int nbt, int nit, hipStream_t stream);
int pack_coefficients_fused(shg_plan* p, bool ns, int rotR, const double* anm, int B, hipStream_t stream);
int synthesis_fused(shg_plan* p, const double* anm, int B, double* grid, hipStream_t stream);
bool has_rotation_symmetry(int nlon, const double* lon, int R);
int rot_layout(int R, int N, int nk[kRotMaxClasses], int cnt[kRotMaxClasses], std::vector<int>* order_slot);
int rot_choose(int nlon, const double* lon_h, int N);
int rot_applicable(const shg_plan* p);
int build_rot_trig(shg_plan* p, const double* lon_h);
void rot_order_cutoffs(int N, int nlat, const double* colat, const double* kn, bool ns, std::vector<int>& levels);
std::vector<int> rot_level_list(int N, const std::vector<int>& levels);
void rot_trig_stream(int R, int N, int level, int nlon, const double* lon_h, std::vector<double>& tab, bool fill_half);
void item_table_host(const shg_plan* p, int N, int level, int od, const std::vector<int>& qoff, int rotR, std::vector<int>& table, int& nrec, int& ntrip);
int synthesis_rot(shg_plan* p, const double* anm, int B, double* grid, hipStream_t stream);
int rot_kernel_waves();           // waves per workgroup of the rotation-folded kernel
int rot_set_stage_limit(shg_plan* p, int limit);
int fused32_applicable(const shg_plan* p);
int synthesis_fused32(shg_plan* p, const double* anm, int B, double* grid, hipStream_t stream);

// Entry points that work on a plan hold this for their duration: one host thread at a time, and a call on another stream than
// the previous one first waits (on the device) for everything that call has enqueued -- two streams or threads sharing a cached
// plan can then not overwrite each other's packed coefficients, panels or partial sums, and a reallocation never frees a
// buffer another stream still reads.  No cost while the stream stays the same.
struct PlanGuard {
    shg_plan* p;
    std::unique_lock<std::mutex> lock;
    PlanGuard(shg_plan* plan, hipStream_t stream) : p(plan), lock(plan->mtx) {
        if (p->used && p->last_stream != stream) {
            bool ordered = false;
            if (p->order_event || hipEventCreateWithFlags(&p->order_event, hipEventDisableTiming) == hipSuccess)
                ordered = hipEventRecord(p->order_event, p->last_stream) == hipSuccess && hipStreamWaitEvent(stream, p->order_event, 0) == hipSuccess;
            if (!ordered) {                      // e.g. the previous stream no longer exists
                (void)hipGetLastError();
                (void)hipDeviceSynchronize();
            }
        }
        p->last_stream = stream;
        p->used = true;
    }
};

// RAII event pair around one kernel launch (no-op unless profiling is enabled on the plan)
struct ProfileScope {
    shg_plan* p;
    hipStream_t stream;
    hipEvent_t stop = nullptr;
    ProfileScope(shg_plan* plan, int kind, hipStream_t s);
    ~ProfileScope();
};
}  // namespace shg

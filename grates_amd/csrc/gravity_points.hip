// Gravitational acceleration g and gradient tensor T = d^2 V / dx_c dx_d at arbitrary points (g replaces grates/gravityfield.py:423-481,
// three per-order Legendre tables of degree N + 1 per point and a dgemv per component and order; the reference has no T).
//
// The reference sums, per coefficient order m, P_{n+1,m-1} f-, P_{n+1,m} f0 and P_{n+1,m+1} f+ times (R/r)^(n+2).  Regrouped by the
// Legendre function (n', k), n' = n + 1 = 0 .. N + 1, each Cartesian component c is a point synthesis of degree N + 1:
//   g_c = GM / (2 R^2) sum_{n', k} (R/r)^(n'+1) P_{n'k} (cos(k lon) A^c_{n'k} + sin(k lon) B^c_{n'k}),    (A^c, B^c) = D_c(C, S)
// where D_c reads the orders k + 1 (C-, S-), k - 1 (C+, S+) and k (C0, S0) of degree n and writes (n + 1, k):
//   x: A = f- C- - f+ C+    B = f- S- - f+ S+        y: A = f- S- + f+ S+    B = -(f- C- + f+ C+)        z: A = -2 f0 C0    B = -2 f0 S0
// (the factors are d_factor_minus / _zero / _plus of common.h).  D works on any solid-harmonic coefficient set, so applying it to
// (A^c, B^c) differentiates once more: with (A^cd, B^cd) = D_d(D_c(C, S)) of degree N + 2,
//   T_cd = dg_c / dx_d = GM / (4 R^3) sum_{n'', k} (R/r)^(n''+1) P_{n''k} (cos(k lon) A^cd_{n''k} + sin(k lon) B^cd_{n''k}).
// Both are one computation with two parameterisations (Acceleration, Gradients below): a combine kernel forms the 2 C numbers A/B of
// the C components (x, y, z or xx, xy, xz, yy, yz, zz) per (n', k) of degree Nq = N + 1 or N + 2 and epoch once per call (the
// gradients' composition fused: the three first-derivative sets it needs are formed in registers), and solid_points_kernel runs one
// column recursion per point and (n', k), SolidColumn of solid.h, which the design matrices run too, for all components and every
// epoch of a pass.  xx, yy and zz each come from their own combination: the trace is a check, not an identity.
//
// The potential itself is the zeroth member of the family (Potential below): no D at all, the coefficients are the (C, S) of (n, k),
//   V = GM / R sum_{n, k} (R/r)^(n+1) P_{nk} (cos(k lon) C_{nk} + sin(k lon) S_{nk}),
// a point synthesis of degree N with one component.
#include "solid.h"

#include <climits>
#include <cmath>

namespace shg {

// Q [pass][packed (n', k) of degree Nq][2 C][EP]: A/B of the C components of EP consecutive epochs.
// Coefficient source: the reference layout anm [B][N+1][N+1] (om == nullptr) or an order-major series om [(N+1)^2][Bpad].
struct CoefSource {
    const double* anm;
    const double* om;
    int N, B, Bpad;
    __device__ double cos_coef(int b, int n, int m) const {
        if (om) return om[(size_t)(om_first_row(m == 0 ? 0 : 2 * m - 1) + n - m) * Bpad + b];
        return anm[((size_t)b * (N + 1) + n) * (N + 1) + m];
    }
    __device__ double sin_coef(int b, int n, int m) const {         // m >= 1
        if (om) return om[(size_t)(om_first_row(2 * m) + n - m) * Bpad + b];
        return anm[((size_t)b * (N + 1) + m - 1) * (N + 1) + n];
    }
    // first row of slot s (0: order 0 cosine, 2m - 1: order m cosine, 2m: order m sine): engine.order_major_first_row
    __device__ int om_first_row(int s) const {
        if (s == 0) return 0;
        const int m = (s + 1) >> 1;
        const int cos_row = (N + 1) + 2 * ((m - 1) * (N + 1) - m * (m - 1) / 2);
        return (s & 1) ? cos_row : cos_row + (N + 1 - m);
    }
};

// The inputs of D at output (np, k): the pairs (C, S) of orders k + 1 (minus), k - 1 (plus) and k (zero) of degree np - 1 with their
// factors.  A factor is zero where its term does not exist; the sine of an order-0 input is never read.
struct DTerms {
    double fm, fp, f0;
    double cm, sm, cp, sp, c0, s0;
};

__device__ inline void d_factors(int np, int k, DTerms& t) {
    t.fm = t.fp = t.f0 = 0.0;
    t.cm = t.sm = t.cp = t.sp = t.c0 = t.s0 = 0.0;
    if (np < 1) return;
    const int n = np - 1;
    if (np >= k + 2) t.fm = d_factor_minus(n, k + 1);
    if (k >= 1) t.fp = d_factor_plus(n, k - 1);
    if (np >= k + 1) t.f0 = d_factor_zero(n, k);
}

// D_c of the terms: (A, B) of component c (0: x, 1: y, 2: z)
__device__ inline void d_apply(int c, const DTerms& t, double& A, double& B) {
    if (c == 0) {
        A = t.fm * t.cm - t.fp * t.cp;
        B = t.fm * t.sm - t.fp * t.sp;
    } else if (c == 1) {
        A = t.fm * t.sm + t.fp * t.sp;
        B = -(t.fm * t.cm + t.fp * t.cp);
    } else {
        A = -2.0 * (t.f0 * t.c0);
        B = -2.0 * (t.f0 * t.s0);
    }
}

// first-derivative coefficients (A^c, B^c) [3][2] of degree n1 <= N + 1 and order k1 <= n1 of epoch b: D_c of the source
__device__ inline void first_derivative(const CoefSource& src, int b, int n1, int k1, double F[3][2]) {
    DTerms t;
    d_factors(n1, k1, t);
    const int n = n1 - 1;
    if (n1 >= k1 + 2) {
        t.cm = src.cos_coef(b, n, k1 + 1);
        t.sm = src.sin_coef(b, n, k1 + 1);
    }
    if (k1 >= 1) {
        t.cp = src.cos_coef(b, n, k1 - 1);
        t.sp = k1 >= 2 ? src.sin_coef(b, n, k1 - 1) : 0.0;
    }
    if (n1 >= k1 + 1) {
        t.c0 = src.cos_coef(b, n, k1);
        t.s0 = k1 >= 1 ? src.sin_coef(b, n, k1) : 0.0;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) d_apply(c, t, F[c][0], F[c][1]);
}

// The thread of a combine kernel: one per (n', k, epoch slot e) of `passes` passes of EP epochs starting at epoch b_first.  q is
// where its numbers go, EP apart; epochs b past B get zeros.
struct CombineSlot {
    int k, np, b;
    double* q;
};

__device__ inline bool combine_slot(int Nq, int numbers, int EP, int b_first, int passes, double* Q, CombineSlot& s) {
    const long long per_pass = (long long)packed_count(Nq) * EP;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= per_pass * passes) return false;
    const int pass = (int)(idx / per_pass);
    const long long rem = idx - pass * per_pass;
    const int e = (int)(rem % EP);
    const int p = (int)(rem / EP);
    int k = 0;                                                       // packed index p -> (k, n'): order_offset(Nq, k) <= p
    while (k < Nq && order_offset(Nq, k + 1) <= p) ++k;
    s.k = k;
    s.np = k + (p - order_offset(Nq, k));
    s.b = b_first + pass * EP + e;
    s.q = Q + (size_t)pass * per_pass * numbers + (size_t)p * numbers * EP + e;
    return true;
}

__global__ __launch_bounds__(256) void acceleration_combine_kernel(CoefSource src, int EP, int b_first, int passes, double* __restrict__ Q) {
    CombineSlot s;
    if (!combine_slot(src.N + 1, 6, EP, b_first, passes, Q, s)) return;
    double F[3][2] = {};
    if (s.b < src.B && s.np >= 1) first_derivative(src, s.b, s.np, s.k, F);
#pragma unroll
    for (int j = 0; j < 6; ++j) s.q[j * EP] = F[j / 2][j % 2];
}

__global__ __launch_bounds__(256) void gradients_combine_kernel(CoefSource src, int EP, int b_first, int passes, double* __restrict__ Q) {
    CombineSlot s;
    if (!combine_slot(src.N + 2, 12, EP, b_first, passes, Q, s)) return;
    const int np = s.np, k = s.k, b = s.b;
    double out[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) out[j] = 0.0;
    if (b < src.B && np >= 1) {
        DTerms t;
        d_factors(np, k, t);
        const int n1 = np - 1;                                       // degree of the first-derivative sets read
        double Fm[3][2] = {}, Fp[3][2] = {}, F0[3][2] = {};
        if (np >= k + 2) first_derivative(src, b, n1, k + 1, Fm);
        if (k >= 1) first_derivative(src, b, n1, k - 1, Fp);
        if (np >= k + 1) first_derivative(src, b, n1, k, F0);
        int j = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            DTerms tc = t;
            tc.cm = Fm[c][0];
            tc.sm = Fm[c][1];
            tc.cp = Fp[c][0];
            tc.sp = k >= 2 ? Fp[c][1] : 0.0;                         // the order-0 sine of the first derivative is never read
            tc.c0 = F0[c][0];
            tc.s0 = k >= 1 ? F0[c][1] : 0.0;
#pragma unroll
            for (int d = c; d < 3; ++d, j += 2) d_apply(d, tc, out[j], out[j + 1]);
        }
    }
#pragma unroll
    for (int j = 0; j < 12; ++j) s.q[j * EP] = out[j];
}

// the zeroth member: (A, B) = (C, S) of (n, k) itself, the sine of order 0 zero
__global__ __launch_bounds__(256) void potential_combine_kernel(CoefSource src, int EP, int b_first, int passes, double* __restrict__ Q) {
    CombineSlot s;
    if (!combine_slot(src.N, 2, EP, b_first, passes, Q, s)) return;
    const bool live = s.b < src.B;
    s.q[0] = live ? src.cos_coef(s.b, s.np, s.k) : 0.0;
    s.q[EP] = live && s.k >= 1 ? src.sin_coef(s.b, s.np, s.k) : 0.0;
}

// degrees per LDS stage of a point kernel with C components and EP epochs: 64, or 32 where 64 would take more than 24 KB (3 x 16: 25 KB
// for 32 degrees with a and b; 6 x 4: 24 KB for 64; 6 workgroups per CU either way; 1 x 16: 16 KB for 64, 1 x 1: 1 KB, two doubles per
// degree, which the double2 copies of the staging still cover exactly)
constexpr int stage_degrees(int C, int EP) { return 64 * 2 * C * EP * 8 > (24 << 10) ? 32 : 64; }

// The values of one point and field: C = 1 V, C = 3 g [3], C = 6 (xx, xy, xz, yy, yz, zz) T [3][3], each off-diagonal value twice.
template <int C>
__device__ inline void store_values(double* o, const double (&v)[C]) {
    if constexpr (C == 6) {
        o[0] = v[0];
        o[1] = v[1];
        o[2] = v[2];
        o[3] = v[1];
        o[4] = v[3];
        o[5] = v[4];
        o[6] = v[2];
        o[7] = v[4];
        o[8] = v[5];
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) o[c] = v[c];
    }
}

// 256 lanes = 256 points x EP epochs (grid.y = pass), C components each.  Per order k the 2 C coefficients of every epoch are staged in
// LDS in chunks of kDegrees degrees, together with the recursion factors a, b of degree Nq; the degree loop reads them as LDS
// broadcasts, so any degree fits.  The recursion itself is SolidColumn<kDirect> (solid.h).  C = 1 writes V [b][pt]; C = 3 writes
// g [b][pt][3]; C = 6 (xx, xy, xz, yy, yz, zz) writes T [b][pt][3][3], each off-diagonal value twice.
template <int C, int EP, int kDegrees, bool kDirect>
__global__ __launch_bounds__(256) void solid_points_kernel(int Nq, int npts, int B, const double* __restrict__ xyz, long long xyz_pass_stride,
                                                           const double2* __restrict__ ab, const double* __restrict__ Q, double R, double scale,
                                                           double* __restrict__ out) {
    constexpr int kStride = 2 * C * EP;                              // doubles per (n', k) in Q and in the stage
    __shared__ __attribute__((aligned(16))) double stage[kDegrees * kStride];
    __shared__ double2 abs_[kDegrees];
    const int tid = threadIdx.x;
    const int pt = blockIdx.x * 256 + tid;
    const int pass = blockIdx.y;
    const bool ok = pt < npts;
    SolidColumn<kDirect> col;
    col.start(xyz + pass * xyz_pass_stride + (size_t)(ok ? pt : 0) * 3, R);
    const double* Qp = Q + (size_t)pass * packed_count(Nq) * kStride;
    double acc[C][EP];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int e = 0; e < EP; ++e) acc[c][e] = 0.0;
    for (int k = 0; k <= Nq; ++k) {
        col.order(k);
        const int off = order_offset(Nq, k);
        for (int n0 = k; n0 <= Nq; n0 += kDegrees) {
            const int cnt = min(kDegrees, Nq + 1 - n0);
            __syncthreads();                                         // the previous chunk has been consumed
            {
                const double2* src = reinterpret_cast<const double2*>(Qp + (size_t)(off + n0 - k) * kStride);
                double2* dst = reinterpret_cast<double2*>(stage);
                for (int i = tid; i < cnt * kStride / 2; i += 256) dst[i] = src[i];
                for (int i = tid; i < cnt; i += 256) abs_[i] = ab[off + n0 - k + i];
            }
            __syncthreads();
            for (int j = 0; j < cnt; ++j) {
                double yc, ys;
                col.degree(n0 + j, k, abs_ + j, yc, ys);
                const double* q = stage + j * kStride;
#pragma unroll
                for (int c = 0; c < C; ++c)
#pragma unroll
                    for (int e = 0; e < EP; ++e) {
                        acc[c][e] = fma(yc, q[(2 * c) * EP + e], acc[c][e]);
                        acc[c][e] = fma(ys, q[(2 * c + 1) * EP + e], acc[c][e]);
                    }
            }
        }
    }
    if (ok) {
#pragma unroll
        for (int e = 0; e < EP; ++e) {
            const int b = pass * EP + e;
            if (b < B) {
                double v[C];
#pragma unroll
                for (int c = 0; c < C; ++c) v[c] = acc[c][e] * scale;
                store_values<C>(out + ((size_t)b * npts + pt) * (C == 6 ? 9 : C), v);
            }
        }
    }
}

// A workgroup of solid_points_at_kernel: `count` <= 256 consecutive points from `begin` whose window starts at field `field` of Q.
struct AtTile {
    int field, begin, count;
};

// Every point at its own fields: out[i] = scale sum_{j < W} weights[i][j] S(field first_i + j, x_i), S the unscaled sums of
// solid_points_kernel.  One workgroup per tile, one lane per point.  Q [field][packed (n', k) of degree Nq][2 C] holds every field
// once; the window is swept in chunks of E fields: per order and kDegrees degrees the chunk's numbers are staged in LDS, transposed to
// the [2 C][E] of solid_points_kernel's stage, and the degree loop is that kernel's, so acc[c][e] is bitwise its value of the field.
// Slots past W are staged as zeros and weighted with zero.  After a sweep the E weights of the point are loaded and res[c] takes
// one fma per field, fields ascending from 0.0; the column restarts for the next chunk.  One plain store per value, after the
// product with scale.
template <int C, int E, int kDegrees, bool kDirect>
__global__ __launch_bounds__(256) void solid_points_at_kernel(int Nq, int W, const AtTile* __restrict__ tiles, const double* __restrict__ xyz,
                                                              const double2* __restrict__ ab, const double* __restrict__ Q,
                                                              const double* __restrict__ weights, double R, double scale, double* __restrict__ out) {
    constexpr int kNumbers = 2 * C;                                  // doubles per (n', k) and field in Q
    constexpr int kStride = kNumbers * E;                            // doubles per (n', k) in the stage
    __shared__ __attribute__((aligned(16))) double stage[kDegrees * kStride];
    __shared__ double2 abs_[kDegrees];
    const int tid = threadIdx.x;
    const AtTile tile = tiles[blockIdx.x];
    const bool ok = tid < tile.count;
    const size_t pt = (size_t)tile.begin + (ok ? tid : 0);
    const size_t field_stride = (size_t)packed_count(Nq) * kNumbers;
    double res[C];
#pragma unroll
    for (int c = 0; c < C; ++c) res[c] = 0.0;
    for (int j0 = 0; j0 < W; j0 += E) {
        const int live = min(E, W - j0);                             // fields of this chunk inside the window
        const double* Qw = Q + (size_t)(tile.field + j0) * field_stride;
        SolidColumn<kDirect> col;
        col.start(xyz + pt * 3, R);
        double acc[C][E];
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int e = 0; e < E; ++e) acc[c][e] = 0.0;
        for (int k = 0; k <= Nq; ++k) {
            col.order(k);
            const int off = order_offset(Nq, k);
            for (int n0 = k; n0 <= Nq; n0 += kDegrees) {
                const int cnt = min(kDegrees, Nq + 1 - n0);
                __syncthreads();                                     // the previous chunk has been consumed
                {
                    // lane -> (field e fastest, number r): the stage is written in order, a field is read in runs of 256 / E doubles
                    const double* src = Qw + (size_t)(off + n0 - k) * kNumbers;
                    for (int i = tid; i < cnt * kStride; i += 256) {
                        const int e = i % E, r = i / E;
                        stage[(r / kNumbers) * kStride + (r % kNumbers) * E + e] = e < live ? src[(size_t)e * field_stride + r] : 0.0;
                    }
                    for (int i = tid; i < cnt; i += 256) abs_[i] = ab[off + n0 - k + i];
                }
                __syncthreads();
                for (int j = 0; j < cnt; ++j) {
                    double yc, ys;
                    col.degree(n0 + j, k, abs_ + j, yc, ys);
                    const double* q = stage + j * kStride;
#pragma unroll
                    for (int c = 0; c < C; ++c)
#pragma unroll
                        for (int e = 0; e < E; ++e) {
                            acc[c][e] = fma(yc, q[(2 * c) * E + e], acc[c][e]);
                            acc[c][e] = fma(ys, q[(2 * c + 1) * E + e], acc[c][e]);
                        }
                }
            }
        }
        if (ok) {
            const double* w = weights + pt * W + j0;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const double we = e < live ? w[e] : 0.0;
#pragma unroll
                for (int c = 0; c < C; ++c) res[c] = fma(we, acc[c][e], res[c]);
            }
        }
    }
    if (ok) {
        double v[C];
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = res[c] * scale;
        store_values<C>(out + pt * (C == 6 ? 9 : C), v);
    }
}

// The three functionals.  kOffset: Nq = N + kOffset; kComponents: C of the kernels (2 C numbers per (n', k) in Q); kValues: values per
// point and epoch; kMaxEP: epochs per pass with shared points are the smallest of 1, 4, 16 that holds all epochs, kMaxEP at most.
struct Acceleration {
    static constexpr int kOffset = 1, kComponents = 3, kValues = 3, kMaxEP = 16;
    static constexpr bool kDirect = false;                           // the reference's s = sqrt(1 - t^2): its consumers depend on it
    static constexpr bool kCheckQ = false;
    static constexpr auto kCombine = acceleration_combine_kernel;
    static constexpr const char* kName = "shg_acceleration_points";             // of the out-of-memory message, both layouts
    static double scale(double GM, double R) { return GM / (2.0 * R * R); }
};

struct Potential {
    // EP = 16 is 16 accumulators: 118 VGPRs, no spills, 4 waves per SIMD, a 64-degree stage of 17 KB.  EP = 32 also compiles without
    // spills (151 VGPRs) but falls to 3 waves and a 32-degree stage (twice the barriers) to halve a recursion that is already a
    // sixteenth of the loop: 16 stays
    static constexpr int kOffset = 0, kComponents = 1, kValues = 1, kMaxEP = 16;
    static constexpr bool kDirect = false;                           // the reference's colatitude form, as the acceleration uses
    static constexpr bool kCheckQ = false;
    static constexpr auto kCombine = potential_combine_kernel;
    static constexpr const char* kName = "shg_potential_points";
    static double scale(double GM, double R) { return GM / R; }
};

struct Gradients {
    // 12 EP accumulators: EP = 4 already holds 48 doubles, EP = 8 would spill or fall to one wave per SIMD
    static constexpr int kOffset = 2, kComponents = 6, kValues = 9, kMaxEP = 4;
    static constexpr bool kDirect = true;
    static constexpr bool kCheckQ = true;                            // the point kernel indexes one pass of Q with int
    static constexpr auto kCombine = gradients_combine_kernel;
    static constexpr const char* kName = "shg_gravitational_gradients_points";
    static double scale(double GM, double R) { return GM / (4.0 * R * R * R); }
};

}  // namespace shg

using namespace shg;

template <class F>
static int solid_points(int N, const double* xyz, int M, int layout, CoefSource src, double GM, double R, double* out, hipStream_t stream) {
    constexpr int C = F::kComponents;
    const int Nq = N + F::kOffset, B = src.B;
    // epochs per pass: per-epoch points take one epoch per pass (each pass has its own points)
    const int EP = layout == SHG_POINTS_PER_EPOCH ? 1 : std::min(B <= 1 ? 1 : B <= 4 ? 4 : 16, F::kMaxEP);
    const int passes = ceil_div(B, EP);
    const long long per_pass = (long long)packed_count(Nq) * 2 * C * EP;      // doubles of Q per pass
    // passes per group: Q of a group stays under 256 MB (and under 65535 passes per launch)
    const int group = (int)std::max<long long>(1, std::min<long long>({(long long)passes, (256LL << 20) / 8 / per_pass, 65535LL}));
    const double scale = F::scale(GM, R);
    {
        Workspace ws = Workspace::plain(stream);
        double2* ab;
        double* Q;
        if (int rc = upload_solid_factors(F::kName, ws, Nq, stream, ab)) return rc;
        if (!ws.alloc(Q, (size_t)group * per_pass)) return fail(SHG_ERR_NOMEM, "%s: workspace allocation failed", F::kName);
        for (int p0 = 0; p0 < passes; p0 += group) {
            const int np = std::min(group, passes - p0);
            const long long threads = (long long)packed_count(Nq) * EP * np;
            hipLaunchKernelGGL(F::kCombine, dim3((unsigned)ceil_div64(threads, 256)), dim3(256), 0, stream, src, EP, p0 * EP, np, Q);
            const long long stride = layout == SHG_POINTS_PER_EPOCH ? 3LL * M : 0;
            const double* x0 = xyz + (size_t)p0 * stride;
            double* o0 = out + (size_t)p0 * EP * M * F::kValues;
            const int Bg = std::min(B - p0 * EP, np * EP);
            const dim3 grid(ceil_div(M, 256), np);
            auto launch = [&](auto ep) {
                constexpr int kEP = decltype(ep)::value;
                hipLaunchKernelGGL((solid_points_kernel<C, kEP, stage_degrees(C, kEP), F::kDirect>), grid, dim3(256), 0, stream, Nq, M, Bg, x0, stride, ab,
                                   Q, R, scale, o0);
            };
            if (EP == 1)
                launch(std::integral_constant<int, 1>());
            else if (EP == 4)
                launch(std::integral_constant<int, 4>());
            else if constexpr (F::kMaxEP == 16)
                launch(std::integral_constant<int, 16>());
            SHG_HIP(hipGetLastError());
        }
    }
    SHG_HIP(hipGetLastError());
    return SHG_OK;
}

// Arguments are checked before the first HIP call (the CPU tests call these without a device).
template <class F>
static int check_points(const char* fn, int N, const double* xyz, int M, int layout, const void* coef, int B, double GM, double R, double* out) {
    SHG_REQUIRE(N >= 0 && M >= 0 && B >= 0, "%s: negative size (N %d, M %d, B %d)", fn, N, M, B);
    SHG_REQUIRE(layout == SHG_POINTS_SHARED || layout == SHG_POINTS_PER_EPOCH, "%s: layout %d, expected 0 (shared points) or 1 (points per epoch)", fn,
                layout);
    SHG_REQUIRE(std::isfinite(GM) && std::isfinite(R) && R > 0.0, "%s: GM and R must be finite and R positive (GM %g, R %g)", fn, GM, R);
    const long long values = (long long)F::kValues * M * B;
    SHG_REQUIRE(values <= (1LL << 40), "%s: output of %lld values is too large", fn, values);
    if constexpr (F::kCheckQ) {
        const long long q_pass = (long long)(N + F::kOffset + 1) * (N + F::kOffset + 2) / 2 * 2 * F::kComponents * F::kMaxEP;
        SHG_REQUIRE(q_pass <= INT_MAX, "%s: degree %d is too large (a pass of Q holds %lld values)", fn, N, q_pass);
    }
    if (M > 0 && B > 0) SHG_REQUIRE(xyz && coef && out, "%s: NULL pointer", fn);
    return SHG_OK;
}

// An entry point behind its checks.  The reference layout has no padding (its source says Bpad = B), so only a series can fail the
// Bpad check.
template <class F>
static int points_entry(const char* fn, const double* xyz, int M, int layout, CoefSource src, double GM, double R, double* out, void* stream) {
    if (int rc = check_points<F>(fn, src.N, xyz, M, layout, src.om ? src.om : src.anm, src.B, GM, R, out)) return rc;
    SHG_REQUIRE(src.Bpad >= src.B, "%s: Bpad %d below B %d", fn, src.Bpad, src.B);
    if (M == 0 || src.B == 0) return SHG_OK;
    return solid_points<F>(src.N, xyz, M, layout, src, GM, R, out, (hipStream_t)stream);
}

extern "C" int shg_acceleration_points(int N, const double* xyz, int M, int layout, const double* anm, int B, double GM, double R, double* g,
                                       void* stream) {
    return points_entry<Acceleration>("shg_acceleration_points", xyz, M, layout, CoefSource{anm, nullptr, N, B, B}, GM, R, g, stream);
}

extern "C" int shg_acceleration_points_om(int N, const double* xyz, int M, int layout, const double* om, int B, int Bpad, double GM, double R, double* g,
                                          void* stream) {
    return points_entry<Acceleration>("shg_acceleration_points_om", xyz, M, layout, CoefSource{nullptr, om, N, B, Bpad}, GM, R, g, stream);
}

extern "C" int shg_gravitational_gradients_points(int N, const double* xyz, int M, int layout, const double* anm, int B, double GM, double R, double* T,
                                                  void* stream) {
    return points_entry<Gradients>("shg_gravitational_gradients_points", xyz, M, layout, CoefSource{anm, nullptr, N, B, B}, GM, R, T, stream);
}

extern "C" int shg_gravitational_gradients_points_om(int N, const double* xyz, int M, int layout, const double* om, int B, int Bpad, double GM, double R,
                                                     double* T, void* stream) {
    return points_entry<Gradients>("shg_gravitational_gradients_points_om", xyz, M, layout, CoefSource{nullptr, om, N, B, Bpad}, GM, R, T, stream);
}

extern "C" int shg_potential_points(int N, const double* xyz, int M, int layout, const double* anm, int B, double GM, double R, double* V, void* stream) {
    return points_entry<Potential>("shg_potential_points", xyz, M, layout, CoefSource{anm, nullptr, N, B, B}, GM, R, V, stream);
}

extern "C" int shg_potential_points_om(int N, const double* xyz, int M, int layout, const double* om, int B, int Bpad, double GM, double R, double* V,
                                       void* stream) {
    return points_entry<Potential>("shg_potential_points_om", xyz, M, layout, CoefSource{nullptr, om, N, B, Bpad}, GM, R, V, stream);
}

// ---- every point at its own fields (shg_*_points_at): DESIGN.md section 4.22

static std::atomic<long long> g_points_at_limit{0};                 // bytes of Q per launch group; 0: the default
constexpr long long kPointsAtDefaultLimit = 256LL << 20;

extern "C" int shg_points_at_set_workspace_limit(long long bytes) {
    SHG_REQUIRE(bytes >= 0, "shg_points_at_set_workspace_limit: negative limit %lld", bytes);
    g_points_at_limit.store(bytes);
    return SHG_OK;
}

struct PointsAtArgs {
    const double* xyz;
    int M;
    const int *run_first, *run_begin;
    int runs;
    const double* weights;
    int W;
    double GM, R;
    double* out;
};

template <class F>
static long long points_at_field_bytes(int N) {                      // Q of one field
    return (long long)(N + F::kOffset + 1) * (N + F::kOffset + 2) / 2 * 2 * F::kComponents * 8;
}

// Arguments are checked before the first HIP call, the run tables in full: no table content reaches the kernel unchecked.
template <class F>
static int check_points_at(const char* fn, const CoefSource& src, const PointsAtArgs& a) {
    const int N = src.N, B = src.B, M = a.M, W = a.W;
    SHG_REQUIRE(N >= 0 && M >= 0 && B >= 0, "%s: negative size (N %d, M %d, B %d)", fn, N, M, B);
    SHG_REQUIRE(W >= 1 && W <= 16, "%s: window of %d fields, expected 1 .. 16", fn, W);
    SHG_REQUIRE(B >= W, "%s: %d fields, fewer than the window of %d", fn, B, W);
    SHG_REQUIRE(a.runs >= 0, "%s: negative number of runs %d", fn, a.runs);
    SHG_REQUIRE(src.Bpad >= B, "%s: Bpad %d below B %d", fn, src.Bpad, B);
    SHG_REQUIRE(std::isfinite(a.GM) && std::isfinite(a.R) && a.R > 0.0, "%s: GM and R must be finite and R positive (GM %g, R %g)", fn, a.GM, a.R);
    const long long values = (long long)F::kValues * M;
    SHG_REQUIRE(values <= (1LL << 40), "%s: output of %lld values is too large", fn, values);
    if constexpr (F::kCheckQ) {
        const long long q_pass = points_at_field_bytes<F>(N) / 8 * F::kMaxEP;
        SHG_REQUIRE(q_pass <= INT_MAX, "%s: degree %d is too large (a pass of Q holds %lld values)", fn, N, q_pass);
    }
    if (M == 0) return SHG_OK;
    SHG_REQUIRE(a.xyz && (src.om ? src.om : src.anm) && a.run_first && a.run_begin && a.weights && a.out, "%s: NULL pointer", fn);
    SHG_REQUIRE(a.run_begin[0] == 0, "%s: run_begin[0] is %d, not 0", fn, a.run_begin[0]);
    for (int r = 0; r < a.runs; ++r) {
        SHG_REQUIRE(a.run_begin[r + 1] > a.run_begin[r] && a.run_begin[r + 1] <= M, "%s: run_begin must increase strictly up to M %d (run %d: %d, %d)", fn,
                    M, r, a.run_begin[r], a.run_begin[r + 1]);
        SHG_REQUIRE(a.run_first[r] >= 0 && a.run_first[r] <= B - W, "%s: run %d starts at field %d, outside 0 .. B - W = %d", fn, r, a.run_first[r],
                    B - W);
    }
    SHG_REQUIRE(a.run_begin[a.runs] == M, "%s: the runs end at point %d, not at M %d", fn, a.run_begin[a.runs], M);
    return SHG_OK;
}

template <class F>
static int solid_points_at(const char* fn, const CoefSource& src, const PointsAtArgs& a, long long limit, hipStream_t stream) {
    constexpr int C = F::kComponents;
    const int Nq = src.N + F::kOffset, B = src.B, W = a.W;
    const long long per_field = points_at_field_bytes<F>(src.N) / 8;           // doubles of Q per field
    // fields per launch group: Q of a group stays under the limit; groups overlap by W - 1 fields, a run goes to the group
    // first / step, whose fields group * step .. group * step + G - 1 hold its window
    const int G = (int)std::min<long long>(B, limit / 8 / per_field);
    const int step = G - W + 1;
    const int groups = (B - W) / step + 1;
    std::vector<long long> tile0(groups + 1, 0);                               // first tile of every group
    for (int r = 0; r < a.runs; ++r) tile0[a.run_first[r] / step + 1] += ceil_div(a.run_begin[r + 1] - a.run_begin[r], 256);
    for (int g = 0; g < groups; ++g) tile0[g + 1] += tile0[g];
    SHG_REQUIRE(tile0[groups] <= INT_MAX, "%s: %lld tiles are too many", fn, tile0[groups]);
    std::vector<AtTile> tiles((size_t)tile0[groups]);
    {
        std::vector<long long> next(tile0.begin(), tile0.end() - 1);
        for (int r = 0; r < a.runs; ++r) {
            const int g = a.run_first[r] / step;
            for (int p = a.run_begin[r]; p < a.run_begin[r + 1]; p += 256)
                tiles[(size_t)next[g]++] = AtTile{a.run_first[r] - g * step, p, std::min(256, a.run_begin[r + 1] - p)};
        }
    }
    // fields per sweep: a sweep of 16 (2 waves per SIMD) costs as much as four sweeps of 4, so it pays from 13 fields on
    // (profiles/points_at_time.txt)
    const int E = W <= 2 ? 2 : W <= 12 ? 4 : std::min(16, F::kMaxEP);
    const double scale = F::scale(a.GM, a.R);
    {
        Workspace ws = Workspace::plain(stream);
        double2* ab;
        double* Q;
        AtTile* table;
        if (int rc = upload_solid_factors(fn, ws, Nq, stream, ab)) return rc;
        if (!ws.alloc(Q, (size_t)G * per_field, table, tiles.size())) return fail(SHG_ERR_NOMEM, "%s: workspace allocation failed", fn);
        SHG_HIP(hipMemcpyAsync(table, tiles.data(), tiles.size() * sizeof(AtTile), hipMemcpyHostToDevice, stream));
        SHG_HIP(hipStreamSynchronize(stream));                       // as upload_solid_factors: the host table goes out of scope
        for (int g = 0; g < groups; ++g) {
            const int count = (int)(tile0[g + 1] - tile0[g]);
            if (count == 0) continue;
            const int fields = std::min(G, B - g * step);
            const long long threads = (long long)packed_count(Nq) * fields;
            hipLaunchKernelGGL(F::kCombine, dim3((unsigned)ceil_div64(threads, 256)), dim3(256), 0, stream, src, 1, g * step, fields, Q);
            auto launch = [&](auto e) {
                constexpr int kE = decltype(e)::value;
                hipLaunchKernelGGL((solid_points_at_kernel<C, kE, stage_degrees(C, kE), F::kDirect>), dim3(count), dim3(256), 0, stream, Nq, W,
                                   table + tile0[g], a.xyz, ab, Q, a.weights, a.R, scale, a.out);
            };
            if (E == 2)
                launch(std::integral_constant<int, 2>());
            else if (E == 4)
                launch(std::integral_constant<int, 4>());
            else if constexpr (F::kMaxEP == 16)
                launch(std::integral_constant<int, 16>());
            SHG_HIP(hipGetLastError());
        }
    }
    SHG_HIP(hipGetLastError());
    return SHG_OK;
}

template <class F>
static int points_at_entry(const char* fn, CoefSource src, const PointsAtArgs& a, void* stream) {
    if (int rc = check_points_at<F>(fn, src, a)) return rc;
    if (a.M == 0) return SHG_OK;
    long long limit = g_points_at_limit.load();
    if (limit == 0) limit = kPointsAtDefaultLimit;
    const long long window = points_at_field_bytes<F>(src.N) * a.W;
    SHG_REQUIRE(limit >= window, "%s: the workspace limit of %lld bytes is below one window of %d fields (%lld bytes)", fn, limit, a.W, window);
    return solid_points_at<F>(fn, src, a, limit, (hipStream_t)stream);
}

#define SHG_POINTS_AT(name, F, value)                                                                                                          \
    extern "C" int name(int N, const double* xyz, int M, const double* anm, int B, const int* run_first, const int* run_begin, int runs,        \
                        const double* weights, int W, double GM, double R, double* value, void* stream) {                                       \
        return points_at_entry<F>(#name, CoefSource{anm, nullptr, N, B, B}, PointsAtArgs{xyz, M, run_first, run_begin, runs, weights, W, GM, R, value}, \
                                  stream);                                                                                                     \
    }                                                                                                                                          \
    extern "C" int name##_om(int N, const double* xyz, int M, const double* om, int B, int Bpad, const int* run_first, const int* run_begin,    \
                             int runs, const double* weights, int W, double GM, double R, double* value, void* stream) {                        \
        return points_at_entry<F>(#name "_om", CoefSource{nullptr, om, N, B, Bpad}, PointsAtArgs{xyz, M, run_first, run_begin, runs, weights, W, GM, R, value}, \
                                  stream);                                                                                                     \
    }
SHG_POINTS_AT(shg_acceleration_points_at, Acceleration, g)
SHG_POINTS_AT(shg_potential_points_at, Potential, V)
SHG_POINTS_AT(shg_gravitational_gradients_points_at, Gradients, T)
#undef SHG_POINTS_AT

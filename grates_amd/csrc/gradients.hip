// Gravitational gradient tensor T = d^2 V / dx_i dx_j at arbitrary points (the Jacobian of the acceleration of acceleration.hip).
//
// acceleration.hip writes each Cartesian component of g as a point synthesis of degree N + 1 whose coefficients are D_c(C, S), where
// D_c (c = x, y, z) reads the orders k + 1, k - 1, k of degree n and writes (n + 1, k):
//   x: A = f- C- - f+ C+    B = f- S- - f+ S+        y: A = f- S- + f+ S+    B = -(f- C- + f+ C+)        z: A = -2 f0 C0    B = -2 f0 S0
// (f- of order 1 and f+ of order 0 carry the extra sqrt(2)).  D works on any solid-harmonic coefficient set, so applying it to
// (A^c, B^c) differentiates once more: with (A^cd, B^cd) = D_d(D_c(C, S)) of degree N + 2,
//   T_cd = dg_c / dx_d = GM / (4 R^3) sum_{n'', k} (R/r)^(n''+1) P_{n''k} (cos(k lon) A^cd_{n''k} + sin(k lon) B^cd_{n''k}).
// gradients_combine_kernel forms the twelve numbers of xx, xy, xz, yy, yz, zz per (n'', k) and epoch once per call (the composition
// fused: the three first-derivative sets of degree n'' - 1 it needs are formed in registers); gradients_points_kernel runs one column
// recursion per point and (n'', k) for the six components of every epoch of a pass.  xx, yy and zz each come from their own
// combination: the trace is a check, not an identity.
#include "common.h"

#include <climits>
#include <cmath>

namespace shg {

// Q [pass][packed (n'', k) of degree N + 2][12][EP]: A/B of xx, xy, xz, yy, yz, zz of EP consecutive epochs.
// Coefficient source: the reference layout anm [B][N+1][N+1] (om == nullptr) or an order-major series om [(N+1)^2][Bpad].
struct GradientSource {
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
    const double dn = np - 1;
    const double base = sqrt((2.0 * dn + 1.0) / (2.0 * dn + 3.0));
    if (np >= k + 2) {                                               // minus term of order m = k + 1
        const double m = k + 1;
        t.fm = sqrt((dn - m + 1.0) * (dn - m + 2.0)) * base;
        if (k == 0) t.fm *= sqrt(2.0);
    }
    if (k >= 1) {                                                    // plus term of order m = k - 1
        const double m = k - 1;
        t.fp = sqrt((dn + m + 1.0) * (dn + m + 2.0)) * base;
        if (k == 1) t.fp *= sqrt(2.0);
    }
    if (np >= k + 1) {                                               // zero term of order m = k
        const double m = k;
        t.f0 = sqrt((dn - m + 1.0) * (dn + m + 1.0)) * base;
    }
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
__device__ inline void first_derivative(const GradientSource& src, int b, int n1, int k1, double F[3][2]) {
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

// one thread per (n'', k, epoch slot) of `passes` passes of EP epochs starting at epoch b_first; epochs past B get zeros
__global__ __launch_bounds__(256) void gradients_combine_kernel(GradientSource src, int EP, int b_first, int passes, double* __restrict__ Q) {
    const int N2 = src.N + 2;
    const long long per_pass = (long long)packed_count(N2) * EP;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= per_pass * passes) return;
    const int pass = (int)(idx / per_pass);
    const long long rem = idx - pass * per_pass;
    const int e = (int)(rem % EP);
    int p = (int)(rem / EP);
    int k = 0;                                                       // packed index p -> (k, n''): order_offset(N2, k) <= p
    while (k < N2 && order_offset(N2, k + 1) <= p) ++k;
    const int np = k + (p - order_offset(N2, k));
    const int b = b_first + pass * EP + e;
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
    double* q = Q + (size_t)pass * per_pass * 12 + (size_t)p * 12 * EP + e;
#pragma unroll
    for (int j = 0; j < 12; ++j) q[j * EP] = out[j];
}

template <int EP>
struct GradientShape {
    static constexpr int kDegrees = 64;                              // degrees per LDS stage: 24 KB at 4 epochs (6 workgroups per CU)
    static constexpr int kStride = 12 * EP;                          // doubles per (n'', k) in Q and in the stage
};

// 256 lanes = 256 points x EP epochs (grid.y = pass).  The column recursion of acceleration_points_kernel, one degree higher, with six
// components per epoch: per order k the twelve coefficients of every epoch are staged in LDS in chunks of kDegrees degrees, with the
// recursion factors a, b of degree N + 2, and read as LDS broadcasts.  r and the longitude come from xyz as grid.cartesian2spherical
// computes them, the colatitude as t = z / r, s = rho / r; (R/r)^(n''+1) is carried along the degree loop.  T [b][pt][3][3] is
// written directly, each off-diagonal value twice.
template <int EP>
__global__ __launch_bounds__(256) void gradients_points_kernel(int N2, int npts, int B, const double* __restrict__ xyz, long long xyz_pass_stride,
                                                               const double* __restrict__ ab, const double* __restrict__ Q, double R, double scale,
                                                               double* __restrict__ T) {
    using S = GradientShape<EP>;
    __shared__ __attribute__((aligned(16))) double stage[S::kDegrees * S::kStride];
    __shared__ __attribute__((aligned(16))) double abs_[S::kDegrees * 2];
    const int tid = threadIdx.x;
    const int pt = blockIdx.x * 256 + tid;
    const int pass = blockIdx.y;
    const bool ok = pt < npts;
    const double* xp = xyz + pass * xyz_pass_stride + (size_t)(ok ? pt : 0) * 3;
    const double x = xp[0], y = xp[1], z = xp[2];
    const double r = sqrt((x * x + y * y) + z * z);                  // np.sum over axis 1: ((x^2 + y^2) + z^2)
    const double lam = atan2(y, x);
    const double u = R / r;
    // cos and sin of the colatitude straight from xyz: s = sqrt(1 - t^2), the acceleration's (and the reference's) form, is 0 within
    // 1.5e-8 rad of the axis, where T_xz = 3 GM x z / r^5 is still up to 2e-8 of max|T|
    const double t = z / r;
    const double s = sqrt(x * x + y * y) / r;
    const double* Qp = Q + (size_t)pass * packed_count(N2) * S::kStride;
    double acc[6][EP];
#pragma unroll
    for (int c = 0; c < 6; ++c)
#pragma unroll
        for (int e = 0; e < EP; ++e) acc[c][e] = 0.0;
    double pmm = 1.0, rk = u;                                        // rk = (R/r)^(k+1)
    for (int k = 0; k <= N2; ++k) {
        if (k == 1)
            pmm = sqrt(3.0) * s;
        else if (k >= 2)
            pmm = sqrt((2.0 * k + 1.0) / (2.0 * k)) * s * pmm;
        if (k >= 1) rk *= u;
        double sk, ck;
        sincos((double)k * lam, &sk, &ck);
        double p1 = pmm, p2 = 0.0, rad = rk;
        const int off = order_offset(N2, k);
        for (int n0 = k; n0 <= N2; n0 += S::kDegrees) {
            const int cnt = min(S::kDegrees, N2 + 1 - n0);
            __syncthreads();                                         // the previous chunk has been consumed
            {
                const double2* src = reinterpret_cast<const double2*>(Qp + (size_t)(off + n0 - k) * S::kStride);
                double2* dst = reinterpret_cast<double2*>(stage);
                for (int i = tid; i < cnt * S::kStride / 2; i += 256) dst[i] = src[i];
                const double2* sab = reinterpret_cast<const double2*>(ab + (size_t)(off + n0 - k) * 2);
                double2* dab = reinterpret_cast<double2*>(abs_);
                for (int i = tid; i < cnt; i += 256) dab[i] = sab[i];
            }
            __syncthreads();
            for (int j = 0; j < cnt; ++j) {
                const int n = n0 + j;
                if (n > k) {
                    const double p = (abs_[2 * j] * t) * p1 - abs_[2 * j + 1] * p2;
                    p2 = p1;
                    p1 = p;
                }
                const double pk = p1 * rad;
                rad *= u;
                const double yc = pk * ck, ys = pk * sk;
                const double* q = stage + j * S::kStride;
#pragma unroll
                for (int c = 0; c < 6; ++c)
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
                const double xx = acc[0][e] * scale, xy = acc[1][e] * scale, xz = acc[2][e] * scale;
                const double yy = acc[3][e] * scale, yz = acc[4][e] * scale, zz = acc[5][e] * scale;
                double* o = T + ((size_t)b * npts + pt) * 9;
                o[0] = xx;
                o[1] = xy;
                o[2] = xz;
                o[3] = xy;
                o[4] = yy;
                o[5] = yz;
                o[6] = xz;
                o[7] = yz;
                o[8] = zz;
            }
        }
    }
}

}  // namespace shg

using namespace shg;

static int gradients_points(int N, const double* xyz, int M, int layout, GradientSource src, double GM, double R, double* T, hipStream_t stream) {
    const int N2 = N + 2, B = src.B;
    // epochs per pass: per-epoch points take one epoch per pass (each pass has its own points); shared points 1 for a single field,
    // 4 otherwise (12 EP accumulators: EP = 4 already holds 48 doubles, EP = 8 would spill or fall to one wave per SIMD)
    const int EP = layout == SHG_POINTS_PER_EPOCH ? 1 : (B <= 1 ? 1 : 4);
    const int passes = ceil_div(B, EP);
    const long long per_pass = (long long)packed_count(N2) * 12 * EP;         // doubles of Q per pass
    // passes per group: Q of a group stays under 256 MB (and under 65535 passes per launch)
    const int group = (int)std::max<long long>(1, std::min<long long>({(long long)passes, (256LL << 20) / 8 / per_pass, 65535LL}));
    const double scale = GM / (4.0 * R * R * R);
    {
        Workspace ws = Workspace::plain(stream);
        double *ab, *Q;
        if (!ws.alloc(ab, (size_t)packed_count(N2) * 2, Q, (size_t)group * per_pass))
            return fail(SHG_ERR_NOMEM, "shg_gravitational_gradients_points: workspace allocation failed");
        {   // recursion factors of degree N + 2, a and b of one (n'', k) side by side (staged together)
            std::vector<double> a, b, h(2 * (size_t)packed_count(N2));
            recursion_tables(N2, a, b);
            for (size_t i = 0; i < a.size(); ++i) {
                h[2 * i] = a[i];
                h[2 * i + 1] = b[i];
            }
            SHG_HIP(hipMemcpyAsync(ab, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, stream));
            SHG_HIP(hipStreamSynchronize(stream));
        }
        for (int p0 = 0; p0 < passes; p0 += group) {
            const int np = std::min(group, passes - p0);
            const long long threads = (long long)packed_count(N2) * EP * np;
            hipLaunchKernelGGL(gradients_combine_kernel, dim3((unsigned)ceil_div64(threads, 256)), dim3(256), 0, stream, src, EP, p0 * EP, np, Q);
            const long long stride = layout == SHG_POINTS_PER_EPOCH ? 3LL * M : 0;
            const double* x0 = xyz + (size_t)p0 * stride;
            double* T0 = T + (size_t)p0 * EP * M * 9;
            const int Bg = std::min(B - p0 * EP, np * EP);
            const dim3 grid(ceil_div(M, 256), np);
            if (EP == 1)
                hipLaunchKernelGGL(gradients_points_kernel<1>, grid, dim3(256), 0, stream, N2, M, Bg, x0, stride, ab, Q, R, scale, T0);
            else
                hipLaunchKernelGGL(gradients_points_kernel<4>, grid, dim3(256), 0, stream, N2, M, Bg, x0, stride, ab, Q, R, scale, T0);
            SHG_HIP(hipGetLastError());
        }
    }
    SHG_HIP(hipGetLastError());
    return SHG_OK;
}

// Arguments are checked before the first HIP call (the CPU tests call these without a device); the rules and messages of
// acceleration.hip's check_acceleration, plus the size of Q.
static int check_gradients(const char* fn, int N, const double* xyz, int M, int layout, const void* coef, int B, double GM, double R, double* T) {
    SHG_REQUIRE(N >= 0 && M >= 0 && B >= 0, "%s: negative size (N %d, M %d, B %d)", fn, N, M, B);
    SHG_REQUIRE(layout == SHG_POINTS_SHARED || layout == SHG_POINTS_PER_EPOCH, "%s: layout %d, expected 0 (shared points) or 1 (points per epoch)", fn,
                layout);
    SHG_REQUIRE(std::isfinite(GM) && std::isfinite(R) && R > 0.0, "%s: GM and R must be finite and R positive (GM %g, R %g)", fn, GM, R);
    SHG_REQUIRE(9LL * M * B <= (1LL << 40), "%s: output of %lld values is too large", fn, 9LL * M * B);
    // the point kernel indexes one pass of Q (12 EP values per (n'', k) of degree N + 2) with int
    const long long q_pass = (long long)(N + 3) * (N + 4) / 2 * 12 * 4;
    SHG_REQUIRE(q_pass <= INT_MAX, "%s: degree %d is too large (a pass of Q holds %lld values)", fn, N, q_pass);
    if (M > 0 && B > 0) SHG_REQUIRE(xyz && coef && T, "%s: NULL pointer", fn);
    return SHG_OK;
}

extern "C" int shg_gravitational_gradients_points(int N, const double* xyz, int M, int layout, const double* anm, int B, double GM, double R, double* T,
                                                  void* stream) {
    if (int rc = check_gradients("shg_gravitational_gradients_points", N, xyz, M, layout, anm, B, GM, R, T)) return rc;
    if (M == 0 || B == 0) return SHG_OK;
    return gradients_points(N, xyz, M, layout, GradientSource{anm, nullptr, N, B, 0}, GM, R, T, (hipStream_t)stream);
}

extern "C" int shg_gravitational_gradients_points_om(int N, const double* xyz, int M, int layout, const double* om, int B, int Bpad, double GM, double R,
                                                     double* T, void* stream) {
    if (int rc = check_gradients("shg_gravitational_gradients_points_om", N, xyz, M, layout, om, B, GM, R, T)) return rc;
    SHG_REQUIRE(Bpad >= B, "shg_gravitational_gradients_points_om: Bpad %d below B %d", Bpad, B);
    if (M == 0 || B == 0) return SHG_OK;
    return gradients_points(N, xyz, M, layout, GradientSource{nullptr, om, N, B, Bpad}, GM, R, T, (hipStream_t)stream);
}

// Gravitational acceleration at arbitrary points (replaces grates/gravityfield.py:423-481, three per-order Legendre tables of degree
// N + 1 per point and a dgemv per component and order).
//
// The reference sums, per coefficient order m, P_{n+1,m-1} f-, P_{n+1,m} f0 and P_{n+1,m+1} f+ times (R/r)^(n+2).  Regrouped by the
// Legendre function (n', k), n' = n + 1 = 0 .. N + 1, each Cartesian component c is a point synthesis of degree N + 1:
//   g_c = GM / (2 R^2) sum_{n', k} (R/r)^(n'+1) P_{n'k} (cos(k lon) A^c_{n'k} + sin(k lon) B^c_{n'k})
// with, for n = n' - 1, (C-, S-) = (C, S)_{n,k+1} (n' >= k + 2), (C+, S+) = (C, S)_{n,k-1} (k >= 1), (C0, S0) = (C, S)_{n,k} (n' >= k + 1):
//   A^x = f- C- - f+ C+    B^x = f- S- - f+ S+    A^y = f- S- + f+ S+    B^y = -(f- C- + f+ C+)    A^z = -2 f0 C0    B^z = -2 f0 S0
// (f- of order 1 and f+ of order 0 carry the reference's extra sqrt(2)).  acceleration_combine_kernel forms these six numbers per
// (n', k) and epoch once per call; acceleration_points_kernel runs one column recursion per point and (n', k) for all three
// components and every epoch of a pass.
#include "common.h"

#include <cmath>

namespace shg {

// Q [pass][packed (n', k) of degree N + 1][6][EP]: the six coefficients A^x B^x A^y B^y A^z B^z of EP consecutive epochs.
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

// one thread per (n', k, epoch slot) of `passes` passes of EP epochs starting at epoch b_first; epochs past B get zeros
__global__ __launch_bounds__(256) void acceleration_combine_kernel(CoefSource src, int EP, int b_first, int passes, double* __restrict__ Q) {
    const int N = src.N, N1 = N + 1;
    const long long per_pass = (long long)packed_count(N1) * EP;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= per_pass * passes) return;
    const int pass = (int)(idx / per_pass);
    const long long rem = idx - pass * per_pass;
    const int e = (int)(rem % EP);
    int p = (int)(rem / EP);
    int k = 0;                                                       // packed index p -> (k, n'): order_offset(N1, k) <= p
    while (k < N1 && order_offset(N1, k + 1) <= p) ++k;
    const int np = k + (p - order_offset(N1, k));
    const int b = b_first + pass * EP + e;
    double ax = 0.0, bx = 0.0, ay = 0.0, by = 0.0, az = 0.0, bz = 0.0;
    if (b < src.B && np >= 1) {
        const int n = np - 1;
        const double dn = n;
        const double base = sqrt((2.0 * dn + 1.0) / (2.0 * dn + 3.0));
        double cm = 0.0, sm = 0.0, fm = 0.0, cp = 0.0, sp = 0.0, fp = 0.0;
        if (np >= k + 2) {                                           // minus term of order m = k + 1
            const double m = k + 1;
            fm = sqrt((dn - m + 1.0) * (dn - m + 2.0)) * base;
            if (k == 0) fm *= sqrt(2.0);
            cm = src.cos_coef(b, n, k + 1);
            sm = src.sin_coef(b, n, k + 1);
        }
        if (k >= 1) {                                                // plus term of order m = k - 1 (n >= m always holds)
            const double m = k - 1;
            fp = sqrt((dn + m + 1.0) * (dn + m + 2.0)) * base;
            if (k == 1) fp *= sqrt(2.0);
            cp = src.cos_coef(b, n, k - 1);
            sp = k >= 2 ? src.sin_coef(b, n, k - 1) : 0.0;
        }
        ax = fm * cm - fp * cp;
        bx = fm * sm - fp * sp;
        ay = fm * sm + fp * sp;
        by = -(fm * cm + fp * cp);
        if (np >= k + 1) {                                           // zero term of order m = k
            const double m = k;
            const double f0 = sqrt((dn - m + 1.0) * (dn + m + 1.0)) * base;
            az = -2.0 * (f0 * src.cos_coef(b, n, k));
            bz = k >= 1 ? -2.0 * (f0 * src.sin_coef(b, n, k)) : 0.0;
        }
    }
    double* q = Q + (size_t)pass * per_pass * 6 + (size_t)p * 6 * EP + e;
    q[0 * EP] = ax;
    q[1 * EP] = bx;
    q[2 * EP] = ay;
    q[3 * EP] = by;
    q[4 * EP] = az;
    q[5 * EP] = bz;
}

template <int EP>
struct AccelShape {
    static constexpr int kDegrees = EP >= 16 ? 32 : 64;              // degrees per LDS stage: 25 KB at 16 epochs (6 workgroups per CU)
    static constexpr int kStride = 6 * EP;                           // doubles per (n', k) in Q and in the stage
};

// 256 lanes = 256 points x EP epochs (grid.y = pass).  Per order k the six coefficients of every epoch are staged in LDS in chunks of
// kDegrees degrees, together with the recursion factors a, b; the degree loop reads them as LDS broadcasts.  (r, colatitude,
// longitude) come from xyz as grid.cartesian2spherical computes them, (R/r)^(n'+1) is carried along the degree loop.
template <int EP>
__global__ __launch_bounds__(256) void acceleration_points_kernel(int N1, int npts, int B, const double* __restrict__ xyz, long long xyz_pass_stride,
                                                                  const double* __restrict__ ab, const double* __restrict__ Q, double R, double scale,
                                                                  double* __restrict__ g) {
    using S = AccelShape<EP>;
    __shared__ __attribute__((aligned(16))) double stage[S::kDegrees * S::kStride];
    __shared__ __attribute__((aligned(16))) double abs_[S::kDegrees * 2];
    const int tid = threadIdx.x;
    const int pt = blockIdx.x * 256 + tid;
    const int pass = blockIdx.y;
    const bool ok = pt < npts;
    const double* xp = xyz + pass * xyz_pass_stride + (size_t)(ok ? pt : 0) * 3;
    const double x = xp[0], y = xp[1], z = xp[2];
    const double r = sqrt((x * x + y * y) + z * z);                  // np.sum over axis 1: ((x^2 + y^2) + z^2)
    const double th = atan2(sqrt(x * x + y * y), z);
    const double lam = atan2(y, x);
    const double u = R / r;
    const double t = cos(th);
    const double s = sqrt(1.0 - t * t);
    const double* Qp = Q + (size_t)pass * packed_count(N1) * S::kStride;
    double acc[3][EP];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int e = 0; e < EP; ++e) acc[c][e] = 0.0;
    double pmm = 1.0, rk = u;                                        // rk = (R/r)^(k+1)
    for (int k = 0; k <= N1; ++k) {
        if (k == 1)
            pmm = sqrt(3.0) * s;
        else if (k >= 2)
            pmm = sqrt((2.0 * k + 1.0) / (2.0 * k)) * s * pmm;
        if (k >= 1) rk *= u;
        double sk, ck;
        sincos((double)k * lam, &sk, &ck);
        double p1 = pmm, p2 = 0.0, rad = rk;
        const int off = order_offset(N1, k);
        for (int n0 = k; n0 <= N1; n0 += S::kDegrees) {
            const int cnt = min(S::kDegrees, N1 + 1 - n0);
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
                for (int c = 0; c < 3; ++c)
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
                double* o = g + ((size_t)b * npts + pt) * 3;
                o[0] = acc[0][e] * scale;
                o[1] = acc[1][e] * scale;
                o[2] = acc[2][e] * scale;
            }
        }
    }
}

}  // namespace shg

using namespace shg;

static int acceleration_points(int N, const double* xyz, int M, int layout, CoefSource src, double GM, double R, double* g, hipStream_t stream) {
    const int N1 = N + 1, B = src.B;
    // epochs per pass: per-epoch points take one epoch per pass (each pass has its own points); shared points the smallest of 1, 4, 16
    // that holds all epochs, 16 beyond
    const int EP = layout == SHG_POINTS_PER_EPOCH ? 1 : (B <= 1 ? 1 : B <= 4 ? 4 : 16);
    const int passes = ceil_div(B, EP);
    const long long per_pass = (long long)packed_count(N1) * 6 * EP;          // doubles of Q per pass
    // passes per group: Q of a group stays under 256 MB (and under 65535 passes per launch)
    const int group = (int)std::max<long long>(1, std::min<long long>({(long long)passes, (256LL << 20) / 8 / per_pass, 65535LL}));
    const double scale = GM / (2.0 * R * R);
    {
        Workspace ws = Workspace::plain(stream);
        double *ab, *Q;
        if (!ws.alloc(ab, (size_t)packed_count(N1) * 2, Q, (size_t)group * per_pass))
            return fail(SHG_ERR_NOMEM, "shg_acceleration_points: workspace allocation failed");
        {   // recursion factors of degree N + 1, a and b of one (n', k) side by side (staged together)
            std::vector<double> a, b, h(2 * (size_t)packed_count(N1));
            recursion_tables(N1, a, b);
            for (size_t i = 0; i < a.size(); ++i) {
                h[2 * i] = a[i];
                h[2 * i + 1] = b[i];
            }
            SHG_HIP(hipMemcpyAsync(ab, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, stream));
            SHG_HIP(hipStreamSynchronize(stream));
        }
        for (int p0 = 0; p0 < passes; p0 += group) {
            const int np = std::min(group, passes - p0);
            const long long threads = (long long)packed_count(N1) * EP * np;
            hipLaunchKernelGGL(acceleration_combine_kernel, dim3((unsigned)ceil_div64(threads, 256)), dim3(256), 0, stream, src, EP, p0 * EP, np, Q);
            const long long stride = layout == SHG_POINTS_PER_EPOCH ? 3LL * M : 0;
            const double* x0 = xyz + (size_t)p0 * stride;
            double* g0 = g + (size_t)p0 * EP * M * 3;
            const int Bg = std::min(B - p0 * EP, np * EP);
            const dim3 grid(ceil_div(M, 256), np);
            if (EP == 1)
                hipLaunchKernelGGL(acceleration_points_kernel<1>, grid, dim3(256), 0, stream, N1, M, Bg, x0, stride, ab, Q, R, scale, g0);
            else if (EP == 4)
                hipLaunchKernelGGL(acceleration_points_kernel<4>, grid, dim3(256), 0, stream, N1, M, Bg, x0, stride, ab, Q, R, scale, g0);
            else
                hipLaunchKernelGGL(acceleration_points_kernel<16>, grid, dim3(256), 0, stream, N1, M, Bg, x0, stride, ab, Q, R, scale, g0);
            SHG_HIP(hipGetLastError());
        }
    }
    SHG_HIP(hipGetLastError());
    return SHG_OK;
}

// Arguments are checked before the first HIP call (the CPU tests call these without a device).
static int check_acceleration(const char* fn, int N, const double* xyz, int M, int layout, const void* coef, int B, double GM, double R, double* g) {
    SHG_REQUIRE(N >= 0 && M >= 0 && B >= 0, "%s: negative size (N %d, M %d, B %d)", fn, N, M, B);
    SHG_REQUIRE(layout == SHG_POINTS_SHARED || layout == SHG_POINTS_PER_EPOCH, "%s: layout %d, expected 0 (shared points) or 1 (points per epoch)", fn,
                layout);
    SHG_REQUIRE(std::isfinite(GM) && std::isfinite(R) && R > 0.0, "%s: GM and R must be finite and R positive (GM %g, R %g)", fn, GM, R);
    SHG_REQUIRE(3LL * M * B <= (1LL << 40), "%s: output of %lld values is too large", fn, 3LL * M * B);
    if (M > 0 && B > 0) SHG_REQUIRE(xyz && coef && g, "%s: NULL pointer", fn);
    return SHG_OK;
}

extern "C" int shg_acceleration_points(int N, const double* xyz, int M, int layout, const double* anm, int B, double GM, double R, double* g,
                                       void* stream) {
    if (int rc = check_acceleration("shg_acceleration_points", N, xyz, M, layout, anm, B, GM, R, g)) return rc;
    if (M == 0 || B == 0) return SHG_OK;
    return acceleration_points(N, xyz, M, layout, CoefSource{anm, nullptr, N, B, 0}, GM, R, g, (hipStream_t)stream);
}

extern "C" int shg_acceleration_points_om(int N, const double* xyz, int M, int layout, const double* om, int B, int Bpad, double GM, double R, double* g,
                                          void* stream) {
    if (int rc = check_acceleration("shg_acceleration_points_om", N, xyz, M, layout, om, B, GM, R, g)) return rc;
    SHG_REQUIRE(Bpad >= B, "shg_acceleration_points_om: Bpad %d below B %d", Bpad, B);
    if (M == 0 || B == 0) return SHG_OK;
    return acceleration_points(N, xyz, M, layout, CoefSource{nullptr, om, N, B, Bpad}, GM, R, g, (hipStream_t)stream);
}

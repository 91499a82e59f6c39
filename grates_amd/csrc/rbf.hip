// Design matrices with respect to the node values of isotropic radial basis functions (gravityfield.RadialBasisFunctions), transposed:
// At [J][K][ldt] with the points innermost, the layout of shg_acceleration_design, so that a block viewed as [J, K Mb] is the operand
// of N += At At^T as it stands.
//
// Node j lies at r_j e_j on the ellipsoid of the basis; with the shape factor k_n of degree n (zero outside min_degree .. N) and, for a
// point x = r xh,
//   t = xh . e_j      q = (R / r)(R / r_j)      d_n = k_n (2n + 1),
// the addition theorem of the 4 pi-normalised harmonics collapses the sum over the orders:
//   V_j(x)      = GM / R     sum_n d_n q^(n+1) P_n(t)
//   grad V_j(x) = GM / (R r) [ -S_r xh + S_t (e_j - t xh) ],   S_r = sum_n (n + 1) d_n q^(n+1) P_n(t),   S_t = sum_n d_n q^(n+1) P'_n(t)
// with the unnormalised Legendre polynomials P_n.  An entry is O(N) work on one (point, node) pair; the same columns through the
// spherical harmonics (A_sh times to_potential_coefficients_matrix) cost O(N^2) per entry.  RbfChain (rbf.h) is the one definition of
// the sums; the four kinds differ in what they do with its result:
//   acceleration           K = 3   g_c(x_i)
//   line of sight          K = 1   e_i . (g(b_i) - g(a_i)), the difference per component first, then the projection (shg_los_design)
//   potential              K = 1   V(x_i)
//   potential difference   K = 1   V(b_i) - V(a_i)
// so a pair's row is, bit for bit, made of what the single-point kinds compute at its two satellites.
#include "rbf.h"

#include <cmath>
#include <vector>

namespace shg {

constexpr int kRbfTile = 16;                          // nodes per workgroup (blockIdx.y)
constexpr int kRbfUnroll = 4;                         // nodes whose chains a lane runs side by side: independent work under the fp64 latency

// One lane per point (pair), 256 per workgroup (blockIdx.x); the workgroup covers the nodes blockIdx.y * kRbfTile ...  The node data
// (e_j, R / r_j) and the degree table are read at wave-uniform addresses: no LDS.  A lane runs the chains of kRbfUnroll nodes (at both
// satellites for the pair kinds) through the degrees in lockstep and stores their entries, consecutive lanes to consecutive doubles
// of a row.  The last group of a tile repeats its last node instead of branching inside the degree loop; the repeats are not stored.
// Every entry is (value * scale) * sqrt(w), in that order (wl 0: none, 1: w [M], 2: w [M][3], acceleration only).
template <int Kind>
__global__ __launch_bounds__(256) void rbf_design_kernel(int N, int J, int M, const RbfDegree* __restrict__ tab, const double* __restrict__ nodes,
                                                         const double* __restrict__ xyz_a, const double* __restrict__ xyz_b,
                                                         const double* __restrict__ directions, const double* __restrict__ w, int wl, double GM_R,
                                                         double R, double* __restrict__ out, size_t ldt) {
    constexpr bool kPairs = Kind == SHG_RBF_LINE_OF_SIGHT || Kind == SHG_RBF_POTENTIAL_DIFFERENCE;
    constexpr bool kGradient = Kind == SHG_RBF_ACCELERATION || Kind == SHG_RBF_LINE_OF_SIGHT;
    constexpr int kSets = kPairs ? 2 : 1;
    constexpr int K = Kind == SHG_RBF_ACCELERATION ? 3 : 1;
    const int pt = blockIdx.x * 256 + threadIdx.x;
    if (pt >= M) return;
    RbfPoint p[kSets];
    p[0].start(xyz_a + (size_t)pt * 3, R);
    if (kPairs) p[kSets - 1].start(xyz_b + (size_t)pt * 3, R);
    double sw[K];
#pragma unroll
    for (int c = 0; c < K; ++c) sw[c] = wl == 0 ? 1.0 : sqrt(wl == 2 ? w[(size_t)pt * K + c] : w[pt]);
    double e[3] = {0.0, 0.0, 0.0};
    if (Kind == SHG_RBF_LINE_OF_SIGHT) {
        if (directions) {
#pragma unroll
            for (int c = 0; c < 3; ++c) e[c] = directions[(size_t)pt * 3 + c];
        } else {                                                     // as los_design_kernel: |d| = sqrt((dx^2 + dy^2) + dz^2), one division each
#pragma unroll
            for (int c = 0; c < 3; ++c) e[c] = xyz_b[(size_t)pt * 3 + c] - xyz_a[(size_t)pt * 3 + c];
            const double len = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
#pragma unroll
            for (int c = 0; c < 3; ++c) e[c] = e[c] / len;
        }
    }
    double scale[kSets];                                             // GM / R for V, GM / (R r) for its gradient
#pragma unroll
    for (int s = 0; s < kSets; ++s) scale[s] = kGradient ? GM_R * p[s].rinv : GM_R;

    const int j0 = blockIdx.y * kRbfTile, j1 = min(j0 + kRbfTile, J);
    const RbfDegree f0 = tab[0];
    for (int jb = j0; jb < j1; jb += kRbfUnroll) {
        RbfChain ch[kSets][kRbfUnroll];
#pragma unroll
        for (int i = 0; i < kRbfUnroll; ++i) {
            const double* node = nodes + (size_t)min(jb + i, j1 - 1) * 4;
#pragma unroll
            for (int s = 0; s < kSets; ++s) ch[s][i].start(p[s], node, f0);
        }
        for (int n = 1; n <= N; ++n) {
            const RbfDegree f = tab[n];
#pragma unroll
            for (int i = 0; i < kRbfUnroll; ++i)
#pragma unroll
                for (int s = 0; s < kSets; ++s) ch[s][i].step(f);
        }
#pragma unroll
        for (int i = 0; i < kRbfUnroll; ++i) {
            if (jb + i >= j1) break;
            const double* node = nodes + (size_t)(jb + i) * 4;
            double v[kSets], g[kSets][3];
#pragma unroll
            for (int s = 0; s < kSets; ++s) {
                ch[s][i].finish(p[s], node, v[s], g[s]);
                v[s] = v[s] * scale[s];
#pragma unroll
                for (int c = 0; c < 3; ++c) g[s][c] = g[s][c] * scale[s];
            }
            double* o = out + (size_t)(jb + i) * K * ldt + pt;
            if (Kind == SHG_RBF_ACCELERATION) {
#pragma unroll
                for (int c = 0; c < K; ++c) o[c * ldt] = g[0][c] * sw[c];
            } else if (Kind == SHG_RBF_LINE_OF_SIGHT) {
                double d[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) d[c] = g[kSets - 1][c] - g[0][c];
                o[0] = ((e[0] * d[0] + e[1] * d[1]) + e[2] * d[2]) * sw[0];
            } else if (Kind == SHG_RBF_POTENTIAL) {
                o[0] = v[0] * sw[0];
            } else {
                o[0] = (v[kSets - 1] - v[0]) * sw[0];
            }
        }
    }
}

// ---- the gradient tensor ---------------------------------------------------------------------------------------------------------------
//   Hess V_j(x) = GM / (R r^2) [ S_rr xh xh^T - (S_r + t S_t)(I - xh xh^T) - (S_rt + S_t)(xh tau^T + tau xh^T) + S_tt tau tau^T ]
// with tau = e_j - t xh and the three further sums of RbfHessianChain (rbf.h).  Symmetric by construction, trace-free degree by degree
// ((n + 1)(n + 2) P_n - 2 (n + 1) P_n - 2 t P'_n + (1 - t^2) P''_n = 0) and regular at t = +-1.
#ifndef SHG_RBF_HESSIAN_UNROLL
#define SHG_RBF_HESSIAN_UNROLL 4
#endif
constexpr int kRbfHessianUnroll = SHG_RBF_HESSIAN_UNROLL;    // chains a lane runs side by side, 14 doubles each: 4 measured 4 % faster than 2
static_assert(kRbfTile % kRbfHessianUnroll == 0, "a tile is a whole number of groups");

// The launch geometry of rbf_design_kernel: one lane per point, the nodes blockIdx.y * kRbfTile ... per workgroup, node data and degree
// table at wave-uniform addresses.  out [J][K][ldt] with the K components of `mask` (bit j: component j of xx, xy, xz, yy, yz, zz) in
// ascending order.  A lane keeps the frame of its point (kFrames: F [3][3], row a = instrument axis a) and the square roots of its
// weights across the nodes; per node it forms the six Earth-fixed entries, then, as gradient_design_kernel (design.hip) does,
// T'_ab = f_a . (T f_b) for the selected components (T f_b once per b), scales by GM / (R r^2) and by sqrt(w) (wl 0: none, 1: w [M],
// 2: w [M][K]) and stores.
template <bool kFrames>
__global__ __launch_bounds__(256) void rbf_gradient_design_kernel(int N, int J, int M, const RbfDegree2* __restrict__ tab, const double* __restrict__ nodes,
                                                                  const double* __restrict__ xyz, const double* __restrict__ frames, int mask, int K,
                                                                  const double* __restrict__ w, int wl, double GM_R, double R,
                                                                  double* __restrict__ out, size_t ldt) {
    const int pt = blockIdx.x * 256 + threadIdx.x;
    if (pt >= M) return;
    RbfPoint p;
    p.start(xyz + (size_t)pt * 3, R);
    double F[3][3];
    if (kFrames) {
#pragma unroll
        for (int i = 0; i < 9; ++i) F[i / 3][i % 3] = frames[(size_t)pt * 9 + i];
    }
    double sw[6];
    {
        const double wp = wl == 1 ? sqrt(w[pt]) : 1.0;
        int k = 0;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            sw[j] = wp;
            if ((mask >> j) & 1) {
                if (wl == 2) sw[j] = sqrt(w[(size_t)pt * K + k]);
                ++k;
            }
        }
    }
    const double scale = (GM_R * p.rinv) * p.rinv;                  // GM / (R r^2)

    const int j0 = blockIdx.y * kRbfTile, j1 = min(j0 + kRbfTile, J);
    const RbfDegree2 f0 = tab[0];
    for (int jb = j0; jb < j1; jb += kRbfHessianUnroll) {
        RbfHessianChain ch[kRbfHessianUnroll];
#pragma unroll
        for (int i = 0; i < kRbfHessianUnroll; ++i) ch[i].start(p, nodes + (size_t)min(jb + i, j1 - 1) * 4, f0);
        for (int n = 1; n <= N; ++n) {
            const RbfDegree2 f = tab[n];
#pragma unroll
            for (int i = 0; i < kRbfHessianUnroll; ++i) ch[i].step(f);
        }
#pragma unroll
        for (int i = 0; i < kRbfHessianUnroll; ++i) {
            if (jb + i >= j1) break;
            double t[6];                                             // xx, xy, xz, yy, yz, zz in the Earth-fixed frame
            ch[i].finish(p, nodes + (size_t)(jb + i) * 4, t);
            double u[3][3] = {};                                     // u[b] = T f_b
            if (kFrames) {
                const int need[3] = {mask & 1, mask & (2 | 8), mask & (4 | 16 | 32)};
#pragma unroll
                for (int b = 0; b < 3; ++b)
                    if (need[b]) {
                        u[b][0] = (t[0] * F[b][0] + t[1] * F[b][1]) + t[2] * F[b][2];
                        u[b][1] = (t[1] * F[b][0] + t[3] * F[b][1]) + t[4] * F[b][2];
                        u[b][2] = (t[2] * F[b][0] + t[4] * F[b][1]) + t[5] * F[b][2];
                    }
            }
            double* o = out + (size_t)(jb + i) * K * ldt + pt;
            int j = 0;
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = a; b < 3; ++b, ++j)
                    if ((mask >> j) & 1) {
                        const double v = kFrames ? (F[a][0] * u[b][0] + F[a][1] * u[b][1]) + F[a][2] * u[b][2] : t[j];
                        *o = (v * scale) * sw[j];
                        o += ldt;
                    }
        }
    }
}

}  // namespace shg

using namespace shg;

// Host only: no HIP call.
extern "C" int shg_rbf_design_info(int which[4]) {
    SHG_REQUIRE(which, "shg_rbf_design_info: NULL pointer");
    which[0] = kRbfTile;
    which[1] = kRbfUnroll;
    which[2] = 256;                                                  // points per workgroup
    which[3] = 65535 * kRbfTile;                                     // the most nodes of one call
    return SHG_OK;
}

template <int Kind>
static void launch_rbf(dim3 grid, hipStream_t stream, int N, int J, int M, const RbfDegree* tab, const double* nodes, const double* xyz_a,
                       const double* xyz_b, const double* directions, const double* w, int wl, double GM_R, double R, double* At, int ldt) {
    hipLaunchKernelGGL(rbf_design_kernel<Kind>, grid, dim3(256), 0, stream, N, J, M, tab, nodes, xyz_a, xyz_b, directions, w, wl, GM_R, R, At, (size_t)ldt);
}

extern "C" int shg_rbf_design(int kind, int N, int min_degree, const double* shape, const double* nodes, int J, const double* xyz_a, const double* xyz_b,
                              const double* directions, int M, const double* weights, int weight_layout, double GM, double R, double* At, int ldt,
                              void* stream_) {
    const char* fn = "shg_rbf_design";
    SHG_REQUIRE(kind >= SHG_RBF_ACCELERATION && kind <= SHG_RBF_POTENTIAL_DIFFERENCE,
                "%s: kind %d, expected 0 (acceleration), 1 (line of sight), 2 (potential) or 3 (potential difference)", fn, kind);
    const bool pairs = kind == SHG_RBF_LINE_OF_SIGHT || kind == SHG_RBF_POTENTIAL_DIFFERENCE;
    const int K = kind == SHG_RBF_ACCELERATION ? 3 : 1;
    SHG_REQUIRE(N >= 0 && min_degree >= 0 && J >= 0 && M >= 0, "%s: negative size (N %d, min_degree %d, J %d, M %d)", fn, N, min_degree, J, M);
    SHG_REQUIRE(min_degree <= N, "%s: min_degree %d above N %d", fn, min_degree, N);
    SHG_REQUIRE(N <= 32767, "%s: N %d is too large", fn, N);
    SHG_REQUIRE(J <= 65535 * kRbfTile, "%s: J %d above the %d nodes of one call", fn, J, 65535 * kRbfTile);
    SHG_REQUIRE(weight_layout == SHG_WEIGHTS_NONE || weight_layout == SHG_WEIGHTS_POINT || (weight_layout == SHG_WEIGHTS_COMPONENT && K == 3),
                "%s: weight layout %d, expected 0 (none), 1 (per point) or, for the acceleration, 2 (per component)", fn, weight_layout);
    SHG_REQUIRE(std::isfinite(GM) && std::isfinite(R) && R > 0.0, "%s: GM and R must be finite and R positive (GM %g, R %g)", fn, GM, R);
    SHG_REQUIRE(ldt >= M, "%s: ldt %d below M %d", fn, ldt, M);
    SHG_REQUIRE(ldt == 0 || (long long)J * K <= (1LL << 40) / ldt, "%s: output of %d x %d x %d values is too large", fn, J, K, ldt);
    if (M == 0 || J == 0) return SHG_OK;
    SHG_REQUIRE(shape && nodes && xyz_a && At && (weights || weight_layout == SHG_WEIGHTS_NONE), "%s: NULL pointer", fn);
    SHG_REQUIRE(xyz_b || !pairs, "%s: NULL pointer (a pair kind needs the positions of the second satellite)", fn);
    hipStream_t stream = (hipStream_t)stream_;
    Workspace ws = Workspace::plain(stream);
    RbfDegree* tab;
    if (!ws.alloc(tab, (size_t)N + 1)) return fail(SHG_ERR_NOMEM, "%s: workspace allocation failed", fn);
    std::vector<RbfDegree> h((size_t)N + 1);
    rbf_degree_table(N, min_degree, shape, h.data());
    SHG_HIP(hipMemcpyAsync(tab, h.data(), h.size() * sizeof(RbfDegree), hipMemcpyHostToDevice, stream));
    SHG_HIP(hipStreamSynchronize(stream));                           // the one wait of a call: the host table goes out of scope
    const dim3 grid(ceil_div(M, 256), ceil_div(J, kRbfTile));
    const double GM_R = GM / R;
    switch (kind) {
        case SHG_RBF_ACCELERATION:
            launch_rbf<SHG_RBF_ACCELERATION>(grid, stream, N, J, M, tab, nodes, xyz_a, xyz_b, directions, weights, weight_layout, GM_R, R, At, ldt);
            break;
        case SHG_RBF_LINE_OF_SIGHT:
            launch_rbf<SHG_RBF_LINE_OF_SIGHT>(grid, stream, N, J, M, tab, nodes, xyz_a, xyz_b, directions, weights, weight_layout, GM_R, R, At, ldt);
            break;
        case SHG_RBF_POTENTIAL:
            launch_rbf<SHG_RBF_POTENTIAL>(grid, stream, N, J, M, tab, nodes, xyz_a, xyz_b, directions, weights, weight_layout, GM_R, R, At, ldt);
            break;
        default:
            launch_rbf<SHG_RBF_POTENTIAL_DIFFERENCE>(grid, stream, N, J, M, tab, nodes, xyz_a, xyz_b, directions, weights, weight_layout, GM_R, R, At, ldt);
    }
    SHG_HIP(hipGetLastError());
    return SHG_OK;
}

extern "C" int shg_rbf_gradient_design(int N, int min_degree, const double* shape, const double* nodes, int J, const double* xyz, int M, const double* frames,
                                       int components, const double* weights, int weight_layout, double GM, double R, double* At, int ldt, void* stream_) {
    const char* fn = "shg_rbf_gradient_design";
    SHG_REQUIRE(components >= 1 && components <= 63, "%s: components %d, expected a set of SHG_GRAD_XX ... SHG_GRAD_ZZ (1 .. 63)", fn, components);
    const int mask = components, K = __builtin_popcount((unsigned)mask);
    SHG_REQUIRE(N >= 0 && min_degree >= 0 && J >= 0 && M >= 0, "%s: negative size (N %d, min_degree %d, J %d, M %d)", fn, N, min_degree, J, M);
    SHG_REQUIRE(min_degree <= N, "%s: min_degree %d above N %d", fn, min_degree, N);
    SHG_REQUIRE(N <= 32767, "%s: N %d is too large", fn, N);
    SHG_REQUIRE(J <= 65535 * kRbfTile, "%s: J %d above the %d nodes of one call", fn, J, 65535 * kRbfTile);
    SHG_REQUIRE(weight_layout == SHG_WEIGHTS_NONE || weight_layout == SHG_WEIGHTS_POINT || weight_layout == SHG_WEIGHTS_COMPONENT,
                "%s: weight layout %d, expected 0 (none), 1 (per point) or 2 (per component)", fn, weight_layout);
    SHG_REQUIRE(std::isfinite(GM) && std::isfinite(R) && R > 0.0, "%s: GM and R must be finite and R positive (GM %g, R %g)", fn, GM, R);
    SHG_REQUIRE(ldt >= M, "%s: ldt %d below M %d", fn, ldt, M);
    SHG_REQUIRE(ldt == 0 || (long long)J * K <= (1LL << 40) / ldt, "%s: output of %d x %d x %d values is too large", fn, J, K, ldt);
    if (M == 0 || J == 0) return SHG_OK;
    SHG_REQUIRE(shape && nodes && xyz && At && (weights || weight_layout == SHG_WEIGHTS_NONE), "%s: NULL pointer", fn);
    hipStream_t stream = (hipStream_t)stream_;
    Workspace ws = Workspace::plain(stream);
    RbfDegree2* tab;
    if (!ws.alloc(tab, (size_t)N + 1)) return fail(SHG_ERR_NOMEM, "%s: workspace allocation failed", fn);
    std::vector<RbfDegree2> h((size_t)N + 1);
    rbf_degree_table(N, min_degree, shape, h.data());
    SHG_HIP(hipMemcpyAsync(tab, h.data(), h.size() * sizeof(RbfDegree2), hipMemcpyHostToDevice, stream));
    SHG_HIP(hipStreamSynchronize(stream));                           // the one wait of a call: the host table goes out of scope
    const dim3 grid(ceil_div(M, 256), ceil_div(J, kRbfTile));
    const double GM_R = GM / R;
    if (frames)
        hipLaunchKernelGGL(rbf_gradient_design_kernel<true>, grid, dim3(256), 0, stream, N, J, M, tab, nodes, xyz, frames, mask, K, weights, weight_layout,
                           GM_R, R, At, (size_t)ldt);
    else
        hipLaunchKernelGGL(rbf_gradient_design_kernel<false>, grid, dim3(256), 0, stream, N, J, M, tab, nodes, xyz, nullptr, mask, K, weights, weight_layout,
                           GM_R, R, At, (size_t)ldt);
    SHG_HIP(hipGetLastError());
    return SHG_OK;
}

// Design matrices with respect to the node values of isotropic radial basis functions (gravityfield.RadialBasisFunctions), transposed:
// At [J][K][ldt] with the points innermost, the layout of shg_acceleration_design and shg_gradient_design, so that a block viewed as
// [J, K Mb] is the operand of N += At At^T as it stands.
//
// Node j lies at r_j e_j on the ellipsoid of the basis; with the shape factor k_n of degree n (zero outside min_degree .. N) and, for a
// point x = r xh,
//   t = xh . e_j      q = (R / r)(R / r_j)      d_n = k_n (2n + 1)      tau = e_j - t xh,
// the addition theorem of the 4 pi-normalised harmonics collapses the sum over the orders:
//   V_j(x)      = GM / R       sum_n d_n q^(n+1) P_n(t)
//   grad V_j(x) = GM / (R r)   [ -S_r xh + S_t tau ]
//   Hess V_j(x) = GM / (R r^2) [ S_rr xh xh^T - (S_r + t S_t)(I - xh xh^T) - (S_rt + S_t)(xh tau^T + tau xh^T) + S_tt tau tau^T ]
// with the unnormalised Legendre polynomials P_n and the sums of RbfChain (rbf.h), the one definition of them.  The Hessian is symmetric
// by construction, trace-free degree by degree ((n + 1)(n + 2) P_n - 2 (n + 1) P_n - 2 t P'_n + (1 - t^2) P''_n = 0) and regular at
// t = +-1.  An entry is O(N) work on one (point, node) pair; the same columns through the spherical harmonics (A_sh times
// to_potential_coefficients_matrix) cost O(N^2) per entry.
//
// One kernel walks the pairs (rbf_sweep_kernel); the five functionals differ in what they do with a finished chain:
//   acceleration           K = 3        g_c(x_i)                                                   RbfObservation, shg_rbf_design
//   line of sight          K = 1        e_i . (g(b_i) - g(a_i)), the difference per component first, then the projection (shg_los_design)
//   potential              K = 1        V(x_i)
//   potential difference   K = 1        V(b_i) - V(a_i)
//   gradient tensor        K = 1 .. 6   the selected components of F_i Hess V(x_i) F_i^T            RbfGradient, shg_rbf_gradient_design
// so a pair's row is, bit for bit, made of what the single-point kinds compute at its two satellites.
//
// The way back from node values to maps is here as well: the surface synthesis St [J][ldt] of a grid's points (rbf_surface_kernel,
// shg_rbf_surface: the same sum with the surface factors of the functional per point and degree) and the column dot products that
// turn St and C St into the formal errors of a map (column_dots_kernel, shg_column_dots).
#include "observe.h"
#include "rbf.h"

#include <cmath>
#include <vector>

namespace shg {

constexpr int kRbfTile = 16;                          // nodes per workgroup (blockIdx.y)
constexpr int kRbfUnroll = 4;                         // nodes whose chains a lane runs side by side: independent work under the fp64 latency
#ifndef SHG_RBF_HESSIAN_UNROLL
#define SHG_RBF_HESSIAN_UNROLL 4
#endif
constexpr int kRbfHessianUnroll = SHG_RBF_HESSIAN_UNROLL;    // the same for the gradient tensor, 14 doubles a chain: 4 measured 4 % faster than 2
static_assert(kRbfTile % kRbfUnroll == 0 && kRbfTile % kRbfHessianUnroll == 0, "a tile is a whole number of groups");

// A functional is the arguments of its entry point (a kernel argument, wave-uniform) and says what the sweep cannot know:
//   kOrder, kSets, kUnroll   derivative order of the chains, satellites per lane (1 | 2), nodes a lane runs side by side
//   positions(s)             the points of satellite s, [M][3]
//   rows()                   K, the rows of At per node
//   Lane, start              what a lane keeps across the nodes, set from its point(s) once
//   store                    what becomes of the finished chains of one node (one per satellite): the K entries o[0], o[ldt], ...
// Every entry is (value * scale) * sqrt(w), in that order.

// The four kinds of shg_rbf_design (wl 0: no weights, 1: w [M], 2: w [M][3], acceleration only).
template <int Kind>
struct RbfObservation {
    static constexpr bool kPairs = Kind == SHG_RBF_LINE_OF_SIGHT || Kind == SHG_RBF_POTENTIAL_DIFFERENCE;
    static constexpr bool kGradient = Kind == SHG_RBF_ACCELERATION || Kind == SHG_RBF_LINE_OF_SIGHT;
    static constexpr int kOrder = 1, kSets = kPairs ? 2 : 1, kUnroll = kRbfUnroll, K = Kind == SHG_RBF_ACCELERATION ? 3 : 1;
    const double *xyz_a, *xyz_b, *directions, *w;
    int wl;
    struct Lane {
        double sw[K], e[3], scale[kSets];             // e: the line of sight; scale: GM / R for V, GM / (R r) for its gradient
    };
    __device__ const double* positions(int s) const { return s ? xyz_b : xyz_a; }
    __device__ int rows() const { return K; }
    __device__ void start(Lane& l, size_t pt, const RbfPoint* p, double GM_R) const {
#pragma unroll
        for (int c = 0; c < K; ++c) l.sw[c] = wl == 0 ? 1.0 : sqrt(wl == 2 ? w[pt * K + c] : w[pt]);
        if (Kind == SHG_RBF_LINE_OF_SIGHT) line_of_sight(!directions, xyz_a, xyz_b, directions, pt, l.e);
#pragma unroll
        for (int s = 0; s < kSets; ++s) l.scale[s] = kGradient ? GM_R * p[s].rinv : GM_R;
    }
    __device__ void store(const Lane& l, const RbfPoint* p, const RbfChain<1>* ch, const double* node, double* o, size_t ldt) const {
        double v[kSets], g[kSets][3];
#pragma unroll
        for (int s = 0; s < kSets; ++s) {
            ch[s].finish(p[s], node, v[s], g[s]);
            v[s] = v[s] * l.scale[s];
#pragma unroll
            for (int c = 0; c < 3; ++c) g[s][c] = g[s][c] * l.scale[s];
        }
        if (Kind == SHG_RBF_ACCELERATION) {
#pragma unroll
            for (int c = 0; c < K; ++c) o[c * ldt] = g[0][c] * l.sw[c];
        } else if (Kind == SHG_RBF_LINE_OF_SIGHT) {
            double d[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) d[c] = g[kSets - 1][c] - g[0][c];
            o[0] = ((l.e[0] * d[0] + l.e[1] * d[1]) + l.e[2] * d[2]) * l.sw[0];
        } else if (Kind == SHG_RBF_POTENTIAL) {
            o[0] = v[0] * l.sw[0];
        } else {
            o[0] = (v[kSets - 1] - v[0]) * l.sw[0];
        }
    }
};

// The gradient tensor of shg_rbf_gradient_design: the K components of `mask` (bit j: component j of xx, xy, xz, yy, yz, zz) in ascending
// order, in the instrument frames of the points (kFrames) or Earth-fixed, with the arithmetic, the component choice and the weights
// (wl 0: none, 1: w [M], 2: w [M][K]) of gradient_design_kernel (design.hip): FrameTensor of observe.h.
template <bool kFrames>
struct RbfGradient {
    static constexpr int kOrder = 2, kSets = 1, kUnroll = kRbfHessianUnroll;
    const double *xyz, *frames, *w;
    int mask, K, wl;
    struct Lane {
        FrameTensor<kFrames> tensor;
        double scale;                                 // GM / (R r^2)
    };
    __device__ const double* positions(int) const { return xyz; }
    __device__ int rows() const { return K; }
    __device__ void start(Lane& l, size_t pt, const RbfPoint* p, double GM_R) const {
        l.tensor.start(frames, mask, K, w, wl, pt);
        l.scale = (GM_R * p->rinv) * p->rinv;
    }
    __device__ void store(const Lane& l, const RbfPoint* p, const RbfChain<2>* ch, const double* node, double* o, size_t ldt) const {
        double t[6];                                                 // xx, xy, xz, yy, yz, zz in the Earth-fixed frame
        ch->finish(*p, node, t);
        l.tensor.store(t, mask, l.scale, o, ldt);
    }
};

// One lane per point (pair), 256 per workgroup (blockIdx.x); the workgroup covers the nodes blockIdx.y * kRbfTile ...  The node data
// (e_j, R / r_j) and the degree table are read at wave-uniform addresses: no LDS.  A lane runs the chains of kUnroll nodes (at both
// satellites for the pair kinds) through the degrees in lockstep and hands them to the functional node by node, which stores their
// entries, consecutive lanes to consecutive doubles of a row.  The last group of a tile repeats its last node instead of branching
// inside the degree loop; the repeats are not stored.
template <class Functional>
__global__ __launch_bounds__(256) void rbf_sweep_kernel(int N, int J, int M, const RbfDegree<Functional::kOrder>* __restrict__ tab,
                                                        const double* __restrict__ nodes, const Functional fn, double GM_R, double R,
                                                        double* __restrict__ out, size_t ldt) {
    constexpr int kSets = Functional::kSets, kUnroll = Functional::kUnroll;
    using Degree = RbfDegree<Functional::kOrder>;
    const int pt = blockIdx.x * 256 + threadIdx.x;
    if (pt >= M) return;
    RbfPoint p[kSets];
#pragma unroll
    for (int s = 0; s < kSets; ++s) p[s].start(fn.positions(s) + (size_t)pt * 3, R);
    typename Functional::Lane lane;
    fn.start(lane, (size_t)pt, p, GM_R);
    const int K = fn.rows();

    const int j0 = blockIdx.y * kRbfTile, j1 = min(j0 + kRbfTile, J);
    const Degree f0 = tab[0];
    for (int jb = j0; jb < j1; jb += kUnroll) {
        RbfChain<Functional::kOrder> ch[kUnroll][kSets];
#pragma unroll
        for (int i = 0; i < kUnroll; ++i) {
            const double* node = nodes + (size_t)min(jb + i, j1 - 1) * 4;
#pragma unroll
            for (int s = 0; s < kSets; ++s) ch[i][s].start(p[s], node, f0);
        }
        for (int n = 1; n <= N; ++n) {
            const Degree f = tab[n];
#pragma unroll
            for (int i = 0; i < kUnroll; ++i)
#pragma unroll
                for (int s = 0; s < kSets; ++s) ch[i][s].step(f);
        }
#pragma unroll
        for (int i = 0; i < kUnroll; ++i) {
            if (jb + i >= j1) break;
            fn.store(lane, p, ch[i], nodes + (size_t)(jb + i) * 4, out + (size_t)(jb + i) * K * ldt + pt, ldt);
        }
    }
}

// ---- the surface synthesis of the node values (shg_rbf_surface) ---------------------------------------------------------------------------
constexpr int kRbfSurfaceUnroll = 4;                  // nodes a lane runs side by side: 6 doubles a chain, 70 VGPRs and 7 waves per SIMD at 4 chains
static_assert(kRbfTile % kRbfSurfaceUnroll == 0, "a tile is a whole number of groups");

// St[j][i] = sum_{n = min_degree .. N} kn[n][i] d_n u_j^(n+1) P_n(e_i . e_j): the launch geometry of rbf_sweep_kernel, one lane per grid
// point, 256 per workgroup (blockIdx.x), the nodes blockIdx.y * kRbfTile ... per workgroup, kRbfSurfaceUnroll chains (RbfSurfaceChain)
// side by side in a lane.  The factor of the point is per degree, so it cannot sit in the wave-uniform table: the lane loads its own
// kn[n][i] (degree-major, consecutive lanes consecutive doubles), one degree ahead of its use, and forms c_n = kn[n][i] d_n once for its
// chains.  The rows of kn below max(min_degree, 1) are not read, row 0 only by a band that starts there.  The last group of a tile
// repeats its last node instead of branching inside the degree loop; the repeats are not stored.
__global__ __launch_bounds__(256) void rbf_surface_kernel(int N, int min_degree, int J, int M, const RbfDegree<1>* __restrict__ tab,
                                                          const double* __restrict__ nodes, const double* __restrict__ points,
                                                          const double* __restrict__ kn, size_t ldk, double* __restrict__ St, size_t ldt) {
    constexpr int kUnroll = kRbfSurfaceUnroll;
    const int pt = blockIdx.x * 256 + threadIdx.x;
    if (pt >= M) return;
    const double xh[3] = {points[(size_t)pt * 3], points[(size_t)pt * 3 + 1], points[(size_t)pt * 3 + 2]};
    const double* kp = kn + pt;
    const int first = max(min_degree, 1);             // the first degree that takes a step with its term
    const double c0 = min_degree == 0 ? kp[0] * tab[0].d : 0.0;

    const int j0 = blockIdx.y * kRbfTile, j1 = min(j0 + kRbfTile, J);
    for (int jb = j0; jb < j1; jb += kUnroll) {
        RbfSurfaceChain ch[kUnroll];
#pragma unroll
        for (int i = 0; i < kUnroll; ++i) ch[i].start(xh, nodes + (size_t)min(jb + i, j1 - 1) * 4, c0);
        for (int n = 1; n < first; ++n) {
            const RbfDegree<1> f = tab[n];
#pragma unroll
            for (int i = 0; i < kUnroll; ++i) ch[i].advance(f.alpha, f.beta);
        }
        double ahead = first <= N ? kp[(size_t)first * ldk] : 0.0;
        for (int n = first; n <= N; ++n) {
            const RbfDegree<1> f = tab[n];
            const double c = ahead * f.d;
            ahead = kp[(size_t)min(n + 1, N) * ldk];
#pragma unroll
            for (int i = 0; i < kUnroll; ++i) ch[i].step(f.alpha, f.beta, c);
        }
#pragma unroll
        for (int i = 0; i < kUnroll; ++i) {
            if (jb + i >= j1) break;
            St[(size_t)(jb + i) * ldt + pt] = ch[i].s;
        }
    }
}

// ---- column dot products (shg_column_dots) -------------------------------------------------------------------------------------------------
constexpr int kDotLanes = 64;                         // columns per workgroup: one lane per column, many workgroups for a block of a few thousand
constexpr int kDotSums = 8;                           // partial sums of a column, loads in flight per operand

// out[i] = sum_r X[r][i] Y[r][i]: row r goes to partial sum r % kDotSums in ascending order, every product rounded before it is added,
// and the partial sums close as ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)).  The order is a function of `rows` alone.
__global__ __launch_bounds__(kDotLanes) void column_dots_kernel(int rows, int cols, const double* __restrict__ X, size_t ldx, const double* __restrict__ Y,
                                                                size_t ldy, double* __restrict__ out) {
    const int c = blockIdx.x * kDotLanes + threadIdx.x;
    if (c >= cols) return;
    const double *x = X + c, *y = Y + c;
    double a[kDotSums];
#pragma unroll
    for (int k = 0; k < kDotSums; ++k) a[k] = 0.0;
    int r = 0;
    for (; r + kDotSums <= rows; r += kDotSums) {
#pragma unroll
        for (int k = 0; k < kDotSums; ++k) a[k] = a[k] + x[(size_t)(r + k) * ldx] * y[(size_t)(r + k) * ldy];
    }
#pragma unroll
    for (int k = 0; k < kDotSums; ++k)
        if (r + k < rows) a[k] = a[k] + x[(size_t)(r + k) * ldx] * y[(size_t)(r + k) * ldy];
    out[c] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
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

// ---- host side: one set of checks and one driver for the two entry points ---------------------------------------------------------------
// What the two entry points pass on as they got it.
struct RbfCall {
    const char* fn;
    int N, min_degree;
    const double *shape, *nodes;
    int J, M;
    double GM, R;
    double* At;
    int ldt;
    hipStream_t stream;
};

// What the entry points check alike, before the first HIP call (the CPU tests call them without a device), in two parts: the check
// of the weight layout, which differs, fires between them.
static int check_rbf_sizes(const RbfCall& c) {
    SHG_REQUIRE(c.N >= 0 && c.min_degree >= 0 && c.J >= 0 && c.M >= 0, "%s: negative size (N %d, min_degree %d, J %d, M %d)", c.fn, c.N, c.min_degree, c.J,
                c.M);
    SHG_REQUIRE(c.min_degree <= c.N, "%s: min_degree %d above N %d", c.fn, c.min_degree, c.N);
    SHG_REQUIRE(c.N <= 32767, "%s: N %d is too large", c.fn, c.N);
    SHG_REQUIRE(c.J <= 65535 * kRbfTile, "%s: J %d above the %d nodes of one call", c.fn, c.J, 65535 * kRbfTile);
    return SHG_OK;
}

// the constants and the output At [J][K][ldt]
static int check_rbf_output(const RbfCall& c, int K) {
    SHG_REQUIRE(std::isfinite(c.GM) && std::isfinite(c.R) && c.R > 0.0, "%s: GM and R must be finite and R positive (GM %g, R %g)", c.fn, c.GM, c.R);
    SHG_REQUIRE(c.ldt >= c.M, "%s: ldt %d below M %d", c.fn, c.ldt, c.M);
    SHG_REQUIRE(c.ldt == 0 || (long long)c.J * K <= (1LL << 40) / c.ldt, "%s: output of %d x %d x %d values is too large", c.fn, c.J, K, c.ldt);
    return SHG_OK;
}

// The table of degrees of one order, built on the host and uploaded to a workspace of the call's stream.
template <int kOrder>
static int rbf_upload_degrees(const RbfCall& c, Workspace& ws, RbfDegree<kOrder>*& tab) {
    if (!ws.alloc(tab, (size_t)c.N + 1)) return fail(SHG_ERR_NOMEM, "%s: workspace allocation failed", c.fn);
    std::vector<RbfDegree<kOrder>> h((size_t)c.N + 1);
    rbf_degree_table(c.N, c.min_degree, c.shape, h.data());
    SHG_HIP(hipMemcpyAsync(tab, h.data(), h.size() * sizeof(RbfDegree<kOrder>), hipMemcpyHostToDevice, c.stream));
    SHG_HIP(hipStreamSynchronize(c.stream));                         // the one wait of a call: the host table goes out of scope
    return SHG_OK;
}

// The call itself, after every check: the table of degrees of the functional's order, then the sweep over all (point, node) pairs.
template <class Functional>
static int rbf_sweep(const RbfCall& c, const Functional& fn) {
    Workspace ws = Workspace::plain(c.stream);
    RbfDegree<Functional::kOrder>* tab;
    if (int rc = rbf_upload_degrees(c, ws, tab)) return rc;
    hipLaunchKernelGGL(rbf_sweep_kernel<Functional>, dim3(ceil_div(c.M, 256), ceil_div(c.J, kRbfTile)), dim3(256), 0, c.stream, c.N, c.J, c.M, tab, c.nodes,
                       fn, c.GM / c.R, c.R, c.At, (size_t)c.ldt);
    SHG_HIP(hipGetLastError());
    return SHG_OK;
}

extern "C" int shg_rbf_design(int kind, int N, int min_degree, const double* shape, const double* nodes, int J, const double* xyz_a, const double* xyz_b,
                              const double* directions, int M, const double* weights, int weight_layout, double GM, double R, double* At, int ldt,
                              void* stream) {
    const RbfCall c{"shg_rbf_design", N, min_degree, shape, nodes, J, M, GM, R, At, ldt, (hipStream_t)stream};
    SHG_REQUIRE(kind >= SHG_RBF_ACCELERATION && kind <= SHG_RBF_POTENTIAL_DIFFERENCE,
                "%s: kind %d, expected 0 (acceleration), 1 (line of sight), 2 (potential) or 3 (potential difference)", c.fn, kind);
    const bool pairs = kind == SHG_RBF_LINE_OF_SIGHT || kind == SHG_RBF_POTENTIAL_DIFFERENCE;
    const int K = kind == SHG_RBF_ACCELERATION ? 3 : 1;
    if (int rc = check_rbf_sizes(c)) return rc;
    SHG_REQUIRE(weight_layout == SHG_WEIGHTS_NONE || weight_layout == SHG_WEIGHTS_POINT || (weight_layout == SHG_WEIGHTS_COMPONENT && K == 3),
                "%s: weight layout %d, expected 0 (none), 1 (per point) or, for the acceleration, 2 (per component)", c.fn, weight_layout);
    if (int rc = check_rbf_output(c, K)) return rc;
    if (M == 0 || J == 0) return SHG_OK;
    SHG_REQUIRE(shape && nodes && xyz_a && At && (weights || weight_layout == SHG_WEIGHTS_NONE), "%s: NULL pointer", c.fn);
    SHG_REQUIRE(xyz_b || !pairs, "%s: NULL pointer (a pair kind needs the positions of the second satellite)", c.fn);
    switch (kind) {
        case SHG_RBF_ACCELERATION:
            return rbf_sweep(c, RbfObservation<SHG_RBF_ACCELERATION>{xyz_a, xyz_b, directions, weights, weight_layout});
        case SHG_RBF_LINE_OF_SIGHT:
            return rbf_sweep(c, RbfObservation<SHG_RBF_LINE_OF_SIGHT>{xyz_a, xyz_b, directions, weights, weight_layout});
        case SHG_RBF_POTENTIAL:
            return rbf_sweep(c, RbfObservation<SHG_RBF_POTENTIAL>{xyz_a, xyz_b, directions, weights, weight_layout});
        default:
            return rbf_sweep(c, RbfObservation<SHG_RBF_POTENTIAL_DIFFERENCE>{xyz_a, xyz_b, directions, weights, weight_layout});
    }
}

extern "C" int shg_rbf_gradient_design(int N, int min_degree, const double* shape, const double* nodes, int J, const double* xyz, int M, const double* frames,
                                       int components, const double* weights, int weight_layout, double GM, double R, double* At, int ldt, void* stream) {
    const RbfCall c{"shg_rbf_gradient_design", N, min_degree, shape, nodes, J, M, GM, R, At, ldt, (hipStream_t)stream};
    SHG_REQUIRE(components >= 1 && components <= 63, "%s: components %d, expected a set of SHG_GRAD_XX ... SHG_GRAD_ZZ (1 .. 63)", c.fn, components);
    const int mask = components, K = __builtin_popcount((unsigned)mask);
    if (int rc = check_rbf_sizes(c)) return rc;
    SHG_REQUIRE(weight_layout == SHG_WEIGHTS_NONE || weight_layout == SHG_WEIGHTS_POINT || weight_layout == SHG_WEIGHTS_COMPONENT,
                "%s: weight layout %d, expected 0 (none), 1 (per point) or 2 (per component)", c.fn, weight_layout);
    if (int rc = check_rbf_output(c, K)) return rc;
    if (M == 0 || J == 0) return SHG_OK;
    SHG_REQUIRE(shape && nodes && xyz && At && (weights || weight_layout == SHG_WEIGHTS_NONE), "%s: NULL pointer", c.fn);
    if (frames) return rbf_sweep(c, RbfGradient<true>{xyz, frames, weights, mask, K, weight_layout});
    return rbf_sweep(c, RbfGradient<false>{xyz, nullptr, weights, mask, K, weight_layout});
}

// Host only: no HIP call.
extern "C" int shg_rbf_surface_info(int which[4]) {
    SHG_REQUIRE(which, "shg_rbf_surface_info: NULL pointer");
    which[0] = kRbfTile;
    which[1] = kRbfSurfaceUnroll;
    which[2] = 256;                                                  // points per workgroup
    which[3] = 65535 * kRbfTile;                                     // the most nodes of one call
    return SHG_OK;
}

extern "C" int shg_rbf_surface(int N, int min_degree, const double* shape, const double* nodes, int J, const double* points, const double* kn, int ldk, int M,
                               double* St, int ldt, void* stream) {
    const RbfCall c{"shg_rbf_surface", N, min_degree, shape, nodes, J, M, 0.0, 0.0, St, ldt, (hipStream_t)stream};
    if (int rc = check_rbf_sizes(c)) return rc;
    SHG_REQUIRE(ldk >= M, "%s: ldk %d below M %d", c.fn, ldk, M);
    SHG_REQUIRE(ldt >= M, "%s: ldt %d below M %d", c.fn, ldt, M);
    SHG_REQUIRE(ldt == 0 || (long long)J <= (1LL << 40) / ldt, "%s: output of %d x %d values is too large", c.fn, J, ldt);
    if (M == 0 || J == 0) return SHG_OK;
    SHG_REQUIRE(shape && nodes && points && kn && St, "%s: NULL pointer", c.fn);
    Workspace ws = Workspace::plain(c.stream);
    RbfDegree<1>* tab;
    if (int rc = rbf_upload_degrees(c, ws, tab)) return rc;
    hipLaunchKernelGGL(rbf_surface_kernel, dim3(ceil_div(M, 256), ceil_div(J, kRbfTile)), dim3(256), 0, c.stream, N, min_degree, J, M, tab, nodes, points, kn,
                       (size_t)ldk, St, (size_t)ldt);
    SHG_HIP(hipGetLastError());
    return SHG_OK;
}

extern "C" int shg_column_dots(int rows, int cols, const double* X, int ldx, const double* Y, int ldy, double* out, void* stream) {
    SHG_REQUIRE(rows >= 0 && cols >= 0, "shg_column_dots: negative size (rows %d, cols %d)", rows, cols);
    SHG_REQUIRE(ldx >= cols && ldy >= cols, "shg_column_dots: leading dimensions %d and %d below the %d columns", ldx, ldy, cols);
    if (cols == 0) return SHG_OK;
    SHG_REQUIRE(out && ((X && Y) || rows == 0), "shg_column_dots: NULL pointer");
    hipLaunchKernelGGL(column_dots_kernel, dim3(ceil_div(cols, kDotLanes)), dim3(kDotLanes), 0, (hipStream_t)stream, rows, cols, X, (size_t)ldx, Y,
                       (size_t)ldy, out);
    SHG_HIP(hipGetLastError());
    return SHG_OK;
}

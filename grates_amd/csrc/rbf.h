// The Legendre sum of one radial basis function at one point and the table of its degree factors: RbfChain<kOrder>, one definition for
// the sums of V_j and its gradient (kOrder 1: the four kinds of shg_rbf_design) and for those of its Hessian (kOrder 2:
// shg_rbf_gradient_design).  The start, the recursions of P_n and P'_n and the sums S_r and S_t are the same statements for both
// orders; the second order adds P''_n and three sums and drops V_j.  The family is tested bit for bit against itself (pairs against
// single points, one batch size against another, a subset of tensor components against all six): that holds because the operations
// below, and their order, exist once.  RbfSurfaceChain at the end is the small chain of the surface synthesis (shg_rbf_surface): the
// same recursion of P_n, a running power of R / r_j and one sum, with a factor per point and degree in the place of d_n.
#pragma once

#include "common.h"

namespace shg {

// What degree n contributes besides P_n: the factors of the recursions and of the sums, built on the host (rbf_degree_table) so that
// the loop divides nothing and converts no integer.  Five doubles for the first order: the second order's entry is a type of its own,
// so that the table, the loads and the registers of the first order do not carry h.
template <int kOrder>
struct RbfDegree {
    double alpha, beta;                               // P_n = alpha t P_{n-1} - beta P_{n-2}: (2n - 1) / n and (n - 1) / n
    double gamma;                                     // P'_n = P'_{n-2} + gamma P_{n-1}, P''_n = P''_{n-2} + gamma P'_{n-1}: 2n - 1
    double d, e;                                      // d_n = k_n (2n + 1), zero outside the band, and (n + 1) d_n
};

template <>
struct RbfDegree<2> : RbfDegree<1> {
    double h;                                         // (n + 2) e_n = (n + 1)(n + 2) d_n
};

// the entries of degrees 0 .. N from the shape factors k [N + 1]; degrees below min_degree carry d = e = h = 0 (they still step: the
// recursions need every degree)
template <int kOrder>
inline void rbf_degree_table(int N, int min_degree, const double* k, RbfDegree<kOrder>* out) {
    for (int n = 0; n <= N; ++n) {
        const double dn = n < min_degree ? 0.0 : k[n] * (2.0 * n + 1.0);
        RbfDegree<kOrder>& f = out[n];
        f.alpha = n ? (2.0 * n - 1.0) / n : 0.0;
        f.beta = n ? (n - 1.0) / n : 0.0;
        f.gamma = n ? 2.0 * n - 1.0 : 0.0;
        f.d = dn;
        f.e = (n + 1.0) * dn;
        if constexpr (kOrder == 2) f.h = (n + 2.0) * f.e;
    }
}

// A point as the chains of all nodes see it: the unit vector, R / r and 1 / r, once per lane.  r = sqrt((x^2 + y^2) + z^2), the
// operation order of SolidColumn.
struct RbfPoint {
    double xh[3], u, rinv;
    __device__ void start(const double* xp, double R) {
        const double x = xp[0], y = xp[1], z = xp[2];
        const double r = sqrt((x * x + y * y) + z * z);
        xh[0] = x / r;
        xh[1] = y / r;
        xh[2] = z / r;
        u = R / r;
        rinv = 1.0 / r;
    }
};

// What a chain carries besides t, q, q^(n+1) and the two values each of P and P': the sums of its order and, for the second, P''.
template <int kOrder>
struct RbfSums;

template <>
struct RbfSums<1> {
    double sv, sr, st;
};

template <>
struct RbfSums<2> {
    double ddp1, ddp2;                                // P''_n, P''_{n-1} after the step of degree n
    double sr, st, srr, srt, stt;
};

// The sums over the degrees for one (point, node) pair, with t = xh . e_j and q = (R / r)(R / r_j):
//   both orders   S_r = sum_n (n + 1) d_n q^(n+1) P_n(t)           S_t  = sum_n d_n q^(n+1) P'_n(t)
//   order 1       v   = sum_n d_n q^(n+1) P_n(t)
//   order 2       S_rr = sum_n (n + 1)(n + 2) d_n q^(n+1) P_n(t)   S_rt = sum_n (n + 1) d_n q^(n+1) P'_n(t)   S_tt = sum_n d_n q^(n+1) P''_n(t)
// start takes degree 0, step(f) every degree from 1 in turn with f the entry of that degree.  alpha_1 = 1, beta_1 = 0 and gamma_1 = 1
// make degree 1 an ordinary step from P_0 = 1, P_{-1} = 0, P'_0 = P'_{-1} = 0, P''_0 = P''_{-1} = 0: the loop has no branch, no
// division and no integer conversion.  No fma: every product is rounded before it is added.  finish returns, unscaled and with
// tau = e_j - t xh,
//   order 1   v and g_c = S_t tau_c - S_r xh_c, to be scaled by GM / R (v) and GM / (R r) (g);
//   order 2   the six Earth-fixed entries xx, xy, xz, yy, yz, zz of
//               S_rr xh xh^T - (S_r + t S_t)(I - xh xh^T) - (S_rt + S_t)(xh tau^T + tau xh^T) + S_tt tau tau^T,
//             to be scaled by GM / (R r^2).  Nothing divides by sin: tau = 0 above a node and antipodal to it, and the expression is
//             regular there.
template <int kOrder>
struct RbfChain {
    static_assert(kOrder == 1 || kOrder == 2, "the sums of the gradient or of the Hessian");
    double t, q, qn;                                  // qn = q^(n+1)
    double p1, p2, dp1, dp2;                          // P_n, P_{n-1}, P'_n, P'_{n-1} after the step of degree n
    RbfSums<kOrder> s;
    __device__ void start(const RbfPoint& pt, const double* node, const RbfDegree<kOrder>& f0) {
        t = (pt.xh[0] * node[0] + pt.xh[1] * node[1]) + pt.xh[2] * node[2];
        q = pt.u * node[3];
        qn = q;
        p1 = 1.0;
        p2 = 0.0;
        dp1 = 0.0;
        dp2 = 0.0;
        s.sr = f0.e * qn;
        s.st = 0.0;
        if constexpr (kOrder == 1) {
            s.sv = f0.d * qn;
        } else {
            s.ddp1 = 0.0;
            s.ddp2 = 0.0;
            s.srr = f0.h * qn;
            s.srt = 0.0;
            s.stt = 0.0;
        }
    }
    __device__ void step(const RbfDegree<kOrder>& f) {
        const double p = (f.alpha * t) * p1 - f.beta * p2;
        const double dp = dp2 + f.gamma * p1;
        if constexpr (kOrder == 2) {
            const double ddp = s.ddp2 + f.gamma * dp1;
            s.ddp2 = s.ddp1;
            s.ddp1 = ddp;
        }
        p2 = p1;
        p1 = p;
        dp2 = dp1;
        dp1 = dp;
        qn *= q;
        const double w = qn * p;
        const double wd = qn * dp;
        if constexpr (kOrder == 1) s.sv = s.sv + f.d * w;            // the sums on P_n ...
        s.sr = s.sr + f.e * w;
        if constexpr (kOrder == 2) s.srr = s.srr + f.h * w;
        s.st = s.st + f.d * wd;                                      // ... on P'_n ...
        if constexpr (kOrder == 2) {
            s.srt = s.srt + f.e * wd;
            s.stt = s.stt + f.d * (qn * s.ddp1);                     // ... and on P''_n
        }
    }
    __device__ double tau(const RbfPoint& pt, const double* node, int c) const { return node[c] - t * pt.xh[c]; }
    __device__ void finish(const RbfPoint& pt, const double* node, double& v, double g[3]) const {
        static_assert(kOrder == 1, "the value and the gradient are the first order's");
        v = s.sv;
#pragma unroll
        for (int c = 0; c < 3; ++c) g[c] = s.st * tau(pt, node, c) - s.sr * pt.xh[c];
    }
    __device__ void finish(const RbfPoint& pt, const double* node, double T[6]) const {
        static_assert(kOrder == 2, "the Hessian is the second order's");
        double ta[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) ta[c] = tau(pt, node, c);
        const double b = s.sr + t * s.st, m = s.srt + s.st;
        int j = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int d = c; d < 3; ++d, ++j) {
                const double xx = pt.xh[c] * pt.xh[d];
                const double k = c == d ? 1.0 - xx : -xx;
                T[j] = ((s.srr * xx - b * k) - m * (pt.xh[c] * ta[d] + ta[c] * pt.xh[d])) + s.stt * (ta[c] * ta[d]);
            }
    }
};

// The sum of the surface synthesis (shg_rbf_surface) for one (grid point, node) pair, with t = e_i . e_j and u = R / r_j:
//   s = sum_{n = min_degree .. N} c_n u^(n+1) P_n(t),      c_n = kn[i][n] d_n, formed once per lane and degree and shared by its chains.
// P_n by the recursion of RbfChain with the same alpha and beta, u^(n+1) as a running product, no derivative, no fma.  start takes
// degree 0 with c0 = c_0 (0.0 for a band that starts above it), advance steps a degree below the band without its term, step a degree
// of the band: un *= u, w = un * p, s = s + c * w, in that order.
struct RbfSurfaceChain {
    double t, u, un;                                  // un = u^(n+1)
    double p1, p2;                                    // P_n, P_{n-1} after the step of degree n
    double s;
    __device__ void start(const double* xh, const double* node, double c0) {
        t = (xh[0] * node[0] + xh[1] * node[1]) + xh[2] * node[2];
        u = node[3];
        un = u;
        p1 = 1.0;
        p2 = 0.0;
        s = c0 * un;
    }
    __device__ double advance(double alpha, double beta) {
        const double p = (alpha * t) * p1 - beta * p2;
        p2 = p1;
        p1 = p;
        un *= u;
        return p;
    }
    __device__ void step(double alpha, double beta, double c) {
        const double p = advance(alpha, beta);
        const double w = un * p;
        s = s + c * w;
    }
};

}  // namespace shg

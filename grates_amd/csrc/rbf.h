// The Legendre sum of one radial basis function at one point, the one every kind of shg_rbf_design runs (rbf.hip: rbf_design_kernel),
// its sibling with second derivatives for shg_rbf_gradient_design (rbf_gradient_design_kernel), and the tables of their degree
// factors.  The family is tested bit for bit against itself (pairs against single points, one batch size against another): that
// holds because the operations below, and their order, exist once.
#pragma once

#include "common.h"

namespace shg {

// What degree n contributes besides P_n: the factors of the two recursions and of the three sums, built on the host (rbf_degree_table)
// so that the loop divides nothing and converts no integer.
struct RbfDegree {
    double alpha, beta;                               // P_n = alpha t P_{n-1} - beta P_{n-2}: (2n - 1) / n and (n - 1) / n
    double gamma;                                     // P'_n = P'_{n-2} + gamma P_{n-1}: 2n - 1
    double d, e;                                      // d_n = k_n (2n + 1), zero outside the band, and (n + 1) d_n
};

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

// V_j = GM / R sum_n d_n q^(n+1) P_n(t) and the two sums of its gradient, S_r = sum_n (n + 1) d_n q^(n+1) P_n(t) and
// S_t = sum_n d_n q^(n+1) P'_n(t), for one (point, node) pair, with t = xh . e_j and q = (R / r)(R / r_j): start takes degree 0,
// step(f) every degree from 1 in turn with f the entry of that degree, finish returns the unscaled values
//   v = sum_n d_n q^(n+1) P_n       g_c = S_t (e_c - t xh_c) - S_r xh_c,
// to be scaled by GM / R (v) and GM / R / r (g).  alpha_1 = 1, beta_1 = 0 and gamma_1 = 1 make degree 1 an ordinary step from
// P_0 = 1, P_{-1} = 0, P'_0 = P'_{-1} = 0: the loop has no branch.  No fma: every product is rounded before it is added.
struct RbfChain {
    double t, q, qn;                                  // qn = q^(n+1)
    double p1, p2, dp1, dp2;                          // P_{n}, P_{n-1}, P'_{n}, P'_{n-1} after the step of degree n
    double sv, sr, st;
    __device__ void start(const RbfPoint& pt, const double* node, const RbfDegree& f0) {
        t = (pt.xh[0] * node[0] + pt.xh[1] * node[1]) + pt.xh[2] * node[2];
        q = pt.u * node[3];
        qn = q;
        p1 = 1.0;
        p2 = 0.0;
        dp1 = 0.0;
        dp2 = 0.0;
        sv = f0.d * qn;
        sr = f0.e * qn;
        st = 0.0;
    }
    __device__ void step(const RbfDegree& f) {
        const double p = (f.alpha * t) * p1 - f.beta * p2;
        const double dp = dp2 + f.gamma * p1;
        p2 = p1;
        p1 = p;
        dp2 = dp1;
        dp1 = dp;
        qn *= q;
        const double w = qn * p;
        sv = sv + f.d * w;
        sr = sr + f.e * w;
        st = st + f.d * (qn * dp);
    }
    __device__ void finish(const RbfPoint& pt, const double* node, double& v, double g[3]) const {
        v = sv;
#pragma unroll
        for (int c = 0; c < 3; ++c) g[c] = st * (node[c] - t * pt.xh[c]) - sr * pt.xh[c];
    }
};

// The entry of a degree for the second derivatives: RbfDegree and (n + 1)(n + 2) d_n.  A type of its own, so that the table, the
// loads and the registers of the four kinds of rbf_design_kernel stay as they are.
struct RbfDegree2 {
    RbfDegree f;
    double h;                                         // (n + 2) e_n = (n + 1)(n + 2) d_n
};

// The five sums of the Hessian of V_j for one (point, node) pair: S_r and S_t of RbfChain, formed by its operations, and
//   S_rr = sum_n (n + 1)(n + 2) d_n q^(n+1) P_n(t)    S_rt = sum_n (n + 1) d_n q^(n+1) P'_n(t)    S_tt = sum_n d_n q^(n+1) P''_n(t)
// with P''_n = P''_{n-2} + gamma_n P'_{n-1}, the shape of the P' recursion (P''_0 = P''_1 = 0: gamma_1 = 1 times P'_0 = 0 makes degree
// 1 an ordinary step).  start / step / finish as RbfChain; finish returns the six unscaled Earth-fixed entries xx, xy, xz, yy, yz, zz of
//   S_rr xh xh^T - (S_r + t S_t)(I - xh xh^T) - (S_rt + S_t)(xh tau^T + tau xh^T) + S_tt tau tau^T,      tau = e_j - t xh,
// to be scaled by GM / (R r^2).  Nothing divides by sin: tau = 0 above a node and antipodal to it, and the expression is regular there.
// No fma, no branch and no division in step.
struct RbfHessianChain {
    double t, q, qn;                                  // qn = q^(n+1)
    double p1, p2, dp1, dp2, ddp1, ddp2;              // P_n, P_{n-1}, P'_n, P'_{n-1}, P''_n, P''_{n-1} after the step of degree n
    double sr, st, srr, srt, stt;
    __device__ void start(const RbfPoint& pt, const double* node, const RbfDegree2& f0) {
        t = (pt.xh[0] * node[0] + pt.xh[1] * node[1]) + pt.xh[2] * node[2];
        q = pt.u * node[3];
        qn = q;
        p1 = 1.0;
        p2 = 0.0;
        dp1 = 0.0;
        dp2 = 0.0;
        ddp1 = 0.0;
        ddp2 = 0.0;
        sr = f0.f.e * qn;
        srr = f0.h * qn;
        st = 0.0;
        srt = 0.0;
        stt = 0.0;
    }
    __device__ void step(const RbfDegree2& f2) {
        const RbfDegree& f = f2.f;
        const double p = (f.alpha * t) * p1 - f.beta * p2;
        const double dp = dp2 + f.gamma * p1;
        const double ddp = ddp2 + f.gamma * dp1;
        p2 = p1;
        p1 = p;
        dp2 = dp1;
        dp1 = dp;
        ddp2 = ddp1;
        ddp1 = ddp;
        qn *= q;
        const double w = qn * p;
        const double wd = qn * dp;
        sr = sr + f.e * w;
        srr = srr + f2.h * w;
        st = st + f.d * wd;
        srt = srt + f.e * wd;
        stt = stt + f.d * (qn * ddp);
    }
    __device__ void finish(const RbfPoint& pt, const double* node, double T[6]) const {
        double tau[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) tau[c] = node[c] - t * pt.xh[c];
        const double b = sr + t * st, m = srt + st;
        int j = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int d = c; d < 3; ++d, ++j) {
                const double xx = pt.xh[c] * pt.xh[d];
                const double k = c == d ? 1.0 - xx : -xx;
                T[j] = ((srr * xx - b * k) - m * (pt.xh[c] * tau[d] + tau[c] * pt.xh[d])) + stt * (tau[c] * tau[d]);
            }
    }
};

// the entry of degree n from the shape factors k [N + 1]; degrees below min_degree carry d = e = 0 (they still step: the recursions
// need every degree)
inline RbfDegree rbf_degree(int n, int min_degree, const double* k) {
    const double dn = n < min_degree ? 0.0 : k[n] * (2.0 * n + 1.0);
    RbfDegree f;
    f.alpha = n ? (2.0 * n - 1.0) / n : 0.0;
    f.beta = n ? (n - 1.0) / n : 0.0;
    f.gamma = n ? 2.0 * n - 1.0 : 0.0;
    f.d = dn;
    f.e = (n + 1.0) * dn;
    return f;
}

// the entries of degrees 0 .. N: the table of RbfChain and, with h = (n + 2) e_n, that of RbfHessianChain
inline void rbf_degree_table(int N, int min_degree, const double* k, RbfDegree* out) {
    for (int n = 0; n <= N; ++n) out[n] = rbf_degree(n, min_degree, k);
}

inline void rbf_degree_table(int N, int min_degree, const double* k, RbfDegree2* out) {
    for (int n = 0; n <= N; ++n) {
        out[n].f = rbf_degree(n, min_degree, k);
        out[n].h = (n + 2.0) * out[n].f.e;
    }
}

}  // namespace shg

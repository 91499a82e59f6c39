// The column recursion of the solid harmonics at one point, the one every point functional and design matrix runs
// (gravity_points.hip: solid_points_kernel; design.hip: design_harmonics_kernel, potential_design_kernel), and the upload of its
// recursion factors.  The family is tested bit for bit against itself (functional against design matrix times coefficients, pairs
// against single points, batches against series): that holds because the operations below, and their order, exist once.
#pragma once

#include "common.h"

namespace shg {

// Yc_nk = (R/r)^(n+1) P_nk cos(k lon) and Ys_nk = (R/r)^(n+1) P_nk sin(k lon) at one point, one call per step: start, then per
// order k = 0, 1, ... order(k) and per degree n = k, k + 1, ... degree(n, k).  r and the longitude come from xyz as
// grid.cartesian2spherical computes them; (R/r)^(n+1) is carried along the degree loop.  The colatitude has two forms:
//   kDirect false: t = cos(atan2(rho, z)), s = sqrt(1 - t^2), the reference's.  The acceleration, the potential and their design
//     matrices use it: their consumers and the comparisons with the reference depend on its bits.
//   kDirect true: t = z / r, s = rho / r straight from xyz.  The gradient tensor and its design matrix use it: the reference's s is 0
//     within 1.5e-8 rad of the axis, where T_xz = 3 GM x z / r^5 is still up to 2e-8 of max|T|.
template <bool kDirect>
struct SolidColumn {
    double t, s, u, lam, pmm, rk;                     // rk = (R/r)^(k+1)
    double p1, p2, rad, ck, sk;
    __device__ void start(const double* xp, double R) {
        const double x = xp[0], y = xp[1], z = xp[2];
        const double r = sqrt((x * x + y * y) + z * z);              // np.sum over axis 1: ((x^2 + y^2) + z^2)
        lam = atan2(y, x);
        u = R / r;
        if constexpr (kDirect) {
            t = z / r;
            s = sqrt(x * x + y * y) / r;
        } else {
            const double th = atan2(sqrt(x * x + y * y), z);
            t = cos(th);
            s = sqrt(1.0 - t * t);
        }
        pmm = 1.0;
        rk = u;
    }
    // on to order k (every order from 0 in turn): the sectoral seed and (R/r)^(k+1); live: the degrees of this order follow
    __device__ void order(int k, bool live = true) {
        if (k == 1)
            pmm = sqrt(3.0) * s;
        else if (k >= 2)
            pmm = sqrt((2.0 * k + 1.0) / (2.0 * k)) * s * pmm;
        if (k >= 1) rk *= u;
        if (live) {
            sincos((double)k * lam, &sk, &ck);
            p1 = pmm;
            p2 = 0.0;
            rad = rk;
        }
    }
    // degree n of order k (every degree from k in turn): Yc and Ys.  a_b points to (a, b) of (n, k) and is read for n > k only: a
    // pointer, not a value or a reference, so that the element of a table is loaded under that condition, behind a branch that is
    // uniform, as the kernels did before they shared this code (a reference is known to be readable, and the compiler then loads it
    // at the head of every step and selects, which cost the forward kernels 2 to 12 %).  The branch is marked likely so that the step
    // falls through into the caller's sums: laid out of line it cost 1 to 3 % (profiles/solid_fold_time.txt, tables 2 and 3)
    __device__ void degree(int n, int k, const double2* a_b, double& yc, double& ys) {
        if (__builtin_expect(n > k, 1)) {
            const double p = (a_b->x * t) * p1 - a_b->y * p2;
            p2 = p1;
            p1 = p;
        }
        const double pk = p1 * rad;
        rad *= u;
        yc = pk * ck;
        ys = pk * sk;
    }
};

// The recursion factors of degree Nq (host-built, in the reference's expression order) in a buffer of ws, a and b of one (n, k) side
// by side as the kernels read them.  Synchronous (it waits for the stream): the host vectors go out of scope.  fn: the caller, for the
// out-of-memory message.
inline int upload_solid_factors(const char* fn, Workspace& ws, int Nq, hipStream_t stream, double2*& ab) {
    if (!ws.alloc(ab, (size_t)packed_count(Nq))) return fail(SHG_ERR_NOMEM, "%s: workspace allocation failed", fn);
    std::vector<double> a, b;
    recursion_tables(Nq, a, b);
    std::vector<double2> h(a.size());
    for (size_t i = 0; i < a.size(); ++i) h[i] = double2{a[i], b[i]};
    SHG_HIP(hipMemcpyAsync(ab, h.data(), h.size() * sizeof(double2), hipMemcpyHostToDevice, stream));
    SHG_HIP(hipStreamSynchronize(stream));
    return SHG_OK;
}

}  // namespace shg

// What an observation does with the Earth-fixed quantities of a point, the same for the spherical harmonics (design.hip) and the
// radial basis functions (rbf.hip): the line of sight of a satellite pair, and the gradient tensor in its instrument frame with
// the choice of components and their weights.  Device code only, no launches; each rule and its operation order exist once, so
// the two families of design matrices agree on them by construction.
#pragma once

#include "common.h"

namespace shg {

// The line of sight of pair `pt`: e = (b - a) / |b - a| from the positions, |d| = sqrt((dx^2 + dy^2) + dz^2) and one division per
// component, or (from_positions false) directions [npairs][3] as given.
__device__ __forceinline__ void line_of_sight(bool from_positions, const double* __restrict__ xyz_a, const double* __restrict__ xyz_b,
                                              const double* __restrict__ directions, size_t pt, double e[3]) {
    if (from_positions) {
#pragma unroll
        for (int c = 0; c < 3; ++c) e[c] = xyz_b[pt * 3 + c] - xyz_a[pt * 3 + c];
        const double len = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
#pragma unroll
        for (int c = 0; c < 3; ++c) e[c] = e[c] / len;
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) e[c] = directions[pt * 3 + c];
    }
}

// The gradient tensor of a point as its instrument sees it.  start, once per lane: the frame of point `pt` (kFrames: F [3][3], row
// a = instrument axis a) and the square roots of its weights, sw[j] for component j of xx, xy, xz, yy, yz, zz (wl 0: none, 1: w
// [npts], 2: w [npts][K], the K components of `mask` in ascending bit order).  store, once per row or node: from the six
// Earth-fixed entries t, T'_ab = f_a . (T f_b) for the selected components (T f_b once per needed b, sums associated (a + b) + c;
// without frames T' = T), each (value * scale) * sw, to o, o + ldt, ... in ascending bit order.
template <bool kFrames>
struct FrameTensor {
    double F[3][3];
    double sw[6];
    __device__ void start(const double* __restrict__ frames, int mask, int K, const double* __restrict__ w, int wl, size_t pt) {
        if (kFrames) {
#pragma unroll
            for (int i = 0; i < 9; ++i) F[i / 3][i % 3] = frames[pt * 9 + i];
        }
        const double wp = wl == 1 ? sqrt(w[pt]) : 1.0;
        int k = 0;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            sw[j] = wp;
            if ((mask >> j) & 1) {
                if (wl == 2) sw[j] = sqrt(w[pt * K + k]);
                ++k;
            }
        }
    }
    __device__ void store(const double t[6], int mask, double scale, double* o, size_t ldt) const {
        double u[3][3] = {};                                         // u[b] = T f_b
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
};

}  // namespace shg

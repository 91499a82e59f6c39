// Design matrix of the gravitational acceleration at points: the partial derivatives of g (gravity_points.hip) with respect to the
// coefficients, transposed, At [P][3][ldt] with the points innermost and the rows in the degree-wise order of
// utilities.ravel_coefficients (C_n0, C_n1, S_n1, C_n2, ... for n = min_degree .. N).
//
// g is linear in the coefficients and the grouping at the head of gravity_points.hip gives every column directly.  With the solid
// harmonics of degree n' = n + 1,
//   Yc_{n'k} = (R/r)^(n'+1) P_{n'k} cos(k lon)      Ys_{n'k} = (R/r)^(n'+1) P_{n'k} sin(k lon),
// and the factors f-, f0, f+ of (n, m) (f- of order 1 and f+ of order 0 carry the reference's extra sqrt(2)), in units of GM / (2 R^2):
//   d g_x / d C_nm = f- Yc_{n+1,m-1} - f+ Yc_{n+1,m+1}      d g_x / d S_nm =  f- Ys_{n+1,m-1} - f+ Ys_{n+1,m+1}
//   d g_y / d C_nm = -f- Ys_{n+1,m-1} - f+ Ys_{n+1,m+1}     d g_y / d S_nm =  f- Yc_{n+1,m-1} + f+ Yc_{n+1,m+1}
//   d g_z / d C_nm = -2 f0 Yc_{n+1,m}                       d g_z / d S_nm = -2 f0 Ys_{n+1,m}
// (the minus terms exist for m >= 1 only).  No sum over degrees: an entry is one or two products.
//
// Two kernels per pass of points: design_harmonics_kernel runs the column recursion of the forward kernel (SolidColumn of solid.h,
// the one definition both sides share) once per point and writes Y [packed (n', k)][2][ldy] of degree N + 1 to a workspace;
// design_gather_kernel forms every row of At from at most two entries of Y per component, following a host-built table of (slot of
// Y, factor) terms.  The table is all the gather kernel knows about the acceleration: another linear functional of the solid
// harmonics is another table.
//
// The design matrix of the gradient tensor (second half of this file) is that other table, of at most four terms on Y of degree N + 2,
// with a gather kernel of its own that rotates the six entries of a point into a per-point instrument frame and keeps only the
// selected components.
//
// The line-of-sight gravity difference of satellite pairs (third part) needs no table of its own: its gather kernel reads the
// acceleration's table at the two satellites of a pair, takes the difference and projects it on the line of sight.
//
// The potential and the potential difference of satellite pairs (fourth part, the energy-balance observations) need no gather at
// all: an entry is one solid harmonic of degree N, which potential_design_kernel stores straight from the recursion to its row.
//
// The host side is one of each: d_terms is the only host code that uses f-, f0, f+ (both tables are built from it; the formulas
// themselves are in common.h, shared with the forward kernels), design_passes is the pass driver (pass size, workspace, upload of
// recursion factors and table) around the launches of an entry point, and check_design holds the argument checks the entry points share.
#include "observe.h"
#include "solid.h"

#include <cmath>
#include <memory>

namespace shg {

// 256 lanes = 256 points, each running SolidColumn<kDirect> (solid.h: kDirect is the gradient tensor's form of the colatitude, exact
// next to the axis; the acceleration and its design matrix follow the reference's).  The recursion factors a, b of one (n', k) lie
// side by side and are read with wave-uniform addresses: no LDS, whatever the degree.  A launch with gridDim.y = 2 runs two sets of
// npts points, xyz and xyz_second, and writes the second set's harmonics to the columns `second` .. of Y (the two satellites of the
// line-of-sight design); with gridDim.y = 1 neither is looked at.
template <bool kDirect>
__global__ __launch_bounds__(256) void design_harmonics_kernel(int N1, int npts, const double* __restrict__ xyz, const double* __restrict__ xyz_second,
                                                               const double2* __restrict__ ab, double R, double* __restrict__ Y_first, size_t ldy,
                                                               size_t second) {
    const int pt = blockIdx.x * 256 + threadIdx.x;
    const bool ok = pt < npts;
    // blockIdx.y = 1 (the line-of-sight design only): a second set of npts points, whose harmonics go to the columns `second` ..
    double* __restrict__ Y = blockIdx.y ? Y_first + second : Y_first;
    SolidColumn<kDirect> col;
    col.start((blockIdx.y ? xyz_second : xyz) + (size_t)(ok ? pt : 0) * 3, R);
    for (int k = 0; k <= N1; ++k) {
        col.order(k);
        const int off = order_offset(N1, k);
        for (int n = k; n <= N1; ++n) {
            double yc, ys;
            col.degree(n, k, ab + off + n - k, yc, ys);
            if (ok) {
                double* yo = Y + (size_t)(off + n - k) * 2 * ldy + pt;
                yo[0] = yc;
                yo[ldy] = ys;
            }
        }
    }
}

// Row `blockIdx.x` of a transposed design matrix with C components whose entries are sums of at most T terms factor * Y[slot]
// (slot = 2 packed + (0 cosine | 1 sine); slot < 0: no term): out [rows][C][ldt], 256 points per workgroup (blockIdx.y).  The slots
// and factors of a row are wave-uniform.  Every entry is scaled by `scale` and then by the square root of the point's weight
// (wl 0: none, 1: w [npts], 2: w [npts][C]).
template <int C, int T>
__global__ __launch_bounds__(256) void design_gather_kernel(int npts, const double* __restrict__ Y, size_t ldy, const int* __restrict__ slot,
                                                            const double* __restrict__ factor, const double* __restrict__ w, int wl, double scale,
                                                            double* __restrict__ out, size_t ldt) {
    const int pt = blockIdx.y * 256 + threadIdx.x;
    if (pt >= npts) return;
    const size_t row = blockIdx.x;
    const double wp = wl == 1 ? sqrt(w[pt]) : 1.0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        double v = 0.0;
#pragma unroll
        for (int j = 0; j < T; ++j) {
            const int sl = slot[(row * C + c) * T + j];
            if (sl >= 0) v = v + factor[(row * C + c) * T + j] * Y[(size_t)sl * ldy + pt];
        }
        const double sw = wl == 2 ? sqrt(w[(size_t)pt * C + c]) : wp;
        out[(row * C + c) * ldt + pt] = (v * scale) * sw;
    }
}

// ---- the term map ------------------------------------------------------------------------------------------------------------------
// One map serves every table of this file: D_c, the derivative along axis c of a single solid-harmonic coefficient (the grouping at
// the head of gravity_points.hip).  The acceleration's rows are D_c of the unit coefficient, the gradient tensor's D_d of D_c.
struct SolidTerm {
    int n, k, kind;                                   // kind 0: cosine, 1: sine
    double f;
};

// D_c (0: x, 1: y, 2: z) of the single coefficient `in`: the terms of degree in.n + 1, the minus term (order k - 1) before the plus term
static int d_terms(int c, const SolidTerm& in, SolidTerm out[2]) {
    int count = 0;
    const int n = in.n, m = in.k, sine = in.kind;
    auto put = [&](int k, int kind, double value) {
        if (kind == 1 && k == 0) return;                             // Ys of order 0 is zero
        out[count++] = SolidTerm{n + 1, k, kind, in.f * value};
    };
    if (c == 2) {
        put(m, sine, -2.0 * d_factor_zero(n, m));
        return count;
    }
    if (m >= 1) {                                                    // minus term: P_{n+1,m-1}
        const double fm = d_factor_minus(n, m);
        if (c == 0)
            put(m - 1, sine, fm);
        else
            put(m - 1, 1 - sine, sine ? fm : -fm);
    }
    const double fp = d_factor_plus(n, m);                           // plus term: P_{n+1,m+1}
    if (c == 0)
        put(m + 1, sine, -fp);
    else
        put(m + 1, 1 - sine, sine ? fp : -fp);
    return count;
}

// slot of a term in Y of degree Ny: 2 packed(n, k) + kind
static int term_slot(int Ny, const SolidTerm& t) { return 2 * (order_offset(Ny, t.k) + t.n - t.k) + t.kind; }

// the unit coefficient of row j of degree n in the order of utilities.degreewise_array_index: C_n0, C_n1, S_n1, C_n2, ...
static SolidTerm unit_coefficient(int n, int j) { return SolidTerm{n, (j + 1) / 2, (j > 0 && j % 2 == 0) ? 1 : 0, 1.0}; }

// terms of the rows of the acceleration's design matrix, [P][3][2] each (the layout design_gather_kernel<3, 2> and los_design_kernel
// read): D_c of the unit coefficient on Y of degree N + 1, in the order of d_terms, then slot -1 and factor 0.0 (no term)
static void acceleration_design_table(int N, int min_degree, int* slot, double* factor) {
    size_t row = 0;
    for (int n = min_degree; n <= N; ++n) {
        for (int j = 0; j <= 2 * n; ++j, ++row) {
            const SolidTerm unit = unit_coefficient(n, j);
            for (int c = 0; c < 3; ++c) {
                SolidTerm terms[2];
                const int count = d_terms(c, unit, terms);
                for (int i = 0; i < 2; ++i) {
                    slot[(row * 3 + c) * 2 + i] = i < count ? term_slot(N + 1, terms[i]) : -1;
                    factor[(row * 3 + c) * 2 + i] = i < count ? terms[i].f : 0.0;
                }
            }
        }
    }
}

// ---- design matrix of the gradient tensor -------------------------------------------------------------------------------------------
// T = d^2 V / dx_c dx_d is the acceleration's map D (head of gravity_points.hip) applied twice, so its partial derivative with respect
// to one coefficient is a sum of at most four terms factor * Y[slot] on the solid harmonics of degree N + 2, in units of GM / (4 R^3):
// D_c turns the unit coefficient (n, m, kind) into at most two of degree n + 1, D_d each of those into at most two of degree n + 2,
// and terms that meet on one slot (the order m of xx, xy and yy) are merged on the host.
constexpr int kGradTerms = 4;
constexpr int kGradRows = 16;                         // rows of At per workgroup of gradient_design_kernel

// terms of the rows of the gradient tensor's design matrix, [P][6][kGradTerms] each (xx, xy, xz, yy, yz, zz: D_d of D_c, c <= d), rows
// in the order of utilities.degreewise_array_index; slot = 2 packed(n + 2, k) + kind at degree N + 2, -1: no term
static void gradient_design_table(int N, int min_degree, int* slot, double* factor) {
    const int N2 = N + 2;
    size_t row = 0;
    for (int n = min_degree; n <= N; ++n) {
        for (int j = 0; j <= 2 * n; ++j, ++row) {
            const SolidTerm unit = unit_coefficient(n, j);
            int comp = 0;
            for (int c = 0; c < 3; ++c) {
                SolidTerm first[2];
                const int n1 = d_terms(c, unit, first);
                for (int d = c; d < 3; ++d, ++comp) {
                    int* sl = slot + (row * 6 + comp) * kGradTerms;
                    double* f = factor + (row * 6 + comp) * kGradTerms;
                    int used = 0;
                    for (int i = 0; i < kGradTerms; ++i) {
                        sl[i] = -1;
                        f[i] = 0.0;
                    }
                    for (int i = 0; i < n1; ++i) {
                        SolidTerm second[2];
                        const int n2 = d_terms(d, first[i], second);
                        for (int q = 0; q < n2; ++q) {
                            const int s = term_slot(N2, second[q]);
                            int at = 0;
                            while (at < used && sl[at] != s) ++at;
                            if (at == used) sl[used++] = s;
                            f[at] = f[at] + second[q].f;
                        }
                    }
                }
            }
        }
    }
}

// Rows blockIdx.x * kGradRows ... of the transposed design matrix of the gradient tensor, 256 points per workgroup (blockIdx.y):
// out [rows][K][ldt] with the K components of `mask` (bit j: component j of xx, xy, xz, yy, yz, zz) in ascending order.  A lane keeps
// the frame of its point and the square roots of its weights across the rows of the workgroup (FrameTensor of observe.h, shared with
// the radial basis functions: wl 0: none, 1: w [npts], 2: w [npts][K]); per row it forms the six Earth-fixed entries from the table
// (wave-uniform slots and factors) and hands them to FrameTensor::store, which rotates, scales by `scale` and by sqrt(w) and stores.
template <bool kFrames>
__global__ __launch_bounds__(256) void gradient_design_kernel(int npts, long long rows, const double* __restrict__ Y, size_t ldy,
                                                              const int* __restrict__ slot, const double* __restrict__ factor,
                                                              const double* __restrict__ frames, int mask, int K, const double* __restrict__ w, int wl,
                                                              double scale, double* __restrict__ out, size_t ldt) {
    const int pt = blockIdx.y * 256 + threadIdx.x;
    if (pt >= npts) return;
    FrameTensor<kFrames> tensor;
    tensor.start(frames, mask, K, w, wl, (size_t)pt);
    const size_t row0 = (size_t)blockIdx.x * kGradRows;
    const size_t row1 = min((unsigned long long)(row0 + kGradRows), (unsigned long long)rows);
    for (size_t row = row0; row < row1; ++row) {
        double t[6];                                                 // xx, xy, xz, yy, yz, zz in the Earth-fixed frame
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            double v = 0.0;
#pragma unroll
            for (int j = 0; j < kGradTerms; ++j) {
                const int sl = slot[(row * 6 + c) * kGradTerms + j];
                if (sl >= 0) v = v + factor[(row * 6 + c) * kGradTerms + j] * Y[(size_t)sl * ldy + pt];
            }
            t[c] = v;
        }
        tensor.store(t, mask, scale, out + row * K * ldt + pt, ldt);
    }
}

// ---- design matrix of the line-of-sight gravity difference of satellite pairs ---------------------------------------------------------
// l_i = e_i . (g(b_i) - g(a_i)): no new table.  A row is the difference of the acceleration's rows at the two satellites, projected on
// the line of sight of the pair, so the gather kernel reads the terms of acceleration_design_table at two points.
constexpr int kLosRows = 16;                          // rows of At per workgroup of los_design_kernel

// Rows blockIdx.x * kLosRows ... of the transposed design matrix of the line-of-sight difference, 256 pairs per workgroup
// (blockIdx.y): out [rows][ldt].  Y holds the solid harmonics of the pass, those of the a-points in the columns 0 .. and those of the
// b-points in the columns `half` .. of every slot.  A lane keeps the line of sight e and sqrt(w) of its pair across the rows of the
// workgroup.  kUnit: e = (b - a) / |b - a| from the positions, otherwise e = directions [npairs][3] as given (line_of_sight of
// observe.h, shared with the radial basis functions).  Per row (wave-uniform slots and factors) the unscaled component sums at b and at a,
// their difference per component, the projection (e_x d_x + e_y d_y) + e_z d_z, then * scale, then * sqrt(w), one store.
template <bool kUnit>
__global__ __launch_bounds__(256) void los_design_kernel(int npairs, long long rows, const double* __restrict__ xyz_a, const double* __restrict__ xyz_b,
                                                         const double* __restrict__ directions, const double* __restrict__ Y, size_t ldy, size_t half,
                                                         const int* __restrict__ slot, const double* __restrict__ factor, const double* __restrict__ w,
                                                         double scale, double* __restrict__ out, size_t ldt) {
    const int pt = blockIdx.y * 256 + threadIdx.x;
    if (pt >= npairs) return;
    double e[3];
    line_of_sight(kUnit, xyz_a, xyz_b, directions, (size_t)pt, e);
    const double sw = w ? sqrt(w[pt]) : 1.0;
    const double* Ya = Y + pt;
    const double* Yb = Y + half + pt;
    const size_t row0 = (size_t)blockIdx.x * kLosRows;
    const size_t row1 = min((unsigned long long)(row0 + kLosRows), (unsigned long long)rows);
    for (size_t row = row0; row < row1; ++row) {
        double d[3];                                                 // g_c(b) - g_c(a), unscaled
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double va = 0.0, vb = 0.0;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int sl = slot[(row * 3 + c) * 2 + j];
                if (sl >= 0) {
                    const double f = factor[(row * 3 + c) * 2 + j];
                    vb = vb + f * Yb[(size_t)sl * ldy];
                    va = va + f * Ya[(size_t)sl * ldy];
                }
            }
            d[c] = vb - va;
        }
        const double v = (e[0] * d[0] + e[1] * d[1]) + e[2] * d[2];
        out[row * ldt + pt] = (v * scale) * sw;
    }
}

// ---- design matrices of the potential and of the potential difference of satellite pairs ------------------------------------------------
// dV / dC_nm = GM / R Yc_nm and dV / dS_nm = GM / R Ys_nm on the solid harmonics of degree N itself: an entry is one harmonic, so
// there is nothing to gather and no table.  The kernel stores every harmonic straight to its row.
constexpr int kPotLanes = 64;                         // points per workgroup: one wave, whose store covers 64 consecutive doubles of a row
constexpr int kPotOrders = 4;                         // orders per workgroup (blockIdx.y)

// out [P][ldt], transposed: the rows of the orders blockIdx.y * kPotOrders ... at the 64 points (pairs) blockIdx.x * 64 ...  One lane
// is one point; kPairs runs the recursions at a and at b in lockstep and stores Y(b) - Y(a).  The orders below the workgroup's first
// only carry the sectoral seed and (R/r)^(k+1) along, so every workgroup sees the values of the one-pass recursion.  Degrees below
// min_degree are computed and not stored; row(n, k) = n^2 - min_degree^2 + (0 | 2k - 1 cosine | 2k sine).  An entry is
// (Y * scale) * sqrt(w) (w NULL: 1).  No workspace but the recursion factors ab of degree N, read with wave-uniform addresses.
template <bool kPairs>
__global__ __launch_bounds__(kPotLanes) void potential_design_kernel(int N, int min_degree, int npts, const double* __restrict__ xyz_a,
                                                                     const double* __restrict__ xyz_b, const double2* __restrict__ ab,
                                                                     const double* __restrict__ w, double R, double scale, double* __restrict__ out,
                                                                     size_t ldt) {
    constexpr int kSets = kPairs ? 2 : 1;
    const int pt = blockIdx.x * kPotLanes + threadIdx.x;
    const bool ok = pt < npts;
    const size_t at = (size_t)(ok ? pt : 0);
    SolidColumn<false> c[kSets];                                     // the reference's colatitude form, as the forward potential uses
    c[0].start(xyz_a + at * 3, R);
    if (kPairs) c[kSets - 1].start(xyz_b + at * 3, R);
    const double sw = w ? sqrt(w[at]) : 1.0;
    const int k0 = blockIdx.y * kPotOrders, k1 = min(k0 + kPotOrders - 1, N);
    const long long below = (long long)min_degree * min_degree;
    for (int k = 0; k <= k1; ++k) {
        const bool live = k >= k0;
#pragma unroll
        for (int i = 0; i < kSets; ++i) c[i].order(k, live);
        if (!live) continue;
        const int off = order_offset(N, k);
        for (int n = k; n <= N; ++n) {
            const double2 f = ab[off + n - k];
            double yc[kSets], ys[kSets];
#pragma unroll
            for (int i = 0; i < kSets; ++i) c[i].degree(n, k, &f, yc[i], ys[i]);
            if (ok && n >= min_degree) {
                const double vc = kPairs ? yc[kSets - 1] - yc[0] : yc[0];
                double* o = out + (size_t)((long long)n * n - below + (k == 0 ? 0 : 2 * k - 1)) * ldt + pt;
                o[0] = (vc * scale) * sw;
                if (k >= 1) {
                    const double vs = kPairs ? ys[kSets - 1] - ys[0] : ys[0];
                    o[ldt] = (vs * scale) * sw;
                }
            }
        }
    }
}

}  // namespace shg

using namespace shg;

// ---- host side: one pass driver and one set of checks for the three design matrices ---------------------------------------------------
using TableBuilder = void (*)(int N, int min_degree, int* slot, double* factor);

static long long design_rows(int N, int min_degree) { return (long long)(N + 1) * (N + 1) - (long long)min_degree * min_degree; }

// points of one set per pass: Y [packed (n', k)][2][sets * pass] of degree Ny stays under 256 MB (the budget of the acceleration's Q),
// in whole workgroups, at least one.  sets = 2: the two satellites of the line-of-sight design share the budget.
static long long design_pass_points(int Ny, int sets) {
    return std::max<long long>((256LL << 20) / 8 / (2LL * sets * packed_count(Ny)) / 256 * 256, 256);
}

// what a pass of points works with: device buffers that live until design_passes returns
struct DesignPass {
    int pass;                                         // points of one set per pass, the offset of the second set in a column of Y
    size_t ldy;                                       // sets * pass
    double2* ab;                                      // recursion factors of degree Ny, a and b of one (n', k) side by side
    double* Y;
    int* slot;                                        // the table of `build`, [P][entries]
    double* factor;
};

// The scaffolding of a design matrix on the solid harmonics of degree Ny at `sets` (1 | 2) sets of M points: pass size, workspace,
// upload of the recursion factors (solid.h) and of the term table (`entries` per row), a wait for the stream (the host table goes out
// of scope), then launch(pass, p0, np) for the points p0 .. p0 + np of every pass, which enqueues the kernels of its functional.
template <class Launch>
static int design_passes(const char* fn, int Ny, int sets, int N, int min_degree, TableBuilder build, int entries, int M, hipStream_t stream,
                         Launch launch) {
    const size_t table = (size_t)design_rows(N, min_degree) * entries, packed = (size_t)packed_count(Ny);
    DesignPass d;
    d.pass = (int)std::min<long long>({design_pass_points(Ny, sets), ((long long)M + 255) / 256 * 256, 65535LL * 256});
    d.ldy = (size_t)sets * d.pass;
    Workspace ws = Workspace::plain(stream);
    if (!ws.alloc(d.Y, packed * 2 * d.ldy, d.factor, table, d.slot, table)) return fail(SHG_ERR_NOMEM, "%s: workspace allocation failed", fn);
    {
        const std::unique_ptr<double[]> f(new double[table]);        // the builders write every entry, padding included
        const std::unique_ptr<int[]> sl(new int[table]);
        build(N, min_degree, sl.get(), f.get());                     // before anything waits: the stream may still be busy with the caller's
        SHG_HIP(hipMemcpyAsync(d.factor, f.get(), table * sizeof(double), hipMemcpyHostToDevice, stream));
        SHG_HIP(hipMemcpyAsync(d.slot, sl.get(), table * sizeof(int), hipMemcpyHostToDevice, stream));
        // the recursion factors last (built on the host while the two copies run): upload_solid_factors ends in a wait for the stream,
        // which is the one wait of a call and covers the two copies above as well; f and sl depend on that wait.  With the wait in
        // front of the table, NormalEquations.from_gradients lost 5 to 8 % (profiles/solid_fold_time.txt, table 4)
        if (int rc = upload_solid_factors(fn, ws, Ny, stream, d.ab)) {
            (void)hipStreamSynchronize(stream);                      // f and sl must outlive their copies on this path too
            return rc;
        }
    }
    for (int p0 = 0; p0 < M; p0 += d.pass) {
        launch(d, p0, std::min(d.pass, M - p0));
        SHG_HIP(hipGetLastError());
    }
    return SHG_OK;
}

// N and min_degree of a table on the solid harmonics of degree N + above (1 | 2): packed indices of that degree are ints
static int check_design_degrees(const char* fn, int N, int min_degree, int above) {
    SHG_REQUIRE(N >= 0 && min_degree >= 0, "%s: negative size (N %d, min_degree %d)", fn, N, min_degree);
    SHG_REQUIRE(min_degree <= N, "%s: min_degree %d above N %d", fn, min_degree, N);
    SHG_REQUIRE(N <= 32767 - above, "%s: N %d is too large", fn, N);
    return SHG_OK;
}

// What the three entry points check alike, before the first HIP call (the CPU tests call them without a device): the output is
// At [P][K][ldt].  The pointers are the caller's to check, after it has returned SHG_OK for M == 0.
static int check_design(const char* fn, int N, int min_degree, int above, int M, int K, int weight_layout, double GM, double R, int ldt) {
    SHG_REQUIRE(M >= 0, "%s: negative size (M %d)", fn, M);
    if (int rc = check_design_degrees(fn, N, min_degree, above)) return rc;
    SHG_REQUIRE(weight_layout == SHG_WEIGHTS_NONE || weight_layout == SHG_WEIGHTS_POINT || weight_layout == SHG_WEIGHTS_COMPONENT,
                "%s: weight layout %d, expected 0 (none), 1 (per point) or 2 (per component)", fn, weight_layout);
    SHG_REQUIRE(std::isfinite(GM) && std::isfinite(R) && R > 0.0, "%s: GM and R must be finite and R positive (GM %g, R %g)", fn, GM, R);
    SHG_REQUIRE(ldt >= M, "%s: ldt %d below M %d", fn, ldt, M);
    const long long P = design_rows(N, min_degree);
    SHG_REQUIRE(ldt == 0 || P * K <= (1LL << 40) / ldt, "%s: output of %lld x %d x %d values is too large", fn, P, K, ldt);
    return SHG_OK;
}

extern "C" int shg_acceleration_design(int N, int min_degree, const double* xyz, int M, const double* weights, int weight_layout, double GM, double R,
                                       double* At, int ldt, void* stream_) {
    const char* fn = "shg_acceleration_design";
    if (int rc = check_design(fn, N, min_degree, 1, M, 3, weight_layout, GM, R, ldt)) return rc;
    if (M == 0) return SHG_OK;
    SHG_REQUIRE(xyz && At && (weights || weight_layout == SHG_WEIGHTS_NONE), "%s: NULL pointer", fn);
    hipStream_t stream = (hipStream_t)stream_;
    const int N1 = N + 1, wl = weight_layout;
    const unsigned P = (unsigned)design_rows(N, min_degree);
    const double scale = GM / (2.0 * R * R);
    return design_passes(fn, N1, 1, N, min_degree, acceleration_design_table, 3 * 2, M, stream, [&](const DesignPass& d, int p0, int np) {
        hipLaunchKernelGGL(design_harmonics_kernel<false>, dim3(ceil_div(np, 256)), dim3(256), 0, stream, N1, np, xyz + (size_t)p0 * 3, nullptr, d.ab, R, d.Y,
                           d.ldy, (size_t)0);
        const double* w = wl == 0 ? nullptr : weights + (size_t)p0 * (wl == 2 ? 3 : 1);
        hipLaunchKernelGGL((design_gather_kernel<3, 2>), dim3(P, ceil_div(np, 256)), dim3(256), 0, stream, np, d.Y, d.ldy, d.slot, d.factor, w, wl,
                           scale, At + p0, (size_t)ldt);
    });
}

// Host only: no HIP call.
extern "C" int shg_gradient_design_terms(int N, int min_degree, int32_t* slot, double* factor, long long capacity) {
    const char* fn = "shg_gradient_design_terms";
    if (int rc = check_design_degrees(fn, N, min_degree, 2)) return rc;
    const long long P = design_rows(N, min_degree);
    SHG_REQUIRE(capacity >= 6 * kGradTerms * P, "%s: capacity %lld below the %lld entries of the table", fn, capacity, 6 * kGradTerms * P);
    SHG_REQUIRE(slot && factor, "%s: NULL pointer", fn);
    gradient_design_table(N, min_degree, slot, factor);
    return SHG_OK;
}

extern "C" int shg_gradient_design(int N, int min_degree, const double* xyz, int M, const double* frames, int components, const double* weights,
                                   int weight_layout, double GM, double R, double* At, int ldt, void* stream_) {
    const char* fn = "shg_gradient_design";
    SHG_REQUIRE(components >= 1 && components <= 63, "%s: components %d, expected a set of SHG_GRAD_XX ... SHG_GRAD_ZZ (1 .. 63)", fn, components);
    const int mask = components, K = __builtin_popcount((unsigned)mask);
    if (int rc = check_design(fn, N, min_degree, 2, M, K, weight_layout, GM, R, ldt)) return rc;
    if (M == 0) return SHG_OK;
    SHG_REQUIRE(xyz && At && (weights || weight_layout == SHG_WEIGHTS_NONE), "%s: NULL pointer", fn);
    hipStream_t stream = (hipStream_t)stream_;
    const int N2 = N + 2, wl = weight_layout;
    const long long P = design_rows(N, min_degree);
    const unsigned row_groups = (unsigned)ceil_div64(P, kGradRows);
    const double scale = GM / (4.0 * R * R * R);
    return design_passes(fn, N2, 1, N, min_degree, gradient_design_table, 6 * kGradTerms, M, stream, [&](const DesignPass& d, int p0, int np) {
        hipLaunchKernelGGL(design_harmonics_kernel<true>, dim3(ceil_div(np, 256)), dim3(256), 0, stream, N2, np, xyz + (size_t)p0 * 3, nullptr, d.ab, R, d.Y,
                           d.ldy, (size_t)0);
        const double* w = wl == 0 ? nullptr : weights + (size_t)p0 * (wl == 2 ? K : 1);
        const dim3 grid(row_groups, ceil_div(np, 256));
        if (frames)
            hipLaunchKernelGGL(gradient_design_kernel<true>, grid, dim3(256), 0, stream, np, P, d.Y, d.ldy, d.slot, d.factor, frames + (size_t)p0 * 9, mask,
                               K, w, wl, scale, At + p0, (size_t)ldt);
        else
            hipLaunchKernelGGL(gradient_design_kernel<false>, grid, dim3(256), 0, stream, np, P, d.Y, d.ldy, d.slot, d.factor, nullptr, mask, K, w, wl, scale,
                               At + p0, (size_t)ldt);
    });
}

// Host only: no HIP call.  Pairs per pass of shg_los_design at degree N (before the call's own M caps it), -1 for a degree it refuses.
extern "C" int shg_los_design_pass(int N) {
    if (N < 0 || N > 32766) return -1;
    return (int)design_pass_points(N + 1, 2);
}

extern "C" int shg_los_design(int N, int min_degree, const double* xyz_a, const double* xyz_b, const double* directions, int M, const double* weights,
                              double GM, double R, double* At, int ldt, void* stream_) {
    const char* fn = "shg_los_design";
    // weights are per pair or absent: there is no layout argument, so the layout check of check_design cannot fail here
    if (int rc = check_design(fn, N, min_degree, 1, M, 1, weights ? SHG_WEIGHTS_POINT : SHG_WEIGHTS_NONE, GM, R, ldt)) return rc;
    if (M == 0) return SHG_OK;
    SHG_REQUIRE(xyz_a && xyz_b && At, "%s: NULL pointer", fn);
    hipStream_t stream = (hipStream_t)stream_;
    const int N1 = N + 1;
    const long long P = design_rows(N, min_degree);
    const unsigned row_groups = (unsigned)ceil_div64(P, kLosRows);
    const double scale = GM / (2.0 * R * R);
    // the acceleration's table, read at both satellites: a-points in the columns 0 .. of Y, b-points in the columns pass ..
    return design_passes(fn, N1, 2, N, min_degree, acceleration_design_table, 3 * 2, M, stream, [&](const DesignPass& d, int p0, int np) {
        const double *xa = xyz_a + (size_t)p0 * 3, *xb = xyz_b + (size_t)p0 * 3;
        // one launch for both satellites (blockIdx.y): the kernel's time hardly depends on the number of workgroups at these sizes
        hipLaunchKernelGGL(design_harmonics_kernel<false>, dim3(ceil_div(np, 256), 2), dim3(256), 0, stream, N1, np, xa, xb, d.ab, R, d.Y, d.ldy,
                           (size_t)d.pass);
        const double* w = weights ? weights + p0 : nullptr;
        const dim3 grid(row_groups, ceil_div(np, 256));
        if (directions)
            hipLaunchKernelGGL(los_design_kernel<false>, grid, dim3(256), 0, stream, np, P, xa, xb, directions + (size_t)p0 * 3, d.Y, d.ldy, (size_t)d.pass,
                               d.slot, d.factor, w, scale, At + p0, (size_t)ldt);
        else
            hipLaunchKernelGGL(los_design_kernel<true>, grid, dim3(256), 0, stream, np, P, xa, xb, nullptr, d.Y, d.ldy, (size_t)d.pass, d.slot, d.factor, w,
                               scale, At + p0, (size_t)ldt);
    });
}

// The potential's two design matrices: the checks they share with the others, then one launch that covers all points (no Y, no
// table, no passes; the recursion factors of degree N are the only workspace).  Weights are per point or absent, as in shg_los_design:
// the layout check of check_design cannot fail here.
template <bool kPairs>
static int potential_design(const char* fn, int N, int min_degree, const double* xyz_a, const double* xyz_b, int M, const double* weights, double GM,
                            double R, double* At, int ldt, hipStream_t stream) {
    if (int rc = check_design(fn, N, min_degree, 0, M, 1, weights ? SHG_WEIGHTS_POINT : SHG_WEIGHTS_NONE, GM, R, ldt)) return rc;
    if (M == 0) return SHG_OK;
    SHG_REQUIRE(xyz_a && (xyz_b || !kPairs) && At, "%s: NULL pointer", fn);
    Workspace ws = Workspace::plain(stream);
    double2* ab;
    if (int rc = upload_solid_factors(fn, ws, N, stream, ab)) return rc;
    hipLaunchKernelGGL(potential_design_kernel<kPairs>, dim3(ceil_div(M, kPotLanes), ceil_div(N + 1, kPotOrders)), dim3(kPotLanes), 0, stream, N, min_degree,
                       M, xyz_a, xyz_b, ab, weights, R, GM / R, At, (size_t)ldt);
    SHG_HIP(hipGetLastError());
    return SHG_OK;
}

extern "C" int shg_potential_design(int N, int min_degree, const double* xyz, int M, const double* weights, double GM, double R, double* At, int ldt,
                                    void* stream) {
    return potential_design<false>("shg_potential_design", N, min_degree, xyz, nullptr, M, weights, GM, R, At, ldt, (hipStream_t)stream);
}

extern "C" int shg_potential_difference_design(int N, int min_degree, const double* xyz_a, const double* xyz_b, int M, const double* weights, double GM,
                                               double R, double* At, int ldt, void* stream) {
    return potential_design<true>("shg_potential_difference_design", N, min_degree, xyz_a, xyz_b, M, weights, GM, R, At, ldt, (hipStream_t)stream);
}

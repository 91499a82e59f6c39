// Fused batched synthesis for grids whose meridians are invariant under lon -> -lon and under R rotations lon -> lon + 2 pi k / R
// (an equi-angular cell-centred grid, grates/grid.py:1146-1151, with nlon a multiple of 2 R): every column of the fundamental
// domain mu_c = (c + 1/2) dlon, c = 0 .. nlon / (2 R) - 1, has 2 R images s mu_c + 2 pi k / R, s = +-1, k = 0 .. R - 1.
//
// Same structure as synthesis_fused.hip (one workgroup = 4 epochs x 16 parallels; Legendre stage on MFMA into an LDS panel,
// longitude stage on MFMA out of it), but the longitude stage evaluates its trigonometric sums on the fundamental domain only
// and forms the 2 R images of a column in registers: the epilogue does the radix-R step of a decimation-in-frequency FFT, the
// MFMAs the remaining DFT of nlon / (2 R) points.
//
// Orders m >= 1 fall into classes r = min(m mod R, R - m mod R) with sign s_m = +1 (m mod R <= R / 2) or -1, because
//     cos(2 pi m k / R) = cos(2 pi r k / R),   sin(2 pi m k / R) = s_m sin(2 pi r k / R).
// With the panel holding A_m = sum_n C_nm PK_nm and B'_m = s_m sum_n S_nm PK_nm (the sign is folded into the coefficient
// repack) and the table T1 = cos(m mu), T2 = s_m sin(m mu), the sums per class
//     CA = A T1,  SA = A T2,  CB = B' T1,  SB = B' T2          (r = 0 and r = R / 2 need CA and SB only)
// give
//     f(s mu + 2 pi k / R) = sum_r cos(2 pi r k / R) (CA_r + s SB_r) + sin(2 pi r k / R) (CB_r - s SA_r).
//
// R is chosen so that the images of a 16-column tile are whole 128-byte lines of the grid: nlon / R must be a multiple of 16.
//   R = 6 (12 images; nlon % 96 == 0: the 0.25 degree grid): classes 0, 3 (two sums) and 1, 2 (four sums) = 12 accumulators per
//          16 rows x 16 columns, 80 MFMAs at d/o 96 where the 4-fold kernel of synthesis_fused.hip issues 144 for the same outputs.
// Measured on the way (d/o 96 -> 0.25 degree): R = 8 (16 images, 84 MFMAs for 16 x 16 x 16 outputs) computes faster but its
// images start at multiples of nlon / 8 = 180 columns, i.e. at 32-byte instead of 128-byte boundaries, and the partial lines
// cost more HBM time than the MFMAs save (0.9 - 1.3 ms against 0.63 ms with the same stores forced onto line boundaries).
//
// Operands of the longitude stage: A fragments (A_m, B'_m) come from the panel with one ds_read_b128 per k-step, B fragments
// (T1, T2) are streamed from L2 by LDS-DMA (global_load_lds_dwordx4, 1 KB per wave-instruction) into a private ring of six
// 1 KB slots per wave, five pieces ahead of their use, and read back with one ds_read_b128: no registers are tied up by the
// prefetch and the loop needs no compile-time knowledge of the class lengths.  The fragments of k-step p + 1 are read while
// the MFMAs of k-step p run (two named register sets).
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "common.h"

#ifndef SHG_STORE_AUX
#define SHG_STORE_AUX 2          // nt: the grids are streamed out and never re-read (see synthesis_fused.hip)
#endif

namespace shg {

typedef double double2_t __attribute__((ext_vector_type(2)));
typedef unsigned int uint4_t __attribute__((ext_vector_type(4)));

#ifndef SHG_ROT_PREFERENCE
#define SHG_ROT_PREFERENCE 10, 9, 6, 3
#endif
#ifndef SHG_ROT_WAVES
#define SHG_ROT_WAVES 8          // waves per workgroup.  12 (three per SIMD; the kernel needs 143 registers, no spill at 168; ring
#endif                           // depth 3 to fit the LDS) measured the same 0.525 ms: the fp64 issue pipe is the bound, not occupancy
#ifndef SHG_RING_DEPTH
#define SHG_RING_DEPTH (SHG_ROT_WAVES > 8 ? 3 : 5)
#endif
constexpr int kWaves = SHG_ROT_WAVES;
constexpr int kColStride = kWaves / 4;              // column tiles of a wave: wave >> 2, + kColStride, ...
constexpr int kRingDepth = SHG_RING_DEPTH;         // trig pieces in flight per wave
constexpr int kRingSlots = kRingDepth + 1;          // ring slots (1 KB each) per wave
constexpr int kRingDoubles = kWaves * kRingSlots * 128;  // the rings of the waves sit at the start of the LDS (DMA offsets < 64 KB)
constexpr int kMaxClasses = kRotMaxClasses;

// class layout for R rotations: classes r = 0 .. R / 2; in the K sequence the two-sum classes come first (r = 0, and r = R / 2 for
// even R), then r = 1, 2, ... with four sums each: 2 R accumulators per 16 rows x 16 columns, which the epilogue turns into the
// 2 R images in place
template <int R>
struct RotTraits {
    static constexpr int kClasses = R / 2 + 1, kTwo = R % 2 == 0 ? 2 : 1, kAcc = 2 * R;
    // accumulators of class r: (CA, SB) at a(r) for the two-sum classes, (CA, SA, CB, SB) at a(r) for the others
    static constexpr int acc_of(int r) { return r == 0 ? 0 : (R % 2 == 0 && 2 * r == R) ? 2 : 2 * kTwo + 4 * (r - 1); }
    static constexpr bool two_sums(int r) { return r == 0 || 2 * r == R; }
    // behind rot_split: X_r(s) and Y_r(s) (-1: the class has none), s = 0 for the sign +1 and 1 for the sign -1, in the accumulators of
    // their class -- X(+) for CA, X(-) for SB, Y(+) for CB, Y(-) for SA --, and the accumulator that rot_half leaves image k of sign s in:
    // the k-th of the sign's own R accumulators (X_0, X_(R/2) for even R, then X_1, Y_1, X_2, Y_2, ...)
    static constexpr int x_of(int r, int s) { return acc_of(r) + (two_sums(r) ? s : 3 * s); }
    static constexpr int y_of(int r, int s) { return two_sums(r) ? -1 : acc_of(r) + 2 - s; }
    static constexpr int img_of(int k, int s) { return k < kTwo ? x_of(k == 0 ? 0 : R / 2, s) : (k - kTwo) % 2 == 0 ? x_of(1 + (k - kTwo) / 2, s) : y_of(1 + (k - kTwo) / 2, s); }
};

struct RotParams {
    int N, nlat, nlon, B, nit, nh;
    int nd;                   // columns of the fundamental domain = nlon / (2 R)
    int nct;                  // column tiles of 16
    int half_fold;            // 1: nd % 16 == 8 and the last column tile runs on the 16 real columns nd - 8 .. nd + 7, ascending images only (rot_phase2)
    int npieces;              // trig pieces (k-steps) per column tile = sum of cls_nk
    int cls_nk[kMaxClasses];  // k-steps (4 orders each) of the classes in K order; their panel slots follow each other: class c starts at 4 * (nk[0] + .. + nk[c-1])
    int cls_cnt[kMaxClasses]; // orders in each class (the slots up to 4 * cls_nk are zero padding)
    int nslot;                // panel slots of the orders >= 1 = 4 * npieces; order 0 sits in slot nslot
#ifdef SHG_EXPERIMENT
    int dbg;                  // experiment switches (SHG_DEBUG): 1 no stores, 2 no Legendre stage, 4 no longitude stage
    int stagger;              // SHG_STAGGER: the first 256 workgroups start up to this many 10 ns ticks late (spread in 32 steps)
    int stagger2;             // SHG_STAGGER2: waves 4 .. 7 enter the longitude stage this many 10 ns ticks behind waves 0 .. 3
#endif
    int Qtot;
    const double* cpk4;       // repacked coefficients (see synthesis_fused.hip), S_nm negated where s_m = -1
    const double* pkf;
    const int4* itemtab;
    int nrec, ntrip;
    int* tickets;             // ticket queues of the Legendre stage, one 128-byte line per XCD: {tickets handed out, stages finished}, 0 between launches
    int xcd_limit;            // at most this many workgroups of one XCD run their Legendre stage at the same time (0 = no limit)
#ifdef SHG_TIMELINE
    unsigned long long* tl;
#endif
    const int* blockmap;
    const int* badmap;
    const double* trig;       // [column tile][npieces][64 lanes][2]: (cos(m mu), s_m sin(m mu)) of order slot 4 ks + lane / 16, column 16 ct + lane % 16
    const int* levtab;        // [nit][kRotLevelInts] order pruning: layout, trig stream and item table of every latitude block (common.h); the fields
                              // npieces, cls_nk, cls_cnt, nslot, nrec, ntrip, trig and itemtab above hold the full level and are replaced by the block's
    double* G;
};

#ifdef SHG_TIMELINE
#define ROT_STAMP(ev)                                                                                         \
    do {                                                                                                      \
        if (P.tl && lane == 0) P.tl[((size_t)blockIdx.x * kWaves + wave) * 16 + (ev)] = wall_clock64();            \
        if (P.tl && lane == 0 && ((ev) == 0 || (ev) == 12))                                                   \
            P.tl[((size_t)blockIdx.x * kWaves + wave) * 16 + ((ev) == 0 ? 13 : 14)] = __builtin_amdgcn_s_memtime();  \
    } while (0)
#else
#define ROT_STAMP(ev)
#endif

// LDS-DMA of one 1 KB piece: lane l copies 16 bytes from gbase + lane_off to LDS address lds_addr + 16 l.
// M0 is overwritten and not restored: hipcc treats it as a reserved register that it loads right in front of every use of
// its own (it refuses it in a clobber list for that reason), and gfx9 LDS instructions do not read it -- saving and restoring it
// around every piece cost three scalar instructions and five idle cycles per k-step.  The s_nop covers the scalar write of M0
// in front of its use by the vector memory instruction.
__device__ __forceinline__ void glds16(const double* gbase, unsigned lane_off, unsigned lds_addr) {
    asm volatile(
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %0, %1"
        :
        : "v"(lane_off), "s"(gbase), "s"(lds_addr)
        : "memory");
}

#ifndef SHG_ROT_X
#define SHG_ROT_X 0          // experiment switches (timing only): 1 no issue-side stream bookkeeping, 2 no consumer-side bookkeeping
#endif

typedef int int4_s __attribute__((ext_vector_type(4)));

// 8-byte non-temporal buffer store with the wave-uniform part of the address in the SCALAR offset (no vector add per store), as
// inline asm.  The scalar offset travels through M0, written by an SALU instruction of the statement itself: hipcc reloads
// spilled scalars with v_readlane right in front of an asm statement, and an SGPR written by the VALU needs five wait states
// before a vector memory instruction may read it -- an SALU read does not.  (M0 is free: gfx9 LDS instructions do not read it,
// and every LDS-DMA of the trig stream sets it in its own statement.)  Stores of at most 8 bytes have no store-data hazard.
__device__ __forceinline__ void store_b64_soff(double v, int4_s rsrc, unsigned voff, unsigned soff) {
    asm volatile("s_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_store_dwordx2 %0, %1, %2, m0 offen nt"
                 :
                 : "v"(v), "v"(voff), "s"(rsrc), "s"(soff)
                 : "memory");
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"i"(N) : "memory");
    __builtin_amdgcn_sched_barrier(0);
}

// The 2 R images of one (row, column) from its sums, in place and in two steps.  rot_split turns the sums of every class into
// X_r(s) = CA_r + s SB_r and Y_r(s) = CB_r - s SA_r for both signs (RotTraits::x_of, y_of): from then on the sign s = +1 (ascending
// columns) and the sign s = -1 (descending columns) own R accumulators each.  rot_half<R, S> forms the R images of one sign from that
// sign's R accumulators and leaves image k in accumulator RotTraits::img_of(k, S): the folded last column tile (rot_phase2) never
// runs the half of s = -1.  Every image is the same expression of the same sums whichever halves run, hence the same bits.
template <int R>
__device__ __forceinline__ void rot_split(double4_t* acc, int r) {
    using T = RotTraits<R>;
#pragma unroll
    for (int c = 0; c <= R / 2; ++c) {
        const int a = T::acc_of(c);
        if (T::two_sums(c)) {
            const double ca = acc[a][r], sb = acc[a + 1][r];
            acc[T::x_of(c, 0)][r] = ca + sb;
            acc[T::x_of(c, 1)][r] = ca - sb;
        } else {
            const double ca = acc[a][r], sa = acc[a + 1][r], cb = acc[a + 2][r], sb = acc[a + 3][r];
            acc[T::x_of(c, 0)][r] = ca + sb;
            acc[T::y_of(c, 0)][r] = cb - sa;
            acc[T::x_of(c, 1)][r] = ca - sb;
            acc[T::y_of(c, 1)][r] = cb + sa;
        }
    }
}

// R = 6, classes 0, 3 (two sums) and 1, 2.  With g = sqrt(3) / 2:
//   E_0 = X_0 + X_2,  E_1 = X_0 - X_2 / 2 + g Y_2,  E_2 = X_0 - X_2 / 2 - g Y_2        (classes 0, 2: period 3 in k)
//   O_0 = X_1 + X_3,  O_1 = X_1 / 2 + g Y_1 - X_3,  O_2 = -X_1 / 2 + g Y_1 + X_3       (classes 1, 3: O_(k+3) = -O_k)
//   f_k = E_k + O_k,  f_(k+3) = E_k - O_k,  k = 0, 1, 2.
template <int S>
__device__ __forceinline__ void rot_half6(double4_t* acc, int r) {
    using T = RotTraits<6>;
    constexpr double g = 0.86602540378443864676;
    const double x0 = acc[T::x_of(0, S)][r], x3 = acc[T::x_of(3, S)][r];
    const double x1 = acc[T::x_of(1, S)][r], y1 = acc[T::y_of(1, S)][r];
    const double x2 = acc[T::x_of(2, S)][r], y2 = acc[T::y_of(2, S)][r];
    const double t = fma(-0.5, x2, x0);
    const double e0 = x0 + x2, e1 = fma(g, y2, t), e2 = fma(-g, y2, t);
    const double u = fma(0.5, x1, -x3);
    const double o0 = x1 + x3, o1 = fma(g, y1, u), o2 = fma(g, y1, -u);
    acc[T::img_of(0, S)][r] = e0 + o0;
    acc[T::img_of(3, S)][r] = e0 - o0;
    acc[T::img_of(1, S)][r] = e1 + o1;
    acc[T::img_of(4, S)][r] = e1 - o1;
    acc[T::img_of(2, S)][r] = e2 + o2;
    acc[T::img_of(5, S)][r] = e2 - o2;
}

// R = 3, classes 0 (two sums) and 1:  f_0 = X_0 + X_1,  f_1,2 = X_0 - X_1 / 2 +- g Y_1.
template <int S>
__device__ __forceinline__ void rot_half3(double4_t* acc, int r) {
    using T = RotTraits<3>;
    constexpr double g = 0.86602540378443864676;
    const double x0 = acc[T::x_of(0, S)][r];
    const double x1 = acc[T::x_of(1, S)][r], y1 = acc[T::y_of(1, S)][r];
    const double t = fma(-0.5, x1, x0);
    acc[T::img_of(0, S)][r] = x0 + x1;
    acc[T::img_of(1, S)][r] = fma(g, y1, t);
    acc[T::img_of(2, S)][r] = fma(-g, y1, t);
}

// R = 9, classes 0 (two sums) and 1 .. 4.  With c_j = cos(40 j deg), s_j = sin(40 j deg)
// (c_3 = -1/2, s_3 = sqrt(3) / 2) and C_k = X_0 + sum_r c_(rk mod 9) X_r, S_k = sum_r s_(rk mod 9) Y_r:
//   f_0 = X_0 + X_1 + X_2 + X_3 + X_4,   f_k = C_k + S_k,   f_(9-k) = C_k - S_k,   k = 1 .. 4.
template <int S>
__device__ __forceinline__ void rot_half9(double4_t* acc, int r) {
    using T = RotTraits<9>;
    constexpr double c1 = 0.76604444311897803520, c2 = 0.17364817766693034885, c4 = -0.93969262078590838405;
    constexpr double s1 = 0.64278760968653932632, s2 = 0.98480775301220805937, s3 = 0.86602540378443864676, s4 = 0.34202014332566873304;
    const double x0 = acc[T::x_of(0, S)][r];
    const double x1 = acc[T::x_of(1, S)][r], x2 = acc[T::x_of(2, S)][r], x3 = acc[T::x_of(3, S)][r], x4 = acc[T::x_of(4, S)][r];
    const double y1 = acc[T::y_of(1, S)][r], y2 = acc[T::y_of(2, S)][r], y3 = acc[T::y_of(3, S)][r], y4 = acc[T::y_of(4, S)][r];
    const double t = (x1 + x2) + x4, x03 = x0 + x3;
    const double h = fma(-0.5, x3, x0), u = s3 * y3;
    const double C1 = fma(c1, x1, fma(c2, x2, fma(c4, x4, h)));
    const double C2 = fma(c2, x1, fma(c4, x2, fma(c1, x4, h)));
    const double C3 = fma(-0.5, t, x03);
    const double C4 = fma(c4, x1, fma(c1, x2, fma(c2, x4, h)));
    const double S1 = fma(s1, y1, fma(s2, y2, fma(s4, y4, u)));
    const double S2 = fma(s2, y1, fma(s4, y2, fma(-s1, y4, -u)));
    const double S3 = s3 * ((y1 - y2) + y4);
    const double S4 = fma(s4, y1, fma(-s1, y2, fma(-s2, y4, u)));
    acc[T::img_of(0, S)][r] = x03 + t;
    acc[T::img_of(1, S)][r] = C1 + S1;
    acc[T::img_of(8, S)][r] = C1 - S1;
    acc[T::img_of(2, S)][r] = C2 + S2;
    acc[T::img_of(7, S)][r] = C2 - S2;
    acc[T::img_of(3, S)][r] = C3 + S3;
    acc[T::img_of(6, S)][r] = C3 - S3;
    acc[T::img_of(4, S)][r] = C4 + S4;
    acc[T::img_of(5, S)][r] = C4 - S4;
}

// R = 10, classes 0, 5 (two sums) and 1 .. 4.  With c1 = cos 36, c2 = cos 72,
// s1 = sin 36, s2 = sin 72 (degrees): the even classes have period 5 in k, the odd ones change sign after 5 steps,
//   E_0 = X_0 + X_2 + X_4,  E_1,4 = (X_0 + c2 X_2 - c1 X_4) +- (s2 Y_2 + s1 Y_4),  E_2,3 = (X_0 - c1 X_2 + c2 X_4) +- (s1 Y_2 - s2 Y_4)
//   O_0 = X_1 + X_3 + X_5,  O_1,4 = (s1 Y_1 + s2 Y_3) +- (c1 X_1 - c2 X_3 - X_5),  O_2,3 = (s2 Y_1 - s1 Y_3) +- (c2 X_1 - c1 X_3 + X_5)
//   f_k = E_k + O_k,  f_(k+5) = E_k - O_k,  k = 0 .. 4.
template <int S>
__device__ __forceinline__ void rot_half10(double4_t* acc, int r) {
    using T = RotTraits<10>;
    constexpr double c1 = 0.80901699437494742410, c2 = 0.30901699437494742410;
    constexpr double s1 = 0.58778525229247312917, s2 = 0.95105651629515357212;
    const double x0 = acc[T::x_of(0, S)][r], x5 = acc[T::x_of(5, S)][r];
    const double x1 = acc[T::x_of(1, S)][r], x2 = acc[T::x_of(2, S)][r], x3 = acc[T::x_of(3, S)][r], x4 = acc[T::x_of(4, S)][r];
    const double y1 = acc[T::y_of(1, S)][r], y2 = acc[T::y_of(2, S)][r], y3 = acc[T::y_of(3, S)][r], y4 = acc[T::y_of(4, S)][r];
    const double e0 = (x0 + x2) + x4;
    const double a1 = fma(c2, x2, fma(-c1, x4, x0)), b1 = fma(s2, y2, s1 * y4);
    const double a2 = fma(-c1, x2, fma(c2, x4, x0)), b2 = fma(s1, y2, -(s2 * y4));
    const double e1 = a1 + b1, e4 = a1 - b1, e2 = a2 + b2, e3 = a2 - b2;
    const double o0 = (x1 + x3) + x5;
    const double p = fma(c1, x1, fma(-c2, x3, -x5)), q = fma(s1, y1, s2 * y3);
    const double u = fma(c2, x1, fma(-c1, x3, x5)), v = fma(s2, y1, -(s1 * y3));
    const double o1 = q + p, o4 = q - p, o2 = v + u, o3 = v - u;
    acc[T::img_of(0, S)][r] = e0 + o0;
    acc[T::img_of(5, S)][r] = e0 - o0;
    acc[T::img_of(1, S)][r] = e1 + o1;
    acc[T::img_of(6, S)][r] = e1 - o1;
    acc[T::img_of(2, S)][r] = e2 + o2;
    acc[T::img_of(7, S)][r] = e2 - o2;
    acc[T::img_of(3, S)][r] = e3 + o3;
    acc[T::img_of(8, S)][r] = e3 - o3;
    acc[T::img_of(4, S)][r] = e4 + o4;
    acc[T::img_of(9, S)][r] = e4 - o4;
}

template <int R, int S>
__device__ __forceinline__ void rot_half(double4_t* acc, int r) {
    static_assert(R == 10 || R == 9 || R == 6 || R == 3, "no butterfly for this rotation count");
    if constexpr (R == 10) rot_half10<S>(acc, r);
    else if constexpr (R == 9) rot_half9<S>(acc, r);
    else if constexpr (R == 6) rot_half6<S>(acc, r);
    else rot_half3<S>(acc, r);
}

// Trig stream and fragment registers of one consumer wave; in the persistent kernel they live across tiles.
struct RotStream {
    const double* iptr;       // next piece to issue
    const double* ibase;      // first piece of the column tile being issued
    const double* ifirst;     // first piece of the wave's first column tile (wave >> 2), ilast: of its last one
    const double* ilast;
    int irem;                 // pieces of the current column tile left to issue
    unsigned im0, ring_lds;   // LDS address of the next ring slot to fill / of the wave's first slot
    int cslot, pf;            // ring slot / k-step (inside its unit) of the next fetch
    double2_t tx, abx;        // fragments of the next k-step to compute
};

// The issue side walks the column tiles of its wave on its own: (wave >> 2), + 2, ..., then again from the start for the next tile.
// EP = epochs (= row tiles) of the workgroup: eight waves, one workgroup per CU
constexpr int EP = 4;
__device__ __forceinline__ void rot_stream_init(RotStream& S, const RotParams& P, const double* As, int wave) {
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) const void*)As;
    S.ring_lds = lds0 + (unsigned)wave * (kRingSlots * 1024);
    S.im0 = S.ring_lds;
    const int ct0 = min(wave / EP, P.nct - 1);
    const int nq = (P.nct - ct0 + kColStride - 1) / kColStride;     // column tiles of this wave
    S.ifirst = P.trig + (size_t)ct0 * P.npieces * 128;
    S.ilast = S.ifirst + (size_t)(nq - 1) * kColStride * P.npieces * 128;
    S.ibase = S.ifirst;
    S.iptr = S.ifirst;
    S.irem = P.npieces;
    S.cslot = 0;
    S.pf = 0;
    S.tx = (double2_t){0.0, 0.0};
    S.abx = (double2_t){0.0, 0.0};
}

__device__ __forceinline__ void rot_issue_piece(RotStream& S, const RotParams& P, unsigned lane_off) {
    glds16(S.iptr, lane_off, S.im0);
#if defined(SHG_ROT_X) && (SHG_ROT_X & 1)
    return;                                        // experiment: no stream bookkeeping (timing only, wrong results)
#endif
    S.im0 = S.im0 + 1024 == S.ring_lds + kRingSlots * 1024 ? S.ring_lds : S.im0 + 1024;
    const bool more = S.irem > 1;
    const double* nbase = S.ibase == S.ilast ? S.ifirst : S.ibase + kColStride * P.npieces * 128;
    S.ibase = more ? S.ibase : nbase;
    S.iptr = more ? S.iptr + 128 : nbase;
    S.irem = more ? S.irem - 1 : P.npieces;
}

// Longitude stage + epilogue of one wave for the tile (bt, it).  A unit = (row tile wave & 3, column tile ct), ct = wave >> 2,
// (wave >> 2) + kColStride, ...  (Taking the column tiles of a row tile from a common counter, so that the older wave of a SIMD, which
// wins every MFMA issue slot and runs ~1.3 times faster, takes more of them, measured 16 % slower: the four waves that work
// on the same column tile then drift apart and no longer share the trig pieces in the L1.)
// On entry (S.tx, S.abx) hold the fragments of the first k-step; on exit those of the first k-step of column tile wave >> 2
// again (trig part; the panel part is re-read by the caller once the next panel is there).
template <bool NS, int R>
__device__ __forceinline__ void rot_phase2(const RotParams& P, const double* As, const double2_t* panel, RotStream& S, int wave, int lane,
                                           int b0, int it) {
    constexpr int PR = 16 * EP;                        // panel rows
    using T = RotTraits<R>;
    const int fr = lane & 15, fk = lane >> 4;
    const int i0 = it * 16, i0n = it * 8;
    const unsigned lane_off = (unsigned)lane * 16u;
    auto grid_row = [&](int s) { return NS ? (s < 8 ? i0n + s : P.nlat - 1 - (i0n + s - 8)) : i0 + s; };
    auto slot_valid = [&](int s) { return NS ? i0n + (s & 7) < P.nh : i0 + s < P.nlat; };

    const int grid_bytes = P.nlat * P.nlon * 8;        // one epoch's grid; < 2^31 (checked on the host)
    const int n2 = P.nlon >> 1, nR = P.nlon / R;
    const double2_t* const ringp = reinterpret_cast<const double2_t*>(As) + wave * (kRingSlots * 64) + lane;   // + slot * 64
    // all units of a wave lie in the same row tile
    const int rt = wave % EP;
    const double2_t* const prow = panel + rt * 16 + fr + fk * PR;        // + 4 PR p: k-step p of the flat class sequence
    // Fragments of the next k-step of the flat (unit, k-step) sequence -> (T_, AB_): one more trig piece issued, the piece of
    // this k-step waited for, ring slot and panel rows read.  Branch-free and unconditional (after the last k-step of the last
    // unit it re-reads valid memory), so that hipcc keeps exact lgkmcnt counts across the loops: the MFMAs of k-step p then
    // wait for their own fragments only (lgkmcnt(2)), not for the reads of k-step p + 1 issued just before them.
    // The wait is always the strict one (all but the kRingDepth youngest operations done): stores of the previous epilogue
    // that are still in flight are waited for too, which measured no different from counting them out.
#define ROT_FETCH(T_, AB_)                                                                                \
    do {                                                                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        if (!(SHG_ROT_X & 8)) rot_issue_piece(S, P, lane_off);                                            \
        if (!(SHG_ROT_X & 8)) wait_vmcnt<kRingDepth>();                                                   \
        if (!(SHG_ROT_X & 4)) T_ = ringp[S.cslot * 64];                                                   \
        if (!(SHG_ROT_X & 2)) S.cslot = S.cslot + 1 == kRingSlots ? 0 : S.cslot + 1;                      \
        AB_ = prow[S.pf * (4 * PR)];                                                                           \
        if (!(SHG_ROT_X & 2)) S.pf = S.pf + 1 == P.npieces ? 0 : S.pf + 1;                                \
        __builtin_amdgcn_sched_barrier(0);                                                                \
    } while (0)
#ifdef SHG_ROT_SETPRIO
#define ROT_PRIO(x) __builtin_amdgcn_s_setprio(x)
#else
#define ROT_PRIO(x)
#endif
#define ROT_MFMA2(A0, T_, AB_)                                                                            \
    ROT_PRIO(1);                                                                                          \
    acc[A0] = __builtin_amdgcn_mfma_f64_16x16x4f64(AB_.x, T_.x, acc[A0], 0, 0, 0);                        \
    ROT_PRIO(2);                                                                                          \
    acc[A0 + 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(AB_.y, T_.y, acc[A0 + 1], 0, 0, 0);                \
    ROT_PRIO(0)
#define ROT_MFMA4(A0, T_, AB_)                                                                            \
    ROT_PRIO(1);                                                                                          \
    acc[A0] = __builtin_amdgcn_mfma_f64_16x16x4f64(AB_.x, T_.x, acc[A0], 0, 0, 0);                        \
    ROT_PRIO(2);                                                                                          \
    acc[A0 + 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(AB_.x, T_.y, acc[A0 + 1], 0, 0, 0);                \
    acc[A0 + 2] = __builtin_amdgcn_mfma_f64_16x16x4f64(AB_.y, T_.x, acc[A0 + 2], 0, 0, 0);                \
    acc[A0 + 3] = __builtin_amdgcn_mfma_f64_16x16x4f64(AB_.y, T_.y, acc[A0 + 3], 0, 0, 0);                \
    ROT_PRIO(0)
    // first k-step of a class: the accumulators start from the constant 0 operand of the MFMA instead of being cleared with
    // eight VALU moves each (96 per unit; a VALU instruction costs the fp64 MFMA stream ~10 cycles).  Accumulator 0 (CA of
    // class 0) starts from the order-0 values, which are loaded into it beforehand.
#define ROT_MFMA2_FIRST(A0, T_, AB_)                                                                      \
    acc[A0] = (A0) == 0 ? __builtin_amdgcn_mfma_f64_16x16x4f64(AB_.x, T_.x, acc[A0], 0, 0, 0)              \
                        : __builtin_amdgcn_mfma_f64_16x16x4f64(AB_.x, T_.x, kZero4, 0, 0, 0);             \
    acc[A0 + 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(AB_.y, T_.y, kZero4, 0, 0, 0)
#define ROT_MFMA4_FIRST(A0, T_, AB_)                                                                      \
    acc[A0] = __builtin_amdgcn_mfma_f64_16x16x4f64(AB_.x, T_.x, kZero4, 0, 0, 0);                         \
    acc[A0 + 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(AB_.x, T_.y, kZero4, 0, 0, 0);                     \
    acc[A0 + 2] = __builtin_amdgcn_mfma_f64_16x16x4f64(AB_.y, T_.x, kZero4, 0, 0, 0);                     \
    acc[A0 + 3] = __builtin_amdgcn_mfma_f64_16x16x4f64(AB_.y, T_.y, kZero4, 0, 0, 0)
    // one class: k-steps in pairs on the register sets (tx, abx) / (ty, aby); the current fragments are in (tx, abx) on entry
    // and on exit, the fragments of the next k-step are fetched before the MFMAs of the current one are issued
#define ROT_CLASS(C, MF, A0, NACC)                                                                        \
    {                                                                                                     \
        const int nk_ = P.cls_nk[C];                                                                      \
        int i_ = 0;                                                                                       \
        if (nk_ >= 2) {                                                                                   \
            ROT_FETCH(ty, aby);                                                                           \
            MF##_FIRST(A0, tx, abx);                                                                      \
            ROT_FETCH(tx, abx);                                                                           \
            MF(A0, ty, aby);                                                                              \
            i_ = 2;                                                                                       \
        } else if (nk_ == 1) {                                                                            \
            ROT_FETCH(ty, aby);                                                                           \
            MF##_FIRST(A0, tx, abx);                                                                      \
            tx = ty;                                                                                      \
            abx = aby;                                                                                    \
            i_ = 1;                                                                                       \
        } else {                                                                                          \
            _Pragma("unroll") for (int z_ = ((A0) == 0 ? 1 : 0); z_ < (NACC); ++z_) acc[(A0) + z_] = kZero4; \
        }                                                                                                 \
        for (; i_ + 2 <= nk_; i_ += 2) {                                                                  \
            ROT_FETCH(ty, aby);                                                                           \
            MF(A0, tx, abx);                                                                              \
            ROT_FETCH(tx, abx);                                                                           \
            MF(A0, ty, aby);                                                                              \
        }                                                                                                 \
        if (i_ < nk_) {                                                                                   \
            ROT_FETCH(ty, aby);                                                                           \
            MF(A0, tx, abx);                                                                              \
            tx = ty;                                                                                      \
            abx = aby;                                                                                    \
        }                                                                                                 \
    }
    const double4_t kZero4 = {0.0, 0.0, 0.0, 0.0};
    double2_t tx = S.tx, abx = S.abx, ty = {0.0, 0.0}, aby = {0.0, 0.0};
    const int ct0 = wave / EP;
    for (int ct = ct0, q = 0; ct < P.nct; ct += kColStride, ++q) {
        (void)q;
        double4_t acc[T::kAcc];
        {
            // order 0 does not depend on the longitude: start value of CA_0 (C/D layout: row = fk + 4 reg, all columns)
            const double2_t* z = panel + P.nslot * PR + rt * 16 + fk;
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[0][r] = z[4 * r].x;
        }
#pragma unroll
        for (int c = 0; c < T::kClasses; ++c) {
            if (c < T::kTwo) {
                ROT_CLASS(c, ROT_MFMA2, 2 * c, 2)
            } else {
                ROT_CLASS(c, ROT_MFMA4, 2 * T::kTwo + 4 * (c - T::kTwo), 4)
            }
        }
        ROT_STAMP(3 + 2 * min(q, 3));

        // ---- epilogue: the images of every column, in place.  Where nd % 16 == 8 the last column tile runs on 16 real columns,
        //      c' = nd - 8 .. nd + 7: the plan's trig stream carries mu_c' = 2 pi / R - mu_(2 nd - 1 - c') in its lanes 8 .. 15, and the descending
        //      image k + 1 of column c IS the ascending image k of column 2 nd - 1 - c (-mu_c + 2 pi (k + 1) / R = mu_c' + 2 pi k / R).  That
        //      tile forms and stores its R ascending images only, 16 columns of every row in one piece, and no descending image at all.
        const bool fold = P.half_fold != 0 && ct == P.nct - 1;           // wave-uniform
        const int b = b0 + rt;
        const bool epoch_ok = b < P.B && !SHG_DBG(P, 1);
        double* const Gb = P.G + (size_t)min(b, P.B - 1) * P.nlat * P.nlon;
        // lanes (2 q, 2 q + 1) hold adjacent columns: after the exchange every lane owns two rows x two adjacent columns and
        // stores 16 bytes.  Byte offset = lane part (row, column inside the tile) + wave-uniform part (image, column tile);
        // lanes outside the grid carry an offset beyond the buffer and are dropped.
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(Gb, 0, grid_bytes, 0x00020000);
        const int par = fr & 1, ce = fr & ~1;
        const int sa = fk + (par ? 8 : 0), sb = sa + 4;
        const bool col_ok = epoch_ok && ct * 16 + ce < (fold ? P.nd + 8 : P.nd);
        const unsigned row_a = col_ok && slot_valid(sa) ? (unsigned)grid_row(sa) * (unsigned)P.nlon * 8u : 0x80000000u;
        const unsigned row_b = col_ok && slot_valid(sb) ? (unsigned)grid_row(sb) * (unsigned)P.nlon * 8u : 0x80000000u;
        // lane part of the store offsets of this unit: row + column inside the tile, ascending (column ce) and descending (14 - ce)
        const unsigned asc_a = row_a + (unsigned)ce * 8u, asc_b = row_b + (unsigned)ce * 8u;
        const unsigned desc_a = row_a + (unsigned)(14 - ce) * 8u, desc_b = row_b + (unsigned)(14 - ce) * 8u;
        // one image of the unit (accumulator vector v): the lane's two rows x two columns at lane part + wave-uniform byte offset
        auto put_image = [&](const double4_t& v, bool ascending, unsigned lane_a, unsigned lane_b, int soff) {
            double a_lo, a_hi, b_lo, b_hi;
            pair_exchange(v[0], v[2], 0xAAAAAAAAAAAAAAAAull, a_lo, a_hi);
            pair_exchange(v[1], v[3], 0xAAAAAAAAAAAAAAAAull, b_lo, b_hi);
            const double2_t va = ascending ? (double2_t){a_lo, a_hi} : (double2_t){a_hi, a_lo};
            const double2_t vb = ascending ? (double2_t){b_lo, b_hi} : (double2_t){b_hi, b_lo};
            // The wave-uniform part goes into the vector offset, not into the scalar offset operand of the store: with a
            // REGISTER soffset hipcc assumes that a 16-byte store's data registers may be overwritten by the very next VALU
            // instruction (the documented exemption of the gfx9 store-data hazard) and schedules one there; on gfx950 that
            // corrupted the low dword of the stored value in some lanes of some launches.
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uint4_t, va), rsrc, lane_a + (unsigned)soff, 0, SHG_STORE_AUX);
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uint4_t, vb), rsrc, lane_b + (unsigned)soff, 0, SHG_STORE_AUX);
        };
        // The images of the sign -1 sit behind a switch that only skips: their half of the butterfly works in place on accumulators
        // of its own and stores them before the switch ends, so no value is live across it in two versions (an in-place update under a
        // run-time switch whose results outlive the switch makes hipcc copy every vector, ~60 moves per row).
#pragma unroll
        for (int r = 0; r < 4; ++r) rot_split<R>(acc, r);
        // (the sums of the sign -1 are pinned here: hipcc would otherwise move their part of rot_split behind the switch, where only it
        // is used, and keep the sums it is formed from alive beside the images that have taken their registers)
#pragma unroll
        for (int k = 0; k < R; ++k) asm volatile("" : "+v"(acc[T::img_of(k, 1)]));
#pragma unroll
        for (int r = 0; r < 4; ++r) rot_half<R, 0>(acc, r);
        // Ascending image k: the tile's run starts at column (n2 + k nR) mod nlon + 16 ct.  In the folded tile all 16 columns are real.
        // Even R: the run starts at a multiple of 16 and ends inside the row (whole 128-byte lines).  Odd R: n2 is an odd multiple of
        // nd = 8 mod 16, the run starts 8 columns into a line and the one that starts at nlon - 8 goes on at column 0: in that image the
        // lanes of the columns 8 .. 15 take a lane part one row lower (no pair straddles the end of the row, the start is even; a lane
        // outside the grid stays outside: its offset stays at 2^31 or above).
        const unsigned row_wrap = R % 2 != 0 && ce >= 8 ? (unsigned)P.nlon * 8u : 0u;
        int w = n2;
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const bool wraps = R % 2 != 0 && w + 16 * ct + 16 > P.nlon;        // wave-uniform
            put_image(acc[T::img_of(k, 0)], true, wraps ? asc_a - row_wrap : asc_a, wraps ? asc_b - row_wrap : asc_b, (w + 16 * ct) * 8);
            w = w + nR >= P.nlon ? w + nR - P.nlon : w + nR;
        }
        if (!fold) {
#pragma unroll
            for (int r = 0; r < 4; ++r) rot_half<R, 1>(acc, r);
            // descending image k: the run (in descending columns) starts at (n2 + k nR - nd) mod nlon + nd - 16 ct - 16
            w = n2 - P.nd;
#pragma unroll
            for (int k = 0; k < R; ++k) {
                put_image(acc[T::img_of(k, 1)], false, desc_a, desc_b, (w + P.nd - 16 * ct - 16) * 8);
                w = w + nR >= P.nlon ? w + nR - P.nlon : w + nR;
            }
        }
        ROT_STAMP(4 + 2 * min(q, 3));
    }
    S.tx = tx;
    S.abx = abx;
#undef ROT_CLASS
#undef ROT_MFMA2
#undef ROT_MFMA4
#undef ROT_MFMA2_FIRST
#undef ROT_MFMA4_FIRST
#undef ROT_FETCH
}

__device__ __forceinline__ void panel_put(double2_t* panel, int index, double2_t v) { panel[index] = v; }

// Tickets of the Legendre stage.  A workgroup does not store while it runs its Legendre stage, and workgroups that share the HBM fall
// into step (tools/timeline.py: the whole chip in the Legendre stage at once, the HBM idle, then the whole chip storing at twice the
// rate the HBM takes).  In step the stage runs at the rate the L2s deliver its operands (690 KB per tile, every byte used once per
// workgroup: 15 - 17 TB/s chip-wide), not at its MFMA time, and the L2 is a resource of the XCD: so the limit is kept per
// XCD.  Workgroups b, b + 8, ... share an XCD and a queue of two words in a 128-byte line of their own: `head`, the tickets handed
// out, and `served`, the stages finished.  A workgroup draws ticket t = head++ and enters the stage when t - served < limit; behind the
// stage it adds one to served.  First come, first served; nobody takes anything back, waiters add to neither word, and a release
// writes a word that only releases write.  Nothing but speed depends on the workgroups of a queue really sharing an XCD.
//   * A waiter LOOKS at served with a read-modify-write that changes nothing: atomics execute at the memory side, a plain agent-scope
//     load was served by the XCD's L2 and saw a release ~100 us late.
//   * A waiter knows its distance d = t - served - limit + 1, the stages that must end before its turn, and the limit stages that run
//     meanwhile end about one per (stage time / limit): it naps half of d such intervals in units of 0.27 us (s_sleep 10 at 2.4 GHz)
//     and looks again, so that it looks once or twice per stage from far away and every 0.27 us plus the look's own round trip (~1 us
//     beside the stores of the others) when it is next.  The stage time is taken as one unit per item of a wave (5 - 6 us for the 22
//     items of a full block at d/o 96 when few workgroups share the L2).
//   * The wait is bounded to a few milliseconds of naps and looks (words left unequal by an aborted launch must not hang the next
//     one); a workgroup that gave up runs its stage and releases like every other, so the counts stay paired.
//   * The last release of a queue's share of the grid takes both words back to 0 (each has been added to exactly `share` times).
constexpr int kTicketQueues = 8, kTicketLineInts = 32;      // one queue per XCD, 128 bytes apart
constexpr int kTicketNapBudget = 12000;                    // nap units (0.27 us), a look counts as four

__device__ __forceinline__ void legendre_ticket_acquire(int* queue, int limit, int stage_units) {
    const int t = __hip_atomic_fetch_add(queue, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int budget = kTicketNapBudget; budget > 0;) {
        // (the look: a compare-and-swap of a value the word never holds against itself.  hipcc folds an add of 0 into the plain load.)
        int served = -1;
        (void)__hip_atomic_compare_exchange_strong(queue + 1, &served, -1, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int d = t - served - limit + 1;
        if (d <= 0) return;
        const int naps = min(max(d * stage_units / (2 * limit), 1), 64);
        for (int i = 0; i < naps; ++i) __builtin_amdgcn_s_sleep(10);
        budget -= naps + 4;
    }
}
__device__ __forceinline__ void legendre_ticket_release(int* queue, int share) {
    if (__hip_atomic_fetch_add(queue + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1 == share) {      // the last of this queue: every ticket is drawn, nobody waits
        (void)__hip_atomic_fetch_add(queue, -share, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_add(queue + 1, -share, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Phase 1: Legendre stage of tile (bt, it) (see synthesis_fused.hip).  The orders of the tile are dealt to the waves that call this
// (work-item records `recs`, one list per wave); the result of order m is one 16-byte pair (A_m, B'_m) per panel row, written to
// `panel` -- the LDS panel of the tile, or (persistent kernel) the image of the NEXT tile's panel in global memory.
// `queue`: the ticket queue of the workgroup when the plan limits the stage (P.xcd_limit > 0).  The wait for the turn sits behind the
// operand loads of the first three items: they are issued unconditionally either way, and a workgroup that gets its turn starts with
// its pipeline full instead of one L2 round trip behind.
template <bool NS, typename PanelPtr>
__device__ __forceinline__ void rot_phase1(const RotParams& P, PanelPtr panel, const int4* recs_wave, int bt, int it, int lane, int* queue) {
    const int fr = lane & 15, fk = lane >> 4;
    // Everything that is the same for all lanes stays on the scalar unit: the work-item records come through scalar loads
    // (constant address space), every operand load is "scalar base + lane offset fixed for the kernel", the flags of a record
    // steer uniform branches, and the two accumulators of an order start from the MFMA's constant-zero operand instead of
    // being cleared with 16 VALU moves.  Measured before: ~9 VALU instructions per MFMA in this stage (64-bit vector address
    // arithmetic from records that sat in vector registers, flag tests, selects, clears); VALU instructions share the issue
    // pipe with the fp64 MFMAs, so the stage was bound by their sum (2 x (6.5 k + 9 k) cycles per SIMD and tile = the 14 us
    // it took), not by the L2 -> L1 rate it had been attributed to.
    constexpr int ASTRIDE = NS ? 128 : 64;
    typedef int int4_v __attribute__((ext_vector_type(4)));
    typedef const int4_v __attribute__((address_space(4))) crec_t;
    // operand loads: buffer loads "descriptor of the tile's table (scalar) + lane offset (fixed) + octet offset (scalar)": not a
    // single vector instruction per load besides the load itself (the global-load form needs a register copy per load to keep
    // its scalar base)
    auto ld16 = [](__amdgpu_buffer_rsrc_t table, unsigned voff, unsigned soff) {
        return __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(table, voff, soff, 0));
    };
    const int bad = NS ? P.badmap[it] : -1;
    const int it_tab = SHG_DBG(P, 16) ? 7 : it, bt_tab = SHG_DBG(P, 32) ? 0 : bt;       // experiment: every workgroup reads the same tables
    __amdgpu_buffer_rsrc_t pku = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(P.pkf + (size_t)it_tab * P.Qtot * 128), 0, 0xffffffffu, 0x00020000);
    const __amdgpu_buffer_rsrc_t cfu =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(NS ? P.cpk4 + (size_t)bt_tab * P.Qtot * 128 : P.cpk4 + (size_t)bt_tab * P.Qtot * 64), 0, 0xffffffffu, 0x00020000);
    const unsigned pk_voff = (unsigned)lane * 16u;
    const unsigned cf_voff = NS ? (unsigned)lane * 16u : (unsigned)(fk * 8 + (fr & 7)) * 16u;
    int mode = NS && bad >= 0 ? 1 : 0;
    int prow = lane;
    const bool arow = NS || fr < 8;
    double4_t acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    const double4_t zero4 = {0.0, 0.0, 0.0, 0.0};
    double sgm = (mode == 0 && fr >= 8) ? -1.0 : 1.0;                 // sign of the lane's own part in the north / south combination
    bool fresh = true;                                              // uniform: the next MFMA pair opens an order

#define ROT_P1_ISSUE(rec, ALO, AHI, BLO, BHI)                                                \
do {                                                                                     \
    ALO = ld16(cfu, cf_voff, (unsigned)(rec).x * (ASTRIDE * 8u));                        \
    BLO = ld16(pku, pk_voff, (unsigned)(rec).x * 1024u);                                 \
    AHI = ld16(cfu, cf_voff, (unsigned)(rec).y * (ASTRIDE * 8u));                        \
    BHI = ld16(pku, pk_voff, (unsigned)(rec).y * 1024u);                                 \
} while (0)

#define ROT_P1_CONSUME(rec, ALO, AHI, BLO, BHI)                                                                     \
do {                                                                                                            \
    if ((rec).w & 1) {                                                                                          \
        const double ax_ = NS ? ALO.x : (arow ? ALO.x : 0.0), ay_ = NS ? ALO.y : (arow ? ALO.y : 0.0);          \
        if (fresh) {                                                                                            \
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(ax_, BLO.x, zero4, 0, 0, 0);                            \
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(ay_, BLO.y, zero4, 0, 0, 0);                            \
        } else {                                                                                                \
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(ax_, BLO.x, acc0, 0, 0, 0);                             \
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(ay_, BLO.y, acc1, 0, 0, 0);                             \
        }                                                                                                       \
        fresh = false;                                                                                          \
    }                                                                                                           \
    if ((rec).w & 2) {                                                                                          \
        const double ax_ = NS ? AHI.x : (arow ? AHI.x : 0.0), ay_ = NS ? AHI.y : (arow ? AHI.y : 0.0);          \
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(ax_, BHI.x, acc0, 0, 0, 0);                                 \
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(ay_, BHI.y, acc1, 0, 0, 0);                                 \
    }                                                                                                           \
    if ((rec).w & 4) {                                  /* last item of an order: see synthesis_fused.hip */     \
        double vc_ = acc0[0] + acc1[0], vs_ = acc0[1] + acc1[1];                                                \
        if (NS) {                                                                                               \
            const double oc_ = acc0[2] + acc1[2], os_ = acc0[3] + acc1[3];                                      \
            /* a lane sends x = (E of slots 0-7 | O of slots 8-15) and receives the other part r: E + O = r + x on */ \
            /* the northern slots, E - O = r - x on the mirrored ones: one exact fma with the lane's sign           */ \
            const double xc_ = fr < 8 ? vc_ : oc_, xs_ = fr < 8 ? vs_ : os_;                                   \
            const double rc_ = swap_half_row(xc_), rs_ = swap_half_row(xs_);                                   \
            vc_ = fma(sgm, xc_, rc_);                                                                           \
            vs_ = fma(sgm, xs_, rs_);                                                                           \
        }                                                                                                       \
        if (!NS || mode == 0 || fr < 8) panel_put(panel, (rec).z * 64 + prow, (double2_t){vc_, vs_});           \
        fresh = true;                                                                                           \
    }                                                                                                           \
} while (0)

    double2 xal = {0, 0}, xah = {0, 0}, xbl = {0, 0}, xbh = {0, 0};
    double2 yal = {0, 0}, yah = {0, 0}, ybl = {0, 0}, ybh = {0, 0};
    double2 zal = {0, 0}, zah = {0, 0}, zbl = {0, 0}, zbh = {0, 0};
    double2 wal = {0, 0}, wah = {0, 0}, wbl = {0, 0}, wbh = {0, 0};
    crec_t* recs = reinterpret_cast<crec_t*>(reinterpret_cast<unsigned long long>(recs_wave));
    for (int pass = 0; pass < (mode == 0 ? 1 : 2); ++pass) {
        if (pass == 1) {                                          // mirrored parallels of a polar block: their own table
            mode = 2;
            sgm = 1.0;
            prow = lane + 8;
            pku = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(P.pkf + (size_t)(P.nit + bad) * P.Qtot * 128), 0, 0xffffffffu, 0x00020000);
        }
        int4_v c0 = recs[0], c1 = recs[1], c2 = recs[2];
        int4_v n0 = recs[3], n1 = recs[4], n2 = recs[5], n3 = recs[6];
        // (scheduling barriers: the order of the first loads must be the order the loop consumes them in, see pipe_phase1)
        ROT_P1_ISSUE(c0, xal, xah, xbl, xbh);
        __builtin_amdgcn_sched_barrier(0);
        ROT_P1_ISSUE(c1, yal, yah, ybl, ybh);
        __builtin_amdgcn_sched_barrier(0);
        ROT_P1_ISSUE(c2, zal, zah, zbl, zbh);
        __builtin_amdgcn_sched_barrier(0);
        if (pass == 0 && P.xcd_limit > 0) {                       // (uniform) the turn of this workgroup; the other waves wait at the barrier
            if (threadIdx.x == 0) legendre_ticket_acquire(queue, P.xcd_limit, P.nrec);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
        }
        for (int trip = 0; trip < P.ntrip; ++trip) {
            const int4_v a3 = n0, a4 = n1, a5 = n2, a6 = n3;
            crec_t* nr = recs + 4 * trip + 7;
            n0 = nr[0];
            n1 = nr[1];
            n2 = nr[2];
            n3 = nr[3];
            ROT_P1_ISSUE(a3, wal, wah, wbl, wbh);
            ROT_P1_CONSUME(c0, xal, xah, xbl, xbh);
            ROT_P1_ISSUE(a4, xal, xah, xbl, xbh);
            ROT_P1_CONSUME(c1, yal, yah, ybl, ybh);
            ROT_P1_ISSUE(a5, yal, yah, ybl, ybh);
            ROT_P1_CONSUME(c2, zal, zah, zbl, zbh);
            ROT_P1_ISSUE(a6, zal, zah, zbl, zbh);
            ROT_P1_CONSUME(a3, wal, wah, wbl, wbh);
            c0 = a4;
            c1 = a5;
            c2 = a6;
        }
    }
#undef ROT_P1_ISSUE
#undef ROT_P1_CONSUME
}

template <bool NS, int R>
__global__ __launch_bounds__(128 * EP) void synthesis_rot_kernel(RotParams P) {
    constexpr int NW = 2 * EP, PR = 16 * EP;           // waves, panel rows
    using T = RotTraits<R>;
    extern __shared__ __attribute__((aligned(16))) double As[];   // rings [8][kRingSlots][64][2], then panel [nslot + 1][64 rows][2]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nbt = (P.B + 3) >> 2;
    const int tile = (int)blockIdx.x;
    if (tile >= nbt * P.nit) return;
    const int bt = P.blockmap ? P.blockmap[2 * tile] : tile % nbt;
    const int it = P.blockmap ? P.blockmap[2 * tile + 1] : tile / nbt;
    const int fr = lane & 15, fk = lane >> 4;
#ifdef SHG_EXPERIMENT
    if (P.stagger > 0 && blockIdx.x < 256) {
        const long long ticks = (long long)P.stagger * (long long)(((blockIdx.x >> 3) * 13) & 31) / 32;
        const long long t0 = wall_clock64();
        for (int i = 0; i < 100000 && (long long)wall_clock64() - t0 < ticks; ++i) __builtin_amdgcn_s_sleep(8);
    }
#endif
    ROT_STAMP(0);

    double2_t* const panel = reinterpret_cast<double2_t*>(As + NW * kRingSlots * 128);      // [(slot * PR + row)], behind the rings of the waves

    // ---- order pruning: the layout, trig stream and item table of this latitude block (a polar block keeps the orders up to its level
    //      only and uses the front slots of the panel, its order-0 slot behind them).  Scalar loads of wave-uniform values, once; from
    //      here on the kernel runs on them as it did on the launch parameters.
    {
        typedef int int4_v __attribute__((ext_vector_type(4)));
        typedef const int4_v __attribute__((address_space(4))) clev_t;
        static_assert(kMaxClasses == 6 && kRotLevelInts == 24, "level record layout");
        clev_t* lv = reinterpret_cast<clev_t*>(reinterpret_cast<unsigned long long>(P.levtab + (size_t)__builtin_amdgcn_readfirstlane(it) * kRotLevelInts));
        const int4_v h = lv[0], o = lv[1], a = lv[2], b = lv[3], c = lv[4];
        P.npieces = h.x;
        P.nslot = h.y;
        P.nrec = h.z;
        P.ntrip = h.w;
        P.trig += (size_t)o.x * 128;
        P.itemtab += o.y;
        P.cls_nk[0] = a.x, P.cls_nk[1] = a.y, P.cls_nk[2] = a.z, P.cls_nk[3] = a.w, P.cls_nk[4] = b.x, P.cls_nk[5] = b.y;
        P.cls_cnt[0] = b.z, P.cls_cnt[1] = b.w, P.cls_cnt[2] = c.x, P.cls_cnt[3] = c.y, P.cls_cnt[4] = c.z, P.cls_cnt[5] = c.w;
    }

    // ---- zero the padding slots of the panel
    {
        int s0 = 0;
#pragma unroll
        for (int c = 0; c < T::kClasses; ++c) {
            for (int s = s0 + P.cls_cnt[c]; s < s0 + 4 * P.cls_nk[c]; ++s)
                if (tid < PR) panel[s * PR + tid] = (double2_t){0.0, 0.0};
            s0 += 4 * P.cls_nk[c];
        }
    }

    // ---- trig stream of this wave.  The issue side runs kRingDepth pieces ahead of the consumer and never stops (when a wave has
    //      no further column tile it re-reads pieces), so that the count of DMAs in flight is the same at every wait.
    RotStream S;
    rot_stream_init(S, P, As, wave);
#pragma unroll
    for (int d = 0; d < kRingDepth; ++d) rot_issue_piece(S, P, (unsigned)lane * 16u);

    // ---- phase 1: Legendre stage.  Orders are distributed over the waves of the workgroup.
    int* const queue = P.tickets + (blockIdx.x % kTicketQueues) * kTicketLineInts;
    if (!SHG_DBG(P, 2)) rot_phase1<NS>(P, panel, P.itemtab + (size_t)wave * P.nrec, bt, it, lane, queue);
    ROT_STAMP(1);
    __syncthreads();          // panel complete; from here on it is read-only and the waves run independently
    if (P.xcd_limit > 0 && !SHG_DBG(P, 2) && tid == 0) legendre_ticket_release(queue, ((int)gridDim.x - (int)(blockIdx.x % kTicketQueues) + kTicketQueues - 1) / kTicketQueues);
    ROT_STAMP(2);
#ifdef SHG_EXPERIMENT
    if (P.stagger2 > 0 && wave >= EP) {
        const long long t0 = wall_clock64();
        for (int i = 0; i < 100000 && (long long)wall_clock64() - t0 < P.stagger2; ++i) __builtin_amdgcn_s_sleep(4);
    }
#endif

    // ---- phase 2: longitude stage
    if (wave / EP < P.nct && !SHG_DBG(P, 4)) {
        const double2_t* const ringp = reinterpret_cast<const double2_t*>(As) + wave * (kRingSlots * 64) + lane;
        rot_issue_piece(S, P, (unsigned)lane * 16u);       // fragments of the first k-step
        wait_vmcnt<kRingDepth>();
        S.tx = ringp[0];
        S.cslot = 1;
        S.abx = panel[(wave % EP) * 16 + fr + fk * PR];
        S.pf = P.npieces > 1 ? 1 : 0;
        rot_phase2<NS, R>(P, As, panel, S, wave, lane, bt * 4, it);
        // The prefetched pieces of the stream must have landed before the LDS is released -- but not the stores: the stores of the
        // last unit are the youngest operations of the wave (its last LDS-DMA was issued in the last k-step, before them), and the
        // counter runs in order, so "at most as many outstanding as that unit stored" means every DMA is done.  That is 4 R stores,
        // or 2 R where the wave's last unit is the folded column tile (waiting for 4 R there would let the LDS go with the prefetched
        // DMAs still in flight into it, i.e. into the next workgroup's panel).  The wave ends with its stores in flight instead of
        // waiting for HBM to acknowledge them.  With the fold on every wave waits for 2 R: the waves that end on a whole unit (the
        // other half of the workgroup; on the headline they have a unit less than those that end on the folded tile) then wait for half of its stores, and
        // telling the two apart by the wave's last column tile cost the kernels of R = 6 and 3 a stack slot.
        if (P.half_fold != 0)
            wait_vmcnt<2 * R>();
        else
            wait_vmcnt<4 * R>();
    } else {
        wait_vmcnt<0>();
    }
    ROT_STAMP(12);
}


// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------

// class position in the K sequence (two-sum classes first: r = 0, then r = R / 2 for even R, then r = 1, 2, ...) and sign of
// order m >= 1 for R rotations
static inline void order_class(int R, int m, int& cls, int& sign) {
    const int rho = m % R;
    const int r = 2 * rho <= R ? rho : R - rho;
    sign = 2 * rho <= R ? 1 : -1;
    if (R % 2 == 0)
        cls = r == 0 ? 0 : 2 * r == R ? 1 : r + 1;
    else
        cls = r;
}
static inline int rot_classes(int R) { return R / 2 + 1; }

// sign of the sine coefficients of order m in the repacked coefficient table (0 = no rotation kernel)
int rot_sigma_negative(int R, int m) { return R > 0 && 2 * (m % R) > R ? 1 : 0; }

// True when the meridians are lon_j = -pi + (j + 1/2) 2 pi / nlon to within a few ulp of pi: every one of the 2 R images
// s mu_c + 2 pi k / R of the fundamental domain mu_c = lon[nlon/2 + c] is a grid column.
bool has_rotation_symmetry(int nlon, const double* lon, int R) {
    if (nlon < 192 || nlon % (2 * R) != 0 || nlon % 2 != 0) return false;
    if ((nlon / R) % 16 != 0) return false;              // images of a column tile = whole 128-byte lines (nd = nlon / (2 R) is then even: 16-byte pair stores)
    const double tol = 3e-15;
    const long double pi = 3.141592653589793238462643383279502884L;
    const int n2 = nlon / 2, nR = nlon / R, nd = nlon / (2 * R);
    for (int c = 0; c < nd; ++c) {
        const long double mu = lon[n2 + c];
        for (int k = 0; k < R; ++k) {
            const int jp = (n2 + k * nR + c) % nlon, jm = (n2 + k * nR - 1 - c + nlon) % nlon;
            long double dp = lon[jp] - (mu + 2 * pi * k / R), dm = lon[jm] - (-mu + 2 * pi * k / R);
            dp -= 2 * pi * std::round((double)(dp / (2 * pi)));
            dm -= 2 * pi * std::round((double)(dm / (2 * pi)));
            if (std::fabs((double)dp) > tol || std::fabs((double)dm) > tol) return false;
        }
    }
    return true;
}

// class layout of the panel / trig stream for degree N; returns the panel slots (without the order-0 slot)
int rot_layout(int R, int N, int nk[kMaxClasses], int cnt[kMaxClasses], std::vector<int>* order_slot) {
    const int nc = rot_classes(R);
    for (int c = 0; c < kMaxClasses; ++c) cnt[c] = nk[c] = 0;
    for (int m = 1; m <= N; ++m) {
        int c, s;
        order_class(R, m, c, s);
        cnt[c]++;
    }
    int s = 0, slot[kMaxClasses];
    for (int c = 0; c < nc; ++c) {
        nk[c] = (cnt[c] + 3) / 4;
        slot[c] = s;
        s += 4 * nk[c];
    }
    if (order_slot) {
        order_slot->assign(N + 1, 0);
        int next[kMaxClasses];
        for (int c = 0; c < nc; ++c) next[c] = slot[c];
        for (int m = 1; m <= N; ++m) {
            int c, sg;
            order_class(R, m, c, sg);
            (*order_slot)[m] = next[c]++;
        }
        (*order_slot)[0] = s;
    }
    return s;
}

int rot_kernel_waves() { return kWaves; }

static size_t rot_lds_bytes(int nslot) { return (size_t)kRingDoubles * 8 + (size_t)(nslot + 1) * 1024; }      // rings, panel

static bool rot_fits(int R, int N) {
    int nk[kMaxClasses], cnt[kMaxClasses];
    return rot_lds_bytes(rot_layout(R, N, nk, cnt, nullptr)) <= 160 * 1024;
}

int rot_applicable(const shg_plan* p) {
    if (p->rotR == 0 || p->N < 1) return 0;
    if ((long long)p->nlat * p->nlon * 8 >= (1LL << 31)) return 0;
    return rot_fits(p->rotR, p->N) ? 1 : 0;
}

// The rotation count of a plan: the first of kRotPreference that the meridians allow and whose panel fits the LDS at degree N.
// 10 rotations (20 images; the 0.25 degree grid: 72 columns in the fundamental domain) need 92 MFMAs per 16 rows x 16 columns x 20
// images at d/o 96, 9 rotations (18 images, 80 columns) 102, 6 rotations (12 images, 120 columns) 80.  The 0.5 degree grid (nlon = 720) allows 9
// and 3: 0.167 against 0.222 ms per 240 epochs at d/o 96.
int rot_choose(int nlon, const double* lon_h, int N) {
    static const int kRotPreference[] = {SHG_ROT_PREFERENCE};
    int fallback = 0;
    for (int R : kRotPreference)
        if (has_rotation_symmetry(nlon, lon_h, R)) {
            if (N < 1 || rot_fits(R, N)) return R;
            if (!fallback) fallback = R;
        }
    return fallback;
}

// trig stream [nct][npieces][64][2] (+ one spare piece) of the orders 1 .. level, built on the host like the other cos/sin tables
// (grates/utilities.py:272-273).  Where nd % 16 == 8 the lanes 8 .. 15 of the last column tile lie beyond the fundamental domain:
// fill_half = false leaves them zero (shg_rot_level_tables, byte for byte what it always returned), fill_half = true (the plan's device
// copy) puts the columns c' = nd .. nd + 7 there, whose ascending images are the descending images of the columns 2 nd - 1 - c' (see
// rot_phase2).  Their angle is derived from the fundamental column, mu_c' = 2 pi / R - mu_(2 nd - 1 - c') in long double, not read from
// lon_h[nlon / 2 + c']: every output column's argument then stays as close to its own meridian as has_rotation_symmetry demands.
void rot_trig_stream(int R, int N, int level, int nlon, const double* lon_h, std::vector<double>& tab, bool fill_half) {
    (void)N;
    const int nd = nlon / (2 * R), nct = ceil_div(nd, 16);
    const long double pi = 3.141592653589793238462643383279502884L;
    int nk[kMaxClasses], cnt[kMaxClasses];
    std::vector<int> order_slot;
    const int nslot = rot_layout(R, level, nk, cnt, &order_slot);
    const int npieces = nslot / 4;
    std::vector<int> slot_order(nslot, -1);
    for (int m = 1; m <= level; ++m) slot_order[order_slot[m]] = m;
    tab.assign(((size_t)nct * npieces + 1) * 128, 0.0);
    for (int ct = 0; ct < nct; ++ct)
        for (int ks = 0; ks < npieces; ++ks)
            for (int l = 0; l < 64; ++l) {
                const int m = slot_order[4 * ks + (l >> 4)], c = 16 * ct + (l & 15);
                if (m < 0 || (c >= nd && !(fill_half && nd % 16 == 8))) continue;
                int cls, sg;
                order_class(R, m, cls, sg);
                double* dst = &tab[(((size_t)ct * npieces + ks) * 64 + l) * 2];
                if (c < nd) {
                    const double arg = (double)m * lon_h[nlon / 2 + c];
                    dst[0] = std::cos(arg);
                    dst[1] = sg * std::sin(arg);
                } else {
                    const long double arg = (long double)m * (2 * pi / R - (long double)lon_h[nlon / 2 + 2 * nd - 1 - c]);
                    dst[0] = (double)std::cos(arg);
                    dst[1] = sg * (double)std::sin(arg);
                }
            }
}

// The streams of all levels of the plan behind each other (each with its spare piece), the full one first.
int build_rot_trig(shg_plan* p, const double* lon_h) {
    const std::vector<int> full(1, p->N);
    const std::vector<int>& levels = p->rot_level_set.empty() ? full : p->rot_level_set;
    std::vector<double> all, tab;
    p->rot_trig_piece.clear();
    for (int level : levels) {
        rot_trig_stream(p->rotR, p->N, level, p->nlon, lon_h, tab, true);
        p->rot_trig_piece.push_back((int)(all.size() / 128));
        all.insert(all.end(), tab.begin(), tab.end());
    }
    p->rot_levtab_valid = false;
    return upload(p->rot_trig, all);
}

// Order pruning.  P_nm(theta) ~ sin^m theta: on a parallel close to a pole the orders above some m_c contribute nothing that an fp64
// sum can hold.  Per parallel, m_c is the largest order of which any degree reaches |kn P_nm| >= tau x the parallel's largest |kn P_nm|
// over all (n, m); a latitude block of the kernel (8 northern parallels and their mirror images, or 16 parallels without the north-south
// symmetry) takes the largest m_c of its parallels, rounded up to a level: the orders 0 .. level with level + 1 a multiple of
// kRotLevelStep, at most N.  The cut-off depends on the colatitudes, kn and N only, never on the coefficients.
// tau = 1e-30: a dropped term is at most tau x the parallel's largest factor M times a coefficient, and there are fewer than (N + 1)^2 < 2e4
// of them (N <= kRotPruneMaxDegree), so what is dropped is below 2e-26 M max|c|.  The grid values of that parallel are sums of factors up
// to M times coefficients: unless the coefficients that meet the large factors are 1e10 times smaller than those of the dropped orders,
// that is 1e-10 of the rounding unit (1.1e-16) of the values themselves and 1e-14 of the project's tolerance (1e-12 of the field maximum).
constexpr double kRotPruneTau = 1e-30;
constexpr int kRotLevelStep = 10;

void rot_order_cutoffs(int N, int nlat, const double* colat, const double* kn, bool ns, std::vector<int>& levels) {
    const int nh = nlat / 2;
    const int nit = ns ? ceil_div(nh, 8) : ceil_div(nlat, 16);
    levels.assign(nit, 0);
    std::vector<double> a, b, big(N + 1);
    recursion_tables(N, a, b);
    for (int i = 0; i < nlat; ++i) {
        const double t = std::cos(colat[i]), st = std::sin(colat[i]);
        const double* k = kn + (size_t)i * (N + 1);
        double pmm = 1.0, all = 0.0;
        bool finite = true;
        for (int m = 0; m <= N; ++m) {
            if (m == 1) pmm = std::sqrt(3.0) * st;
            if (m > 1) pmm = std::sqrt((2.0 * m + 1.0) / (2.0 * m)) * st * pmm;
            const int off = order_offset(N, m);
            double p1 = pmm, p2 = 0.0, mx = std::fabs(p1 * k[m]);
            for (int n = m + 1; n <= N; ++n) {
                const double pn = (a[off + n - m] * t) * p1 - b[off + n - m] * p2;
                p2 = p1;
                p1 = pn;
                const double v = std::fabs(pn * k[n]);
                if (!(v <= mx)) mx = v;                      // (keeps a NaN)
            }
            big[m] = mx;
            if (!std::isfinite(mx)) finite = false;
            if (mx > all) all = mx;
        }
        int mc = N;                                          // nothing to compare with: keep everything
        if (finite && all > 0.0) {
            mc = 0;
            for (int m = N; m >= 1; --m)
                if (big[m] >= kRotPruneTau * all) {
                    mc = m;
                    break;
                }
        }
        const int block = ns ? (i < nh ? i : nlat - 1 - i) >> 3 : i >> 4;
        if (block < nit) levels[block] = std::max(levels[block], mc);
    }
    for (int& l : levels) l = std::min(N, ceil_div(l + 1, kRotLevelStep) * kRotLevelStep - 1);
}

// the distinct levels of a plan: N first (the full tables, which a plan with pruning off uses for every block), then descending
std::vector<int> rot_level_list(int N, const std::vector<int>& levels) {
    std::vector<int> set(levels);
    set.push_back(N);
    std::sort(set.begin(), set.end(), [](int x, int y) { return x > y; });
    set.erase(std::unique(set.begin(), set.end()), set.end());
    return set;
}

// level records of the latitude blocks (common.h: kRotLevelInts), pruning on, then off
static int build_rot_levtab(shg_plan* p, int R, int nit) {
    if (p->rot_levtab_valid && p->rot_levtab_d.size() == (size_t)2 * nit * kRotLevelInts) return SHG_OK;
    const std::vector<int>& set = p->rot_level_set;
    if ((int)p->rot_levels.size() != nit || set.empty() || set[0] != p->N || p->rot_trig_piece.size() != set.size() || p->rot_item_rec.size() != set.size())
        return fail(SHG_ERR_INVALID, "rotation-folded synthesis kernel: the level tables of the plan are incomplete");
    std::vector<int> tab((size_t)2 * nit * kRotLevelInts, 0);
    for (int off = 0; off < 2; ++off)
        for (int it = 0; it < nit; ++it) {
            const int level = off ? p->N : p->rot_levels[it];
            const size_t l = std::find(set.begin(), set.end(), level) - set.begin();
            if (l >= set.size()) return fail(SHG_ERR_INVALID, "rotation-folded synthesis kernel: level %d has no tables", level);
            int* rec = &tab[((size_t)off * nit + it) * kRotLevelInts];
            rec[1] = rot_layout(R, level, rec + 8, rec + 8 + kMaxClasses, nullptr);
            rec[0] = rec[1] / 4;
            rec[2] = p->rot_item_nrec[l];
            rec[3] = p->rot_item_ntrip[l];
            rec[4] = p->rot_trig_piece[l];
            rec[5] = p->rot_item_rec[l];
        }
    if (p->rot_levtab_d) SHG_HIP(hipDeviceSynchronize());
    const int rc = upload(p->rot_levtab_d, tab);
    if (rc) return rc;
    p->rot_levtab_valid = true;
    return SHG_OK;
}

template <int R>
static int launch_rot(bool ns, const RotParams& P, size_t lds, dim3 grid_dim, hipStream_t stream) {
    if (ns) {
        SHG_HIP(hipFuncSetAttribute((const void*)synthesis_rot_kernel<true, R>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((synthesis_rot_kernel<true, R>), grid_dim, dim3(64 * kWaves), lds, stream, P);
    } else {
        SHG_HIP(hipFuncSetAttribute((const void*)synthesis_rot_kernel<false, R>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((synthesis_rot_kernel<false, R>), grid_dim, dim3(64 * kWaves), lds, stream, P);
    }
    return SHG_OK;
}

// the ticket queues back to zero, synchronously: no launch is in flight when they are written and none can see them half written
static int zero_tickets(shg_plan* p) {
    const unsigned seen = hip_failures();
    if (!p->tickets_d && p->tickets_d.assign(kTicketQueues * kTicketLineInts) != hipSuccess) return fail(SHG_ERR_NOMEM, "ticket queue allocation failed");
    SHG_HIP(hipDeviceSynchronize());
    SHG_HIP(hipMemset(p->tickets_d.get(), 0, p->tickets_d.size() * sizeof(int)));
    SHG_HIP(hipDeviceSynchronize());
    p->tickets_failures = seen;
    return SHG_OK;
}

static int device_cus(int* cus) {
    int dev = 0;
    SHG_HIP(hipGetDevice(&dev));
    SHG_HIP(hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, dev));
    return SHG_OK;
}

// The limit of a plan on which rot_set_stage_limit was never called.  Measured on the headline (240 x d/o 96 -> 0.25 degree, 2700
// workgroups; tools/stage_limit_sweep.py, profiles/tickets_ab.txt): 4/16 of the CUs in the stage at once is the best setting (-4.1 % of
// the step), 5/16 and 6/16 take 2 % off, 3/16 no longer admits the share of the CUs that the stage needs and costs 12 %.  That share
// is the stage's part of a tile's time: the stage's time goes with its operand octets (Qtot, 345 on the headline), the rest of the
// tile's with the nlon (1440) columns it computes and stores -- so the default scales 4/16 by (Qtot / nlon) / (345 / 1440) and is no
// limit where that reaches the whole device.  A grid of at most one workgroup per CU has nothing to keep out of step: no limit either.
static int default_stage_limit(const shg_plan* p, int workgroups, int* limit) {
    int cus = 0;
    const int rc = device_cus(&cus);
    if (rc) return rc;
    *limit = 0;
    if (workgroups <= cus) return SHG_OK;
    const double share = 4.0 / 16.0 * ((double)p->Qtot / p->nlon) / (345.0 / 1440.0);
    const int n = (int)std::ceil(cus * share);
    if (n < cus) *limit = std::max(n, kTicketQueues);
    return SHG_OK;
}

int synthesis_rot(shg_plan* p, const double* anm, int B, double* grid, hipStream_t stream) {
    if (!rot_applicable(p)) return fail(SHG_ERR_UNSUPPORTED, "rotation-folded synthesis kernel not applicable to this plan");
    const int R = p->rotR;
    const bool ns = p->sym_ns;
    int rc = build_pkf_table(p, ns, R, stream);
    if (rc) return rc;
    const int nbt = ceil_div(B, 4);
    const int nit = ns ? ceil_div(p->nlat / 2, 8) : ceil_div(p->nlat, 16);
    rc = pack_coefficients_fused(p, ns, R, anm, B, stream);
    if (rc) return rc;
    RotParams P;
    P.N = p->N;
    P.nlat = p->nlat;
    P.nlon = p->nlon;
    P.B = B;
    P.nit = nit;
    P.nh = p->nlat / 2;
    P.nd = p->nlon / (2 * R);
    P.nct = ceil_div(P.nd, 16);
    P.half_fold = p->half_tile_fold && P.nd % 16 == 8 ? 1 : 0;
    P.nslot = rot_layout(R, p->N, P.cls_nk, P.cls_cnt, nullptr);
    P.npieces = P.nslot / 4;
#ifdef SHG_EXPERIMENT
    P.dbg = experiment_switches();
    P.stagger = getenv("SHG_STAGGER") ? atoi(getenv("SHG_STAGGER")) : 0;
    P.stagger2 = getenv("SHG_STAGGER2") ? atoi(getenv("SHG_STAGGER2")) : 0;
#endif
    P.Qtot = p->Qtot;
    P.cpk4 = p->cpk4.get();
    P.pkf = p->pkf.get();
    P.itemtab = reinterpret_cast<const int4*>(p->itemtab_d.get());
    P.nrec = p->itemtab_nrec;
    P.ntrip = p->itemtab_ntrip;
    int limit = p->stage_limit;
    if (!p->stage_limit_set) {                      // nobody has called rot_set_stage_limit: the default
        rc = default_stage_limit(p, nbt * nit, &limit);
        if (rc) return rc;
    }
    // The queues are allocated and zeroed synchronously before the first launch that uses them and are 0 again whenever a grid has
    // drained.  A launch that did not drain may have left them unequal, and such a launch shows as a HIP error of some later call: zero
    // them again behind any.
    if (limit > 0 && (!p->tickets_d || p->tickets_failures != hip_failures())) {
        rc = zero_tickets(p);
        if (rc) return rc;
    }
    P.tickets = p->tickets_d.get();
    P.xcd_limit = limit > 0 ? ceil_div(limit, kTicketQueues) : 0;
#ifdef SHG_EXPERIMENT
    if (getenv("SHG_SEM") && limit > 0) P.xcd_limit = ceil_div(atoi(getenv("SHG_SEM")), kTicketQueues);
#endif
    P.badmap = p->badmap_d.get();
    P.blockmap = nullptr;
    if (!SHG_DBG(P, 2048)) {
        rc = build_blockmap(p, nbt, nit, stream);
        if (rc) return rc;
        P.blockmap = p->blockmap_d.get();
    }
    P.trig = p->rot_trig.get();
    rc = build_rot_levtab(p, R, nit);
    if (rc) return rc;
    P.levtab = p->rot_levtab_d.get() + (p->order_pruning ? 0 : (size_t)nit * kRotLevelInts);
    P.G = grid;
#ifdef SHG_TIMELINE
    P.tl = getenv("SHG_TIMELINE_PTR") ? (unsigned long long*)strtoull(getenv("SHG_TIMELINE_PTR"), nullptr, 0) : nullptr;
#endif
    const size_t lds = rot_lds_bytes(P.nslot);
    const dim3 grid_dim((unsigned)(nbt * nit));
    ProfileScope ps(p, 2, stream);
    switch (R) {
        case 10: rc = launch_rot<10>(ns, P, lds, grid_dim, stream); break;
        case 9: rc = launch_rot<9>(ns, P, lds, grid_dim, stream); break;
        case 6: rc = launch_rot<6>(ns, P, lds, grid_dim, stream); break;
        case 3: rc = launch_rot<3>(ns, P, lds, grid_dim, stream); break;
        default: return fail(SHG_ERR_UNSUPPORTED, "rotation-folded synthesis kernel: no kernel for %d rotations", R);
    }
    if (rc) return rc;
    SHG_HIP(hipGetLastError());
    return SHG_OK;
}

// Limit on the workgroups that run their Legendre stage at once (see legendre_ticket_acquire), kept per XCD: an eighth of it, rounded
// up, per ticket queue.  limit > 0: that many workgroups; < 0: that many sixteenths of the device's CUs; 0: no limit.  A plan on which
// this was never called runs with default_stage_limit; any call, 0 included, replaces the default for good.  The queues are allocated
// and zeroed here, synchronously, so that no launch can see them uninitialised or left unequal by an aborted launch.
int rot_set_stage_limit(shg_plan* p, int limit) {
    if (limit < 0) {
        int cus = 0;
        const int rc = device_cus(&cus);
        if (rc) return rc;
        limit = std::max(1, cus * -limit / 16);
    }
    if (limit > 0) {
        const int rc = zero_tickets(p);
        if (rc) return rc;
    }
    p->stage_limit = limit;
    p->stage_limit_set = true;
    return SHG_OK;
}

}  // namespace shg

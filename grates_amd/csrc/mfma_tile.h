// The fp64 MFMA tile shared by the dense product kernels: output tile 32 F x 32 F of a workgroup of 4 waves as
// 2 x 2, F x F accumulators of v_mfma_f64_16x16x4_f64 per wave, K tiles of 16 = four k-steps of F x F MFMAs.
//   gemm.hip                                uniform-base loads, lds_double_t, tile_mfmas (its rotated K loop stays its own)
//   blas.hip                                uniform-base loads, tile_mfmas (its rotated K loop stays its own)
//   leverage.hip                            uniform-base loads, lds_double_t, tile_multiply, SHG_TILE_PIPELINE
//   whiten_long.hip                         lds_double_t, tile_multiply, SHG_TILE_PIPELINE
//   covprop.hip                             tile_multiply (its loop advances a stateful fetch and peels its tail)
// The accumulators are zeroed by a loop in each kernel: behind a helper that takes the array, however it is written, hipcc
// allocates registers differently in every one of these kernels (none then compiles to the code it had).  The one timing of
// that form, a few processes per library, had the covariance kernels of gemm.hip about 0.3 % slower: too thin a basis to call
// it a slowdown, enough not to trade identical code for four lines.
// What the pieces have in common: fp64 MFMAs and the VALU instructions of all waves of a SIMD share one issue pipe
// (tools/mfma64_issue.hip; an integer VALU instruction costs the pipe more than a tenth of an MFMA, profiles/r01_mfma64_issue.txt), so
// a K loop keeps its address arithmetic on the scalar unit and in instruction immediates.
#pragma once

#include "common.h"

namespace shg {

// 32-bit LDS addresses: a pointer to lds_double_t stays the operand of ds_read / ds_write as it is.  A kernel makes the lane's
// fragment base opaque (asm volatile("" : "+v"(base))), so that every fragment read is one ds_read_b64 "lane base + 16-bit
// immediate": left to see through the base, the compiler splits the 72 KB of offsets differently and adds to the base with a VALU
// instruction per k-step.  Reading through a volatile pointer keeps the reads from being paired into ds_read2_b64, which moves
// half the bytes per LDS cycle and whose 8-bit offsets need such an add as well.
typedef double __attribute__((address_space(3))) lds_double_t;

// A load as "uniform 64-bit base (advanced per K tile by scalar instructions) + per-lane 32-bit byte offset (fixed for the whole
// kernel)".  The empty asm pins the uniform base in scalar registers -- without it the compiler folds base + lane offset into one
// loop-invariant 64-bit vector address and adds the scalar part with a VALU instruction per load; the address goes through an
// integer, so the pointer is rebuilt in the global address space explicitly.  The 32 -> 64 bit extension of the lane offset has
// to stay in the basic block of the load for the scalar-base form to be selected: pass the offset through pin_vector there.
__device__ __forceinline__ unsigned pin_vector(unsigned v) {
    asm volatile("" : "+v"(v));
    return v;
}
__device__ __forceinline__ double load_uniform_base(const double* base, unsigned byte_off) {
    typedef const double __attribute__((address_space(1))) gdouble_t;
    typedef const char __attribute__((address_space(1))) gbyte_t;
    unsigned long long b = reinterpret_cast<unsigned long long>(base);
    asm volatile("" : "+s"(b));
    return *reinterpret_cast<gdouble_t*>(reinterpret_cast<gbyte_t*>(b) + byte_off);
}
__device__ __forceinline__ double2 load2_uniform_base(const double* base, unsigned byte_off) {      // 16 bytes, 16-byte aligned
    typedef double gdouble2_v __attribute__((ext_vector_type(2)));
    typedef const gdouble2_v __attribute__((address_space(1))) gdouble2_t;
    typedef const char __attribute__((address_space(1))) gbyte_t;
    unsigned long long b = reinterpret_cast<unsigned long long>(base);
    asm volatile("" : "+s"(b));
    const gdouble2_v v = *reinterpret_cast<gdouble2_t*>(reinterpret_cast<gbyte_t*>(b) + byte_off);
    return make_double2(v.x, v.y);
}

// The F x F MFMAs of one k-step, closed by a scheduling barrier.  NLOADS > 0: the NLOADS vector-memory loads issued in front of
// the call in the source are dealt between the MFMAs, F F / NLOADS MFMAs per load (16 MFMAs: 4, 2, 1 for 4, 8, 12 .. 16 loads).  A
// wave issues in order, and 24 loads in a row keep it away from the MFMA pipe for ~1800 cycles (the address unit takes one load
// per ~16 cycles and serves eight waves).
template <int F, int NLOADS>
__device__ __forceinline__ void tile_mfmas(const double (&af)[F], const double (&bf)[F], double4_t (&acc)[F][F]) {
    // in use: 0, 4, 8, 12 and 16 loads at F = 4, 0 and 4 at F = 2; for these F F / NLOADS is what gemm.hip and blas.hip each had
    static_assert(NLOADS >= 0 && NLOADS % 4 == 0 && NLOADS <= F * F, "tile_mfmas: 0, 4, 8, ... F F loads");
#pragma unroll
    for (int a = 0; a < F; ++a)
#pragma unroll
        for (int b = 0; b < F; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[a], bf[b], acc[a][b], 0, 0, 0);
    if constexpr (NLOADS > 0) {
#pragma unroll
        for (int i = 0; i < NLOADS; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, F * F / NLOADS, 0);
            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
}

// The four k-steps of a staged K tile: read F + F fragments at compile-time strides (AK / BK doubles per k-step, AS / BS per
// fragment, from the lane's fragment bases), then F x F MFMAs.  The pointer types are the caller's: const volatile lds_double_t*
// for the ds_read_b64 form described above, plain pointers where the compiler's own choice stands.
template <int F, int AK, int AS, int BK, int BS, typename PA, typename PB>
__device__ __forceinline__ void tile_multiply(PA a_ptr, PB b_ptr, double4_t (&acc)[F][F]) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        double af[F], bf[F];
#pragma unroll
        for (int a = 0; a < F; ++a) af[a] = a_ptr[ks * AK + a * AS];
#pragma unroll
        for (int b = 0; b < F; ++b) bf[b] = b_ptr[ks * BK + b * BS];
#pragma unroll
        for (int a = 0; a < F; ++a)
#pragma unroll
            for (int b = 0; b < F; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[a], bf[b], acc[a][b], 0, 0, 0);
    }
}

// Double-buffered K loop over the tiles 0 .. nt - 1 (nt >= 1, uniform): fetch(i) requests the operands of tile i into registers,
// stage(buf, i) writes them to LDS buffer buf, multiply(buf) is the tile_multiply of that buffer.  Tile i is multiplied from
// buffer i & 1 while the operands of tile i + 1 are requested in front of its MFMAs and staged behind them; one barrier per
// tile, two tiles per trip so that the buffer of every access is a literal.
// A macro, not a function template: as a template (callables by reference, by value, with or without the inner lambda) hipcc
// compiles the lag arithmetic of whiten_long_kernel's B tile differently (114 of its 2297 instructions); expanded in the kernel
// both users compile to the code they had with the loop written out in them.
#define SHG_TILE_PIPELINE(nt, fetch, stage, multiply)                                     \
    do {                                                                                  \
        auto step_ = [&](int buf, int i) {                                                \
            const bool more = i + 1 < (nt);                           /* uniform */       \
            if (more) fetch(i + 1);                                                       \
            multiply(buf);                                                                \
            if (more) stage(buf ^ 1, i + 1);                                              \
            __syncthreads();                                                              \
        };                                                                                \
        fetch(0);                                                                         \
        stage(0, 0);                                                                      \
        __syncthreads();                                                                  \
        int i_ = 0;                                                                       \
        for (; i_ + 1 < (nt); i_ += 2) {                                                  \
            step_(0, i_);                                                                 \
            step_(1, i_ + 1);                                                             \
        }                                                                                 \
        if (i_ < (nt)) step_(0, i_);                                                      \
    } while (0)

}  // namespace shg

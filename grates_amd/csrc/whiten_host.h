// Host side of shg_whiten_rows (whiten.hip), shg_whiten_rows_long (whiten_long.hip) and shg_whiten_rows_vector (whiten_vector.hip)
// without any HIP: the one contract of the three calls, so that a stand-alone program can run it under a host sanitizer
// (tools/whiten_host_check.cpp).
#pragma once

#include <cstddef>
#include <cstdint>

#include "host_require.h"

namespace shg {

constexpr int kWhitenMaxOrder = 128;                // q of shg_whiten_rows, lstsq.MAX_WHITENING_ORDER
constexpr int kWhitenLongMaxOrder = 4095;           // q of shg_whiten_rows_long, lstsq.MAX_COVARIANCE_ORDER
constexpr int kVectorMaxOrder = 128;                // q of shg_whiten_rows_vector
constexpr int kVectorMinDim = 2, kVectorMaxDim = 6; // K of shg_whiten_rows_vector

// What the calls differ in: the name, what they count ("rows" that take the tap tables of `channels` channels in turn, or "groups" of
// `per` = K rows that are filtered jointly and have no channels) and the largest order.
struct WhitenCall { const char *fn, *noun; int max_order; bool joint; };
constexpr WhitenCall kWhitenRows = {"shg_whiten_rows", "rows", kWhitenMaxOrder, false};
constexpr WhitenCall kWhitenRowsLong = {"shg_whiten_rows_long", "rows", kWhitenLongMaxOrder, false};
constexpr WhitenCall kWhitenRowsVector = {"shg_whiten_rows_vector", "groups", kVectorMaxOrder, true};

// 0: launch; 1: nothing to do; -1: refused, with the reason in message.  `count` rows (per = 1) or groups of `per` rows
inline int whiten_check(const WhitenCall& call, long long count, int per, int channels, int M, const double* X, long long ldx, const void* stage,
                        const void* taps, int q, int skip, const double* Y, long long ldy, char* message, size_t size) {
    const char *fn = call.fn, *noun = call.noun;
    SHG_HOST_REQUIRE(count >= 0 && M >= 0 && ldx >= 0 && ldy >= 0, "%s: negative size (%s %lld, M %d, ldx %lld, ldy %lld)", fn, noun, count, M, ldx, ldy);
    if (call.joint) {
        SHG_HOST_REQUIRE(per >= kVectorMinDim && per <= kVectorMaxDim, "%s: dimension K %d outside %d .. %d", fn, per, kVectorMinDim, kVectorMaxDim);
    } else {
        SHG_HOST_REQUIRE(channels >= 1, "%s: channels %d below 1", fn, channels);
        SHG_HOST_REQUIRE(count % channels == 0, "%s: %s %lld are not a multiple of channels %d", fn, noun, count, channels);
    }
    SHG_HOST_REQUIRE(q >= 0 && q <= call.max_order, "%s: order q %d outside 0 .. %d", fn, q, call.max_order);
    SHG_HOST_REQUIRE(skip >= 0 && skip <= M, "%s: skip %d outside 0 .. M %d", fn, skip, M);
    SHG_HOST_REQUIRE(ldx >= M, "%s: ldx %lld below M %d", fn, ldx, M);
    SHG_HOST_REQUIRE(ldy >= M - skip, "%s: ldy %lld below M - skip %d", fn, ldy, M - skip);
    const long long limit = 1LL << 40;
    if (call.joint) SHG_HOST_REQUIRE(count <= limit / per, "%s: %lld %s of %d rows are too large", fn, count, noun, per);
    const long long rows = count * per;
    const bool fits = (ldx == 0 || rows <= limit / ldx) && (ldy == 0 || rows <= limit / ldy);
    if (call.joint) SHG_HOST_REQUIRE(fits, "%s: %lld %s of %d rows of %lld (X) and %lld (Y) values are too large", fn, count, noun, per, ldx, ldy);
    SHG_HOST_REQUIRE(fits, "%s: %lld %s of %lld (X) and %lld (Y) values are too large", fn, count, noun, ldx, ldy);
    if (count == 0 || M == skip) return 1;
    SHG_HOST_REQUIRE(X && stage && taps && Y, "%s: NULL pointer", fn);
    const uintptr_t x0 = (uintptr_t)X, x1 = x0 + (uintptr_t)((rows - 1) * ldx + M) * sizeof(double);       // at most 2^43 + 2^34 bytes each
    const uintptr_t y0 = (uintptr_t)Y, y1 = y0 + (uintptr_t)((rows - 1) * ldy + (M - skip)) * sizeof(double);
    SHG_HOST_REQUIRE(x1 <= y0 || y1 <= x0, "%s: X and Y overlap (the call is out of place)", fn);
    return 0;
}

}  // namespace shg

// Host side of shg_segment_lag_products_long (lags_long.hip) without any HIP: the argument rules, the work items and the sizes of the
// workspace, so that a stand-alone program can run them under a host sanitizer (tools/lags_long_host_check.cpp).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "host_require.h"

namespace shg {

constexpr int kLagLongMax = 4095;           // lags of shg_segment_lag_products_long, lstsq.MAX_COVARIANCE_ORDER
constexpr int kLagLongTile = 256;           // lags of one 16 x 16 accumulator: D[i][j] is the lag k0 + 16 i + j
constexpr int kLagLongWaves = 4;            // waves of a workgroup: wave w takes quarter w of the chunk
constexpr int kLagLongQuarter = 512;        // columns of a quarter
constexpr int kLagLongChunk = kLagLongWaves * kLagLongQuarter;      // columns of a work item, counted from the start of the segment
constexpr int kLagLongTail = 512;           // the last chunk of a segment takes up to this many columns more, in place of a short chunk of its own
constexpr int kLagLongLongest = kLagLongChunk + kLagLongTail;       // columns of a chunk at most
constexpr int kLagLongGroup = 4;            // accumulators that a wave holds at a time (tiles of one sweep over its quarter)
constexpr int kLagLongSkew = 240;           // A[i][c] = x[c - 16 i]: the columns behind a quarter that still meet one of its values
constexpr int kLagLongBlocks = 1 << 20;     // workgroups of a launch at most: the rest is a grid stride

constexpr int lag_long_tiles(int lags) { return lags / kLagLongTile + 1; }
// columns that the chunk takes of the `left` columns from its first one to the end of the segment: all of them if that ends the segment
constexpr int lag_long_take(int left) { return left <= kLagLongLongest ? left : kLagLongChunk; }
// columns of a wave of a chunk of `take` columns: 512, or a quarter of a last chunk that is longer than 2048, rounded up to a K-step
constexpr int lag_long_quarter(int take) { return take <= kLagLongChunk ? kLagLongQuarter : (take + 15) / 16 * 4; }
// K-steps of 4 columns of a quarter of `length` columns (0 .. 640), a multiple of 4 (the A fragments rotate through 4 registers)
constexpr int lag_long_steps(int length) { return length <= 0 ? 0 : (length + kLagLongSkew + 15) / 16 * 4; }
// doubles of x that a workgroup stages for `tiles` accumulators: the longest chunk, the skew with the round-up of the steps (255 at most), the 15
// columns of j and the first lag of the last tile; no index c + j + k0 lies outside
constexpr int lag_long_staged(int tiles) { return kLagLongLongest + 256 + 16 + kLagLongTile * (tiles - 1); }
// LDS of a workgroup in doubles: the staged values, and the accumulators of the waves 1 .. 3 of one sweep on their way to wave 0
constexpr int kLagLongLds = kLagLongLongest + 256 + 16 + kLagLongTile * (kLagLongMax / kLagLongTile) + (kLagLongWaves - 1) * kLagLongGroup * kLagLongTile;

// Chunks have slots: the chunks of segment s, which starts at column `start` of the clamped table, are the slots
// start / chunk + s, ... one after the other.  The segments of a clamped table do not overlap, so no two chunks share a slot and all
// slots lie below M / chunk + nseg (segment s + 1 starts where s ends: start / chunk + ceil(length / chunk) <= end / chunk + 1).
// Chunk j starts at column j chunk of the segment; a remainder of up to kLagLongTail columns goes to the chunk in front of it.
constexpr long long lag_long_first_slot(int start, int s) { return (long long)(start / kLagLongChunk) + s; }
constexpr int lag_long_chunks(int length) {
    return length <= 0 ? 0 : length <= kLagLongLongest ? 1 : (length - kLagLongTail + kLagLongChunk - 1) / kLagLongChunk;
}

struct LagLongGeometry {
    int tiles;                              // accumulators of 256 lags that cover 0 .. lags
    long long slots;                        // chunk slots of a row, M / chunk + nseg: the used ones are the work items
    long long items;                        // (row, slot) pairs, one workgroup each
    unsigned blocks;                        // workgroups of the launch
    long long partials;                     // doubles of the workspace: [rows][slots][tiles 256] partial sums
    int staged;                             // lag_long_staged(tiles)
    size_t lds_bytes;
};

inline LagLongGeometry segment_lag_products_long_geometry(long long rows, int M, int nseg, int lags) {
    LagLongGeometry g;
    g.tiles = lag_long_tiles(lags);
    g.slots = (long long)(M / kLagLongChunk) + nseg;
    g.items = rows * g.slots;
    g.blocks = (unsigned)std::min<long long>(g.items, kLagLongBlocks);
    g.partials = g.items * g.tiles * kLagLongTile;
    g.staged = lag_long_staged(g.tiles);
    g.lds_bytes = (size_t)kLagLongLds * sizeof(double);
    return g;
}

// 0: launch; 1: nothing to do; -1: refused, with the reason in message
inline int segment_lag_products_long_check(long long rows, int M, const void* X, long long ldx, int lags, int nseg, const void* seg, const void* S,
                                           char* message, size_t size) {
    const char* fn = "shg_segment_lag_products_long";
    SHG_HOST_REQUIRE(rows >= 0 && M >= 0 && ldx >= 0, "%s: negative size (rows %lld, M %d, ldx %lld)", fn, rows, M, ldx);
    SHG_HOST_REQUIRE(lags >= 0 && lags <= kLagLongMax, "%s: lags %d outside 0 .. %d", fn, lags, kLagLongMax);
    SHG_HOST_REQUIRE(nseg >= 0, "%s: nseg %d is negative", fn, nseg);
    SHG_HOST_REQUIRE(ldx >= M, "%s: ldx %lld below M %d", fn, ldx, M);
    const long long limit = 1LL << 40;
    SHG_HOST_REQUIRE(ldx == 0 || rows <= limit / ldx, "%s: %lld rows of %lld values of X are too large", fn, rows, ldx);
    SHG_HOST_REQUIRE(nseg == 0 || rows <= limit / ((long long)nseg * (lags + 1)), "%s: %lld rows of %d segments and %d values of S are too large", fn,
                     rows, nseg, lags + 1);
    const long long slots = (long long)(M / kLagLongChunk) + nseg, each = (long long)lag_long_tiles(lags) * kLagLongTile;
    SHG_HOST_REQUIRE(nseg == 0 || (slots <= INT32_MAX && rows <= limit / (slots * each)),
                     "%s: %lld rows of %lld chunks and %lld partial sums of the workspace are too large", fn, rows, slots, each);
    if (rows == 0 || nseg == 0) return 1;
    SHG_HOST_REQUIRE(X && seg && S, "%s: NULL pointer", fn);
    return 0;
}

}  // namespace shg

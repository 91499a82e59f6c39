// Host side of shg_segment_products (arcs.hip) without any HIP: the argument rules and the launch geometry, so that a stand-alone
// program can run them under a host sanitizer (tools/arcs_host_check.cpp).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "host_require.h"

namespace shg {

constexpr int kSegMaxParameters = 16;       // u of shg_segment_products, lstsq.MAX_ARC_PARAMETERS
// rows of one channel that a wave takes through a segment together (one read of Bt for all of them): u accumulators per row and lane
constexpr int segment_rows(int u) { return u > 8 ? 2 : 4; }
constexpr int kSegWaves = 4;                // waves of a workgroup, one work item each
constexpr int kSegBlocks = 256 * 8;         // workgroups of a launch at most: the rest is a grid stride

struct SegmentGeometry {
    long long groups;                       // groups of segment_rows(u) rows of one channel
    long long items;                        // (group, segment) pairs: one wave each
    unsigned blocks;                        // workgroups of kSegWaves waves
};

// 0: launch; 1: nothing to do; -1: refused, with the reason in message
inline int segment_products_check(long long rows, int channels, int M, const void* X, long long ldx, const void* Bt, long long ldb, int u, int nseg,
                                  const void* seg, const void* S, char* message, size_t size) {
    const char* fn = "shg_segment_products";
    SHG_HOST_REQUIRE(rows >= 0 && M >= 0 && ldx >= 0 && ldb >= 0, "%s: negative size (rows %lld, M %d, ldx %lld, ldb %lld)", fn, rows, M, ldx, ldb);
    SHG_HOST_REQUIRE(channels >= 1, "%s: channels %d below 1", fn, channels);
    SHG_HOST_REQUIRE(rows % channels == 0, "%s: rows %lld are not a multiple of channels %d", fn, rows, channels);
    SHG_HOST_REQUIRE(u >= 1 && u <= kSegMaxParameters, "%s: u %d outside 1 .. %d", fn, u, kSegMaxParameters);
    SHG_HOST_REQUIRE(nseg >= 0, "%s: nseg %d is negative", fn, nseg);
    SHG_HOST_REQUIRE(ldx >= M, "%s: ldx %lld below M %d", fn, ldx, M);
    SHG_HOST_REQUIRE(ldb >= M, "%s: ldb %lld below M %d", fn, ldb, M);
    const long long limit = 1LL << 40;
    SHG_HOST_REQUIRE(ldx == 0 || rows <= limit / ldx, "%s: %lld rows of %lld values of X are too large", fn, rows, ldx);
    SHG_HOST_REQUIRE(nseg == 0 || rows <= limit / ((long long)nseg * u), "%s: %lld rows of %d segments and %d values of S are too large", fn, rows, nseg,
                     u);
    if (rows == 0 || nseg == 0) return 1;
    SHG_HOST_REQUIRE(X && Bt && seg && S, "%s: NULL pointer", fn);
    return 0;
}

inline SegmentGeometry segment_products_geometry(long long rows, int channels, int nseg, int u) {
    SegmentGeometry g;
    g.groups = (rows / channels + segment_rows(u) - 1) / segment_rows(u) * channels;
    g.items = g.groups * nseg;
    g.blocks = (unsigned)std::min<long long>((g.items + kSegWaves - 1) / kSegWaves, kSegBlocks);
    return g;
}

}  // namespace shg

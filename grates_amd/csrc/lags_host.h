// Host side of shg_segment_lag_products (lags.hip) without any HIP: the argument rules and the launch geometry, so that a stand-alone
// program can run them under a host sanitizer (tools/lags_host_check.cpp).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "host_require.h"

namespace shg {

constexpr int kLagMax = 128;                // lags of shg_segment_lag_products, lstsq.MAX_WHITENING_ORDER
constexpr int kLagWaves = 4;                // waves of a workgroup
constexpr int kLagRows = 4;                 // lags = 0: rows that a wave takes through a segment together, one work item per wave
constexpr int kLagTile = 1024;              // lags > 0: columns of a segment that a workgroup stages in LDS, with kLagMax more behind them
constexpr int kLagMaxGroup = 33;            // lags > 0: accumulators of a lane at most; 4 waves of 33 hold the 129 lags of lags = 128
constexpr int kLagBlocks = 256 * 8;         // workgroups of a launch at most: the rest is a grid stride

// lags > 0: the lags of one wave of the workgroup (wave w holds the lags w g .. w g + g - 1), the smallest of 1, 2, 4, 8, 16, 33 with
// which the four waves cover 0 .. lags
constexpr int lag_group(int lags) {
    const int need = (lags + kLagWaves) / kLagWaves;
    return need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : need <= 8 ? 8 : need <= 16 ? 16 : kLagMaxGroup;
}

struct LagGeometry {
    int group;                              // 0: the kernel of lags = 0; else lag_group(lags)
    long long items;                        // lags = 0: (group of kLagRows rows, segment) pairs, one wave each; else (row, segment) pairs, one workgroup each
    unsigned blocks;                        // workgroups of kLagWaves waves
};

// 0: launch; 1: nothing to do; -1: refused, with the reason in message
inline int segment_lag_products_check(long long rows, int M, const void* X, long long ldx, int lags, int nseg, const void* seg, const void* S,
                                      char* message, size_t size) {
    const char* fn = "shg_segment_lag_products";
    SHG_HOST_REQUIRE(rows >= 0 && M >= 0 && ldx >= 0, "%s: negative size (rows %lld, M %d, ldx %lld)", fn, rows, M, ldx);
    SHG_HOST_REQUIRE(lags >= 0 && lags <= kLagMax, "%s: lags %d outside 0 .. %d", fn, lags, kLagMax);
    SHG_HOST_REQUIRE(nseg >= 0, "%s: nseg %d is negative", fn, nseg);
    SHG_HOST_REQUIRE(ldx >= M, "%s: ldx %lld below M %d", fn, ldx, M);
    const long long limit = 1LL << 40;
    SHG_HOST_REQUIRE(ldx == 0 || rows <= limit / ldx, "%s: %lld rows of %lld values of X are too large", fn, rows, ldx);
    SHG_HOST_REQUIRE(nseg == 0 || rows <= limit / ((long long)nseg * (lags + 1)), "%s: %lld rows of %d segments and %d values of S are too large", fn,
                     rows, nseg, lags + 1);
    if (rows == 0 || nseg == 0) return 1;
    SHG_HOST_REQUIRE(X && seg && S, "%s: NULL pointer", fn);
    return 0;
}

inline LagGeometry segment_lag_products_geometry(long long rows, int nseg, int lags) {
    LagGeometry g;
    if (lags == 0) {
        g.group = 0;
        g.items = (rows + kLagRows - 1) / kLagRows * nseg;
        g.blocks = (unsigned)std::min<long long>((g.items + kLagWaves - 1) / kLagWaves, kLagBlocks);
    } else {
        g.group = lag_group(lags);
        g.items = rows * nseg;
        g.blocks = (unsigned)std::min<long long>(g.items, kLagBlocks);
    }
    return g;
}

}  // namespace shg

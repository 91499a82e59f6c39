// Host checks of shg_segment_lag_products under a sanitizer: the argument rules and the launch geometry of
// grates_amd/csrc/lags_host.h, which need no HIP.  A stand-alone program for the CPU:
//   hipcc -std=c++17 -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/lags_host_check.cpp -o lags_host_check
//   (or any host compiler: g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all ...) and run it: it prints "ok".
#include <cstdio>
#include <cstring>

#include "../grates_amd/csrc/lags_host.h"

using namespace shg;

static int failures = 0;

static void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        ++failures;
    }
}

static int check(long long rows, int M, bool x, long long ldx, int lags, int nseg, bool seg, bool s, const char* text, size_t size = 256) {
    static double target;
    char message[256] = "";
    const int status = segment_lag_products_check(rows, M, x ? &target : nullptr, ldx, lags, nseg, seg ? &target : nullptr, s ? &target : nullptr,
                                                  message, size);
    if (text && !std::strstr(message, text)) {
        std::printf("FAILED: '%s' not in '%s'\n", text, message);
        ++failures;
    }
    return status;
}

int main() {
    expect(check(6, 10, true, 10, 5, 2, true, true, nullptr) == 0, "valid arguments");
    expect(check(6, 10, true, 10, 0, 2, true, true, nullptr) == 0, "lags = 0");
    expect(check(6, 10, true, 10, 128, 2, true, true, nullptr) == 0, "lags = 128");
    expect(check(-1, 10, true, 10, 5, 2, true, true, "negative size") == -1, "negative rows");
    expect(check(6, -1, true, 10, 5, 2, true, true, "negative size") == -1, "negative M");
    expect(check(6, 10, true, -1, 5, 2, true, true, "negative size") == -1, "negative ldx");
    expect(check(6, 10, true, 10, -1, 2, true, true, "lags -1 outside 0 .. 128") == -1, "lags = -1");
    expect(check(6, 10, true, 10, 129, 2, true, true, "lags 129 outside 0 .. 128") == -1, "lags = 129");
    expect(check(6, 10, true, 10, 5, -1, true, true, "nseg -1 is negative") == -1, "nseg");
    expect(check(6, 10, true, 9, 5, 2, true, true, "ldx 9 below M 10") == -1, "ldx");
    expect(check((1LL << 20) + 1, 1 << 20, true, 1 << 20, 5, 2, true, true, "values of X are too large") == -1, "X above 2^40");
    expect(check(1LL << 20, 4, true, 4, 15, (1 << 16) + 1, true, true, "values of S are too large") == -1, "S above 2^40");
    expect(check(1LL << 62, 0, true, 0, 128, 2147483647, true, true, "values of S are too large") == -1, "the largest sizes do not overflow");
    expect(check(0, 10, false, 10, 5, 2, false, false, nullptr) == 1, "rows = 0");
    expect(check(6, 10, false, 10, 5, 0, false, false, nullptr) == 1, "nseg = 0");
    expect(check(6, 10, false, 10, 5, 2, true, true, "NULL pointer") == -1, "NULL X");
    expect(check(6, 10, true, 10, 5, 2, false, true, "NULL pointer") == -1, "NULL seg");
    expect(check(6, 10, true, 10, 5, 2, true, false, "NULL pointer") == -1, "NULL S");
    expect(check(-1, 10, true, 10, 5, 2, true, true, nullptr, 8) == -1, "a short message buffer is not overrun");

    for (int lags = 0; lags <= kLagMax; ++lags) {
        const int group = lag_group(lags);
        expect(group >= 1 && group <= kLagMaxGroup && kLagWaves * group >= lags + 1, "the waves of a workgroup cover the lags");
        const int smaller = group == kLagMaxGroup ? 16 : group / 2;
        expect(group == 1 || kLagWaves * smaller < lags + 1, "the smallest group that does");
        for (long long rows : {1LL, 3LL, 4LL, 5LL, 303LL, 1LL << 32}) {
            for (int nseg : {1, 2, 1000}) {
                if (rows > (1LL << 40) / ((long long)nseg * (lags + 1))) continue;               // refused by the check
                const LagGeometry g = segment_lag_products_geometry(rows, nseg, lags);
                if (lags == 0) {
                    expect(g.group == 0 && g.items == (rows + kLagRows - 1) / kLagRows * nseg, "one item per group of rows and segment");
                    expect(g.blocks >= 1 && g.blocks <= (unsigned)kLagBlocks && (long long)g.blocks * kLagWaves < g.items + kLagWaves, "workgroups of waves");
                } else {
                    expect(g.group == group && g.items == rows * nseg, "one item per row and segment");
                    expect(g.blocks >= 1 && g.blocks <= (unsigned)kLagBlocks && g.blocks <= g.items, "workgroups");
                }
            }
        }
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}

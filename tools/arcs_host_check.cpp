// Host checks of shg_segment_products under a sanitizer: the argument rules and the launch geometry of grates_amd/csrc/arcs_host.h,
// which need no HIP.  A stand-alone program for the CPU:
//   hipcc -std=c++17 -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/arcs_host_check.cpp -o arcs_host_check
//   (or any host compiler: g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all ...) and run it: it prints "ok".
#include <cstdio>
#include <cstring>

#include "../grates_amd/csrc/arcs_host.h"

using namespace shg;

static int failures = 0;

static void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        ++failures;
    }
}

static int check(long long rows, int channels, int M, bool x, long long ldx, bool bt, long long ldb, int u, int nseg, bool seg, bool s, const char* text,
                 size_t size = 256) {
    static double target;
    char message[256] = "";
    const int status = segment_products_check(rows, channels, M, x ? &target : nullptr, ldx, bt ? &target : nullptr, ldb, u, nseg,
                                              seg ? &target : nullptr, s ? &target : nullptr, message, size);
    if (text && !std::strstr(message, text)) {
        std::printf("FAILED: '%s' not in '%s'\n", text, message);
        ++failures;
    }
    return status;
}

int main() {
    expect(check(6, 3, 10, true, 10, true, 10, 4, 2, true, true, nullptr) == 0, "valid arguments");
    expect(check(-1, 3, 10, true, 10, true, 10, 4, 2, true, true, "negative size") == -1, "negative rows");
    expect(check(6, 3, -1, true, 10, true, 10, 4, 2, true, true, "negative size") == -1, "negative M");
    expect(check(6, 3, 10, true, -1, true, 10, 4, 2, true, true, "negative size") == -1, "negative ldx");
    expect(check(6, 3, 10, true, 10, true, -1, 4, 2, true, true, "negative size") == -1, "negative ldb");
    expect(check(6, 0, 10, true, 10, true, 10, 4, 2, true, true, "channels 0 below 1") == -1, "channels");
    expect(check(7, 3, 10, true, 10, true, 10, 4, 2, true, true, "not a multiple") == -1, "rows % channels");
    expect(check(6, 3, 10, true, 10, true, 10, 0, 2, true, true, "u 0 outside 1 .. 16") == -1, "u = 0");
    expect(check(6, 3, 10, true, 10, true, 10, 17, 2, true, true, "u 17 outside 1 .. 16") == -1, "u = 17");
    expect(check(6, 3, 10, true, 10, true, 10, 4, -1, true, true, "nseg -1 is negative") == -1, "nseg");
    expect(check(6, 3, 10, true, 9, true, 10, 4, 2, true, true, "ldx 9 below M 10") == -1, "ldx");
    expect(check(6, 3, 10, true, 10, true, 9, 4, 2, true, true, "ldb 9 below M 10") == -1, "ldb");
    expect(check((1LL << 20) + 1, 1, 1 << 20, true, 1 << 20, true, 1 << 20, 4, 2, true, true, "values of X are too large") == -1, "X above 2^40");
    expect(check(1LL << 20, 1, 4, true, 4, true, 4, 16, (1 << 16) + 1, true, true, "values of S are too large") == -1, "S above 2^40");
    expect(check(1LL << 62, 1, 0, true, 0, true, 0, 16, 2147483647, true, true, "values of S are too large") == -1, "the largest sizes do not overflow");
    expect(check(0, 3, 10, false, 10, false, 10, 4, 2, false, false, nullptr) == 1, "rows = 0");
    expect(check(6, 3, 10, false, 10, false, 10, 4, 0, false, false, nullptr) == 1, "nseg = 0");
    expect(check(6, 3, 10, false, 10, true, 10, 4, 2, true, true, "NULL pointer") == -1, "NULL X");
    expect(check(6, 3, 10, true, 10, false, 10, 4, 2, true, true, "NULL pointer") == -1, "NULL Bt");
    expect(check(6, 3, 10, true, 10, true, 10, 4, 2, false, true, "NULL pointer") == -1, "NULL seg");
    expect(check(6, 3, 10, true, 10, true, 10, 4, 2, true, false, "NULL pointer") == -1, "NULL S");
    expect(check(-1, 3, 10, true, 10, true, 10, 4, 2, true, true, nullptr, 8) == -1, "a short message buffer is not overrun");

    for (int u = 1; u <= kSegMaxParameters; ++u) {
        expect(segment_rows(u) == (u > 8 ? 2 : 4), "rows of a wave");
        for (long long rows : {1LL, 3LL, 4LL, 5LL, 28215LL, 1LL << 40}) {
            for (int channels : {1, 3}) {
                if (rows % channels) continue;
                for (int nseg : {1, 2, 1000}) {
                    if (rows > (1LL << 40) / ((long long)nseg * u)) continue;           // refused by the check
                    const SegmentGeometry g = segment_products_geometry(rows, channels, nseg, u);
                    const long long per = segment_rows(u), outer = rows / channels;
                    expect(g.groups % channels == 0 && g.groups / channels * per >= outer && (g.groups / channels - 1) * per < outer, "groups cover the rows");
                    expect(g.items == g.groups * nseg && g.items >= 1, "one item per group and segment");
                    expect(g.blocks >= 1 && g.blocks <= (unsigned)kSegBlocks && (long long)g.blocks * kSegWaves < g.items + kSegWaves, "workgroups");
                }
            }
        }
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}

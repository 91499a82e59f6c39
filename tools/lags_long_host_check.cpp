// Host checks of shg_segment_lag_products_long under a sanitizer: the argument rules, the work items and the sizes of
// grates_amd/csrc/lags_long_host.h, which need no HIP.  A stand-alone program for the CPU:
//   hipcc -std=c++17 -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/lags_long_host_check.cpp -o lags_long_host_check
//   (or any host compiler: g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all ...) and run it: it prints "ok".
// Beyond the rules it replays, with plain arrays in place of LDS and the workspace, every index the kernels form: the slot of every
// chunk of clamped segment tables (each used once, all inside the table), and the staged values a wave reads at every quarter length.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../grates_amd/csrc/lags_long_host.h"

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
    const int status = segment_lag_products_long_check(rows, M, x ? &target : nullptr, ldx, lags, nseg, seg ? &target : nullptr,
                                                       s ? &target : nullptr, message, size);
    if (text && !std::strstr(message, text)) {
        std::printf("FAILED: '%s' not in '%s'\n", text, message);
        ++failures;
    }
    return status;
}

// the table as segment_range of lags_device.h reads it: clamped to 0 .. M, non-decreasing
static std::vector<int> clamped(const std::vector<long long>& seg, int M) {
    std::vector<int> out;
    int high = 0;
    for (long long v : seg) {
        high = std::max(high, (int)std::min<long long>(std::max<long long>(v, 0), M));
        out.push_back(high);
    }
    return out;
}

// what lag_long_slots_kernel writes: every slot exactly once, the chunks of a segment in consecutive slots of their own
static void slots_of(const std::vector<long long>& seg, int M) {
    const int nseg = (int)seg.size() - 1;
    const std::vector<int> c = clamped(seg, M);
    const LagLongGeometry g = segment_lag_products_long_geometry(1, M, nseg, kLagLongMax);
    std::vector<int> written((size_t)g.slots, 0), owner((size_t)g.slots, -1);
    long long chunks = 0;
    for (int s = 0; s < nseg; ++s) {
        const int start = c[s], end = c[s + 1];
        const long long own = lag_long_first_slot(start, s), from = s == 0 ? 0 : own;
        const long long to = s == nseg - 1 ? g.slots : lag_long_first_slot(end, s + 1);
        const int n = lag_long_chunks(end - start);
        expect(from >= 0 && from <= to && to <= g.slots && own + n <= to, "the slots of a segment lie inside the table and in front of the next segment's");
        int covered = 0;
        for (long long slot = from; slot < to; ++slot) {
            ++written[(size_t)slot];                                                          // the vector is the bound: ASan sees a stray index
            if (slot >= own && slot < own + n) {
                owner[(size_t)slot] = s;
                const int first = (int)(slot - own) * kLagLongChunk, left = end - start - first;
                expect(left > 0 && first == covered, "a used slot has columns left and starts where the chunk in front of it ends");
                const int take = lag_long_take(left);
                expect(take >= 1 && take <= kLagLongLongest && (take == left) == (slot == own + n - 1), "the last chunk, and no other, takes the rest");
                covered += take;
                ++chunks;
            }
        }
        expect(covered == end - start, "the chunks of a segment cover it once");
    }
    bool once = true;
    for (int count : written) once = once && count == 1;
    expect(once, "every slot is written exactly once");
    long long expected = 0;
    for (int s = 0; s < nseg; ++s) expected += lag_long_chunks(c[s + 1] - c[s]);
    expect(chunks == expected, "every chunk has a slot");
}

int main() {
    expect(check(6, 10, true, 10, 5, 2, true, true, nullptr) == 0, "valid arguments");
    expect(check(6, 10, true, 10, 0, 2, true, true, nullptr) == 0, "lags = 0");
    expect(check(6, 10, true, 10, 4095, 2, true, true, nullptr) == 0, "lags = 4095");
    expect(check(-1, 10, true, 10, 5, 2, true, true, "negative size") == -1, "negative rows");
    expect(check(6, -1, true, 10, 5, 2, true, true, "negative size") == -1, "negative M");
    expect(check(6, 10, true, -1, 5, 2, true, true, "negative size") == -1, "negative ldx");
    expect(check(6, 10, true, 10, -1, 2, true, true, "lags -1 outside 0 .. 4095") == -1, "lags = -1");
    expect(check(6, 10, true, 10, 4096, 2, true, true, "lags 4096 outside 0 .. 4095") == -1, "lags = 4096");
    expect(check(6, 10, true, 10, 5, -1, true, true, "nseg -1 is negative") == -1, "nseg");
    expect(check(6, 10, true, 9, 5, 2, true, true, "ldx 9 below M 10") == -1, "ldx");
    expect(check((1LL << 20) + 1, 1 << 20, true, 1 << 20, 5, 2, true, true, "values of X are too large") == -1, "X above 2^40");
    expect(check(1LL << 20, 4, true, 4, 15, (1 << 16) + 1, true, true, "values of S are too large") == -1, "S above 2^40");
    expect(check(1LL << 20, 4, true, 4, 15, 1 << 15, true, true, "of the workspace are too large") == -1, "the workspace alone above 2^40");
    expect(check(1, 2147483647, true, 2147483647, 0, 2147483647, true, true, "of the workspace are too large") == -1, "more slots than an int");
    expect(check(1LL << 62, 0, true, 0, 4095, 2147483647, true, true, "values of S are too large") == -1, "the largest sizes do not overflow");
    expect(check(0, 10, false, 10, 5, 2, false, false, nullptr) == 1, "rows = 0");
    expect(check(6, 10, false, 10, 5, 0, false, false, nullptr) == 1, "nseg = 0");
    expect(check(6, 10, false, 10, 4096, 0, false, false, "outside 0 .. 4095") == -1, "the checks come before the early return");
    expect(check(6, 10, false, 10, 5, 2, true, true, "NULL pointer") == -1, "NULL X");
    expect(check(6, 10, true, 10, 5, 2, false, true, "NULL pointer") == -1, "NULL seg");
    expect(check(6, 10, true, 10, 5, 2, true, false, "NULL pointer") == -1, "NULL S");
    expect(check(-1, 10, true, 10, 5, 2, true, true, nullptr, 8) == -1, "a short message buffer is not overrun");

    // sizes
    expect(kLagLongChunk == kLagLongWaves * kLagLongQuarter && (kLagLongMax + 1) % kLagLongTile == 0 && kLagLongSkew == 16 * 15, "constants");
    expect(kLagLongLds * sizeof(double) * 2 <= 160 * 1024, "two workgroups per CU");
    for (int lags = 0; lags <= kLagLongMax; ++lags) {
        const int tiles = lag_long_tiles(lags);
        expect(tiles >= 1 && tiles <= 16 && tiles * kLagLongTile > lags && (tiles - 1) * kLagLongTile <= lags, "the tiles cover the lags");
        for (long long rows : {1LL, 3LL, 1LL << 20}) {
            for (int nseg : {1, 240}) {
                const int M = 518400;
                const LagLongGeometry g = segment_lag_products_long_geometry(rows, M, nseg, lags);
                expect(g.tiles == tiles && g.slots == M / kLagLongChunk + nseg && g.items == rows * g.slots, "one item per row and slot");
                expect(g.blocks >= 1 && g.blocks <= (unsigned)kLagLongBlocks && g.blocks <= g.items, "workgroups");
                expect(g.partials == g.items * tiles * kLagLongTile && g.staged == lag_long_staged(tiles), "workspace");
                expect(g.staged + (kLagLongWaves - 1) * kLagLongGroup * kLagLongTile <= kLagLongLds && g.lds_bytes == kLagLongLds * sizeof(double), "LDS");
            }
        }
    }

    // every index of a sweep: a wave reads x[c0 + (lane >> 4)] and x[c0 + k0 + (lane & 15) + (lane >> 4)] of the staged values
    for (int tiles = 1; tiles <= 16; tiles += 5) {
        std::vector<double> staged((size_t)lag_long_staged(tiles), 1.0);
        double sum = 0.0;
        for (int take = 1; take <= kLagLongLongest; ++take) {
            const int quarter = lag_long_quarter(take);
            expect(quarter % 4 == 0 && kLagLongWaves * quarter >= take && (take > kLagLongChunk || quarter == kLagLongQuarter), "the quarters cover the chunk");
            for (int wave = 0; wave < kLagLongWaves; ++wave) {
                const int q0 = wave * quarter, length = std::min(quarter, take - q0), steps = lag_long_steps(length);
                expect(steps % 4 == 0 && (length <= 0 ? steps == 0 : 4 * steps >= length + kLagLongSkew && 4 * steps <= length + kLagLongSkew + 15),
                       "the steps cover the quarter and its skew, in fours");
                if (steps == 0) continue;
                const int last = q0 + 4 * (steps - 1) + 3;                                    // c0 + (lane >> 4) at most
                sum += staged[(size_t)last];
                sum += staged[(size_t)(last + 15 + kLagLongTile * (tiles - 1))];
            }
        }
        expect(sum > 0.0, "reads of the staged values");
    }

    // slots
    const int C = kLagLongChunk;
    slots_of({0, 1, 4, 300, 700}, 700);
    slots_of({3, 3, 70, 650}, 700);
    slots_of({0, 518400}, 518400);
    slots_of({0, C - 1, 2 * C - 1, 3 * C, 5 * C + 3}, 5 * C + 10);
    slots_of({5, 5 + C, 5 + C, 6 + 2 * C, 6 + 2 * C + 1}, 3 * C);
    slots_of({-5, 700 + 3, 20, 10}, 700);
    slots_of({2147483647LL, -2147483648LL, 5, 2}, 700);
    slots_of({0, 0, 0, 0}, 0);
    slots_of({C, 2 * C, 3 * C, 4 * C}, 4 * C);
    slots_of({C - 1, C, C + 1, 4 * C}, 4 * C);
    slots_of({0, C + kLagLongTail, 2 * C + 2 * kLagLongTail + 1, 5 * C}, 5 * C);
    {
        std::vector<long long> month;
        for (int a = 0; a <= 240; ++a) month.push_back(2160LL * a);
        slots_of(month, 518400);
    }
    unsigned state = 12345u;
    for (int round = 0; round < 200; ++round) {
        std::vector<long long> seg;
        state = state * 1664525u + 1013904223u;
        const int M = (int)(state >> 8) % (6 * C), n = 1 + (int)(state >> 3) % 9;
        for (int i = 0; i <= n; ++i) {
            state = state * 1664525u + 1013904223u;
            seg.push_back((long long)((state >> 8) % (unsigned)(M + 40)) - 20);
        }
        slots_of(seg, M);
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}

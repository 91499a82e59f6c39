// Host checks of shg_whiten_rows, shg_whiten_rows_long and shg_whiten_rows_vector under a sanitizer: the one contract of the three calls,
// grates_amd/csrc/whiten_host.h, which needs no HIP.  A stand-alone program for the CPU:
//   hipcc -std=c++17 -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/whiten_host_check.cpp -o whiten_host_check
//   (or any host compiler: g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all ...) and run it: it prints "ok".
#include <cstdio>
#include <cstring>

#include "../grates_amd/csrc/whiten_host.h"

using namespace shg;

static int failures = 0;

static void expect(bool ok, const char* name, const char* what) {
    if (!ok) {
        std::printf("FAILED: %s: %s\n", name, what);
        ++failures;
    }
}

static double buffer[4096];                  // X at its start; Y behind it, or inside it for the overlap rule
static int32_t stage_table[16];

struct Arguments {
    long long count = 6;                     // rows, or groups of `per` rows
    int per = 1, channels = 3, M = 10;
    const double* X = buffer;
    long long ldx = 10;
    const void* stage = stage_table;
    const void* taps = buffer;
    int q = 5, skip = 2;
    const double* Y = buffer + 2048;
    long long ldy = 8;
};

// the status, and `text` (if any) must be the whole message behind "<fn>: "
static int check(const WhitenCall& call, const Arguments& a, const char* text, size_t size = 256) {
    char message[256] = "";
    const int status = whiten_check(call, a.count, a.per, a.channels, a.M, a.X, a.ldx, a.stage, a.taps, a.q, a.skip, a.Y, a.ldy, message, size);
    char whole[320];
    std::snprintf(whole, sizeof(whole), "%s: %s", call.fn, text ? text : "");
    if (text ? std::strcmp(message, whole) != 0 : message[0] != 0) {
        std::printf("FAILED: %s: '%s' in place of '%s'\n", call.fn, message, text ? whole : "");
        ++failures;
    }
    return status;
}

// the rules that the three calls share; `joint`: groups of K rows without channels
static void shared_rules(const WhitenCall& call, int max_order, bool joint) {
    const char* fn = call.fn;
    Arguments valid;
    if (joint) valid.per = 3, valid.channels = 1, valid.ldx = 10;
    char text[256];
    Arguments a = valid;
    expect(check(call, a, nullptr) == 0, fn, "valid arguments");
    a = valid, a.q = 0;
    expect(check(call, a, nullptr) == 0, fn, "q = 0");
    a = valid, a.q = max_order;
    expect(check(call, a, nullptr) == 0, fn, "the largest order");
    a = valid, a.skip = 0, a.ldy = 10;
    expect(check(call, a, nullptr) == 0, fn, "skip = 0");

    const char* noun = joint ? "groups" : "rows";
    a = valid, a.count = -1;
    std::snprintf(text, sizeof(text), "negative size (%s -1, M 10, ldx 10, ldy 8)", noun);
    expect(check(call, a, text) == -1, fn, "negative count");
    a = valid, a.M = -1;
    std::snprintf(text, sizeof(text), "negative size (%s 6, M -1, ldx 10, ldy 8)", noun);
    expect(check(call, a, text) == -1, fn, "negative M");
    a = valid, a.ldx = -1;
    std::snprintf(text, sizeof(text), "negative size (%s 6, M 10, ldx -1, ldy 8)", noun);
    expect(check(call, a, text) == -1, fn, "negative ldx");
    a = valid, a.ldy = -1;
    std::snprintf(text, sizeof(text), "negative size (%s 6, M 10, ldx 10, ldy -1)", noun);
    expect(check(call, a, text) == -1, fn, "negative ldy");

    a = valid, a.q = -1;
    std::snprintf(text, sizeof(text), "order q -1 outside 0 .. %d", max_order);
    expect(check(call, a, text) == -1, fn, "q = -1");
    a = valid, a.q = max_order + 1;
    std::snprintf(text, sizeof(text), "order q %d outside 0 .. %d", max_order + 1, max_order);
    expect(check(call, a, text) == -1, fn, "q above the limit");
    a = valid, a.skip = -1;
    expect(check(call, a, "skip -1 outside 0 .. M 10") == -1, fn, "skip = -1");
    a = valid, a.skip = 11;
    expect(check(call, a, "skip 11 outside 0 .. M 10") == -1, fn, "skip above M");
    a = valid, a.ldx = 9;
    expect(check(call, a, "ldx 9 below M 10") == -1, fn, "ldx below M");
    a = valid, a.ldy = 7;
    expect(check(call, a, "ldy 7 below M - skip 8") == -1, fn, "ldy below M - skip");

    // nothing to do: after every rule on the sizes, before the pointers
    a = valid, a.count = 0, a.X = a.Y = nullptr, a.stage = a.taps = nullptr;
    expect(check(call, a, nullptr) == 1, fn, "count = 0");
    a = valid, a.skip = 10, a.ldy = 0, a.X = a.Y = nullptr, a.stage = a.taps = nullptr;
    expect(check(call, a, nullptr) == 1, fn, "M = skip");
    a = valid, a.count = 0, a.q = max_order + 1;
    expect(check(call, a, text) == -1, fn, "the rules come before the early return");

    a = valid, a.X = nullptr;
    expect(check(call, a, "NULL pointer") == -1, fn, "NULL X");
    a = valid, a.stage = nullptr;
    expect(check(call, a, "NULL pointer") == -1, fn, "NULL stage");
    a = valid, a.taps = nullptr;
    expect(check(call, a, "NULL pointer") == -1, fn, "NULL taps");
    a = valid, a.Y = nullptr;
    expect(check(call, a, "NULL pointer") == -1, fn, "NULL Y");

    // X holds rows * ldx - (ldx - M) doubles from its start, Y rows * ldy - (ldy - (M - skip)): they may touch and not overlap
    const long long rows = valid.count * valid.per, x_span = (rows - 1) * valid.ldx + valid.M, y_span = (rows - 1) * valid.ldy + (valid.M - valid.skip);
    a = valid, a.Y = buffer + x_span;
    expect(check(call, a, nullptr) == 0, fn, "Y right behind X");
    a = valid, a.Y = buffer + x_span - 1;
    expect(check(call, a, "X and Y overlap (the call is out of place)") == -1, fn, "Y starts in the last value of X");
    a = valid, a.Y = buffer;
    expect(check(call, a, "X and Y overlap (the call is out of place)") == -1, fn, "in place");
    a = valid, a.X = buffer + y_span, a.Y = buffer;
    expect(check(call, a, nullptr) == 0, fn, "X right behind Y");
    a = valid, a.X = buffer + y_span - 1, a.Y = buffer;
    expect(check(call, a, "X and Y overlap (the call is out of place)") == -1, fn, "X starts in the last value of Y");

    a = valid, a.count = -1;
    expect(check(call, a, nullptr, 0) == -1 && check(call, a, nullptr, 1) == -1, fn, "a message buffer of no length is not written");
    char small[8];
    expect(whiten_check(call, -1, a.per, a.channels, a.M, a.X, a.ldx, a.stage, a.taps, a.q, a.skip, a.Y, a.ldy, small, sizeof(small)) == -1 &&
               std::strlen(small) == sizeof(small) - 1,
           fn, "a short message buffer is not overrun");
}

// rows with channels: shg_whiten_rows and shg_whiten_rows_long
static void row_rules(const WhitenCall& call) {
    const char* fn = call.fn;
    Arguments a;
    a.channels = 0;
    expect(check(call, a, "channels 0 below 1") == -1, fn, "channels = 0");
    a = Arguments(), a.channels = 4;
    expect(check(call, a, "rows 6 are not a multiple of channels 4") == -1, fn, "rows and channels");
    a = Arguments(), a.per = 1, a.channels = 1, a.count = (1LL << 20) + 1, a.M = 1 << 20, a.ldx = 1 << 20, a.ldy = 1 << 20;
    expect(check(call, a, "1048577 rows of 1048576 (X) and 1048576 (Y) values are too large") == -1, fn, "X above 2^40");
    a.ldx = 1LL << 20, a.ldy = 1LL << 21, a.count = 1 << 20;
    expect(check(call, a, "1048576 rows of 1048576 (X) and 2097152 (Y) values are too large") == -1, fn, "Y above 2^40");
    a = Arguments(), a.channels = 1, a.count = 1LL << 62, a.M = 0, a.skip = 0, a.ldx = 0, a.ldy = 0;
    expect(check(call, a, nullptr) == 1, fn, "the largest count of empty rows does not overflow");
}

// groups of K rows: shg_whiten_rows_vector
static void group_rules(const WhitenCall& call) {
    const char* fn = call.fn;
    Arguments valid;
    valid.per = 3, valid.channels = 1;
    Arguments a = valid;
    for (int K = kVectorMinDim; K <= kVectorMaxDim; ++K) {
        a.per = K;
        expect(check(call, a, nullptr) == 0, fn, "every dimension");
    }
    a = valid, a.per = 1;
    expect(check(call, a, "dimension K 1 outside 2 .. 6") == -1, fn, "K = 1");
    a = valid, a.per = 0;
    expect(check(call, a, "dimension K 0 outside 2 .. 6") == -1, fn, "K = 0");
    a = valid, a.per = 7;
    expect(check(call, a, "dimension K 7 outside 2 .. 6") == -1, fn, "K = 7");
    a = valid, a.channels = 0;
    expect(check(call, a, nullptr) == 0, fn, "groups have no channels");
    a = valid, a.count = (1LL << 40) / 3 + 1, a.M = 0, a.skip = 0, a.ldx = 0, a.ldy = 0;
    expect(check(call, a, "366503875926 groups of 3 rows are too large") == -1, fn, "groups above 2^40 / K");
    a.count = (1LL << 40) / 3;
    expect(check(call, a, nullptr) == 1, fn, "groups of 2^40 / K empty rows");
    a.count = 1LL << 62;
    expect(check(call, a, "4611686018427387904 groups of 3 rows are too large") == -1, fn, "the largest count does not overflow");
    a = valid, a.count = (1LL << 19) + 1, a.per = 2, a.M = 1 << 20, a.ldx = 1 << 20, a.ldy = 1 << 20;
    expect(check(call, a, "524289 groups of 2 rows of 1048576 (X) and 1048576 (Y) values are too large") == -1, fn, "X above 2^40");
}

int main() {
    shared_rules(kWhitenRows, 128, false);
    shared_rules(kWhitenRowsLong, 4095, false);
    shared_rules(kWhitenRowsVector, 128, true);
    row_rules(kWhitenRows);
    row_rules(kWhitenRowsLong);
    group_rules(kWhitenRowsVector);
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}

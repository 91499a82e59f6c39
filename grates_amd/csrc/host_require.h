// The refusal of the host-side argument checks (arcs_host.h, lags_host.h, lags_long_host.h, whiten_host.h), without any HIP: inside
// a check function with the parameters `char* message, size_t size` that returns 0 (launch), 1 (nothing to do) or -1 (refused).
#pragma once

#include <cstddef>
#include <cstdio>

#define SHG_HOST_REQUIRE(cond, ...)                                                  \
    do {                                                                             \
        if (!(cond)) return snprintf(message, size, __VA_ARGS__), -1;                \
    } while (0)

// A/B timer of the potential's design matrix: the direct kernel that ships (shg_potential_design: one lane per
// point, every harmonic stored straight to its row) against the table route of the other design matrices, which lives only here:
// design_harmonics_kernel<false> writes Y of degree N to a workspace and design_gather_kernel<1, 1> copies one slot per row, under the
// pass driver design_passes with a table of one term per row.  Both routes must give the same bits.  A stand-alone program that
// compiles grates_amd/csrc/design.hip into itself and links the library's other objects (after `make -C grates_amd/csrc`; not
// libshg.so, whose copy of these kernels would be registered under the same handles):
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -Iinclude -c tools/potential_design_ab.hip -o ab.o
//   hipcc --offload-arch=gfx950 ab.o $(ls grates_amd/csrc/build/*.o | grep -v '/design.o\|_timeline') -o tools/scratch/potential_design_ab
//   tools/scratch/potential_design_ab [N = 96] [repeats = 100] > profiles/potential_design_ab.txt
// M is NormalEquations.default_block_points(P, 1) = max(256 MB / (8 P) rounded down to a multiple of 256, 256), min_degree 0.  The two
// routes alternate call by call in one process; a call is timed with device events around the whole entry point (host table, upload,
// wait and kernels) and, for the kernels alone, between an event recorded after the upload's wait and the end.  Bytes from shapes:
// the direct route writes P M doubles; the table route writes 2 packed(N) M doubles of Y, reads P M of them and writes P M.
#include "../grates_amd/csrc/design.hip"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

// the table of the potential: row (n, j) is the one slot 2 packed(n, k) + kind of Y of degree N, factor 1
static void potential_design_table(int N, int min_degree, int* slot, double* factor) {
    size_t row = 0;
    for (int n = min_degree; n <= N; ++n)
        for (int j = 0; j <= 2 * n; ++j, ++row) {
            slot[row] = term_slot(N, unit_coefficient(n, j));
            factor[row] = 1.0;
        }
}

static hipEvent_t g_mark;                             // recorded where the kernels of a call start

static int table_route(int N, int min_degree, const double* xyz, int M, const double* weights, double GM, double R, double* At, int ldt,
                       hipStream_t stream) {
    const char* fn = "table_route";
    if (int rc = check_design(fn, N, min_degree, 0, M, 1, weights ? SHG_WEIGHTS_POINT : SHG_WEIGHTS_NONE, GM, R, ldt)) return rc;
    const unsigned P = (unsigned)design_rows(N, min_degree);
    return design_passes(fn, N, 1, N, min_degree, potential_design_table, 1, M, stream, [&](const DesignPass& d, int p0, int np) {
        if (p0 == 0) (void)hipEventRecord(g_mark, stream);
        hipLaunchKernelGGL(design_harmonics_kernel<false>, dim3(ceil_div(np, 256)), dim3(256), 0, stream, N, np, xyz + (size_t)p0 * 3, nullptr, d.ab, R, d.Y,
                           d.ldy, (size_t)0);
        hipLaunchKernelGGL((design_gather_kernel<1, 1>), dim3(P, ceil_div(np, 256)), dim3(256), 0, stream, np, d.Y, d.ldy, d.slot, d.factor,
                           weights ? weights + p0 : nullptr, weights ? 1 : 0, GM / R, At + p0, (size_t)ldt);
    });
}

#define CHECK(call)                                                                       \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess) {                                                           \
            std::printf("%s failed: %s\n", #call, hipGetErrorString(e_));                 \
            return 1;                                                                     \
        }                                                                                 \
    } while (0)

static double median(std::vector<float> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

int main(int argc, char** argv) {
    const int N = argc > 1 ? std::atoi(argv[1]) : 96, repeats = argc > 2 ? std::atoi(argv[2]) : 100;
    const double GM = 3.9860044150e+14, R = 6.3781363000e+06;
    const long long P = design_rows(N, 0);
    const int M = (int)std::max<long long>((256LL << 20) / (8 * P) / 256 * 256, 256);
    std::vector<double> xyz((size_t)M * 3);
    unsigned long long state = 2891;                  // seeded points 350 .. 550 km above R, any direction
    auto uniform = [&] {
        state = state * 6364136223846793005ULL + 1442695040888963407ULL;
        return (double)(state >> 11) / 9007199254740992.0;
    };
    for (int i = 0; i < M; ++i) {
        const double z = 2.0 * uniform() - 1.0, lon = 6.283185307179586 * uniform(), r = R + 350e3 + 200e3 * uniform(), rho = std::sqrt(1.0 - z * z);
        xyz[3 * (size_t)i] = r * rho * std::cos(lon);
        xyz[3 * (size_t)i + 1] = r * rho * std::sin(lon);
        xyz[3 * (size_t)i + 2] = r * z;
    }
    hipStream_t stream;
    CHECK(hipStreamCreate(&stream));
    double *x_d, *direct_d, *table_d;
    const size_t count = (size_t)P * M;
    CHECK(hipMalloc((void**)&x_d, xyz.size() * sizeof(double)));
    CHECK(hipMalloc((void**)&direct_d, count * sizeof(double)));
    CHECK(hipMalloc((void**)&table_d, count * sizeof(double)));
    CHECK(hipMemcpy(x_d, xyz.data(), xyz.size() * sizeof(double), hipMemcpyHostToDevice));
    hipEvent_t t0, t1;
    CHECK(hipEventCreate(&t0));
    CHECK(hipEventCreate(&t1));
    CHECK(hipEventCreate(&g_mark));
    std::vector<float> call[2], kernels[2];
    for (int it = -3; it < repeats; ++it) {           // three warm-up rounds
        for (int route = 0; route < 2; ++route) {
            CHECK(hipEventRecord(t0, stream));
            int rc;
            if (route == 0)
                rc = shg_potential_design(N, 0, x_d, M, nullptr, GM, R, direct_d, M, stream);      // the shipping entry point
            else
                rc = table_route(N, 0, x_d, M, nullptr, GM, R, table_d, M, stream);
            CHECK(hipEventRecord(t1, stream));
            CHECK(hipEventSynchronize(t1));
            if (rc) {
                std::printf("route %d failed: %s\n", route, shg_last_error());
                return 1;
            }
            float ms = 0.0f, ms_kernels = 0.0f;
            CHECK(hipEventElapsedTime(&ms, t0, t1));
            if (route == 1) CHECK(hipEventElapsedTime(&ms_kernels, g_mark, t1));
            if (it >= 0) {
                call[route].push_back(ms);
                kernels[route].push_back(ms_kernels);
            }
        }
    }
    // the direct route's kernel alone, as the entry point launches it, on recursion factors uploaded once
    std::vector<float> direct_kernel;
    {
        std::vector<double> fa, fb, h(2 * (size_t)packed_count(N));
        recursion_tables(N, fa, fb);
        for (size_t i = 0; i < fa.size(); ++i) {
            h[2 * i] = fa[i];
            h[2 * i + 1] = fb[i];
        }
        double2* ab_d;
        CHECK(hipMalloc((void**)&ab_d, h.size() * sizeof(double)));
        CHECK(hipMemcpy(ab_d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
        for (int it = -3; it < repeats; ++it) {
            CHECK(hipEventRecord(t0, stream));
            hipLaunchKernelGGL(potential_design_kernel<false>, dim3(ceil_div(M, kPotLanes), ceil_div(N + 1, kPotOrders)), dim3(kPotLanes), 0, stream, N, 0, M,
                               x_d, (const double*)nullptr, ab_d, (const double*)nullptr, R, GM / R, direct_d, (size_t)M);
            CHECK(hipEventRecord(t1, stream));
            CHECK(hipEventSynchronize(t1));
            float ms = 0.0f;
            CHECK(hipEventElapsedTime(&ms, t0, t1));
            if (it >= 0) direct_kernel.push_back(ms);
        }
        CHECK(hipFree(ab_d));
    }
    std::vector<double> a(count), b(count);
    CHECK(hipMemcpy(a.data(), direct_d, count * sizeof(double), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(b.data(), table_d, count * sizeof(double), hipMemcpyDeviceToHost));
    size_t different = 0;
    double worst = 0.0, largest = 0.0;
    for (size_t i = 0; i < count; ++i) {
        different += a[i] != b[i];
        worst = std::max(worst, std::fabs(a[i] - b[i]));
        largest = std::max(largest, std::fabs(a[i]));
    }
    if (different) {
        const double r0 = std::sqrt((xyz[0] * xyz[0] + xyz[1] * xyz[1]) + xyz[2] * xyz[2]);
        std::printf("largest difference %.3e of max|At| %.3e; row 0, point 0: direct %.17g, table %.17g, GM / r %.17g\n", worst, largest, a[0], b[0],
                    (R / r0) * (GM / R));
        for (size_t i : {(size_t)1, (size_t)M, count / 2, count - 1}) std::printf("  entry %zu: direct %.17g, table %.17g\n", i, a[i], b[i]);
    }
    const double packed = (double)packed_count(N);
    const double direct_bytes = 8.0 * P * M, table_bytes = 8.0 * M * (2.0 * packed + 2.0 * P);
    const double d_ms = median(call[0]), t_ms = median(call[1]), tk_ms = median(kernels[1]);
    std::printf("potential design, d/o %d, P %lld, M %d, %d alternating repeats (medians; minimum in brackets)\n", N, P, M, repeats);
    std::printf("direct call : %8.3f ms [%8.3f]  %7.1f GB/s of %.1f MB from shapes\n", d_ms, *std::min_element(call[0].begin(), call[0].end()),
                direct_bytes / d_ms / 1e6, direct_bytes / 1e6);
    std::printf("table call  : %8.3f ms [%8.3f]  %7.1f GB/s of %.1f MB from shapes (%.2f x the direct call)\n", t_ms,
                *std::min_element(call[1].begin(), call[1].end()), table_bytes / t_ms / 1e6, table_bytes / 1e6, t_ms / d_ms);
    const double dk_ms = median(direct_kernel);
    std::printf("direct kernel alone                     : %8.3f ms  %7.1f GB/s\n", dk_ms, direct_bytes / dk_ms / 1e6);
    std::printf("table kernels alone (harmonics + gather): %8.3f ms  %7.1f GB/s (%.2f x the direct kernel)\n", tk_ms, table_bytes / tk_ms / 1e6,
                tk_ms / dk_ms);
    std::printf("entries that differ between the routes: %zu of %zu\n", different, count);
    return different ? 2 : 0;
}

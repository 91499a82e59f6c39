// Basin geometry and basin statistics of grid series.
//   shg_basin_pip         replaces the per-point work of spherical_pip              (grates/grid.py:1751-1824)
//   shg_basin_buffer      replaces the per-point work of spherical_pib              (grates/grid.py:1827-1890)
//   shg_winding_number    replaces winding_number                                   (grates/grid.py:1715-1748)
//   shg_mask_pack         bool masks [B][P] -> one uint64 of mask bits per point
//   shg_basin_statistics  Grid.mean / rms / std (mask) for every epoch and mask     (grates/grid.py:174-260)
//
// Point-in-polygon: the host does the O(k) work per polygon in the reference's NumPy operations (unit vertices, the
// antipode a of their mean, the cap bound, and per edge q = b0 x b1, b0 x q, b1 x q); the device does the per-point work.
// A first pass tests every point against the polygon's spherical cap and appends the survivors to a compacted index list
// (one atomic per wave: the order of the list varies from run to run, the result per point does not); the second pass
// walks the list, one lane per point, with the edge table staged in LDS chunk by chunk so that the edge loop is
// wave-uniform and the table is read as LDS broadcasts.  The arithmetic mirrors the reference element by element (built
// with -ffp-contract=off: no FMA; cross products as NumPy forms them; three-term sums as ((x0 + x1) + x2); true division
// by sqrt): results agree with the reference except at points whose answer the reference's own rounding decides (its cap
// test and its buffer products go through BLAS).
//
// Statistics: lane <-> epoch, a workgroup owns a tile of points and 256 epochs; the values of 16 points x 256 epochs are
// staged through LDS (coalesced loads of the next chunk are in flight while the current one is summed), the weight and the
// mask bits of a point are wave-uniform, so the mask loop branches on scalar bits, four masks at a time, and only the groups
// of masks that contain a point cost vector work.  Partial sums per tile are reduced over the tiles in a fixed order by a
// second kernel (no atomics: bitwise reproducible).  Pass 1 gives sum w v and sum w v^2 per (epoch, mask) -- an extra row of ones gives sum w --,
// pass 2 sum w (v - mean)^2 (the reference's two-pass std).
#include "common.h"

#include <algorithm>

namespace shg {

// ---- points ----------------------------------------------------------------------------------------------------------
// Regular grid (xyz == NULL): point i = (parallel i / nlon, meridian i % nlon); lat_tab [2][nlat] = ((N + h) cos phi,
// ((1 - e^2) N + h) sin phi), lon_tab [2][nlon] = (cos lambda, sin lambda): x = (N cos phi) cos lambda as in
// geodetic2cartesian (grates/grid.py:1920-1950).  Point list: xyz [n][3] as geodetic2cartesian gives it.
struct Points {
    int nlat, nlon;
    const double* lat_tab;
    const double* lon_tab;
    const double* xyz;
    long long n;
};

__device__ __forceinline__ void unit_point(const Points& s, long long i, double& x, double& y, double& z) {
    if (s.xyz) {
        x = s.xyz[3 * i];
        y = s.xyz[3 * i + 1];
        z = s.xyz[3 * i + 2];
    } else {
        const long long r = i / s.nlon;
        const long long c = i - r * s.nlon;
        const double rc = s.lat_tab[r];
        x = rc * s.lon_tab[c];
        y = rc * s.lon_tab[s.nlon + c];
        z = s.lat_tab[s.nlat + r];
    }
    const double nrm = sqrt((x * x + y * y) + z * z);     // xyz /= np.sqrt(np.sum(xyz**2, axis=1))
    x = x / nrm;
    y = y / nrm;
    z = z / nrm;
}

// np.cross(u, v) for 3-vectors: products first, then the difference
__device__ __forceinline__ void cross3(double u0, double u1, double u2, double v0, double v1, double v2, double& c0, double& c1, double& c2) {
    c0 = u1 * v2 - u2 * v1;
    c1 = u2 * v0 - u0 * v2;
    c2 = u0 * v1 - u1 * v0;
}

__device__ __forceinline__ double dot3(double u0, double u1, double u2, double v0, double v1, double v2) {
    return (u0 * v0 + u1 * v1) + u2 * v2;
}

struct Frame {
    double a0, a1, a2, bound;
};

// Cap test (-x . a >= bound) and compaction of the points inside: list[1 + k] = point index, list[0] = count.  first != 0:
// also clears the mask of every point (the parities of several polygons are XOR-ed into it).
__global__ __launch_bounds__(256) void cap_kernel(Points s, Frame f, int first, unsigned long long* __restrict__ list,
                                                  unsigned char* __restrict__ mask) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool in = false;
    if (i < s.n) {
        double x, y, z;
        unit_point(s, i, x, y, z);
        in = ((-x) * f.a0 + (-y) * f.a1) + (-z) * f.a2 >= f.bound;
        if (first) mask[i] = 0;
    }
    const unsigned long long bal = __ballot(in);
    const int lane = threadIdx.x & 63;
    unsigned long long base = 0;
    if (lane == 0 && bal) base = atomicAdd(list, (unsigned long long)__popcll(bal));
    base = __shfl(base, 0, 64);
    if (in) list[1 + base + __popcll(bal & ((1ull << lane) - 1))] = (unsigned long long)i;
}

__global__ void list_reset_kernel(unsigned long long* list) { list[0] = 0; }

constexpr int kPipChunk = 256;          // edges per LDS chunk: 256 x 9 doubles = 18 KB
constexpr int kPibChunk = 128;          // 128 x 16 doubles = 16 KB

// Crossing count of the great-circle segment a -> x with every edge (grates/grid.py:1795-1822).  edges [k][9] =
// (q, b0 x q, b1 x q) with b0 = vertex e + 1, b1 = vertex e of the closed polygon.
__global__ __launch_bounds__(256) void pip_kernel(Points s, Frame f, int nedges, const double* __restrict__ edges,
                                                  const unsigned long long* __restrict__ list, unsigned char* __restrict__ mask) {
    __shared__ double tab[kPipChunk * 9];
    const unsigned long long count = list[0];
    for (unsigned long long base = (unsigned long long)blockIdx.x * 256; base < count; base += (unsigned long long)gridDim.x * 256) {
        const bool active = base + threadIdx.x < count;
        long long i = 0;
        double p0 = 0, p1 = 0, p2 = 0, xp0 = 0, xp1 = 0, xp2 = 0, ap0 = 0, ap1 = 0, ap2 = 0;
        if (active) {
            i = (long long)list[1 + base + threadIdx.x];
            double x, y, z;
            unit_point(s, i, x, y, z);
            cross3(x, y, z, f.a0, f.a1, f.a2, p0, p1, p2);              // p = x x a
            cross3(x, y, z, p0, p1, p2, xp0, xp1, xp2);                 // x x p
            cross3(f.a0, f.a1, f.a2, p0, p1, p2, ap0, ap1, ap2);        // a x p
        }
        int parity = 0;
        for (int e0 = 0; e0 < nedges; e0 += kPipChunk) {
            const int ne = min(kPipChunk, nedges - e0);
            __syncthreads();
            for (int k = threadIdx.x; k < ne * 9; k += 256) tab[k] = edges[(size_t)e0 * 9 + k];
            __syncthreads();
            if (!active) continue;
            for (int e = 0; e < ne; ++e) {
                const double* E = tab + 9 * e;
                double t0, t1, t2;
                cross3(p0, p1, p2, E[0], E[1], E[2], t0, t1, t2);      // t = p x q
                const double nt = sqrt((t0 * t0 + t1 * t1) + t2 * t2);
                if (!(nt > 0)) continue;                                 // parallel great circles: no crossing
                t0 = t0 / nt;
                t1 = t1 / nt;
                t2 = t2 / nt;
                const double s1 = dot3(xp0, xp1, xp2, t0, t1, t2);
                const double s2 = dot3(ap0, ap1, ap2, t0, t1, t2);
                const double s3 = dot3(E[3], E[4], E[5], t0, t1, t2);
                const double s4 = dot3(E[6], E[7], E[8], t0, t1, t2);
                // sign(-s1) + sign(s2) + sign(-s3) + sign(s4) == +-4
                parity ^= (int)((s1 < 0 && s2 > 0 && s3 < 0 && s4 > 0) || (s1 > 0 && s2 < 0 && s3 > 0 && s4 < 0));
            }
        }
        if (active && parity) mask[i] ^= 1;
    }
}

// Buffer test (grates/grid.py:1862-1890): within cos(buffer / a) of a vertex or of the arc of an edge.  edges [k][16] =
// (b0, b1, n = (b0 x b1) / |b0 x b1|, b0 x b1, b1 x b0, valid).  A point found inside gets mask = value.
__global__ __launch_bounds__(256) void pib_kernel(Points s, double cosb, int nedges, const double* __restrict__ edges,
                                                  const unsigned long long* __restrict__ list, unsigned char value,
                                                  unsigned char* __restrict__ mask) {
    __shared__ double tab[kPibChunk * 16];
    const unsigned long long count = list[0];
    for (unsigned long long base = (unsigned long long)blockIdx.x * 256; base < count; base += (unsigned long long)gridDim.x * 256) {
        const bool active = base + threadIdx.x < count;
        long long i = 0;
        double x = 0, y = 0, z = 0;
        if (active) {
            i = (long long)list[1 + base + threadIdx.x];
            unit_point(s, i, x, y, z);
        }
        bool in = false;
        for (int e0 = 0; e0 < nedges; e0 += kPibChunk) {
            const int ne = min(kPibChunk, nedges - e0);
            if (!__syncthreads_or(active && !in)) break;            // every point of the block decided: early exit
            for (int k = threadIdx.x; k < ne * 16; k += 256) tab[k] = edges[(size_t)e0 * 16 + k];
            __syncthreads();
            if (!active) continue;
            for (int e = 0; e < ne && !in; ++e) {
                const double* E = tab + 16 * e;
                if (cosb <= dot3(x, y, z, E[0], E[1], E[2]) || cosb <= dot3(x, y, z, E[3], E[4], E[5])) {
                    in = true;
                    break;
                }
                if (E[15] == 0.0) continue;                              // |b0 x b1| == 0: no arc
                const double sn = dot3(x, y, z, E[6], E[7], E[8]);
                double q0 = x - sn * E[6], q1 = y - sn * E[7], q2 = z - sn * E[8];
                const double nq = sqrt((q0 * q0 + q1 * q1) + q2 * q2);
                q0 = q0 / nq;
                q1 = q1 / nq;
                q2 = q2 / nq;
                double c0, c1, c2, d0, d1, d2;
                cross3(E[0], E[1], E[2], q0, q1, q2, c0, c1, c2);      // b0 x p
                cross3(E[3], E[4], E[5], q0, q1, q2, d0, d1, d2);      // b1 x p
                if (dot3(c0, c1, c2, E[9], E[10], E[11]) >= 0 && dot3(d0, d1, d2, E[12], E[13], E[14]) >= 0 &&
                    cosb <= dot3(q0, q1, q2, x, y, z))
                    in = true;
            }
        }
        if (active && in) mask[i] = value;
    }
}

// Planar winding number (grates/grid.py:1715-1748), element-wise.  edges [k][5] = (x0, y0, y1, x1 - x0, y1 - y0).
__global__ __launch_bounds__(256) void winding_kernel(int nedges, const double* __restrict__ edges, const double* __restrict__ px,
                                                      const double* __restrict__ py, long long n, unsigned char* __restrict__ mask) {
    __shared__ double tab[kPipChunk * 5];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool active = i < n;
    const double x = active ? px[i] : 0.0, y = active ? py[i] : 0.0;
    int wn = 0;
    for (int e0 = 0; e0 < nedges; e0 += kPipChunk) {
        const int ne = min(kPipChunk, nedges - e0);
        __syncthreads();
        for (int k = threadIdx.x; k < ne * 5; k += 256) tab[k] = edges[(size_t)e0 * 5 + k];
        __syncthreads();
        for (int e = 0; e < ne; ++e) {
            const double* E = tab + 5 * e;
            const bool l1 = E[1] <= y, l2 = E[2] > y;
            const double loc = E[3] * (y - E[1]) - (x - E[0]) * E[4];
            wn += (l1 && l2 && loc > 0) ? 1 : 0;
            wn -= (!l1 && !l2 && loc < 0) ? 1 : 0;
        }
    }
    if (active) mask[i] = wn != 0;
}

// ---- statistics -------------------------------------------------------------------------------------------------------
constexpr int kStatRows = 256;         // epochs per workgroup (lane <-> epoch)
constexpr int kStatPts = 16;           // points per LDS chunk
constexpr int kStatLd = kStatPts + 1;  // row pitch: lanes l and l + 1 read 8-byte words 17 apart, on distinct banks

__global__ __launch_bounds__(256) void mask_pack_kernel(const unsigned char* __restrict__ masks, int B, long long P,
                                                        unsigned long long* __restrict__ bits) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    unsigned long long m = 0;
    for (int b = 0; b < B; ++b) m |= (unsigned long long)(masks[(size_t)b * P + p] != 0) << b;
    bits[p] = m;
}

// PASS 1: partial[tile][r][b][0..1] = sums over the tile of w v and w v^2 for rows r < T, of w (row T, v = 1).
// PASS 2: partial[tile][r][b] = sum over the tile of w (v - mean[r][b])^2.
template <int NB, int PASS>
__global__ __launch_bounds__(256) void stats_kernel(const double* __restrict__ V, int T, long long P, const double* __restrict__ w,
                                                    const unsigned long long* __restrict__ bits, long long tile,
                                                    const double* __restrict__ mean, double* __restrict__ partial) {
    constexpr int K = PASS == 1 ? 2 : 1;
    __shared__ double lds[kStatRows * kStatLd];
    const int rows = PASS == 1 ? T + 1 : T;
    const int r0 = blockIdx.y * kStatRows;
    const int r = r0 + threadIdx.x;
    const long long t0 = (long long)blockIdx.x * tile;
    const long long t1 = t0 + tile < P ? t0 + tile : P;

    double a1[NB], a2[NB], mu[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        a1[b] = 0.0;
        a2[b] = 0.0;
        mu[b] = (PASS == 2 && r < T) ? mean[(size_t)r * NB + b] : 0.0;
    }

    // staging: element k of a thread's share is (row, col) = ((tid + 256 k) / 16, (tid + 256 k) % 16): a wave reads four
    // rows of 16 consecutive points (128 B each) per load
    constexpr int kShare = kStatRows * kStatPts / 256;
    double stage[kShare];
    // the mask bits and weights of a chunk travel with its values (16 lanes load them, LDS hands them to every lane): read
    // point by point through scalar loads, each a dependent cache access, they cost more than the values themselves
    __shared__ unsigned long long lds_bits[kStatPts];
    __shared__ double lds_w[kStatPts];
    unsigned long long stage_bits = 0;
    double stage_w = 0.0;
    auto load = [&](long long pc) {
        if (threadIdx.x < kStatPts) {
            const long long p = pc + threadIdx.x;
            stage_bits = p < t1 ? bits[p] : 0ull;
            stage_w = p < t1 ? w[p] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < kShare; ++k) {
            const int e = threadIdx.x + 256 * k, row = r0 + e / kStatPts;
            const long long p = pc + e % kStatPts;
            double v = 0.0;
            if (p < t1) {
                if (row < T) v = __builtin_nontemporal_load(V + (size_t)row * P + p);
                else if (PASS == 1 && row == T) v = 1.0;
            }
            stage[k] = v;
        }
    };
    if (t0 < t1) load(t0);
    for (long long pc = t0; pc < t1; pc += kStatPts) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kShare; ++k) {
            const int e = threadIdx.x + 256 * k;
            lds[(e / kStatPts) * kStatLd + e % kStatPts] = stage[k];
        }
        if (threadIdx.x < kStatPts) {
            lds_bits[threadIdx.x] = stage_bits;
            lds_w[threadIdx.x] = stage_w;
        }
        __syncthreads();
        if (pc + kStatPts < t1) load(pc + kStatPts);
#pragma unroll 4
        for (int k = 0; k < kStatPts; ++k) {
            const unsigned long long mv = lds_bits[k];
            const unsigned long long m = ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(mv >> 32)) << 32) |
                                         (unsigned)__builtin_amdgcn_readfirstlane((unsigned)mv);     // the same for every lane
            if (!m) continue;
            const double wk = lds_w[k];
            const double v = lds[threadIdx.x * kStatLd + k];
            if (PASS == 1) {
                const double wv = wk * v, wv2 = wv * v;
#pragma unroll
                for (int g = 0; g < NB; g += 4) {
                    if (!((m >> g) & 15)) continue;                    // a scalar branch past masks that miss the point
#pragma unroll
                    for (int b = g; b < g + 4 && b < NB; ++b)
                        if ((m >> b) & 1) {
                            a1[b] += wv;
                            a2[b] += wv2;
                        }
                }
            } else {
#pragma unroll
                for (int g = 0; g < NB; g += 4) {
                    if (!((m >> g) & 15)) continue;
#pragma unroll
                    for (int b = g; b < g + 4 && b < NB; ++b)
                        if ((m >> b) & 1) {
                            const double d = v - mu[b];
                            a1[b] += (wk * d) * d;
                        }
                }
            }
        }
    }
    if (r >= rows) return;
    double* out = partial + ((size_t)blockIdx.x * rows + r) * NB * K;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        out[b * K] = a1[b];
        if (K == 2) out[b * K + 1] = a2[b];
    }
}

// Sums of the partials over the tiles, one wave per (epoch, mask): lane l adds the tiles l, l + 64, ... in order, a butterfly adds
// the lanes (a fixed order: the same bits in every run).  PASS 1: mean, rms; mean and sum w kept in `keep` ([T][NB] means,
// then [NB] sums of w) for pass 2.  PASS 2: std.  out = [3][T][B] (mean, rms, std).
template <int NB, int PASS>
__global__ __launch_bounds__(256) void stats_reduce_kernel(int T, int B, int ntiles, const double* __restrict__ partial,
                                                           double* __restrict__ keep, double* __restrict__ out) {
    constexpr int K = PASS == 1 ? 2 : 1;
    const int idx = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (idx >= T * NB) return;
    const int t = idx / NB, b = idx % NB;
    const int rows = PASS == 1 ? T + 1 : T;
    const size_t stride = (size_t)rows * NB * K;
    double s1 = 0.0, s2 = 0.0, sw = 0.0;
    const double* q = partial + ((size_t)t * NB + b) * K;
    const double* qw = partial + ((size_t)T * NB + b) * K;
    for (int k = lane; k < ntiles; k += 64) {
        s1 += q[k * stride];
        if (PASS == 1) {
            s2 += q[k * stride + 1];
            sw += qw[k * stride];
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o);
        if (PASS == 1) {
            s2 += __shfl_xor(s2, o);
            sw += __shfl_xor(sw, o);
        }
    }
    if (lane != 0) return;
    double* means = keep;
    double* sums_w = keep + (size_t)T * NB;
    if (PASS == 1) {
        const double mu = s1 / sw;
        means[idx] = mu;
        if (t == 0) sums_w[b] = sw;
        if (b < B) {
            out[(size_t)t * B + b] = mu;
            out[(size_t)T * B + (size_t)t * B + b] = sqrt(s2 / sw);
        }
    } else if (b < B) {
        out[2 * (size_t)T * B + (size_t)t * B + b] = sqrt(s1 / sums_w[b]);
    }
}

template <int NB>
int basin_statistics(const double* V, int T, long long P, const double* w, const unsigned long long* bits, int B, double* out,
                     hipStream_t stream) {
    // tiles: about 1024 workgroups (512 with 64 masks, whose partials are 4x larger), a whole number of LDS chunks each
    const long long target = NB <= 16 ? 1024 : 512;
    long long tile = (P + target - 1) / target;
    tile = (tile + kStatPts - 1) / kStatPts * kStatPts;
    const long long ntiles = (P + tile - 1) / tile;
    SHG_REQUIRE(ntiles <= 0x7fffffff, "shg_basin_statistics: too many points");
    const size_t n_partial = (size_t)ntiles * (T + 1) * NB * 2;
    const size_t n_keep = (size_t)T * NB + NB;
    Workspace ws = Workspace::pooled(stream);
    double* work;
    if (!ws.alloc(work, n_partial + n_keep)) return fail(SHG_ERR_NOMEM, "shg_basin_statistics: workspace allocation failed");
    double* partial = work;
    double* keep = work + n_partial;
    const unsigned red_blocks = (unsigned)((T * NB + 3) / 4);
    hipLaunchKernelGGL((stats_kernel<NB, 1>), dim3((unsigned)ntiles, (unsigned)((T + 1 + kStatRows - 1) / kStatRows)), dim3(256), 0, stream, V, T,
                       P, w, bits, tile, (const double*)nullptr, partial);
    hipLaunchKernelGGL((stats_reduce_kernel<NB, 1>), dim3(red_blocks), dim3(256), 0, stream, T, B, (int)ntiles, (const double*)partial, keep, out);
    hipLaunchKernelGGL((stats_kernel<NB, 2>), dim3((unsigned)ntiles, (unsigned)((T + kStatRows - 1) / kStatRows)), dim3(256), 0, stream, V, T, P,
                       w, bits, tile, (const double*)keep, partial);
    hipLaunchKernelGGL((stats_reduce_kernel<NB, 2>), dim3(red_blocks), dim3(256), 0, stream, T, B, (int)ntiles, (const double*)partial, keep, out);
    SHG_HIP(hipGetLastError());
    return SHG_OK;
}

int check_points(const char* fn, int nlat, const double* lat_tab, int nlon, const double* lon_tab, const double* xyz, long long npts) {
    SHG_REQUIRE(npts >= 0 && nlat >= 0 && nlon >= 0, "%s: negative size", fn);
    if (xyz == nullptr) {
        SHG_REQUIRE(lat_tab != nullptr && lon_tab != nullptr, "%s: NULL pointer (no point list and no grid tables)", fn);
        SHG_REQUIRE(npts == (long long)nlat * nlon, "%s: %lld points where the grid has %d x %d", fn, npts, nlat, nlon);
    }
    return SHG_OK;
}

}  // namespace shg

using namespace shg;

extern "C" int shg_basin_pip(int nlat, const double* lat_tab, int nlon, const double* lon_tab, const double* xyz, long long npts, const double* frame_h,
                             int nedges, const double* edges, int first, unsigned long long* work, unsigned char* mask, void* stream_) {
    if (int st = check_points("shg_basin_pip", nlat, lat_tab, nlon, lon_tab, xyz, npts)) return st;
    SHG_REQUIRE(nedges >= 0, "shg_basin_pip: negative size");
    SHG_REQUIRE(frame_h != nullptr && work != nullptr && mask != nullptr && (edges != nullptr || nedges == 0), "shg_basin_pip: NULL pointer");
    if (npts == 0) return SHG_OK;
    const hipStream_t stream = (hipStream_t)stream_;
    const Points s{nlat, nlon, lat_tab, lon_tab, xyz, npts};
    const Frame f{frame_h[0], frame_h[1], frame_h[2], frame_h[3]};
    const long long blocks = (npts + 255) / 256;
    SHG_REQUIRE(blocks <= 0x7fffffff, "shg_basin_pip: %lld points exceed the launch grid", npts);
    hipLaunchKernelGGL(list_reset_kernel, dim3(1), dim3(1), 0, stream, work);
    hipLaunchKernelGGL(cap_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, s, f, first, work, mask);
    if (nedges > 0)
        hipLaunchKernelGGL(pip_kernel, dim3((unsigned)std::min(blocks, 4096LL)), dim3(256), 0, stream, s, f, nedges, edges,
                           (const unsigned long long*)work, mask);
    SHG_HIP(hipGetLastError());
    return SHG_OK;
}

extern "C" int shg_basin_buffer(int nlat, const double* lat_tab, int nlon, const double* lon_tab, const double* xyz, long long npts,
                                const double* frame_h, int nedges, const double* edges, int value, unsigned long long* work, unsigned char* mask,
                                void* stream_) {
    if (int st = check_points("shg_basin_buffer", nlat, lat_tab, nlon, lon_tab, xyz, npts)) return st;
    SHG_REQUIRE(nedges >= 0, "shg_basin_buffer: negative size");
    SHG_REQUIRE(frame_h != nullptr && work != nullptr && mask != nullptr && (edges != nullptr || nedges == 0), "shg_basin_buffer: NULL pointer");
    SHG_REQUIRE(value == 0 || value == 1, "shg_basin_buffer: value must be 0 or 1");
    if (npts == 0 || nedges == 0) return SHG_OK;
    const hipStream_t stream = (hipStream_t)stream_;
    const Points s{nlat, nlon, lat_tab, lon_tab, xyz, npts};
    const Frame f{frame_h[0], frame_h[1], frame_h[2], frame_h[3]};
    const long long blocks = (npts + 255) / 256;
    SHG_REQUIRE(blocks <= 0x7fffffff, "shg_basin_buffer: %lld points exceed the launch grid", npts);
    hipLaunchKernelGGL(list_reset_kernel, dim3(1), dim3(1), 0, stream, work);
    hipLaunchKernelGGL(cap_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, s, f, 0, work, mask);
    hipLaunchKernelGGL(pib_kernel, dim3((unsigned)std::min(blocks, 4096LL)), dim3(256), 0, stream, s, frame_h[4], nedges, edges,
                       (const unsigned long long*)work, (unsigned char)value, mask);
    SHG_HIP(hipGetLastError());
    return SHG_OK;
}

extern "C" int shg_winding_number(int nedges, const double* edges, const double* x, const double* y, long long npts, unsigned char* mask,
                                  void* stream_) {
    SHG_REQUIRE(nedges >= 0 && npts >= 0, "shg_winding_number: negative size");
    SHG_REQUIRE((edges != nullptr || nedges == 0) && ((x != nullptr && y != nullptr && mask != nullptr) || npts == 0),
                "shg_winding_number: NULL pointer");
    if (npts == 0) return SHG_OK;
    const long long blocks = (npts + 255) / 256;
    SHG_REQUIRE(blocks <= 0x7fffffff, "shg_winding_number: %lld points exceed the launch grid", npts);
    hipLaunchKernelGGL(winding_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream_, nedges, edges, x, y, npts, mask);
    SHG_HIP(hipGetLastError());
    return SHG_OK;
}

extern "C" int shg_mask_pack(const unsigned char* masks, int B, long long P, unsigned long long* bits, void* stream_) {
    SHG_REQUIRE(B >= 0 && P >= 0, "shg_mask_pack: negative size");
    SHG_REQUIRE(B <= 64, "shg_mask_pack: %d masks, at most 64 are supported", B);
    SHG_REQUIRE(bits != nullptr && (masks != nullptr || B == 0), "shg_mask_pack: NULL pointer");
    if (P == 0) return SHG_OK;
    const long long blocks = (P + 255) / 256;
    SHG_REQUIRE(blocks <= 0x7fffffff, "shg_mask_pack: %lld points exceed the launch grid", P);
    hipLaunchKernelGGL(mask_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream_, masks, B, P, bits);
    SHG_HIP(hipGetLastError());
    return SHG_OK;
}

extern "C" int shg_basin_statistics(const double* values, int T, long long P, const double* w, const unsigned long long* bits, int B, double* out,
                                    void* stream_) {
    SHG_REQUIRE(T >= 0 && P >= 0 && B >= 0, "shg_basin_statistics: negative size");
    SHG_REQUIRE(B >= 1 && B <= 64, "shg_basin_statistics: %d masks, 1 to 64 are supported", B);
    SHG_REQUIRE(values != nullptr && w != nullptr && bits != nullptr && out != nullptr, "shg_basin_statistics: NULL pointer");
    if (T == 0) return SHG_OK;
    SHG_REQUIRE(P > 0, "shg_basin_statistics: no points");
    SHG_REQUIRE((long long)T * 64 <= 0x7fffffff, "shg_basin_statistics: too many epochs");
    const hipStream_t stream = (hipStream_t)stream_;
    if (B == 1) return basin_statistics<1>(values, T, P, w, bits, B, out, stream);
    if (B <= 4) return basin_statistics<4>(values, T, P, w, bits, B, out, stream);
    if (B <= 16) return basin_statistics<16>(values, T, P, w, bits, B, out, stream);
    return basin_statistics<64>(values, T, P, w, bits, B, out, stream);
}

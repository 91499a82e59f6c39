// One-sided Jacobi (Hestenes) singular value decomposition of small matrices in LDS (shg_jacobi_svd; no
// reference counterpart: the reference calls LAPACK).  G [r][c] <- G V with V the product of the plane rotations that make the
// columns of G orthogonal: the final G is U diag(sigma), the column norms are the singular values, V the right singular vectors.
//   One workgroup per matrix, up to 16 waves.  G stays in LDS for the whole call, column-contiguous with an odd column stride
//   ld = r | 1: the lanes of a wave read consecutive doubles of one column (ds_read_b64 over consecutive addresses: no conflict
//   whatever the stride), and the transposing copies from and to the row-major matrix in memory step by ld doubles from lane to
//   lane, which an odd ld spreads over all banks (16 lanes of a ds_write_b64 group: 2 ld k mod 32, k < 16, are distinct).
//   128 x 129 doubles are 129 KiB of the CU's 160; V [c][c | 1] sits behind G where both fit (c (r | 1) + c (c | 1) doubles within
//   kJacobiLds, e.g. up to 90 x 90 and any 128 x c with c <= 31).  Otherwise V lives in a workspace in memory, one column of V per
//   contiguous row, and goes through the LDS (free by then) on its way to the caller's row-major V.
//   A sweep is the round-robin tournament over m = c rounded up to even players: m - 1 stages of m / 2 disjoint pairs, stage s pairs
//   (m - 1, s) and ((s + k) mod (m - 1), (s - k) mod (m - 1)), k = 1 .. m / 2 - 1; with odd c the player m - 1 = c does not exist and
//   its partner idles.  A wave takes four pairs at a time, k = wave + u waves: the twelve dot products are summed together
//   (wave_sum16) and end in the quad of lanes u, which works out the rotation of pair u -- the fp64 square roots and divisions,
//   some 250 instructions per rotation and the bulk of a stage when every lane repeats them for one pair, are paid once per four
//   pairs.  A workgroup barrier ends every stage.  The order of the pairs and the trees of the sums are fixed: two calls on one input
//   give the same bits.
//   Pair (p, q), p < q: a = g_p.g_p, b = g_q.g_q, d = g_p.g_q; rotate when |d| > sqrt(r) 2^-53 sqrt(a) sqrt(b) (LAPACK dgesvj) with
//   z = (b - a) / (2 d), t = sign(z) / (|z| + sqrt(1 + z^2)), cs = 1 / sqrt(1 + t^2), sn = cs t:
//   g_p <- cs g_p - sn g_q, g_q <- sn g_p + cs g_q, and the same for the columns of V.  A sweep without a rotation ends the call.
//   A NaN or an infinity in G makes no rotation fire (the test is false for NaN, and the load notes non-finite entries): one sweep.
#include "common.h"

namespace shg {
namespace {

constexpr int kJacobiMax = 128;                        // largest r and c (include/shg.h)
constexpr size_t kJacobiLds = 160 * 1024 - 64;         // dynamic LDS the kernel may ask for; the rest holds its two flags

constexpr int kPairs = 4;                              // pairs a wave works on at once (wave_sum16: one quad of lanes per pair)

// x of another lane of the row of 16 lanes (DPP control `ctrl`)
template <int ctrl>
__device__ __forceinline__ double row_move(double x) {
    const long long bits = __builtin_bit_cast(long long, x);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)bits, ctrl, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(bits >> 32), ctrl, 0xF, 0xF, true);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}

__device__ __forceinline__ double lane_value(double x, int lane) {
    const long long bits = __builtin_bit_cast(long long, x);
    const int lo = __builtin_amdgcn_readlane((int)bits, lane), hi = __builtin_amdgcn_readlane((int)(bits >> 32), lane);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}

// Sum over the 64 lanes, the same bits in every lane: four exchanges inside the rows of 16 lanes, each between two lanes that
// both form x + x' (neighbours, pairs of a quad, the quads of a half row mirrored, the half rows mirrored), then the four row
// sums as (row 0 + row 1) + (row 2 + row 3).  All lanes must be active.
__device__ __forceinline__ double wave_sum(double x) {
    x += row_move<0xB1>(x);                            // quad_perm [1, 0, 3, 2]
    x += row_move<0x4E>(x);                            // quad_perm [2, 3, 0, 1]
    x += row_move<0x141>(x);                           // row_half_mirror
    x += row_move<0x140>(x);                           // row_mirror
    return (lane_value(x, 0) + lane_value(x, 16)) + (lane_value(x, 32) + lane_value(x, 48));
}

// Sixteen sums over the 64 lanes at once: lane l ends with the sum of v[4 ((l >> 2) & 3) + (l & 3)] (every row of 16 lanes holds
// all sixteen).  Each exchange halves the values a lane carries: the lanes whose bit is clear keep the even ones and pass the odd
// ones to their partner, which does the opposite, so 8 + 4 + 2 + 1 exchanges, then two over the rows, stand for 16 x 6.  Partner
// lanes form the same sums x + x' in every exchange, and the tree is fixed.  All lanes must be active.
__device__ __forceinline__ double wave_sum16(const double (&v)[4 * kPairs], int lane) {
    static_assert(kPairs == 4, "wave_sum16 sums four values for each of four pairs");
    const bool b0 = lane & 1, b1 = lane & 2, b2 = lane & 4, b3 = lane & 8;
    double w8[8], w4[4], w2[2];
#pragma unroll
    for (int i = 0; i < 8; ++i) w8[i] = (b0 ? v[2 * i + 1] : v[2 * i]) + row_move<0xB1>(b0 ? v[2 * i] : v[2 * i + 1]);         // lane ^ 1
#pragma unroll
    for (int i = 0; i < 4; ++i) w4[i] = (b1 ? w8[2 * i + 1] : w8[2 * i]) + row_move<0x4E>(b1 ? w8[2 * i] : w8[2 * i + 1]);   // lane ^ 2
#pragma unroll
    for (int i = 0; i < 2; ++i) w2[i] = (b2 ? w4[2 * i + 1] : w4[2 * i]) + __shfl_xor(b2 ? w4[2 * i] : w4[2 * i + 1], 4);
    double t = (b3 ? w2[1] : w2[0]) + __shfl_xor(b3 ? w2[0] : w2[1], 8);
    t += __shfl_xor(t, 16);
    t += __shfl_xor(t, 32);
    return t;
}

template <bool VLDS>
__global__ __launch_bounds__(1024) void jacobi_kernel(double* G, int ldg, long long strideG, double* V, int ldv, long long strideV, double* sigma,
                                                      double* W, int r, int c, int max_sweeps, int* sweeps) {
    extern __shared__ double lds[];                    // G [c][r | 1], then V [c][c | 1] (VLDS)
    __shared__ int flags[2];                           // [0] a rotation fired in this sweep, [1] the input holds a NaN or an infinity
    const int tid = threadIdx.x, nt = blockDim.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nw = nt >> 6;
    const int ldr = r | 1, ldc = c | 1;
    double* Gl = lds;
    double* Vl = VLDS ? lds + c * ldr : W + (long long)blockIdx.x * c * c;      // column j of V: Vl + j ldv_
    const int ldv_ = VLDS ? ldc : c;
    G += (long long)blockIdx.x * strideG;
    V += (long long)blockIdx.x * strideV;
    sigma += (long long)blockIdx.x * c;

    if (tid == 0) flags[0] = flags[1] = 0;
    __syncthreads();
    bool bad = false;
    for (int idx = tid; idx < r * c; idx += nt) {
        const int i = idx / c, j = idx - i * c;
        const double x = G[(long long)i * ldg + j];
        Gl[j * ldr + i] = x;
        bad |= !__builtin_isfinite(x);
    }
    if (bad) atomicOr(&flags[1], 1);
    for (int idx = tid; idx < c * c; idx += nt) {
        const int j = idx / c, i = idx - j * c;
        Vl[j * ldv_ + i] = i == j ? 1.0 : 0.0;
    }
    __syncthreads();

    const int m = (c + 1) & ~1, pairs = m >> 1;
    const double tol = sqrt((double)r) * 0x1p-53;
    int used = (c < 2 || flags[1]) ? 1 : -1;           // nothing to rotate: one (empty) sweep
    if (used < 0) {
        for (int sweep = 1; sweep <= max_sweeps; ++sweep) {
            for (int s = 0; s < m - 1; ++s) {
                for (int k0 = wave; k0 < pairs; k0 += nw * kPairs) {
                    // kPairs pairs of the wave side by side (disjoint columns): all loads, then all sums, then all rotations
                    int p[kPairs], q[kPairs];
                    bool live[kPairs], fire[kPairs];
                    double x0[kPairs], x1[kPairs], y0[kPairs], y1[kPairs], cs[kPairs], sn[kPairs];
#pragma unroll
                    for (int u = 0; u < kPairs; ++u) {
                        const int k = k0 + u * nw;
                        int pp = k == 0 ? m - 1 : (s + k) % (m - 1);
                        int qq = k == 0 ? s : (s - k + 2 * (m - 1)) % (m - 1);
                        if (pp > qq) { const int t = pp; pp = qq; qq = t; }
                        live[u] = k < pairs && qq < c;              // odd c: the partner of the player that does not exist idles
                        p[u] = live[u] ? pp : 0;
                        q[u] = live[u] ? qq : 0;
                        const double* gp = Gl + p[u] * ldr;
                        const double* gq = Gl + q[u] * ldr;
                        x0[u] = lane < r ? gp[lane] : 0.0, x1[u] = lane + 64 < r ? gp[lane + 64] : 0.0;
                        y0[u] = lane < r ? gq[lane] : 0.0, y1[u] = lane + 64 < r ? gq[lane + 64] : 0.0;
                    }
                    double part[4 * kPairs];
#pragma unroll
                    for (int u = 0; u < kPairs; ++u) {
                        part[4 * u] = x0[u] * x0[u] + x1[u] * x1[u];
                        part[4 * u + 1] = y0[u] * y0[u] + y1[u] * y1[u];
                        part[4 * u + 2] = x0[u] * y0[u] + x1[u] * y1[u];
                        part[4 * u + 3] = 0.0;
                    }
                    // lane 4 u + j of every row: a, b, d (j = 0, 1, 2) of pair u; then all three in every lane of the quad u, which works
                    // out the rotation of its pair: the square roots and divisions of the four pairs cost those of one
                    const double sum = wave_sum16(part, lane);
                    const double a = row_move<0x00>(sum), b = row_move<0x55>(sum), d = row_move<0xAA>(sum);      // quad_perm [j, j, j, j]
                    const bool rotate = fabs(d) > tol * (sqrt(a) * sqrt(b));
                    const double z = (b - a) / (2.0 * d);
                    const double t = copysign(1.0, z) / (fabs(z) + sqrt(1.0 + z * z));
                    const double cs_quad = 1.0 / sqrt(1.0 + t * t), sn_quad = cs_quad * t;
                    const unsigned long long rotates = __ballot(rotate);
                    bool any = false;
#pragma unroll
                    for (int u = 0; u < kPairs; ++u) {
                        fire[u] = live[u] && ((rotates >> (4 * u)) & 1);
                        cs[u] = lane_value(cs_quad, 4 * u);
                        sn[u] = lane_value(sn_quad, 4 * u);
                        any |= fire[u];
                    }
#pragma unroll
                    for (int u = 0; u < kPairs; ++u) {
                        if (!fire[u]) continue;
                        double* gp = Gl + p[u] * ldr;
                        double* gq = Gl + q[u] * ldr;
                        if (lane < r) {
                            gp[lane] = cs[u] * x0[u] - sn[u] * y0[u];
                            gq[lane] = sn[u] * x0[u] + cs[u] * y0[u];
                        }
                        if (lane + 64 < r) {
                            gp[lane + 64] = cs[u] * x1[u] - sn[u] * y1[u];
                            gq[lane + 64] = sn[u] * x1[u] + cs[u] * y1[u];
                        }
                    }
                    // the columns of V: the loads of all rotations before the first store (in memory they take a microsecond)
#pragma unroll
                    for (int u = 0; u < kPairs; ++u) {
                        const double* vp = Vl + p[u] * ldv_;
                        const double* vq = Vl + q[u] * ldv_;
                        x0[u] = fire[u] && lane < c ? vp[lane] : 0.0, x1[u] = fire[u] && lane + 64 < c ? vp[lane + 64] : 0.0;
                        y0[u] = fire[u] && lane < c ? vq[lane] : 0.0, y1[u] = fire[u] && lane + 64 < c ? vq[lane + 64] : 0.0;
                    }
#pragma unroll
                    for (int u = 0; u < kPairs; ++u) {
                        if (!fire[u]) continue;
                        double* vp = Vl + p[u] * ldv_;
                        double* vq = Vl + q[u] * ldv_;
                        if (lane < c) {
                            vp[lane] = cs[u] * x0[u] - sn[u] * y0[u];
                            vq[lane] = sn[u] * x0[u] + cs[u] * y0[u];
                        }
                        if (lane + 64 < c) {
                            vp[lane + 64] = cs[u] * x1[u] - sn[u] * y1[u];
                            vq[lane + 64] = sn[u] * x1[u] + cs[u] * y1[u];
                        }
                    }
                    if (any && lane == 0) atomicOr(&flags[0], 1);
                }
                __syncthreads();                       // orders the LDS columns and the rows of the V workspace in memory alike
            }
            const int any = flags[0];
            __syncthreads();
            if (tid == 0) flags[0] = 0;
            __syncthreads();
            if (!any) {
                used = sweep;
                break;
            }
        }
    }

    for (int j = wave; j < c; j += nw) {
        const double* g = Gl + j * ldr;
        const double x0 = lane < r ? g[lane] : 0.0, x1 = lane + 64 < r ? g[lane + 64] : 0.0;
        const double a = wave_sum(x0 * x0 + x1 * x1);
        if (lane == 0) sigma[j] = sqrt(a);
    }
    for (int idx = tid; idx < r * c; idx += nt) {
        const int i = idx / c, j = idx - i * c;
        G[(long long)i * ldg + j] = Gl[j * ldr + i];
    }
    const double* Vt = Vl;
    int ldt = ldv_;
    if (!VLDS) {                                       // the workspace holds V transposed: through the LDS, which G has left
        __syncthreads();
        for (int idx = tid; idx < c * c; idx += nt) {
            const int j = idx / c, i = idx - j * c;
            lds[j * ldc + i] = Vl[j * c + i];
        }
        __syncthreads();
        Vt = lds;
        ldt = ldc;
    }
    for (int idx = tid; idx < c * c; idx += nt) {
        const int i = idx / c, j = idx - i * c;
        V[(long long)i * ldv + j] = Vt[j * ldt + i];
    }
    if (tid == 0) sweeps[blockIdx.x] = used;
}

}  // namespace
}  // namespace shg

using namespace shg;

extern "C" int shg_jacobi_svd(double* G, int ldg, long strideG, double* V, int ldv, long strideV, double* sigma, int r, int c, int batch,
                              int max_sweeps, int* sweeps, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    SHG_REQUIRE(r >= 1 && r <= kJacobiMax && c >= 1 && c <= kJacobiMax, "shg_jacobi_svd: r %d, c %d outside 1 .. %d", r, c, kJacobiMax);
    SHG_REQUIRE(batch >= 1, "shg_jacobi_svd: batch %d below 1", batch);
    SHG_REQUIRE(max_sweeps >= 1, "shg_jacobi_svd: max_sweeps %d below 1", max_sweeps);
    SHG_REQUIRE(ldg >= c && ldv >= c, "shg_jacobi_svd: ldg %d or ldv %d below the %d columns", ldg, ldv, c);
    SHG_REQUIRE(batch == 1 || (strideG >= (long)(r - 1) * ldg + c && strideV >= (long)(c - 1) * ldv + c),
                "shg_jacobi_svd: strideG %ld or strideV %ld below the extent of one matrix", strideG, strideV);
    SHG_REQUIRE(G != nullptr && V != nullptr && sigma != nullptr && sweeps != nullptr, "shg_jacobi_svd: NULL pointer");
    const int ldr = r | 1, ldc = c | 1;
    const size_t both = (size_t)(c * ldr + c * ldc) * sizeof(double);
    const bool v_lds = both <= kJacobiLds;
    const size_t lds_bytes = v_lds ? both : (size_t)c * std::max(ldr, ldc) * sizeof(double);
    const int waves = std::min(16, std::max(1, ceil_div((c + 1) / 2, kPairs)));      // kPairs pairs of a stage per wave
    if (v_lds) {
        SHG_SET_LDS_ONCE(jacobi_kernel<true>, kJacobiLds);
        hipLaunchKernelGGL(jacobi_kernel<true>, dim3((unsigned)batch), dim3(64 * waves), lds_bytes, stream, G, ldg, (long long)strideG, V, ldv,
                           (long long)strideV, sigma, (double*)nullptr, r, c, max_sweeps, sweeps);
        SHG_HIP(hipGetLastError());
        return SHG_OK;
    }
    Workspace ws = Workspace::pooled(stream);
    double* W;
    if (!ws.alloc(W, (size_t)batch * c * c)) return fail(SHG_ERR_NOMEM, "shg_jacobi_svd: workspace of %d x %d x %d doubles", batch, c, c);
    SHG_SET_LDS_ONCE(jacobi_kernel<false>, kJacobiLds);
    hipLaunchKernelGGL(jacobi_kernel<false>, dim3((unsigned)batch), dim3(64 * waves), lds_bytes, stream, G, ldg, (long long)strideG, V, ldv,
                       (long long)strideV, sigma, W, r, c, max_sweeps, sweeps);
    SHG_HIP(hipGetLastError());
    return SHG_OK;
}

/*
 * shg.h -- C ABI of libshg: spherical-harmonic synthesis / analysis / covariance propagation / filter
 *          kernels for AMD MI355X (gfx950, CDNA4).
 *
 * This is the drop-in boundary for the hot path of akvas/grates.  The reference is
 * pure Python and has no FFI of its own; every entry point below names the reference function whose inner
 * loop it replaces (paths relative to the reference checkout).  INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns 0 on success or a negative shg_status; shg_last_error() gives the message of
 *     the last failure on the calling thread.  No exception crosses the boundary.
 *   - pointers named *_h are HOST pointers (read during the call, not retained); all other array
 *     pointers are DEVICE pointers to contiguous fp64 / int arrays owned by the caller
 *     (e.g. torch.Tensor.data_ptr()).
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls are asynchronous with
 *     respect to the host; a plan may have only one operation in flight at a time (it owns workspace).
 *   - coefficient arrays use the reference packing  anm[n][m] = C_nm (m <= n),  anm[m-1][n] = S_nm (m >= 1)
 *     (grates/gravityfield.py:156-159); "degree-wise" vectors use  index(C,n,0) = n^2 - nmin^2,
 *     index(C,n,m) = n^2 + 2m - 1 - nmin^2,  index(S,n,m) = n^2 + 2m - nmin^2  (grates/utilities.py:331-343).
 *   - grids are [nlat][nlon] row-major, parallels north to south (grates/grid.py:609-625, 1146-1151).
 */
#ifndef SHG_H
#define SHG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct shg_plan shg_plan;

typedef enum {
    SHG_OK = 0,
    SHG_ERR_INVALID = -1,   /* bad argument (NULL pointer, negative size, degree mismatch ...) */
    SHG_ERR_HIP = -2,       /* a HIP runtime call failed                                        */
    SHG_ERR_NOMEM = -3,     /* workspace allocation failed                                      */
    SHG_ERR_UNSUPPORTED = -4
} shg_status;

/* ------------------------------------------------------------------------------------------------
 * Plan: per-(degree, parallels, kernel table, meridians) tables held on the device.
 *   replaces the per-call table rebuild of PotentialCoefficients.to_grid
 *   (grates/gravityfield.py:353-365: colatitude/radius -> kn, legendre_functions, trigonometric_functions).
 *
 *   N        maximum degree
 *   colat_h  [nlat] geocentric colatitude of every parallel                  (grates/utilities.py:438-459)
 *   kn_h     [nlat][N+1] per-parallel degree factors (1/k_n)(R/r)^(n+1) GM/R  (grates/gravityfield.py:356)
 *   lon_h    [nlon] longitude of every meridian
 * ------------------------------------------------------------------------------------------------ */
int shg_plan_create(shg_plan** out, int N, int nlat, const double* colat_h, const double* kn_h,
                    int nlon, const double* lon_h, int device);
int shg_plan_destroy(shg_plan* plan);

/* Number of epochs processed per internal pass (workspace is sized for it).  Default 16. */
int shg_plan_set_chunk(shg_plan* plan, int epochs_per_pass);

/* Synthesis path: 0 = automatic, 1 = three-kernel path (pack, Legendre stage, longitude stage; any grid, any degree),
 * 2 = single fused kernel (4-fold symmetric meridians, degree <= 126), 5 = fused kernel with 32-row panels (both symmetries,
 * degree <= ~210; chosen automatically above degree 126), 6 = single fused kernel for equi-angular cell-centred meridians that
 * folds the longitude stage over 10, 9, 6 or 3 rotations (the first of these for which nlon is a multiple of 2 R and nlon / R a
 * multiple of 16, see shg_plan_set_rotations) and the reflection of the meridian set (degree <= ~110; the automatic choice where
 * it applies).  Kernels 2 and 6 use the north-south symmetry of the
 * parallels when the grid has it and their plain variant otherwise; the variant is not a choice of the caller. */
int shg_plan_set_path(shg_plan* plan, int path);

/* Kernel 6 only: at most `limit` workgroups run their Legendre stage (in which they do not store) at the same time, kept per XCD by
 * ticket queues; limit < 0 = that many sixteenths of the device's CUs, 0 = no limit.  A plan on which this was never called runs with
 * the ticket limit of DESIGN.md 4.1: grids of more than one workgroup per CU are limited to 4/16 of the CUs x (Qtot / nlon) / (345 / 1440)
 * (4/16 on the d/o-96 / 0.25 degree plan: -4.2 % of its step on MI355X), no limit where that reaches the whole device.  Any call, 0
 * included, replaces that default for good.  Waits for the device whenever a limit > 0 is set (the queues are zeroed). */
int shg_plan_set_stage_limit(shg_plan* plan, int limit);

/* Rotation count R of kernel 6: the longitude sums are evaluated on nlon / (2 R) columns and the 2 R images of every column are
 * formed in registers.  0 = the plan's own choice (the default: 10 where nlon / 10 is a multiple of 16 -- the 0.25 degree grid --,
 * else 9 -- the 0.5 degree grid --, else 6, else 3), or one of 3, 6, 9, 10; the meridians must be equi-angular and cell-centred with nlon a multiple of 2 R and
 * nlon / R a multiple of 16, and the panel of that count must fit the LDS.  Waits for the device (the tables are rebuilt).
 * shg_plan_info reports the count in use in bits 8.. of which[7]. */
int shg_plan_set_rotations(shg_plan* plan, int R);

/* Kernel 6 only: order pruning.  P_nm(theta) ~ sin^m theta, so a block of parallels next to a pole keeps the orders 0 .. level only,
 * where no higher order has a term |kn P_nm| above 1e-30 of the largest term of any parallel of the block (levels end at 9, 19, ...
 * and at N; they depend on the colatitudes, kn and N, not on the coefficients).  enable = 1 (the default; the grids measured bit-identical and the
 * d/o-96 / 0.25 degree kernel 3.6 % faster on MI355X) or 0: every block keeps all orders, the launch of the kernel
 * without pruning (for comparisons).  shg_plan_order_cutoffs reports the level of every latitude block of kernel 6 (8 northern parallels and
 * their mirror images, or 16 parallels without the north-south symmetry; *nblocks = 0 where kernel 6 does not apply) and whether
 * they are in use.  shg_rot_order_cutoffs works the same levels out from host tables alone, and shg_rot_level_tables builds the
 * tables of one level (header: 24 ints -- k-steps, panel slots, item records per wave, trips, trig pieces, item records, 0, 0,
 * k-steps of the 6 classes, orders of the 6 classes; trig stream [pieces][64][2]; work items [records][4]): neither needs a device. */
int shg_plan_set_order_pruning(shg_plan* plan, int enable);
int shg_plan_order_cutoffs(const shg_plan* plan, int* levels, int capacity, int* nblocks, int* enabled);
int shg_rot_order_cutoffs(int N, int nlat, const double* colat_h, const double* kn_h, int* levels, int capacity, int* nblocks);
int shg_rot_level_tables(int R, int N, int level, int ns, int nlon, const double* lon_h, int32_t header[24], double* trig,
                         int64_t trig_capacity, int32_t* items, int64_t items_capacity);

/* Kernel 6 only: the half column tile.  Where the fundamental domain has nd = nlon / (2 R) = 8 mod 16 columns (R = 10 and 6 on the 0.25
 * degree grid, R = 9 on the 0.5 degree grid) the last column tile of 16 has 8 columns.  enable = 1 (the default): that tile runs on the
 * 16 real columns nd - 8 .. nd + 7 and forms and stores its R ascending images only -- the descending image k + 1 of column c is the
 * ascending image k of column 2 nd - 1 - c --, half the butterfly and half the stores of that tile, each store a whole 16-column
 * piece.  enable = 0: that tile forms all 2 R images like every other and the hardware drops the 8 columns beyond nd (for
 * comparisons).  The plan's own device copy of the trig stream carries cos / sin of m (2 pi / R - mu_(2 nd - 1 - c)) in the lanes 8 .. 15
 * of that tile's pieces either way; shg_rot_level_tables returns zeros there.  The grids of the two settings differ in the 8 R columns
 * of the former descending images only, by rounding, and the d/o-96 / 0.25 degree kernel measured 1.9 % faster with the fold on MI355X
 * (DESIGN.md 4.1).  No effect where nd % 16 == 0.  shg_plan_info: bit 3 of which[3]. */
int shg_plan_set_half_tile_fold(shg_plan* plan, int enable);

/* Introspection: which[0]=N, [1]=nlat, [2]=nlon, [3]=bit 0: 4-fold longitude symmetry, bit 1: parallels symmetric about the
 * equator, bit 2: the rotation-folded kernel (path 6) applies, bit 3: kernel 6 folds its half column tile (shg_plan_set_half_tile_fold is on and nd % 16 == 8),
 * [4]=epochs per pass, [5]=K slots of the longitude stage, [6]=1 if synthesis uses the fused kernel, [7]=path | rotation count of kernel 6 << 8. */
int shg_plan_info(const shg_plan* plan, int64_t which[8]);

/* Per-kernel timing with HIP events recorded on the caller's stream around every kernel a plan launches.
 * kinds: 0 pack_coefficients, 1 legendre_stage, 2 lon_stage, 3 covprop, 4 analysis_lon, 5 analysis_solve.
 * enable: 0 = off, 1 = every kind, otherwise a mask of kinds shifted by one (bit k + 1 = kind k; an event pair costs the stream ~5 us).
 * shg_plan_profile_read synchronises the recorded events, returns accumulated milliseconds and launch
 * counts per kind since the last read, and resets the accumulators. */
#define SHG_PROFILE_KINDS 8
int shg_plan_profile(shg_plan* plan, int enable);
int shg_plan_profile_read(shg_plan* plan, double ms[SHG_PROFILE_KINDS], int64_t launches[SHG_PROFILE_KINDS]);

/* ------------------------------------------------------------------------------------------------
 * Synthesis  V[b][i][j] = sum_nm kn[i][n] P_nm(theta_i) (C_nm[b] cos m lon_j + S_nm[b] sin m lon_j)
 *   replaces PotentialCoefficients.to_grid, regular-grid branch   (grates/gravityfield.py:352-368)
 *   anm  [B][N+1][N+1]      grid  [B][nlat][nlon]
 * ------------------------------------------------------------------------------------------------ */
int shg_synthesis(shg_plan* plan, const double* anm, int B, double* grid, void* stream);

/* Point-list synthesis, one thread block per block of points
 *   replaces PotentialCoefficients.to_grid, AttributeError branch  (grates/gravityfield.py:370-388)
 *   colat, lon [npts]; kn [npts][N+1]; anm [B][N+1][N+1]; values [B][npts]
 *   Any degree: fewer than 48 epochs run a recursion kernel that keeps 256 (N+1) bytes of coefficients in LDS, as long as the
 *   device grants a workgroup that much (d/o 639 on CDNA4); beyond that, and from 48 epochs on, the values are one GEMM per
 *   chunk of points with generated harmonic rows.  That path allocates its Legendre table, up to 2 GB per chunk, whatever
 *   the number of epochs: a short series beyond the LDS limit pays for it.                                */
int shg_synthesis_points(int N, const double* colat, const double* lon, const double* kn, int npts,
                         const double* anm, int B, double* values, void* stream);

/* RMS over the epochs of a batch of grids, the reduction of gridded_rms (grates/gravityfield.py:1164-1170):
 *   acc[i] = (accumulate ? acc[i] : 0) + sum_b values[b][i]^2   (epoch order, no FMA);   count > 0: acc[i] = sqrt(acc[i] / count).
 * values [B][M] (grids of a batch, flattened), acc [M].  Batches are chained with accumulate = 1, the last call passes the
 * number of epochs as count. */
int shg_epoch_rms(const double* values, int B, long long M, int accumulate, long long count, double* acc, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Parity hooks for the table functions
 *   shg_legendre          utilities.legendre_functions            (grates/utilities.py:13-59)
 *                         colat [k] -> pnm [k][N+1][N+1] (packed, sine slots mirrored)
 *   shg_legendre_order    utilities.legendre_functions_per_order   (grates/utilities.py:62-115)
 *                         colat [k] -> pm [k][N+1-m]   (uses s = sqrt(1 - t^2))
 *   shg_trigonometric     utilities.trigonometric_functions        (grates/utilities.py:249-275)
 *                         lon [k] -> cs [k][N+1][N+1]
 * ------------------------------------------------------------------------------------------------ */
int shg_legendre(int N, const double* colat, int k, double* pnm, void* stream);
int shg_legendre_order(int N, int m, const double* colat, int k, double* pm, void* stream);
int shg_trigonometric(int N, const double* lon, int k, double* cs, void* stream);

/* Operator block of one order m (RegularGrid.synthesis_matrix_per_order, grates/grid.py:627-663, and
 * IrregularGrid.synthesis_matrix_per_order, grates/grid.py:957-991): columns = degrees max(m, nmin) .. N,
 *   out_cos[row][c] = kn[i][n] P_nm(colat_i) cos(m lon_j),   out_sin likewise with sin   (n = max(m, nmin) + c),
 * with P_nm from the per-order recursion (s = sqrt(1 - t^2), like shg_legendre_order).
 *   pointwise = 0: regular grid, colat / kn rows of the nlat parallels, lon of the nlon meridians, row = i * nlon + j;
 *   pointwise = 1: point list, colat / lon / kn rows of the nlat points (nlon is ignored), row = i.
 * m = 0: only out_cos is written (cos 0 = 1); out_sin may be NULL. */
int shg_synthesis_matrix_order(int N, int m, int nmin, const double* colat, int nlat, const double* lon, int nlon, const double* kn,
                               int pointwise, double* out_cos, double* out_sin, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Degree-wise ravel / unravel of batches (integer index maps applied on the device)
 *   replaces utilities.ravel_coefficients / unravel_coefficients   (grates/utilities.py:310-411)
 *   and TimeSeries.to_array                                        (grates/gravityfield.py:964-980)
 *   arr [B][Na+1][Na+1]  <->  vec [B][(nmax+1)^2 - nmin^2]; degrees > Na read as zero / are dropped.
 * ------------------------------------------------------------------------------------------------ */
int shg_ravel(const double* arr, int B, int Na, int nmin, int nmax, double* vec, void* stream);
int shg_unravel(const double* vec, int B, int nmin, int nmax, double* arr /* [B][nmax+1][nmax+1], zero-filled */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Covariance propagation  sigma[i*nlon + j] = sqrt(a_ij^T Sigma a_ij),  a_ij = row of the synthesis matrix
 *   replaces RegularGrid.covariance_propagation                     (grates/grid.py:817-839)
 *   cov    [P][P] degree-wise order, P = (N+1)^2 - nmin^2 (only N == plan degree is accepted)
 *   sigma  [(lat1-lat0)*nlon]  for the band of parallels lat0 <= i < lat1 (latitude-band sharding)
 *   The A rows are generated on the fly (never materialised); A*Sigma runs on v_mfma_f64_16x16x4_f64.
 * ------------------------------------------------------------------------------------------------ */
int shg_covprop_diag(shg_plan* plan, const double* cov, int nmin, int lat0, int lat1, double* sigma, void* stream);
/* The same for a symmetric Sigma of which only the upper triangle is read: half of the MFMA work
 *   sigma2 = sum_c [ sum_{p<c} 2 a_p Sigma_pc + a_c Sigma_cc ] a_c
 * (an extension; the reference multiplies with the full matrix, grates/grid.py:833).  shg_symmetry_defect writes
 * max |S[p][c] - S[c][p]| to *defect (device double): 0 means the shortcut reproduces the general result up to summation order. */
int shg_covprop_diag_symmetric(shg_plan* plan, const double* cov, int nmin, int lat0, int lat1, double* sigma, void* stream);
int shg_symmetry_defect(const double* S, int n, int ld, double* defect, void* stream);
/* A NaN on one side of the diagonal makes the defect NaN, an infinity makes it infinite or NaN: never 0.  shg_covprop_diag_symmetric loads the entries
 * below the diagonal of the 128 x 128 diagonal blocks but discards them unread: they may hold anything, NaN included. */

/* Host-only diagnostic: the kernel that shg_covprop_diag (symmetric 0) or shg_covprop_diag_symmetric (symmetric 1) runs for a band
 * of M = (lat1 - lat0) * nlon grid rows and a P x P matrix whose base address is (aligned 1) or is not (0) a multiple of 16
 * bytes.  Makes no HIP call; returns the kind, or SHG_ERR_INVALID.  The thresholds are tuning, not contract. */
typedef enum {
    SHG_COVPROP_ROUTE_NONE = 0,       /* P == 0 or an empty band: no product                                            */
    SHG_COVPROP_ROUTE_ROWS = 1,       /* row-tiled kernel: parallels padded to 128 meridians, at most 4 % of padding    */
    SHG_COVPROP_ROUTE_DIRECT = 2,     /* general kernel, Sigma tiles copied straight into LDS, 16 bytes at a time       */
    SHG_COVPROP_ROUTE_REGISTER = 3,   /* general kernel, Sigma through registers, 8 bytes at a time (odd P or base)     */
    SHG_COVPROP_ROUTE_PADDED = 4,     /* copy of Sigma with even, padded rows, then DIRECT (odd P or base, M P^2 > 1e12) */
    SHG_COVPROP_ROUTE_SYMMETRIC = 5   /* upper-triangle kernel, Sigma through registers, 8 bytes at a time              */
} shg_covprop_route_kind;
int shg_covprop_route(int nlon, int P, int aligned, long long M, int symmetric);
/* The same result through the separable structure of the synthesis matrix (an extension, see csrc/covsep.hip):
 *   sigma^2(i, j) = t(j)^T B_i t(j),  B_i[s][s'] = sum_{n,n'} PK_n,s(i) Sigma[(n,s)][(n',s')] PK_n',s'(i)
 * 2 nlat P^2 flops instead of 2 nlat nlon P^2 (d/o 180, 0.5 deg: 8e11 instead of 5.6e14); differs from shg_covprop_diag by
 * summation order only.  Workspace: about P^2 + 32 P nlat doubles (17 GB at d/o 180 for the full grid). */
int shg_covprop_diag_separable(shg_plan* plan, const double* cov, int nmin, int lat0, int lat1, double* sigma, void* stream);
/* cov symmetric (caller's promise, cf. shg_symmetry_defect): B_i is symmetric too and only its slot pairs s >= s' are formed,
 * half the work of shg_covprop_diag_separable. */
int shg_covprop_diag_separable_symmetric(shg_plan* plan, const double* cov, int nmin, int lat0, int lat1, double* sigma, void* stream);

/* Point-list variant  (grates/grid.py:1096-1120): colat, lon [npts]; kn [npts][N+1]; sigma [npts] */
int shg_covprop_points(int N, const double* colat, const double* lon, const double* kn, int npts,
                       const double* cov, int nmin, double* sigma, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Filters
 *   shg_degree_scale      Gaussian.filter / Butterworth.filter degree-wise scaling (grates/filter.py:61-72)
 *                         anm_out[b][slot of degree n] = w[n] * anm_in   for n >= nfirst, copied below
 *   shg_orderwise_filter  OrderWiseFilter.filter                      (grates/filter.py:175-191)
 *                         blocks packed back to back in the reference list order
 *                         [order0_cos, order1_cos, order1_sin, ...], block k row-major with leading
 *                         dimension block_dim[k] = Nb+1-m; block_off [2Nb+1] offsets in doubles.
 *                         Coefficients of degree N <= Nb are filtered with the leading (N+1-m)^2 sub-block;
 *                         degrees 0 and 1 are restored from the input.
 *   shg_dense_filter      GeneralMatrix.filter core  Y = W X           (grates/filter.py:473-474)
 *                         W [P][P], X [P][T] (epoch fastest), Y [P][T]; fp64 MFMA GEMM.
 * ------------------------------------------------------------------------------------------------ */
int shg_degree_scale(const double* w /* [N+1] device */, int N, int nfirst, const double* anm_in, int B,
                     double* anm_out, void* stream);
int shg_orderwise_filter(const double* blocks_packed, const int64_t* block_off, int Nb, int N,
                         const double* anm_in, int B, double* anm_out, void* stream);
int shg_dense_filter(const double* W, int P, const double* X, int T, double* Y, void* stream);
/* Which kernels shg_orderwise_filter takes for B epochs of degree N (host only, no device call): which[0] = 1 if the batch goes through
 * the order-major layout (pack, shg_orderwise_filter_om, unpack), [1] = orders per workgroup of the kernel on the reference layout
 * (8, 4 or 2; 0: the degree exceeds its LDS stage and it refuses), [2] = dynamic LDS bytes of that launch, [3] = its epochs per workgroup. */
int shg_orderwise_filter_info(int N, int B, int which[4]);

/* Order-major series: a time series of coefficient sets kept on the device between operators -- the batching the reference does with
 * TimeSeries.to_array (grates/gravityfield.py:964-980), in the layout the order-wise operators want:
 *   om [(N+1)^2 rows][Bpad]   epochs fastest (Bpad = B rounded up to a multiple of 32), row of (slot s, k = n - m) = first_row(s) + k with
 *   the slots in the order of the DDK block list (s = 0: order 0 cosine, 2m - 1: order m cosine, 2m: order m sine; grates/filter.py:153-191).
 *   shg_order_major_pack / _unpack   from / to the reference arrays anm [B][N+1][N+1]
 *   shg_orderwise_filter_om          OrderWiseFilter.filter of all epochs: Y_s = W_s X_s per slot on whole matrices (no gather / scatter);
 *                                    degrees 0 and 1 keep the input, N <= Nb as in shg_orderwise_filter
 *   shg_degree_scale_om              shg_degree_scale (Gaussian / Butterworth) of all epochs of a series
 *   shg_synthesis_om                 shg_synthesis of a series of degree Ns >= the plan's N (higher degrees are not read); fused kernels on
 *                                    parallels symmetric about the equator only (SHG_ERR_INVALID otherwise: unpack the series) */
int shg_order_major_pack(const double* anm, int N, int B, double* om, int Bpad, void* stream);
int shg_order_major_unpack(const double* om, int N, int B, int Bpad, double* anm, void* stream);
int shg_orderwise_filter_om(const double* blocks_packed, const int64_t* block_off, int Nb, int N, const double* om_in, int B, int Bpad,
                            double* om_out, void* stream);
int shg_degree_scale_om(const double* w /* [N+1] device */, int N, int nfirst, const double* om_in, int B, int Bpad, double* om_out, void* stream);
int shg_synthesis_om(shg_plan* plan, const double* om, int Ns, int B, int Bpad, double* grid, void* stream);

/* DDK block construction  W_k = (N_k + diag(w[m:]))^-1 N_k  for all 2Nb+1 order-wise normal blocks
 *   replaces the dense solves of DDK.__init__ / DDKGeneric.__init__      (grates/filter.py:252-255, 344-347)
 *   normals_packed / blocks_out / work: blocks back to back as in shg_orderwise_filter (work: scratch of the
 *   same size); weights [Nb+1] device array (w_0 = 1, w_n = scale n^4). */
int shg_ddk_blocks(const double* normals_packed, const int64_t* block_off, int Nb, const double* weights, double* work,
                   double* blocks_out, void* stream);

/* X = A^-1 B for a symmetric positive definite A [n][n], B / X [n][k] (Cholesky on the device)
 *   replaces the normal-equation solve of IrregularGrid.analysis_matrix   (grates/grid.py:1015-1017) */
int shg_spd_solve(const double* A, int n, const double* B, int k, double* X, void* stream);

/* General fp64 MFMA GEMM  C[M][N] = A[M][K] B[K][N]  (row-major, leading dimensions in elements). */
int shg_dgemm(int M, int N, int K, const double* A, int lda, const double* B, int ldb, double* C, int ldc, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Dense block operations of the block-banded normal-equation solver ("Kalman smoother", grates/lstsq.py:698-883).
 * The reference loops over the non-zero blocks of a BlockMatrix in Python and calls NumPy / SciPy LAPACK per block;
 * the replacement keeps those loops on the host and runs every block operation on the device:
 *   shg_gemm    C = alpha op(A) op(B) + beta C, row-major, transX != 0 -> operand stored transposed
 *               replaces the `@` products of blocks          (grates/lstsq.py:679, 711, 743-748, 770-774, 805, 815, 846, 860-882)
 *   shg_potrf   A = U^T U in place, upper triangle referenced, strictly lower triangle zeroed on exit; *info (device int,
 *               may be NULL) receives the 1-based index of the first non-positive pivot, 0 on success
 *               replaces scipy.linalg.cholesky(lower=False)  (grates/lstsq.py:713; numpy.linalg.cholesky lstsq.py:197)
 *   shg_trtri   X = U^-1 for an upper triangular U (X != U; strictly lower triangle of X zeroed).  Triangular solves
 *               with a factor block are GEMMs with this inverse
 *               replaces scipy.linalg.solve_triangular / inv (grates/lstsq.py:716, 807, 817, 835, 839, 856, 868)
 * ------------------------------------------------------------------------------------------------ */
int shg_gemm(int transa, int transb, int M, int N, int K, double alpha, const double* A, int lda, const double* B, int ldb,
             double beta, double* C, int ldc, void* stream);
/* In-place products of shg_gemm and shg_gemm_ex.  The output may start at the address of an operand in two forms only:
 *     C == B:  transb == 0, M == K <= 128, ldc == ldb (and strideC == strideB)    -- B <- alpha op(A) B + beta B
 *     C == A:  transa == 0, N == K <= 128, ldc == lda (and strideC == strideA)    -- A <- alpha A op(B) + beta A
 * (one workgroup then reads every entry that it overwrites).  Every other call with C == A or C == B returns SHG_ERR_INVALID
 * before any HIP call.  An operand that overlaps the output WITHOUT starting at its address gives undefined results, as in BLAS;
 * disjoint blocks of one matrix (interleaved rows, different columns) are separate arrays in this sense and are fine. */

/* shg_gemm_ex: the strided-batched, structure-aware form of shg_gemm that the block solver uses internally.
 *     C_i = alpha op(A_i) op(B_i) + beta C_i,   X_i = X + i strideX (elements),   i = 0 .. batch - 1
 *   A stride of 0 repeats an operand for every item; strideC must be positive when batch > 1 (the outputs must not overlap).
 *   flags: SHG_GEMM_A_UPPER / _A_LOWER   op(A) is upper / lower triangular (needs M == K; at most one of the two)
 *          SHG_GEMM_B_UPPER / _B_LOWER   op(B) is upper / lower triangular (needs K == N; at most one of the two)
 *              entries on the zero side of a triangular operand are not read (they may hold anything, NaN included): the
 *              call works on a zero-filled copy of the triangle in stream scratch, one extra pass over K^2 entries per item
 *          SHG_GEMM_UPPER_ONLY           only the upper triangle of C is wanted (needs M == N): output tiles that lie entirely
 *              below the diagonal are not written -- every block C[128 a .. 128 a + 127][128 b .. 128 b + 127] with a > b keeps
 *              its contents; which other entries below the diagonal are written is unspecified, those on and above it all are
 *   Leading dimensions and NULL pointers as in shg_gemm; violations return SHG_ERR_INVALID before any HIP call. */
enum {
    SHG_GEMM_A_UPPER = 1,
    SHG_GEMM_A_LOWER = 2,
    SHG_GEMM_B_UPPER = 4,
    SHG_GEMM_B_LOWER = 8,
    SHG_GEMM_UPPER_ONLY = 16
};
int shg_gemm_ex(int transa, int transb, int M, int N, int K, double alpha, const double* A, int lda, long long strideA, const double* B,
                int ldb, long long strideB, double beta, double* C, int ldc, long long strideC, int batch, int flags, void* stream);

/* Host-only diagnostic: the kernels that shg_gemm_ex (and shg_gemm: strides 0, batch 1, flags 0) would launch for these arguments.
 * Takes the arguments of shg_gemm_ex, pointers included (alignment and aliasing steer the choice), checks them like shg_gemm_ex,
 * makes no HIP call and touches no memory but `which`:
 *   which[0] route kind (below) of the product, or of its first which[4] rows
 *   which[1] split-K slices (1: not split), which[2] entries of K per slice (0: not split)
 *   which[3] 1: row-strip workgroup order
 *   which[4] tail split: > 0: rows of the first product; the remaining rows are a second product with
 *   which[7]    kind | slices << 8 | strip order << 16   (0 without a tail split)
 *   which[5] panel kernel: bit 0 the K range ends at the diagonal of a lower triangular op(A), bit 1: of an upper triangular op(B)
 *   which[6] bit 0: C is A, bit 1: C is B
 * The thresholds behind the choice are performance tuning, not contract (DESIGN.md "Routes of the dense product"). */
typedef enum {
    SHG_GEMM_ROUTE_NONE = 0,      /* empty output: nothing is launched                                       */
    SHG_GEMM_ROUTE_TALL = 1,      /* whole-width stream-K kernel for 178 .. 240 columns                      */
    SHG_GEMM_ROUTE_GEMV = 2,      /* one wave per output row, at most 8 columns                              */
    SHG_GEMM_ROUTE_PANEL = 3,     /* K <= 128 and a thin output: the whole K range in registers              */
    SHG_GEMM_ROUTE_TILE64 = 4,    /* 64 x 64 output tiles                                                    */
    SHG_GEMM_ROUTE_TILE128 = 5,   /* 128 x 128 output tiles, possibly split over K                           */
    SHG_GEMM_ROUTE_SCALE = 6      /* K == 0: C = beta C                                                      */
} shg_gemm_route_kind;
int shg_gemm_route(int transa, int transb, int M, int N, int K, double alpha, const double* A, int lda, long long strideA, const double* B,
                   int ldb, long long strideB, double beta, const double* C, int ldc, long long strideC, int batch, int flags, int64_t which[8]);
int shg_potrf(int n, double* A, int lda, int* info, void* stream);
/* Y = alpha X + beta Y on [rows][cols] blocks: _scale / _axpy of blocks and vectors (grates/lstsq.py:889-903, 1107-1117) */
int shg_axpby(int rows, int cols, double alpha, const double* X, int ldx, double beta, double* Y, int ldy, void* stream);
int shg_transpose_in_place(int n, double* A, int lda, void* stream);      /* A <- A^T, square, in its own storage */
int shg_trtri(int n, const double* U, int ldu, double* X, int ldx, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Sparse block Cholesky of the block-banded normal equations ("Kalman smoother"), one call per operation: the blocks stay in
 * HBM, the call walks them on the device (csrc/blockchol.hip).  nb block rows / columns with boundaries bounds[0..nb]; the
 * stored blocks (j >= i) in compressed row form: entries rowptr[i] .. rowptr[i+1]-1 of row i, colidx[e] ascending from the
 * diagonal, blk[e] = device address of block (i, colidx[e]) (row-major [rows_i][cols_j]);
 * inv[i] = scratch [rows_i][rows_i] holding U_ii^-1 (written by shg_block_potrf, read by the others).  inv[i] may be the
 * diagonal block itself: then U_ii^-1 is kept INSTEAD of U_ii (solve and sparse inverse need nothing else; a third less
 * memory for a long chain), and shg_block_multiply / shg_block_inverse, which read U_ii, must not be used on that factor.
 *   shg_block_potrf           N = W^T W in place, fill-in allocated by the caller       (grates/lstsq.py:698-717)
 *   shg_block_potrf_rows      the same for the block rows first <= r < last only: earlier rows count as factored, later rows are
 *                             left as the Schur complement (two half chains of a tridiagonal system on two streams)
 *   shg_block_solve           W x = b / W^T x = b for B [n][k] in place                 (grates/lstsq.py:778-821, 950-968)
 *   shg_block_sparse_inverse  (W^T W)^-1 on the pattern of W (Takahashi), in place      (grates/lstsq.py:823-846, 1026-1042)
 *   shg_block_inverse         full inverse, upper blocks, in place                      (grates/lstsq.py:848-882)
 *   shg_block_multiply        V = W B (mode 0), the reference's W^T B (1), N B for a symmetric N (2)   (grates/lstsq.py:719-776)
 * ------------------------------------------------------------------------------------------------ */
int shg_block_potrf(int nb, const int* bounds, const int* rowptr, const int* colidx, double* const* blk, double* const* inv, int* info, void* stream);
int shg_block_potrf_rows(int nb, const int* bounds, const int* rowptr, const int* colidx, double* const* blk, double* const* inv, int first, int last,
                         int* info, void* stream);
/* shg_block_potrf_rows for TWO matrices of the same structure (one table, two sets of blocks and inverses): every launch
 * serves both, info[0] and info[1] receive the two pivot flags.  The two half chains of a two-ended elimination go through the
 * device as one string of launches instead of two that the card overlaps only in part. */
int shg_block_potrf_rows_pair(int nb, const int* bounds, const int* rowptr, const int* colidx, double* const* blk0, double* const* inv0,
                              double* const* blk1, double* const* inv1, int first, int last, int* info, void* stream);
/* The factorisation of a diagonal block larger than 256 overlaps its 128-column panel steps on two more streams of the device
 * (look-ahead; the caller's stream waits for them before the call returns control of the data).  A THREAD that factors matrices
 * beside other threads turns it off for itself: the card does not overlap that many queues (csrc/blas.hip).  The first such
 * factorisation on a stream synchronises that stream once: the side streams are chosen by a timing experiment so that they do
 * not share a hardware queue with it or with each other (csrc/plan.hip); every later call only enqueues. */
int shg_block_set_lookahead(int mode);
/* mode (of the calling thread): 0 = off (recursive sweep on the caller's stream), 1 = on (the default): panel sweep with look-ahead;
 * a chain row -- a block row whose only coupling is to the next one, as in the block-tridiagonal normal equations of a smoother,
 * grates/lstsq.py:364-392 -- carries its coupling block and the next diagonal block through the sweep on the second side stream
 * WHEN that stream has a hardware queue of its own (found by the timing experiment); 2 = on, chain rows always carry them;
 * 3 = on, chain rows never do (the coupling block is formed after the sweep, by one product).  The results of the variants agree to
 * rounding (different summation orders); which one mode 1 takes on this stream is reported by
 * shg_block_lookahead_info: which[0] = mode, [1] = side streams with a hardware queue of their own (0 .. 2), [2] = 1 if chain
 * rows carry their coupling along under the current mode.  (Synchronises the stream once, like the first factorisation.) */
int shg_block_lookahead_info(void* stream, int which[4]);
int shg_block_solve(int nb, const int* bounds, const int* rowptr, const int* colidx, double* const* blk, double* const* inv, int transpose, double* B,
                    int k, int ldb, void* stream);
int shg_block_sparse_inverse(int nb, const int* bounds, const int* rowptr, const int* colidx, double* const* blk, double* const* inv, void* stream);
/* Row ranges (chains cut into segments at separator epochs, grates_amd/distributed.py): the forward sweep eliminates the rows
 * first <= r < last only and leaves the reduced right-hand side in the later rows; the backward sweep and the Takahashi recursion
 * process the rows last - 1 .. first and take the solution / the entries of the inverse of the later rows as given. */
int shg_block_solve_rows(int nb, const int* bounds, const int* rowptr, const int* colidx, double* const* blk, double* const* inv, int transpose,
                         int first, int last, double* B, int k, int ldb, void* stream);
int shg_block_sparse_inverse_rows(int nb, const int* bounds, const int* rowptr, const int* colidx, double* const* blk, double* const* inv,
                                  int first, int last, void* stream);
int shg_block_inverse(int nb, const int* bounds, const int* rowptr, const int* colidx, double* const* blk, double* const* inv, void* stream);
int shg_block_multiply(int nb, const int* bounds, const int* rowptr, const int* colidx, double* const* blk, int mode, const double* B, int k, int ldb,
                       double* V, int ldv, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Analysis (area-weighted least squares per order)
 *   replaces RegularGrid.to_potential_coefficients                    (grates/grid.py:665-696, 752-790)
 *   grid [B][nlat][nlon]; area [nlat][nlon]; anm [B][N+1][N+1] (degrees < nmin left zero)
 * The per-order operators depend on the plan, the weights and nmin only; they are cached in the plan and every call compares
 * `area` with the weights they were built for (on the device; the verdict costs one host synchronisation at the end of the call).
 * area == NULL: "the weights of the previous call" -- the cached operators are used as they are and nothing is compared or
 * waited for; an error if the plan holds no operators for this nmin.
 * ------------------------------------------------------------------------------------------------ */
int shg_analysis(shg_plan* plan, const double* grid, const double* area, int nmin, int B, double* anm, void* stream);

/* How the cached operators of a plan are applied: info[0] = 1 when the operator product uses the north-south parity split (parallels
 * that are mirror images of each other, mirror-symmetric weights: x_n = sum over the northern parallels of Hp[n][i] (g[i] +- g[mirror i]),
 * half the products), 0 for the full product, -1 when the plan holds no operators yet; info[1] = the largest entry of the operators
 * that the split drops relative to their largest entry (the split is used below 5e-12; asymmetric weights give ~1). */
int shg_analysis_info(const shg_plan* plan, double info[2]);

/* ------------------------------------------------------------------------------------------------
 * Full-matrix forms of the operators
 *   shg_synthesis_matrix  dense synthesis operator of a point list, A [npts][Pn], Pn = (N+1)^2 - nmin^2 degree-wise
 *                         columns: A[p][c] = kn[p][n] P_nm(colat_p) cos|sin(m lon_p)          (grates/grid.py:412-443)
 *                         colat, lon [npts], kn [npts][N+1] device arrays
 *   shg_analysis_matrix   dense analysis operator of a regular grid, F [Pn][nlat * nlon]: the least-squares operator of
 *                         shg_analysis written out (F v = analysis of v)                      (grates/grid.py:698-730)
 *   shg_congruence        C [n][n] = W [n][k] S [k][k] W^T: filtered covariance matrix `W @ S @ W.T` built from
 *                         SpatialFilter.matrix() (grates/filter.py:74-95, 193-222, 481-509) ahead of the covariance
 *                         propagation (grates/grid.py:792-839); two fp64 MFMA GEMMs, the second on the upper tiles only;
 *                         work [n][k] scratch
 * ------------------------------------------------------------------------------------------------ */
int shg_synthesis_matrix(int N, int nmin, const double* colat, const double* lon, const double* kn, int npts, double* A, void* stream);
int shg_analysis_matrix(shg_plan* plan, const double* area, int nmin, double* F, void* stream);
int shg_congruence(int n, int k, const double* W, int ldw, const double* S, int lds, double* C, int ldc, double* work, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Basins: point-in-polygon masks and masked statistics of grid series
 *   Points of the mask calls: a regular grid (xyz == NULL, npts = nlat * nlon, point i = parallel i / nlon, meridian i % nlon)
 *   given by lat_tab [2][nlat] = ((N + h) cos phi, ((1 - e^2) N + h) sin phi) and lon_tab [2][nlon] = (cos lambda, sin lambda),
 *   or a point list xyz [npts][3] = geodetic2cartesian(lon, lat) (grates/grid.py:1920-1950); both are normalised to unit
 *   vectors on the device.  mask [npts] bytes (0 / 1); work [npts + 1] scratch (the compacted list of the cap test).
 *   shg_basin_pip       mask ^= inside one polygon (first != 0: mask = inside), the per-point part of spherical_pip
 *                       (grates/grid.py:1751-1824).  frame_h [4] HOST = (antipode a, min_k(-v_k . a)); edges [nedges][9] =
 *                       (q = b0 x b1, b0 x q, b1 x q) for b0 = vertex k + 1, b1 = vertex k of the closed unit polygon
 *   shg_basin_buffer    mask = value where a point lies within the buffer of one polygon, the per-point part of spherical_pib
 *                       (grates/grid.py:1827-1890).  frame_h [5] HOST = (a, cos(acos(min_k(-v_k . a)) + buffer / a_e),
 *                       cos(buffer / a_e)); edges [nedges][16] = (b0, b1, n = (b0 x b1) / |b0 x b1|, b0 x b1, b1 x b0,
 *                       |b0 x b1| != 0); value 0 or 1
 *   shg_winding_number  mask = winding number != 0 (grates/grid.py:1715-1748).  edges [nedges][5] = (x0, y0, y1, x1 - x0,
 *                       y1 - y0) of the closed polygon; x, y [npts]
 *   shg_mask_pack       bits [P] = sum_b (masks[b][p] != 0) << b for masks [B][P] bytes, B <= 64
 *   shg_basin_statistics  out [3][T][B] = the area-weighted mean, rms and std of values [T][P] over the points of each mask
 *                       (Grid.mean / rms / std, grates/grid.py:174-260); w [P] weights, bits [P] from shg_mask_pack,
 *                       1 <= B <= 64.  std is the two-pass sum w (v - mean)^2; an empty mask gives NaN.  Sums over fixed
 *                       tiles, reduced in a fixed order: bitwise reproducible.
 *   shg_basin_functionals  F [B][Pn] (Pn = (N+1)^2 - nmin^2, degree-wise columns as shg_ravel orders them) with F[b] . x = the
 *                       mean over mask b, weighted by area [nlat][nlon], of the plan's synthesis of the degree-wise vector x
 *                       (degrees nmin .. N, kernel factors of the plan): sum_i kn[i][n] P_nm(theta_i) g_{b,s}[i] / S_b with the
 *                       longitude transform g of shg_analysis applied to the masks and S_b = sum of area over mask b.  bits [nlat * nlon]
 *                       from shg_mask_pack, 1 <= B <= 64; an empty mask gives a row of NaN.  Bitwise reproducible; the plan's
 *                       analysis operators are not touched.
 *   shg_basin_covariance  C [B][B] (row-major, ld B) = F S F^T for F [B][n] (ld ldf) and a symmetric S [n][n] (ld lds) of which
 *                       ONLY THE UPPER TRIANGLE is read (LAPACK 'U'; nothing below the diagonal is loaded).  1 <= B <= 64,
 *                       ldf, lds >= n.  fp64 MFMA, partial sums reduced in a fixed order: C is exactly symmetric and repeated
 *                       calls are bitwise equal.
 * ------------------------------------------------------------------------------------------------ */
int shg_basin_pip(int nlat, const double* lat_tab, int nlon, const double* lon_tab, const double* xyz, long long npts, const double* frame_h,
                  int nedges, const double* edges, int first, unsigned long long* work, unsigned char* mask, void* stream);
int shg_basin_buffer(int nlat, const double* lat_tab, int nlon, const double* lon_tab, const double* xyz, long long npts, const double* frame_h,
                     int nedges, const double* edges, int value, unsigned long long* work, unsigned char* mask, void* stream);
int shg_winding_number(int nedges, const double* edges, const double* x, const double* y, long long npts, unsigned char* mask, void* stream);
int shg_mask_pack(const unsigned char* masks, int B, long long P, unsigned long long* bits, void* stream);
int shg_basin_statistics(const double* values, int T, long long P, const double* w, const unsigned long long* bits, int B, double* out,
                         void* stream);
int shg_basin_functionals(shg_plan* plan, const unsigned long long* bits, int B, const double* area, int nmin, double* F, void* stream);
int shg_basin_covariance(int B, int n, const double* F, int ldf, const double* S, int lds, double* C, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Gravitational acceleration at points (PotentialCoefficients.gravitational_acceleration, grates/gravityfield.py:423-481)
 *   g [B][M][3] (m/s^2) of the fields anm [B][N+1][N+1] (one GM and R for all) at the Cartesian positions xyz:
 *     layout SHG_POINTS_SHARED     xyz [M][3], the same points for every field
 *     layout SHG_POINTS_PER_EPOCH  xyz [B][M][3], points of their own for every field
 *   Regrouped by the Legendre function (n', k) of degree n' <= N + 1, each component is a point synthesis of degree N + 1: one
 *   column recursion per point and (n', k) serves the three components of all epochs of a pass.  No atomics: a field's result does
 *   not depend on the other fields of the call or on the layout, and repeated calls are bitwise equal.  Points at the poles and
 *   below R are fine; r = 0 is not.
 *   shg_acceleration_points_om  the same from an order-major series om [(N+1)^2][Bpad] (shg_order_major_pack), Bpad >= B.
 *   Arguments are checked before the first HIP call.
 * ------------------------------------------------------------------------------------------------ */
enum { SHG_POINTS_SHARED = 0, SHG_POINTS_PER_EPOCH = 1 };
int shg_acceleration_points(int N, const double* xyz, int M, int layout, const double* anm, int B, double GM, double R, double* g,
                            void* stream);
int shg_acceleration_points_om(int N, const double* xyz, int M, int layout, const double* om, int B, int Bpad, double GM, double R,
                               double* g, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Gravitational gradient tensor at points (the Jacobian of shg_acceleration_points; no reference counterpart)
 *   T [B][M][3][3] (s^-2; 1 E = 1e-9 s^-2), T[b][m][c][d] = d g_c / d x_d = d^2 V / dx_c dx_d, of the fields anm [B][N+1][N+1]
 *   (one GM and R for all) at the Cartesian positions xyz, in their Earth-fixed frame:
 *     layout SHG_POINTS_SHARED     xyz [M][3], the same points for every field
 *     layout SHG_POINTS_PER_EPOCH  xyz [B][M][3], points of their own for every field
 *   Each component is a point synthesis of degree N + 2 whose coefficients are the acceleration's first-derivative map applied
 *   twice: one column recursion per point and (n'', k) serves the six components of all epochs of a pass.  Each off-diagonal value is
 *   computed once and stored twice (T[..][c][d] == T[..][d][c] bitwise); xx, yy and zz are computed independently.  No atomics: a
 *   field's result does not depend on the other fields of the call or on the layout, and repeated calls are bitwise equal.  Points at
 *   the poles and below R are fine; r = 0 is not.
 *   shg_gravitational_gradients_points_om  the same from an order-major series om [(N+1)^2][Bpad] (shg_order_major_pack), Bpad >= B.
 *   Arguments are checked before the first HIP call (the rules of shg_acceleration_points, and N small enough that one pass of the
 *   combined coefficients, 48 (N+3)(N+4)/2 values, is indexable by int); nothing to do (M = 0 or B = 0) returns 0 at once.
 * ------------------------------------------------------------------------------------------------ */
int shg_gravitational_gradients_points(int N, const double* xyz, int M, int layout, const double* anm, int B, double GM, double R,
                                       double* T, void* stream);
int shg_gravitational_gradients_points_om(int N, const double* xyz, int M, int layout, const double* om, int B, int Bpad, double GM,
                                          double R, double* T, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Design matrix of the gravitational acceleration at points (the partial derivatives of shg_acceleration_points with respect to
 * the coefficients; no reference counterpart)
 *   At [P][3][ldt], transposed: row p is coefficient p of utilities.ravel_coefficients(., min_degree, N) (C_n0, C_n1, S_n1, C_n2, ...
 *   for n = min_degree .. N; P = (N+1)^2 - min_degree^2, the column order of shg_synthesis_matrix), then the component x, y, z, then
 *   the M points xyz [M][3] innermost (ldt >= M; the entries from M to ldt of a row are not touched).  For a field without
 *   coefficients below min_degree, sum_p At[p][c][i] x_p = g[i][c] of shg_acceleration_points.
 *   Every entry is one or two products of a solid harmonic of degree n + 1 with a constant: a first kernel writes the solid harmonics
 *   of degree N + 1 of a pass of points to a workspace (at most 256 MB per pass), a second forms the rows from them.
 *   weights: SHG_WEIGHTS_NONE (weights is not read), SHG_WEIGHTS_POINT w [M] or SHG_WEIGHTS_COMPONENT w [M][3], finite and >= 0:
 *   the entries of point i (component c) are multiplied by sqrt(w), as the last operation.
 *   No atomics: the entries of a point do not depend on the other points of the call, and repeated calls are bitwise equal.  Points
 *   at the poles and below R are fine; r = 0 is not.
 *   Arguments are checked before the first HIP call (negative sizes, min_degree > N, N > 32766, NULL pointers, GM or R not finite,
 *   R <= 0, ldt < M, more than 2^40 values of At); M = 0 returns 0 at once.
 * ------------------------------------------------------------------------------------------------ */
enum { SHG_WEIGHTS_NONE = 0, SHG_WEIGHTS_POINT = 1, SHG_WEIGHTS_COMPONENT = 2 };
int shg_acceleration_design(int N, int min_degree, const double* xyz, int M, const double* weights, int weight_layout, double GM, double R,
                            double* At, int ldt, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Design matrix of the gravitational gradient tensor at points, in per-point instrument frames (the partial derivatives of
 * shg_gravitational_gradients_points with respect to the coefficients; no reference counterpart)
 *   At [P][K][ldt], transposed like shg_acceleration_design: row p is coefficient p of utilities.ravel_coefficients(., min_degree, N),
 *   then the K = popcount(components) selected tensor components in ascending bit order (xx, xy, xz, yy, yz, zz), then the M points
 *   xyz [M][3] innermost (ldt >= M; the entries from M to ldt of a row are not touched).  At[p][k][i] = d T'_ab(point i) / d x_p in
 *   s^-2.
 *   frames == NULL: T' = T, the Earth-fixed tensor.  Otherwise frames [M][3][3], row a of frames[i] the instrument axis a in
 *   Earth-fixed coordinates, and T' = F T F^T; the rows must be orthonormal, which is not checked here.
 *   An Earth-fixed entry is the acceleration's first-derivative map applied twice to a unit coefficient: at most four terms
 *   factor * Y[slot] on the solid harmonics of degree N + 2, in units of GM / (4 R^3) (terms on one slot are merged).  A first kernel
 *   writes the solid harmonics of a pass of points to a workspace (at most 256 MB per pass; the colatitude enters as z / r and
 *   rho / r, as in shg_gravitational_gradients_points), a second forms the six entries of a row per point, rotates the selected ones
 *   (each off-diagonal value once) and stores them.
 *   weights: SHG_WEIGHTS_NONE, SHG_WEIGHTS_POINT w [M] or SHG_WEIGHTS_COMPONENT w [M][K] over the selected components, finite and
 *   >= 0: the entries are multiplied by sqrt(w), as the last operation.
 *   No atomics: the entries of a point do not depend on the other points of the call or on the other selected components, and
 *   repeated calls are bitwise equal.  Points at the poles and below R are fine; r = 0 is not.
 *   Arguments are checked before the first HIP call (the rules of shg_acceleration_design with N <= 32765, components in 1 .. 63,
 *   at most 2^40 values of At); M = 0 returns 0 at once.
 *   shg_gradient_design_terms  host only, no HIP call: the table of the Earth-fixed entries, slot / factor [P][6][4] (capacity >= 24 P
 *   entries each): slot = 2 packed(n'', k) + (0 cosine | 1 sine) at degree N + 2 (packed(n, k) = k (N + 3) - k (k - 1) / 2 + n - k), or
 *   -1 for no term; the factors carry the signs but not GM / (4 R^3).  The device call uses the same builder.
 * ------------------------------------------------------------------------------------------------ */
enum { SHG_GRAD_XX = 1, SHG_GRAD_XY = 2, SHG_GRAD_XZ = 4, SHG_GRAD_YY = 8, SHG_GRAD_YZ = 16, SHG_GRAD_ZZ = 32 };
int shg_gradient_design(int N, int min_degree, const double* xyz, int M, const double* frames, int components, const double* weights,
                        int weight_layout, double GM, double R, double* At, int ldt, void* stream);
int shg_gradient_design_terms(int N, int min_degree, int32_t* slot, double* factor, long long capacity);

/* ------------------------------------------------------------------------------------------------
 * Design matrix of the line-of-sight gravity difference of satellite pairs, l_i = e_i . (g(b_i) - g(a_i)) (the inter-satellite link
 * in the acceleration approach; no reference counterpart)
 *   At [P][ldt], transposed like shg_acceleration_design: row p is coefficient p of utilities.ravel_coefficients(., min_degree, N),
 *   the M pairs xyz_a [M][3], xyz_b [M][3] innermost (ldt >= M; the entries from M to ldt of a row are not touched).
 *   At[p][i] = sqrt(w_i) e_i . (d g(b_i) / d x_p - d g(a_i) / d x_p) in m/s^2.
 *   directions == NULL: e_i = (b_i - a_i) / |b_i - a_i|, computed in the kernel as d = b - a per component,
 *   |d| = sqrt((d_x d_x + d_y d_y) + d_z d_z), e_c = d_c / |d|.  A pair with a_i == b_i then gives NaN in its column i: callers must
 *   not pass one (the Python layer refuses them).  Otherwise e_i = directions[i] of directions [M][3], taken as given: unit length is
 *   not checked here.
 *   Per pass of pairs the solid harmonics kernel of shg_acceleration_design runs on the a-points and on the b-points, in one launch
 *   (bitwise the harmonics that call uses), into one workspace; both halves together stay within its 256 MB, so a pass holds
 *   max(256 MB / 8 / (4 packed(N + 1)) rounded down to a multiple of 256, 256) pairs, packed(n) = (n + 1)(n + 2) / 2
 *   (shg_los_design_pass returns this number: host only, no HIP call, -1 for N < 0 or N > 32766).  A second kernel forms, per row and
 *   pair, the three unscaled component sums of the acceleration's table at b and at a, their difference per component, the projection
 *   (e_x d_x + e_y d_y) + e_z d_z, then * GM / (2 R^2), then * sqrt(w) (weights [M], finite and >= 0, or NULL), and stores once.
 *   No atomics: the entries of a pair do not depend on the other pairs of the call, and repeated calls are bitwise equal.  Swapping a
 *   and b leaves At bitwise unchanged with directions == NULL and negates it bitwise with directions given.
 *   Arguments are checked before the first HIP call (the rules of shg_acceleration_design: negative sizes, min_degree > N,
 *   N > 32766, GM or R not finite, R <= 0, ldt < M; NULL xyz_a, xyz_b or At; more than 2^40 values of At); M = 0 returns 0 at once.
 * ------------------------------------------------------------------------------------------------ */
int shg_los_design(int N, int min_degree, const double* xyz_a, const double* xyz_b, const double* directions, int M, const double* weights,
                   double GM, double R, double* At, int ldt, void* stream);
int shg_los_design_pass(int N);

/* ------------------------------------------------------------------------------------------------
 * Gravitational potential at points (the zeroth member beside shg_acceleration_points and shg_gravitational_gradients_points; the
 * reference reaches it only as a grid synthesis with kernel 'potential')
 *   V [B][M] (m^2/s^2), V = GM / R sum_{n,k} (R/r)^(n+1) P_nk (C_nk cos(k lon) + S_nk sin(k lon)), of the fields anm [B][N+1][N+1]
 *   (one GM and R for all) at the Cartesian positions xyz:
 *     layout SHG_POINTS_SHARED     xyz [M][3], the same points for every field
 *     layout SHG_POINTS_PER_EPOCH  xyz [B][M][3], points of their own for every field
 *   A point synthesis of degree N with one component, by the point kernel of shg_acceleration_points (the same column recursion, the
 *   colatitude from atan2 as there), up to 16 epochs per pass.  No atomics: a field's result does not depend on the other fields of
 *   the call or on the layout, and repeated calls are bitwise equal.  Points at the poles and below R are fine; r = 0 is not.
 *   The centrifugal potential and the dissipative integrals of the energy equation are not part of V: they are the caller's reduction.
 *   shg_potential_points_om  the same from an order-major series om [(N+1)^2][Bpad] (shg_order_major_pack), Bpad >= B.
 *   Arguments are checked before the first HIP call (the rules of shg_acceleration_points); nothing to do (M = 0 or B = 0) returns 0 at
 *   once.
 * ------------------------------------------------------------------------------------------------ */
int shg_potential_points(int N, const double* xyz, int M, int layout, const double* anm, int B, double GM, double R, double* V,
                         void* stream);
int shg_potential_points_om(int N, const double* xyz, int M, int layout, const double* om, int B, int Bpad, double GM, double R,
                            double* V, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Point functionals of time-variable fields, every point at its own epoch (no reference counterpart: the reference blends the
 * coefficients per epoch, TimeSeries.interpolate_to / Trend / Oscillation.evaluate_at, and evaluates one point at a time)
 *   A time-variable field is a weighted sum of fixed fields, V(t) = sum_j w_j(t) V_j, and the functionals are linear, so
 *     out[i][c] = scale sum_{j < W} weights[i][j] S_c(field first_i + j, x_i)
 *   with S the unscaled component sum of shg_acceleration_points / shg_potential_points / shg_gravitational_gradients_points and
 *   scale their GM / (2 R^2), GM / R, GM / (4 R^3): g [M][3], V [M] or T [M][3][3] (each off-diagonal value stored twice) at the
 *   Cartesian positions xyz [M][3], of the B fields anm [B][N+1][N+1] (one GM and R for all), 1 <= W <= 16 of them per point.
 *   xyz, weights [M][W], the fields and the output are device pointers.  run_first [runs] and run_begin [runs + 1] are HOST arrays:
 *   run r covers the consecutive points run_begin[r] .. run_begin[r + 1] - 1, all of which use the consecutive fields
 *   run_first[r] .. run_first[r] + W - 1 (a time-ordered orbit against a series: one run per interval between two nodes).
 *   Runs are cut into workgroups of at most 256 points; per workgroup the column recursion of the existing point kernel sweeps
 *   the window in chunks of 2, 4 or 16 fields (gradients: 2 or 4), with the Q values of the existing combine kernels and the same fma
 *   order over orders and degrees, so the sum of a field is bitwise the existing entry point's.  The weighted sum then runs over j
 *   ascending from 0.0 with one fma per term, and the product with scale comes last, once.  No atomics and no read-modify-write: a
 *   point's result depends only on its position, its W weights and its W fields -- not on how the points are cut into runs or
 *   workgroups, on the other points, on B or on the source layout -- and repeated calls are bitwise equal.  With weights that are
 *   one 1.0 and zeros the result equals the existing entry point's value of that field at that point.
 *   The combined coefficients of a launch group of fields stay under a workspace limit (256 MB by default); with more fields the call
 *   loops over field ranges that overlap by W - 1 and launches the runs whose window lies in the range.
 *   shg_*_points_at_om  the same from an order-major series om [(N+1)^2][Bpad] (shg_order_major_pack), Bpad >= B.
 *   shg_points_at_set_workspace_limit  that limit in bytes, process-wide (0 restores the default; negative values are refused); a
 *   call whose window of W fields does not fit the limit fails with a message.
 *   Arguments are checked before the first HIP call: negative sizes, W outside 1 .. 16, B < W, runs < 0, Bpad < B, GM or R not
 *   finite, R <= 0, more than 2^40 output values, the gradients' degree rule of shg_gravitational_gradients_points; then, for
 *   M > 0, NULL pointers, run_begin[0] != 0, run_begin not strictly increasing or not ending at M, and run_first[r] outside
 *   0 .. B - W, so that no table content can make the kernel read outside its buffers.  M = 0 returns 0 at once.
 * ------------------------------------------------------------------------------------------------ */
int shg_acceleration_points_at(int N, const double* xyz, int M, const double* anm, int B, const int* run_first, const int* run_begin, int runs,
                               const double* weights, int W, double GM, double R, double* g, void* stream);
int shg_acceleration_points_at_om(int N, const double* xyz, int M, const double* om, int B, int Bpad, const int* run_first, const int* run_begin,
                                  int runs, const double* weights, int W, double GM, double R, double* g, void* stream);
int shg_potential_points_at(int N, const double* xyz, int M, const double* anm, int B, const int* run_first, const int* run_begin, int runs,
                            const double* weights, int W, double GM, double R, double* V, void* stream);
int shg_potential_points_at_om(int N, const double* xyz, int M, const double* om, int B, int Bpad, const int* run_first, const int* run_begin,
                               int runs, const double* weights, int W, double GM, double R, double* V, void* stream);
int shg_gravitational_gradients_points_at(int N, const double* xyz, int M, const double* anm, int B, const int* run_first, const int* run_begin,
                                          int runs, const double* weights, int W, double GM, double R, double* T, void* stream);
int shg_gravitational_gradients_points_at_om(int N, const double* xyz, int M, const double* om, int B, int Bpad, const int* run_first,
                                             const int* run_begin, int runs, const double* weights, int W, double GM, double R, double* T,
                                             void* stream);
int shg_points_at_set_workspace_limit(long long bytes);

/* ------------------------------------------------------------------------------------------------
 * Design matrices of the energy-balance observations: the potential at points, and the potential difference V(b_i) - V(a_i) of
 * satellite pairs (the partial derivatives of shg_potential_points with respect to the coefficients; no reference counterpart)
 *   At [P][ldt], transposed like shg_acceleration_design: row p is coefficient p of utilities.ravel_coefficients(., min_degree, N),
 *   the M points xyz [M][3] (pairs xyz_a [M][3], xyz_b [M][3]) innermost (ldt >= M; the entries from M to ldt of a row are not
 *   touched).  For a field without coefficients below min_degree, sum_p At[p][i] x_p = V[i] of shg_potential_points (V(b_i) - V(a_i)).
 *   An entry is one solid harmonic of degree N, d V / d C_nm = GM / R Yc_nm and d V / d S_nm = GM / R Ys_nm: one kernel runs the
 *   column recursion of shg_acceleration_design's harmonics (the same operation order, at degree N) with one lane per point, at both
 *   satellites of a pair in lockstep, and stores every value straight to row n^2 - min_degree^2 + (0 | 2k - 1 cosine | 2k sine).  No
 *   workspace beyond the recursion factors, no passes of points.
 *     shg_potential_design             At[p][i] = (Y_p(x_i) * GM / R) * sqrt(w_i), in that order
 *     shg_potential_difference_design  At[p][i] = ((Y_p(b_i) - Y_p(a_i)) * GM / R) * sqrt(w_i): swapping a and b negates At bitwise, and
 *                                      a pair with a_i == b_i gives an exactly zero column i (nothing divides by the separation: such
 *                                      pairs are legal)
 *   weights [M], finite and >= 0, or NULL.  No atomics: the entries of a point do not depend on the other points of the call, and
 *   repeated calls are bitwise equal.  Points at the poles and below R are fine; r = 0 is not.
 *   Arguments are checked before the first HIP call (the rules of shg_acceleration_design with N <= 32767: negative sizes,
 *   min_degree > N, GM or R not finite, R <= 0, ldt < M; NULL positions or At; more than 2^40 values of At); M = 0 returns 0 at once.
 * ------------------------------------------------------------------------------------------------ */
int shg_potential_design(int N, int min_degree, const double* xyz, int M, const double* weights, double GM, double R, double* At, int ldt,
                         void* stream);
int shg_potential_difference_design(int N, int min_degree, const double* xyz_a, const double* xyz_b, int M, const double* weights, double GM,
                                    double R, double* At, int ldt, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Design matrices with respect to the node values of isotropic radial basis functions (gravityfield.RadialBasisFunctions; the
 * reference can only convert that representation, nothing estimates it)
 *   At [J][K][ldt], transposed like shg_acceleration_design: row j is node j, the M points (pairs) innermost (ldt >= M; the entries
 *   from M to ldt of a row are not touched).  nodes (device) [J][4]: the unit vector e_j of node j and R / r_j.  shape (host) [N + 1]:
 *   the shape factor k_n of every degree; degrees below min_degree are not read and count as zero.  With, for a point x = r xh,
 *   t = xh . e_j, q = (R / r)(R / r_j) and d_n = k_n (2n + 1),
 *     V_j(x)      = GM / R sum_n d_n q^(n+1) P_n(t)
 *     grad V_j(x) = GM / (R r) [ -S_r xh + S_t (e_j - t xh) ],  S_r = sum_n (n + 1) d_n q^(n+1) P_n(t),  S_t = sum_n d_n q^(n+1) P'_n(t)
 *   (P_n the unnormalised Legendre polynomials, P_n = (2n-1)/n t P_{n-1} - (n-1)/n P_{n-2}, P'_n = P'_{n-2} + (2n-1) P_{n-1}); these
 *   are the columns of the spherical harmonic design matrices of degrees min_degree .. N times to_potential_coefficients_matrix.
 *     kind SHG_RBF_ACCELERATION          K = 3  At[j][c][i] = d g_c(x_i) / d v_j; weights NONE, POINT w [M] or COMPONENT w [M][3]
 *     kind SHG_RBF_LINE_OF_SIGHT         K = 1  At[j][i] = e_i . (grad V_j(b_i) - grad V_j(a_i)), the difference per component first,
 *                                               then (e_x d_x + e_y d_y) + e_z d_z; e_i = directions[i] as given, or with directions ==
 *                                               NULL (b_i - a_i) / |b_i - a_i| as shg_los_design forms it (NaN for a_i == b_i)
 *     kind SHG_RBF_POTENTIAL             K = 1  At[j][i] = V_j(x_i)
 *     kind SHG_RBF_POTENTIAL_DIFFERENCE  K = 1  At[j][i] = V_j(b_i) - V_j(a_i): swapping a and b negates At bitwise, a_i == b_i gives an
 *                                               exactly zero column i
 *   The single-point kinds read xyz_a only (xyz_b and directions are not looked at); the three kinds with K = 1 take weights NONE or
 *   POINT w [M].  Every entry is (value * scale) * sqrt(w) with scale = GM / R or GM / (R r), the weight last: a weighted matrix is
 *   bitwise the unweighted one times sqrt(w).  One kernel, one lane per point and 256 points per workgroup, a tile of nodes per
 *   workgroup, the recursion of several nodes side by side in a lane (shg_rbf_design_info, host only: which = {nodes per tile, nodes
 *   side by side, points per workgroup, most nodes of a call}); no workspace but the table of N + 1 degrees, no fma, no atomics: an
 *   entry depends on its point and its node only, not on M, J, ldt or the place in the batch, and repeated calls are bitwise equal.
 *   The rows of a pair kind are made of the values the single-point kind computes at the two satellites.  r = 0 is not allowed.
 *   Arguments are checked before the first HIP call (kind outside 0 .. 3, negative sizes, min_degree > N, N > 32767, more nodes than
 *   one call takes, a weight layout the kind does not have, GM or R not finite, R <= 0, ldt < M, more than 2^40 values of At; NULL
 *   shape, nodes, xyz_a, At or weights that are due; NULL xyz_b for a pair kind); M = 0 or J = 0 returns 0 at once.
 * ------------------------------------------------------------------------------------------------ */
enum { SHG_RBF_ACCELERATION = 0, SHG_RBF_LINE_OF_SIGHT = 1, SHG_RBF_POTENTIAL = 2, SHG_RBF_POTENTIAL_DIFFERENCE = 3 };
int shg_rbf_design(int kind, int N, int min_degree, const double* shape, const double* nodes, int J, const double* xyz_a, const double* xyz_b,
                   const double* directions, int M, const double* weights, int weight_layout, double GM, double R, double* At, int ldt,
                   void* stream);
int shg_rbf_design_info(int which[4]);

/* ------------------------------------------------------------------------------------------------
 * Design matrix of the gravitational gradient tensor with respect to the node values of isotropic radial basis functions
 *   At [J][K][ldt], the layout of shg_gradient_design with the nodes of shg_rbf_design as rows: At[j][k][i] is the derivative of the
 *   k-th selected component of T' = F_i T F_i^T at point i with respect to node value j (ldt >= M; the entries from M to ldt of a row
 *   are not touched).  shape, nodes, N and min_degree as in shg_rbf_design; frames, components, weights and weight_layout as in
 *   shg_gradient_design (frames NULL: the Earth-fixed tensor; components a set of SHG_GRAD_* bits, rows in ascending bit order;
 *   weights NONE, POINT w [M] or COMPONENT w [M][K]).  With the notation of shg_rbf_design and tau = e_j - t xh,
 *     Hess V_j(x) = GM / (R r^2) [ S_rr xh xh^T - (S_r + t S_t)(I - xh xh^T) - (S_rt + S_t)(xh tau^T + tau xh^T) + S_tt tau tau^T ]
 *     S_rr = sum_n (n + 1)(n + 2) d_n q^(n+1) P_n(t),  S_rt = sum_n (n + 1) d_n q^(n+1) P'_n(t),  S_tt = sum_n d_n q^(n+1) P''_n(t)
 *   (P''_n = P''_{n-2} + (2n-1) P'_{n-1}): symmetric by construction, trace-free degree by degree, regular above a node and antipodal
 *   to it (tau = 0; nothing divides by a sine).  These are the columns of shg_gradient_design of degrees min_degree .. N times
 *   to_potential_coefficients_matrix.  The rotation is that of shg_gradient_design, T f_b once per needed b, then f_a . (T f_b), exact
 *   for identity frames; every entry is (value * scale) * sqrt(w) with scale = GM / (R r^2).  The launch geometry is that of
 *   shg_rbf_design (shg_rbf_design_info: the same node tile, nodes side by side in a lane and points per workgroup);
 *   no workspace but the table of N + 1 degrees, no fma, no atomics: an entry depends on its point, its frame and its node only, not
 *   on M, J, ldt, the component set or the place in the batch, and repeated calls are bitwise equal.  r = 0 is not allowed.
 *   Every argument is checked before the first HIP call (components outside 1 .. 63; N, min_degree, J or M < 0; min_degree > N;
 *   N > 32767; J above the nodes one call takes; an unknown weight layout; GM or R not finite, R <= 0; ldt < M; more than 2^40 values
 *   of At; NULL shape, nodes, xyz, At or weights that are due); M = 0 or J = 0 returns 0 at once.
 * ------------------------------------------------------------------------------------------------ */
int shg_rbf_gradient_design(int N, int min_degree, const double* shape, const double* nodes, int J, const double* xyz, int M, const double* frames,
                            int components, const double* weights, int weight_layout, double GM, double R, double* At, int ldt, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Surface synthesis of the node values of isotropic radial basis functions (no reference counterpart)
 *   St [J][ldt], transposed with the points innermost (the layout of shg_rbf_design: St viewed as [J, M] is a gemm operand as it
 *   stands; ldt >= M, the entries from M to ldt of a row are not touched):
 *     St[j][i] = sum_{n = min_degree .. N} kn[n][i] d_n u_j^(n+1) P_n(e_i . e_j),     d_n = k_n (2n + 1),  u_j = R / r_j
 *   the value at grid point i of the functional whose surface factors are kn, for a unit value at node j.  shape [N + 1] (host), nodes
 *   [J][4] (device), N and min_degree as in shg_rbf_design; points [M][3] (device) are the unit vectors e_i of the grid points; kn
 *   [N + 1][ldk] (device, ldk >= M) is DEGREE-MAJOR with the points innermost, kn[n][i] = (1 / k_n(r_i, theta_i)) (R / r_i)^(n+1) GM / R
 *   of gravityfield.surface_factors.  The rows of kn below max(min_degree, 1) are never read, row 0 only when min_degree is 0: an
 *   inverse kernel coefficient that is not finite at degree 0 or 1 does not reach a band that starts at 2.
 *   One kernel with the launch geometry of shg_rbf_design (shg_rbf_surface_info, host only: which = {nodes per tile, nodes side by
 *   side in a lane, points per workgroup, most nodes of a call}); P_n by the recursion of shg_rbf_design, u^(n+1) as a running
 *   product, c = kn[n][i] d_n once per lane and degree, then s = s + c (u^(n+1) P_n); no workspace but the table of N + 1 degrees, no
 *   fma, no atomics, no LDS: an entry depends on its point and its node only, not on M, J, ldk, ldt or the place in the batch, and
 *   repeated calls are bitwise equal.  Arguments are checked before the first HIP call (N, min_degree, J or M < 0; min_degree > N;
 *   N > 32767; J above the nodes one call takes; ldk < M; ldt < M; more than 2^40 values of St; NULL shape, nodes, points, kn or St);
 *   M = 0 or J = 0 returns 0 at once.
 * ------------------------------------------------------------------------------------------------ */
int shg_rbf_surface(int N, int min_degree, const double* shape, const double* nodes, int J, const double* points, const double* kn, int ldk, int M,
                    double* St, int ldt, void* stream);
int shg_rbf_surface_info(int which[4]);

/* ------------------------------------------------------------------------------------------------
 * Column dot products: out[i] = sum_r X[r][i] Y[r][i] for X [rows][ldx], Y [rows][ldy] (device, ldx, ldy >= cols), out [cols]
 *   The diagonal of X^T Y without the product: with X = St and Y = C St of shg_rbf_surface, diag(S C S^T).  One lane per column; row r
 *   goes to partial sum r % 8 of its column in ascending order, every product rounded before it is added (no fma), and the eight sums
 *   close as ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)): the order depends on `rows` alone, not on cols, the launch or the
 *   position of the column, no atomics -- two calls, or a column computed within any batch, give the same bits.  rows = 0 gives zeros.
 *   Checked before the first HIP call: negative sizes, ldx or ldy < cols, NULL out, NULL X or Y with rows > 0; cols = 0 returns 0 at once.
 * ------------------------------------------------------------------------------------------------ */
int shg_column_dots(int rows, int cols, const double* X, int ldx, const double* Y, int ldy, double* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Leverages of observations: out[j] = sum_{p < n} z_pj^2, z_pj = sum_{q <= p} Ui[q][p] X[q][j]  (no reference
 * counterpart)
 *   Ui [n][ldu] (device): the upper triangular inverse U^-1 of the Cholesky factor N = U^T U, as shg_trtri writes it; what lies below
 *   its diagonal is not used and may hold anything, NaN included (the entries are replaced by zeros while a tile of the diagonal block
 *   is staged, as under the SHG_GEMM_A_* flags).  X [n][ldx] (device) with `cols` columns in use: a block At~ [P][K Mb] of the whitened,
 *   weighted transposed design matrix as it stands.  out [cols]: out[j] = |U^-T x_j|^2 = x_j^T N^-1 x_j, the diagonal of the hat matrix.
 *   Z = Ui^T X is never written: a workgroup forms a 128 x 128 tile of it on the fp64 MFMA (v_mfma_f64_16x16x4_f64), squares the
 *   accumulators and sums them over the rows of the tile.  The K range of row tile t ends with its diagonal block (q < 128 t + 128):
 *   half the MFMAs of the full product.  Workgroups tile (row tile, column tile), longest row tiles first; every tile writes its sums
 *   to [row tiles][cols] doubles of the stream's scratch (shg_scratch_release) and a second kernel adds the row tiles in ascending
 *   order.
 *   Order: q ascending from 0 in steps of 4 (one MFMA each), whatever cols, the alignment or the launch; per tile and column the
 *   squares are added by fma in ascending row order per lane, the four lanes of a column by the butterfly over lanes ^ 16, ^ 32, then
 *   the two wave rows.  No atomics: out[j] depends on n, Ui and column j only -- a column computed alone, in any batch or at any column
 *   offset gives the same bits, and repeated calls are bitwise equal.
 *   A flat 64-bit index, so n x ldx may exceed 2^31.  The entries of out beyond cols and the padding of X from cols to ldx are neither
 *   read nor written.
 *   Arguments are checked before the first HIP call (negative sizes, ldu < n, ldx < cols, more than 2^40 values of Ui or X, and with
 *   cols > 0: NULL out, NULL Ui or X when n > 0); cols = 0 returns 0 at once, n = 0 writes zeros.
 * ------------------------------------------------------------------------------------------------ */
int shg_leverages(int n, long long cols, const double* Ui, int ldu, const double* X, long long ldx, double* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Decorrelation of coloured observation noise along the point axis (the banded lower-triangular W with W^T W = Sigma^-1 of a sequence
 * of scalar AR models of orders 0 .. q; no reference counterpart)
 *   X [rows][ldx] with M columns in use, row r of channel r % channels: the transposed design matrix At [P][K][ldt] of the three calls
 *   above is rows = P K, channels = K; observations laid out [K][M] are rows = K, channels = K.
 *   taps (device) [channels][q+1][q+1]: row s of a channel is h[s][0] = 1 / sigma_s, h[s][k] = -phi_k / sigma_s (1 <= k <= s) of its AR
 *   model of order s, zero beyond.  stage (device) [M]: the order in use at column t, min(t - start of its arc, q).
 *   Y[r][t - skip] = sum_{k = 0 .. n} h[n][k] X[r][t - k] for skip <= t < M, with n = min(max(stage[t], 0), q, t): the first skip
 *   columns are read as history and not written (the halo of a block of a longer series); the entries of a row of Y from M - skip
 *   to ldy are not touched.  The kernel never reads before column 0 of a row and never a tap outside its table, whatever stage holds.
 *   The sum is acc = h[0] x[t], then acc = fma(h[k], x[t-k], acc) for k ascending: Y[r][t - skip] depends on x[t-n .. t], stage[t] and
 *   the taps only, not on skip, M, the tiling or the other rows.  No atomics; repeated calls are bitwise equal, and a block whitened
 *   with a halo of q columns is bitwise the same columns of the whole.
 *   One workgroup per tile of 1024 columns of a row, staged through LDS with the q columns in front (one read and one write of the
 *   matrix); a flat 64-bit index, so rows x ld may exceed 2^31.
 *   Arguments are checked before the first HIP call (negative sizes, channels < 1, rows not a multiple of channels, q outside 0 .. 128,
 *   skip outside 0 .. M, ldx < M, ldy < M - skip, more than 2^40 values of X or Y, NULL pointers, address ranges of X and Y that
 *   overlap: the call is out of place); rows = 0 or M = skip returns 0 at once.
 * ------------------------------------------------------------------------------------------------ */
int shg_whiten_rows(long long rows, int channels, int M, const double* X, long long ldx, const int32_t* stage, const double* taps, int q,
                    int skip, double* Y, long long ldy, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Decorrelation with long filters, 0 <= q <= 4095: the arcs of a series under their full covariance matrices, W = inv(cholesky(
 * Toeplitz(c_0 .. c_q))) for every arc of up to q + 1 points and the AR(q) continuation beyond (no reference
 * counterpart)
 *   The arguments and the definition of shg_whiten_rows: X [rows][ldx] with M columns in use, row r of channel r % channels, taps
 *   (device) [channels][q+1][q+1], stage (device) [M], and
 *   Y[r][t - skip] = sum_{k = 0 .. n} h_c[n][k] X[r][t - k] for skip <= t < M, n = min(max(stage[t], 0), q, t), c = r % channels.
 *   Per channel this is the product Y_c = X_c B_c with the banded upper triangular B_c[t'][t] = h_c[n_t][t - t'] (0 <= t - t' <= n_t,
 *   +0.0 elsewhere) on the fp64 MFMA (v_mfma_f64_16x16x4_f64).  B is never stored: a workgroup owns 128 rows of one channel by 128
 *   output columns and generates the 16 x 128 tiles of its band of B from the tap table while it stages them; its K range runs from
 *   the smallest t - n_t of its columns to its last column, 2 rows (M - skip) (q~ + 128) flops in all, fewer in the start-up tiles of
 *   an arc.  Grid (column tiles, row tiles x channels), the latter in launches of 32768; a flat 64-bit index, so rows x ld may
 *   exceed 2^31.
 *   Order: one workgroup per output tile, K ascending from the first column of the band in steps of 4 (one MFMA each).  No atomics;
 *   repeated calls are bitwise equal.
 *   The one difference from shg_whiten_rows: the zeros of B multiply values of X outside x[t - n .. t], so the columns 0 .. M - 1 of
 *   X must be finite, and Y[r][t - skip] depends on the position of t in its tile: a block whitened with its halo equals the same
 *   columns of the whole within the rounding bound (n + 2) 2^-53 sum_k |h[n][k]| |x[t-k]| of either, not bitwise.
 *   The padding of X from M to ldx is never read, the padding of Y from M - skip to ldy never written.  stage is clamped as in
 *   shg_whiten_rows: a wrong table gives wrong numbers, never an access outside a row or the tap table.  Rows past `rows` and columns
 *   past M are clamped on load and not stored.
 *   Arguments are checked before the first HIP call as in shg_whiten_rows (negative sizes, channels < 1, rows not a multiple of
 *   channels, q outside 0 .. 4095, skip outside 0 .. M, ldx < M, ldy < M - skip, more than 2^40 values of X or Y, NULL pointers,
 *   address ranges of X and Y that overlap); rows = 0 or M = skip returns 0 at once.
 * ------------------------------------------------------------------------------------------------ */
int shg_whiten_rows_long(long long rows, int channels, int M, const double* X, long long ldx, const int32_t* stage, const double* taps, int q,
                         int skip, double* Y, long long ldy, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Products of the rows of a matrix with a basis, cut at arc boundaries: what the elimination of arc-wise parameters needs of the
 * transposed design matrix (C_a = A_a^T B_a; no reference counterpart)
 *   X [rows][ldx] with M columns in use, row r of channel r % channels (the row convention of shg_whiten_rows: At [P][K][ldt] is
 *   rows = P K, channels = K; observations laid out [K][M] are rows = K, channels = K).  Bt [u][channels][ldb]: the basis, transformed
 *   like the design matrix and transposed, 1 <= u <= 16.  seg (device) [nseg + 1]: column indices, segment s is seg[s] .. seg[s+1] - 1.
 *   S[r][s][j] = sum_{t = seg[s] .. seg[s+1] - 1} X[r][t] Bt[j][r % channels][t];  S [rows][nseg][u] is dense and every entry is
 *   written, 0 for an empty segment.
 *   Locality: S[r][s][j] depends only on X[r][seg[s] .. seg[s+1]) and on the basis values at those columns, not on rows, nseg, M, the
 *   other segments, the position of the segment in the row or the launch geometry.  Columns outside every segment are not read.
 *   Summation order, relative to the start of the segment: chain i of 64 is acc = 0, acc = fma(x[t], b[t], acc) over the columns
 *   t = start + i, start + i + 64, ... ascending (an empty chain is 0); the chains are added by the butterfly v_i += v_(i ^ m) for
 *   m = 32, 16, 8, 4, 2, 1, and entry 0 is the result.  No atomics; repeated calls are bitwise equal.
 *   Clamping: entry i of seg is read as c_i = max over k <= i of min(max(seg[k], 0), M), so the table in effect lies in 0 .. M and
 *   does not decrease; a wrong table gives wrong numbers, never a read outside a row.
 *   One wave per segment of 4 rows of one channel (2 rows above u = 8; lane <-> column, coalesced): X is read from global memory
 *   once, a basis value once per 4 (2) rows (from cache: the basis of a block is at most 16 K M doubles); a flat 64-bit index, so
 *   rows x ldx may exceed 2^31.
 *   Arguments are checked before the first HIP call (negative sizes, channels < 1, rows not a multiple of channels, u outside
 *   1 .. 16, nseg < 0, ldx < M, ldb < M, more than 2^40 values of X or S, NULL pointers); rows = 0 or nseg = 0 returns 0 at once.
 * ------------------------------------------------------------------------------------------------ */
int shg_segment_products(long long rows, int channels, int M, const double* X, long long ldx, const double* Bt, long long ldb, int u, int nseg,
                         const int32_t* seg, double* S, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Lagged products of the rows of a matrix with themselves, cut at arc boundaries: the square sums per arc (lag 0) and the empirical
 * autocovariance (lags 0 .. q) of post-fit residuals (no reference counterpart)
 *   X [rows][ldx] with M columns in use.  seg (device) [nseg + 1]: column indices, segment s is seg[s] .. seg[s+1] - 1.  0 <= lags <= 128.
 *   S[r][s][k] = sum over t with seg[s] <= t and t + k < seg[s+1] of X[r][t] X[r][t + k], k = 0 .. lags;  S [rows][nseg][lags + 1] is
 *   dense and every entry is written, 0 where the segment has k columns or fewer.
 *   Locality: S[r][s][k] depends only on X[r][seg[s] .. seg[s+1]) and on k, not on rows, nseg, M, lags, the other segments, the
 *   position of the segment in the row or the launch geometry.  Columns outside every segment and the padding from M to ldx are not
 *   read.
 *   Summation order, relative to the start of the segment: chain i of 64 is acc = 0, acc = fma(x[t], x[t + k], acc) over
 *   t = start + i, start + i + 64, ... ascending while t + k < end (an empty chain is 0); the chains are added by the butterfly
 *   v_i += v_(i ^ m) for m = 32, 16, 8, 4, 2, 1, and entry 0 is the result.  No atomics; repeated calls are bitwise equal.
 *   Clamping: entry i of seg is read as c_i = max over k <= i of min(max(seg[k], 0), M), so the table in effect lies in 0 .. M and
 *   does not decrease; a wrong table gives wrong numbers, never a read outside a row.
 *   lags = 0: one wave per segment of 4 consecutive rows (lane <-> column, coalesced), X is read from global memory once.  lags > 0:
 *   one workgroup of 4 waves per segment of a row, in tiles of 1024 columns staged in LDS with the `lags` columns behind them; wave w
 *   holds the lags w G .. w G + G - 1, G the smallest of 1, 2, 4, 8, 16, 33 with 4 G > lags.  A flat 64-bit index, so rows x ldx may
 *   exceed 2^31.
 *   Arguments are checked before the first HIP call (negative sizes, lags outside 0 .. 128, nseg < 0, ldx < M, more than 2^40 values
 *   of X or S, NULL pointers); rows = 0 or nseg = 0 returns 0 at once.
 * ------------------------------------------------------------------------------------------------ */
int shg_segment_lag_products(long long rows, int M, const double* X, long long ldx, int lags, int nseg, const int32_t* seg, double* S,
                             void* stream);

/* ------------------------------------------------------------------------------------------------
 * The same lagged products for up to 4095 lags, on the fp64 MFMA: the covariance function of post-fit residuals as far as
 * shg_whiten_rows_long can use it (no reference counterpart)
 *   The definition, the arguments and the layout of S are those of shg_segment_lag_products, with 0 <= lags <= 4095:
 *   S[r][s][k] = sum over t with seg[s] <= t and t + k < seg[s+1] of X[r][t] X[r][t + k], k = 0 .. lags;  S [rows][nseg][lags + 1] is
 *   dense and every entry is written; an entry without a pair (a segment of k columns or fewer, an empty segment) is exactly 0.0.
 *   Formulation: relative to the start of the segment, A[i][c] = x[c - 16 i], B[c][j] = x[c + j + k0] and D = A B on
 *   v_mfma_f64_16x16x4_f64: D[i][j] is the lag k0 + 16 i + j, so one 16 x 16 accumulator holds `tile_lags` = 256 consecutive lags and
 *   nothing is discarded.  A segment is cut into chunks of `chunk` = 2048 columns counted from its start, the last one taking what is
 *   left, up to 2560; a chunk is one workgroup, which stages its values of x in LDS once; wave w of 4 takes the first factors x[t]
 *   of quarter w of the chunk (512 columns; a fourth, rounded up to a multiple of 4, of a chunk above 2048).
 *   Summation order of an entry: per quarter the chain of MFMA steps over t ascending, 4 columns a step, from the start of the
 *   quarter; the quarters of a chunk are added as ((q0 + q1) + q2) + q3 (a quarter past the end of the segment is +0.0) and written
 *   to a workspace of the call; a second kernel adds the chunks of a segment in ascending order.  No atomics.
 *   Locality: S[r][s][k] depends only on X[r][seg[s] .. seg[s+1]) and on k, not on the row index, rows, nseg, M, lags, the other
 *   segments, the position of the segment in the row (odd offsets included) or the launch; repeated calls are bitwise equal.
 *   Positions outside the segment become +0.0 by a select while the values are staged, never by a product: columns outside every
 *   segment and the padding from M to ldx may hold anything (NaN, 1e300) and are not read.  Zeros do multiply values of the segment
 *   itself (a partner past its end, a first factor of another quarter), so the values inside a segment must be finite, unlike under
 *   shg_segment_lag_products and as under shg_whiten_rows_long.
 *   Clamping: entry i of seg is read as c_i = max over k <= i of min(max(seg[k], 0), M), by the function shg_segment_lag_products
 *   uses; a wrong table gives wrong numbers, never an access outside a row, the table or the workspace.
 *   Workspace (stream-ordered, freed with the call): rows x (M / 2048 + nseg) x 256 (lags / 256 + 1) doubles of partial sums and
 *   two small tables.
 *   Arguments are checked before the first HIP call (negative sizes, lags outside 0 .. 4095, nseg < 0, ldx < M, more than 2^40 values
 *   of X, of S or of the workspace, NULL pointers); rows = 0 or nseg = 0 returns 0 after these checks, before any pointer is looked at.
 *   shg_segment_lag_long_info: chunk (2048), tile_lags (256) and max_lags (4095); host only, NULL pointers are skipped.
 * ------------------------------------------------------------------------------------------------ */
int shg_segment_lag_products_long(long long rows, int M, const double* X, long long ldx, int lags, int nseg, const int32_t* seg, double* S,
                                  void* stream);
int shg_segment_lag_long_info(int* chunk, int* tile_lags, int* max_lags);

/* ------------------------------------------------------------------------------------------------
 * Decorrelation of vector noise along the point axis: the block lower-triangular banded W with W^T W = Sigma^-1 of a sequence of
 * VAR models of dimension K and orders 0 .. q, which couple the components of a point (no reference
 * counterpart)
 *   X [groups K][ldx] with M columns in use, row g K + c is component c of group g: the transposed design matrix At [P][K][ldt] is
 *   groups = P; observations laid out [K][M] are groups = 1.  2 <= K <= 6.
 *   taps (device) [q+1][q+1][K][K]: H[s][0] = R_s^-T, H[s][k] = -R_s^-T B_k^(s) (1 <= k <= s) of the model of order s with coefficients
 *   B_k^(s) and white-noise covariance R_s^T R_s (R_s upper triangular), zero beyond.  stage (device) [M]: the order in use at column t,
 *   min(t - start of its arc, q).
 *   Y[g K + c][t - skip] = sum_{k = 0 .. n} sum_{c' = 0 .. K-1} H[n][k][c][c'] X[g K + c'][t - k] for skip <= t < M, with
 *   n = min(max(stage[t], 0), q, t): the first skip columns are read as history and not written (the halo of a block of a longer
 *   series); the entries of a row of Y from M - skip to ldy are not touched, the padding of X from M to ldx is not read.  The kernel
 *   never reads before column 0 of a row and never a tap outside its table, whatever stage holds.
 *   The sum runs over k ascending and, inside, over c' ascending; the first term is a product, every later one acc = fma(H, x, acc):
 *   an output depends on x[t-n .. t] of its group, stage[t] and the taps only, not on skip, M, the tiling or the other groups.  No
 *   atomics; repeated calls are bitwise equal, and a block whitened with a halo of q columns is bitwise the same columns of the whole.
 *   One workgroup per tile of columns of the K rows of a group, staged through LDS with the q columns in front; a lane owns 4 (K <= 3)
 *   or 2 consecutive columns of all K rows, takes the taps of the stationary model through scalar loads and keeps the values of x it
 *   meets again at the next lag in registers.  shg_whiten_vector_info gives the tile: 1024 columns for K <= 3, 512 above.  A flat
 *   64-bit index, so groups x K x ld may exceed 2^31.
 *   Arguments are checked before the first HIP call (negative sizes, K outside 2 .. 6, q outside 0 .. 128, skip outside 0 .. M,
 *   ldx < M, ldy < M - skip, more than 2^40 values of X or Y, NULL pointers, address ranges of X and Y that overlap: the call is out
 *   of place); groups = 0 or M = skip returns 0 at once.
 *   shg_whiten_vector_info: host only; -1 for K outside 2 .. 6, a NULL pointer is skipped.
 * ------------------------------------------------------------------------------------------------ */
int shg_whiten_rows_vector(long long groups, int K, int M, const double* X, long long ldx, const int32_t* stage, const double* taps, int q,
                           int skip, double* Y, long long ldy, void* stream);
int shg_whiten_vector_info(int K, int* tile_columns);

/* ------------------------------------------------------------------------------------------------
 * Lagged products between the rows of a matrix, cut at arc boundaries: the empirical cross-covariance function of the K components
 * of post-fit residuals (no reference counterpart)
 *   X [K][ldx] with M columns in use, 1 <= K <= 6.  seg (device) [nseg + 1]: column indices, segment s is seg[s] .. seg[s+1] - 1.
 *   0 <= lags <= 128.
 *   S[s][k][c][c'] = sum over t with seg[s] <= t and t + k < seg[s+1] of X[c][t] X[c'][t + k], k = 0 .. lags;  S [nseg][lags + 1][K][K]
 *   is dense and every entry is written; an entry without a pair is exactly 0.0.
 *   The summation order, the locality and the clamping of seg are those of shg_segment_lag_products: chain i of 64 is acc = 0,
 *   acc = fma(x_c[t], x_c'[t + k], acc) over t = start + i, start + i + 64, ... ascending while t + k < end, the chains are added by
 *   the butterfly v_i += v_(i ^ m) for m = 32, 16, 8, 4, 2, 1; entry i of seg is read as max over k <= i of min(max(seg[k], 0), M).
 *   So S[s][k][c][c] is bitwise shg_segment_lag_products of row c; an entry depends on the two rows inside the segment and on k
 *   only.  Columns outside every segment and the padding from M to ldx are not read.  No atomics; repeated calls are bitwise equal.
 *   One workgroup of 4 waves per segment of a pair (c, c'), in tiles of 1024 columns staged in LDS.
 *   Arguments are checked before the first HIP call (negative sizes, K outside 1 .. 6, lags outside 0 .. 128, nseg < 0 or above
 *   2^24, ldx < M, more than 2^40 values of X, NULL pointers); nseg = 0 returns 0 at once.
 * ------------------------------------------------------------------------------------------------ */
int shg_segment_cross_lag_products(int K, int M, const double* X, long long ldx, int lags, int nseg, const int32_t* seg, double* S,
                                   void* stream);

/* ------------------------------------------------------------------------------------------------
 * Window expansion of a transposed design matrix: the adjoint of the window model of the shg_*_points_at calls, for parameters
 * that vary in time (no reference counterpart)
 *   T [rows][ldt] with n columns in use (the transposed design matrix At [P][K][ldt] of a block is rows = P K).  factors (device)
 *   [n][W], 1 <= W <= 16: the W factors of every column.  run_slot [runs] and run_begin [runs + 1] are HOST tables, as the
 *   shg_*_points_at calls take theirs: run r covers the columns run_begin[r] .. run_begin[r + 1] - 1, whose window starts at slot
 *   run_slot[r], 0 <= run_slot[r] <= E - W, W <= E <= 16.
 *   S[e][r][t] = factors[t][e - slot(t)] * T[r][t] for slot(t) <= e < slot(t) + W and +0.0 for every other e < E, at
 *   S + e slot_stride + r lds + t: all E slots of the n columns of every row are written, each exactly once, the zeros included (no
 *   memset, no read of S, no atomics; one IEEE product per entry inside the window, whatever the launch geometry: repeated calls are
 *   bitwise equal).  The entries of a row of S from n to lds and whatever lies between the slots are not touched.
 *   Bandwidth-bound: one read of T and E writes.  Lanes run along t; a lane keeps the factors of its columns in registers and walks
 *   down the rows.  With T and S on 16-byte boundaries and ldt, lds and slot_stride even, a lane holds two adjacent columns and
 *   stores 16 bytes (a pair across a run boundary and the last column of an odd n: 8 bytes); otherwise one column, 8 bytes.  A flat
 *   64-bit index, so rows x ld may exceed 2^31.
 *   Arguments are checked before the first HIP call (negative sizes, W outside 1 .. 16, E outside W .. 16, ldt < n, lds < n,
 *   slot_stride below the extent of one slot, more than 2^40 values of T or S, NULL pointers, address ranges of T and S that overlap),
 *   the run tables in full (run_begin[0] = 0, strictly increasing, run_begin[runs] = n, every run_slot in 0 .. E - W): no table
 *   content can make the kernel read or write outside its buffers.  The tables reach the device through a workspace of the call
 *   (one copy and one wait on the stream).  rows = 0 or n = 0 returns 0 at once.
 * ------------------------------------------------------------------------------------------------ */
int shg_window_expand(long long rows, int n, const double* T, long long ldt, const int32_t* run_slot, const int32_t* run_begin, int runs,
                      const double* factors, int W, int E, double* S, long long lds, long long slot_stride, void* stream);

/* ------------------------------------------------------------------------------------------------
 * One-sided Jacobi singular value decomposition of small matrices, one workgroup per matrix, G in LDS for the whole call
 * (jacobi.hip; no reference counterpart)
 *   G [batch][r][ldg] row-major with c columns in use (device), in: the matrices, out: G V = U diag(sigma): its columns are
 *   orthogonal.  V [batch][c][ldv]: the right singular vectors as columns (the product of the rotations); may not be NULL.
 *   sigma [batch][c]: the column norms of the final G in the order of its columns (unsorted).  sweeps [batch] (device int): sweeps
 *   used, the last of them without a rotation, or -1 when max_sweeps (>= 1) did not suffice.
 *   Limits: 1 <= r <= 128, 1 <= c <= 128 (128 x 129 doubles of the CU's 160 KiB of LDS), batch >= 1, ldg >= c, ldv >= c, and for
 *   batch > 1 strides that cover one matrix; anything else returns SHG_ERR_INVALID before any HIP call.  r < c is allowed (the
 *   surplus columns end as zeros up to rounding).
 *   Round-robin order of the pairs, rotation when |g_p.g_q| > sqrt(r) 2^-53 |g_p| |g_q| (LAPACK dgesvj); the order of every sum is
 *   fixed, so repeated calls are bitwise equal.  A zero column stays zero.  Non-finite input fires no rotation: the call reports one
 *   sweep and its outputs are unspecified, but in bounds.  Entries of G and V beyond column c and sigma, G, V of other matrices are
 *   not touched.  Where G and V do not fit the LDS together, V is kept in a stream-ordered workspace of batch c^2 doubles.
 * ------------------------------------------------------------------------------------------------ */
int shg_jacobi_svd(double* G, int ldg, long strideG, double* V, int ldv, long strideV, double* sigma, int r, int c, int batch, int max_sweeps,
                   int* sweeps, void* stream);

/* Some operations keep their scratch buffers per stream between calls (the split-K workspace of the block products, the
 * buffers of shg_analysis: freeing stream-ordered memory costs more than these calls take).  This gives them back; it waits
 * for the device first. */
int shg_scratch_release(void);
const char* shg_last_error(void);
const char* shg_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SHG_H */

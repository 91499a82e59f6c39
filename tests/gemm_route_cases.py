"""
The routes of the dense fp64 product dispatcher (grates_amd/csrc/blas.hip: gemm_route) as one table of named cases,
arguments -> expected route, shared by tests/test_gemm_routes_cpu.py (the decision alone, no GPU) and
tests/test_gpu_gemm_routes.py (every case run and checked on the device).  DESIGN.md "Routes of the dense product" is the prose twin.

Every expectation below was worked out by hand from the rules; the arithmetic is in the comment of the case.  Notation:
t128 / t64 = output tiles of 128 / 64 (rows x columns x batch), gx x gy = grid of the chosen tile size.

Thresholds of the dispatcher that NO argument set can reach alone (found while building the table; the conditions are implied by others):
  * split-K `tiles < 384`: a product is only split when t64 < 256 (else it takes 64-tiles), and then tiles <= t64 < 256; the
    padded strip grid has at most 8 * 2 * 6 = 96 workgroups under t64 < 256.  No 383 / 384 pair exists.
  * tail split `tiles >= 512`, `tiles > 768` and `rows_per_round >= 8`: whole > 0 and rest > 0 already mean
    (rows_per_round + 1) * col_tiles > 768 tiles, and col_tiles <= 8 gives rows_per_round >= 96.  768 tiles (8 x 96, no remaining
    rows) and the smallest split products (769 = 1 x 769, 770 = 7 x 110) stand on the two sides instead.
  * narrow `tiles64 >= 512`: narrow only matters where t128 >= 512, and t64 >= t128.
"""

A_UPPER, A_LOWER, B_UPPER, B_LOWER, UPPER_ONLY = 1, 2, 4, 8, 16

MODIFIERS = ('splitk1', 'splitk2', 'strips', 'tail', 'a_lower', 'b_upper', 'tri_gemv', 'upper_only', 'batch>2', 'narrow', 'inplace')

CASES = {}


def route(kind, slices=1, chunk=0, strips=False, m_main=0, a_lower=False, b_upper=False, alias='', rest=None):
    return {'kind': kind, 'slices': slices, 'chunk': chunk, 'strips': strips, 'm_main': m_main, 'a_lower': a_lower, 'b_upper': b_upper,
            'alias': alias, 'rest': rest}


def case(name, M, N, K, expect, ta=False, tb=False, batch=1, flags=0, pad=(0, 0, 3), b_offset=0, inplace='', repeat='', covers=(), door='ex'):
    """pad: extra columns of the stored A, B, C (leading dimension = columns + pad); b_offset: elements between an aligned
    address and B; inplace: 'A' / 'B' = the output IS that operand (pad of C ignored); repeat: operands with stride 0 in a batch;
    covers: the modifiers of MODIFIERS this case stands for; door: 'ex' = shg_gemm_ex only, 'both' = shg_gemm takes it too."""
    assert name not in CASES and all(c in MODIFIERS for c in covers)
    if batch == 1 and flags == 0 and not inplace:
        door = 'both'
    CASES[name] = dict(name=name, M=M, N=N, K=K, ta=ta, tb=tb, batch=batch, flags=flags, pad=pad, b_offset=b_offset, inplace=inplace,
                       repeat=repeat, covers=tuple(covers), expect=expect, door=door)


def layout(c):
    """Stored shapes, leading dimensions and item strides (elements) of a case: dict with rowsA, colsA, lda, strideA, ... ldc, strideC."""
    M, N, K = c['M'], c['N'], c['K']
    rowsA, colsA = (K, M) if c['ta'] else (M, K)
    rowsB, colsB = (N, K) if c['tb'] else (K, N)
    lda, ldb, ldc = max(colsA + c['pad'][0], 1), max(colsB + c['pad'][1], 1), max(N + c['pad'][2], 1)
    if c['inplace'] == 'A':
        ldc = lda
    if c['inplace'] == 'B':
        ldc = ldb
    many = c['batch'] > 1
    return dict(rowsA=rowsA, colsA=colsA, lda=lda, strideA=rowsA * lda if many and 'A' not in c['repeat'] else 0,
                rowsB=rowsB, colsB=colsB, ldb=ldb, strideB=rowsB * ldb + c['b_offset'] if many and 'B' not in c['repeat'] else 0,
                ldc=ldc, strideC=(rowsA * lda if c['inplace'] == 'A' else rowsB * ldb + c['b_offset'] if c['inplace'] == 'B' else M * ldc) if many else 0)


def route_arguments(c, a_ptr, b_ptr, c_ptr):
    """The leading arguments of engine.gemm_route for a case and the addresses of its operands (b_ptr: the address of B itself)."""
    L = layout(c)
    return (c['ta'], c['tb'], c['M'], c['N'], c['K'], a_ptr, L['lda'], L['strideA'], b_ptr, L['ldb'], L['strideB'],
            c_ptr, L['ldc'], L['strideC'], c['batch'], c['flags'])


T64, T128 = 'TILE64', 'TILE128'

# ---- one case per route kind ---------------------------------------------------------------------------------------------------
case('none_no_rows', 0, 5, 3, route('NONE'))
case('scale_k0', 150, 70, 0, route('SCALE'))
case('tall_2048_240', 2048, 240, 2048, route('TALL'), pad=(5, 6, 2))
case('gemv_256_8_256', 256, 8, 256, route('GEMV'))
case('panel_k128', 100, 300, 128, route('PANEL'))
# ---- panel borders: K 128 / 129, M or N 128 / 129, batch 4 / 5, transposed B ---------------------------------------------------
case('panel_k129', 100, 300, 129, route(T64))                           # t128 = 3 < 512, K < 512
case('panel_m128', 128, 300, 100, route('PANEL'))
case('panel_m129_n128', 129, 128, 100, route('PANEL'), ta=True)         # thin in N instead
case('panel_m129_n129', 129, 129, 100, route(T64))
case('panel_batch4', 100, 300, 64, route('PANEL'), batch=4, covers=('batch>2',))
case('panel_batch5', 100, 300, 64, route(T64), batch=5, covers=('batch>2',))        # t128 = 3 * 5
case('panel_tb', 100, 300, 64, route(T64), tb=True)
case('panel_a_lower', 128, 300, 128, route('PANEL', a_lower=True), ta=True, flags=A_LOWER, covers=('a_lower',))     # U12 = U11^-T A12
case('panel_b_upper', 300, 100, 100, route('PANEL', b_upper=True), flags=B_UPPER, covers=('b_upper',))
case('panel_a_upper', 100, 300, 100, route('PANEL'), flags=A_UPPER)                 # no shortcut for this side: full K range
case('panel_b_lower', 300, 100, 100, route('PANEL'), flags=B_LOWER)
case('panel_upper_only', 128, 128, 64, route('PANEL'), flags=UPPER_ONLY, covers=('upper_only',))
case('panel_upper_only_300', 300, 300, 100, route(T64), flags=UPPER_ONLY, tb=True)              # neither M nor N <= 128
# ---- gemv borders: M and K 255 / 256, N 8 / 9, transposes, triangular A ----------------------------------------------------------
case('gemv_m255', 255, 8, 256, route(T64))                              # t64 = 4, K < 512: not split
case('gemv_k255', 256, 8, 255, route(T64))
case('gemv_n9', 256, 9, 256, route(T64))
case('gemv_n1_k1681', 1681, 1, 1681, route('GEMV'))                     # backward sweep of the smoother
case('gemv_ta', 1681, 1, 1681, route(T128, slices=12, chunk=144), ta=True, covers=('splitk1',))
#   forward sweep: t64 = 27 < 256 -> 128-tiles, 14 of them: min(16, 1681 / 128 = 13, 512 / 14) = 13 asked, chunk = round16(130) = 144 -> 12 slices
case('gemv_a_upper', 300, 3, 300, route('GEMV'), flags=A_UPPER, covers=('tri_gemv',))
case('gemv_a_lower', 300, 3, 300, route('GEMV'), flags=A_LOWER, covers=('tri_gemv',))
case('gemv_batch2', 300, 3, 1681, route(T128, slices=12, chunk=144), batch=2, covers=('splitk2',))
#   t64 = 5 * 2 = 10 < 256; gx x gy = 1 x 3, tiles = 6: min(16, 13, 85) = 13 slices asked, chunk 144, 12 slices
# ---- tall kernel borders (M = K = 2048): N 176 / 178 / 240 / 242, odd N, odd ldb, B off 16-byte alignment, M and K 2047 ---------
#   not tall: t64 = 3 or 4 x 32 <= 128 < 256 -> 128-tiles, 2 x 16 = 32 of them, min(16, 2048 / 128, 512 / 32) = 16 slices of 128
case('tall_n176', 2048, 176, 2048, route(T128, slices=16, chunk=128), covers=('splitk1',))
case('tall_n178', 2048, 178, 2048, route('TALL'))
case('tall_n242', 2048, 242, 2048, route(T128, slices=16, chunk=128))
case('tall_n239_odd', 2048, 239, 2048, route(T128, slices=16, chunk=128))
case('tall_odd_ldb', 2048, 240, 2048, route(T128, slices=16, chunk=128), pad=(0, 1, 2))
case('tall_b_misaligned', 2048, 240, 2048, route(T128, slices=16, chunk=128), pad=(0, 2, 2), b_offset=1)
case('tall_m2047', 2047, 240, 2048, route(T128, slices=16, chunk=128))
case('tall_k2047', 2048, 240, 2047, route(T128, slices=15, chunk=144))          # 2047 / 128 = 15 slices asked: round16(137) = 144, 15 slices
case('tall_ragged', 2176, 238, 2063, route('TALL'), pad=(5, 6, 2))
# ---- 128-tiles by count: t128 511 / 512 ------------------------------------------------------------------------------------------
case('work_tiles_511', 769, 9217, 16, route(T64))                       # 7 x 73
case('work_tiles_512', 897, 8065, 16, route(T128))                      # 8 x 64
# ---- split candidates: t64 255 / 256, K 511 / 512 ----------------------------------------------------------------------------------
case('tiles64_255', 960, 1088, 512, route(T128, slices=4, chunk=128))   # 15 x 17; 128-tiles 8 x 9 = 72: min(16, 4, 7) = 4
case('tiles64_256', 1024, 1024, 512, route(T64))
case('splitk_k511', 960, 1088, 511, route(T64))
# ---- row-strip order: gx 1 / 2 / 8 / 9, gy 31 / 32, a padded strip grid, strips together with split-K ------------------------------
case('strips_gx1', 2048, 64, 130, route(T64))
case('strips_gx2', 2048, 65, 130, route(T64, strips=True), covers=('strips',))
case('strips_gx8', 2048, 512, 130, route(T64, strips=True))
case('strips_gx9', 2048, 513, 130, route(T64))
case('strips_gy31', 1984, 512, 130, route(T64))
case('strips_gy32', 1985, 512, 130, route(T64, strips=True))
case('strips_gy33_padded', 2049, 200, 130, route(T64, strips=True), ta=True)      # 33 row tiles in a grid padded to 40
case('strips_splitk', 3969, 200, 512, route(T128, slices=4, chunk=128, strips=True), tb=True)
#   t64 = 4 x 63 = 252 < 256 -> 128-tiles 2 x 32, strip grid 8 * 2 * 4 = 64 workgroups: min(16, 4, 8) = 4 slices
case('strips_batch2', 2048, 512, 130, route(T64), batch=2)              # strips are for single products
# ---- tail split (K >= 2048, at most 8 column tiles of 64, rows beyond the whole rounds of 768 workgroup slots) -----------------------
case('tail_768_tiles', 6144, 512, 2048, route(T64, strips=True))        # 8 x 96: one whole round, no rows remain
case('tail_769_tiles', 49153, 9, 2048, route(T64, m_main=49152, rest={'kind': T128, 'slices': 16, 'strips': False}), covers=('tail',))
#   1 x 769 tiles: 768 rows of tiles, then ONE row of the matrix: t64 = 1 -> 128-tile split 16 x 128
case('tail_770_tiles', 6977, 400, 2048, route(T64, strips=True, m_main=6976, rest={'kind': T128, 'slices': 16, 'strips': False}), covers=('tail',))
#   7 x 110 tiles, rows_per_round = 109: main 6976 rows (t128 = 4 x 55, strips 7 x 109), rest 1 row: t64 = 7, 4 128-tiles -> 16 slices
case('tail_rest_half', 9216, 512, 2048, route(T64, strips=True, m_main=6144, rest={'kind': T64, 'slices': 1, 'strips': True}), covers=('tail',))
#   8 x 144, rows_per_round = 96, rest = 48 = half a round; the rest has t64 = 384 >= 256: 64-tiles in strips 8 x 48
case('tail_rest_over_half', 9280, 512, 2048, route(T64, strips=True))   # rest = 49 rows of tiles: not split
case('tail_col_tiles_9', 5504, 576, 2048, route(T64))                   # 9 x 86 = 774 tiles, but nine column tiles
case('tail_k2047', 6977, 400, 2047, route(T64, strips=True))
case('tail_ta', 6977, 400, 2048, route(T64, strips=True), ta=True)
# ---- narrow: at most 64 rows, t128 >= 512 ----------------------------------------------------------------------------------------
case('narrow_m64', 64, 65409, 130, route(T64), covers=('narrow',))      # t128 = 512, t64 = 1023
case('narrow_m65', 65, 65409, 130, route(T128))
# ---- upper tiles only ------------------------------------------------------------------------------------------------------------
case('upper_only_tile64', 700, 700, 200, route(T64), tb=True, flags=UPPER_ONLY, covers=('upper_only',))             # (36 + 6) / 2 tiles
case('upper_only_tile64_b3', 2300, 2300, 40, route(T64), ta=True, batch=3, flags=UPPER_ONLY)                        # (18^2 * 3 + 18) / 2 = 495
case('upper_only_tile128_b3', 2305, 2305, 40, route(T128), ta=True, batch=3, flags=UPPER_ONLY, covers=('upper_only', 'batch>2'))    # (19^2 * 3 + 19) / 2 = 551
case('upper_only_no_split', 128, 128, 1024, route(T64), flags=UPPER_ONLY, ta=True)                                  # upper_only products are never split
# ---- triangular operands in the tiled kernel (K ranges per tile) -----------------------------------------------------------------
case('tri_a_upper', 300, 200, 300, route(T64), flags=A_UPPER)
case('tri_a_lower_ta', 300, 200, 300, route(T64), ta=True, flags=A_LOWER)
case('tri_b_upper', 200, 300, 300, route(T64), flags=B_UPPER)
case('tri_b_lower_tb', 200, 300, 300, route(T64), tb=True, flags=B_LOWER)
case('tri_uinv_uinvt', 500, 500, 500, route(T64), tb=True, flags=A_UPPER | B_LOWER | UPPER_ONLY)                   # Z = U^-1 U^-T of the sparse inverse
case('tri_batch8_tile128', 1000, 1000, 1000, route(T128), batch=8, flags=A_UPPER, repeat='A', covers=('batch>2',))  # t128 = 64 * 8
case('tri_splitk', 600, 9, 600, route(T128, slices=4, chunk=160), flags=A_UPPER)
#   t64 = 10 < 256 -> 128-tiles 1 x 5: min(16, 600 / 128 = 4, 102) = 4, chunk = round16(150) = 160 (the split launch drops the K ranges)
case('batch3_no_split', 300, 3, 1681, route(T64), batch=3, covers=('batch>2',))
# ---- in place ----------------------------------------------------------------------------------------------------------------------
case('inplace_b_panel', 128, 300, 128, route('PANEL', a_lower=False, alias='B'), ta=True, inplace='B', covers=('inplace',))
case('inplace_b_panel_batch2', 100, 333, 100, route('PANEL', alias='B'), ta=True, batch=2, inplace='B', pad=(0, 5, 0))
case('inplace_b_tile128', 100, 700, 100, route(T128, alias='B'), batch=5, inplace='B', repeat='A', covers=('inplace', 'batch>2'))     # batch > 4: not the panel kernel
case('inplace_b_tb_free_a', 128, 128, 128, route(T128, alias='B'), tb=False, ta=False, inplace='B', batch=6)
case('inplace_a_tile128', 300, 100, 100, route(T128, alias='A'), inplace='A', covers=('inplace',))
case('inplace_a_tb', 700, 128, 128, route(T128, alias='A'), tb=True, inplace='A', pad=(4, 0, 0))

# ---- argument and aliasing rules: (name, changes to a base case, fragment of the message) --------------------------------------
REFUSED = [
    ('two_bits_a', dict(base='tri_a_upper', flags=A_UPPER | A_LOWER), 'op(A) cannot be upper and lower'),
    ('two_bits_b', dict(base='tri_b_upper', flags=B_UPPER | B_LOWER), 'op(B) cannot be upper and lower'),
    ('tri_a_not_square', dict(base='tri_b_upper', flags=A_UPPER), 'triangular op(A) needs M == K'),
    ('tri_b_not_square', dict(base='tri_a_upper', flags=B_LOWER), 'triangular op(B) needs K == N'),
    ('upper_only_not_square', dict(base='tri_a_upper', flags=UPPER_ONLY), 'upper_only needs M == N'),
    ('unknown_flag', dict(base='panel_k128', flags=32), 'unknown flag bits'),
    ('negative_batch', dict(base='panel_k128', batch=-1), 'negative dimension'),
    ('inplace_b_transposed', dict(base='inplace_b_tb_free_a', tb=True), 'overwrite B only where'),
    ('inplace_b_two_row_tiles', dict(base='inplace_b_panel', M=129, K=129), 'overwrite B only where'),
    ('inplace_b_not_square', dict(base='inplace_b_panel', M=100, K=128, ta=True), 'overwrite B only where'),
    ('inplace_a_transposed', dict(base='inplace_a_tile128', ta=True, M=100), 'overwrite A only where'),
    ('inplace_a_two_column_tiles', dict(base='inplace_a_tile128', N=129, K=129), 'overwrite A only where'),
]

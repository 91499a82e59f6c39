"""
The routing decision of the dense fp64 product (shg_gemm_route: host logic only, no GPU) against the table of
tests/gemm_route_cases.py: every route kind of include/shg.h and every modifier has a case, every threshold of the dispatcher has a
shape on each side, and the argument and aliasing rules of shg_gemm / shg_gemm_ex answer SHG_ERR_INVALID before any HIP call.
A threshold that moves makes the case that names its border fail here, instead of moving a GPU test onto another kernel unnoticed.
"""
import ctypes
import os
import re

import pytest

import gemm_route_cases as rc
from conftest import ROOT
from grates_amd import _lib, engine

# stand-in addresses (nothing is read): 256-byte aligned like device allocations, B moved by the case's offset
A_PTR, B_PTR, C_PTR = 0x7f1000000000, 0x7f2000000000, 0x7f3000000000


def pointers(c):
    b = B_PTR + 8 * c['b_offset']
    return A_PTR, b, {'': C_PTR, 'A': A_PTR, 'B': b}[c['inplace']]


def header_route_kinds():
    text = open(os.path.join(ROOT, 'include', 'shg.h')).read()
    body = re.search(r'typedef enum \{([^}]*)\} shg_gemm_route_kind;', text).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    return {name: int(value) for name, value in re.findall(r'SHG_GEMM_ROUTE_([A-Z0-9]+)\s*=\s*(\d+)', body)}


@pytest.mark.parametrize('name', list(rc.CASES))
def test_route_of_case(name):
    c = rc.CASES[name]
    got = engine.gemm_route(*rc.route_arguments(c, *pointers(c)))
    assert got == c['expect'], 'case {0}: route {1}, the table expects {2}'.format(name, got, c['expect'])


def test_every_route_kind_and_modifier_has_a_case():
    kinds = header_route_kinds()
    assert len(kinds) >= 7 and [k for k, _ in sorted(kinds.items(), key=lambda kv: kv[1])] == list(engine.GEMM_ROUTE_KINDS)
    seen = {c['expect']['kind'] for c in rc.CASES.values()} | {c['expect']['rest']['kind'] for c in rc.CASES.values() if c['expect']['rest']}
    assert seen == set(kinds), 'route kinds without a case: {0}'.format(sorted(set(kinds) - seen))
    covered = {m for c in rc.CASES.values() for m in c['covers']}
    assert covered == set(rc.MODIFIERS), 'modifiers without a case: {0}'.format(sorted(set(rc.MODIFIERS) - covered))
    # a case stands for a modifier only if its arguments and its route really show it
    shows = {'splitk1': lambda c, e: c['batch'] == 1 and e['slices'] > 1 and e['chunk'] > 0,
             'splitk2': lambda c, e: c['batch'] == 2 and e['slices'] > 1,
             'strips': lambda c, e: e['strips'],
             'tail': lambda c, e: e['m_main'] > 0 and e['rest'] is not None,
             'a_lower': lambda c, e: e['kind'] == 'PANEL' and e['a_lower'],
             'b_upper': lambda c, e: e['kind'] == 'PANEL' and e['b_upper'],
             'tri_gemv': lambda c, e: e['kind'] == 'GEMV' and c['flags'] & 3,
             'upper_only': lambda c, e: c['flags'] & rc.UPPER_ONLY,
             'batch>2': lambda c, e: c['batch'] > 2,
             'narrow': lambda c, e: e['kind'] == 'TILE64' and c['M'] <= 64 and -(-c['N'] // 128) * c['batch'] >= 512,
             'inplace': lambda c, e: c['inplace'] and e['alias'] == c['inplace']}
    for c in rc.CASES.values():
        for m in c['covers']:
            assert shows[m](c, c['expect']), 'case {0} does not show {1}'.format(c['name'], m)
    # both doors are in the table, and shg_gemm's cases are plain products
    assert any(c['door'] == 'both' for c in rc.CASES.values())
    assert all(c['batch'] == 1 and c['flags'] == 0 and not c['inplace'] for c in rc.CASES.values() if c['door'] == 'both')


def refused_arguments(spec):
    changes = dict(spec)
    c = dict(rc.CASES[changes.pop('base')])
    c.update(changes)
    return c


@pytest.mark.parametrize('name,spec,message', rc.REFUSED, ids=[r[0] for r in rc.REFUSED])
def test_refused_arguments(name, spec, message):
    """shg_gemm_route and shg_gemm_ex apply the same rules, both before any HIP call (there is no GPU here)."""
    lib = _lib.load()
    c = refused_arguments(spec)
    ta, tb, M, N, K, a, lda, sa, b, ldb, sb, out, ldc, sc, batch, flags = rc.route_arguments(c, *pointers(c))
    with pytest.raises(_lib.ShgError) as err:
        engine.gemm_route(ta, tb, M, N, K, a, lda, sa, b, ldb, sb, out, ldc, sc, batch, flags)
    assert err.value.status == -1 and message in str(err.value)
    p = ctypes.c_void_p
    assert lib.shg_gemm_ex(int(ta), int(tb), M, N, K, 1.0, p(a), lda, sa, p(b), ldb, sb, 0.0, p(out), ldc, sc, batch, flags, None) == -1
    assert message in lib.shg_last_error().decode() and 'shg_gemm_ex' in lib.shg_last_error().decode()


def test_argument_rules_of_both_doors():
    lib = _lib.load()
    p = ctypes.c_void_p
    a, b, c = p(A_PTR), p(B_PTR), p(C_PTR)
    error = lambda: lib.shg_last_error().decode()      # noqa: E731
    # shg_gemm: in-place forms other than the two supported ones (M = K = 100 rows of B overwritten: fine; 200 rows: refused)
    assert lib.shg_gemm(0, 0, 200, 50, 200, 1.0, a, 200, b, 50, 0.0, b, 50, None) == -1 and 'shg_gemm: the output may overwrite B only where' in error()
    assert lib.shg_gemm(0, 1, 50, 50, 50, 1.0, a, 50, b, 50, 0.0, b, 50, None) == -1 and 'overwrite B' in error()
    assert lib.shg_gemm(0, 0, 100, 50, 100, 1.0, a, 100, b, 50, 0.0, b, 51, None) == -1 and 'overwrite B' in error()        # ldc != ldb
    assert lib.shg_gemm(1, 0, 50, 50, 50, 1.0, a, 50, b, 50, 0.0, a, 50, None) == -1 and 'overwrite A' in error()
    assert lib.shg_gemm(0, 0, 200, 200, 200, 1.0, a, 200, b, 200, 0.0, a, 200, None) == -1 and 'overwrite A' in error()
    # shg_gemm_ex: strides, pointers, leading dimensions
    ex = lambda *args: lib.shg_gemm_ex(*args, None)    # noqa: E731
    assert ex(0, 0, 10, 10, 10, 1.0, a, 10, -1, b, 10, 0, 0.0, c, 10, 0, 1, 0) == -1 and 'negative stride' in error()
    assert ex(0, 0, 10, 10, 10, 1.0, a, 10, 100, b, 10, 100, 0.0, c, 10, 0, 2, 0) == -1 and 'strideC > 0' in error()
    assert ex(0, 0, 10, 10, 10, 1.0, None, 10, 0, b, 10, 0, 0.0, c, 10, 0, 1, 0) == -1 and 'NULL pointer' in error()
    assert ex(0, 0, 10, 10, 10, 1.0, a, 10, 0, b, 10, 0, 0.0, None, 10, 0, 1, 0) == -1 and 'bad output' in error()
    assert ex(0, 0, 10, 10, 10, 1.0, a, 9, 0, b, 10, 0, 0.0, c, 10, 0, 1, 0) == -1 and 'leading dimension too small' in error()
    assert ex(1, 1, 10, 12, 14, 1.0, a, 10, 0, b, 13, 0, 0.0, c, 12, 0, 1, 0) == -1 and 'leading dimension too small' in error()
    assert ex(0, 0, 10, 10, 10, 1.0, a, 10, 0, b, 10, 0, 0.0, c, 9, 0, 1, 0) == -1 and 'bad output' in error()
    assert ex(0, 0, 200, 50, 200, 1.0, a, 200, 0, b, 50, 0, 0.0, b, 50, 0, 1, 0) == -1 and 'shg_gemm_ex: the output may overwrite B' in error()
    assert ex(0, 0, 100, 50, 100, 1.0, a, 100, 0, b, 50, 5000, 0.0, b, 50, 6000, 2, 0) == -1 and 'overwrite B' in error()      # strideC != strideB
    # nothing to do: no pointer is looked at and no HIP call is made
    assert ex(0, 0, 0, 10, 10, 1.0, None, 10, 0, None, 10, 0, 0.0, None, 10, 0, 1, 0) == 0
    assert ex(0, 0, 10, 10, 10, 1.0, None, 10, 0, None, 10, 0, 0.0, None, 10, 0, 0, 0) == 0
    which = (ctypes.c_int64 * 8)()
    assert lib.shg_gemm_route(0, 0, 10, 10, 10, 1.0, a, 10, 0, b, 10, 0, 0.0, c, 10, 0, 1, 0, None) == -1 and 'NULL result' in error()
    assert lib.shg_gemm_route(0, 0, 10, 0, 10, 1.0, None, 10, 0, None, 10, 0, 0.0, None, 10, 0, 1, 0, which) == 0 and which[0] == 0


def test_blocks_of_one_matrix_are_separate_operands():
    """Interleaved blocks of one allocation (test_gemm_alpha_beta_and_views) do not start at the output's address: routed, not refused."""
    base, ld = A_PTR, 400
    at = lambda i, j: base + 8 * (i * ld + j)          # noqa: E731
    got = engine.gemm_route(False, False, 130, 70, 90, at(10, 5), ld, 0, at(200, 300), ld, 0, at(150, 100), ld, 0)
    assert got['kind'] == 'PANEL' and got['alias'] == ''

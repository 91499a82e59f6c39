"""
Every transform and operator branch of csrc/analysis.hip at its seams, against the long-double reference of ALL orders
(tests/analysis_reference.py; its own spread against the oracle is at most 2.4e-14, tests/test_analysis_reference_cpu.py).

    analysis_transform_kernel<MT, ROWW>   MT = 2 | 3 | 4 for N <= 64 | 96 | 126, row-constant and varying weights, odd quarter domains
    fold kernel + GEMMs (N >= 127), weight transpose + GEMM (meridians without the four-fold symmetry)
    operator product: parity split | analysis_operator_kernel | gemm_ex + analysis_scatter_kernel (R > 128 or odd nlat)
    operator builder: factor_invert_batched up to R = 128, the potrf_upper / trtri_upper loop beyond
    analysis_pass: the second pass of B > 256 epochs (b0 = 256), several epoch groups with a partial last one
    analysis_matrix_kernel at a degree where slots span more than one row tile

Every case compares every entry of every epoch: max |got - ref| / max |ref| < TOL, the tolerance of tests/test_gpu_analysis.py
(the normal matrices of these grids are well conditioned: two decades above the reference's spread).  The preconditions that
select a branch (four-fold symmetry, degree range, parity split, R and the parity of nlat) are asserted, so that a change of the
dispatch cannot move a case elsewhere unnoticed.  With B = 3 the 64-row workgroups of the transform straddle epochs and end in a
partial block on every grid but 128 x 256 (the grid without any tail).  Each figure is printed before it is asserted (pytest -s).

Measured on the MI355X (max |got - ref| / max |ref| over all epochs; the file takes 6 s):
    d/o  64, 66 x 132    const 6.3e-15, varying 7.7e-15        d/o 127 from 4, 130 x 256   varying 1.5e-14
    d/o  65, 67 x 132    const 9.4e-15, varying 6.2e-15        d/o 128, 130 x 260          const 1.3e-14, varying 1.7e-14
    d/o  96 from 3, 98 x 196   const 1.1e-14, varying 1.1e-14  d/o 128 from 2, 130 x 259   varying 1.1e-14
    d/o  97 from 2, 100 x 196  const 1.1e-14, varying 1.2e-14  d/o 65, 67 x 132 shifted    varying 3.8e-15
    d/o 126, 128 x 256   const 1.5e-14, varying 1.4e-14        d/o 20 from 20, 24 x 44     const 4.3e-15
    d/o 12 from 1, 300 and 257 epochs: 16 x 28 1.9e-15, 18 x 28 2.5e-15, 17 x 28 1.9e-15, 18 x 28 shifted 1.7e-15
    d/o 33 from 2, 36 x 68: F @ v against analysis(v) 4.1e-15, against the reference 5.0e-15; analysis 3.7e-15 | 3.4e-15
A library whose MT = 4 transform has the sign of one fold combination swapped fails the four d/o 97 and d/o 126 cases with errors
of 1.4 ... 1.7 while tests/test_gpu_analysis.py and tests/test_gpu_edge_cases.py pass on it: they never run that kernel.
"""

import numpy as np
import pytest

import grates_amd as ga
import analysis_reference as ar
from oracle import shg_oracle as orc

pytestmark = pytest.mark.gpu
TOL = 1e-12


def make_plan(case):
    colat, _, kn = ga.gravityfield.surface_factors(ga.kernel.get_kernel('potential'), case.N, case.parallels(), ar.GM, ar.R,
                                                   orc.GRS80_A, orc.GRS80_F)
    return ga.engine.Plan(case.N, colat, kn, case.meridians())


def worst(got, ref):
    """max over the epochs of max |got - ref| / max |ref| (per epoch, every entry)"""
    return max(float(np.max(np.abs(g - r)) / np.max(np.abs(r))) for g, r in zip(got, ref))


def check_branch(case, plan):
    """the preconditions that select the case's transform and operator product (csrc/analysis.hip: longitude_transform,
    launch_fused_transform, build_parity_operator, analysis_pass)"""
    N, nlat, nlon = case.N, case.nlat, case.nlon
    info = plan.info()
    assert (info['max_degree'], info['nlat'], info['nlon']) == (N, nlat, nlon)
    assert info['fourfold_symmetry'] is case.fourfold, case.id
    lo, hi = ar.TRANSFORM_DEGREES[case.transform]
    assert lo <= N <= hi, case.id
    area = case.area()
    assert bool(np.all(area == area[:, :1])) is (case.kind == 'const')                   # ROWW of the fused kernel
    split = plan.analysis_info()['parity_split']
    direct = N + 1 <= 128 and nlat % 2 == 0
    if case.product == 'parity':
        assert split is True and direct and nlat % 4 == 0, (case.id, plan.analysis_info())
    elif case.product == 'operator':
        assert split is False and direct, (case.id, plan.analysis_info())
    else:
        assert split is False and not direct, (case.id, plan.analysis_info())


@pytest.mark.parametrize('case', ar.SEAM_CASES, ids=[c.id for c in ar.SEAM_CASES])
def test_degree_and_shape_seams(case):
    N, nmin, B = case.N, case.nmin, 3
    vals, area = case.values(B), case.area()
    plan = make_plan(case)
    assert plan.analysis_info()['parity_split'] is None
    out = ga.engine.to_host(plan.analysis(vals, area, nmin))
    check_branch(case, plan)
    assert out.shape == (B, N + 1, N + 1)
    ref = ar.analysis(vals, area, nmin, N, case.meridians(), case.parallels())
    err = worst(out, ref)
    print('{0}: B = {1}, device against the reference {2:.2e}'.format(case.id, B, err))
    assert err < TOL
    if nmin > 0:
        assert not out[:, :nmin, :nmin].any()                                          # degrees below min_degree: exactly zero
    if nmin == N:                                                                       # one row per slot: nothing else is written
        assert np.array_equal(out != 0.0, np.broadcast_to(ar.order_mask(N, nmin, range(N + 1)), out.shape))


@pytest.mark.parametrize('B', [300, 257])
@pytest.mark.parametrize('case', ar.BATCH_CASES, ids=[c.id for c in ar.BATCH_CASES])
def test_batch_seams(case, B):
    """B = 300: the first pass takes 256 epochs in four full groups of 64, the second 44 epochs (one partial group) at b0 = 256;
    B = 257: a second pass of a single epoch.  The epochs of the second pass are those of a call of their own: bitwise on the
    parity-split grid (the launches are the same), to TOL elsewhere."""
    import torch
    N, nmin = case.N, case.nmin
    vals, area = case.values(B), case.area()
    plan = make_plan(case)
    dvals = ga.engine.to_device(vals)
    long_call = plan.analysis(dvals, area, nmin)
    check_branch(case, plan)
    out = ga.engine.to_host(long_call)
    assert out.shape == (B, N + 1, N + 1)
    ref = ar.analysis(vals, area, nmin, N, case.meridians(), case.parallels())
    err = worst(out, ref)
    first, second = worst(out[:256], ref[:256]), worst(out[256:], ref[256:])
    print('{0}: B = {1}, device against the reference {2:.2e} (first pass {3:.2e}, second pass {4:.2e})'.format(case.id, B, err, first, second))
    assert err < TOL
    assert not out[:, :nmin, :nmin].any()
    tail = plan.analysis(dvals[256:B], area, nmin)
    if case.product == 'parity':
        assert torch.equal(tail, long_call[256:])
    else:
        assert worst(ga.engine.to_host(tail), out[256:]) < TOL
    assert worst(ga.engine.to_host(tail), ref[256:]) < TOL


def test_dense_operator():
    """analysis_matrix at d/o 33 from degree 2 on 36 x 68 (1152 x 2448 entries, three row tiles in the low orders): F @ v is the
    analysis of v, and the operators it rebuilt for other weights do not leak into the next analysis call."""
    import torch
    const, varying = ar.DENSE_CASES
    N, nmin, B = varying.N, varying.nmin, 3
    vals = varying.values(B)
    mer, par = varying.meridians(), varying.parallels()
    plan = make_plan(varying)
    ref_const = ar.analysis(vals, const.area(), nmin, N, mer, par)
    ref_varying = ar.analysis(vals, varying.area(), nmin, N, mer, par)
    dvals = ga.engine.to_device(vals)

    before = ga.engine.to_host(plan.analysis(dvals, const.area(), nmin))                # operators of the row-constant weights
    check_branch(const, plan)
    err = worst(before, ref_const)
    print('{0}: device against the reference {1:.2e}'.format(const.id, err))
    assert err < TOL

    F = plan.analysis_matrix(varying.area(), nmin)                                      # rebuilds them for the varying weights
    assert tuple(F.shape) == ((N + 1) ** 2 - nmin ** 2, varying.nlat * varying.nlon) == (1152, 2448)
    check_branch(varying, plan)
    direct = plan.analysis(dvals, varying.area(), nmin)
    check_branch(varying, plan)
    product = F @ dvals.reshape(B, -1).T                                                # [P, B] on the device
    host_direct, host_product = ga.engine.to_host(direct), ga.engine.to_host(product)
    for e in range(B):
        want = orc.ravel_coefficients(host_direct[e], nmin, N)
        err_direct = float(np.max(np.abs(host_product[:, e] - want)) / np.max(np.abs(want)))
        want = orc.ravel_coefficients(ref_varying[e], nmin, N)
        err_ref = float(np.max(np.abs(host_product[:, e] - want)) / np.max(np.abs(want)))
        print('{0}: epoch {1}, F @ v against analysis(v) {2:.2e}, against the reference {3:.2e}'.format(varying.id, e, err_direct, err_ref))
        assert err_direct < TOL and err_ref < TOL
    err = worst(host_direct, ref_varying)
    print('{0}: device against the reference {1:.2e}'.format(varying.id, err))
    assert err < TOL and not host_direct[:, :nmin, :nmin].any()
    assert torch.isfinite(F).all()

    after = ga.engine.to_host(plan.analysis(dvals, const.area(), nmin))                 # back to the row-constant weights
    check_branch(const, plan)
    err = worst(after, ref_const)
    print('{0}: after analysis_matrix, device against the reference {1:.2e}'.format(const.id, err))
    assert err < TOL
    assert np.array_equal(after, before)

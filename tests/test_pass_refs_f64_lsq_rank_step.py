"""CPU tests of tests/pass_refs_f64_lsq_rank_step.py: the numpy model of the CholeskyQR step and of the whole rank-aware solve with it,
on the seven cases of tests/pass_refs_f64_lsq_rank.py and on an R0 as a model of the R-only ladder leaves it
(tools/lstsq_rank_contraction.ladder_r0_model).  With the step every case is inside pass_refs_f64_lsq_rank.check at refine = 1; with the
step left out the copied interior column at 4096 x 16 is not -- the check the device entry is held to can tell the two apart."""
import numpy as np
import pytest

from tests import pass_refs_f64_lsq_rank as pk
from tests import pass_refs_f64_lsq_rank_step as ps
from tools import lstsq_rank_contraction as lc

_r0 = {}


def ladder_r0(name):
    if name not in _r0:
        _r0[name] = lc.ladder_r0_model(np.array(pk.case_matrix(name)))[0]
    return _r0[name]


@pytest.mark.parametrize("kind", pk.RHS_KINDS)
@pytest.mark.parametrize("case", pk.CASES, ids=[c[0] for c in pk.CASES])
def test_model_with_the_step_is_inside_the_bound(case, kind):
    name, m, n, _, rcond, k_expected = case[:6]
    a, b = np.array(pk.case_matrix(name)), np.array(pk.case_rhs(name, kind))
    x, r, p, k, z = ps.model_lstsq_rank_step(a, b, pk.rcond_of(rcond, m, n), refine=1, r0=ladder_r0(name))
    f = pk.check(name, kind, x, p, k)
    print("%-16s %-10s err %.2e lapack %.2e bound %.2e" % (name, kind, f["err"], f["lapack"], f["bound"]))
    assert pk.structure_ok(z, p, k, n)


@pytest.mark.parametrize("kind", pk.RHS_KINDS)
def test_step_left_out_misses_the_bound_on_the_copied_column(kind):
    name, m, n, _, rcond = pk.CASES[0][:5]
    assert name == "copied_4096x16"
    a, b = np.array(pk.case_matrix(name)), np.array(pk.case_rhs(name, kind))
    x, r, p, k, _ = ps.model_lstsq_rank_step(a, b, pk.rcond_of(rcond, m, n), refine=1, defect="left_out", r0=ladder_r0(name))
    f = pk.figures(name, kind, x, p, k)
    assert k == 15 and f["zero_rows"]
    if kind == "gaussian":
        assert f["err"] > 100.0 * f["bound"], f
        with pytest.raises(AssertionError):
            pk.check(name, kind, x, p, k)


@pytest.mark.parametrize("n,k", ps.STEP_SHAPES)
@pytest.mark.parametrize("eps", ps.STEP_EPS)
def test_step_model_orthonormalises_and_keeps_the_zero_structure(n, k, eps):
    zeff, g1, p, r11, qtq = ps.step_case(n, k, eps)
    zout, verdict = ps.step_of(zeff, g1, k)
    assert verdict == 0 and pk.structure_ok(zout, p, k, n)
    res, allow = ps.step_residual(zout, p, k, r11, qtq), ps.step_allowance(zeff, g1, p, k, r11, qtq)
    assert res <= allow, (n, k, eps, res, allow)
    if eps == 2e-2 and k > 1:
        before = ps.step_residual(zeff, p, k, r11, qtq)
        assert before > 1e-3 and before > 1e6 * res, "the case does not need the step"
    # the measure can tell a wrong step: the transposed inverse, and a non-zero in a zero row
    if k > 1 and eps > 0:
        bad, _ = ps.step_of(zeff, g1, k, defect="transposed")
        assert ps.step_residual(bad, p, k, r11, qtq) > allow or not pk.structure_ok(bad, p, k, n)
    if k < n:
        bad, _ = ps.step_of(zeff, g1, k, defect="dense_rows")
        assert not pk.structure_ok(bad, p, k, n)


def test_step_model_verdicts():
    zeff, g1, p, r11, qtq = ps.step_case(16, 15, 1e-8)
    z0, v0 = ps.step_of(zeff, g1, 0)
    assert v0 == 0 and not z0.any()
    g_bad = g1.copy()
    g_bad[7, 7] = -1.0
    zb, vb = ps.step_of(zeff, g_bad, 15)
    assert vb == 1 and not zb.any()
    g_nan = g1.copy()
    g_nan[0, 0] = np.nan
    assert ps.step_of(zeff, g_nan, 15)[1] == 1


def test_pack_g_is_the_tile_layout_the_kernel_reads():
    """entry (i, j), i <= j, of tile pair (i >> 4, j >> 4) at idx * 256 + ((i & 15) >> 2) * 64 + (i & 3) * 16 + (j & 15), the pairs
    (ti <= tj) in row order: the index arithmetic of lsq_rank_step_f64_kernel"""
    n = 51
    g = np.arange(n * n, dtype=np.float64).reshape(n, n)
    g = np.triu(g) + np.triu(g, 1).T
    v = ps.pack_g(g, n)
    nt = 4
    for i, j in ((0, 0), (3, 50), (17, 18), (33, 47), (50, 50), (15, 16), (31, 32)):
        ti, tj, ri = i >> 4, j >> 4, i & 15
        idx = ti * nt - (ti * (ti - 1)) // 2 + (tj - ti)
        assert v[idx * 256 + (ri >> 2) * 64 + (ri & 3) * 16 + (j & 15)] == g[i, j]

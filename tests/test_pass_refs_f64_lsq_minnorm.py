"""CPU tests of tests/pass_refs_f64_lsq_minnorm.py: the numpy model of the minimum-norm rank-aware solve on the seven cases of
tests/pass_refs_f64_lsq_rank.py with both kinds of right-hand side, on an R0 as a model of the R-only ladder leaves it
(tools/lstsq_rank_contraction.ladder_r0_model), held to rel_err(X, X*) <= max(2 x LAPACK's, floor_of(n)) at refine = 1 against the
extended-precision minimum-norm solution of the truncated problem; LAPACK's dgelsy on the whole A as a second opinion on X*; the
defects the check must catch; the model of the update factor on the shapes of the kernel's GPU test."""
import numpy as np
import pytest

from tests import pass_refs_f64_lsq as pl
from tests import pass_refs_f64_lsq_minnorm as pm
from tests import pass_refs_f64_lsq_rank as pk
from tests import pass_refs_f64_lsq_rank_step as ps
from tests.test_pass_refs_f64_lsq_rank_step import ladder_r0

IDS = [c[0] for c in pk.CASES]


def run(name, kind, r0=None, **kw):
    _, m, n, _, rcond = next(c[:5] for c in pk.CASES if c[0] == name)
    a, b = np.array(pk.case_matrix(name)), np.array(pk.case_rhs(name, kind))
    return pm.model_lstsq_minnorm(a, b, pk.rcond_of(rcond, m, n), r0=ladder_r0(name) if r0 is None else r0, **kw)


def perturbed_r0():
    """the ladder's R0 of copied_4096x16 with 1e-10 |R0| of noise on its columns 11 .. 15, the copied column and those behind it: what
    a ladder that never stores Q may leave there.  It is a hundredth of rcond = 1e-8, so the rank decision stands."""
    r0 = np.array(ladder_r0("copied_4096x16"))
    rng = np.random.default_rng(11)
    r0[:, 11:] += 1e-10 * np.abs(r0).max() * np.triu(rng.standard_normal(r0.shape))[:, 11:]
    return r0


@pytest.mark.parametrize("kind", pk.RHS_KINDS)
@pytest.mark.parametrize("case", pk.CASES, ids=IDS)
def test_model_is_inside_the_bound(case, kind):
    """refine = 1: all 14 (case, kind) pairs inside the bound; r, p, rank are the basic model's; X is no longer than the basic X and has
    its residual; at full rank it IS the basic X"""
    name, m, n, _, rcond = case[:5]
    x, r, p, k, z, zmn = run(name, kind)
    f = pm.check(name, kind, x, p, k)
    print("%-16s %-10s err %.2e lapack %.2e bound %.2e ratio %.2f" % (name, kind, f["err"], f["lapack"], f["bound"], f["err"] / f["bound"]))
    a, b = np.array(pk.case_matrix(name)), np.array(pk.case_rhs(name, kind))
    xb, rb, pb, kb, zb = ps.model_lstsq_rank_step(a, b, pk.rcond_of(rcond, m, n), refine=1, r0=ladder_r0(name))
    assert kb == k and np.array_equal(pb, p) and np.array_equal(rb, r) and np.array_equal(zb, z)
    assert np.all(np.linalg.norm(x, axis=0) <= np.linalg.norm(xb, axis=0) * (1 + 4 * pk.U))
    if k == n:
        assert np.array_equal(zmn, z) and np.array_equal(x, xb)


@pytest.mark.parametrize("case", pk.CASES, ids=IDS)
def test_reference_agrees_with_gelsy(case):
    """X* against scipy.linalg.lstsq(lapack_driver="gelsy") on the WHOLE A at the case's rcond: the same definition, LAPACK's own
    pivoting.  1e-14 on the six cases with exact rank; on rank 40 of 64 (cond(A P1) = 1e4, a trailing block of 1e-11) the two pivot
    orders truncate slightly different problems: 1e-11 there."""
    import scipy.linalg
    name, m, n, _, rcond = case[:5]
    for kind in pk.RHS_KINDS:
        _, _, p, k, _, _ = run(name, kind)
        ref, _ = pm.yardstick(name, kind, p, k)
        xg = scipy.linalg.lstsq(np.array(pk.case_matrix(name)), np.array(pk.case_rhs(name, kind)), cond=pk.rcond_of(rcond, m, n),
                                lapack_driver="gelsy")[0]
        assert pl.rel_err(xg.reshape(n, -1), ref) <= (1e-11 if name.startswith("rank40") else 1e-14), (name, kind)


def test_norm_on_the_copied_column():
    """the figure of the entry's description: ||X||_F of the minimum-norm solution on copied_4096x16 with a Gaussian B, and rows 4 and
    11 of X equal to rounding"""
    x, _, _, k, _, _ = run("copied_4096x16", "gaussian")
    assert k == 15 and abs(np.linalg.norm(x) - 0.148) < 1e-3
    assert np.all(np.abs(x[4] - x[11]) <= 16 * pk.U * np.abs(x[4]))


def test_sound_model_does_not_depend_on_a_perturbed_r0():
    """G12 comes from A: with perturbed_r0() the model is still inside the bound"""
    for kind in pk.RHS_KINDS:
        x, _, p, k, _, _ = run("copied_4096x16", kind, r0=perturbed_r0())
        pm.check("copied_4096x16", kind, x, p, k)


@pytest.mark.parametrize("defect", ["r12_from_r", "no_perm", "basic"])
def test_defects_miss_the_bound(defect):
    """R12 taken from the pivoted R instead of G12, fed with perturbed_r0(); Zmn without the permutation; the rows M^T V dropped (the
    basic solution): each misses the bound on the copied interior column, by a factor of 100 at least"""
    for kind in pk.RHS_KINDS:
        x, _, p, k, _, _ = run("copied_4096x16", kind, defect=defect, r0=perturbed_r0() if defect == "r12_from_r" else None)
        f = pm.figures("copied_4096x16", kind, x, p, k)
        assert k == 15 and f["err"] > 100.0 * f["bound"], (defect, kind, f)
        with pytest.raises(AssertionError):
            pm.check("copied_4096x16", kind, x, p, k)


def test_no_perm_and_basic_defects_on_another_case():
    for defect in ("no_perm", "basic"):
        x, _, p, k, _, _ = run("tail3_100x7", "gaussian", defect=defect)
        f = pm.figures("tail3_100x7", "gaussian", x, p, k)
        assert f["err"] > 100.0 * f["bound"], (defect, f)


@pytest.mark.parametrize("n,k", pm.FACTOR_SHAPES)
def test_factor_model_on_the_shapes_of_the_kernel_test(n, k):
    """Zmn of the model: the zero structure, S P^T Zmn = I_k and range(P^T Zmn) in range(S^T) within the allowance the kernel is held
    to; Zmn is Zeff bit for bit at k = n and zero at k = 0; the measures can tell the defects"""
    g, zeff, p = pm.factor_case(n, k)
    zmn, verdict = pm.zmn_of(g, zeff, p, k)
    assert verdict == 0 and pm.structure_ok(zmn, k, n)
    if k == 0:
        assert not zmn.any()
        return
    if k == n:
        assert np.array_equal(zmn, zeff)
    s = pm.s_of_inputs(g, zeff, p, k)
    res = pm.factor_residuals(s, zmn, p, k)
    allow, yard, floor = pm.factor_allowance(g, zeff, p, k)
    print("factor model n %2d k %2d: residuals %.2e %.2e, pinv's %.2e %.2e, floor %.2e" % ((n, k) + res + yard + (floor,)))
    assert res[0] <= allow[0] and res[1] <= allow[1], (res, allow)
    if k < n:
        bad, _ = pm.zmn_of(g, zeff, p, k, defect="basic")
        assert pm.factor_residuals(s, bad, p, k)[1] > 1e6 * allow[1]
    if k < n and not np.array_equal(p, np.arange(n)):
        bad, _ = pm.zmn_of(g, zeff, p, k, defect="no_perm")
        r0, r1 = pm.factor_residuals(s, bad, p, k)
        assert r0 > 1e6 * allow[0] or r1 > 1e6 * allow[1]


def test_factor_model_verdicts():
    g, zeff, p = pm.factor_case(16, 15)
    g_bad = g.copy()
    g_bad[7, 7] = -1.0
    zb, vb = pm.zmn_of(g_bad, zeff, p, 15)
    assert vb == 1 and not zb.any()
    g_inf = g.copy()
    g_inf[3, 15] = np.inf
    with np.errstate(invalid="ignore"):
        zb, vb = pm.zmn_of(g_inf, zeff, p, 15)
    assert vb == 2 and not zb.any()

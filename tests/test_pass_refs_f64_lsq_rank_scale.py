"""CPU checks of tests/pass_refs_f64_lsq_rank_scale.py: every precondition of tests/test_gpu_f64_lstsq_rank_scale.py is proved here on numpy
models, and every assertion of it is shown to catch a defect.

  threshold  on the R of pass_refs_f64_lsq_rank.model_lstsq_rank the rcond list is never degenerate (a value lands exactly on
             fl(rcond R_00) == R_jj in every case), and a rule with >= in place of > fails there.  A default of max(m, n) 2^-53 is NOT
             caught by those lists -- no pivot of the four cases lies between max(m, n) 2^-53 and 2^-52 of R_00, printed below -- so the
             closed-form part carries one case built for it (DEFAULT_SHAPE), and that one catches it;
  tiles      the closed-form expectations hold for the model on model_chol's R0 of the exact diagonal Gram matrix, and each of the
             defects rank_plus, rank_minus, no_perm, dropped_row, tri_skip fails at least one (n, t) of the grid;
  scaling    every intermediate of a model of either entry stays inside [2^-1000, 2^1000] for every (case, k, j_c) used, the model is
             bitwise covariant, and a Zg whose unit entries scale with A, or a D narrowed to float, is not."""
import functools

import numpy as np
import pytest

from tests import pass_refs_f64_lsq as pl
from tests import pass_refs_f64_lsq_rank as pk
from tests import pass_refs_f64_lsq_rank_scale as pr
from tests import pass_refs_f64_qrcp as pq
from tests import pass_refs_f64_scale as ps

CASE_IDS = [c[0] for c in pk.CASES]


# ---- part 2 ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model_r(name):
    _, m, n, _, rcond, _ = pr.case_of(name)[:6]
    _, r, p, k = pk.model_lstsq_rank(pk.case_matrix(name), pk.case_rhs(name, "gaussian"), pk.rcond_of(rcond, m, n), refine=0)
    return r, p, k


@pytest.mark.parametrize("name", pr.THRESHOLD_CASES)
def test_threshold_list_is_never_degenerate_and_catches_ge(name):
    _, m, n, _, rcond, k_expected = pr.case_of(name)[:6]
    r, _, k = _model_r(name)
    assert k == k_expected
    d = np.diag(r)
    values = pr.threshold_rconds(d, m, n, k_expected, rcond)
    js = pr.threshold_indices(n, k_expected)
    assert len(js) >= 4 and {k_expected - 1, k_expected, n - 1} <= set(js) | {0}
    assert [v for _, v in values[:3]] == [0.0, -1.0, rcond] and all(v < 1.0 for _, v in values)
    landed, ge, half = [], [], []
    for label, v in values:
        rc = pr.default_rcond(m, n) if v < 0 else v
        want = pr.entry_rank(r, v, m, n)
        assert want == pk.rank_of(r, rc)
        if pr.lands_on(d, rc):
            landed.append(label)
            assert pr.entry_rank(r, v, m, n, "ge") == want + len(pr.lands_on(d, rc))
        if pr.entry_rank(r, v, m, n, "ge") != want:
            ge.append(label)
        if pr.entry_rank(r, v, m, n, "default_half") != want:
            half.append(label)
    between = [j for j in range(n) if pr.default_rcond(m, n, "default_half") * d[0] < d[j] <= pr.default_rcond(m, n) * d[0]]
    print("threshold %-16s %d values, landing exactly %s; '>=' fails at %s; the halved default fails at %s (pivots between the two "
          "defaults: %s)" % (name, len(values), landed, ge, half, between))
    assert landed and ge == landed
    assert half == [] and between == []       # (recorded: these lists cannot see the default; test_default_case_catches_a_halved_default)
    # the three doubles around every ratio are all there, and the rank steps by the pivots they bracket
    for j in js:
        if d[j] > 0 and d[j] / d[0] < 1.0:
            labels = [l for l, _ in values]
            assert {"j%d-1" % j, "j%d+0" % j, "j%d+1" % j} <= set(labels)


# ---- part 3 ----------------------------------------------------------------------------------------------------------------------------------
def _block_model(n, nrhs, rcond, reorth=0, defect=None, extra_rows=3, span=None):
    e = pr.graded_e(n, span)
    a, b = pr.block_orthogonal(n, e, extra_rows=extra_rows, nrhs=nrhs)
    rc = pr.default_rcond(a.shape[0], n) if rcond < 0 else rcond
    x, r, p, k = pk.model_lstsq_rank(a, b, rc, refine=1, defect=defect, r0=pr.block_r0(a, reorth))
    return e, a, b, x, r, p, k


def test_block_orthogonal_is_what_it_says():
    for n, nrhs in pr.TILE_SHAPES:
        e = pr.graded_e(n)
        a, b = pr.block_orthogonal(n, e, nrhs=nrhs)
        assert a.shape == (16 * n + 3, n) and a.shape[0] % 32 != 0 and b.shape == (a.shape[0], nrhs)
        g = a.T @ a
        assert np.array_equal(g, np.diag(np.ldexp(16.0, -2 * e.astype(np.int32)))), "A^T A is not the exact diagonal"
        assert e.min() == pr.E_OFFSET and e.max() - e.min() <= 40 and len(set(e.tolist())) < n and sorted(e.tolist()) != e.tolist()
        assert np.abs(b).max() <= 3 and np.array_equal(b, np.rint(b)) and not a[16 * n:].any()
        for j in range(n):
            assert np.array_equal(np.flatnonzero(a[:, j]), np.arange(16 * j, 16 * j + 16))
            assert np.array_equal(np.ldexp(a[16 * j:16 * j + 16, j], int(e[j])), np.ldexp(a[:16, 0], int(e[0])))
        ks = [k for k, _, _ in pr.tile_grid(n)]
        assert ks == [k for k in pr.TILE_RANKS if k < n] + [n]
        assert sum(lands for _, _, lands in pr.tile_grid(n)) >= 2
    assert {k for n, _ in pr.TILE_SHAPES for k, _, _ in pr.tile_grid(n)} >= set(pr.TILE_RANKS) | {17, 33, 48, 64}


def test_expected_jpvt_is_the_pivoting_kernels_rule():
    """on a diagonal R0 householder_qrcp (the kernel's conventions) takes expected_jpvt's pivots; they sort e, and differ from the
    stable argsort once an exchange has moved a tied column"""
    assert pr.expected_jpvt([1, 1, 0]).tolist() == [2, 1, 0]
    differs = 0
    for n, _ in pr.TILE_SHAPES:
        e = pr.graded_e(n)
        _, _, p = pq.householder_qrcp(np.diag(np.ldexp(4.0, -e.astype(np.int32))), dtype=np.float64)
        want = pr.expected_jpvt(e)
        assert np.array_equal(p, want) and np.all(np.diff(e[want]) >= 0)
        differs += not np.array_equal(want, np.argsort(e, kind="stable"))
    assert differs, "no shape has a tie that an exchange displaces"


@pytest.mark.parametrize("n,nrhs", pr.TILE_SHAPES)
def test_closed_form_holds_for_the_model(n, nrhs):
    for i, (k, t, lands) in enumerate(pr.tile_grid(n)):
        reorth = i % 2
        e, a, b, x, r, p, rank = _block_model(n, nrhs, 2.0 ** -t, reorth)
        assert pr.expected_rank(e, 2.0 ** -t) == k
        if lands:
            assert np.any(e - e.min() == t), "no pivot sits on this threshold"
        f = pr.check_block(e, a, b, 2.0 ** -t, 0, 2 if reorth else 1, reorth, x, r, p, rank)
        print("block model n %d t %2d rank %2d (on the threshold: %s): err %.2e floor %.2e" % (n, t, k, lands, f["err"], f["floor"]))


@pytest.mark.parametrize("defect", ["rank_plus", "rank_minus", "no_perm", "dropped_row", "tri_skip"])
def test_closed_form_catches_the_seeded_defects(defect):
    caught = []
    for n, nrhs in pr.TILE_SHAPES:
        for k, t, _ in pr.tile_grid(n):
            e, a, b, x, r, p, rank = _block_model(n, nrhs, 2.0 ** -t, 0, defect)
            try:
                pr.check_block(e, a, b, 2.0 ** -t, 0, 1, 0, x, r, p, rank)
            except AssertionError:
                caught.append((n, t))
    print("defect %-12s caught at %d of the (n, t): %s" % (defect, len(caught), caught[:8]))
    assert caught, defect


def test_closed_form_catches_wrong_pivots_ratios_and_sweeps():
    n, nrhs = 33, 5
    k, t, _ = pr.tile_grid(n)[2]
    e, a, b, x, r, p, rank = _block_model(n, nrhs, 2.0 ** -t)
    ok = lambda **kw: pr.check_block(e, a, b, 2.0 ** -t, **{**dict(state=0, sweeps=1, reorth=0, x=x, r=r, jpvt=p, rank=rank), **kw})
    ok()
    for bad in (dict(jpvt=np.argsort(e, kind="stable")), dict(state=3), dict(sweeps=2), dict(r=r * (1 + np.eye(n)[5] * 2.0 ** -52)),
                dict(r=r + np.eye(n, k=1) * 1e-300), dict(x_minnorm=x + 2.0 ** -80)):
        with pytest.raises(AssertionError):
            ok(**bad)
    ok(x_minnorm=x.copy())


def test_default_case_catches_a_halved_default():
    """DEFAULT_SHAPE: m = 4097, one pivot at exactly 2^-40 of R_00.  max(m, n) 2^-52 = 2^-40 (1 + 2^-12) drops it, rank 63;
    max(m, n) 2^-53 keeps it, rank 64"""
    n, nrhs, extra = pr.DEFAULT_SHAPE
    e, a, b, x, r, p, rank = _block_model(n, nrhs, -1.0, extra_rows=extra, span=40)
    assert a.shape[0] == 4097 and e.max() - e.min() == 40 and pr.expected_rank(e, -1.0, 4097) == 63 == rank
    pr.check_block(e, a, b, -1.0, 0, 1, 0, x, r, p, rank)
    assert pr.entry_rank(r, -1.0, 4097, n, "default_half") == 64
    with pytest.raises(AssertionError):
        pr.check_block(e, a, b, -1.0, 0, 1, 0, x, r, p, pr.entry_rank(r, -1.0, 4097, n, "default_half"))


# ---- part 4 ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _trace(name, minimum_norm):
    _, m, n, _, rcond, _ = pr.case_of(name)[:6]
    return pr.model_trace(pk.case_matrix(name), pk.case_rhs(name, "gaussian"), rcond, max(pr.SCALE_REFINES), minimum_norm)


def _scaled(name, minimum_norm, k, j, defect=None, refine=max(pr.SCALE_REFINES)):
    a, b = ps.scale_uniform(pk.case_matrix(name), k), ps.scale_columns(pk.case_rhs(name, "gaussian"), j)
    return pr.model_trace(a, b, pr.case_of(name)[4], refine, minimum_norm, defect)


def test_model_trace_is_the_model():
    from tests import pass_refs_f64_lsq_minnorm as pm
    from tests import pass_refs_f64_lsq_rank_step as pst
    for name in ("tail3_100x7", "rank1_777x33"):
        _, m, n, _, rcond, _ = pr.case_of(name)[:6]
        a, b = pk.case_matrix(name), pk.case_rhs(name, "gaussian")
        for refine in (0, 2):
            x, r, p, k, tr = pr.model_trace(a, b, rcond, refine, False)
            x0, r0, p0, k0, _ = pst.model_lstsq_rank_step(a, b, rcond, refine)
            assert pl.same_bits(x, x0) and pl.same_bits(r, r0) and k == k0 and np.array_equal(p, p0) and pl.same_bits(tr["X%d" % refine], x)
            x, r, p, k, tr = pr.model_trace(a, b, rcond, refine, True)
            x0, r0, p0, k0, _, zmn = pm.model_lstsq_minnorm(a, b, rcond, refine)
            assert pl.same_bits(x, x0) and pl.same_bits(r, r0) and k == k0 and pl.same_bits(tr["Zmn"], zmn)


@pytest.mark.parametrize("minimum_norm", [False, True], ids=["basic", "minnorm"])
@pytest.mark.parametrize("name", CASE_IDS)
def test_scaled_intermediates_stay_in_range_and_the_model_is_covariant(name, minimum_norm):
    """for every (k, j_c) the GPU test uses: the operands scale exactly, every intermediate (R0, rcond R_00, Zeff, G1, Rc, G12, S12, M,
    C, Zmn, the residual, D and X of every pass) stays inside [2^-1000, 2^1000], and the model of the scaled call is the scaled model,
    bit for bit, after every pass (X of pass p is the result of refine = p)"""
    base = _trace(name, minimum_norm)
    nrhs = pr.case_of(name)[3]
    lo, hi, worst = 0.0, 0.0, None
    ends = set()
    for k, j in pr.scale_pairs(name):
        assert j.shape == (nrhs,) and np.abs(j).max() == pr.B_SPAN
        ends |= {int(j.min()), int(j.max())}
        for what, (l, h) in pr.scaled_spans(base[4], k, j).items():
            if l < lo:
                lo, worst = l, (what, k)
            hi = max(hi, h)
            assert -pr.RANGE_LOG2 <= l and h <= pr.RANGE_LOG2, (name, what, k, l, h)
        scaled = _scaled(name, minimum_norm, k, j)
        assert pr.covariant(base, scaled, k, j), (name, k, "the model is not covariant")
        for t in pr.SCALE_REFINES:
            assert pl.same_bits(scaled[4]["X%d" % t], pl.scale_x(base[4]["X%d" % t], k, j)), (name, k, t)
    assert {-pr.B_SPAN, pr.B_SPAN} <= ends, "an end of the range of j_c is never used"
    assert set(pr.SCALE_K) == set(ps.UNIFORM_K)
    print("%-16s %s: rank %d, log2 of the non-zero intermediates from %.1f to %.1f (lowest: %s)"
          % (name, "minnorm" if minimum_norm else "basic", base[3], lo, hi, worst))


def test_scaled_unit_entries_of_zg_break_the_covariance():
    """Zg with unit entries that scale with A: G12 then scales by 4^k, M by 2^k, and the minimum-norm X is no longer covariant; the
    basic entry never forms Zg and keeps the property"""
    for name in ("copied_4096x16", "tail3_100x7"):
        base = _scaled(name, True, 0, np.zeros(pr.case_of(name)[3], np.int64), "zg_scaled", 1)
        k, j = pr.scale_pairs(name)[1]
        assert not pr.covariant(base, _scaled(name, True, k, j, "zg_scaled", 1), k, j), name
        assert pr.covariant(_trace(name, False), _scaled(name, False, k, j, "zg_scaled"), k, j), name


@pytest.mark.parametrize("minimum_norm", [False, True], ids=["basic", "minnorm"])
def test_a_float_d_breaks_the_covariance(minimum_norm):
    """D narrowed to float leaves float's range once B carries 2^+-400: X is zero or not finite in those columns"""
    for name in ("full_300x17", "rank32_1029x51"):
        base = _scaled(name, minimum_norm, 0, np.zeros(pr.case_of(name)[3], np.int64), "float_d", 1)
        assert np.isfinite(base[0]).all() and base[0].any()
        k, j = pr.scale_pairs(name)[0]
        assert not pr.covariant(base, _scaled(name, minimum_norm, k, j, "float_d", 1), k, j), name

"""CPU checks of tests/pass_refs_f64_lsq_rank.py: the numpy model of the rank-aware least-squares solve is held to the assertions
of its cases, and the seeded defects must be caught by them."""
import numpy as np
import pytest

from tests import pass_refs_f64_lsq as pl
from tests import pass_refs_f64_lsq_rank as pk
from tests import pass_refs_f64_qrcp as pq

CASE_IDS = [c[0] for c in pk.CASES]


@pytest.mark.parametrize("name", CASE_IDS)
def test_case_preconditions(name):
    """every case keeps a factor 1e3 on either side of its threshold, and the default rcond is numpy's"""
    lead, trail = pk.precondition(name)
    print("precondition %-16s lowest leading |R_jj/R_00| %.3e, highest trailing %.3e" % (name, lead, trail))
    assert pk.rcond_of(None, 300, 17) == 300 * np.finfo(np.float64).eps


@pytest.mark.parametrize("kind", pk.RHS_KINDS)
@pytest.mark.parametrize("name", CASE_IDS)
def test_model_meets_the_assertions(name, kind):
    _, m, n, nrhs, rcond, k_expected = next(c[:6] for c in pk.CASES if c[0] == name)
    a, b = pk.case_matrix(name), pk.case_rhs(name, kind)
    rc = pk.rcond_of(rcond, m, n)
    trace = []
    x1, r, p, k = pk.model_lstsq_rank(a, b, rc, refine=1, trace=trace)
    f1 = pk.check(name, kind, x1, p, k)
    x2, _, p2, k2 = pk.model_lstsq_rank(a, b, rc, refine=2)
    f2 = pk.figures(name, kind, x2, p2, k2)
    print("model %-16s %-10s rank %2d err refine 1 %.2e refine 2 %.2e LAPACK %.2e max|D| %s"
          % (name, kind, k, f1["err"], f2["err"], f1["lapack"], ["%.1e" % t for t in trace]))
    assert f2["zero_rows"] and f2["err"] <= max(2.0 * f1["err"], f1["bound"])
    d = np.diag(r)
    assert np.all(d >= 0) and np.all(np.diff(d) <= 0) and np.array_equal(r, np.triu(r))


@pytest.mark.parametrize("defect", ["no_perm", "rank_plus", "rank_minus", "dropped_row", "tri_skip"])
def test_seeded_defects_are_caught(defect):
    """Zeff without the permutation, a rank off by one, a dropped row of X that is not zero, the triangular skip left on in the dense
    pass: each fails the assertions on at least one case"""
    caught = []
    for name, m, n, nrhs, rcond, k_expected in (c[:6] for c in pk.CASES):
        a, b = pk.case_matrix(name), pk.case_rhs(name, "gaussian")
        x, _, p, k = pk.model_lstsq_rank(a, b, pk.rcond_of(rcond, m, n), refine=1, defect=defect)
        try:
            pk.check(name, "gaussian", x, p, k)
        except AssertionError:
            caught.append(name)
    print("defect %-12s caught on %s" % (defect, caught))
    assert caught, defect
    if defect in ("rank_plus", "rank_minus"):
        assert len(caught) == len(pk.CASES)
    if defect == "dropped_row":
        assert caught == [c[0] for c in pk.CASES if c[5] < c[2]]


def test_zeff_and_rank_rule():
    """Zeff = P1 inverse(R11): A Zeff has orthonormal columns 0 .. k - 1 and zero columns beyond; the structure check sees a misplaced
    entry; the inverse stays inside its allowance; rcond = 0 keeps every column with R_jj > 0"""
    a = pk.case_matrix("rank32_1029x51")
    n = a.shape[1]
    r, _, p = pq.householder_qrcp(pl.householder_r(a), dtype=np.float64)
    k = pk.rank_of(r, 1e-6)
    assert k == 32
    z = pk.zeff_of(r, p, k)
    q = a @ z
    assert np.linalg.norm(q[:, :k].T @ q[:, :k] - np.eye(k)) < 1e-8 and not q[:, k:].any()
    zp = pk.unpad_z(pk.pad_z(z), n)
    assert pk.structure_ok(zp, p, k, n)
    assert pk.inverse_residual(r, zp, p, k) <= pk.inverse_allowance(r, k)
    bad = zp.copy()
    bad[p[3], 2] = 1e-300
    assert not pk.structure_ok(bad, p, k, n)
    assert not pk.structure_ok(pk.unpad_z(pk.pad_z(pk.zeff_of(r, p, k, "no_perm")), n), p, k, n)
    r2 = np.triu(np.ones((4, 4)))
    r2[3, 3] = 1e-300
    r2[2, 2] = 0.0
    assert pk.rank_of(r2, 0.0) == 3 and pk.rank_of(r2, 1e-8) == 2


@pytest.mark.parametrize("n,m,nrhs", [(1, 1, 1), (17, 33, 5), (33, 100, 16), (64, 4099, 16)])
def test_dense_pass_model_and_its_defect(n, m, nrhs):
    """on exact integers the model of the dense pass equals the exact D; with the triangular skip left on it differs for n > 16 and a
    dense Z, and equals it for an upper triangular Z"""
    a, z, x, b = pk.exact_dense_case(np.random.default_rng(n + m), m, n, nrhs)
    want = pl.pack_d(pl.d_exact(a, z, x, b), n)
    assert np.array_equal(pk.model_dense_pass(a, z, x, b), want)
    assert np.array_equal(pk.model_dense_pass(a, z, None, b), pl.pack_d(pl.d_exact(a, z, None, b), n))
    skipped = pk.model_dense_pass(a, z, x, b, defect="tri_skip")
    assert np.array_equal(skipped, want) == (n <= 16)
    a, zu, x, b = pk.exact_dense_case(np.random.default_rng(n), m, n, nrhs, upper=True)
    assert np.array_equal(pk.model_dense_pass(a, zu, x, b, defect="tri_skip"), pl.pack_d(pl.d_exact(a, zu, x, b), n))

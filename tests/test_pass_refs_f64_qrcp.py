"""The reference of tests/pass_refs_f64_qrcp.py against scipy.linalg.qr(pivoting=True) (LAPACK dgeqp3): the longdouble Householder QR
with column pivoting must reproduce R0 P far below fp64 rounding with an orthogonal H, have the structure the kernel promises, give
LAPACK's |diag R| to rounding, and take LAPACK's pivots on matrices whose candidate norms are separated at every step.  LAPACK's own
figures on the test matrices are recorded and held to what was measured for the issue (residual <= 6e-16, ||H^T H - I||_F <= 5e-15,
diag(R) monotone -- up to rounding at cond 1), so that the allowance the GPU tests derive from them is a known quantity."""
import numpy as np
import pytest

from tests import pass_refs_f64 as p64
from tests import pass_refs_f64_qrcp as pq

LD = np.longdouble
NS = (17, 33, 64)
CONDS = (1.0, 1e6, 1e12)


def setup_module(module):
    p64.require_longdouble()


def scipy_qrcp(r0):
    import scipy.linalg
    h, r, p = scipy.linalg.qr(np.asarray(r0, np.float64), pivoting=True)
    return h, r, p


@pytest.mark.parametrize("n", NS)
def test_reference_against_lapack(n):
    for cond in CONDS:
        r0 = pq.r_of_cond(n, cond, 7 * n)
        r, h, p = pq.householder_qrcp(r0)
        f = pq.figures(r0, r, h, p)
        assert f["upper"] and f["diag_ok"] and f["perm"], f
        assert f["residual"] <= 1e-17 * n and f["h_orth"] <= 1e-17 * n, f
        assert pq.pivot_slack(r) <= 1e-17 * n * n
        lap = pq.lapack_figures(r0)
        print("LAPACK n %d cond %.0e: residual %.3e, ||HtH-I|| %.3e" % (n, cond, lap["residual"], lap["h_orth"]))
        assert lap["residual"] <= 6e-16 and lap["h_orth"] <= 5e-15 and lap["perm"], lap
        _, rs, _ = scipy_qrcp(r0)
        d, ds = np.diag(np.asarray(r, np.float64)), np.abs(np.diag(rs))
        # (dgeqp3 downdates its norms: at cond 1, where R0 is the identity up to rounding, its diagonal is monotone up to rounding only)
        assert np.all(np.diff(ds) <= 8 * p64.U * ds[0]), "LAPACK's |diag R| is not monotone"
        assert np.max(np.abs(d - ds)) <= 8 * n * p64.U * ds[0], "|diag R| against LAPACK"


@pytest.mark.parametrize("n", (1, 2) + NS)
def test_reference_takes_lapacks_pivots_when_the_candidates_are_separated(n):
    r0 = pq.separated(n, 11 * n)
    gaps = pq.candidate_gaps(r0)
    assert all(g <= 0.75 ** 2 * (1 + 1e-9) for g in gaps), max(gaps)
    r, h, p = pq.householder_qrcp(r0)
    _, _, ps_ = scipy_qrcp(r0)
    assert np.array_equal(p, ps_), (p, ps_)
    r64, h64, p64_ = pq.householder_qrcp(r0, np.float64)      # the fp64 model of the kernel takes them too
    assert np.array_equal(p64_, p)
    f = pq.figures(r0, r64, h64, p64_)
    lap = pq.lapack_figures(r0)
    assert f["residual"] <= pq.allowance(lap["residual"], n) and f["h_orth"] <= pq.allowance(lap["h_orth"], n), (f, lap)


def test_reference_conventions_on_fixed_cases():
    for n in (1, 5, 64):
        r, h, p = pq.householder_qrcp(np.eye(n))
        assert np.array_equal(r, np.eye(n)) and np.array_equal(h, np.eye(n)) and np.array_equal(p, np.arange(n))
        r, h, p = pq.householder_qrcp(np.zeros((n, n)))
        assert np.array_equal(r, np.zeros((n, n))) and np.array_equal(h, np.eye(n)) and np.array_equal(p, np.arange(n))
        d = np.arange(1.0, n + 1.0)
        r, h, p = pq.householder_qrcp(np.diag(d))
        assert np.array_equal(np.asarray(r, np.float64), np.diag(d[::-1])) and np.array_equal(p, np.arange(n)[::-1])
        assert np.array_equal(np.abs(np.asarray(h, np.float64)), np.eye(n)[:, ::-1])
    r0 = np.triu(np.random.default_rng(3).standard_normal((9, 9)))
    r0[:, 6] = r0[:, 2]                                       # two identical columns (the copy upper triangular too: rows 3.. of column 2 are zero)
    r0[:, 2] *= 64.0
    r0[:, 6] *= 64.0                                          # ... and the largest, so that they tie for the first pivot
    r, h, p = pq.householder_qrcp(r0)
    assert p[0] == 2, p
    assert abs(float(r[-1, -1])) <= 1e-17 * 9 * pq.fro(r0)    # (rank 8)
    r, h, p = pq.householder_qrcp(-np.eye(3))                 # a negative diagonal is made positive, H takes the sign
    assert np.array_equal(r, np.eye(3)) and np.array_equal(h, -np.eye(3))


def test_rank_and_slack_helpers():
    r0 = pq.r_of_rank(33, 16, 5)
    assert np.array_equal(r0, np.triu(r0)) and np.all(r0[16:] == 0) and np.linalg.matrix_rank(r0) == 16
    r, h, p = pq.householder_qrcp(r0)
    assert np.max(np.abs(np.diag(np.asarray(r, np.float64))[16:])) <= 1e-17 * 33 * pq.fro(r0)
    r0 = pq.r_of_rank_rounded(33, 16, 5)
    assert np.array_equal(r0, np.triu(r0)) and np.any(r0[16:] != 0) and np.linalg.matrix_rank(r0) == 16
    assert pq.fro(r0[16:]) <= 33 * p64.U * pq.fro(r0)         # (rank 16 up to the rounding of the product and the QR)
    assert pq.pivot_slack(np.eye(4)) == 0.0
    assert pq.pivot_slack(np.array([[1.0, 2.0], [0.0, 1.0]])) == 4.0
    assert pq.pivot_slack(np.array([[0.0, 1.0], [0.0, 0.0]])) == np.inf
    assert pq.allowance(0.0, 64) == 64 * p64.U

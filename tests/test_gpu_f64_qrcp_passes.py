"""The pivoting pass of the fp64 pivoted QR entry alone (qrcp_r_f64_kernel through the test library and the product's launcher):
R0 P = H R of an n x n upper triangular R0.

Accuracy: ||R0 P - H R||_F / ||R0||_F and ||H^T H - I||_F are each at most max(4 x the same figure of scipy.linalg.qr(pivoting=True)
on the same R0, n 2^-53), the allowance of the SVD pass tests.  Structure: R exactly upper triangular, diag(R) >= 0 and non-increasing,
jpvt a permutation.  Pivot property: R_kk^2 >= (1 - 8 n^2 2^-53) sum_{i=k..j} R_ij^2 for all j > k -- the norm of a column's remaining
part is preserved by each of the at most n later reflectors up to a relative change of order n u, and the pivot was the largest when it
was taken.  Rank: for R0 of exact rank r, |R_kk| <= 4 n 2^-53 ||R0||_F for k >= r.  Fixed cases, power-of-two scaling, and memory:
NaN below the diagonal of the input is never read, sentinels around every output are untouched, H is zero padded, two runs agree
bitwise, and r may be r0 itself.  Every figure is printed before it is asserted."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import pass_refs_f64 as p64
from tests import pass_refs_f64_qrcp as pq

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
SENT = -777.0
ISENT = -777
c_sz, c_p, c_i = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int
NS = [1, 2, 15, 16, 17, 33, 63, 64]
CONDS = (1.0, 1e6, 1e12)


@pytest.fixture(scope="module")
def st():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    L = ctypes.CDLL(os.path.join(ROOT, "tsqr_gpu_amd", "csrc", "libtsqr_selftest.so"))
    L.tsqr_selftest_f64_qrcp_r.restype = c_i
    L.tsqr_selftest_f64_qrcp_r.argtypes = [c_p, c_sz, c_p, c_sz, c_p, c_p, c_p, c_i]
    return L, torch


def qrcp_r(st, r0, pad=3, want_h=True, in_place=False):
    """-> (R (n x n), H (n x n or None), jpvt, status); checks the zero padding of H and the sentinels around every output"""
    L, torch = st
    n = r0.shape[0]
    NP = 16 * ((n + 15) // 16)
    ldr0 = n + pad
    ldr = ldr0 if in_place else n + pad + 2
    fill = SENT if in_place else NAN
    rh = np.full((n, ldr0), fill)
    rh[:, :n] = np.triu(r0).T                                # column-major with ld ldr0
    rh[:, :n][np.tril(np.ones((n, n), bool), -1).T] = NAN    # NaN below the diagonal: never read
    r0d = torch.from_numpy(rh).cuda()
    rd = r0d if in_place else torch.full((n, ldr), SENT, dtype=torch.float64, device="cuda")
    hd = torch.full((NP * NP + 2,), SENT, dtype=torch.float64, device="cuda")
    pd = torch.full((n + 2,), ISENT, dtype=torch.int32, device="cuda")
    status = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    rc = L.tsqr_selftest_f64_qrcp_r(r0d.data_ptr(), ldr0, rd.data_ptr(), ldr, pd.data_ptr() + 4, hd.data_ptr() + 8 if want_h else None,
                                    status.data_ptr(), n)
    assert rc == 0, rc
    r, h, p, stat = rd.cpu().numpy(), hd.cpu().numpy(), pd.cpu().numpy(), status.cpu().numpy()
    assert np.all(r[:, n:] == SENT), "the padding of r was written"
    assert p[0] == ISENT and p[-1] == ISENT and h[0] == SENT and h[-1] == SENT and np.all(stat[2:] == 77)
    assert stat[0] == n
    if not in_place:
        back = r0d.cpu().numpy()
        assert np.array_equal(np.isnan(back), np.isnan(rh)) and np.array_equal(back[~np.isnan(rh)], rh[~np.isnan(rh)]), "R0 was written"
    if want_h:
        hfull = h[1:-1].reshape(NP, NP).T
        assert np.all(hfull[n:, :] == 0) and np.all(hfull[:, n:] == 0), "H is not zero padded"
        hout = hfull[:n, :n].copy()
    else:
        assert np.all(h == SENT), "H was written although it was not wanted"
        hout = None
    return r[:, :n].T.copy(), hout, p[1:-1].copy(), stat[:2].copy()


@functools.lru_cache(maxsize=None)
def reference(n, cond, seed):
    r0 = pq.r_of_cond(n, cond, seed)
    r0.setflags(write=False)
    return r0, pq.lapack_figures(r0)


def check_structure(r0, r, h, p, what):
    n = r0.shape[0]
    f = pq.figures(r0, r, h, p)
    assert f["perm"], (what, "jpvt is not a permutation", p)
    assert f["upper"], (what, "R is not exactly upper triangular")
    assert f["diag_ok"], (what, "diag(R) is not non-negative and non-increasing", np.diag(r))
    slack = pq.pivot_slack(r)
    bound = 8.0 * n * n * p64.U
    print("qrcp_r %s pivot slack: %.3e (allowed %.3e)" % (what, slack, bound))
    assert 1.0 >= (1.0 - bound) * (1.0 + slack), (what, slack)       # R_kk^2 >= (1 - bound) sum, for the worst (k, j)
    return f


@pytest.mark.parametrize("n", NS)
def test_qrcp_r_against_lapack(st, n):
    for cond in CONDS:
        r0, lapack = reference(n, cond, 7 * n)
        what = "n %d cond %.0e" % (n, cond)
        r, h, p, _ = qrcp_r(st, r0)
        f = check_structure(r0, r, h, p, what)
        for key in ("residual", "h_orth"):
            print("qrcp_r %s %s: %.3e (LAPACK %.3e, allowed %.3e)" % (what, key, f[key], lapack[key], pq.allowance(lapack[key], n)))
        for key in ("residual", "h_orth"):
            assert f[key] <= pq.allowance(lapack[key], n), (what, key, f[key], lapack[key])
        r2, h2, p2, _ = qrcp_r(st, r0)
        assert all(np.array_equal(x.view(np.int64), y.view(np.int64)) for x, y in ((r, r2), (h, h2))) and np.array_equal(p, p2), "two runs differ"
        r3, h3, p3, _ = qrcp_r(st, r0, want_h=False, in_place=True)
        assert h3 is None and np.array_equal(r.view(np.int64), r3.view(np.int64)) and np.array_equal(p, p3), "in place without H differs"


@pytest.mark.parametrize("n", [1, 2, 17, 33, 64])
def test_qrcp_r_takes_the_reference_pivots_when_the_candidates_are_separated(st, n):
    r0 = pq.separated(n, 11 * n)
    r_ref, _, p_ref = pq.householder_qrcp(r0)
    r, h, p, _ = qrcp_r(st, r0)
    check_structure(r0, r, h, p, "separated n %d" % n)
    assert np.array_equal(p, p_ref), (p, p_ref)
    err = float(np.max(np.abs(np.diag(r) - np.diag(np.asarray(r_ref, np.float64)))))
    print("qrcp_r separated n %d: max |diag R - reference| %.3e" % (n, err))
    assert err <= 8 * n * p64.U * float(r_ref[0, 0])


@pytest.mark.parametrize("n", [33, 64])
def test_qrcp_r_reveals_an_exact_rank(st, n):
    # exact: rows rank .. of R0 are exact zeros (the trailing pivots then come out exactly 0); rounded: the same product behind an
    # orthogonal transform, re-triangularised and nothing zeroed -- the trailing pivots are finite and the bound has something to bound
    for rank, make in [(rank, make) for rank in (1, n // 2, n - 1) for make in (pq.r_of_rank, pq.r_of_rank_rounded)]:
        r0 = make(n, rank, 100 * n + rank)
        kind = "exact" if make is pq.r_of_rank else "rounded"
        r, h, p, stat = qrcp_r(st, r0)
        check_structure(r0, r, h, p, "rank %d of %d %s" % (rank, n, kind))
        tail = float(np.max(np.abs(np.diag(r)[rank:])))
        bound = 4 * n * p64.U * pq.fro(r0)
        print("qrcp_r n %d rank %d %s: R_rr %.3e, max |R_kk|, k >= rank %.3e (allowed %.3e)"
              % (n, rank, kind, r[rank - 1, rank - 1], tail, bound))
        assert tail <= bound, (n, rank, tail, bound)
        assert r[rank - 1, rank - 1] > 1e3 * bound
        f = pq.figures(r0, r, h, p)
        lap = pq.lapack_figures(r0)
        assert f["residual"] <= pq.allowance(lap["residual"], n) and f["h_orth"] <= pq.allowance(lap["h_orth"], n), (f, lap)


def test_qrcp_r_fixed_cases(st):
    for n in (1, 17, 64):
        r, h, p, stat = qrcp_r(st, np.eye(n))
        assert np.array_equal(r, np.eye(n)) and np.array_equal(h, np.eye(n)) and np.array_equal(p, np.arange(n)) and stat[1] == 0
        r, h, p, stat = qrcp_r(st, np.zeros((n, n)))
        assert np.array_equal(r, np.zeros((n, n))) and np.array_equal(h, np.eye(n)) and np.array_equal(p, np.arange(n)) and stat[1] == n
        d = np.arange(1.0, n + 1.0)
        r, h, p, stat = qrcp_r(st, np.diag(d))
        assert np.array_equal(r, np.diag(d[::-1])) and np.array_equal(p, np.arange(n)[::-1])
        assert np.array_equal(np.abs(h), np.eye(n)[:, ::-1])
        assert np.array_equal(np.diag(d)[:, p], h @ r)
    r, h, p, _ = qrcp_r(st, -np.eye(5))
    assert np.array_equal(r, np.eye(5)) and np.array_equal(h, -np.eye(5)) and np.array_equal(p, np.arange(5))
    n = 33
    r0 = np.triu(np.random.default_rng(3).standard_normal((n, n)))
    r0[:, 20] = r0[:, 7]                                      # two identical columns, upper triangular both (rows 8 .. of column 7 are zero)
    r0[:, [7, 20]] *= 64.0                                    # ... and the largest: they tie for the first pivot
    r, h, p, _ = qrcp_r(st, r0)
    check_structure(r0, r, h, p, "two identical columns")
    assert p[0] == 7, p                                       # the lower index is picked first
    assert abs(r[-1, -1]) <= 4 * n * p64.U * pq.fro(r0)       # (rank n - 1)


@pytest.mark.parametrize("k", [500, -500])
def test_qrcp_r_power_of_two_scaling_is_exact(st, k):
    r0, _ = reference(33, 1e6, 7 * 33)
    ra, ha, pa, _ = qrcp_r(st, r0)
    rb, hb, pb, _ = qrcp_r(st, np.ldexp(np.array(r0), k))
    assert np.array_equal(rb, np.ldexp(ra, k)), "R does not scale exactly"
    assert np.array_equal(hb.view(np.int64), ha.view(np.int64)) and np.array_equal(pa, pb)

"""tsqr_mi_qrcp_f64 end to end on the GPU, through the C entry and blockqr.qrcp_f64_tensor.

Bands (the QR entry's): ||Q^T Q - I||_F <= 1e-11 (1e-12 with reorth = 1) and ||A[:, p] - Q R||_F / ||A||_F <= 1e-13; R exactly upper
triangular with diag(R) >= 0 and non-increasing, jpvt a permutation.  Composition: Q, R and jpvt of jobq = 1 are bitwise the two pass
exports (qrcp_r, applyd) on tsqr_mi_qr_f64_lay's Q0 and R0.  R and jpvt of jobq = 0 and jobq = 1 agree in every bit when the ladder
took one sweep (the R-only entry's R0 is then the QR entry's); otherwise the two ladders hand the kernel R0 that differ in the last
digits, and every shape, conditioned ones included, is held to check_agreement's two bounds: the pass allowance plus what that
measured difference of the inputs accounts for.  R and jpvt of jobq = 0 get the structure and pivot-property checks of their own.
All four layout pairs and in place give the same bits; A is
untouched unless q == a; state 3 is passed through before the kernel runs; the numerical rank of a rank-n/2 product plus noise is read
off diag(R) as scipy reads it; the tensor-level call on contiguous, transposed and odd-strided tensors."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import pass_refs_f64 as p64
from tests import pass_refs_f64_qrcp as pq

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COL, ROW = 0, 1
PAIRS = ((COL, COL), (ROW, COL), (COL, ROW), (ROW, ROW))
NAN = float("nan")
ISENT = -777
vp, c_sz, c_i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@functools.lru_cache(maxsize=None)
def selftest():
    L = ctypes.CDLL(os.path.join(ROOT, "tsqr_gpu_amd", "csrc", "libtsqr_selftest.so"))
    for name, args in {"tsqr_selftest_f64_qrcp_r": [vp, c_sz, vp, c_sz, vp, vp, vp, c_i],
                       "tsqr_selftest_f64_applyd_lay": [c_i, c_i, vp, c_sz, vp, c_sz, c_sz, c_i, vp, c_i]}.items():
        getattr(L, name).restype = c_i
        getattr(L, name).argtypes = args
    return L


@functools.lru_cache(maxsize=None)
def matrix(m, n, cond):
    """computed once, shared, never written; cond None: Gaussian, else harness.latms with singular values graded 1 .. 1 / cond"""
    if cond is None:
        a = np.random.default_rng(13 * m + n).standard_normal((m, n))
    else:
        _torch()
        from tsqr_gpu_amd import harness
        s = np.ones(1) if n == 1 else cond ** (-np.arange(n) / (n - 1.0))
        a = harness.latms(m, n, n, s, seed=13 * m + n).double().cpu().numpy().T.copy()      # (latms returns the (n, m) storage)
    a.setflags(write=False)
    return a


def dev(torch, a, layout, pad):
    """a device copy of a in the layout with a leading dimension `pad` above the minimal one (the padding holds NaN), as an m x n view"""
    m, n = a.shape
    if layout == ROW:
        pool = torch.full((m, n + pad), NAN, dtype=torch.float64, device="cuda")
        view = pool[:, :n]
    else:
        pool = torch.full((n, m + pad), NAN, dtype=torch.float64, device="cuda")
        view = pool[:, :m].t()
    view.copy_(torch.from_numpy(np.array(a)).cuda())
    return pool, view, (n if layout == ROW else m) + pad


def bits(t):
    import torch
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t.contiguous()      # (jpvt: integers already)


def same(x, y):
    import torch
    return bool(torch.equal(bits(x), bits(y)))


def qrcp_call(bq, a, a_layout=COL, q_layout=COL, jobq=1, reorth=0, in_place=False, pad=3):
    """the C entry -> (state, ladder sweeps, Q (m x n device view or None), R (n x n device view), jpvt (device, int32))"""
    torch = _torch()
    L = bq.lib()
    m, n = a.shape
    apool, ad, lda = dev(torch, a, a_layout, pad)
    before = apool.clone()
    if jobq and in_place:
        qpool, qd, ldq = apool, ad, lda
    elif jobq:
        qpool, qd, ldq = dev(torch, np.full((m, n), NAN), q_layout, pad + 2)
    else:
        qpool, qd, ldq = None, None, 0
    ldr = n + 1
    r = torch.full((n, ldr), NAN, dtype=torch.float64, device="cuda")
    jp = torch.full((n + 2,), ISENT, dtype=torch.int32, device="cuda")
    wq = torch.empty(L.tsqr_mi_working_q_size_f64_qrcp(m, n, jobq), dtype=torch.float64, device="cuda")
    wr = torch.empty(L.tsqr_mi_working_r_size_f64_qrcp(m, n, jobq), dtype=torch.float64, device="cuda")
    state = L.tsqr_mi_qrcp_f64(a_layout, q_layout, jobq, reorth, vp(qd.data_ptr()) if jobq else None, ldq, vp(r.data_ptr()), ldr,
                               vp(jp.data_ptr() + 4), vp(ad.data_ptr()), lda, m, n, vp(wq.data_ptr()), vp(wr.data_ptr()),
                               vp(torch.cuda.current_stream().cuda_stream))
    sweeps = L.tsqr_mi_last_sweeps_f64()
    torch.cuda.synchronize()
    if not (jobq and in_place):
        assert same(apool, before), "A was written"
    assert int(jp[0]) == ISENT and int(jp[-1]) == ISENT, "jpvt was written outside its n values"
    assert bool(torch.isnan(r[:, n:]).all()), "the padding of r was written"
    if jobq:
        outside = torch.ones_like(qpool, dtype=torch.bool)
        (outside[:, :n] if (a_layout if in_place else q_layout) == ROW else outside[:, :m]).fill_(False)
        assert bool(torch.isnan(qpool[outside]).all()), "the padding of q was written"
    return state, sweeps, qd, r[:, :n].t(), jp[1:-1]


def check_structure(r, jp, what):
    """what every R and jpvt must be, with or without Q: a permutation, exactly upper triangular, diag(R) >= 0 and non-increasing, the
    pivot property; -> (slack, its bound)"""
    rh = r.cpu().numpy()
    n = rh.shape[0]
    d = np.diag(rh)
    assert sorted(jp.tolist()) == list(range(n)), (what, "jpvt is not a permutation")
    assert np.array_equal(rh, np.triu(rh)), (what, "R is not exactly upper triangular")
    assert np.all(d >= 0) and np.all(np.diff(d) <= 0), (what, "diag(R) is not non-negative and non-increasing", d)
    slack, pbound = pq.pivot_slack(rh), 8.0 * n * n * p64.U
    assert 1.0 >= (1.0 - pbound) * (1.0 + slack), (what, slack)
    return slack, pbound


def check_bands(a, reorth, q, r, jp, what):
    torch = _torch()
    m, n = a.shape
    ad = torch.from_numpy(np.array(a)).cuda()
    p = jp.long()
    slack, pbound = check_structure(r, jp, what)
    orth = float(torch.linalg.norm(q.t() @ q - torch.eye(n, dtype=torch.float64, device="cuda")))
    res = float(torch.linalg.norm(ad[:, p] - q @ r) / torch.linalg.norm(ad))
    b_q = 1e-12 if reorth else 1e-11
    print("qrcp %s reorth %d: ||QtQ-I|| %.3e (bound %.0e)  residual %.3e (bound 1e-13)  pivot slack %.3e (allowed %.3e)"
          % (what, reorth, orth, b_q, res, slack, pbound))
    assert orth <= b_q, orth
    assert res <= 1e-13, res


def ladder_r0(bq, a, reorth):
    """R0 of the two ladders on the same A, as the entry gets them: (tsqr_mi_qr_f64_lay's, tsqr_mi_r_f64_lay's), n x n host arrays"""
    torch = _torch()
    L = bq.lib()
    m, n = a.shape
    stream = vp(torch.cuda.current_stream().cuda_stream)
    _, ad, lda = dev(torch, a, COL, 0)
    _, qd, ldq = dev(torch, np.zeros((m, n)), COL, 0)
    out = []
    for with_q in (True, False):
        r = torch.zeros((n, n), dtype=torch.float64, device="cuda")
        sizes = (L.tsqr_mi_working_q_size_f64, L.tsqr_mi_working_r_size_f64) if with_q else (L.tsqr_mi_working_q_size_f64_r, L.tsqr_mi_working_r_size_f64_r)
        wq, wr = (torch.empty(f(m, n), dtype=torch.float64, device="cuda") for f in sizes)
        tail = (vp(r.data_ptr()), n, vp(ad.data_ptr()), lda, m, n, vp(wq.data_ptr()), vp(wr.data_ptr()), stream)
        st = L.tsqr_mi_qr_f64_lay(COL, COL, reorth, vp(qd.data_ptr()), ldq, *tail) if with_q else L.tsqr_mi_r_f64_lay(COL, reorth, *tail)
        assert st == 0, (with_q, st)
        out.append(r.t().cpu().numpy())
    return out


def check_agreement(bq, a, cond, reorth, what, r1, jp1, r0, jp0):
    """R and jpvt of jobq = 1 (r1, jp1) against jobq = 0 (r0, jp0) when the ladders took more than one sweep.  Their inputs then differ:
    delta0 = ||R0(QR ladder) - R0(R-only ladder)||_F / ||R0||_F is measured on the two existing entries.  With eps_res and eps_H the
    pass allowances (max(4 x LAPACK on the call's R0, n 2^-53)):
      Gram     P R^T R P^T = R0^T R0 + (R^T (H^T H - I) R + 2 sym(R^T H^T F)) with F the pass residual, so the two calls' P R^T R P^T
               differ by at most (2 (eps_H + 2.5 eps_res) + 2.1 delta0) ||R0||_F^2 -- whatever the pivots are; asserted for every shape;
      R        with equal pivots R is the triangular factor of R0 P, and the first-order bound for that factor (Stewart; Sun) is
               ||dR||_F / ||R||_F <= sqrt(2) cond(R) delta0: asserted as eps_res + 2 cond(R) delta0.  eps_res alone is what the issue
               names; the second term is what the ladders put in, one ulp of R already exceeds n 2^-53 at n = 1
               (profiles/fp64_qrcp_accuracy.md).  Gaussian shapes must take equal pivots."""
    n = a.shape[1]
    ra, rb = r1.cpu().numpy(), r0.cpu().numpy()
    pa, pb = jp1.cpu().numpy(), jp0.cpu().numpy()
    r0q, r0r = ladder_r0(bq, a, reorth)
    norm0 = pq.fro(r0q)
    delta0 = pq.fro(r0q - r0r) / norm0
    lap = pq.lapack_figures(r0q)
    eps_res, eps_h = pq.allowance(lap["residual"], n), pq.allowance(lap["h_orth"], n)

    def gram(rr, p):
        g = np.zeros((n, n), dtype=np.longdouble)
        g[np.ix_(p, p)] = p64.matmul_ld(rr.T, rr)
        return g

    gdiff = pq.fro(gram(ra, pa) - gram(rb, pb)) / norm0 ** 2
    gbound = 2 * (eps_h + 2.5 * eps_res) + 2.1 * delta0
    same_pivots = bool(np.array_equal(pa, pb))
    kappa = float(np.linalg.cond(ra))
    fig = pq.fro(ra - rb) / pq.fro(ra) if same_pivots else float("nan")
    print("qrcp %s reorth %d agreement: delta0 %.3e  Gram difference %.3e (allowed %.3e)  pivots equal %s  ||dR||/||R|| %.3e "
          "(pass allowance %.3e, with 2 cond(R) delta0 %.3e; cond(R) %.2e)"
          % (what, reorth, delta0, gdiff, gbound, same_pivots, fig, eps_res, eps_res + 2 * kappa * delta0, kappa))
    assert gdiff <= gbound, (gdiff, gbound)
    if cond is None:
        assert same_pivots, (pa, pb)
    if same_pivots and 2 * kappa * delta0 < 0.1:          # (beyond that the first-order bound says nothing)
        assert fig <= eps_res + 2 * kappa * delta0, (fig, eps_res, kappa, delta0)


SMALL_M = {1: 64, 16: 1024, 17: 1088, 51: 3264, 64: 4100}     # 64 n-ish, and no multiple of the 32-row block at n = 64
GRID = [(m, n, None) for n in (1, 16, 17, 51, 64) for m in (SMALL_M[n], 4096, 9211)]
GRID += [(4096, n, cond) for n in (16, 17, 51, 64) for cond in (1e6, 1e12)] + [(9211, 51, 1e6), (9211, 64, 1e12)]


@pytest.mark.parametrize("m,n,cond", GRID)
def test_qrcp_bands_layouts_and_agreement(bq, m, n, cond):
    a = matrix(m, n, cond)
    what = "%dx%d %s" % (m, n, cond)
    for reorth in (0, 1):
        state, sweeps, q, r, jp = qrcp_call(bq, a, COL, COL, 1, reorth)
        assert state == 0 and sweeps >= 1, (state, sweeps, bq.last_error())
        print("qrcp %s reorth %d: ladder sweeps %d" % (what, reorth, sweeps))
        check_bands(a, reorth, q, r, jp, what)
        again = qrcp_call(bq, a, COL, COL, 1, reorth)
        assert all(same(x, y) for x, y in zip((q, r, jp), again[2:])), "two calls differ"
        for a_lay, q_lay in PAIRS[1:]:
            other = qrcp_call(bq, a, a_lay, q_lay, 1, reorth)
            assert other[0] == 0 and all(same(x, y) for x, y in zip((q, r, jp), other[2:])), ("layout pairs differ", a_lay, q_lay)
        for lay in (COL, ROW):
            inp = qrcp_call(bq, a, lay, lay, 1, reorth, in_place=True)
            assert inp[0] == 0 and all(same(x, y) for x, y in zip((q, r, jp), inp[2:])), ("in place differs", lay)
        # jobq = 0: A read only (qrcp_call checks it), both layouts the same bits
        state0, sweeps0, _, r0, jp0 = qrcp_call(bq, a, COL, COL, 0, reorth)
        assert state0 == 0, (state0, bq.last_error())
        row0 = qrcp_call(bq, a, ROW, COL, 0, reorth)
        assert row0[0] == 0 and same(r0, row0[3]) and same(jp0, row0[4]), "jobq = 0: the row-major call differs"
        slack0, pbound0 = check_structure(r0, jp0, what + " jobq 0")
        print("qrcp %s reorth %d jobq 0: ladder sweeps %d, pivot slack %.3e (allowed %.3e)" % (what, reorth, sweeps0, slack0, pbound0))
        if sweeps == 1 and sweeps0 == 1:
            assert same(r, r0) and same(jp, jp0), "one sweep: R and jpvt of jobq = 0 and jobq = 1 differ"
        else:
            check_agreement(bq, a, cond, reorth, what, r, jp, r0, jp0)


def test_qrcp_one_sweep_agreement_is_exercised(bq):
    # a Gaussian matrix takes one sweep with reorth = 0 in both ladders: the bitwise branch above is not an empty promise
    a = matrix(4096, 16, None)
    s1, sw1, _, r1, jp1 = qrcp_call(bq, a, COL, COL, 1, 0)
    s0, sw0, _, r0, jp0 = qrcp_call(bq, a, COL, COL, 0, 0)
    assert (s1, s0) == (0, 0) and (sw1, sw0) == (1, 1), (s1, s0, sw1, sw0)
    assert same(r1, r0) and same(jp1, jp0)


@pytest.mark.parametrize("m,n,cond,reorth", [(4096, 64, None, 0), (4096, 51, 1e6, 1), (64, 16, None, 0), (9211, 17, None, 0)])
def test_qrcp_is_the_composition_of_its_passes(bq, m, n, cond, reorth):
    torch = _torch()
    L, T = bq.lib(), selftest()
    a = matrix(m, n, cond)
    stream = vp(torch.cuda.current_stream().cuda_stream)
    for layout in (COL, ROW):
        state, sweeps, q, r, jp = qrcp_call(bq, a, layout, layout, 1, reorth)
        assert state == 0
        _, ad, lda = dev(torch, a, layout, 3)
        qpool, qd, ldq = dev(torch, np.zeros((m, n)), layout, 3)
        r0 = torch.zeros((n, 64), dtype=torch.float64, device="cuda")
        wq = torch.empty(L.tsqr_mi_working_q_size_f64(m, n), dtype=torch.float64, device="cuda")
        wr = torch.empty(L.tsqr_mi_working_r_size_f64(m, n), dtype=torch.float64, device="cuda")
        assert L.tsqr_mi_qr_f64_lay(layout, layout, reorth, vp(qd.data_ptr()), ldq, vp(r0.data_ptr()), 64, vp(ad.data_ptr()), lda, m, n,
                                    vp(wq.data_ptr()), vp(wr.data_ptr()), stream) == 0
        assert L.tsqr_mi_last_sweeps_f64() == sweeps
        NP = 16 * ((n + 15) // 16)
        r2 = torch.empty((n, n), dtype=torch.float64, device="cuda")
        h2 = torch.empty(NP * NP, dtype=torch.float64, device="cuda")
        jp2 = torch.empty(n, dtype=torch.int32, device="cuda")
        assert T.tsqr_selftest_f64_qrcp_r(r0.data_ptr(), 64, r2.data_ptr(), n, jp2.data_ptr(), h2.data_ptr(), None, n) == 0
        assert T.tsqr_selftest_f64_applyd_lay(layout, layout, qd.data_ptr(), ldq, qd.data_ptr(), ldq, m, n, h2.data_ptr(), 0) == 0
        assert same(r, r2.t()) and same(jp, jp2) and same(q, qd), "the entry is not the composition of its passes"


def test_qrcp_passes_state_3_through(bq):
    a = np.array(matrix(4096, 16, None))
    a[17, 3] = NAN
    for jobq in (0, 1):
        state, _, _, _, jp = qrcp_call(bq, a, COL, COL, jobq, 0)
        assert state == bq.error_not_finite, (jobq, state)
        assert bool((jp == ISENT).all()), "the pivoting kernel ran after state 3"


def test_qrcp_numerical_rank(bq):
    import scipy.linalg
    m, n, rank = 4096, 64, 32
    rng = np.random.default_rng(77)
    a = rng.standard_normal((m, rank)) @ rng.standard_normal((rank, n))
    a += 1e-10 * np.linalg.norm(a) / np.sqrt(m * n) * rng.standard_normal((m, n))     # noise of relative size 1e-10, entry by entry
    for jobq in (0, 1):
        state, sweeps, q, r, jp = qrcp_call(bq, a, COL, COL, jobq, 0)
        assert state == 0, (state, bq.last_error())
        d = np.diag(r.cpu().numpy())
        print("qrcp rank: jobq %d, sweeps %d, R_00 %.3e, R_%d %.3e, R_%d %.3e, R_last %.3e"
              % (jobq, sweeps, d[0], rank - 1, d[rank - 1], rank, d[rank], d[-1]))
        assert int(np.sum(d > 1e-7 * d[0])) == rank, d
    _, rs, _ = scipy.linalg.qr(a, mode="economic", pivoting=True)
    ds = np.abs(np.diag(rs))
    assert int(np.sum(ds > 1e-7 * ds[0])) == rank
    print("qrcp rank: scipy R_%d %.3e, R_%d %.3e (the pivots may differ: only the count is compared)" % (rank - 1, ds[rank - 1], rank, ds[rank]))


def test_qrcp_copied_column_is_recorded(bq):
    """outside the band: the ladder accepts an exactly copied column on its shifted path -- recorded in profiles/fp64_qrcp_accuracy.md.
    The bands are not asserted; when the state is 0, what holds whatever the ladder did is (check_structure: a permutation, R exactly
    upper triangular, diag(R) >= 0 and non-increasing, the pivot property).  This is the input the rank-aware least-squares entry
    exists for: on the same A with rcond = 1e-8 it returns rank 15, and the column it drops is one of the two copies."""
    torch = _torch()
    a = np.array(matrix(4096, 16, None))
    a[:, 11] = a[:, 4]
    for jobq in (0, 1):
        state, sweeps, _, r, jp = qrcp_call(bq, a, COL, COL, jobq, 0)
        d = np.diag(r.cpu().numpy()) if state == 0 else None
        print("qrcp copied column: jobq %d state %d sweeps %d jpvt %s diag(R) %s"
              % (jobq, state, sweeps, jp.tolist() if state == 0 else None, None if d is None else np.array2string(d, precision=3)))
        assert state in (0, bq.error_not_finite)
        if state == 0:
            check_structure(r, jp, "copied column jobq %d" % jobq)
    b = np.random.default_rng(5).standard_normal((4096, 3))
    x, r, p, rank = bq.lstsq_rank_f64(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), rcond=1e-8)
    print("qrcp copied column: lstsq_rank_f64 rank %d jpvt %s" % (rank, p.tolist()))
    assert rank == 15 and int(p[15]) in (4, 11) and not bool(x[int(p[15])].any())


def test_qrcp_f64_tensor(bq):
    torch = _torch()
    m, n = 4096, 51
    a = matrix(m, n, None)
    at = torch.from_numpy(np.array(a)).cuda()
    eye = torch.eye(n, dtype=torch.float64, device="cuda")

    def check(x, q, r, p):
        assert q.shape == (m, n) and r.shape == (n, n) and p.shape == (n,) and p.dtype == torch.int64
        res = float(torch.linalg.norm(x[:, p] - q @ r) / torch.linalg.norm(x))
        orth = float(torch.linalg.norm(q.t() @ q - eye))
        assert res <= 1e-13 and orth <= 1e-11, (res, orth)
        d = torch.diagonal(r)
        assert bool((d >= 0).all()) and bool((d[1:] <= d[:-1]).all()) and bool(torch.equal(r, torch.triu(r)))

    q, r, p = bq.qrcp_f64_tensor(at)                                          # contiguous: row-major, used where it lies
    check(at, q, r, p)
    _, _, q0, r0, jp0 = qrcp_call(bq, a, ROW, ROW, 1, 0)
    assert same(q, q0) and same(r, r0) and same(p.int(), jp0), "the tensor call differs from the C entry"
    tt = at.t().contiguous().t()                                              # transposed storage: column-major strides
    q2, r2, p2 = bq.qrcp_f64_tensor(tt, reorth=True)
    assert q2.stride() == (1, m) and bq.last_sweeps_f64() % 100 >= 2
    check(tt, q2, r2, p2)
    wide = torch.zeros((m, 2 * n), dtype=torch.float64, device="cuda")
    wide[:, ::2] = at
    q3, r3, p3 = bq.qrcp_f64_tensor(wide[:, ::2])                             # neither rows nor columns contiguous: copied once
    assert same(q3, q) and same(r3, r) and bool(torch.equal(p3, p))
    keep = at.clone()
    r4, p4 = bq.qrcp_f64_tensor(at, compute_q=False)
    assert bool(torch.equal(at, keep)) and r4.shape == (n, n) and bool(torch.equal(torch.sort(p4).values, torch.arange(n, device="cuda")))
    if bq.last_sweeps_f64() == 1:
        assert same(r4, r) and bool(torch.equal(p4, p))
    work = at.clone()
    q5, r5, p5 = bq.qrcp_f64_tensor(work, overwrite_a=True)
    assert q5.data_ptr() == work.data_ptr() and same(q5, q) and same(r5, r) and bool(torch.equal(p5, p))
    bad = at.clone()
    bad[5, 5] = NAN
    for compute_q in (True, False):
        with pytest.raises(bq.QrcpError) as e:
            bq.qrcp_f64_tensor(bad, compute_q=compute_q)
        assert e.value.state == bq.error_not_finite
    with pytest.raises(bq.QrcpError) as e:
        bq.qrcp_f64_tensor(torch.zeros((100, 65), dtype=torch.float64, device="cuda"))
    assert e.value.state == bq.error_unsupported_mode

"""tsqr_mi_svd_f64 end to end on the GPU, through the C entry and blockqr.svd_f64_tensor.

Bounds, with b_Q the QR entry's documented orthogonality band (1e-11; 1e-12 with reorth = 1) and eps_W, eps_R, eps_sigma the pass-level
allowances of tests/pass_refs_f64_svd.py (max(4 x LAPACK's figure on the call's own R, n 2^-53)):
  ||U^T U - I||_F <= b_Q (1 + eps_W) + eps_W          (U^T U - I = W^T (Q^T Q - I) W + W^T W - I)
  ||A - U S V^T||_F / ||A||_F <= 1e-13 + eps_R
  |s_j - s*_j| <= b_Q s*_j + (1e-13 + eps_sigma) s*_1   against the extended-precision QR-then-Jacobi reference
  jobu = 0: E_sigma <= max(8 x LAPACK's on the same A, 1e-13), the R-only entry's band.
Composition: U, S, V are bitwise the two pass exports on tsqr_mi_qr_f64_lay's Q and R; with jobu = 0, S and V are bitwise svd_r on
tsqr_mi_r_f64_lay's R.  A is untouched unless u == a; state 3 is passed through; two calls agree bitwise; 2^+-300 A gives the same
bits of U and V and an exactly scaled S; the tensor-level call on a non-contiguous tensor matches the contiguous one."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import pass_refs_f64_r as p64r
from tests import pass_refs_f64_svd as ps

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COL, ROW = 0, 1
NAN = float("nan")
vp, c_sz, c_i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@functools.lru_cache(maxsize=None)
def selftest():
    L = ctypes.CDLL(os.path.join(ROOT, "tsqr_gpu_amd", "csrc", "libtsqr_selftest.so"))
    for name, args in {"tsqr_selftest_f64_svd_r": [vp, c_sz, vp, vp, vp, c_sz, vp, c_i, c_i],
                       "tsqr_selftest_f64_applyd_lay": [c_i, c_i, vp, c_sz, vp, c_sz, c_sz, c_i, vp, c_i]}.items():
        getattr(L, name).restype = c_i
        getattr(L, name).argtypes = args
    return L


@functools.lru_cache(maxsize=None)
def matrix(m, n, cond):
    """computed once, shared, never written; cond None: Gaussian, 'uniform': the generator of the golden uniform fixtures"""
    if cond == "uniform":
        from oracle import ref_oracle as ro
        a = ro.uniform_matrix(m, n, seed=0).astype(np.float64)
    elif cond is None:
        a = np.random.default_rng(13 * m + n).standard_normal((m, n))
    else:
        a = p64r.cond_matrix(m, n, cond, 13 * m + n)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def sigma_ref(m, n, cond):
    a = matrix(m, n, cond)
    _, r = ps.qr_ld(a)
    return ps.jacobi_svd(r)[0]


def dev(torch, a, layout):
    """a device copy of a in the layout, as an m x n view, and its leading dimension"""
    m, n = a.shape
    if layout == ROW:
        return torch.from_numpy(np.ascontiguousarray(a)).cuda(), n
    return torch.from_numpy(np.ascontiguousarray(a.T)).cuda().t(), m


def svd_call(bq, a, layout=COL, jobu=1, reorth=0, in_place=False, want_v=True):
    """the C entry -> (state, ladder sweeps, Jacobi sweeps, U (m x n device view or None), s, V (n x n device view or None))"""
    torch = _torch()
    L = bq.lib()
    m, n = a.shape
    ad, lda = dev(torch, a, layout)
    before = ad.clone()
    if jobu and not in_place:
        ud = torch.full((m, n) if layout == ROW else (n, m), NAN, dtype=torch.float64, device="cuda")
        ud = ud if layout == ROW else ud.t()
    else:
        ud = ad
    s = torch.full((n,), NAN, dtype=torch.float64, device="cuda")
    v = torch.full((n, n), NAN, dtype=torch.float64, device="cuda")
    wq = torch.empty(L.tsqr_mi_working_q_size_f64_svd(m, n, jobu), dtype=torch.float64, device="cuda")
    wr = torch.empty(L.tsqr_mi_working_r_size_f64_svd(m, n, jobu), dtype=torch.float64, device="cuda")
    state = L.tsqr_mi_svd_f64(layout, layout, jobu, reorth, vp(ud.data_ptr()) if jobu else None, lda, vp(s.data_ptr()),
                              vp(v.data_ptr()) if want_v else None, n, vp(ad.data_ptr()), lda, m, n, vp(wq.data_ptr()), vp(wr.data_ptr()),
                              vp(torch.cuda.current_stream().cuda_stream))
    sweeps, jsweeps = L.tsqr_mi_last_sweeps_f64(), L.tsqr_mi_last_jacobi_sweeps_f64()
    torch.cuda.synchronize()
    if not (jobu and in_place):
        assert same(ad, before), "A was written"
    return state, sweeps, jsweeps, (ud if jobu else None), s, (v.t() if want_v else None)


def bits(t):
    import torch
    return t.contiguous().view(torch.int64)


def same(x, y):
    import torch
    return bool(torch.equal(bits(x), bits(y)))


def pass_allowances(r_host):
    """eps_sigma, eps_W, eps_R of the call's own R (n x n upper triangular, host)"""
    n = r_host.shape[0]
    lap = ps.lapack_figures(r_host, ps.jacobi_svd(r_host)[0])
    return tuple(ps.allowance(lap[k], n) for k in ("sigma", "w_orth", "residual"))


def check_bands(bq, a, cond_key, reorth, u, s, v):
    torch = _torch()
    m, n = a.shape
    L = bq.lib()
    ad, _ = dev(torch, a, COL)
    r = torch.empty((n, n), dtype=torch.float64, device="cuda")
    wq = torch.empty(L.tsqr_mi_working_q_size_f64_r(m, n), dtype=torch.float64, device="cuda")
    wr = torch.empty(L.tsqr_mi_working_r_size_f64_r(m, n), dtype=torch.float64, device="cuda")
    assert L.tsqr_mi_r_f64(reorth, vp(r.data_ptr()), n, vp(ad.data_ptr()), m, m, n, vp(wq.data_ptr()), vp(wr.data_ptr()),
                           vp(torch.cuda.current_stream().cuda_stream)) == 0
    eps_s, eps_w, eps_r = pass_allowances(r.t().cpu().numpy())
    b_q = 1e-12 if reorth else 1e-11
    orth = float(torch.linalg.norm(u.t() @ u - torch.eye(n, dtype=torch.float64, device="cuda")))
    res = float(torch.linalg.norm(ad - (u * s) @ v.t()) / torch.linalg.norm(ad))
    s_ref = np.asarray(sigma_ref(m, n, cond_key), np.float64)
    sh = s.cpu().numpy()
    serr = np.abs(sh - s_ref)
    sbound = b_q * s_ref + (1e-13 + eps_s) * s_ref[0]
    print("svd %dx%d %s reorth %d: ||UtU-I|| %.3e (bound %.3e)  residual %.3e (bound %.3e)  max sigma err / bound %.3e"
          % (m, n, cond_key, reorth, orth, b_q * (1 + eps_w) + eps_w, res, 1e-13 + eps_r, float(np.max(serr / sbound))))
    assert orth <= b_q * (1 + eps_w) + eps_w, orth
    assert res <= 1e-13 + eps_r, res
    assert np.all(serr <= sbound), float(np.max(serr / sbound))
    assert np.all(np.diff(sh) <= 0) and np.all(sh >= 0)


GRID = [(m, n, None) for m in (64, 4096, 16384) for n in (1, 16, 51, 64)] + [(4096, 64, 1e6), (4096, 64, 1e12), (9211, 51, "uniform")]


@pytest.mark.parametrize("m,n,cond", GRID)
def test_svd_bands_layouts_and_determinism(bq, m, n, cond):
    a = matrix(m, n, cond)
    first = None
    for reorth in (0, 1):
        for layout in (COL, ROW):
            state, sweeps, jsweeps, u, s, v = svd_call(bq, a, layout, 1, reorth)
            assert state == 0 and 1 <= jsweeps <= 30 and sweeps >= 1, (state, sweeps, jsweeps, bq.last_error())
            print("svd %dx%d %s reorth %d layout %d: ladder sweeps %d, Jacobi sweeps %d" % (m, n, cond, reorth, layout, sweeps, jsweeps))
            if layout == COL:
                check_bands(bq, a, cond, reorth, u, s, v)
                first = (u, s, v)
                again = svd_call(bq, a, layout, 1, reorth)
                assert all(same(x, y) for x, y in zip(first, again[3:])), "two calls differ"
                inp = svd_call(bq, a, layout, 1, reorth, in_place=True)
                assert all(same(x, y) for x, y in zip(first, inp[3:])), "in place differs"
            else:
                assert all(same(x, y) for x, y in zip(first, (u, s, v))), "the row-major call differs from the column-major one"


@pytest.mark.parametrize("m,n,cond,reorth", [(4096, 64, None, 0), (4096, 51, 1e6, 1), (64, 16, None, 0)])
def test_svd_is_the_composition_of_its_passes(bq, m, n, cond, reorth):
    torch = _torch()
    L, T = bq.lib(), selftest()
    a = matrix(m, n, cond)
    stream = vp(torch.cuda.current_stream().cuda_stream)
    for layout in (COL, ROW):
        state, sweeps, _, u, s, v = svd_call(bq, a, layout, 1, reorth)
        assert state == 0
        ad, lda = dev(torch, a, layout)
        qd = torch.empty_like(ad.t() if layout == COL else ad)
        qd = qd.t() if layout == COL else qd
        r = torch.empty((64, 64), dtype=torch.float64, device="cuda")
        wq = torch.empty(L.tsqr_mi_working_q_size_f64(m, n), dtype=torch.float64, device="cuda")
        wr = torch.empty(L.tsqr_mi_working_r_size_f64(m, n), dtype=torch.float64, device="cuda")
        assert L.tsqr_mi_qr_f64_lay(layout, layout, reorth, vp(qd.data_ptr()), lda, vp(r.data_ptr()), 64, vp(ad.data_ptr()), lda, m, n,
                                    vp(wq.data_ptr()), vp(wr.data_ptr()), stream) == 0
        assert L.tsqr_mi_last_sweeps_f64() == sweeps
        NP = 16 * ((n + 15) // 16)
        s2 = torch.empty(n, dtype=torch.float64, device="cuda")
        w2 = torch.empty(NP * NP, dtype=torch.float64, device="cuda")
        v2 = torch.empty((n, n), dtype=torch.float64, device="cuda")
        st2 = torch.zeros(2, dtype=torch.int32, device="cuda")
        assert T.tsqr_selftest_f64_svd_r(r.data_ptr(), 64, s2.data_ptr(), w2.data_ptr(), v2.data_ptr(), n, st2.data_ptr(), n, 1) == 0
        assert T.tsqr_selftest_f64_applyd_lay(layout, layout, qd.data_ptr(), lda, qd.data_ptr(), lda, m, n, w2.data_ptr(), 0) == 0
        assert same(s, s2) and same(v, v2.t()) and same(u, qd), "the entry is not the composition of its passes"
    # jobu = 0: S and V from the R-only entry's R
    state, sweeps, jsweeps, _, s, v = svd_call(bq, a, COL, 0, reorth)
    assert state == 0
    ad, lda = dev(torch, a, COL)
    r = torch.empty((64, 64), dtype=torch.float64, device="cuda")
    wq = torch.empty(L.tsqr_mi_working_q_size_f64_r(m, n), dtype=torch.float64, device="cuda")
    wr = torch.empty(L.tsqr_mi_working_r_size_f64_r(m, n), dtype=torch.float64, device="cuda")
    assert L.tsqr_mi_r_f64_lay(COL, reorth, vp(r.data_ptr()), 64, vp(ad.data_ptr()), lda, m, n, vp(wq.data_ptr()), vp(wr.data_ptr()), stream) == 0
    assert L.tsqr_mi_last_sweeps_f64() == sweeps
    s2 = torch.empty(n, dtype=torch.float64, device="cuda")
    v2 = torch.empty((n, n), dtype=torch.float64, device="cuda")
    st2 = torch.zeros(2, dtype=torch.int32, device="cuda")
    assert T.tsqr_selftest_f64_svd_r(r.data_ptr(), 64, s2.data_ptr(), None, v2.data_ptr(), n, st2.data_ptr(), n, 1) == 0
    assert same(s, s2) and same(v, v2.t()) and int(st2[0]) == jsweeps
    s_only = svd_call(bq, a, ROW, 0, reorth, want_v=False)
    assert s_only[0] == 0 and same(s_only[4], s), "jobu = 0 without V, row-major"


@pytest.mark.parametrize("m,n,cond", [(4096, 64, None), (4096, 64, 1e6), (16384, 51, None), (64, 1, None)])
def test_svd_values_alone_against_lapack(bq, m, n, cond):
    a = matrix(m, n, cond)
    state, _, _, _, s, _ = svd_call(bq, a, COL, 0, 0)
    assert state == 0
    s_ref = np.asarray(sigma_ref(m, n, cond), np.float64)
    e_lapack = float(np.max(np.abs(np.linalg.svd(a, compute_uv=False) - s_ref)) / s_ref[0])
    e = float(np.max(np.abs(s.cpu().numpy() - s_ref)) / s_ref[0])
    print("svd jobu 0 %dx%d %s: E_sigma %.3e (LAPACK %.3e)" % (m, n, cond, e, e_lapack))
    assert e <= max(8 * e_lapack, 1e-13), (e, e_lapack)


def test_svd_passes_state_3_through(bq):
    for spoil in ("nan", "zero column"):
        a = np.array(matrix(4096, 16, None))
        if spoil == "nan":
            a[17, 3] = NAN
        else:
            a[:, 5] = 0.0
        for jobu in (0, 1):
            state, _, jsweeps, _, _, _ = svd_call(bq, a, COL, jobu, 0)
            assert state == bq.error_not_finite and jsweeps == 0, (spoil, jobu, state, jsweeps)


@pytest.mark.parametrize("k", [300, -300])
def test_svd_power_of_two_scaling(bq, k):
    a = matrix(4096, 51, None)
    _, sweeps0, j0, u0, s0, v0 = svd_call(bq, a, COL, 1, 0)
    state, sweeps1, j1, u1, s1, v1 = svd_call(bq, np.ldexp(np.array(a), k), COL, 1, 0)
    assert state == 0 and (sweeps1, j1) == (sweeps0, j0)
    assert same(u0, u1) and same(v0, v1), "U or V changed under a power-of-two scaling"
    assert np.array_equal(s1.cpu().numpy(), np.ldexp(s0.cpu().numpy(), k)), "S does not scale exactly"


def test_svd_f64_tensor_matches_the_contiguous_call(bq):
    torch = _torch()
    a = matrix(4096, 51, None)
    at = torch.from_numpy(np.array(a)).cuda()
    u, s, vh = bq.svd_f64_tensor(at)
    assert u.shape == (4096, 51) and s.shape == (51,) and vh.shape == (51, 51)
    _, _, _, u0, s0, v0 = svd_call(bq, a, ROW, 1, 0)
    assert same(u, u0) and same(s, s0) and same(vh, v0.t()), "Vh is not V transposed, or U, S differ from the C entry"
    wide = torch.zeros((4096, 102), dtype=torch.float64, device="cuda")
    wide[:, ::2] = at
    u2, s2, vh2 = bq.svd_f64_tensor(wide[:, ::2])              # neither rows nor columns contiguous: copied once
    assert same(u2, u) and same(s2, s) and same(vh2, vh)
    u3, s3, vh3 = bq.svd_f64_tensor(at.t().contiguous().t(), reorth=True)   # column-major strides
    assert u3.stride() == (1, 4096) and bq.last_sweeps_f64() % 100 >= 2
    assert same(bq.svd_f64_tensor(at, compute_uv=False), s)
    assert 1 <= bq.last_jacobi_sweeps_f64() <= 30
    res = float(torch.linalg.norm(at - (u * s) @ vh) / torch.linalg.norm(at))
    assert res <= 2e-13, res
    bad = at.clone()
    bad[5, 5] = NAN
    with pytest.raises(bq.SvdError) as e:
        bq.svd_f64_tensor(bad)
    assert e.value.state == bq.error_not_finite

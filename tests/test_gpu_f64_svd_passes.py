"""The two passes of the fp64 SVD entry, each alone through the test library with the product's launchers.

svd_r (svd_r_f64_kernel; transpose = 1 is the product's choice, 0 is run as well): R = W diag(s) V^T held against the longdouble
Jacobi reference of tests/pass_refs_f64_svd.py.  Each of E_sigma, ||W^T W - I||_F, ||V^T V - I||_F and ||R - W S V^T||_F / ||R||_F
is at most max(4 x the same figure of numpy.linalg.svd on the same R, n 2^-53); at most 30 sweeps; two runs agree bitwise; a factor
2^+-500 scales s exactly and changes no bit of W or V; everything around the outputs is untouched.  Every figure and sweep count is
printed before it is asserted.

applyd (applyd_f64_kernel<NT, QROW, UROW>): U = Q W for a dense W, every entry within (n + 2) 2^-53 (|Q| |W|)_ij of the product in
longdouble, the four layout pairs and in place bitwise equal, guards around the operands untouched."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import pass_refs_f64 as p64
from tests import pass_refs_f64_svd as ps
from tests.test_gpu_f64_apply_rowmajor_passes import COL, NAN, PAIRS, ROW, SENT, Operand
from tests.test_gpu_f64_r_passes import z_dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
c_sz, c_p, c_i = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int
NS = [1, 2, 15, 16, 17, 33, 63, 64]


@pytest.fixture(scope="module")
def st():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    L = ctypes.CDLL(os.path.join(ROOT, "tsqr_gpu_amd", "csrc", "libtsqr_selftest.so"))
    for name, args in {"tsqr_selftest_f64_svd_r": [c_p, c_sz, c_p, c_p, c_p, c_sz, c_p, c_i, c_i],
                       "tsqr_selftest_f64_applyd_lay": [c_i, c_i, c_p, c_sz, c_p, c_sz, c_sz, c_i, c_p, c_i]}.items():
        getattr(L, name).restype = c_i
        getattr(L, name).argtypes = args
    return L, torch


def svd_r(st, r, transpose=1, pad=3):
    """-> (s, W (n x n), V, sweeps, failed); checks the zero padding of W and the sentinels around every output"""
    L, torch = st
    n = r.shape[0]
    NP = 16 * ((n + 15) // 16)
    ldr, ldv = n + pad, n + pad + 1
    rh = np.full((n, ldr), NAN)
    rh[:, :n] = np.triu(r).T                                 # column-major with ld ldr; NaN below the diagonal too: never read
    rh[:, :n][np.tril(np.ones((n, n), bool), -1).T] = NAN
    rd = torch.from_numpy(rh).cuda()
    sd = torch.full((n + 2,), SENT, dtype=torch.float64, device="cuda")
    wd = torch.full((NP * NP + 2,), SENT, dtype=torch.float64, device="cuda")
    vd = torch.full((n, ldv), SENT, dtype=torch.float64, device="cuda")
    status = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    rc = L.tsqr_selftest_f64_svd_r(rd.data_ptr(), ldr, sd.data_ptr() + 8, wd.data_ptr() + 8, vd.data_ptr(), ldv, status.data_ptr(), n, transpose)
    assert rc == 0, rc
    s, w, v, stat = sd.cpu().numpy(), wd.cpu().numpy(), vd.cpu().numpy(), status.cpu().numpy()
    assert s[0] == SENT and s[-1] == SENT and w[0] == SENT and w[-1] == SENT and np.all(v[:, n:] == SENT) and np.all(stat[2:] == 77)
    wfull = w[1:-1].reshape(NP, NP).T
    assert np.all(wfull[n:, :] == 0) and np.all(wfull[:, n:] == 0), "W is not zero padded"
    return s[1:-1].copy(), wfull[:n, :n].copy(), v[:, :n].T.copy(), int(stat[0]), int(stat[1])


@functools.lru_cache(maxsize=None)
def reference(n, cond, seed):
    r = ps.r_of_cond(n, cond, seed)
    r.setflags(write=False)
    s_ref = ps.jacobi_svd(r)[0]
    return r, s_ref, ps.lapack_figures(r, s_ref)


def check_figures(r, s, w, v, s_ref, lapack, what):
    n = r.shape[0]
    f = ps.figures(r, s, w, v, s_ref)
    for key in ("sigma", "w_orth", "v_orth", "residual"):
        print("svd_r %s %s: %.3e (LAPACK %.3e, allowed %.3e)" % (what, key, f[key], lapack[key], ps.allowance(lapack[key], n)))
    for key in ("sigma", "w_orth", "v_orth", "residual"):
        assert f[key] <= ps.allowance(lapack[key], n), (what, key, f[key], lapack[key])
    assert np.all(np.diff(s) <= 0) and np.all(s >= 0), (what, "s is not descending and non-negative")


@pytest.mark.parametrize("n", NS)
def test_svd_r_against_longdouble_jacobi_and_lapack(st, n):
    for cond in (1.0, 1e6, 1e12):
        r, s_ref, lapack = reference(n, cond, 7 * n)
        for transpose in (1, 0):
            s, w, v, sweeps, failed = svd_r(st, r, transpose)
            print("svd_r n %d cond %.0e transpose %d: %d sweeps" % (n, cond, transpose, sweeps))
            assert 1 <= sweeps <= 30, (n, cond, transpose, sweeps)
            if transpose == 1:                                   # (the product's choice carries the claims; the other is recorded)
                assert failed == 0, (n, cond, sweeps)
                check_figures(r, s, w, v, s_ref, lapack, "n %d cond %.0e" % (n, cond))
                s2, w2, v2, sweeps2, _ = svd_r(st, r, transpose)
                assert sweeps2 == sweeps and all(np.array_equal(x.view(np.int64), y.view(np.int64))
                                                 for x, y in ((s, s2), (w, w2), (v, v2))), "two runs differ"


def test_svd_r_identity_and_ascending_diagonal(st):
    for n in (1, 17, 64):
        s, w, v, sweeps, failed = svd_r(st, np.eye(n))
        assert (sweeps, failed) == (1, 0) and np.array_equal(s, np.ones(n))
        assert np.array_equal(w, np.eye(n)) and np.array_equal(v, np.eye(n))
    n = 33
    d = np.arange(1.0, n + 1.0)
    s, w, v, sweeps, failed = svd_r(st, np.diag(d))
    assert (sweeps, failed) == (1, 0) and np.array_equal(s, d[::-1])
    assert np.array_equal(w, np.eye(n)[:, ::-1]) and np.array_equal(v, np.eye(n)[:, ::-1])


@pytest.mark.parametrize("k", [500, -500])
def test_svd_r_power_of_two_scaling_is_exact(st, k):
    r, _, _ = reference(33, 1e6, 7 * 33)
    s0, w0, v0, sweeps0, _ = svd_r(st, r)
    s1, w1, v1, sweeps1, failed = svd_r(st, np.ldexp(np.array(r), k))
    assert failed == 0 and sweeps1 == sweeps0
    assert np.array_equal(s1, np.ldexp(s0, k)), "s does not scale exactly"
    assert np.array_equal(w1.view(np.int64), w0.view(np.int64)) and np.array_equal(v1.view(np.int64), v0.view(np.int64))


def applyd(st, q_op, u_op, wp, wgs=0):
    L, _ = st
    rc = L.tsqr_selftest_f64_applyd_lay(q_op.layout, u_op.layout, u_op.ptr, u_op.ld, q_op.ptr, q_op.ld, q_op.m, q_op.n, wp, wgs)
    assert rc == 0, (rc, q_op.layout, u_op.layout, q_op.m, q_op.n)


@pytest.mark.parametrize("n", [1, 17, 33, 48, 64])           # (NT = 1, 2, 3, 3, 4: every instantiation, 48 the full three-tile W)
def test_applyd_dense_w_all_layouts(st, n):
    _, torch = st
    rng = np.random.default_rng(40 + n)
    w = rng.standard_normal((n, n))
    wpool, wp = z_dev(torch, w, n)
    for m in (1, 31, 33, 4097):
        q = rng.standard_normal((m, n))
        ref = p64.matmul_ld(q, w)
        bound = (n + 2) * p64.U * (np.abs(q) @ np.abs(w))
        want = None
        for pad, wgs in ((0, 0), (5, 3)):
            for q_lay, u_lay in PAIRS:
                q_op = Operand(m, n, q_lay, pad, NAN, q).upload(torch)
                u_op = Operand(m, n, u_lay, pad + (2 if u_lay == COL else 0), SENT).upload(torch)
                applyd(st, q_op, u_op, wp, wgs)
                u, outside = u_op.download()
                assert np.all(outside == SENT), ("U's padding was written", m, n, q_lay, u_lay, pad)
                qb, qout = q_op.download()
                assert np.array_equal(qb, q) and np.all(np.isnan(qout)), "Q was written"
                err = np.abs(np.asarray(u.astype(LD) - ref, np.float64))
                assert np.all(err <= bound), (m, n, q_lay, u_lay, float(np.max(err / bound)))
                want = u if want is None else want
                assert np.array_equal(u.view(np.int64), want.view(np.int64)), ("layout pairs differ", m, n, q_lay, u_lay, pad, wgs)
            for lay in (COL, ROW):
                op = Operand(m, n, lay, pad, NAN, q).upload(torch)
                applyd(st, op, op, wp, wgs)
                u, outside = op.download()
                assert np.all(np.isnan(outside)), ("in place: the padding was written", m, n, lay, pad)
                assert np.array_equal(u.view(np.int64), want.view(np.int64)), ("in place differs", m, n, lay, pad, wgs)
    assert np.array_equal(wpool.cpu().numpy()[[0, -1]], [SENT, SENT])

"""The two kernels the minimum-norm rank-aware fp64 least-squares entry adds, on their own through the test library:
lsq_zg_f64_kernel (tsqr_selftest_f64_lsq_zg) and lsq_minnorm_f64_kernel (tsqr_selftest_f64_lsq_minnorm), on inputs built on the host from
the model (tests/pass_refs_f64_lsq_minnorm.factor_case), with the conventions of tests/test_gpu_f64_lstsq_rank_step_passes.py: sentinels
around every operand, base pointers offset by one double, inputs checked to be unwritten.

The update factor is held to ||S P^T Zmn - I_k||_F and ||(I - pinv(S) S) P^T Zmn||_F, S formed in longdouble from the kernel's own
inputs, each within 2 x the same figure of numpy.linalg.pinv in fp64 on the same inputs or k cond(C) 2^-53 if larger
(pass_refs_f64_lsq_minnorm.factor_allowance).  Measured on the device: profiles/fp64_lstsq_minnorm_accuracy.md."""
import ctypes
import os

import numpy as np
import pytest

from tests import pass_refs_f64_lsq as pl
from tests import pass_refs_f64_lsq_minnorm as pm
from tests import pass_refs_f64_lsq_rank as pk
from tests import pass_refs_f64_lsq_rank_step as ps

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -777.0
c_p, c_i = ctypes.c_void_p, ctypes.c_int


@pytest.fixture(scope="module")
def st():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    L = ctypes.CDLL(os.path.join(ROOT, "tsqr_gpu_amd", "csrc", "libtsqr_selftest.so"))
    sig = {"tsqr_selftest_f64_lsq_zg": [c_p, c_p, c_p, c_i], "tsqr_selftest_f64_lsq_minnorm": [c_p, c_p, c_p, c_p, c_p, c_p, c_i]}
    for name, args in sig.items():
        getattr(L, name).restype = c_i
        getattr(L, name).argtypes = args
    return L, torch


def z_pool(torch, z):
    """an n x n Z as the NP x NP block the kernels take, a sentinel in front and eight behind"""
    return torch.from_numpy(np.concatenate([[SENT], pk.pad_z(z), np.full(8, SENT)])).cuda()


def p_pool(torch, p):
    return torch.from_numpy(np.concatenate([[-5], np.asarray(p, np.int32), np.full(4, -5, np.int32)]).astype(np.int32)).cuda()


def minnorm_kernel(st, g, zeff, p, k):
    """-> (verdict, NP x NP Zmn); G as the summed tiles; the inputs are not written"""
    L, torch = st
    n = zeff.shape[0]
    np_ = pl.np_of(n)
    gpool = torch.from_numpy(np.concatenate([[SENT], ps.pack_g(g, n), np.full(8, SENT)])).cuda()
    zpool, ppool = z_pool(torch, zeff), p_pool(torch, p)
    out = torch.full((1 + np_ * np_ + 8,), SENT, dtype=torch.float64, device="cuda")
    rank = torch.tensor([k, 99, 99, 99], dtype=torch.int32, device="cuda")
    status = torch.full((4,), 99, dtype=torch.int32, device="cuda")
    before = [t.clone() for t in (gpool, zpool, ppool, rank)]
    assert L.tsqr_selftest_f64_lsq_minnorm(gpool.data_ptr() + 8, rank.data_ptr(), ppool.data_ptr() + 4, zpool.data_ptr() + 8,
                                           out.data_ptr() + 8, status.data_ptr(), n) == 0
    for u, v in zip(before, (gpool, zpool, ppool, rank)):
        assert torch.equal(u, v) or torch.equal(u.view(torch.int32), v.view(torch.int32)), "an input was written"
    oh, sh = out.cpu().numpy(), status.cpu().numpy()
    assert oh[0] == SENT and np.all(oh[1 + np_ * np_:] == SENT) and np.all(sh[1:] == 99)
    return int(sh[0]), pk.unpad_z(oh[1:], n)


@pytest.mark.parametrize("n,k", pm.FACTOR_SHAPES)
def test_minnorm_kernel(st, n, k):
    """verdict 0; columns >= k and the padding exact zeros; the two residuals within their allowances; at k = n Zmn is Zeff bit for bit;
    at k = 0 Zmn = 0; two runs give equal bits"""
    g, zeff, p = pm.factor_case(n, k)
    verdict, zmn = minnorm_kernel(st, g, zeff, p, k)
    assert verdict == 0
    assert pm.structure_ok(zmn, k, n)
    if k == 0:
        assert not zmn.any()
    else:
        s = pm.s_of_inputs(g, zeff, p, k)
        res = pm.factor_residuals(s, zmn[:n, :n], p, k)
        allow, yard, floor = pm.factor_allowance(g, zeff, p, k)
        print("minnorm kernel n %2d k %2d: ||S Zmn - I||_F %.2e (pinv %.2e, allowed %.2e)  ||(I - S+ S) Zmn||_F %.2e (pinv %.2e, allowed %.2e)"
              % (n, k, res[0], yard[0], allow[0], res[1], yard[1], allow[1]))
        assert res[0] <= allow[0] and res[1] <= allow[1], (res, allow)
    if k == n:
        assert np.array_equal(zmn[:n, :n].view(np.int64), zeff.view(np.int64))
    verdict2, zmn2 = minnorm_kernel(st, g, zeff, p, k)
    assert verdict2 == 0 and np.array_equal(zmn.view(np.int64), zmn2.view(np.int64))


def test_minnorm_kernel_verdicts(st):
    """a negative pivot in G11: verdict 1; an infinite entry of G12: verdict 2; Zmn wholly zero both times -- plain data paths"""
    g, zeff, p = pm.factor_case(16, 15)
    bad = g.copy()
    bad[7, 7] = -1.0
    verdict, zmn = minnorm_kernel(st, bad, zeff, p, 15)
    assert verdict == 1 and not zmn.any()
    bad = g.copy()
    bad[3, 15] = np.inf
    verdict, zmn = minnorm_kernel(st, bad, zeff, p, 15)
    assert verdict == 2 and not zmn.any()


@pytest.mark.parametrize("n,k", pm.FACTOR_SHAPES)
def test_zg_kernel(st, n, k):
    """entry (p[j], j) becomes 1 for k <= j < n and nothing else moves, the padding and the sentinels included"""
    L, torch = st
    rng = np.random.default_rng(n + k)
    z = rng.standard_normal((n, n))
    p = rng.permutation(n)
    zpool, ppool = z_pool(torch, z), p_pool(torch, p)
    rank = torch.tensor([k, 99], dtype=torch.int32, device="cuda")
    assert L.tsqr_selftest_f64_lsq_zg(ppool.data_ptr() + 4, rank.data_ptr(), zpool.data_ptr() + 8, n) == 0
    want = z.copy()
    for j in range(k, n):
        want[p[j], j] = 1.0
    zh = zpool.cpu().numpy()
    assert np.array_equal(zh.view(np.int64), np.concatenate([[SENT], pk.pad_z(want), np.full(8, SENT)]).view(np.int64))
    assert rank.cpu().tolist() == [k, 99] and ppool.cpu().tolist() == [-5] + [int(i) for i in p] + [-5] * 4

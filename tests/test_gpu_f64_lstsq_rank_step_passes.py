"""The two kernels of the CholeskyQR step of the rank-aware fp64 least-squares entry on their own, through the test library:
gramq_dense_f64_kernel with the product's plan and the reduction (tsqr_selftest_f64_gramq_dense_lay), bit for bit on exact integer
data, and lsq_rank_step_f64_kernel (tsqr_selftest_f64_lsq_rank_step) against numpy's Cholesky and scipy's triangular solve, with the
conventions of tests/test_gpu_f64_lstsq_rank_passes.py: NaN in the padding of A, sentinels behind every output, base pointers offset
by one double and odd leading dimensions.  References: tests/pass_refs_f64_lsq_rank_step.py."""
import ctypes
import os

import numpy as np
import pytest

from tests import pass_refs as pr
from tests import pass_refs_f64_lsq as pl
from tests import pass_refs_f64_lsq_rank as pk
from tests import pass_refs_f64_lsq_rank_step as ps
from tests.test_gpu_f64_lstsq_rank_passes import dense_z_dev, operand
from tests.test_gpu_f64_r_passes import padded, r_plan

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -777.0
c_sz, c_p, c_i = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int


@pytest.fixture(scope="module")
def st():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    L = ctypes.CDLL(os.path.join(ROOT, "tsqr_gpu_amd", "csrc", "libtsqr_selftest.so"))
    gram = [c_i, c_p, c_p, c_sz, c_sz, c_i, c_p, c_p, c_sz, c_i]
    sig = {
        "tsqr_selftest_f64r_plan": [c_sz, c_sz, c_p],
        "tsqr_selftest_f64_gramq_lay": gram,
        "tsqr_selftest_f64_gramq_dense_lay": gram,
        "tsqr_selftest_f64_lsq_rank_step": [c_p, c_p, c_p, c_p, c_i],
    }
    for name, args in sig.items():
        getattr(L, name).restype = c_i
        getattr(L, name).argtypes = args
    return L, torch


def gram_pass(st, a, z, a_row=0, odd=1, nwaves=0, dense=True):
    """the pass (dense or triangular form) and the reduction -> NP x NP matrix; checks the row count word, the sentinels and that no
    input was written"""
    L, torch = st
    m, n = a.shape
    apool, ap, lda = operand(torch, a, a_row, odd)
    zpool, zp = dense_z_dev(torch, z)
    before = [apool.clone(), zpool.clone()]
    plan = r_plan(L, m, n)
    ntri = plan["ntri"]
    nblocks = (nwaves + 3) // 4 if nwaves else plan["nblocks"]
    cap = nblocks * ntri * 256
    if not nwaves:
        assert cap <= plan["wr"]
    part = torch.full((cap + 8,), SENT, dtype=torch.float64, device="cuda")
    gs = torch.full((ntri * 256 + 1 + 8,), SENT, dtype=torch.float64, device="cuda")
    fn = L.tsqr_selftest_f64_gramq_dense_lay if dense else L.tsqr_selftest_f64_gramq_lay
    rc = fn(a_row, gs.data_ptr(), ap, lda, m, n, zp, part.data_ptr(), cap, nwaves)
    assert rc == 0, rc
    g = gs.cpu().numpy()
    assert g[ntri * 256] == float(m), "the row count word behind gsum"
    assert np.all(g[ntri * 256 + 1:] == SENT) and np.all(part[cap:].cpu().numpy() == SENT)
    for p, q in zip(before, (apool, zpool)):
        assert torch.equal(p.view(torch.int64), q.view(torch.int64)), "an input was written"
    return pr.unpack_tiles(g[:ntri * 256], n, False), g[:ntri * 256]


GRAM_N = [1, 16, 17, 33, 64]
GRAM_M = [1, 15, 16, 17, 100, 1029]


@pytest.mark.parametrize("a_row", [0, 1])
@pytest.mark.parametrize("m", GRAM_M)
def test_dense_gram_exact_bit_for_bit(st, m, a_row):
    """integers and a DENSE Z in {-1, 0, 1} (pass_refs_f64_lsq_rank_step.exact_dense_gram_case: every partial sum below 2^53, asserted
    there): the summed tiles equal (A Z)^T (A Z) bit for bit and the tiles of columns >= n are exact zeros, for every NT with and
    without column padding, every row-tile tail, in both layouts of A.  The triangular form on the same data misses it for n > 16
    (checked once per m: the test can tell the two forms apart)"""
    for n in GRAM_N:
        a, z = ps.exact_dense_gram_case(np.random.default_rng(1000 * m + n), m, n)
        g, _ = gram_pass(st, a, z, a_row, n & 1)
        assert np.array_equal(g, padded(ps.gram_dense_exact(a, z), g.shape[0])), (m, n)
    if a_row == 0 and m >= 16:
        a, z = ps.exact_dense_gram_case(np.random.default_rng(m), m, 33)
        g, _ = gram_pass(st, a, z, dense=False)
        assert not np.array_equal(g, padded(ps.gram_dense_exact(a, z), g.shape[0]))


@pytest.mark.parametrize("nwaves", [1, 4, 5])
@pytest.mark.parametrize("n,a_row", [(17, 0), (64, 1), (64, 0)])
def test_dense_gram_exact_wave_override(st, n, a_row, nwaves):
    """one, four, five waves at m = 1029 (65 row tiles, the last one cut by m): a wave strides over several tiles, and with five waves
    three waves of the second workgroup are idle -- they still take part in staging Z"""
    m = 1029
    a, z = ps.exact_dense_gram_case(np.random.default_rng(m + n + nwaves), m, n)
    g, _ = gram_pass(st, a, z, a_row, 1, nwaves)
    assert np.array_equal(g, padded(ps.gram_dense_exact(a, z), g.shape[0]))


@pytest.mark.parametrize("m,n", [(17, 16), (100, 33), (1029, 64), (1029, 17)])
def test_dense_gram_equals_triangular_pass_on_triangular_z(st, m, n):
    """with an upper triangular Z, inside the exact-integer setting, the dense kernel's tiles equal gramq_f64_kernel's bit for bit, in
    both layouts"""
    a, z = ps.exact_dense_gram_case(np.random.default_rng(m * n), m, n, upper=True)
    for a_row in (0, 1):
        gd, vd = gram_pass(st, a, z, a_row)
        gt, vt = gram_pass(st, a, z, a_row, dense=False)
        assert np.array_equal(vd.view(np.int64), vt.view(np.int64))
        assert np.array_equal(gd, padded(ps.gram_dense_exact(a, z), gd.shape[0]))


# ---- lsq_rank_step_f64_kernel -----------------------------------------------------------------------------------------------------------------
def step_kernel(st, zeff, g1, k):
    """-> (verdict, NP x NP Zeff after the step); G1 as the summed tiles with a sentinel behind them, sentinels around Zeff and behind
    the verdict word; the inputs G1 and the rank word are not written"""
    L, torch = st
    n = zeff.shape[0]
    np_ = pl.np_of(n)
    tiles = ps.pack_g(g1, n)
    gpool = torch.from_numpy(np.concatenate([[SENT], tiles, np.full(8, SENT)])).cuda()
    zv = pk.pad_z(zeff)
    zpool = torch.from_numpy(np.concatenate([[SENT], zv, np.full(8, SENT)])).cuda()
    rank = torch.tensor([k, 99, 99, 99], dtype=torch.int32, device="cuda")
    status = torch.full((4,), 99, dtype=torch.int32, device="cuda")
    gbefore = gpool.clone()
    assert L.tsqr_selftest_f64_lsq_rank_step(gpool.data_ptr() + 8, rank.data_ptr(), zpool.data_ptr() + 8, status.data_ptr(), n) == 0
    assert torch.equal(gbefore.view(torch.int64), gpool.view(torch.int64)) and rank.cpu().tolist() == [k, 99, 99, 99]
    zh, sh = zpool.cpu().numpy(), status.cpu().numpy()
    assert zh[0] == SENT and np.all(zh[1 + np_ * np_:] == SENT) and np.all(sh[1:] == 99)
    return int(sh[0]), pk.unpad_z(zh[1:], n)


@pytest.mark.parametrize("eps", ps.STEP_EPS)
@pytest.mark.parametrize("n,k", ps.STEP_SHAPES)
def test_step_kernel(st, n, k, eps):
    """G1 = Q^T Q for Q = orth + eps noise seen through a permuted Zeff (pass_refs_f64_lsq_rank_step.step_case): verdict 0,
    ||Zout^T G Zout - I_k||_F in longdouble, from the true Gram matrix of the columns, within 4 x the same figure of numpy's Cholesky
    plus scipy.linalg.solve_triangular on the same data or k 2^-53; the zero structure of Zeff kept exactly; two runs give equal bits"""
    zeff, g1, p, r11, qtq = ps.step_case(n, k, eps)
    verdict, zout = step_kernel(st, zeff, g1, k)
    assert verdict == 0
    assert pk.structure_ok(zout, p, k, n)
    res, allow = ps.step_residual(zout, p, k, r11, qtq), ps.step_allowance(zeff, g1, p, k, r11, qtq)
    print("step kernel n %2d k %2d eps %.0e: ||Zout^T G Zout - I||_F %.2e, allowance %.2e" % (n, k, eps, res, allow))
    assert res <= allow
    verdict2, zout2 = step_kernel(st, zeff, g1, k)
    assert verdict2 == 0 and np.array_equal(zout.view(np.int64), zout2.view(np.int64))


@pytest.mark.parametrize("n,k,at", [(16, 15, 0), (64, 40, 23), (33, 1, 0)])
def test_step_kernel_verdict_on_a_negative_pivot(st, n, k, at):
    """a G1 whose leading block has a negative diagonal entry: verdict 1 and Zeff wholly zero -- a plain data path"""
    zeff, g1, p, _, _ = ps.step_case(n, k, 1e-8)
    g1 = g1.copy()
    g1[at, at] = -1.0
    verdict, zout = step_kernel(st, zeff, g1, k)
    assert verdict == 1 and not zout.any()


@pytest.mark.parametrize("n", [1, 33, 64])
def test_step_kernel_rank_zero(st, n):
    """k = 0: Zeff = 0 and verdict 0, whatever G1 and Zeff hold"""
    zeff, g1, _, _, _ = ps.step_case(n, 1, 1e-8)
    verdict, zout = step_kernel(st, zeff + 5.0, g1, 0)
    assert verdict == 0 and not zout.any()

"""One pass of the fp64 least-squares entry on its own, through the test library (tsqr_selftest_f64_lsq: lsq_f64_kernel with the
product's plan, f64_plan.h, and the reduction; tsqr_selftest_f64_lsq_update: the solution update), bit for bit on exact data, with the
conventions of tests/test_gpu_f64_r_passes.py: NaN in the leading-dimension padding and behind the last column of A and B, sentinels
behind `part`, the summed D, Z and X, base pointers offset by one double and odd leading dimensions next to aligned ones.  References
and their bit budget: tests/pass_refs_f64_lsq.py."""
import ctypes
import os

import numpy as np
import pytest

from tests import pass_refs_f64_lsq as pl
from tests.test_gpu_passes import upload
from tests.test_gpu_f64_r_passes import r_plan, z_dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
SENT = -777.0
c_sz, c_p, c_i = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int


@pytest.fixture(scope="module")
def st():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    L = ctypes.CDLL(os.path.join(ROOT, "tsqr_gpu_amd", "csrc", "libtsqr_selftest.so"))
    sig = {
        "tsqr_selftest_f64r_plan": [c_sz, c_sz, c_p],
        "tsqr_selftest_f64_lsq": [c_p, c_p, c_sz, c_p, c_sz, c_sz, c_i, c_i, c_p, c_p, c_p, c_sz, c_i],
        "tsqr_selftest_f64_lsq_update": [c_p, c_p, c_sz, c_p, c_p, c_i, c_i, c_i, c_i],
    }
    for name, args in sig.items():
        getattr(L, name).restype = c_i
        getattr(L, name).argtypes = args
    return L, torch


def x_dev(torch, x, n):
    """X as the passes read it (NP x 16, ld NP, zero padded) at an 8-byte aligned address, sentinels around it"""
    v = pl.pad_x(x, n)
    host = np.full(1 + v.size + 8, SENT)
    host[1:1 + v.size] = v
    pool = torch.from_numpy(host).cuda()
    return pool, pool.data_ptr() + 8


def lsq_pass(st, a, z, x, b, lda, ldb, offset, nwaves=0):
    """the pass and the reduction -> the NT * 256 summed doubles; x None: a null pointer.  Checks the row count word, the sentinels and
    that no input was written"""
    L, torch = st
    m, n = a.shape
    nrhs = b.shape[1]
    apool, ap = upload(torch, np.asarray(a, np.float64), lda, pad=NAN, offset=offset, slack=16, dtype=np.float64)
    bpool, bp = upload(torch, np.asarray(b, np.float64), ldb, pad=NAN, offset=offset, slack=16, dtype=np.float64)
    zpool, zp = z_dev(torch, z, n)
    xpool, xp = x_dev(torch, x, n) if x is not None else (torch.zeros(1, dtype=torch.float64, device="cuda"), None)
    before = [p.clone() for p in (apool, bpool, zpool, xpool)]
    plan = r_plan(L, m, n)
    nt = plan["NT"]
    nblocks = (nwaves + 3) // 4 if nwaves else plan["nblocks"]
    cap = nblocks * nt * 256
    if not nwaves:
        assert cap <= plan["wr"]
    part = torch.full((cap + 8,), SENT, dtype=torch.float64, device="cuda")
    ds = torch.full((nt * 256 + 1 + 8,), SENT, dtype=torch.float64, device="cuda")
    rc = L.tsqr_selftest_f64_lsq(ds.data_ptr(), ap, lda, bp, ldb, m, n, nrhs, zp, xp, part.data_ptr(), cap, nwaves)
    assert rc == 0, rc
    d = ds.cpu().numpy()
    assert d[nt * 256] == float(m), "the row count word behind the summed D"
    assert np.all(d[nt * 256 + 1:] == SENT) and np.all(part[cap:].cpu().numpy() == SENT)
    for p, q in zip(before, (apool, bpool, zpool, xpool)):
        assert torch.equal(p.view(torch.int64), q.view(torch.int64)), "an input was written"
    return d[:nt * 256]


LSQ_N = [1, 15, 16, 17, 33, 48, 64]
LSQ_M = [1, 15, 16, 17, 31, 32, 33, 100, 4099]
LSQ_NRHS = [1, 5, 16]


@pytest.mark.parametrize("m", LSQ_M)
def test_lsq_pass_exact_bit_for_bit(st, m):
    """integers (pass_refs_f64_lsq.exact_case: every partial sum below 2^53, asserted there): the summed tiles equal (A Z)^T (B - A X)
    bit for bit, rows >= n and right-hand sides >= nrhs are exact zeros, for every NT, every column tail, every row-tile tail and
    nrhs 1, 5 and 16; base pointers 8-byte aligned only and odd leading dimensions for odd n, aligned and even for even n"""
    for n in LSQ_N:
        for nrhs in LSQ_NRHS:
            a, z, x, b = pl.exact_case(np.random.default_rng(1000 * m + 17 * n + nrhs), m, n, nrhs)
            odd = n & 1
            lda, ldb = (m + 3, m + 5) if odd else (m + (-m) % 2, m + (-m) % 2 + 2)
            got = lsq_pass(st, a, z, x, b, lda, ldb, odd)
            assert np.array_equal(got, pl.pack_d(pl.d_exact(a, z, x, b), n)), (m, n, nrhs)


@pytest.mark.parametrize("nwaves", [1, 4, 5])
@pytest.mark.parametrize("n,nrhs", [(17, 5), (64, 16)])
def test_lsq_pass_exact_wave_override(st, n, nrhs, nwaves):
    """one, four, five waves at m = 4099 (257 row tiles): every wave strides over many tiles, the last tile is ragged, and with five
    waves three waves of the second workgroup are idle"""
    m = 4099
    a, z, x, b = pl.exact_case(np.random.default_rng(m + n + nwaves), m, n, nrhs)
    got = lsq_pass(st, a, z, x, b, m + 1, m + 3, 1, nwaves)
    assert np.array_equal(got, pl.pack_d(pl.d_exact(a, z, x, b), n))


def test_lsq_pass_exact_product_plan_2p16(st):
    """the product's plan at 2^16 x 64: 4096 row tiles on 2048 waves, two tiles a wave, 512 partials through the reduction"""
    L, _ = st
    m, n, nrhs = 1 << 16, 64, 16
    plan = r_plan(L, m, n)
    assert plan["nwaves"] == 2048 and plan["nblocks"] == 512 and plan["ntiles"] == 4096
    a, z, x, b = pl.exact_case(np.random.default_rng(5), m, n, nrhs)
    got = lsq_pass(st, a, z, x, b, m, m, 0)
    assert np.array_equal(got, pl.pack_d(pl.d_exact(a, z, x, b), n))


@pytest.mark.parametrize("m,n,nrhs", [(33, 1, 1), (100, 17, 5), (4099, 64, 16)])
def test_lsq_pass_null_x_is_zero_x(st, m, n, nrhs):
    """x = null and x = 0 give the same bits, those of (A Z)^T B; also on Gaussian data, where the two could differ by a rounding"""
    a, z, _, b = pl.exact_case(np.random.default_rng(m + n), m, n, nrhs)
    zero = np.zeros((n, nrhs))
    d_null, d_zero = lsq_pass(st, a, z, None, b, m + 1, m + 3, 1), lsq_pass(st, a, z, zero, b, m + 1, m + 3, 1)
    assert np.array_equal(d_null.view(np.int64), d_zero.view(np.int64))
    assert np.array_equal(d_null, pl.pack_d(pl.d_exact(a, z, None, b), n))
    rng = np.random.default_rng(m)
    ag, bg, zg = rng.standard_normal((m, n)), rng.standard_normal((m, nrhs)), np.triu(rng.standard_normal((n, n)))
    d_null, d_zero = lsq_pass(st, ag, zg, None, bg, m + 1, m + 3, 1), lsq_pass(st, ag, zg, zero, bg, m + 1, m + 3, 1)
    assert np.array_equal(d_null.view(np.int64), d_zero.view(np.int64))


@pytest.mark.parametrize("n,nrhs", [(1, 1), (17, 5), (64, 16)])
def test_lsq_update_exact_bit_for_bit(st, n, nrhs):
    """integer Z (unit upper triangular, {-1, 0, 1}), D and X: X + Z D is exact.  first: X is taken as zero and its junk is not read;
    last: the caller's x (ldx = n + 3) receives the n x nrhs block and nothing else; the work copy is wholly written, zeros outside"""
    L, torch = st
    rng = np.random.default_rng(n + nrhs)
    z = np.triu(rng.integers(-1, 2, size=(n, n)), 1).astype(np.float64) + np.eye(n)
    d = rng.integers(-1000, 1001, size=(n, nrhs)).astype(np.float64)
    x0 = rng.integers(-1000, 1001, size=(n, nrhs)).astype(np.float64)
    np_ = pl.np_of(n)
    zpool, zp = z_dev(torch, z, n)
    dsum = torch.from_numpy(pl.pack_d(d, n)).cuda()
    ldx = n + 3
    for first, last in ((1, 0), (0, 1), (1, 1)):
        xw_host = np.full(1 + 16 * np_ + 8, SENT)
        if not first:
            xw_host[1:1 + 16 * np_] = pl.pad_x(x0, n)
        xw = torch.from_numpy(xw_host).cuda()
        xo = torch.full((nrhs * ldx + 8,), SENT, dtype=torch.float64, device="cuda")
        assert L.tsqr_selftest_f64_lsq_update(xw.data_ptr() + 8, xo.data_ptr(), ldx, zp, dsum.data_ptr(), n, nrhs, first, last) == 0
        want = z @ d + (0.0 if first else x0)
        out = xw.cpu().numpy()
        assert out[0] == SENT and np.all(out[1 + 16 * np_:] == SENT)
        got = pl.unpad_x(out[1:], n)
        assert np.array_equal(got[:n, :nrhs], want) and not got[n:].any() and not got[:, nrhs:].any()
        xh = xo.cpu().numpy()
        if last:
            assert np.array_equal(xh[:nrhs * ldx].reshape(nrhs, ldx)[:, :n].T, want)
            assert np.all(xh[:nrhs * ldx].reshape(nrhs, ldx)[:, n:] == SENT) and np.all(xh[nrhs * ldx:] == SENT)
        else:
            assert np.all(xh == SENT)

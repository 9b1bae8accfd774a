"""The two kernels of the R-only fp64 entry on their own, through the test library (tsqr_selftest_f64_gramq, tsqr_selftest_f64_zmul: the
product's kernels with the product's plan, f64_plan.h), with the conventions of tests/test_gpu_f64_passes.py: NaN in the leading-dimension
padding and behind the last column, sentinels behind `part`, `gsum` and Z, the base pointer offset by one double, odd leading dimensions
next to aligned ones.  References, bounds and their derivations: tests/pass_refs_f64_r.py.  Every bounded check prints
max(measured / bound)."""
import ctypes
import os

import numpy as np
import pytest

from tests import pass_refs as pr
from tests import pass_refs_f64 as p64
from tests import pass_refs_f64_r as p64r
from tests.test_gpu_passes import report, upload

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
SENT = -777.0
LD = np.longdouble
c_sz, c_p, c_i = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int


@pytest.fixture(scope="module")
def st():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    L = ctypes.CDLL(os.path.join(ROOT, "tsqr_gpu_amd", "csrc", "libtsqr_selftest.so"))
    sig = {
        "tsqr_selftest_f64r_plan": [c_sz, c_sz, c_p],
        "tsqr_selftest_f64_gramq": [c_p, c_p, c_sz, c_sz, c_i, c_p, c_p, c_sz, c_i],
        "tsqr_selftest_f64_zmul": [c_p, c_p, c_i],
    }
    for name, args in sig.items():
        getattr(L, name).restype = c_i
        getattr(L, name).argtypes = args
    return L, torch


def r_plan(L, m, n):
    out = (ctypes.c_longlong * 8)()
    assert L.tsqr_selftest_f64r_plan(m, n, ctypes.cast(out, c_p)) == 0
    return dict(zip("NT ntri ntiles nwaves nblocks wq wr waves".split(), out))


def z_dev(torch, z, n):
    """Z as chol_f64_kernel leaves it (NP x NP, ld NP, zero padded) at an 8-byte aligned address, sentinels around it"""
    v = p64r.pad_z(z, n)
    host = np.full(1 + v.size + 8, SENT)
    host[1:1 + v.size] = v
    pool = torch.from_numpy(host).cuda()
    return pool, pool.data_ptr() + 8


def gramq(st, a, z, lda, offset, nwaves=0):
    """the pass and the reduction -> NP x NP matrix; checks the row count word, the sentinels and that no input was written"""
    L, torch = st
    m, n = a.shape
    pool, ap = upload(torch, np.asarray(a, np.float64), lda, pad=NAN, offset=offset, slack=16, dtype=np.float64)
    before = pool.clone()
    zpool, zp = z_dev(torch, z, n)
    zbefore = zpool.clone()
    plan = r_plan(L, m, n)
    ntri = plan["ntri"]
    assert ntri * 256 == pr.gram_elems(n)
    nblocks = (nwaves + 3) // 4 if nwaves else plan["nblocks"]
    cap = nblocks * ntri * 256
    if not nwaves:
        assert cap <= plan["wr"]
    part = torch.full((cap + 8,), SENT, dtype=torch.float64, device="cuda")
    gs = torch.full((ntri * 256 + 1 + 8,), SENT, dtype=torch.float64, device="cuda")
    rc = L.tsqr_selftest_f64_gramq(gs.data_ptr(), ap, lda, m, n, zp, part.data_ptr(), cap, nwaves)
    assert rc == 0, rc
    g = gs.cpu().numpy()
    assert g[ntri * 256] == float(m), "the row count word behind gsum"
    assert np.all(g[ntri * 256 + 1:] == SENT) and np.all(part[cap:].cpu().numpy() == SENT)
    assert torch.equal(before.view(torch.int64), pool.view(torch.int64)) and torch.equal(zbefore, zpool)
    return pr.unpack_tiles(g[:ntri * 256], n, False)


def padded(g, np_):
    out = np.zeros((np_, np_))
    out[:g.shape[0], :g.shape[1]] = g
    return out


GRAMQ_N = [1, 15, 16, 17, 33, 48, 64]
GRAMQ_M = [1, 15, 16, 17, 31, 32, 33, 100, 4099]


@pytest.mark.parametrize("m", GRAMQ_M)
def test_gramq_exact_bit_for_bit(st, m):
    """integers (pass_refs_f64_r.exact_pair: |A Z| <= 192, m 192^2 < 2^53 asserted): the summed tiles equal (A Z)^T (A Z) bit for bit and
    the tiles of columns >= n are exact zeros, for every NT, every column tail and every row-tile tail; the base pointer 8-byte aligned
    only and lda odd for odd n, 16-byte aligned and lda even for even n"""
    for n in GRAMQ_N:
        a, z = p64r.exact_pair(np.random.default_rng(1000 * m + n), m, n)
        odd = n & 1
        g = gramq(st, a, z, m + 3 if odd else m + (-m) % 2, odd)
        assert np.array_equal(g, padded(p64r.gramq_exact(a, z), g.shape[0])), (m, n)


@pytest.mark.parametrize("nwaves", [1, 4, 5])
@pytest.mark.parametrize("n", [17, 64])
def test_gramq_exact_wave_override(st, n, nwaves):
    """one, four, five waves at m = 4099 (257 row tiles): every wave strides over many tiles, the last tile is ragged, and with five
    waves three waves of the second workgroup are idle"""
    m = 4099
    a, z = p64r.exact_pair(np.random.default_rng(m + n + nwaves), m, n)
    g = gramq(st, a, z, m + 1, 1, nwaves)
    assert np.array_equal(g, padded(p64r.gramq_exact(a, z), g.shape[0]))


def test_gramq_exact_product_plan_2p16(st):
    """the product's plan at 2^16 x 64: 4096 row tiles on 2048 waves, two tiles a wave, 512 partials through the reduction"""
    L, _ = st
    m, n = 1 << 16, 64
    plan = r_plan(L, m, n)
    assert plan["nwaves"] == 2048 and plan["nblocks"] == 512 and plan["ntiles"] == 4096
    a, z = p64r.exact_pair(np.random.default_rng(5), m, n)
    g = gramq(st, a, z, m, 0)
    assert np.array_equal(g, p64r.gramq_exact(a, z))


@pytest.mark.parametrize("m,n", [(1000, 7), (4099, 33), (8192, 64)])
def test_gramq_dense_bound(st, m, n):
    """Gaussian A, upper-triangular Z with column scales 1e-6 .. 1e6, against longdouble, per entry:
    |G^ - G| <= 1.01 (m + 2 n + 16) u (|A| |Z|)^T (|A| |Z|)  (pass_refs_f64_r.gramq_bound)"""
    rng = np.random.default_rng(m + n)
    a, z = rng.standard_normal((m, n)), p64r.mixed_triangular(rng, n)
    g = gramq(st, a, z, m + 3, 1)
    assert p64.padding_is_zero(g, n)
    err = np.asarray(g[:n, :n].astype(LD) - p64r.gramq_ld(a, z), np.float64)
    report("gramq_f64 %d x %d" % (m, n), np.abs(err), p64r.gramq_bound(a, z))


@pytest.mark.parametrize("n", [1, 17, 64])
def test_zmul_exact_bit_for_bit(st, n):
    """integer upper-triangular factors (n kmax^2 < 2^53: the product is exact): Z <- Z Zk bit for bit, the whole NP x NP block written
    (zeros below the diagonal and in the padding, whatever was there), nothing behind it, Zk untouched"""
    L, torch = st
    rng = np.random.default_rng(n)
    z1, z2 = p64.int_triangular(rng, n), p64.int_triangular(rng, n)
    np_ = p64r.np_of(n)
    dirty = np.full((np_, np_), 5.0)                       # the padding and the lower triangle hold junk that must not enter the product
    dirty[:n, :n] = z1 + np.tril(np.full((n, n), 7.0), -1)
    host = np.full(1 + np_ * np_ + 8, SENT)
    host[1:1 + np_ * np_] = np.ascontiguousarray(dirty.T).reshape(-1)
    zpool = torch.from_numpy(host).cuda()
    kpool, kp = z_dev(torch, z2, n)
    kbefore = kpool.clone()
    assert L.tsqr_selftest_f64_zmul(zpool.data_ptr() + 8, kp, n) == 0
    out = zpool.cpu().numpy()
    assert out[0] == SENT and np.all(out[1 + np_ * np_:] == SENT) and torch.equal(kbefore, kpool)
    got = p64r.unpad_z(out[1:], n)
    assert np.array_equal(got, padded(z1 @ z2, np_))

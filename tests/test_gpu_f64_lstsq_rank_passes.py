"""The passes of a rank-aware fp64 least-squares solve on their own, through the test library: the dense-Z form of lsq_f64_kernel with
the product's plan and the reduction (tsqr_selftest_f64_lsq_dense_lay), lsq_rank_f64_kernel (tsqr_selftest_f64_lsq_rank) and the dense
form of lsq_update_f64_kernel with the stagnation rule (tsqr_selftest_f64_lsq_update_rule), bit for bit on exact data, with the
conventions of tests/test_gpu_f64_lsq_pass.py: NaN in the padding of A and B, sentinels behind every output, base pointers offset by
one double and odd leading dimensions.  References: tests/pass_refs_f64_lsq_rank.py."""
import ctypes
import os

import numpy as np
import pytest

from tests import pass_refs_f64_lsq as pl
from tests import pass_refs_f64_lsq_rank as pk
from tests import pass_refs_f64_qrcp as pq
from tests.test_gpu_passes import upload
from tests.test_gpu_f64_r_passes import r_plan

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
SENT = -777.0
c_sz, c_p, c_i, c_d = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int, ctypes.c_double


@pytest.fixture(scope="module")
def st():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    L = ctypes.CDLL(os.path.join(ROOT, "tsqr_gpu_amd", "csrc", "libtsqr_selftest.so"))
    lay = [c_i, c_i, c_p, c_p, c_sz, c_p, c_sz, c_sz, c_i, c_i, c_p, c_p, c_p, c_sz, c_i]
    sig = {
        "tsqr_selftest_f64r_plan": [c_sz, c_sz, c_p],
        "tsqr_selftest_f64_lsq_lay": lay,
        "tsqr_selftest_f64_lsq_dense_lay": lay,
        "tsqr_selftest_f64_lsq_rank": [c_p, c_sz, c_p, c_d, c_p, c_p, c_i],
        "tsqr_selftest_f64_lsq_update_rule": [c_i, c_p, c_p, c_sz, c_p, c_p, c_i, c_i, c_i, c_i, c_p, c_i],
    }
    for name, args in sig.items():
        getattr(L, name).restype = c_i
        getattr(L, name).argtypes = args
    return L, torch


def dense_z_dev(torch, z):
    """a dense n x n Z as the passes read it (NP x NP, ld NP, zero padded) at an 8-byte aligned address, sentinels around it"""
    v = pk.pad_z(z)
    host = np.full(1 + v.size + 8, SENT)
    host[1:1 + v.size] = v
    pool = torch.from_numpy(host).cuda()
    return pool, pool.data_ptr() + 8


def operand(torch, s, row_major, odd):
    """(pool, address, leading dimension) of an m x c operand in either layout: NaN in the padding, an odd offset and stride for odd"""
    m, c = s.shape
    if row_major:
        ld = c + (3 if odd else 2)
        pool, p = upload(torch, np.ascontiguousarray(s.T), ld, pad=NAN, offset=odd, slack=16, dtype=np.float64)
    else:
        ld = m + 3 if odd else m + (-m) % 2 + 2
        pool, p = upload(torch, np.asarray(s, np.float64), ld, pad=NAN, offset=odd, slack=16, dtype=np.float64)
    return pool, p, ld


def lsq_pass(st, a, z, x, b, a_row=0, b_row=0, odd=1, nwaves=0, dense=True):
    """the pass (dense or triangular form) and the reduction -> the NT * 256 summed doubles; x None: a null pointer.  Checks the row
    count word, the sentinels and that no input was written"""
    from tests.test_gpu_f64_lsq_pass import x_dev
    L, torch = st
    m, n = a.shape
    nrhs = b.shape[1]
    apool, ap, lda = operand(torch, a, a_row, odd)
    bpool, bp, ldb = operand(torch, b, b_row, odd)
    zpool, zp = dense_z_dev(torch, z)
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
    fn = L.tsqr_selftest_f64_lsq_dense_lay if dense else L.tsqr_selftest_f64_lsq_lay
    rc = fn(a_row, b_row, ds.data_ptr(), ap, lda, bp, ldb, m, n, nrhs, zp, xp, part.data_ptr(), cap, nwaves)
    assert rc == 0, rc
    d = ds.cpu().numpy()
    assert d[nt * 256] == float(m), "the row count word behind the summed D"
    assert np.all(d[nt * 256 + 1:] == SENT) and np.all(part[cap:].cpu().numpy() == SENT)
    for p, q in zip(before, (apool, bpool, zpool, xpool)):
        assert torch.equal(p.view(torch.int64), q.view(torch.int64)), "an input was written"
    return d[:nt * 256]


DENSE_N = [1, 15, 16, 17, 33, 48, 64]
DENSE_M = [1, 16, 17, 33, 100, 4099]
DENSE_NRHS = [1, 5, 16]


@pytest.mark.parametrize("a_row,b_row", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("m", DENSE_M)
def test_dense_pass_exact_bit_for_bit(st, m, a_row, b_row):
    """integers and a DENSE Z in {-1, 0, 1} (pass_refs_f64_lsq_rank.exact_dense_case: every partial sum below 2^53, asserted there):
    the summed tiles equal (A Z)^T (B - A X) bit for bit, rows >= n and right-hand sides >= nrhs are exact zeros, for every NT, column
    tail, row-tile tail and nrhs 1, 5 and 16, in both layouts of A and of B.  The triangular form on the same data misses it for n > 16
    (checked once per m on the column-major pair: the test can tell the two forms apart)"""
    for n in DENSE_N:
        for nrhs in DENSE_NRHS:
            a, z, x, b = pk.exact_dense_case(np.random.default_rng(1000 * m + 17 * n + nrhs), m, n, nrhs)
            want = pl.pack_d(pl.d_exact(a, z, x, b), n)
            got = lsq_pass(st, a, z, x, b, a_row, b_row, n & 1)
            assert np.array_equal(got, want), (m, n, nrhs)
    if (a_row, b_row) == (0, 0) and m >= 16:
        a, z, x, b = pk.exact_dense_case(np.random.default_rng(m), m, 33, 5)
        assert not np.array_equal(lsq_pass(st, a, z, x, b, dense=False), pl.pack_d(pl.d_exact(a, z, x, b), 33))


@pytest.mark.parametrize("nwaves", [1, 4, 5])
@pytest.mark.parametrize("n,nrhs,a_row,b_row", [(17, 5, 0, 1), (64, 16, 1, 0), (64, 16, 0, 0)])
def test_dense_pass_exact_wave_override(st, n, nrhs, a_row, b_row, nwaves):
    """one, four, five waves at m = 4099 (257 row tiles): every wave strides over many tiles, the last tile is ragged, and with five
    waves three waves of the second workgroup are idle -- they still take part in staging Z"""
    m = 4099
    a, z, x, b = pk.exact_dense_case(np.random.default_rng(m + n + nwaves), m, n, nrhs)
    got = lsq_pass(st, a, z, x, b, a_row, b_row, 1, nwaves)
    assert np.array_equal(got, pl.pack_d(pl.d_exact(a, z, x, b), n))


@pytest.mark.parametrize("m,n,nrhs", [(33, 1, 1), (100, 17, 5), (4099, 64, 16)])
def test_dense_pass_null_x_is_zero_x(st, m, n, nrhs):
    """x = null gives the bits of x = 0, those of (A Z)^T B; also on Gaussian data"""
    a, z, _, b = pk.exact_dense_case(np.random.default_rng(m + n), m, n, nrhs)
    zero = np.zeros((n, nrhs))
    d_null, d_zero = lsq_pass(st, a, z, None, b), lsq_pass(st, a, z, zero, b)
    assert np.array_equal(d_null.view(np.int64), d_zero.view(np.int64))
    assert np.array_equal(d_null, pl.pack_d(pl.d_exact(a, z, None, b), n))
    rng = np.random.default_rng(m)
    ag, bg, zg = rng.standard_normal((m, n)), rng.standard_normal((m, nrhs)), rng.standard_normal((n, n))
    d_null, d_zero = lsq_pass(st, ag, zg, None, bg), lsq_pass(st, ag, zg, zero, bg)
    assert np.array_equal(d_null.view(np.int64), d_zero.view(np.int64))


@pytest.mark.parametrize("m,n,nrhs", [(17, 15, 1), (100, 33, 5), (4099, 48, 16), (4099, 64, 16)])
def test_dense_pass_equals_triangular_pass_on_triangular_z(st, m, n, nrhs):
    """with an upper triangular Z, inside the exact-integer setting, the dense kernel's D equals the triangular kernel's bit for bit,
    in all four layout pairs"""
    a, z, x, b = pk.exact_dense_case(np.random.default_rng(m * n), m, n, nrhs, upper=True)
    want = pl.pack_d(pl.d_exact(a, z, x, b), n)
    for a_row, b_row in ((0, 0), (1, 1), (1, 0), (0, 1)):
        dense = lsq_pass(st, a, z, x, b, a_row, b_row)
        tri = lsq_pass(st, a, z, x, b, a_row, b_row, dense=False)
        assert np.array_equal(dense.view(np.int64), tri.view(np.int64)) and np.array_equal(dense, want)


# ---- lsq_rank_f64_kernel ----------------------------------------------------------------------------------------------------------------------
def rank_kernel(st, r, p, rcond, ldr=None):
    """-> (rank, NP x NP Zeff); r with NaN below the diagonal and in the padding of ldr (neither is read), sentinels behind Zeff"""
    L, torch = st
    n = r.shape[0]
    ldr = ldr or n + 3
    rr = np.where(np.tril(np.ones((n, n), bool), -1), NAN, r)
    rpool, rp = upload(torch, rr, ldr, pad=NAN, offset=1, slack=16, dtype=np.float64)
    jp = torch.from_numpy(np.concatenate([np.asarray(p, np.int32), np.full(4, -9, np.int32)])).cuda()
    np_ = pl.np_of(n)
    zpool = torch.full((1 + np_ * np_ + 8,), SENT, dtype=torch.float64, device="cuda")
    status = torch.full((4,), 99, dtype=torch.int32, device="cuda")
    before = rpool.clone()
    assert L.tsqr_selftest_f64_lsq_rank(rp, ldr, jp.data_ptr(), rcond, zpool.data_ptr() + 8, status.data_ptr(), n) == 0
    assert torch.equal(before.view(torch.int64), rpool.view(torch.int64))
    zh, sh = zpool.cpu().numpy(), status.cpu().numpy()
    assert zh[0] == SENT and np.all(zh[1 + np_ * np_:] == SENT) and np.all(sh[1:] == 99)
    return int(sh[0]), pk.unpad_z(zh[1:], n)


def scipy_qrcp(r0):
    import scipy.linalg
    _, r, p = scipy.linalg.qr(r0, pivoting=True)
    return np.triu(r * np.where(np.diag(r) < 0, -1.0, 1.0)[:, None]), p


RANK_INPUTS = [("gauss", 33, None), ("gauss", 64, None), ("gauss", 1, None), ("gauss", 17, None)] + \
    [(kind, n, r) for kind in ("exact", "rounded") for n, r in ((33, 1), (33, 16), (33, 32), (64, 1), (64, 32), (64, 63))]


@pytest.mark.parametrize("kind,n,rank", RANK_INPUTS)
def test_rank_kernel(st, kind, n, rank):
    """on R and jpvt of scipy.linalg.qr(pivoting=True): the rank is the expected one (rcond 1e-10, a factor 1e3 clear of every pivot on either side -- asserted), Zeff has exact zeros outside the permuted triangle and in the
    padding, ||R11 (P1^T Zeff)[:k, :k] - I||_F <= 4 x scipy.linalg.solve_triangular's figure or k 2^-53, and rcond = 0 keeps every
    column with R_jj > 0"""
    rng = np.random.default_rng(100 * n + (rank or 0))
    if kind == "gauss":
        r0, rank = pl.householder_r(rng.standard_normal((4 * n + 3, n))), n
    else:
        r0 = (pq.r_of_rank if kind == "exact" else pq.r_of_rank_rounded)(n, rank, 100 * n + rank)
    r, p = scipy_qrcp(r0)
    d = np.diag(r)
    assert np.all(d >= 0) and d[rank - 1] >= 1e-7 * d[0] and (rank == n or d[rank] <= 1e-13 * d[0]), "the case sits on the threshold"
    k, zeff = rank_kernel(st, r, p, 1e-10)
    assert k == rank
    assert pk.structure_ok(zeff, p, k, n)
    res, allow = pk.inverse_residual(r, zeff, p, k), pk.inverse_allowance(r, k)
    print("rank kernel %-7s n %2d rank %2d: ||R11 Z11 - I||_F %.2e, allowance %.2e" % (kind, n, k, res, allow))
    assert res <= allow
    k0, z0 = rank_kernel(st, r, p, 0.0, ldr=n)
    assert k0 == int(np.sum(d > 0)) and pk.structure_ok(z0, p, k0, n)
    if k0 == k:
        assert np.array_equal(z0.view(np.int64), zeff.view(np.int64))


# ---- the dense update -------------------------------------------------------------------------------------------------------------------------
def update(st, dense, z, d, x0, first, last, dprev=None, guard=0):
    """-> (X work copy NP x 16, the caller's x or None, dprev after the call)"""
    L, torch = st
    n, nrhs = d.shape
    np_ = pl.np_of(n)
    zpool, zp = dense_z_dev(torch, z)
    dsum = torch.from_numpy(pl.pack_d(d, n)).cuda()
    ldx = n + 3
    xw_host = np.full(1 + 16 * np_ + 8, SENT)
    if not first:
        xw_host[1:1 + 16 * np_] = pl.pad_x(x0, n)
    xw = torch.from_numpy(xw_host).cuda()
    xo = torch.full((nrhs * ldx + 8,), SENT, dtype=torch.float64, device="cuda")
    dp = torch.from_numpy(np.concatenate([np.asarray(dprev, np.float64), [SENT]])).cuda() if dprev is not None else None
    rc = L.tsqr_selftest_f64_lsq_update_rule(dense, xw.data_ptr() + 8, xo.data_ptr(), ldx, zp, dsum.data_ptr(), n, nrhs, first, last,
                                             dp.data_ptr() if dp is not None else None, guard)
    assert rc == 0
    out = xw.cpu().numpy()
    assert out[0] == SENT and np.all(out[1 + 16 * np_:] == SENT)
    xh = xo.cpu().numpy()
    xc = None
    if last:
        xc = xh[:nrhs * ldx].reshape(nrhs, ldx)[:, :n].T.copy()
        assert np.all(xh[:nrhs * ldx].reshape(nrhs, ldx)[:, n:] == SENT) and np.all(xh[nrhs * ldx:] == SENT)
    else:
        assert np.all(xh == SENT)
    dph = None
    if dp is not None:
        dph = dp.cpu().numpy()
        assert dph[16] == SENT
        dph = dph[:16]
    return pl.unpad_x(out[1:], n), xc, dph


@pytest.mark.parametrize("n,nrhs", [(1, 1), (17, 5), (33, 16), (64, 16)])
def test_dense_update_exact_bit_for_bit(st, n, nrhs):
    """integer dense Z in {-1, 0, 1}, D and X: X + Z D is exact, for every first / last combination; the work copy is wholly written,
    zeros outside; the caller's x receives the n x nrhs block only when last.  The triangular form on the same Z gives another result"""
    rng = np.random.default_rng(n + nrhs)
    z = rng.integers(-1, 2, size=(n, n)).astype(np.float64)
    d = rng.integers(-1000, 1001, size=(n, nrhs)).astype(np.float64)
    x0 = rng.integers(-1000, 1001, size=(n, nrhs)).astype(np.float64)
    for first, last in ((1, 0), (0, 1), (1, 1), (0, 0)):
        want = z @ d + (0.0 if first else x0)
        got, xc, _ = update(st, 1, z, d, x0, first, last)
        assert np.array_equal(got[:n, :nrhs], want) and not got[n:].any() and not got[:, nrhs:].any()
        if last:
            assert np.array_equal(xc, want)
    if n > 1:
        tri, _, _ = update(st, 0, z, d, x0, 1, 0)
        assert np.array_equal(tri[:n, :nrhs], np.triu(z) @ d) and not np.array_equal(tri[:n, :nrhs], z @ d)


@pytest.mark.parametrize("n,nrhs", [(17, 5), (64, 16)])
def test_dense_update_stagnation_rule_as_the_triangular_one(st, n, nrhs):
    """dprev and guard: column j with max |D| above half of the pass before is not applied and stops (dprev -1), a stopped column stays
    stopped, the others are applied and dprev takes their max |D|; without guard everything is applied.  The dense and the triangular
    form take the same decisions and leave the same dprev; on an upper triangular Z they leave the same X too"""
    rng = np.random.default_rng(7 * n + nrhs)
    zt = np.triu(rng.integers(-1, 2, size=(n, n))).astype(np.float64)
    zd = rng.integers(-1, 2, size=(n, n)).astype(np.float64)
    d = rng.integers(-1000, 1001, size=(n, nrhs)).astype(np.float64)
    x0 = rng.integers(-1000, 1001, size=(n, nrhs)).astype(np.float64)
    dm = np.abs(d).max(axis=0)
    prev = np.zeros(16)
    prev[:nrhs] = np.where(np.arange(nrhs) % 3 == 0, 4.0 * dm, np.where(np.arange(nrhs) % 3 == 1, 1.5 * dm, -1.0))
    applied = (np.arange(nrhs) % 3 == 0)
    for guard in (1, 0):
        ok = applied if guard else np.ones(nrhs, bool)
        want_prev = np.where(ok, dm, -1.0)
        got_d, xc_d, dp_d = update(st, 1, zd, d, x0, 0, 1, prev, guard)
        assert np.array_equal(got_d[:n, :nrhs], np.where(ok[None, :], x0 + zd @ d, x0)) and np.array_equal(xc_d, got_d[:n, :nrhs])
        got_t, _, dp_t = update(st, 0, zt, d, x0, 0, 1, prev, guard)
        got_dt, _, dp_dt = update(st, 1, zt, d, x0, 0, 1, prev, guard)
        assert np.array_equal(got_t[:n, :nrhs], np.where(ok[None, :], x0 + zt @ d, x0))
        assert np.array_equal(got_t.view(np.int64), got_dt.view(np.int64))
        for dp in (dp_d, dp_t, dp_dt):
            assert np.array_equal(dp[:nrhs], want_prev)

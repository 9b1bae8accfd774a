"""The row-major forms of the three streaming fp64 kernels (gram_f64_kernel, gramq_f64_kernel and lsq_f64_kernel with their AROW / BROW flags set), pass by pass,
through the test library's tsqr_selftest_f64_{gram,gramq,lsq}_lay: EVERY workgroup partial of the row-major kernel equals, bit for bit,
the partial of the column-major kernel on the transposed copy of the same matrix -- the statement of include/tsqr_mi.h that the entry-level
equality rests on.  The data are Gaussian (nothing has to be exact: both runs form the same products in the same order).  The padding
between n and lda (nrhs and ldb), the elements in front of the base pointer and sixteen more behind the last row are NaN, so any use of
them shows in the partials.  nwaves = 3 makes every wave take several 16-row tiles (at m = 1031 also several 64-row chunks of the Gram pass), so
the prefetch of the next tile runs at these sizes; the product's own plan and a two-workgroup grid are run as well."""
import ctypes
import os

import numpy as np
import pytest

from tests.test_gpu_passes import upload
from tests.test_gpu_f64_r_passes import z_dev
from tests.test_gpu_f64_lsq_pass import x_dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
SENT = -777.0
COL, ROW = 0, 1
c_sz, c_p, c_i = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int

MS = [1, 15, 16, 17, 63, 64, 65, 130, 1031]
NS = [1, 3, 16, 17, 33, 51, 64]
PADS = [0, 1, 13]                          # lda = n + pad, ldb = nrhs + pad
NRHS = [1, 5, 16]


@pytest.fixture(scope="module")
def st():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    L = ctypes.CDLL(os.path.join(ROOT, "tsqr_gpu_amd", "csrc", "libtsqr_selftest.so"))
    sig = {
        "tsqr_selftest_f64_gram_lay": [c_i, c_p, c_p, c_sz, c_sz, c_i, c_p, c_sz, c_i],
        "tsqr_selftest_f64_gramq_lay": [c_i, c_p, c_p, c_sz, c_sz, c_i, c_p, c_p, c_sz, c_i],
        "tsqr_selftest_f64_lsq_lay": [c_i, c_i, c_p, c_p, c_sz, c_p, c_sz, c_sz, c_i, c_i, c_p, c_p, c_p, c_sz, c_i],
    }
    for name, args in sig.items():
        getattr(L, name).restype = c_i
        getattr(L, name).argtypes = args
    return L, torch


def put(torch, mat, layout, pad, offset):
    """mat on the device in the given layout -> (pool, address, leading dimension).  Column-major: ld = rows + pad; row-major: ld = columns
    + pad, which is the column-major image of the transpose.  NaN in the padding, in front of the matrix and sixteen elements behind it."""
    src = mat if layout == COL else mat.T
    ld = src.shape[0] + pad
    pool, ptr = upload(torch, np.ascontiguousarray(src), ld, pad=NAN, offset=offset, slack=16, dtype=np.float64)
    return pool, ptr, ld


def nblocks_of(m, rows_per_unit, nwaves):
    """workgroups of the plan (f64_plan / f64r_plan: at most 2048 waves, a whole number of units each) or of the override"""
    if not nwaves:
        units = -(-m // rows_per_unit)
        per = max(1, -(-units // 2048))
        nwaves = -(-units // per)
    return (nwaves + 3) // 4


def run_pass(st, kind, a, a_lay, pad, nwaves, z=None, x=None, b=None, b_lay=COL):
    """one pass -> (the int64 image of every partial, of the reduced sum); checks the sentinels and that no operand was written"""
    L, torch = st
    m, n = a.shape
    nt = (n + 15) // 16
    tiles = nt if kind == "lsq" else nt * (nt + 1) // 2
    nblocks = nblocks_of(m, 64 if kind == "gram" else 16, nwaves)
    cap = nblocks * tiles * 256
    offset = 1 if pad & 1 else 0                              # (odd leading dimensions go with an 8-byte aligned base)
    apool, ap, lda = put(torch, a, a_lay, pad, offset)
    pools = [apool]
    part = torch.full((cap + 8,), SENT, dtype=torch.float64, device="cuda")
    out = torch.full((tiles * 256 + 1 + 8,), SENT, dtype=torch.float64, device="cuda")
    if kind == "gram":
        rc = L.tsqr_selftest_f64_gram_lay(a_lay, out.data_ptr(), ap, lda, m, n, part.data_ptr(), cap, nwaves)
    else:
        zpool, zp = z_dev(torch, z, n)
        pools.append(zpool)
        if kind == "gramq":
            rc = L.tsqr_selftest_f64_gramq_lay(a_lay, out.data_ptr(), ap, lda, m, n, zp, part.data_ptr(), cap, nwaves)
        else:
            bpool, bp, ldb = put(torch, b, b_lay, pad, offset)
            xpool, xp = x_dev(torch, x, n) if x is not None else (torch.zeros(1, dtype=torch.float64, device="cuda"), None)
            pools += [bpool, xpool]
            rc = L.tsqr_selftest_f64_lsq_lay(a_lay, b_lay, out.data_ptr(), ap, lda, bp, ldb, m, n, b.shape[1], zp, xp,
                                             part.data_ptr(), cap, nwaves)
    assert rc == 0, (rc, kind, m, n, a_lay, b_lay, pad, nwaves)
    p, o = part.cpu().numpy(), out.cpu().numpy()
    assert np.all(p[cap:] == SENT) and np.all(o[tiles * 256 + 1:] == SENT) and o[tiles * 256] == float(m)
    assert not np.isnan(p[:cap]).any(), ("NaN in a partial: padding or a row behind m was used", kind, m, n, a_lay, b_lay, pad, nwaves)
    return p[:cap].view(np.int64).copy(), o[:tiles * 256].view(np.int64).copy()


def same(got, want, what):
    assert np.array_equal(got[0], want[0]), ("a workgroup partial differs",) + what
    assert np.array_equal(got[1], want[1]), ("the reduced sum differs",) + what


def waves_for(m):
    """3 everywhere (the issue's override); the product's plan and five waves (two workgroups, three idle waves) where there are tiles for them"""
    return [3] + ([0, 5] if m >= 130 else [])


@pytest.mark.parametrize("m", MS)
def test_gram_rowmajor_partials_equal_colmajor(st, m):
    for n in [n for n in NS if n <= m]:
        a = np.random.default_rng(100 * m + n).standard_normal((m, n))
        for nwaves in waves_for(m):
            want = run_pass(st, "gram", a, COL, 0, nwaves)
            for pad in PADS:
                same(run_pass(st, "gram", a, ROW, pad, nwaves), want, (m, n, pad, nwaves))


@pytest.mark.parametrize("m", MS)
def test_gramq_rowmajor_partials_equal_colmajor(st, m):
    for n in [n for n in NS if n <= m]:
        rng = np.random.default_rng(200 * m + n)
        a, z = rng.standard_normal((m, n)), np.triu(rng.standard_normal((n, n)))
        for nwaves in waves_for(m):
            want = run_pass(st, "gramq", a, COL, 0, nwaves, z=z)
            for pad in PADS:
                same(run_pass(st, "gramq", a, ROW, pad, nwaves, z=z), want, (m, n, pad, nwaves))


@pytest.mark.parametrize("m", MS)
def test_lsq_all_layout_pairs_partials_equal_colmajor(st, m):
    for n in [n for n in NS if n <= m]:
        for nrhs in NRHS:
            rng = np.random.default_rng(300 * m + 17 * n + nrhs)
            a, z = rng.standard_normal((m, n)), np.triu(rng.standard_normal((n, n)))
            b = rng.standard_normal((m, nrhs))
            x = rng.standard_normal((n, nrhs)) if (n + nrhs) & 1 else None       # (null x: the first pass of the entry)
            for nwaves in waves_for(m) if nrhs == 5 else [3]:
                want = run_pass(st, "lsq", a, COL, 0, nwaves, z=z, x=x, b=b, b_lay=COL)
                for a_lay, b_lay in ((COL, COL), (ROW, COL), (COL, ROW), (ROW, ROW)):
                    for pad in PADS:
                        if (a_lay, b_lay, pad) != (COL, COL, 0):
                            same(run_pass(st, "lsq", a, a_lay, pad, nwaves, z=z, x=x, b=b, b_lay=b_lay), want,
                                 (m, n, nrhs, a_lay, b_lay, pad, nwaves))


def test_lsq_nonfinite_b_spoils_its_row_in_every_layout(st):
    """one NaN in B: the identity k-blocks carry it into every right-hand side of its row, row-major B included -- the partials stay
    those of the column-major kernel (NaN payloads aside: compared with equal_nan)"""
    L, torch = st
    m, n, nrhs = 130, 33, 5
    rng = np.random.default_rng(9)
    a, z, b = rng.standard_normal((m, n)), np.triu(rng.standard_normal((n, n))), rng.standard_normal((m, nrhs))
    b[77, 2] = NAN

    def partials(a_lay, b_lay):
        apool, ap, lda = put(torch, a, a_lay, 1, 1)
        bpool, bp, ldb = put(torch, b, b_lay, 1, 1)
        zpool, zp = z_dev(torch, z, n)
        cap = 3 * 256
        part = torch.full((cap,), SENT, dtype=torch.float64, device="cuda")
        out = torch.full((3 * 256 + 1,), SENT, dtype=torch.float64, device="cuda")
        assert L.tsqr_selftest_f64_lsq_lay(a_lay, b_lay, out.data_ptr(), ap, lda, bp, ldb, m, n, nrhs, zp, None, part.data_ptr(), cap, 3) == 0
        return part.cpu().numpy()

    want = partials(COL, COL)
    assert np.isnan(want).any()
    for pair in ((ROW, COL), (COL, ROW), (ROW, ROW)):
        assert np.array_equal(partials(*pair), want, equal_nan=True), pair

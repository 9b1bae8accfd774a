"""The layout forms of the fp64 apply pass (apply_f64_kernel<NT, AROW, QROW>: AROW the layout of the operand read, QROW of the operand
written), through the test library's tsqr_selftest_f64_apply_lay, over all four layout pairs:

  exact     integer A times an exact inverse pair (tests/pass_refs_f64.py, budget asserted): the result equals a @ z bit for bit for
            every tile count, every m mod 32 tail, contiguous and padded leading dimensions, the product's grid and grids of one and
            three workgroups, out of place and -- for the two equal-layout pairs -- in place;
  bounds    A carries NaN in its leading-dimension padding, in front of its first element and behind its last row (so a read of any of
            them shows in Q), Q a sentinel everywhere outside the m x n block (so a write to any of it shows);
  Gaussian  a general upper triangular Z on Gaussian A: the four pairs give IDENTICAL bits, and those of the plain hook
            (tsqr_selftest_f64_apply, the column-major kernel of tests/test_gpu_f64_passes.py).  A row-major Q is formed with the MFMA
            operands swapped -- the same products, each with its factors exchanged, summed in the same order -- and this is the check on
            the device that the swap changes no bit."""
import ctypes
import os

import numpy as np
import pytest

from tests import pass_refs_f64 as p64
from tests.test_gpu_f64_r_passes import z_dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
SENT = -777.0
LD = np.longdouble
COL, ROW = 0, 1
PAIRS = ((COL, COL), (ROW, COL), (COL, ROW), (ROW, ROW))
c_sz, c_p, c_i = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int

NS = [1, 7, 16, 17, 33, 49, 51, 64]
PADS = [0, 1, 13]                          # row-major: ld = n + pad; column-major: ld = m + pad
WGS = [0, 1, 3]


@pytest.fixture(scope="module")
def st():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    L = ctypes.CDLL(os.path.join(ROOT, "tsqr_gpu_amd", "csrc", "libtsqr_selftest.so"))
    for name, args in {"tsqr_selftest_f64_apply_lay": [c_i, c_i, c_p, c_sz, c_p, c_sz, c_sz, c_i, c_p, c_i],
                       "tsqr_selftest_f64_apply": [c_p, c_sz, c_p, c_sz, c_sz, c_i, c_p, c_i]}.items():
        getattr(L, name).restype = c_i
        getattr(L, name).argtypes = args
    return L, torch


def ms_for(n):
    base = 32 * -(-n // 32)                # m = 32 k + tail >= n for every tail and every NT
    return [base + t for t in (0, 1, 15, 16, 17, 31)] + [1015, 4097]


class Operand:
    """An m x n matrix in a host pool in the given layout: `lines` contiguous runs of `length` elements (columns of m, or rows of n), ld
    apart, the first at element `offset`; everything else of the pool -- the offset, the padding between the runs, and behind the last run
    room for 32 more rows -- is `fill`."""

    def __init__(self, m, n, layout, pad, fill, mat=None):
        self.m, self.n, self.layout = m, n, layout
        self.lines, self.length = (m, n) if layout == ROW else (n, m)
        self.ld = self.length + pad
        self.offset = 1 if self.ld & 1 else 0             # (odd leading dimensions go with a base that is only 8-byte aligned)
        slack = 32 * self.ld + 16 if layout == ROW else 48
        self.host = np.full(self.offset + (self.lines - 1) * self.ld + self.length + slack, fill)
        self.idx = self.offset + np.arange(self.lines)[:, None] * self.ld + np.arange(self.length)[None, :]
        if mat is not None:
            self.host[self.idx] = mat if layout == ROW else mat.T

    def upload(self, torch):
        self.pool = torch.from_numpy(self.host).cuda()
        self.ptr = self.pool.data_ptr() + 8 * self.offset
        return self

    def download(self):
        """(the matrix, everything of the pool outside it)"""
        host = self.pool.cpu().numpy()
        mat = host[self.idx]
        outside = np.ones(host.size, bool)
        outside[self.idx.reshape(-1)] = False
        return (mat if self.layout == ROW else mat.T).copy(), host[outside]


def apply_lay(st, a_op, q_op, zp, wgs):
    L, _ = st
    rc = L.tsqr_selftest_f64_apply_lay(a_op.layout, q_op.layout, q_op.ptr, q_op.ld, a_op.ptr, a_op.ld, a_op.m, a_op.n, zp, wgs)
    assert rc == 0, (rc, a_op.layout, q_op.layout, a_op.m, a_op.n, a_op.ld, q_op.ld, wgs)


def run(st, a, zp, a_lay, q_lay, pad, wgs, a_cache=None):
    """out of place -> Q; checks that nothing outside Q's m x n block was written"""
    _, torch = st
    m, n = a.shape
    key = (a_lay, pad)
    if a_cache is None or key not in a_cache:
        a_op = Operand(m, n, a_lay, pad, NAN, a).upload(torch)
        if a_cache is not None:
            a_cache[key] = a_op
    else:
        a_op = a_cache[key]
    q_op = Operand(m, n, q_lay, pad + (2 if q_lay == COL else 0), SENT).upload(torch)
    apply_lay(st, a_op, q_op, zp, wgs)
    q, outside = q_op.download()
    assert np.all(outside == SENT), ("Q's padding was written", m, n, a_lay, q_lay, pad, wgs)
    return q


def run_in_place(st, a, zp, lay, pad, wgs):
    _, torch = st
    m, n = a.shape
    op = Operand(m, n, lay, pad, NAN, a).upload(torch)
    apply_lay(st, op, op, zp, wgs)
    q, outside = op.download()
    assert np.all(np.isnan(outside)), ("in place: the padding of A was written", m, n, lay, pad, wgs)
    return q


@pytest.mark.parametrize("n", NS)
def test_apply_layouts_exact_bit_for_bit(st, n):
    _, torch = st
    rng = np.random.default_rng(1000 + n)
    amax = bmax = (1 << 20) - 1
    split = n // 2
    p64.assert_apply_budget(amax, split, bmax)
    _, z = p64.exact_inverse_pair64(rng, n, split, bmax)
    zpool, zp = z_dev(torch, z, n)
    for m in ms_for(n):
        a = rng.integers(-amax, amax + 1, size=(m, n)).astype(np.float64)
        ref = a @ z
        assert np.array_equal(ref.astype(LD), p64.matmul_ld(a, z))
        cache = {}
        for pad in PADS:
            for wgs in WGS:
                for a_lay, q_lay in PAIRS:
                    q = run(st, a, zp, a_lay, q_lay, pad, wgs, cache)
                    assert np.array_equal(q, ref), (m, n, a_lay, q_lay, pad, wgs)
                for lay in (COL, ROW):
                    assert np.array_equal(run_in_place(st, a, zp, lay, pad, wgs), ref), (m, n, lay, pad, wgs, "in place")
    del zpool


def test_apply_layouts_read_no_padding_and_no_row_behind_m(st):
    """NaN between n and the leading dimension, in front of A and in the 32 rows behind row m: every pair's Q stays finite and exact;
    the hook refuses what the entry refuses"""
    L, torch = st
    rng = np.random.default_rng(5)
    m, n = 77, 19
    amax = bmax = (1 << 20) - 1
    _, z = p64.exact_inverse_pair64(rng, n, 9, bmax)
    zpool, zp = z_dev(torch, z, n)
    a = rng.integers(-amax, amax + 1, size=(m, n)).astype(np.float64)
    for a_lay, q_lay in PAIRS:
        for pad in (1, 13):
            q = run(st, a, zp, a_lay, q_lay, pad, 1)
            assert np.isfinite(q).all(), (a_lay, q_lay, pad)
            assert np.array_equal(q, a @ z), (a_lay, q_lay, pad)
    op = Operand(m, n, ROW, 0, NAN, a).upload(torch)
    for al, ql, ldq, lda in ((2, ROW, n, n), (ROW, -1, n, n), (ROW, ROW, n - 1, n), (ROW, ROW, n, n - 1), (COL, ROW, n, m - 1),
                             (ROW, COL, m - 1, n), (ROW, COL, m, m), (ROW, ROW, n + 1, n)):       # the last two: q == a, mixed or unequal ld
        assert L.tsqr_selftest_f64_apply_lay(al, ql, op.ptr, ldq, op.ptr, lda, m, n, zp, 1) == -100, (al, ql, ldq, lda)
    del zpool


@pytest.mark.parametrize("m,n", [(1055, 64), (4097, 33)])
def test_apply_layout_pairs_identical_bits_on_gaussian(st, m, n):
    """general data: nothing is exact, so equal bits mean the same products summed in the same order in all four instantiations"""
    L, torch = st
    rng = np.random.default_rng(m + n)
    a = rng.standard_normal((m, n))
    z = np.triu(rng.standard_normal((n, n)))
    zpool, zp = z_dev(torch, z, n)
    a_op = Operand(m, n, COL, 0, NAN, a).upload(torch)
    q_op = Operand(m, n, COL, 0, SENT).upload(torch)
    assert L.tsqr_selftest_f64_apply(q_op.ptr, q_op.ld, a_op.ptr, a_op.ld, m, n, zp, 0) == 0          # the plain hook: today's kernel
    want, _ = q_op.download()
    assert np.isfinite(want).all()
    err = np.abs(np.asarray(want.astype(LD) - p64.matmul_ld(a, z), np.float64))
    assert np.all(err <= p64.apply_bound(a, z)), "the column-major reference itself is off"
    for a_lay, q_lay in PAIRS:
        for pad, wgs in ((0, 0), (13, 3)):
            q = run(st, a, zp, a_lay, q_lay, pad, wgs)
            assert np.array_equal(q.view(np.int64), want.view(np.int64)), (m, n, a_lay, q_lay, pad, wgs)
    for lay in (COL, ROW):
        q = run_in_place(st, a, zp, lay, 1, 0)
        assert np.array_equal(q.view(np.int64), want.view(np.int64)), (m, n, lay, "in place")
    del zpool

"""The layout forms of the two passes of the wide fp64 entry that touch A or Q (gram_wide_f64_kernel<AROW>,
apply_wide_f64_kernel<AROW, QROW>, tsqr_f64_wide.hip), through the test library's tsqr_selftest_f64w_gram_lay and
tsqr_selftest_f64w_apply_lay, against the plain entries (the column-major kernels of tests/test_gpu_f64_passes.py) on the transposed
copy -- BIT FOR BIT, on Gaussian data, where nothing is exact and equal bits mean the same values in the same registers and the same
products summed in the same order:

  Gram     every partial and the summed G of a row-major A.  lda == n: a column >= n of the zero-padded last block, if it were loaded,
           would be the next row's data (and beyond the allocation on the last row); lda = n + 3: NaN in the padding.  A NaN guard band
           lies in front of the first element and behind the last row.  The product's partition and slices of three 16-row chunks.
  apply    all four layout pairs, and in place for the two equal-layout pairs, on a random upper triangular Z in the block store.  A
           carries NaN in its padding and guard bands, Q is NaN everywhere before the call and must still be NaN outside the m x n block.

Shapes: a last block of 1 column (65) and of 36 (100), three full blocks (192); row tails against 16, against 32 and against the slice."""
import ctypes
import os

import numpy as np
import pytest

from tests import pass_refs_f64 as p64
from tests.test_gpu_f64_apply_rowmajor_passes import COL, PAIRS, ROW, Operand

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
c_sz, c_p, c_i = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int
SHAPES = [(65, 65), (200, 65), (1000, 100), (777, 192)]


@pytest.fixture(scope="module")
def st():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    L = ctypes.CDLL(os.path.join(ROOT, "tsqr_gpu_amd", "csrc", "libtsqr_selftest.so"))
    for name, args in {"tsqr_selftest_f64w_plan": [c_sz, c_sz, c_p],
                       "tsqr_selftest_f64w_gram": [c_p, c_p, c_sz, c_sz, c_i, c_p, c_sz, c_sz],
                       "tsqr_selftest_f64w_gram_lay": [c_i, c_p, c_p, c_sz, c_sz, c_i, c_p, c_sz, c_sz],
                       "tsqr_selftest_f64w_apply": [c_p, c_sz, c_p, c_sz, c_sz, c_i, c_p],
                       "tsqr_selftest_f64w_apply_lay": [c_i, c_i, c_p, c_sz, c_p, c_sz, c_sz, c_i, c_p]}.items():
        getattr(L, name).restype = c_i
        getattr(L, name).argtypes = args
    return L, torch


def plan(L, m, n):
    out = (ctypes.c_longlong * 20)()
    assert L.tsqr_selftest_f64w_plan(m, n, ctypes.cast(out, c_p)) == 0
    return dict(zip("nb npairs ngroups nslices cps nch bs".split(), out))


class RowOp(Operand):
    """Operand (row-major: m rows of n, ld apart, NaN everywhere else, room for 32 more rows behind the last one) with a NaN band of 64
    doubles in FRONT of the first element too, whatever the parity of ld"""

    def __init__(self, m, n, layout, pad, fill, mat=None):
        Operand.__init__(self, m, n, layout, pad, fill, mat)
        shift = 64 - self.offset
        self.host = np.concatenate([np.full(shift, fill), self.host])
        self.idx = self.idx + shift
        self.offset = 64


@pytest.mark.parametrize("m,n", SHAPES)
def test_wide_gram_row_major_partials_bit_for_bit(st, m, n):
    L, torch = st
    rng = np.random.default_rng(m * 1000 + n)
    a = rng.standard_normal((m, n))
    pl = plan(L, m, n)
    col = Operand(m, n, COL, 0, NAN, a).upload(torch)
    for cps in (0, 3):
        nslices = -(-pl["nch"] // cps) if cps else pl["nslices"]
        cap = nslices * pl["bs"]

        def gram(call):
            part = torch.full((cap + 8,), -777.0, dtype=torch.float64, device="cuda")
            gs = torch.full((pl["bs"] + 1 + 8,), -777.0, dtype=torch.float64, device="cuda")
            assert call(gs.data_ptr(), part.data_ptr()) == 0
            return gs.cpu().numpy(), part.cpu().numpy()

        want_g, want_p = gram(lambda g, p: L.tsqr_selftest_f64w_gram(g, col.ptr, col.ld, m, n, p, cap, cps))
        assert np.isfinite(want_g[:pl["bs"]]).all() and want_g[pl["bs"]] == float(m)
        assert np.all(want_p[cap:] == -777.0) and np.all(want_g[pl["bs"] + 1:] == -777.0)
        full = p64.pack_blocks(a.T @ a, n)
        assert np.allclose(want_g[:pl["bs"]], full, rtol=0, atol=1e-9 * m), "the column-major reference itself is off"
        for pad in (0, 3):                               # lda == n: a masked column would be the next row; lda = n + 3: NaN padding
            row = RowOp(m, n, ROW, pad, NAN, a).upload(torch)
            assert row.ld == n + pad
            got_g, got_p = gram(lambda g, p: L.tsqr_selftest_f64w_gram_lay(ROW, g, row.ptr, row.ld, m, n, p, cap, cps))
            assert np.array_equal(got_p.view(np.int64), want_p.view(np.int64)), (m, n, cps, pad, "partials")
            assert np.array_equal(got_g.view(np.int64), want_g.view(np.int64)), (m, n, cps, pad, "summed G")
        # the _lay hook at layout 0 is the plain hook
        got_g, got_p = gram(lambda g, p: L.tsqr_selftest_f64w_gram_lay(COL, g, col.ptr, col.ld, m, n, p, cap, cps))
        assert np.array_equal(got_g.view(np.int64), want_g.view(np.int64)) and np.array_equal(got_p.view(np.int64), want_p.view(np.int64))
    # what the hook refuses: a layout other than 0 / 1, a row-major ld below n, a column-major ld below m
    z = torch.zeros(8, dtype=torch.float64, device="cuda")
    for lay, lda in ((2, m), (-1, n), (ROW, n - 1), (COL, m - 1)):
        assert L.tsqr_selftest_f64w_gram_lay(lay, z.data_ptr(), col.ptr, lda, m, n, z.data_ptr(), 8, 0) == -100


@pytest.mark.parametrize("m,n", SHAPES)
def test_wide_apply_layout_pairs_bit_for_bit(st, m, n):
    L, torch = st
    rng = np.random.default_rng(m * 1000 + n + 1)
    a = rng.standard_normal((m, n))
    z = np.triu(rng.standard_normal((n, n)))
    zw = torch.from_numpy(p64.pack_blocks(z, n)).cuda()
    zp = zw.data_ptr()
    a_col = Operand(m, n, COL, 0, NAN, a).upload(torch)
    q_col = Operand(m, n, COL, 0, NAN).upload(torch)
    assert L.tsqr_selftest_f64w_apply(q_col.ptr, q_col.ld, a_col.ptr, a_col.ld, m, n, zp) == 0           # the plain hook
    want, _ = q_col.download()
    assert np.isfinite(want).all()
    ref = a @ z
    assert np.abs(want - ref).max() <= 64 * n * 2.0 ** -53 * (np.abs(a) @ np.abs(z)).max(), "the column-major reference itself is off"

    def operand(lay, pad, mat=None):
        return (RowOp if lay == ROW else Operand)(m, n, lay, pad, NAN, mat).upload(torch)

    for pad in (0, 3):
        for a_lay, q_lay in PAIRS:
            a_op, q_op = operand(a_lay, pad, a), operand(q_lay, pad)
            assert L.tsqr_selftest_f64w_apply_lay(a_lay, q_lay, q_op.ptr, q_op.ld, a_op.ptr, a_op.ld, m, n, zp) == 0
            q, outside = q_op.download()
            assert np.array_equal(q.view(np.int64), want.view(np.int64)), (m, n, a_lay, q_lay, pad)
            assert np.all(np.isnan(outside)), ("Q's padding or guard rows were written", m, n, a_lay, q_lay, pad)
        for lay in (COL, ROW):
            op = operand(lay, pad, a)
            assert L.tsqr_selftest_f64w_apply_lay(lay, lay, op.ptr, op.ld, op.ptr, op.ld, m, n, zp) == 0
            q, outside = op.download()
            assert np.array_equal(q.view(np.int64), want.view(np.int64)), (m, n, lay, pad, "in place")
            assert np.all(np.isnan(outside)), ("in place: the padding of A was written", m, n, lay, pad)
    # what the hook refuses: layouts, leading dimensions, q == a with mixed layouts or unequal strides
    op = operand(ROW, 0, a)
    for al, ql, ldq, lda in ((2, ROW, n, n), (ROW, -1, n, n), (ROW, ROW, n - 1, n), (ROW, ROW, n, n - 1), (COL, ROW, n, m - 1),
                             (ROW, COL, m - 1, n), (ROW, COL, m, m), (ROW, ROW, n + 1, n)):
        assert L.tsqr_selftest_f64w_apply_lay(al, ql, op.ptr, ldq, op.ptr, lda, m, n, zp) == -100, (al, ql, ldq, lda)

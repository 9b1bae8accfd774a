"""tsqr_mi_r_f64_lay and tsqr_mi_lstsq_f64_lay on the GPU: R, X, the state and tsqr_mi_last_sweeps_f64 of a call on row-major operands
equal, BIT FOR BIT, those of the column-major entries (tsqr_mi_r_f64, tsqr_mi_lstsq_f64) on the same matrices -- the statement of
include/tsqr_mi.h.  Nothing here measures accuracy: the column-major entries have their own tests (tests/test_gpu_f64_r.py,
tests/test_gpu_f64_lstsq.py), and equal bits carry every one of their statements over.  Inputs: tests/pass_refs_f64_lsq.accuracy_input --
Gaussian (one sweep; reorth = 1: the second sweep streams A through gramq), cond 1e12 (the shifted path: three or more sweeps, Z
accumulated by zmul).  Row-major operands carry NaN between n and lda (nrhs and ldb) and behind the last row.  Then the wrapper:
blockqr.lstsq_f64 on a contiguous tensor allocates no copy of A, and blockqr.r_f64(row_major=True)."""
import ctypes
import functools

import numpy as np
import pytest

from tests import pass_refs_f64_lsq as pl

pytestmark = pytest.mark.gpu
NAN = float("nan")
COL, ROW = 0, 1
vp = ctypes.c_void_p


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@functools.lru_cache(maxsize=None)
def inputs(m, n, nrhs, cond):
    """(A, B) of tests/pass_refs_f64_lsq.py, computed once, shared, never written"""
    a, b = pl.accuracy_input(m, n, nrhs, cond, "gaussian")
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def device_operand(torch, mat, layout, pad):
    """mat on the device -> (tensor that owns the storage, leading dimension).  Row-major: rows of cols + pad elements and two more rows
    behind the last, NaN wherever the matrix is not; column-major: columns of rows + pad elements, NaN padding."""
    rows, cols = mat.shape
    if layout == ROW:
        t = torch.full((rows + 2, cols + pad), NAN, dtype=torch.float64, device="cuda")
        t[:rows, :cols] = torch.from_numpy(np.array(mat)).cuda()
        return t, cols + pad
    t = torch.full((cols, rows + pad), NAN, dtype=torch.float64, device="cuda")
    t[:, :rows] = torch.from_numpy(np.array(mat.T, order="C")).cuda()
    return t, rows + pad


def lstsq_call(bq, a, b, a_lay, b_lay, reorth, refine, pad=0, stream=None, legacy=False):
    """the C entry on device copies of a and b -> (state, sweeps, X, R as host arrays); legacy: tsqr_mi_lstsq_f64 itself (column-major)"""
    torch = _torch()
    L = bq.lib()
    m, n = a.shape
    nrhs = b.shape[1]
    ad, lda = device_operand(torch, a, a_lay, pad)
    bd, ldb = device_operand(torch, b, b_lay, pad)
    before = ad.clone(), bd.clone()
    x = torch.full((nrhs, n), NAN, dtype=torch.float64, device="cuda")
    r = torch.full((n, n), NAN, dtype=torch.float64, device="cuda")
    wq = torch.empty(L.tsqr_mi_working_q_size_f64_lstsq(m, n, nrhs), dtype=torch.float64, device="cuda")
    wr = torch.empty(L.tsqr_mi_working_r_size_f64_lstsq(m, n, nrhs), dtype=torch.float64, device="cuda")
    s = stream if stream is not None else torch.cuda.current_stream()
    tail = (vp(x.data_ptr()), n, vp(r.data_ptr()), n, vp(ad.data_ptr()), lda, vp(bd.data_ptr()), ldb, m, n, nrhs,
            vp(wq.data_ptr()), vp(wr.data_ptr()), vp(s.cuda_stream))
    if legacy:
        assert (a_lay, b_lay) == (COL, COL)
        state = L.tsqr_mi_lstsq_f64(reorth, refine, *tail)
    else:
        state = L.tsqr_mi_lstsq_f64_lay(a_lay, b_lay, reorth, refine, *tail)
    sweeps = L.tsqr_mi_last_sweeps_f64()
    torch.cuda.synchronize()
    for t, t0 in zip((ad, bd), before):
        assert torch.equal(t.view(torch.int64), t0.view(torch.int64)), "an operand was written"
    return state, sweeps, x.t().cpu().numpy().copy(), r.t().cpu().numpy().copy()


def r_call(bq, a, a_lay, reorth, pad=0, legacy=False):
    torch = _torch()
    L = bq.lib()
    m, n = a.shape
    ad, lda = device_operand(torch, a, a_lay, pad)
    r = torch.full((n, n), NAN, dtype=torch.float64, device="cuda")
    wq = torch.empty(L.tsqr_mi_working_q_size_f64_r(m, n), dtype=torch.float64, device="cuda")
    wr = torch.empty(L.tsqr_mi_working_r_size_f64_r(m, n), dtype=torch.float64, device="cuda")
    tail = (vp(r.data_ptr()), n, vp(ad.data_ptr()), lda, m, n, vp(wq.data_ptr()), vp(wr.data_ptr()), vp(torch.cuda.current_stream().cuda_stream))
    state = L.tsqr_mi_r_f64(reorth, *tail) if legacy else L.tsqr_mi_r_f64_lay(a_lay, reorth, *tail)
    sweeps = L.tsqr_mi_last_sweeps_f64()
    torch.cuda.synchronize()
    return state, sweeps, r.t().cpu().numpy().copy()


def bits(x):
    return np.ascontiguousarray(x).view(np.int64)


# (name, cond, reorth, what the ladder has to do): sweeps % 100 is the sweep count, + 100 marks the shifted path
LADDERS = [("gauss", None, 0, lambda s: s == 1), ("gauss_reorth", None, 1, lambda s: s == 2), ("cond1e12", 1e12, 0, lambda s: s >= 103)]


@pytest.mark.parametrize("m,n,nrhs", [(9211, 51, 5), (4096, 64, 16)])
@pytest.mark.parametrize("name,cond,reorth,expect", LADDERS, ids=[l[0] for l in LADDERS])
def test_r_f64_lay_bits_equal_colmajor(bq, m, n, nrhs, name, cond, reorth, expect):
    a, _ = inputs(m, n, nrhs, cond)
    want = r_call(bq, a, COL, reorth, legacy=True)
    assert want[0] == 0 and expect(want[1]), want[:2]
    for lay, pad in ((COL, 3), (ROW, 0), (ROW, 1), (ROW, 13)):
        got = r_call(bq, a, lay, reorth, pad=pad)
        assert got[:2] == want[:2], (lay, pad, got[:2], want[:2])
        assert np.array_equal(bits(got[2]), bits(want[2])), ("R differs", lay, pad)


@pytest.mark.parametrize("refine", [0, 1])
@pytest.mark.parametrize("m,n,nrhs", [(9211, 51, 5), (4096, 64, 16)])
@pytest.mark.parametrize("name,cond,reorth,expect", LADDERS, ids=[l[0] for l in LADDERS])
def test_lstsq_f64_lay_bits_equal_colmajor(bq, m, n, nrhs, name, cond, reorth, expect, refine):
    a, b = inputs(m, n, nrhs, cond)
    want = lstsq_call(bq, a, b, COL, COL, reorth, refine, legacy=True)
    assert want[0] == 0 and expect(want[1]), want[:2]
    for a_lay, b_lay, pad in ((COL, COL, 0), (ROW, ROW, 0), (ROW, COL, 1), (COL, ROW, 1), (ROW, ROW, 13)):
        got = lstsq_call(bq, a, b, a_lay, b_lay, reorth, refine, pad=pad)
        assert got[:2] == want[:2], (a_lay, b_lay, pad, got[:2], want[:2])
        assert np.array_equal(bits(got[3]), bits(want[3])), ("R differs", a_lay, b_lay, pad)
        assert np.array_equal(bits(got[2]), bits(want[2])), ("X differs", a_lay, b_lay, pad)


def test_second_chunk_and_second_tile_131139x64(bq):
    """with the product's own plans a wave takes a second 64-row chunk of the Gram pass (cdiv(m, 64) = 2050 > 2048 waves) and several
    16-row tiles of gramq and lsq (8197 tiles), and the last chunk and the last tile are ragged (m = 3 mod 16): the strides over chunks
    and tiles and the prefetch, as the entries launch them"""
    m, n, nrhs = 131139, 64, 16
    assert -(-m // 64) > 2048 and -(-m // 16) > 2048 and m % 16
    a, b = inputs(m, n, nrhs, None)
    want = lstsq_call(bq, a, b, COL, COL, 1, 1, legacy=True)
    got = lstsq_call(bq, a, b, ROW, ROW, 1, 1, pad=1)
    assert want[0] == 0 and want[1] == 2 and got[:2] == want[:2]
    assert np.array_equal(bits(got[3]), bits(want[3])) and np.array_equal(bits(got[2]), bits(want[2]))


def test_nan_in_a_is_state_3_in_both_layouts(bq):
    a, b = inputs(9211, 51, 5, None)
    a = np.array(a)
    a[517, 3] = NAN
    want = lstsq_call(bq, a, b, COL, COL, 0, 1, legacy=True)
    got = lstsq_call(bq, a, b, ROW, ROW, 0, 1, pad=1)
    assert want[0] == 3 == bq.error_not_finite and got[:2] == want[:2]
    assert r_call(bq, a, ROW, 0, pad=1)[:2] == r_call(bq, a, COL, 0, legacy=True)[:2] == (3, want[1])


def test_nan_in_b_spoils_x_alike(bq):
    """one NaN in B: state 0 and every column of X non-finite, as include/tsqr_mi.h says of the column-major entry; the row-major X is the
    same (NaN payloads aside)"""
    a, b = inputs(9211, 51, 5, None)
    b = np.array(b)
    b[4242, 2] = NAN
    want = lstsq_call(bq, a, b, COL, COL, 0, 1, legacy=True)
    assert want[0] == 0 and np.isnan(want[2]).any()
    for a_lay, b_lay in ((ROW, ROW), (COL, ROW)):
        got = lstsq_call(bq, a, b, a_lay, b_lay, 0, 1, pad=1)
        assert got[:2] == want[:2]
        assert np.array_equal(got[2], want[2], equal_nan=True) and np.array_equal(bits(got[3]), bits(want[3]))


def test_side_stream(bq):
    torch = _torch()
    a, b = inputs(4096, 64, 16, None)
    want = lstsq_call(bq, a, b, COL, COL, 1, 1, legacy=True)
    side = torch.cuda.Stream()
    got = lstsq_call(bq, a, b, ROW, ROW, 1, 1, stream=side)
    assert got[:2] == want[:2] and np.array_equal(bits(got[2]), bits(want[2])) and np.array_equal(bits(got[3]), bits(want[3]))


def test_wrapper_reads_row_major_tensors_where_they_lie(bq):
    """blockqr.lstsq_f64 on plain contiguous tensors, a padded row-major view and a one-dimensional b; blockqr.r_f64(row_major=True):
    the bits of the column-major call"""
    torch = _torch()
    m, n, nrhs = 9211, 51, 5
    a, b = inputs(m, n, nrhs, None)
    want = lstsq_call(bq, a, b, COL, COL, 0, 1, legacy=True)
    ad, bd = torch.from_numpy(np.array(a)).cuda(), torch.from_numpy(np.array(b)).cuda()
    x, r = bq.lstsq_f64(ad, bd)
    assert bq.last_sweeps_f64() == want[1]
    assert np.array_equal(bits(x.cpu().numpy()), bits(want[2])) and np.array_equal(bits(r.cpu().numpy()), bits(want[3]))
    wide = torch.full((m, n + 3), NAN, dtype=torch.float64, device="cuda")
    wide[:, :n] = ad
    x2, r2 = bq.lstsq_f64(wide[:, :n], bd)                  # rows padded: stride(0) = n + 3
    assert torch.equal(x2, x) and torch.equal(r2, r)
    xv, _ = bq.lstsq_f64(ad, bd[:, 1])                      # a one-dimensional b (a strided column of B: used where it lies)
    want1 = lstsq_call(bq, a, np.ascontiguousarray(b[:, 1:2]), COL, COL, 0, 1, legacy=True)
    assert xv.shape == (n,) and np.array_equal(bits(xv.cpu().numpy()), bits(want1[2][:, 0]))
    xc, _ = bq.lstsq_f64(ad[:, ::2], bd)                    # neither rows nor columns contiguous: copied once, as before
    want2 = lstsq_call(bq, np.ascontiguousarray(a[:, ::2]), b, COL, COL, 0, 1, legacy=True)
    assert np.array_equal(bits(xc.cpu().numpy()), bits(want2[2]))
    rr = torch.empty((n, n), dtype=torch.float64, device="cuda")
    bf = bq.buffer_f64_r(False)
    bf.allocate(m, n)
    assert bq.r_f64(rr, n, ad, n, m, n, bf, row_major=True) == 0
    assert np.array_equal(bits(rr.t().cpu().numpy()), bits(want[3]))
    assert bq.r_f64(rr, n, wide, n + 3, m, n, bf, row_major=True) == 0
    assert np.array_equal(bits(rr.t().cpu().numpy()), bits(want[3]))
    with pytest.raises(ValueError):
        bq.r_f64(rr, n, ad, n - 1, m, n, bf, row_major=True)


def test_wrapper_allocates_no_copy_of_a(bq):
    """a contiguous 65536 x 64 tensor: the peak of allocated memory across lstsq_f64 grows by less than half of A's bytes (a transposing
    copy is all of A's), and A and B keep their bytes"""
    torch = _torch()
    m, n, nrhs = 65536, 64, 16
    g = torch.Generator(device="cuda").manual_seed(3)
    a = torch.randn(m, n, dtype=torch.float64, device="cuda", generator=g)
    b = torch.randn(m, nrhs, dtype=torch.float64, device="cuda", generator=g)
    a0, b0 = a.clone(), b.clone()
    bq.lstsq_f64(a[:1024], b[:1024])                        # (the library and its pinned words are set up outside the measured call)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    x, r = bq.lstsq_f64(a, b)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - base
    print("lstsq_f64 on a contiguous %d x %d tensor: peak allocation grew by %d bytes, A has %d" % (m, n, growth, 8 * m * n))
    assert growth < 8 * m * n // 2, (growth, 8 * m * n)
    assert torch.equal(a.view(torch.int64), a0.view(torch.int64)) and torch.equal(b.view(torch.int64), b0.view(torch.int64))
    assert x.shape == (n, nrhs) and bool(torch.isfinite(x).all())

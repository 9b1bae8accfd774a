"""tsqr_mi_qr_f64_lay on the GPU, through the C entry, blockqr.qr_f64(row_major=True) and blockqr.qr_f64_tensor: Q (read as a matrix), R,
the state and tsqr_mi_last_sweeps_f64 of a call on row-major operands equal, BIT FOR BIT, those of tsqr_mi_qr_f64 on a column-major copy
of the same matrix -- the statement of include/tsqr_mi.h -- over the one-sweep path (Gaussian, reorth 0), the two-sweep path (reorth 1)
and the shifted path (cond 1e6 and 1e12: both beyond the CholeskyQR2 bound cond <= 1 / (8 sqrt(u (m n + n (n + 1)))) = 2.3e4 at
4096 x 64).  The same results are held against the header's own bands, evaluated in fp64 on the device: ||Q^T Q - I||_F <= 1e-11
(1e-12 with reorth = 1), ||A - Q R||_F / ||A||_F <= 1e-13.  Row-major operands carry NaN between n and the leading dimension and behind
the last row, Q a sentinel wherever the matrix is not."""
import ctypes
import functools

import numpy as np
import pytest

from tests import pass_refs_f64_r as p64r

pytestmark = pytest.mark.gpu
NAN = float("nan")
SENT = -777.0
COL, ROW = 0, 1
vp = ctypes.c_void_p

# (name, m, n, cond)
SHAPES = [("gauss_4097x64", 4097, 64, None), ("cond1e6_4096x64", 4096, 64, 1e6), ("cond1e12_4096x64", 4096, 64, 1e12),
          ("gauss_131139x64", 131139, 64, None), ("gauss_777x5", 777, 5, None)]


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@functools.lru_cache(maxsize=None)
def matrix(m, n, cond):
    """computed once, shared, never written"""
    seed = 11 * m + n
    a = np.random.default_rng(seed).standard_normal((m, n)) if cond is None else p64r.cond_matrix(m, n, cond, seed)
    a.setflags(write=False)
    return a


def device_operand(torch, rows, cols, layout, pad, fill, mat=None):
    """-> (tensor that owns the storage, leading dimension).  Row-major: rows of cols + pad elements and two more rows behind the last;
    column-major: columns of rows + pad elements; `fill` wherever the matrix is not."""
    if layout == ROW:
        t = torch.full((rows + 2, cols + pad), fill, dtype=torch.float64, device="cuda")
        if mat is not None:
            t[:rows, :cols] = torch.from_numpy(np.array(mat)).cuda()
        return t, cols + pad
    t = torch.full((cols, rows + pad), fill, dtype=torch.float64, device="cuda")
    if mat is not None:
        t[:, :rows] = torch.from_numpy(np.array(mat.T, order="C")).cuda()
    return t, rows + pad


def block(t, rows, cols, layout):
    """the m x n matrix inside a device_operand tensor, as an m x n view"""
    return t[:rows, :cols] if layout == ROW else t[:, :rows].t()


def padding_intact(torch, t, rows, cols, layout, fill):
    c = t.clone()
    block(c, rows, cols, layout).fill_(fill)
    return bool(torch.isnan(c).all()) if fill != fill else bool((c == fill).all())


@functools.lru_cache(maxsize=None)
def reference(m, n, cond, reorth):
    """tsqr_mi_qr_f64 itself on the column-major copy -> (state, sweeps, Q, R) with Q and R on the device (m x n, n x n views)"""
    torch = _torch()
    from tsqr_gpu_amd import blockqr as bq
    return qr_call(bq, matrix(m, n, cond), COL, COL, reorth, legacy=True)


def qr_call(bq, a, a_lay, q_lay, reorth, pad=0, legacy=False, in_place=False):
    """the C entry on a device copy of a -> (state, sweeps, Q as an m x n device view, R as an n x n device view)"""
    torch = _torch()
    L = bq.lib()
    m, n = a.shape
    ad, lda = device_operand(torch, m, n, a_lay, pad, NAN, a)
    before = ad.clone()
    if in_place:
        assert a_lay == q_lay
        qd, ldq = ad, lda
    else:
        qd, ldq = device_operand(torch, m, n, q_lay, pad + 2, SENT)
    r = torch.full((n, n), NAN, dtype=torch.float64, device="cuda")
    wq = torch.empty(L.tsqr_mi_working_q_size_f64(m, n), dtype=torch.float64, device="cuda")
    wr = torch.empty(L.tsqr_mi_working_r_size_f64(m, n), dtype=torch.float64, device="cuda")
    tail = (vp(qd.data_ptr()), ldq, vp(r.data_ptr()), n, vp(ad.data_ptr()), lda, m, n, vp(wq.data_ptr()), vp(wr.data_ptr()),
            vp(torch.cuda.current_stream().cuda_stream))
    if legacy:
        assert (a_lay, q_lay) == (COL, COL)
        state = L.tsqr_mi_qr_f64(reorth, *tail)
    else:
        state = L.tsqr_mi_qr_f64_lay(a_lay, q_lay, reorth, *tail)
    sweeps = L.tsqr_mi_last_sweeps_f64()
    torch.cuda.synchronize()
    if in_place:
        assert padding_intact(torch, ad, m, n, a_lay, NAN), "in place: the padding of A was written"
    else:
        assert torch.equal(ad.view(torch.int64), before.view(torch.int64)), "A was written"
        assert padding_intact(torch, qd, m, n, q_lay, SENT), "Q's padding was written"
    return state, sweeps, block(qd, m, n, q_lay), r.t()


def same_bits(torch, x, y):
    return bool(torch.equal(x.contiguous().view(torch.int64), y.contiguous().view(torch.int64)))


def assert_same(torch, got, want, what):
    assert got[:2] == want[:2], (what, got[:2], want[:2])
    assert same_bits(torch, got[3], want[3]), ("R differs",) + what
    assert same_bits(torch, got[2], want[2]), ("Q differs",) + what


def bands(torch, a, q, r, reorth):
    """the header's bands in fp64 on the device (the evaluation's own rounding, about sqrt(m) u per entry, is far below them)"""
    ad = torch.from_numpy(np.array(a)).cuda()
    n = a.shape[1]
    orth = torch.linalg.norm(q.t() @ q - torch.eye(n, dtype=torch.float64, device="cuda")).item()
    res = (torch.linalg.norm(ad - q @ r) / torch.linalg.norm(ad)).item()
    print("||QtQ - I||_F = %.3e   ||A - QR||_F / ||A||_F = %.3e   (reorth %d)" % (orth, res, reorth))
    assert orth <= (1e-12 if reorth else 1e-11), orth
    assert res <= 1e-13, res


@pytest.mark.parametrize("reorth", [0, 1])
@pytest.mark.parametrize("name,m,n,cond", SHAPES, ids=[s[0] for s in SHAPES])
def test_qr_f64_lay_bits_equal_colmajor_and_bands(bq, name, m, n, cond, reorth):
    torch = _torch()
    a = matrix(m, n, cond)
    want = reference(m, n, cond, reorth)
    assert want[0] == 0, want[:2]
    if cond is None:
        assert want[1] == (2 if reorth else 1), want[1]        # Gaussian: one sweep, or CholeskyQR2 when asked
    if cond == 1e12:
        assert want[1] >= 103, want[1]                         # the shifted path
    assert bool(torch.equal(want[3], torch.triu(want[3]))) and bool((torch.diagonal(want[3]) > 0).all())
    for pad in ((0, 1) if m > 100000 else (0, 1, 13)):
        got = qr_call(bq, a, ROW, ROW, reorth, pad=pad)
        assert_same(torch, got, want, (name, reorth, ROW, ROW, pad))
    bands(torch, a, got[2], got[3], reorth)


def test_the_three_paths_are_covered(bq):
    seen = {reference(m, n, cond, reorth)[1] for _, m, n, cond in SHAPES if m < 100000 for reorth in (0, 1)}
    assert 1 in seen and 2 in seen and any(s >= 103 for s in seen), seen


@pytest.mark.parametrize("name,m,n,cond", [SHAPES[0], SHAPES[2], SHAPES[4]], ids=[SHAPES[0][0], SHAPES[2][0], SHAPES[4][0]])
def test_in_place_and_mixed_layouts(bq, name, m, n, cond):
    torch = _torch()
    a = matrix(m, n, cond)
    for reorth in (0, 1):
        want = reference(m, n, cond, reorth)
        got = qr_call(bq, a, ROW, ROW, reorth, pad=3, in_place=True)          # q == a, row-major, lda = n + 3
        assert_same(torch, got, want, (name, reorth, "in place, row-major"))
        got = qr_call(bq, a, COL, COL, reorth, pad=3, in_place=True)          # the layout entry in place on column-major operands
        assert_same(torch, got, want, (name, reorth, "in place, column-major"))
        for a_lay, q_lay in ((COL, ROW), (ROW, COL), (COL, COL)):
            got = qr_call(bq, a, a_lay, q_lay, reorth, pad=1)
            assert_same(torch, got, want, (name, reorth, a_lay, q_lay))


def test_nan_in_a_is_state_3_in_every_layout(bq):
    a = np.array(matrix(4097, 64, None))
    a[517, 3] = NAN
    want = qr_call(bq, a, COL, COL, 0, legacy=True)
    assert want[0] == 3 == bq.error_not_finite
    for a_lay, q_lay in ((ROW, ROW), (COL, ROW), (ROW, COL)):
        assert qr_call(bq, a, a_lay, q_lay, 0, pad=1)[:2] == want[:2], (a_lay, q_lay)
    torch = _torch()
    with pytest.raises(bq.QrError) as e:
        bq.qr_f64_tensor(torch.from_numpy(a).cuda())
    assert e.value.state == bq.error_not_finite


def test_blockqr_qr_f64_row_major_keyword(bq):
    torch = _torch()
    m, n = 4097, 64
    a = matrix(m, n, None)
    want = reference(m, n, None, 1)
    wide = torch.full((m, n + 3), NAN, dtype=torch.float64, device="cuda")
    wide[:, :n] = torch.from_numpy(np.array(a)).cuda()
    q = torch.full((m, n), SENT, dtype=torch.float64, device="cuda")
    r = torch.empty((n, n), dtype=torch.float64, device="cuda")
    bf = bq.buffer_f64(True)
    bf.allocate(m, n)
    assert bq.qr_f64(q, n, r, n, wide, n + 3, m, n, bf, row_major=True) == 0
    assert bq.last_sweeps_f64() == want[1]
    assert same_bits(torch, q, want[2]) and same_bits(torch, r.t(), want[3])
    with pytest.raises(ValueError):
        bq.qr_f64(q, n - 1, r, n, wide, n + 3, m, n, bf, row_major=True)
    with pytest.raises(ValueError):
        bq.qr_f64(q, n, r, n, wide, n + 4, m, n, bf, row_major=True)            # a's span is one row short
    with pytest.raises(ValueError):
        bq.qr_f64(wide, n + 2, r, n, wide, n + 3, m, n, bf, row_major=True)     # q overlaps a without being a
    assert bq.qr_f64(wide, n + 3, r, n, wide, n + 3, m, n, bf, row_major=True) == 0          # in place
    assert same_bits(torch, wide[:, :n], want[2]) and bool(torch.isnan(wide[:, n:]).all())
    assert bq.qr_f64(q, 65, r, 65, wide, 65, 100, 65, bf, row_major=True) == bq.error_unsupported_mode


def test_qr_f64_tensor(bq):
    torch = _torch()
    m, n = 4097, 64
    a_host = matrix(m, n, None)
    for reorth in (False, True):
        want = reference(m, n, None, int(reorth))
        a = torch.from_numpy(np.array(a_host)).cuda()                  # contiguous: rows contiguous
        twin = a.t().contiguous().t()                                  # columns contiguous
        big = torch.full((m, 2 * n), NAN, dtype=torch.float64, device="cuda")
        big[:, ::2] = a
        a0 = a.clone()
        q, r = bq.qr_f64_tensor(a, reorth=reorth)
        assert bq.last_sweeps_f64() == want[1]
        assert q.shape == (m, n) and q.is_contiguous() and r.shape == (n, n) and q.data_ptr() != a.data_ptr()
        assert same_bits(torch, q, want[2]) and same_bits(torch, r, want[3]) and torch.equal(a, a0)
        q2, r2 = bq.qr_f64_tensor(twin, reorth=reorth)
        assert q2.shape == (m, n) and q2.stride() == (1, m) and torch.equal(twin, a0)
        assert same_bits(torch, q2, q) and same_bits(torch, r2, r)
        q3, r3 = bq.qr_f64_tensor(big[:, ::2], reorth=reorth)          # neither: copied once, column-major
        assert q3.shape == (m, n) and same_bits(torch, q3, q) and same_bits(torch, r3, r)
        assert same_bits(torch, big[:, ::2], a0) and bool(torch.isnan(big[:, 1::2]).all())
        # overwrite_a: q is a's storage, for either usable layout; a view that has to be copied is left alone
        q4, r4 = bq.qr_f64_tensor(a, reorth=reorth, overwrite_a=True)
        assert q4.data_ptr() == a.data_ptr() and q4.stride() == a.stride() and same_bits(torch, a, q) and same_bits(torch, r4, r)
        q5, _ = bq.qr_f64_tensor(twin, reorth=reorth, overwrite_a=True)
        assert q5.data_ptr() == twin.data_ptr() and q5.stride() == (1, m) and same_bits(torch, twin, q)
        q6, _ = bq.qr_f64_tensor(big[:, ::2], reorth=reorth, overwrite_a=True)
        assert q6.data_ptr() != big.data_ptr() and same_bits(torch, big[:, ::2], a0) and same_bits(torch, q6, q)
    # a padded row-major view, in place: the padding keeps its NaN
    wide = torch.full((m, n + 3), NAN, dtype=torch.float64, device="cuda")
    wide[:, :n] = a0
    q7, _ = bq.qr_f64_tensor(wide[:, :n], reorth=True, overwrite_a=True)
    assert q7.data_ptr() == wide.data_ptr() and same_bits(torch, wide[:, :n], q) and bool(torch.isnan(wide[:, n:]).all())
    # one column: contiguous, and a strided column of a row-major matrix
    col = a0[:, 5:6].contiguous()
    qc, rc = bq.qr_f64_tensor(col)
    qs, rs = bq.qr_f64_tensor(a0[:, 5:6])
    assert qc.shape == qs.shape == (m, 1) and rc.shape == (1, 1) and same_bits(torch, qc, qs) and same_bits(torch, rc, rs)
    assert rc.item() > 0 and abs((qc.t() @ qc).item() - 1.0) <= 1e-11                        # the header's bands at n = 1
    assert (torch.linalg.norm(qc * rc - col) / torch.linalg.norm(col)).item() <= 1e-13
    # sizes the entry does not take
    with pytest.raises(bq.QrError) as e:
        bq.qr_f64_tensor(torch.zeros(100, 65, dtype=torch.float64, device="cuda"))
    assert e.value.state == bq.error_unsupported_mode and "n <= 64" in str(e.value)
    with pytest.raises(bq.QrError) as e:
        bq.qr_f64_tensor(torch.zeros(4, 8, dtype=torch.float64, device="cuda"))
    assert e.value.state == bq.error_invalid_matrix_size

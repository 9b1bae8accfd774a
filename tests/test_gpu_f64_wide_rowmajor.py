"""The wide fp64 entry on operands in either layout (tsqr_mi_qr_f64_wide_lay, 64 < n <= 1024) on the GPU, against the column-major call
(tsqr_mi_qr_f64_wide) on the same matrix BIT FOR BIT: Q read as a matrix, R, the state and last_sweeps_f64(), for all four layout pairs,
in place for row-major, with NaN padding that must survive; the shifted ladder; non-finite input; the one-panel forwarding; the tensor
call qr_f64_wide_tensor and the row_major keyword of qr_f64_wide.  The bands are those of include/tsqr_mi.h for this entry."""
import ctypes

import numpy as np
import pytest

from tests.test_gpu_f64_wide import _cond_matrix, _gauss

pytestmark = pytest.mark.gpu
COL, ROW = 0, 1
PAIRS = ((COL, COL), (ROW, COL), (COL, ROW), (ROW, ROW))
NAN = float("nan")
SHAPES = [(65, 65), (200, 65), (1000, 100), (777, 192), (4096, 256), (1100, 1024)]


def _torch():
    import torch
    return torch


def _store(mat, layout, pad):
    """an all-NaN device tensor with room for a matrix of mat's shape in the given layout, ld = the layout's minimum + pad;
    returns (tensor, ld)"""
    torch = _torch()
    m, n = mat.shape
    lines, length = (m, n) if layout == ROW else (n, m)
    t = torch.full((lines, length + pad), NAN, dtype=torch.float64, device="cuda")
    return t, length + pad


def _put(t, mat, layout):
    m, n = mat.shape
    if layout == ROW:
        t[:, :n] = mat
    else:
        t[:, :m] = mat.T
    return t


def _matrix(t, m, n, layout):
    """(the m x n matrix stored in t, whether all of t's padding is still NaN)"""
    torch = _torch()
    if layout == ROW:
        return t[:, :n], bool(torch.isnan(t[:, n:]).all())
    return t[:, :m].T, bool(torch.isnan(t[:, m:]).all())


class Call:
    """one work space per shape; wide_lay / wide run the two C entries on freshly stored operands and return
    (state, sweeps, Q as an (m, n) tensor, R as an (n, n) tensor, padding intact)"""

    def __init__(self, bq, m, n):
        torch = _torch()
        self.bq, self.L, self.m, self.n = bq, bq.lib(), m, n
        self.wq = torch.empty(self.L.tsqr_mi_working_q_size_f64_wide(m, n), dtype=torch.float64, device="cuda")
        self.wr = torch.empty(self.L.tsqr_mi_working_r_size_f64_wide(m, n), dtype=torch.float64, device="cuda")
        self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def _finish(self, st, q, q_lay, r, a=None, a_lay=None, a_dev=None):
        torch = _torch()
        torch.cuda.synchronize()
        m, n = self.m, self.n
        sweeps = self.bq.last_sweeps_f64()
        Q, ok_q = _matrix(q, m, n, q_lay)
        ok = ok_q and bool(torch.isnan(r[:, n:]).all())
        if a is not None:                                  # out of place: A and its padding are untouched
            A, ok_a = _matrix(a, m, n, a_lay)
            ok = ok and ok_a and torch.equal(torch.nan_to_num(A, nan=7.0), torch.nan_to_num(a_dev, nan=7.0))
        return st, sweeps, Q.clone(), r[:, :n].T.clone(), ok

    def wide_lay(self, a_dev, a_lay, q_lay, reorth, pad=0, in_place=False, entry="tsqr_mi_qr_f64_wide_lay"):
        torch = _torch()
        m, n = self.m, self.n
        a, lda = _store(a_dev, a_lay, pad)
        _put(a, a_dev, a_lay)
        if in_place:
            assert a_lay == q_lay
            q, ldq = a, lda
        else:
            q, ldq = _store(a_dev, q_lay, pad + (2 if pad else 0))
        r = torch.full((n, n + pad), NAN, dtype=torch.float64, device="cuda")
        st = getattr(self.L, entry)(a_lay, q_lay, reorth, q.data_ptr(), ldq, r.data_ptr(), n + pad, a.data_ptr(), lda, m, n,
                                    self.wq.data_ptr(), self.wr.data_ptr(), self.stream)
        return self._finish(st, q, q_lay, r, None if in_place else a, a_lay, a_dev)

    def wide(self, a_dev, reorth):
        torch = _torch()
        m, n = self.m, self.n
        a, lda = _store(a_dev, COL, 0)
        _put(a, a_dev, COL)
        q, ldq = _store(a_dev, COL, 0)
        r = torch.full((n, n), NAN, dtype=torch.float64, device="cuda")
        st = self.L.tsqr_mi_qr_f64_wide(reorth, q.data_ptr(), ldq, r.data_ptr(), n, a.data_ptr(), lda, m, n,
                                        self.wq.data_ptr(), self.wr.data_ptr(), self.stream)
        return self._finish(st, q, COL, r, a, COL, a_dev)


def _same(got, want, what):
    torch = _torch()
    assert got[0] == want[0] and got[1] == want[1], (what, "state / sweeps", got[:2], want[:2])
    assert got[4], (what, "padding or A was written")
    if want[0] == 0:
        assert torch.equal(got[2].view(torch.int64), want[2].view(torch.int64)), (what, "Q differs")
        assert torch.equal(got[3].view(torch.int64), want[3].view(torch.int64)), (what, "R differs")


def _bands(a_dev, Q, R, reorth):
    torch = _torch()
    m, n = a_dev.shape
    I = torch.eye(n, dtype=torch.float64, device="cuda")
    orth = torch.linalg.norm(Q.T @ Q - I).item()
    res = (torch.linalg.norm(a_dev - Q @ R) / torch.linalg.norm(a_dev)).item()
    print("%d x %d reorth %d: ||QtQ-I||_F %.2e  residual %.2e" % (m, n, reorth, orth, res))
    assert orth <= (1e-12 if reorth else 1e-11) * max(1.0, n / 64.0), ("orthogonality", orth)
    assert res <= 1e-13, ("residual", res)
    return orth, res


@pytest.mark.parametrize("m,n", SHAPES)
def test_all_layout_pairs_have_the_bits_of_the_column_major_call(bq, m, n):
    a_dev = _gauss(m, n, 7 * m + n)
    c = Call(bq, m, n)
    for reorth in (0, 1):
        want = c.wide(a_dev, reorth)
        assert want[0] == 0 and want[4], (want[0], bq.last_error())
        for a_lay, q_lay in PAIRS:
            _same(c.wide_lay(a_dev, a_lay, q_lay, reorth), want, (m, n, reorth, a_lay, q_lay))
        _same(c.wide_lay(a_dev, ROW, ROW, reorth, in_place=True), want, (m, n, reorth, "ROW/ROW in place"))
    # padded lda / ldq / ldr with NaN padding that must survive, out of place and in place
    _same(c.wide_lay(a_dev, ROW, ROW, 1, pad=3), want, (m, n, "padded"))
    _same(c.wide_lay(a_dev, ROW, ROW, 1, pad=3, in_place=True), want, (m, n, "padded, in place"))
    _same(c.wide_lay(a_dev, COL, COL, 1, pad=5, in_place=True), want, (m, n, "padded, column-major in place"))
    _bands(a_dev, want[2], want[3], 1)


def test_shifted_ladder_row_major(bq):
    m, n = 4096, 128
    a_dev = _cond_matrix(m, n, 1e12, seed=12 + n)
    c = Call(bq, m, n)
    for reorth in (0, 1):
        want = c.wide(a_dev, reorth)
        assert want[0] == 0, (want[0], bq.last_error())
        assert want[1] >= 100, ("cond 1e12 did not take the shifted ladder", want[1])
        for a_lay, q_lay in PAIRS:
            got = c.wide_lay(a_dev, a_lay, q_lay, reorth)
            _same(got, want, (reorth, a_lay, q_lay))
        got = c.wide_lay(a_dev, ROW, ROW, reorth, in_place=True)
        _same(got, want, (reorth, "in place"))
        assert got[1] >= 100
        _bands(a_dev, got[2], got[3], reorth)              # (implied by the equal bits; checked once on the row-major output)


def test_nan_in_a_is_state_3_in_every_layout_pair(bq):
    m, n = 777, 192
    a_dev = _gauss(m, n, 5)
    c = Call(bq, m, n)
    for row, col in ((500, 191), (776, 64), (0, 0)):
        bad = a_dev.clone()
        bad[row, col] = NAN
        want = c.wide(bad, 0)
        assert want[0] == bq.error_not_finite == 3
        for a_lay, q_lay in PAIRS:
            got = c.wide_lay(bad, a_lay, q_lay, 0)
            assert got[0] == 3 and got[1] == want[1], (row, col, a_lay, q_lay, got[:2], want[:2])
    _same(c.wide_lay(a_dev, ROW, ROW, 0), c.wide(a_dev, 0), "the same work space, good data")


def test_one_panel_is_qr_f64_lay(bq):
    m, n = 500, 51
    a_dev = _cond_matrix(m, n, 1e5, seed=n)
    c = Call(bq, m, n)
    for reorth in (0, 1):
        want = c.wide_lay(a_dev, ROW, ROW, reorth, entry="tsqr_mi_qr_f64_lay")
        assert want[0] == 0 and want[4]
        _same(c.wide_lay(a_dev, ROW, ROW, reorth), want, ("n <= 64", reorth))
        _same(c.wide_lay(a_dev, ROW, ROW, reorth, pad=3, in_place=True), want, ("n <= 64, in place", reorth))


# ---- qr_f64_wide_tensor ---------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(_torch().int64)


@pytest.mark.parametrize("m,n", [(777, 192), (2000, 100)])
def test_tensor_call_same_bits_for_every_storage(bq, m, n):
    torch = _torch()
    a_row = _gauss(m, n, m + n)                            # contiguous (m, n)
    a_col = a_row.t().contiguous().t()                     # its column-major twin
    base = torch.full((m, 2 * n), NAN, dtype=torch.float64, device="cuda")
    base[:, ::2] = a_row
    a_str = base[:, ::2]                                   # neither rows nor columns contiguous: copied once
    assert a_row.stride() == (n, 1) and a_col.stride() == (1, m) and a_str.stride() == (2 * n, 2)
    c = Call(bq, m, n)
    for reorth in (False, True):
        want = c.wide(a_row, int(reorth))
        assert want[0] == 0
        for a, strides in ((a_row, (n, 1)), (a_col, (1, m)), (a_str, (1, m))):
            keep = a.clone()
            q, r = bq.qr_f64_wide_tensor(a, reorth=reorth)
            assert bq.last_sweeps_f64() == want[1]
            assert q.shape == (m, n) and q.stride() == strides and r.shape == (n, n)
            assert torch.equal(_bits(q), _bits(want[2])) and torch.equal(_bits(r), _bits(want[3])), (reorth, strides)
            assert torch.equal(a, keep), "a was written"
        # overwrite_a: q IS a where a is used where it lies; a strided a is copied and left alone
        for a in (a_row.clone(), a_col.clone()):
            q, r = bq.qr_f64_wide_tensor(a, reorth=reorth, overwrite_a=True)
            assert q is a
            assert torch.equal(_bits(q), _bits(want[2])) and torch.equal(_bits(r), _bits(want[3]))
        q, r = bq.qr_f64_wide_tensor(a_str, reorth=reorth, overwrite_a=True)
        assert q is not a_str and torch.equal(a_str, a_row) and bool(torch.isnan(base[:, 1::2]).all())
        assert torch.equal(_bits(q), _bits(want[2])) and torch.equal(_bits(r), _bits(want[3]))


def test_tensor_call_limits_and_one_panel(bq):
    torch = _torch()
    with pytest.raises(bq.QrError) as e:
        bq.qr_f64_wide_tensor(torch.zeros(1100, 1025, dtype=torch.float64, device="cuda"))
    assert e.value.state == bq.error_unsupported_mode and "n <= 1024" in str(e.value)
    with pytest.raises(bq.QrError) as e:
        bq.qr_f64_wide_tensor(torch.zeros(100, 101, dtype=torch.float64, device="cuda"))
    assert e.value.state == bq.error_invalid_matrix_size
    bad = _gauss(300, 100, 1)
    bad[17, 99] = NAN
    with pytest.raises(bq.QrError) as e:
        bq.qr_f64_wide_tensor(bad)
    assert e.value.state == bq.error_not_finite
    for m, n in ((500, 51), (1000, 64)):           # n <= 64: the bits of qr_f64_tensor
        a = _gauss(m, n, n)
        for reorth in (False, True):
            q1, r1 = bq.qr_f64_tensor(a, reorth=reorth)
            s1 = bq.last_sweeps_f64()
            q2, r2 = bq.qr_f64_wide_tensor(a, reorth=reorth)
            assert bq.last_sweeps_f64() == s1 and q2.stride() == q1.stride()
            assert torch.equal(_bits(q1), _bits(q2)) and torch.equal(_bits(r1), _bits(r2))


def test_tensor_call_agrees_with_torch_linalg_qr(bq):
    """Against LAPACK's Householder QR in fp64 on the CPU, columns of Q (rows of R) signed so that R's diagonal is positive.  Both
    factorisations satisfy A = Q R + E with ||E||_F <= res ||A||_F (res: the header's 1e-13 here, a few u for LAPACK) and an
    orthogonality defect orth (the header's band here, a few u sqrt(n) for LAPACK); first-order perturbation theory of the QR
    factorisation (Stewart 1977; Sun 1991) bounds the change of Q by about sqrt(2) cond_2(A) ||E||_F / ||A||_2 plus the defect, and the
    relative change of R likewise.  With ||A||_F <= sqrt(n) ||A||_2:  tol = cond_2(A) (2 sqrt(n) 1e-13 + orth band)."""
    torch = _torch()
    m, n = 2000, 100
    a = _gauss(m, n, 99)
    a_host = a.cpu()
    q_ref, r_ref = torch.linalg.qr(a_host)
    sgn = torch.sign(torch.diagonal(r_ref))
    q_ref, r_ref = q_ref * sgn, sgn[:, None] * r_ref
    cond = torch.linalg.cond(a_host).item()
    for reorth in (False, True):
        q, r = bq.qr_f64_wide_tensor(a, reorth=reorth)
        _bands(a, q, r, int(reorth))
        band = (1e-12 if reorth else 1e-11) * max(1.0, n / 64.0)
        tol = cond * (2.0 * np.sqrt(n) * 1e-13 + band)
        dq = torch.linalg.norm(q.cpu() - q_ref).item()
        dr = (torch.linalg.norm(r.cpu() - r_ref) / torch.linalg.norm(r_ref)).item()
        print("reorth %d: cond %.2f  ||Q - Q_lapack||_F %.2e  ||R - R_lapack||_F / ||R||_F %.2e  tol %.2e" % (reorth, cond, dq, dr, tol))
        assert dq <= tol and dr <= tol
        assert torch.all(torch.tril(r, -1) == 0) and torch.all(torch.diagonal(r) > 0)


# ---- qr_f64_wide(row_major=True) ------------------------------------------------------------------------------------------------------
def test_row_major_keyword_of_qr_f64_wide(bq):
    torch = _torch()
    m, n = 1000, 100
    a_dev = _gauss(m, n, 3)
    c = Call(bq, m, n)
    want = c.wide(a_dev, 1)
    bf = bq.buffer_f64_wide(True)
    bf.allocate(m, n)
    ld = n + 3
    a = torch.full((m, ld), NAN, dtype=torch.float64, device="cuda")
    a[:, :n] = a_dev
    q = torch.full((m, ld), NAN, dtype=torch.float64, device="cuda")
    r = torch.full((n, n), NAN, dtype=torch.float64, device="cuda")
    # operand errors come before any launch: q and r still hold NaN afterwards
    with pytest.raises(ValueError):
        bq.qr_f64_wide(q, n - 1, r, n, a, ld, m, n, bf, row_major=True)                    # ldq < n
    with pytest.raises(ValueError):
        bq.qr_f64_wide(q[:-1], ld, r, n, a, ld, m, n, bf, row_major=True)                  # q one row short
    with pytest.raises(ValueError):
        bq.qr_f64_wide(a, ld - 1, r, n, a, ld, m, n, bf, row_major=True)                   # in place with ldq != lda
    with pytest.raises(ValueError):
        bq.qr_f64_wide(q, ld, r, n, a, ld, m, n, bf)                                       # the same operands column-major: ld < m
    with pytest.raises(TypeError):
        bq.qr_f64_wide(q.float(), ld, r, n, a, ld, m, n, bf, row_major=True)
    torch.cuda.synchronize()
    assert bool(torch.isnan(q).all()) and bool(torch.isnan(r).all())
    assert bq.qr_f64_wide(q, 1025, r, 1025, a, 1025, 2000, 1025, bf, row_major=True) == bq.error_unsupported_mode
    st = bq.qr_f64_wide(q, ld, r, n, a, ld, m, n, bf, row_major=True)
    torch.cuda.synchronize()
    assert st == 0 and bq.last_sweeps_f64() == want[1]
    assert torch.equal(_bits(q[:, :n]), _bits(want[2])) and torch.equal(_bits(r.T), _bits(want[3])) and bool(torch.isnan(q[:, n:]).all())
    st = bq.qr_f64_wide(a, ld, r, n, a, ld, m, n, bf, row_major=True)                      # in place
    torch.cuda.synchronize()
    assert st == 0 and torch.equal(_bits(a[:, :n]), _bits(want[2])) and bool(torch.isnan(a[:, n:]).all())

"""The R-only fp64 entry (tsqr_mi_r_f64) on the GPU, through the Python wrapper and the C ABI: R's shape, guard bands, A untouched,
determinism, the quality of R measured on the CPU in longdouble against Householder QR's R on the same matrix, the ladder's agreement
with tsqr_mi_qr_f64, non-finite input, a non-default stream and a call with an fp32 ticket in flight.
Measures and matrices: tests/pass_refs_f64_r.py.  Every case prints its figures before it asserts."""
import functools

import numpy as np
import pytest

from tests import pass_refs_f64_r as p64r

pytestmark = pytest.mark.gpu

SENT = -777.0
FLOOR = {0: 1e-11, 1: 1e-12}              # the published bands of the full call (include/tsqr_mi.h), reorth = 0 / 1
FACTOR = 8.0                              # over Householder's R on the same A
RESIDUAL = 1e-13


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@functools.lru_cache(maxsize=None)
def matrix(m, n, cond):
    """(A, A^T A in longdouble, ||Q~^T Q~ - I||_F of numpy's Householder R); cond None: Gaussian"""
    a = np.random.default_rng(m + n).standard_normal((m, n)) if cond is None else p64r.cond_matrix(m, n, cond, int(np.log10(cond)) + m)
    r = np.linalg.qr(a, mode="r").reshape(n, n)
    r = np.sign(np.diag(r))[:, None] * r
    return a, p64r.gram_ld(a), p64r.orth_of_r(a, r)


def run_r(bq, a_host, reorth, pad=(3, 2), stream=None):
    """r_f64 on a_host with lda = m + pad[0] (NaN in the padding rows) and ldr = n + pad[1] (sentinels everywhere): state, R (host),
    sweeps; checks R's shape, the guard bands and that A kept its bits"""
    torch = _torch()
    m, n = a_host.shape
    lda, ldr = m + pad[0], n + pad[1]
    a = torch.full((n, lda), float("nan"), dtype=torch.float64, device="cuda")
    a[:, :m] = torch.from_numpy(np.ascontiguousarray(a_host.T)).cuda()
    before = a.clone()
    r = torch.full((n, ldr), SENT, dtype=torch.float64, device="cuda")
    bf = bq.buffer_f64_r(bool(reorth))
    bf.allocate(m, n)
    st = bq.r_f64(r, ldr, a, lda, m, n, bf, stream=stream)
    sweeps = bq.last_sweeps_f64()
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int64), before.view(torch.int64)), "A was written"
    assert (r[:, n:] == SENT).all(), "R's padding rows were written"
    R = r[:, :n].T.cpu().numpy().copy()
    if st == 0:
        assert np.all(np.tril(R, -1) == 0.0), "R has non-zeros below the diagonal"
        assert np.all(np.diag(R) > 0.0), "R's diagonal is not positive"
    return st, R, sweeps


def run_qr(bq, a_host, reorth, pad=(3, 5, 2)):
    """tsqr_mi_qr_f64 on the same operand layout: state, R, sweeps"""
    torch = _torch()
    m, n = a_host.shape
    lda, ldq, ldr = m + pad[0], m + pad[1], n + pad[2]
    a = torch.full((n, lda), float("nan"), dtype=torch.float64, device="cuda")
    a[:, :m] = torch.from_numpy(np.ascontiguousarray(a_host.T)).cuda()
    q = torch.empty((n, ldq), dtype=torch.float64, device="cuda")
    r = torch.full((n, ldr), SENT, dtype=torch.float64, device="cuda")
    bf = bq.buffer_f64(bool(reorth))
    bf.allocate(m, n)
    st = bq.qr_f64(q, ldq, r, ldr, a, lda, m, n, bf)
    sweeps = bq.last_sweeps_f64()
    torch.cuda.synchronize()
    return st, r[:, :n].T.cpu().numpy().copy(), sweeps


def check_case(bq, m, n, cond, reorth):
    a, ata, orth_ref = matrix(m, n, cond)
    st, R, sweeps = run_r(bq, a, reorth)
    assert st == 0, (st, bq.last_error())
    st2, R2, sweeps2 = run_r(bq, a, reorth)
    assert st2 == 0 and sweeps2 == sweeps and np.array_equal(R, R2), "a second call gives other bits"
    orth, res = p64r.orth_of_r(a, R), p64r.gram_residual_of_r(ata, R)
    bound = max(FACTOR * orth_ref, FLOOR[reorth])
    ratio = orth / orth_ref if orth_ref > 0 else float(orth > 0)       # (1 x 1: both are exact zeros)
    stq, Rq, sweepsq = run_qr(bq, a, reorth)
    print("r_f64 %d x %d cond %s reorth %d: sweeps %d (qr_f64: %d)  ||Q~tQ~ - I||_F %.3e, Householder's R %.3e, ratio %.3g, "
          "over bound %.3g;  ||RtR - AtA||_F / ||AtA||_F %.3e"
          % (m, n, "gauss" if cond is None else "%.0e" % cond, reorth, sweeps, sweepsq, orth, orth_ref, ratio, orth / bound, res))
    assert orth <= bound, ("orthogonality of A inverse(R)", orth, orth_ref)
    assert res <= RESIDUAL, ("Gram residual", res)
    # the ladder against the full call on the same input
    assert stq == 0
    assert (sweeps >= 100) == (sweepsq >= 100), (sweeps, sweepsq)
    assert sweeps % 100 <= 6
    if cond is None or cond <= 1e4:
        assert sweeps == sweepsq, (sweeps, sweepsq)
    if cond == 1.0 and not reorth:
        assert sweeps == 1
    if sweeps == 1:
        assert np.array_equal(R, Rq), "one sweep: the same Gram kernel, plan and Cholesky launch as tsqr_mi_qr_f64"
    return ratio


@pytest.mark.parametrize("m,n", [(1, 1), (65, 64), (1000, 7), (9211, 51), (4096, 64)])
@pytest.mark.parametrize("reorth", [0, 1])
def test_r_f64_shapes(bq, m, n, reorth):
    check_case(bq, m, n, None, reorth)
    assert bq.last_sweeps_f64() % 100 >= 1


@pytest.mark.parametrize("m,n", [(4096, 64), (9211, 51)])
@pytest.mark.parametrize("cond", [1.0, 1e4, 1e8, 1e12])
@pytest.mark.parametrize("reorth", [0, 1])
def test_r_f64_conditioning(bq, m, n, cond, reorth):
    check_case(bq, m, n, cond, reorth)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_r_f64_non_finite_input(bq, bad):
    a = np.array(matrix(1000, 7, None)[0])
    a[517, 3] = bad
    for reorth in (0, 1):
        st, _, _ = run_r(bq, a, reorth)
        assert st == bq.error_not_finite, st


def test_r_f64_on_a_side_stream(bq):
    torch = _torch()
    a, _, _ = matrix(9211, 51, None)
    st0, R0, sw0 = run_r(bq, a, 1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    st1, R1, sw1 = run_r(bq, a, 1, stream=side)
    assert st0 == 0 and st1 == 0 and sw0 == sw1 == 2 and np.array_equal(R0, R1)


def test_r_f64_with_an_fp32_ticket_in_flight(bq, oracle):
    """latch_all: the fp32 call submitted before reads its verdict first; both results are those of the calls made alone"""
    torch = _torch()
    from tests.test_gpu_async import Problem, blocking, same
    mode = bq.compute_mode.fp32_tc_cor
    a32 = oracle.uniform_matrix(9211, 51, seed=1)
    want = blocking(bq, torch, a32, mode)
    a, _, _ = matrix(4096, 64, 1e4)
    st0, R0, sw0 = run_r(bq, a, 0)
    p = Problem(bq, torch, a32, mode)
    t = bq.submit(*p.args())
    assert t.pending == 1
    st1, R1, sw1 = run_r(bq, a, 0)
    assert bq.finish(t) == 0
    assert st0 == 0 and st1 == 0 and sw0 == sw1 and np.array_equal(R0, R1)
    assert same(p.result(), want)


def test_r_f64_c_abi_direct(bq):
    """the C entry itself, lda == m and ldr == n, work space of exactly the advertised sizes with sentinels behind it"""
    import ctypes
    torch = _torch()
    m, n = 1000, 7
    a_host, ata, orth_ref = matrix(m, n, None)
    L = bq.lib()
    a = torch.from_numpy(np.ascontiguousarray(a_host.T)).cuda()
    r = torch.full((n, n), SENT, dtype=torch.float64, device="cuda")
    nq, nr = L.tsqr_mi_working_q_size_f64_r(m, n), L.tsqr_mi_working_r_size_f64_r(m, n)
    wq = torch.full((nq + 8,), SENT, dtype=torch.float64, device="cuda")
    wr = torch.full((nr + 8,), SENT, dtype=torch.float64, device="cuda")
    vp = ctypes.c_void_p
    st = L.tsqr_mi_r_f64(1, vp(r.data_ptr()), n, vp(a.data_ptr()), m, m, n, vp(wq.data_ptr()), vp(wr.data_ptr()),
                         vp(torch.cuda.current_stream().cuda_stream))
    assert st == 0 and L.tsqr_mi_last_sweeps_f64() == 2
    assert (wq[nq:] == SENT).all() and (wr[nr:] == SENT).all(), "written behind the work space"
    R = r.T.cpu().numpy()
    assert np.array_equal(R, run_r(bq, np.array(a_host), 1)[1])
    assert p64r.orth_of_r(a_host, R) <= max(FACTOR * orth_ref, FLOOR[1])

"""The fp64 least-squares entry (tsqr_mi_lstsq_f64) on the GPU through blockqr.lstsq_f64: the error of X against a longdouble
Householder solve on the CPU, next to the same measure of numpy.linalg.lstsq (LAPACK, fp64) on the same data -- the yardstick is never
the code under test; R against blockqr.r_f64, bit for bit; A and B untouched; determinism; the effect of the refinement count; the
ladder's state 3.  Inputs, references and measures: tests/pass_refs_f64_lsq.py (tests/test_pass_refs_f64_lsq.py runs a numpy model of
the call through the same check on the CPU).  Every case prints its figures before it asserts.

The assertion, for refine = 1:  err <= max(FACTOR * err_lapack, 4 n u).  FACTOR was fixed as the issue of this entry prescribes: the
numpy model's largest ratio err / err_lapack on these inputs is 0.62, the largest measured on an MI355X is 0.69
(profiles/fp64_lstsq_accuracy.md has both tables); FACTOR is that maximum times a margin of 2 to 4 (1.4 .. 2.8), rounded up to a power
of two."""
import functools

import numpy as np
import pytest

from tests import pass_refs_f64_lsq as pl

pytestmark = pytest.mark.gpu

FACTOR = 2.0


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@functools.lru_cache(maxsize=None)
def reference(case):
    """(A, B, X_ref in longdouble, error of numpy's lstsq, its normal-equations residual): computed once, shared, never written"""
    _, m, n, nrhs, cond, kind = case
    a, b = pl.accuracy_input(m, n, nrhs, cond, kind)
    ref = pl.lstsq_ld(a, b)
    xl = np.linalg.lstsq(a, b, rcond=None)[0]
    for arr in (a, b, ref):
        arr.setflags(write=False)
    return a, b, ref, pl.rel_err(xl, ref), pl.normal_residual(a, b, xl)


def solve(bq, a_host, b_host, reorth, refine, colmajor=True):
    """lstsq_f64 on device copies (column-major with padded leading dimensions, or plain row-major tensors): X, R on the host and the
    sweep count; checks that A and B kept their bytes"""
    torch = _torch()
    m, n = a_host.shape
    nrhs = b_host.shape[1]
    if colmajor:
        a = torch.full((n, m + 3), float("nan"), dtype=torch.float64, device="cuda")
        a[:, :m] = torch.from_numpy(np.array(a_host.T, order="C")).cuda()
        b = torch.full((nrhs, m + 5), float("nan"), dtype=torch.float64, device="cuda")
        b[:, :m] = torch.from_numpy(np.array(b_host.T, order="C")).cuda()
        av, bv = a[:, :m].t(), b[:, :m].t()                # m x n and m x nrhs views with contiguous columns: used where they lie
    else:
        a, b = torch.from_numpy(np.array(a_host)).cuda(), torch.from_numpy(np.array(b_host)).cuda()
        av, bv = a, b
    before = a.clone(), b.clone()
    x, r = bq.lstsq_f64(av, bv, reorth=bool(reorth), refine=refine)
    sweeps = bq.last_sweeps_f64()
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int64), before[0].view(torch.int64)), "A was written"
    assert torch.equal(b.view(torch.int64), before[1].view(torch.int64)), "B was written"
    assert x.shape == (n, nrhs) and r.shape == (n, n)
    return x.cpu().numpy().copy(), r.cpu().numpy().copy(), sweeps


def r_only(bq, a_host, reorth):
    torch = _torch()
    m, n = a_host.shape
    a = torch.from_numpy(np.array(a_host.T, order="C")).cuda()
    r = torch.empty((n, n), dtype=torch.float64, device="cuda")
    bf = bq.buffer_f64_r(bool(reorth))
    bf.allocate(m, n)
    assert bq.r_f64(r, n, a, m, m, n, bf) == 0
    return r.T.cpu().numpy().copy(), bq.last_sweeps_f64()


@pytest.mark.parametrize("reorth", [0, 1])
@pytest.mark.parametrize("case", pl.accuracy_cases(), ids=lambda c: c[0])
def test_lstsq_f64_accuracy(bq, case, reorth):
    a, b, ref, err_lapack, nres_lapack = reference(case)
    n = a.shape[1]
    floor = pl.floor_of(n)
    errs, nres = {}, {}
    for refine in (0, 1, 2):
        x, r, sweeps = solve(bq, a, b, reorth, refine)
        errs[refine], nres[refine] = pl.rel_err(x, ref), pl.normal_residual(a, b, x)
        if refine == 1:
            x1, r1, sw1 = x, r, sweeps
    ratio = errs[1] / err_lapack if err_lapack > 0 else float(errs[1] > 0)
    print("lstsq_f64 %-32s reorth %d sweeps %d: err refine 0 %.3e  1 %.3e  2 %.3e  lapack %.3e  ratio(refine 1) %.3g  floor %.3e;  "
          "||At(B - AX)||_F / (||A||_F ||B||_F) refine 1 %.3e  lapack %.3e"
          % (case[0], reorth, sw1, errs[0], errs[1], errs[2], err_lapack, ratio, floor, nres[1], nres_lapack))
    assert errs[1] <= max(FACTOR * err_lapack, floor), ("refine = 1 against LAPACK", errs[1], err_lapack)
    assert errs[2] <= 2.0 * max(errs[1], floor), ("refine = 2 is worse than refine = 1", errs[2], errs[1])
    # R is the R-only entry's, bit for bit, and the ladder took the same sweeps
    rr, swr = r_only(bq, a, reorth)
    assert sw1 == swr and np.array_equal(r1, rr), "R differs from r_f64's"
    assert np.all(np.tril(r1, -1) == 0.0) and np.all(np.diag(r1) > 0.0)
    # a second call gives the same bits; a row-major operand (copied once by the wrapper) too
    x2, r2, _ = solve(bq, a, b, reorth, 1)
    assert np.array_equal(x1, x2) and np.array_equal(r1, r2), "a second call gives other bits"
    x3, r3, _ = solve(bq, a, b, reorth, 1, colmajor=False)
    assert np.array_equal(x1, x3) and np.array_equal(r1, r3), "the operand's layout changed the bits"


def test_lstsq_f64_vector_rhs_and_default_refine(bq):
    torch = _torch()
    case = [c for c in pl.accuracy_cases() if c[0] == "gauss_1000x7_gaussian"][0]
    a, b, ref, err_lapack, _ = reference(case)
    ad, bd = torch.from_numpy(np.array(a)).cuda(), torch.from_numpy(np.array(b)).cuda()
    x, r = bq.lstsq_f64(ad, bd[:, 1])
    assert x.shape == (7,) and r.shape == (7, 7)
    xm, _ = bq.lstsq_f64(ad, bd, refine=1)
    print("vector right-hand side: bits equal to the matrix call's column: %s" % torch.equal(x, xm[:, 1].contiguous()))
    e = ref[:, 1:2]
    err_col_lapack = pl.rel_err(np.linalg.lstsq(a, b[:, 1:2], rcond=None)[0], e)
    assert pl.rel_err(x.cpu().numpy()[:, None], e) <= max(FACTOR * err_col_lapack, pl.floor_of(7))
    import tsqr_gpu_amd
    x0, _ = tsqr_gpu_amd.lstsq_f64(ad, bd)                   # refine defaults to 1
    assert torch.equal(x0, xm)


def test_lstsq_f64_nan_in_a_is_state_3(bq):
    """the ladder's state 3, through the wrapper (LstsqError.state) and through the C entry itself"""
    import ctypes
    torch = _torch()
    case = [c for c in pl.accuracy_cases() if c[0] == "gauss_1000x7_gaussian"][0]
    a, b = np.array(reference(case)[0]), reference(case)[1]
    a[517, 3] = float("nan")
    m, n = a.shape
    nrhs = b.shape[1]
    ad, bd = torch.from_numpy(np.ascontiguousarray(a.T)).cuda(), torch.from_numpy(np.ascontiguousarray(b.T)).cuda()
    with pytest.raises(bq.LstsqError) as e:
        bq.lstsq_f64(ad.t(), bd.t())
    assert e.value.state == bq.error_not_finite
    L = bq.lib()
    x = torch.zeros((nrhs, n), dtype=torch.float64, device="cuda")
    r = torch.zeros((n, n), dtype=torch.float64, device="cuda")
    wq = torch.empty(L.tsqr_mi_working_q_size_f64_lstsq(m, n, nrhs), dtype=torch.float64, device="cuda")
    wr = torch.empty(L.tsqr_mi_working_r_size_f64_lstsq(m, n, nrhs), dtype=torch.float64, device="cuda")
    vp = ctypes.c_void_p
    for reorth in (0, 1):
        st = L.tsqr_mi_lstsq_f64(reorth, 1, vp(x.data_ptr()), n, vp(r.data_ptr()), n, vp(ad.data_ptr()), m, vp(bd.data_ptr()), m,
                                 m, n, nrhs, vp(wq.data_ptr()), vp(wr.data_ptr()), vp(torch.cuda.current_stream().cuda_stream))
        assert st == 3 == bq.error_not_finite
        assert L.tsqr_mi_last_sweeps_f64() >= 1


def test_lstsq_f64_c_abi_direct(bq):
    """the C entry itself with work space of exactly the advertised sizes and sentinels behind it, ldx and ldr padded"""
    import ctypes
    torch = _torch()
    case = [c for c in pl.accuracy_cases() if c[0] == "gauss_9211x51_gaussian"][0]
    a, b, ref, err_lapack, _ = reference(case)
    m, n = a.shape
    nrhs = b.shape[1]
    SENT = -777.0
    L = bq.lib()
    ad, bd = torch.from_numpy(np.ascontiguousarray(a.T)).cuda(), torch.from_numpy(np.ascontiguousarray(b.T)).cuda()
    ldx, ldr = n + 2, n + 3
    x = torch.full((nrhs, ldx), SENT, dtype=torch.float64, device="cuda")
    r = torch.full((n, ldr), SENT, dtype=torch.float64, device="cuda")
    nq, nr = L.tsqr_mi_working_q_size_f64_lstsq(m, n, nrhs), L.tsqr_mi_working_r_size_f64_lstsq(m, n, nrhs)
    wq = torch.full((nq + 8,), SENT, dtype=torch.float64, device="cuda")
    wr = torch.full((nr + 8,), SENT, dtype=torch.float64, device="cuda")
    vp = ctypes.c_void_p
    st = L.tsqr_mi_lstsq_f64(1, 2, vp(x.data_ptr()), ldx, vp(r.data_ptr()), ldr, vp(ad.data_ptr()), m, vp(bd.data_ptr()), m,
                             m, n, nrhs, vp(wq.data_ptr()), vp(wr.data_ptr()), vp(torch.cuda.current_stream().cuda_stream))
    assert st == 0 and L.tsqr_mi_last_sweeps_f64() == 2
    assert (wq[nq:] == SENT).all() and (wr[nr:] == SENT).all(), "written behind the work space"
    assert (x[:, n:] == SENT).all() and (r[:, n:] == SENT).all(), "written into the padding rows of x or r"
    xs, rs, _ = solve(bq, a, b, 1, 2)
    assert np.array_equal(x[:, :n].T.cpu().numpy(), xs) and np.array_equal(r[:, :n].T.cpu().numpy(), rs)
    assert pl.rel_err(xs, ref) <= 2.0 * max(FACTOR * err_lapack, pl.floor_of(n))

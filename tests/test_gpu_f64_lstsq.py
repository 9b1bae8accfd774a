"""The fp64 least-squares entry (tsqr_mi_lstsq_f64) on the GPU through blockqr.lstsq_f64: the error of X against a longdouble
Householder solve on the CPU, next to the same measure of numpy.linalg.lstsq (LAPACK, fp64) on the same data -- the yardstick is never
the code under test; R against blockqr.r_f64, bit for bit; A and B untouched; determinism; the effect of the refinement count; the
ladder's state 3.  Inputs, references and measures: tests/pass_refs_f64_lsq.py (tests/test_pass_refs_f64_lsq.py runs a numpy model of
the call through the same check on the CPU).  Every case prints its figures before it asserts.

The assertion, for refine = 1:  err <= max(FACTOR * err_lapack, 4 n u).  FACTOR was fixed as the issue of this entry prescribes: the
numpy model's largest ratio err / err_lapack on these inputs is 0.62, the largest measured on an MI355X is 0.69
(profiles/fp64_lstsq_accuracy.md has both tables); FACTOR is that maximum times a margin of 2 to 4 (1.4 .. 2.8), rounded up to a power
of two.  With the cases at pass_refs_f64_lsq.RUNG_SHAPES (both conditioned rungs of the ladder with NP != n) the largest measured ratio
is 1.05 (model 0.66); FACTOR stays."""
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


def solve_state(bq, a_host, b_host, reorth, refine, colmajor=True):
    """lstsq_f64 on device copies with padded leading dimensions and NaN guard bands (column-major: lda = m + 3, ldb = m + 5; row-major:
    lda = n + 3, ldb = nrhs + 5; both are read where they lie): (state, X, R, sweeps) with X, R on the host (None unless the state is 0);
    checks that A, B and the guard bands kept their bytes"""
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
        a = torch.full((m, n + 3), float("nan"), dtype=torch.float64, device="cuda")
        a[:, :n] = torch.from_numpy(np.array(a_host, order="C")).cuda()
        b = torch.full((m, nrhs + 5), float("nan"), dtype=torch.float64, device="cuda")
        b[:, :nrhs] = torch.from_numpy(np.array(b_host, order="C")).cuda()
        av, bv = a[:, :n], b[:, :nrhs]                     # views with contiguous rows: used where they lie
    before = a.clone(), b.clone()
    try:
        x, r = bq.lstsq_f64(av, bv, reorth=bool(reorth), refine=refine)
        state = 0
    except bq.LstsqError as e:
        x, r, state = None, None, e.state
    sweeps = bq.last_sweeps_f64()
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int64), before[0].view(torch.int64)), "A was written"
    assert torch.equal(b.view(torch.int64), before[1].view(torch.int64)), "B was written"
    if state != 0:
        return state, None, None, sweeps
    assert x.shape == (n, nrhs) and r.shape == (n, n)
    return 0, x.cpu().numpy().copy(), r.cpu().numpy().copy(), sweeps


def solve(bq, a_host, b_host, reorth, refine, colmajor=True):
    """solve_state for a call that must end with state 0: X, R on the host and the sweep count"""
    state, x, r, sweeps = solve_state(bq, a_host, b_host, reorth, refine, colmajor)
    assert state == 0, (state, bq.last_error())
    return x, r, sweeps


def r_only_state(bq, a_host, reorth):
    torch = _torch()
    m, n = a_host.shape
    a = torch.from_numpy(np.array(a_host.T, order="C")).cuda()
    r = torch.empty((n, n), dtype=torch.float64, device="cuda")
    bf = bq.buffer_f64_r(bool(reorth))
    bf.allocate(m, n)
    st = bq.r_f64(r, n, a, m, m, n, bf)
    return st, r.T.cpu().numpy().copy(), bq.last_sweeps_f64()


def r_only(bq, a_host, reorth):
    st, r, sweeps = r_only_state(bq, a_host, reorth)
    assert st == 0
    return r, sweeps


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


@pytest.mark.parametrize("reorth", [0, 1])
@pytest.mark.parametrize("case", pl.accuracy_cases(), ids=lambda c: c[0])
def test_lstsq_f64_refine_3_and_4(bq, case, reorth):
    """the rule that ties refine = 2 to refine = 1, for the two largest counts: err_3 and err_4 <= 2 max(err_2, floor).
    This is the case that found the stagnation rule of lsq_update_f64_kernel: with every correction applied,
    cond1e+06_300x17_consistent gave err of refine 1 .. 4 = 9.564e-13, 1.300e-12, 2.796e-12, 1.845e-12 on an MI355X (LAPACK
    3.344e-12), err_3 / err_2 = 2.15 -- past convergence a correction is the rounding noise of its own pass, and the numpy model
    without the rule shows the same on fresh matrices of this shape (5 of 120 ratios above 2, the largest 3.6; with the rule none,
    tests/test_pass_refs_f64_lsq.py).  profiles/fp64_lstsq_accuracy.md has the figures with the rule."""
    a, b, ref, err_lapack, _ = reference(case)
    floor = pl.floor_of(a.shape[1])
    errs = {refine: pl.rel_err(solve(bq, a, b, reorth, refine)[0], ref) for refine in (2, 3, 4)}
    print("lstsq_f64 %-32s reorth %d: err refine 2 %.3e  3 %.3e  4 %.3e  lapack %.3e  floor %.3e  err_3 / err_2 %.3g  err_4 / err_2 %.3g"
          % (case[0], reorth, errs[2], errs[3], errs[4], err_lapack, floor, errs[3] / max(errs[2], floor), errs[4] / max(errs[2], floor)))
    assert errs[3] <= 2.0 * max(errs[2], floor), ("refine = 3 is worse than refine = 2", errs[3], errs[2])
    assert errs[4] <= 2.0 * max(errs[2], floor), ("refine = 4 is worse than refine = 2", errs[4], errs[2])


def test_lstsq_f64_rung_cases_reach_both_conditioned_rungs(bq):
    """the cases at pass_refs_f64_lsq.RUNG_SHAPES (NP != n, NT = 2, 3, 4) end on a CholeskyQR2 ladder (2 sweeps: Z = Z_1 Z_2 through
    f64r_zmul) and on a shifted one (103 or more: two further products) -- if the rule drifts so that a rung loses its input, this says so"""
    seen = {}
    for case in pl.rung_cases():
        a, b = reference(case)[:2]
        seen[case[0]] = solve(bq, a, b, 0, 1)[2]
    print("sweeps: " + "  ".join("%s %d" % kv for kv in seen.items()))
    assert 2 in seen.values() and any(s >= 103 for s in seen.values()), seen
    for m, n, _ in pl.RUNG_SHAPES:
        assert n % 16 != 0


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


def _c_abi_direct(bq, name, reorth, refine, sweeps_ok):
    import ctypes
    torch = _torch()
    case = [c for c in pl.accuracy_cases() if c[0] == name][0]
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
    st = L.tsqr_mi_lstsq_f64(reorth, refine, vp(x.data_ptr()), ldx, vp(r.data_ptr()), ldr, vp(ad.data_ptr()), m, vp(bd.data_ptr()), m,
                             m, n, nrhs, vp(wq.data_ptr()), vp(wr.data_ptr()), vp(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == 0 and sweeps_ok(L.tsqr_mi_last_sweeps_f64()), (st, L.tsqr_mi_last_sweeps_f64())
    assert (wq[nq:] == SENT).all() and (wr[nr:] == SENT).all(), "written behind the work space"
    assert (x[:, n:] == SENT).all() and (r[:, n:] == SENT).all(), "written into the padding rows of x or r"
    xs, rs, _ = solve(bq, a, b, reorth, refine)
    assert np.array_equal(x[:, :n].T.cpu().numpy(), xs) and np.array_equal(r[:, :n].T.cpu().numpy(), rs)
    assert pl.rel_err(xs, ref) <= 2.0 * max(FACTOR * err_lapack, pl.floor_of(n))


def test_lstsq_f64_c_abi_direct(bq):
    """the C entry itself with work space of exactly the advertised sizes and sentinels behind it, ldx and ldr padded"""
    _c_abi_direct(bq, "gauss_9211x51_gaussian", 1, 2, lambda s: s == 2)


def test_lstsq_f64_c_abi_direct_refine_4(bq):
    """the same with the largest refinement count, behind a shifted ladder (three products into Z) with a column tail"""
    _c_abi_direct(bq, "cond1e+06_1029x51_consistent", 0, 4, lambda s: s >= 103)

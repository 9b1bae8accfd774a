"""The fp64 entries (tsqr_mi_qr_f64, tsqr_mi_r_f64, tsqr_mi_qr_f64_wide, tsqr_mi_qr_f64_dist_cb on one rank) under power-of-two scaling
and on dependent columns.  Generators, exponents and the longdouble measures: tests/pass_refs_f64_scale.py (checked on the CPU by
tests/test_pass_refs_f64_scale.py, which also proves that the exponents used for the covariance tests keep A^T A normal with margin).

What is asserted follows from the code, not from what the code returns:
  uniform scaling   A -> 2^k A multiplies every intermediate of every rung of the ladder -- the shift s = shift_coef trace(G) included -- by
                    an exact power of two: the same state and sweep count, the same bits of Q, R' = 2^k R exactly;
  graded scaling    A -> A diag(2^k_j) does the same on the unshifted rungs (the verdicts are ratios of like-scaled quantities):
                    the same bits of Q, column j of R multiplied by 2^k_j exactly;
  outside the range a Gram matrix that overflows or underflows ends in state 3 or in a result inside the header's bands, never in a
                    state 0 with a wrong answer;
  dependent columns state 0 or 3, the same on the entries documented as bitwise equal; a state 0 comes with finite Q and R, the shifted
                    path, the header's residual, and orthonormal leading columns.
Operands as in tests/test_gpu_f64.py: padded leading dimensions, NaN guard bands checked after every call, A compared with its bits
before the call.  Every case prints its figures before it asserts."""
import ctypes

import numpy as np
import pytest

from tests import pass_refs_f64 as p64
from tests import pass_refs_f64_r as p64r
from tests import pass_refs_f64_scale as ps

pytestmark = pytest.mark.gpu

PAD = (3, 5, 2)                                           # lda - m, ldq - m, ldr - n
ENTRY_SHAPES = ([("qr", m, n) for m, n in ps.NARROW_SHAPES] + [("r", m, n) for m, n in ps.NARROW_SHAPES]
                + [("wide", m, n) for m, n in ps.WIDE_SHAPES] + [("dist", m, n) for m, n in ps.DIST_SHAPES])
_IDS = ["%s-%dx%d" % e for e in ENTRY_SHAPES]

_ALLREDUCE_ONE_RANK = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p)(
    lambda user, buf, count, stream: 0)                   # the sum over one rank: the buffer as it is (tests/test_gpu_f64_dist.py)


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _bits(t):
    torch = _torch()
    return t.contiguous().view(torch.int64)


def _call(bq, entry, a_host, reorth):
    """one call of `entry` on a_host (m x n, host) with padded leading dimensions and NaN guard bands.  Returns (state, sweeps, Q, R):
    Q the n x m device tensor of Q^T's rows (column-major Q; None for the R-only entry), R the n x n host array."""
    torch = _torch()
    m, n = a_host.shape
    lda, ldq, ldr = m + PAD[0], m + PAD[1], n + PAD[2]
    a = torch.full((n, lda), float("nan"), dtype=torch.float64, device="cuda")
    a[:, :m] = torch.from_numpy(np.array(a_host.T, order="C")).cuda()      # (a copy: the shared inputs are read-only)
    before = a.clone()
    q = torch.full((n, ldq), float("nan"), dtype=torch.float64, device="cuda")
    r = torch.full((n, ldr), float("nan"), dtype=torch.float64, device="cuda")
    if entry == "qr":
        bf = bq.buffer_f64(bool(reorth)); bf.allocate(m, n)
        st = bq.qr_f64(q, ldq, r, ldr, a, lda, m, n, bf)
    elif entry == "wide":
        bf = bq.buffer_f64_wide(bool(reorth)); bf.allocate(m, n)
        st = bq.qr_f64_wide(q, ldq, r, ldr, a, lda, m, n, bf)
    elif entry == "r":
        bf = bq.buffer_f64_r(bool(reorth)); bf.allocate(m, n)
        st = bq.r_f64(r, ldr, a, lda, m, n, bf)
    else:
        assert entry == "dist", entry
        L = bq.lib()
        wq = torch.empty(max(L.tsqr_mi_working_q_size_f64_dist(m, n, 1), 1), dtype=torch.float64, device="cuda")
        wr = torch.empty(max(L.tsqr_mi_working_r_size_f64_dist(m, n, 1), 1), dtype=torch.float64, device="cuda")
        st = L.tsqr_mi_qr_f64_dist_cb(int(reorth), q.data_ptr(), ldq, r.data_ptr(), ldr, a.data_ptr(), lda, m, n, wq.data_ptr(), wr.data_ptr(),
                                      _ALLREDUCE_ONE_RANK, None, 1, torch.cuda.current_stream().cuda_stream)
        assert st >= 0, (st, bq.last_error())
    sweeps = bq.last_sweeps_f64()
    torch.cuda.synchronize()
    assert torch.equal(_bits(a), _bits(before)), "A was written"
    assert torch.isnan(r[:, n:]).all(), "R's padding rows were written"
    if entry == "r":
        assert torch.isnan(q).all(), "the R-only entry wrote Q"
        Q = None
    else:
        assert torch.isnan(q[:, m:]).all(), "Q's padding rows were written"
        Q = q[:, :m].contiguous()
    return st, sweeps, Q, r[:, :n].T.cpu().numpy().copy()


def _same(x, y):
    return np.array_equal(np.ascontiguousarray(x).view(np.int64), np.ascontiguousarray(y).view(np.int64))


def _r_shape(R, lead=None):
    n = R.shape[0]
    assert np.all(np.isfinite(R)), "R is not finite"
    assert np.all(np.tril(R, -1) == 0.0), "R has non-zeros below the diagonal"
    assert np.all(np.diag(R)[:n if lead is None else lead] > 0.0), "R's diagonal is not positive"


def _check_bands(tag, entry, a_host, Q, R, reorth, sweeps):
    """the header's bands in longdouble; for the R-only entry the two measures of its header (tests/test_gpu_f64_r.py's FLOOR)"""
    m, n = a_host.shape
    _r_shape(R)
    if entry == "r":
        # (its header: A inverse(R) within a small factor of Householder's R on the same A -- the rule of tests/test_gpu_f64_r.py, factor 8
        # over the floor of the full call's bands: on an ill-conditioned A no R does better than cond(A) u)
        rh = np.linalg.qr(a_host, mode="r").reshape(n, n)
        orth_ref = p64r.orth_of_r(a_host, np.sign(np.diag(rh))[:, None] * rh)
        orth, res = p64r.orth_of_r(a_host, R), p64r.gram_residual_of_r(p64r.gram_ld(a_host), R)
        print("%s: sweeps %d  ||Q~tQ~-I||_F %.2e (Householder's R: %.2e)  ||RtR-AtA||_F/||AtA||_F %.2e" % (tag, sweeps, orth, orth_ref, res))
        assert orth <= max(8.0 * orth_ref, 1e-12 if reorth else 1e-11) and res <= 1e-13, (tag, orth, orth_ref, res)
        return
    orth, res, cols = ps.ext_metrics(a_host, Q.T.cpu().numpy(), R)
    print("%s: sweeps %d  ||QtQ-I||_F %.2e  residual %.2e  worst column %.2e" % (tag, sweeps, orth, res, cols.max()))
    orth_max, res_max = ps.bands(n, reorth)
    assert orth <= orth_max and res <= res_max, (tag, orth, res)


# ---- 3a: uniform scaling, every rung -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,m,n", ENTRY_SHAPES, ids=_IDS)
@pytest.mark.parametrize("kind", ps.UNIFORM_INPUTS)
@pytest.mark.parametrize("reorth", [0, 1])
def test_uniform_scaling_is_bitwise_covariant(bq, entry, m, n, kind, reorth):
    """A and 2^k A, k in {-400, -1, 1, 401}: the same state and sweeps, the same bits of Q, R_k = 2^k R exactly, on whichever rung the
    input ends (Gaussian: 1 sweep, 2 with reorth; cond 1e6 and 1e12: CholeskyQR2 or the shifted path, printed); the unscaled call
    meets the header's bands in longdouble, and bitwise covariance carries that to the scaled ones."""
    torch = _torch()
    a_host = ps.uniform_input(kind, m, n)
    tag = "%s %d x %d %s reorth %d" % (entry, m, n, kind, reorth)
    st0, sw0, Q0, R0 = _call(bq, entry, a_host, reorth)
    assert st0 == 0, (tag, st0, bq.last_error())
    if kind == "gauss":
        assert sw0 == (2 if reorth else 1), (tag, sw0)
    elif kind == "cond1e12" and n >= 51:
        assert sw0 >= 100, (tag, sw0)
    for k in ps.UNIFORM_K:
        st, sw, Q, R = _call(bq, entry, ps.scale_uniform(a_host, k), reorth)
        assert st == st0 and sw == sw0, (tag, k, st, sw, sw0)
        assert Q0 is None or torch.equal(_bits(Q), _bits(Q0)), (tag, k, "Q changed bits")
        assert _same(R, np.ldexp(R0, k)), (tag, k, "R is not 2^k R")
    _check_bands(tag, entry, a_host, Q0, R0, reorth, sw0)


def test_uniform_inputs_reach_every_rung(bq):
    """the inputs of the test above, unscaled, on tsqr_mi_qr_f64 with reorth = 0: over the shapes the ladder ends after one sweep, after
    two (CholeskyQR2) and on the shifted path -- if the rule drifts so that a rung loses its input, this says so"""
    seen = {}
    for m, n in ps.NARROW_SHAPES:
        for kind in ps.UNIFORM_INPUTS:
            st, sw, _, _ = _call(bq, "qr", ps.uniform_input(kind, m, n), 0)
            assert st == 0
            seen[(m, n, kind)] = sw
    print("sweeps: " + "  ".join("%dx%d %s %d" % (m, n, kind, sw) for (m, n, kind), sw in seen.items()))
    rungs = set(seen.values())
    assert 1 in rungs and 2 in rungs and any(r >= 100 for r in rungs), rungs


@pytest.mark.parametrize("lg", [20, 23])
def test_cond_1e12_at_the_documented_sizes(bq, lg):
    """cond(A) = 1e12 at 2^20 and 2^23 rows x 64, the far end of the header's promise, data built on the device (U diag(sigma) V^T,
    sigma logarithmic from 1 to 1e-12): state 0, the header's bands, and a ladder that ends at least one sweep below its cap of six --
    the pivot floor of the later sweeps (CholArgs64) may cost this input a shifted sweep, never the call.  Sweeps are printed."""
    torch = _torch()
    m, n = 1 << lg, 64
    g = torch.Generator(device="cuda").manual_seed(lg)
    u, _ = torch.linalg.qr(torch.randn(m, n, dtype=torch.float64, device="cuda", generator=g))
    v, _ = torch.linalg.qr(torch.randn(n, n, dtype=torch.float64, device="cuda", generator=g))
    a = ((u * torch.logspace(0.0, -12.0, n, dtype=torch.float64, device="cuda")) @ v.T).T.contiguous()     # column-major m x n
    del u
    q = torch.empty_like(a)
    r = torch.full((n, n + 2), float("nan"), dtype=torch.float64, device="cuda")
    for reorth in (0, 1):
        bf = bq.buffer_f64(bool(reorth)); bf.allocate(m, n)
        st = bq.qr_f64(q, m, r, n + 2, a, m, m, n, bf)
        torch.cuda.synchronize()
        sweeps = bq.last_sweeps_f64()
        assert st == 0, (st, sweeps, bq.last_error())
        rt = r[:, :n]                                                                  # R^T
        orth = torch.linalg.norm(q @ q.T - torch.eye(n, dtype=torch.float64, device="cuda")).item()
        res = (torch.linalg.norm(a - rt @ q) / torch.linalg.norm(a)).item()
        print("2^%d x 64 cond 1e12 reorth %d: sweeps %d  ||QtQ-I||_F %.2e  residual %.2e" % (lg, reorth, sweeps, orth, res))
        assert sweeps >= 100 and sweeps % 100 <= 5, sweeps
        assert torch.isnan(r[:, n:]).all() and torch.all(torch.triu(rt, 1) == 0) and torch.all(torch.diagonal(rt) > 0)
        assert orth <= (1e-12 if reorth else 1e-11) and res <= 1e-13, (orth, res)


# ---- 3b: per-column scaling, unshifted rungs -----------------------------------------------------------------------------------------------
_GRADED_NAMES = ("gauss",) + ps.GRADED_LADDER_ROWS          # (one column: S = 1, there is no ladder matrix; the Gaussian case alone)
_GRADED = [(e, m, n, w) for e, m, n in ENTRY_SHAPES for w in range(len(_GRADED_NAMES) if n > 1 else 1)]


@pytest.mark.parametrize("entry,m,n,which", _GRADED,
                         ids=["%s-%dx%d-%s" % (e, m, n, _GRADED_NAMES[w].replace(" ", "")) for e, m, n, w in _GRADED])
def test_graded_scaling_is_bitwise_covariant_on_the_unshifted_rungs(bq, entry, m, n, which):
    """A and A diag(2^k_j), k_j in [-300, 300] with both extremes: Gaussian input and the ladder matrices below, between and above the
    one-sweep bound on the CholeskyQR2 side (pass_refs_f64.ladder_targets).  The sweep counts are the ladder's own (no shift: the
    acceptance rule sees S of the column-scaled matrix, as CholArgs64 says), Q keeps its bits, column j of R is multiplied by 2^k_j."""
    torch = _torch()
    name, a_host = ps.graded_inputs(m, n)[which]
    assert name == _GRADED_NAMES[which]
    k = ps.graded_k(m, n)
    a_scaled = ps.scale_columns(a_host, k)
    want = {"gauss": (1, 2)}
    want.update({nm: (s0, s1) for nm, _, s0, s1 in p64.ladder_targets(m, n)} if n > 1 else {})
    for reorth in (0, 1):
        tag = "%s %d x %d %s reorth %d" % (entry, m, n, name, reorth)
        st0, sw0, Q0, R0 = _call(bq, entry, a_host, reorth)
        st1, sw1, Q1, R1 = _call(bq, entry, a_scaled, reorth)
        print("%s: state %d / %d  sweeps %d / %d  (k from %d to %d)" % (tag, st0, st1, sw0, sw1, k.min(), k.max()))
        assert st0 == 0 and st1 == 0, (tag, st0, st1, bq.last_error())
        assert sw0 == want[name][reorth], (tag, sw0, want[name])
        assert sw1 == sw0, (tag, sw0, sw1)
        assert Q0 is None or torch.equal(_bits(Q1), _bits(Q0)), (tag, "Q changed bits")
        bad = [j for j in range(n) if not _same(R1[:, j], np.ldexp(R0[:, j], int(k[j])))]
        assert not bad, (tag, "columns of R that are not 2^k_j times the unscaled ones", bad[:8])


# ---- 3c: outside the range -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,m,n", [("qr", 4097, 64), ("r", 4097, 64), ("wide", 4097, 64), ("wide", 2063, 130)],
                         ids=["qr-4097x64", "r-4097x64", "wide-4097x64", "wide-2063x130"])
@pytest.mark.parametrize("k", ps.RANGE_K)
def test_a_gram_matrix_outside_the_range_is_never_a_silent_wrong_answer(bq, entry, m, n, k):
    """Gaussian A scaled by 2^k until A^T A overflows (506 at 4097 rows, 520), sits within a factor 2 of the largest double (506 at
    2063 rows), is subnormal (-520) or all zero (-545) -- tests/test_pass_refs_f64_scale.py shows each in numpy.  The call returns
    state 3, or state 0 with Q and 2^-k R inside the header's bands against the unscaled A."""
    a_host = ps.gaussian(m, n)
    a_scaled = ps.scale_uniform(a_host, k)
    for reorth in (0, 1):
        tag = "%s %d x %d k %d reorth %d" % (entry, m, n, k, reorth)
        st, sw, Q, R = _call(bq, entry, a_scaled, reorth)
        print("%s: state %d  sweeps %d" % (tag, st, sw))
        assert st in (0, 3), (tag, st, bq.last_error())
        if st == 0:
            assert np.all(np.isfinite(R)), (tag, "R is not finite")
            R0 = np.ldexp(R, -k)
            assert _same(np.ldexp(R0, k), R), (tag, "R does not rescale exactly")
            _check_bands(tag, entry, a_host, Q, R0, reorth, sw)


# ---- 3d: dependent columns -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", ps.DEPENDENT_SHAPES)
@pytest.mark.parametrize("case", range(4), ids=ps.DEPENDENT_NAMES)
@pytest.mark.parametrize("reorth", [0, 1])
def test_dependent_columns(bq, m, n, case, reorth):
    """Column j0 = n // 2 a copy of its neighbour (a), zero (b), the rounded sum of two others (c), or the whole tail copies of column 0
    (d).  Every entry returns 0 or 3, the same on tsqr_mi_qr_f64, tsqr_mi_qr_f64_wide and the one-rank callback entry (bitwise equal by
    their headers).  State 0: finite Q and R, exact zeros below R's diagonal, a positive diagonal on the j0 independent columns, the
    shifted path for a, b and d, residual <= 1e-13 (CholeskyQR's residual does not depend on conditioning), orthonormal leading columns
    (column j of Z depends on the leading block of G + s I only, a well-conditioned Gaussian Gram matrix: the header's band), and no
    column of Q longer than 1 + 1e-11.  Printed, not asserted: sweeps and the full ||Q^T Q - I||_F."""
    torch = _torch()
    name, a_host, j0 = ps.dependent_matrices(m, n)[case]
    entries = ("qr", "wide", "dist") if n <= 64 else ("wide", "dist")
    out = {}
    for entry in entries + (("r",) if n <= 64 else ()):
        out[entry] = _call(bq, entry, a_host, reorth)
        print("%d x %d %s reorth %d %s: state %d  sweeps %d" % (m, n, name, reorth, entry, out[entry][0], out[entry][1]))
    for entry in out:
        assert out[entry][0] in (0, 3), (entry, out[entry][0], bq.last_error())
    first = out[entries[0]]
    for entry in entries[1:]:
        assert out[entry][0] == first[0] and out[entry][1] == first[1], ("states differ", entries[0], first[:2], entry, out[entry][:2])
        if first[0] == 0:
            assert torch.equal(_bits(out[entry][2]), _bits(first[2])) and _same(out[entry][3], first[3]), (entry, "differs from", entries[0])
    if "r" in out and out["r"][0] == 0:
        _r_shape(out["r"][3], lead=j0)
        assert name.startswith("c_") or out["r"][1] >= 100, ("r", out["r"][1])
    st, sw, Q, R = first
    if st != 0:
        return
    assert bool(torch.isfinite(Q).all()), "Q is not finite"
    _r_shape(R, lead=j0)
    q_host = Q.T.cpu().numpy()
    full = ps.ext_metrics(a_host, q_host, R)[0]
    orth, res, cols = ps.ext_metrics(a_host, q_host, R, lead=j0)
    ql = q_host.astype(p64.LD)
    norms = np.sqrt(np.sum(ql[:, j0:] * ql[:, j0:], axis=0))
    print("%d x %d %s reorth %d: sweeps %d  leading %d columns ||QtQ-I||_F %.2e  full %.2e  residual %.2e  worst column %.2e  "
          "longest of the other columns 1 + %.2e" % (m, n, name, reorth, sw, j0, orth, full, res, cols.max(), float(norms.max() - 1)))
    assert name.startswith("c_") or sw >= 100, (name, sw)
    assert res <= 1e-13, ("residual", res)
    assert orth <= (1e-12 if reorth else 1e-11), ("orthogonality of the leading columns", orth)
    assert float(norms.max() - 1) <= 1e-11, ("a column of Q beyond j0 is longer than 1", float(norms.max() - 1))

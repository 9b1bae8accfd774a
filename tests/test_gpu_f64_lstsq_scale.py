"""The fp64 least-squares entry (tsqr_mi_lstsq_f64 / tsqr_mi_lstsq_f64_lay through blockqr.lstsq_f64) under power-of-two scaling of A and
of B, with B at and beyond the ends of its documented range, and on dependent columns.  Generators, exponents, the documented range and
the longdouble measures: tests/pass_refs_f64_lsq.py on tests/pass_refs_f64_scale.py; tests/test_pass_refs_f64_lsq.py proves on the CPU
that every exponent used for a covariance case keeps Z, the residual, D and X of every pass inside [2^-1000, 2^1000], that a numpy model
of the call has the asserted property bit for bit, and that a D narrowed to float breaks it.

What is asserted follows from the code, not from what the code returns.  Behind the ladder (whose own covariance
tests/test_gpu_f64_scale.py asserts) every operation is a product, an FMA or an MFMA accumulate, Z scales exactly with R, A Z keeps its
bits and everything else is linear in B.  So while no intermediate leaves the normal range, A -> A diag(2^k_c), B -> B diag(2^j_c) gives
the same state, the same sweep count, X' = diag(2^-k_c) X diag(2^j_c) and R' = R diag(2^k_c), bit for bit: uniform k on every rung
(the shift follows a uniform scaling only), per-column k on the unshifted rungs, per-column j everywhere.
Operands as in tests/test_gpu_f64_lstsq.py (its solve_state): padded leading dimensions, NaN guard bands, A and B compared bit for bit
before and after every call; the scaled calls alternate between the column-major and the row-major operands, the unscaled call is made
with both.  Every case prints its figures before it asserts."""
import functools

import numpy as np
import pytest

from tests import pass_refs_f64 as p64
from tests import pass_refs_f64_lsq as pl
from tests import pass_refs_f64_scale as ps
from tests.test_gpu_f64_lstsq import FACTOR, r_only_state, solve, solve_state

pytestmark = pytest.mark.gpu

_IDS = ["%dx%dx%d" % s for s in pl.SCALE_SHAPES]
_UNSHIFTED = ("gauss",) + ps.GRADED_LADDER_ROWS


@functools.lru_cache(maxsize=None)
def _yardstick(m, n, nrhs, name):
    """(X_ref in longdouble, LAPACK's X) of a covariance case: computed once, never written"""
    a, b = pl.scale_case(m, n, nrhs, name)
    return pl.lstsq_ld(a, b), np.linalg.lstsq(a, b, rcond=None)[0]


def _accuracy(tag, m, n, nrhs, name, x, assert_rule):
    """the rule of tests/test_gpu_f64_lstsq.py on the consistent and on the Gaussian columns of B, each against LAPACK on the same columns"""
    ref, xl = _yardstick(m, n, nrhs, name)
    for group, cols in pl.rhs_groups(nrhs):
        err, lapack = pl.column_err(x, ref, cols), pl.column_err(xl, ref, cols)
        print("%s %s columns: err %.3e  lapack %.3e  ratio %.3g  floor %.3e" % (tag, group, err, lapack, err / lapack, pl.floor_of(n)))
        if assert_rule:
            assert err <= max(FACTOR * lapack, pl.floor_of(n)), (tag, group, err, lapack)


def _base(bq, tag, a, b, reorth, refine):
    """the unscaled call in both layouts: the same bits"""
    x0, r0, sw0 = solve(bq, a, b, reorth, refine)
    x1, r1, sw1 = solve(bq, a, b, reorth, refine, colmajor=False)
    assert sw1 == sw0 and pl.same_bits(x1, x0) and pl.same_bits(r1, r0), (tag, "the operand's layout changed the bits")
    return x0, r0, sw0


# ---- 1a: uniform A, uniform B, every rung ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,nrhs", pl.SCALE_SHAPES, ids=_IDS)
@pytest.mark.parametrize("kind", ps.UNIFORM_INPUTS)
@pytest.mark.parametrize("reorth", [0, 1])
def test_uniform_scaling_of_a_and_b_is_bitwise_covariant(bq, m, n, nrhs, kind, reorth):
    """A -> 2^k A, B -> 2^j B for k in {-400, -1, 1, 401} x j in {-400, 0, 401}, refine 0, 1 and 2: X' = 2^(j - k) X and R' = 2^k R
    exactly, with the unscaled call's state and sweep count, on whichever rung the input ends (asserted as in
    tests/test_gpu_f64_scale.py).  The unscaled refine = 1 result meets the accuracy rule where cond <= 1e6 (cond 1e12: printed);
    bitwise covariance carries that to the scaled calls."""
    a, b = pl.scale_case(m, n, nrhs, kind)
    scaled_a = {k: ps.scale_uniform(a, k) for k in pl.SCALE_K}
    scaled_b = {j: ps.scale_uniform(b, j) for j in pl.SCALE_J}
    for refine in pl.SCALE_REFINES:
        tag = "uniform %d x %d nrhs %d %s reorth %d refine %d" % (m, n, nrhs, kind, reorth, refine)
        x0, r0, sw0 = _base(bq, tag, a, b, reorth, refine)
        if kind == "gauss":
            assert sw0 == (2 if reorth else 1), (tag, sw0)
        elif kind == "cond1e12" and n >= 51:
            assert sw0 >= 100, (tag, sw0)
        print("%s: sweeps %d" % (tag, sw0))
        if refine == 1:
            _accuracy(tag, m, n, nrhs, kind, x0, kind != "cond1e12")
        for i, (k, j) in enumerate(pl.uniform_pairs()):
            st, x, r, sw = solve_state(bq, scaled_a[k], scaled_b[j], reorth, refine, colmajor=i % 2 == 0)
            assert st == 0 and sw == sw0, (tag, k, j, st, sw, sw0)
            assert pl.same_bits(r, np.ldexp(r0, k)), (tag, k, j, "R is not 2^k R")
            assert pl.same_bits(x, pl.scale_x(x0, k, j)), (tag, k, j, "X is not 2^(j - k) X")


# ---- 1b: per-column A, unshifted rungs -------------------------------------------------------------------------------------------------------
_GRADED = [(m, n, nrhs, w) for m, n, nrhs in pl.SCALE_SHAPES for w in range(len(_UNSHIFTED) if n > 1 else 1)]


@pytest.mark.parametrize("m,n,nrhs,which", _GRADED, ids=["%dx%dx%d-%s" % (m, n, q, _UNSHIFTED[w].replace(" ", "")) for m, n, q, w in _GRADED])
def test_graded_scaling_of_a_is_bitwise_covariant_on_the_unshifted_rungs(bq, m, n, nrhs, which):
    """A -> A diag(2^k_c), k_c in [-300, 300] with both extremes (pass_refs_f64_scale.graded_k), Gaussian input and the ladder matrices
    on the CholeskyQR2 side: the ladder's own sweep counts, row c of X multiplied by 2^-k_c and column c of R by 2^k_c, exactly"""
    name = _UNSHIFTED[which]
    a, b = pl.scale_case(m, n, nrhs, name)
    k = ps.graded_k(m, n)
    a_scaled = ps.scale_columns(a, k)
    want = {"gauss": (1, 2)}
    want.update({nm: (s0, s1) for nm, _, s0, s1 in p64.ladder_targets(m, n)} if n > 1 else {})
    for reorth in (0, 1):
        for refine in pl.SCALE_REFINES:
            tag = "graded %d x %d nrhs %d %s reorth %d refine %d" % (m, n, nrhs, name, reorth, refine)
            x0, r0, sw0 = _base(bq, tag, a, b, reorth, refine)
            st, x, r, sw = solve_state(bq, a_scaled, b, reorth, refine, colmajor=(reorth + refine) % 2 == 0)
            print("%s: state %d  sweeps %d / %d  (k from %d to %d)" % (tag, st, sw0, sw, k.min(), k.max()))
            if refine == 1:
                _accuracy(tag, m, n, nrhs, name, x0, True)
            assert sw0 == want[name][reorth], (tag, sw0, want[name])
            assert st == 0 and sw == sw0, (tag, st, sw, sw0)
            assert pl.same_bits(r, ps.scale_columns(r0, k)), (tag, "a column of R is not 2^k_c times the unscaled one")
            assert pl.same_bits(x, pl.scale_x(x0, k, 0)), (tag, "a row of X is not 2^-k_c times the unscaled one")


# ---- 1c: per-column B ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,nrhs", pl.SCALE_SHAPES, ids=_IDS)
@pytest.mark.parametrize("kind", ps.UNIFORM_INPUTS)
def test_graded_scaling_of_b_is_bitwise_covariant(bq, m, n, nrhs, kind):
    """B -> B diag(2^j_c), j_c in [-400, 400] with both extremes: column c of X is multiplied by 2^j_c exactly and R keeps its bits, on
    every rung.  Then one column alone is scaled by 2^400: every other column of X keeps its bits -- B enters the residual through
    products with the zeros of an identity operand, and those products stay zeros."""
    a, b = pl.scale_case(m, n, nrhs, kind)
    j = pl.b_exponents(m, n, nrhs)
    b_scaled = ps.scale_columns(b, j)
    c = nrhs // 2
    b_one = pl.scale_one_column(b, c, pl.B_SPAN)
    others = [i for i in range(nrhs) if i != c]
    for reorth in (0, 1):
        for refine in pl.SCALE_REFINES:
            tag = "columns of B %d x %d nrhs %d %s reorth %d refine %d" % (m, n, nrhs, kind, reorth, refine)
            x0, r0, sw0 = _base(bq, tag, a, b, reorth, refine)
            st, x, r, sw = solve_state(bq, a, b_scaled, reorth, refine, colmajor=(reorth + refine) % 2 == 1)
            st1, x1, r1, sw1 = solve_state(bq, a, b_one, reorth, refine, colmajor=(reorth + refine) % 2 == 0)
            print("%s: states %d %d  sweeps %d / %d / %d  (j from %d to %d)" % (tag, st, st1, sw0, sw, sw1, j.min(), j.max()))
            assert st == 0 and st1 == 0 and sw == sw0 and sw1 == sw0, (tag, st, st1, sw, sw1, sw0)
            assert pl.same_bits(r, r0) and pl.same_bits(r1, r0), (tag, "B changed R")
            assert pl.same_bits(x, pl.scale_x(x0, 0, j)), (tag, "a column of X is not 2^j_c times the unscaled one")
            assert pl.same_bits(x1[:, c], np.ldexp(x0[:, c], pl.B_SPAN)), (tag, "the scaled column")
            assert pl.same_bits(x1[:, others], x0[:, others]), (tag, "a column of B that was not scaled changed its column of X")


# ---- 2: B at and beyond the ends of its documented range -------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,nrhs", pl.RANGE_SHAPES, ids=["%dx%dx%d" % s for s in pl.RANGE_SHAPES])
@pytest.mark.parametrize("kind", pl.RHS_KINDS)
def test_b_at_and_beyond_the_ends_of_its_range(bq, m, n, nrhs, kind):
    """Gaussian A, one column of B scaled by 2^j (tests/test_pass_refs_f64_lsq.py shows every j on the data).  j just inside each end of
    the range in include/tsqr_mi.h: the column of X, scaled back exactly, meets the accuracy rule.  j beyond each end: that column is
    not finite, or meets the rule all the same -- never a finite wrong answer.  Every other column of X keeps its bits throughout."""
    a, b = pl.range_case(m, n, nrhs, kind)
    c = pl.RANGE_COLUMN
    others = [i for i in range(nrhs) if i != c]
    ref = pl.lstsq_ld(a, b)
    lapack = pl.column_err(np.linalg.lstsq(a, b, rcond=None)[0], ref, [c])
    bound = max(FACTOR * lapack, pl.floor_of(n))
    for reorth in (0, 1):
        for refine in (1, 2):
            tag = "range %d x %d %s reorth %d refine %d" % (m, n, kind, reorth, refine)
            x0, r0, sw0 = _base(bq, tag, a, b, reorth, refine)
            print("%s: unscaled err of column %d %.3e  lapack %.3e" % (tag, c, pl.column_err(x0, ref, [c]), lapack))
            for i, (j, inside) in enumerate([(j, True) for j in pl.RANGE_J_INSIDE] + [(j, False) for j in pl.RANGE_J_BEYOND]):
                st, x, r, sw = solve_state(bq, a, pl.scale_one_column(b, c, j), reorth, refine, colmajor=i % 2 == 0)
                assert st == 0 and sw == sw0 and pl.same_bits(r, r0), (tag, j, st, sw)
                finite = bool(np.all(np.isfinite(x[:, c])))
                with np.errstate(over="ignore", under="ignore"):
                    xc = np.ldexp(x[:, c], -j)
                err = pl.rel_err(xc[:, None], ref[:, [c]]) if finite else float("nan")
                print("%s: j %5d (%s)  column finite %s  err after rescaling %.3e  bound %.3e  same bits as the unscaled column %s"
                      % (tag, j, "inside" if inside else "beyond", finite, err, bound, finite and pl.same_bits(xc, x0[:, c])))
                assert pl.same_bits(x[:, others], x0[:, others]), (tag, j, "a column of B that was not scaled changed its column of X")
                if inside:
                    assert finite and err <= bound, (tag, j, err, bound)
                else:
                    assert (not finite) or err <= bound, (tag, j, "a finite wrong column with state 0", err, bound)


# ---- 4: dependent columns --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,nrhs", pl.DEPENDENT_SHAPES, ids=["%dx%dx%d" % s for s in pl.DEPENDENT_SHAPES])
@pytest.mark.parametrize("case", range(4), ids=ps.DEPENDENT_NAMES)
@pytest.mark.parametrize("reorth", [0, 1])
def test_dependent_columns(bq, m, n, nrhs, case, reorth):
    """pass_refs_f64_scale.dependent_matrices (a copied column, a zero column, a rounded sum of two columns, a tail of copies); B with
    consistent (even) and Gaussian (odd) columns.  The state is 0 or 3 and, with the sweep count, that of tsqr_mi_r_f64 on the same A;
    on state 0 R is that entry's bit for bit, and a second call and the row-major call return the same bits of X.  Printed, not
    asserted (nothing in the code bounds them): whether X is finite, and ||B - A X||_F next to the minimum in longdouble with the
    dependent columns pivoted out, for the consistent and for the Gaussian columns."""
    name, a, j0 = ps.dependent_matrices(m, n)[case]
    b = pl.scale_rhs(a, nrhs, ps.shape_seed(m, n, 19))
    keep = pl.independent_columns(name, n, j0)
    tag = "dependent %d x %d nrhs %d %s reorth %d" % (m, n, nrhs, name, reorth)
    st_r, r_r, sw_r = r_only_state(bq, a, reorth)
    st, x, r, sw = solve_state(bq, a, b, reorth, 1)
    print("%s: state %d (r_f64: %d)  sweeps %d (r_f64: %d)" % (tag, st, st_r, sw, sw_r))
    assert st in (0, 3), (tag, st, bq.last_error())
    assert st == st_r and sw == sw_r, (tag, "the state or the sweeps differ from r_f64's", st, st_r, sw, sw_r)
    st2, x2, r2, sw2 = solve_state(bq, a, b, reorth, 1)
    st3, x3, r3, sw3 = solve_state(bq, a, b, reorth, 1, colmajor=False)
    assert (st2, sw2) == (st, sw) and (st3, sw3) == (st, sw), (tag, "a second call or the row-major call ends differently")
    if st != 0:
        return
    assert pl.same_bits(r, r_r), (tag, "R differs from r_f64's")
    finite = bool(np.all(np.isfinite(x)))
    for group, cols in pl.rhs_groups(nrhs):
        got = pl.residual_ld(a, b[:, cols], x[:, cols]) if finite else float("nan")
        print("%s %s columns: X finite %s  largest |X| %.3e  ||B - A X||_F %.3e  minimum %.3e  ||B||_F %.3e"
              % (tag, group, finite, float(np.abs(x[:, cols]).max()), got, pl.min_residual_ld(a, b[:, cols], keep),
                 float(np.linalg.norm(b[:, cols]))))
    assert np.array_equal(x2.view(np.int64), x.view(np.int64)) and pl.same_bits(r2, r), (tag, "a second call gives other bits")
    assert np.array_equal(x3.view(np.int64), x.view(np.int64)) and pl.same_bits(r3, r), (tag, "the operand's layout changed the bits")

"""CPU checks of tests/pass_refs_f64_lsq.py: the exact reference of the least-squares pass agrees with a model of the pass, every seeded
defect of the model is caught by the comparison the GPU tests make, and the numpy model of the whole call passes the accuracy check of
tests/test_gpu_f64_lstsq.py on that test's own inputs -- the algorithm itself can meet what the entry is asked to meet.  Every accuracy
case prints its figures (profiles/fp64_lstsq_accuracy.md records them)."""
import functools

import numpy as np
import pytest

from tests import pass_refs_f64_lsq as pl


@pytest.mark.parametrize("m,n,nrhs", [(1, 1, 1), (17, 17, 5), (100, 33, 16), (4099, 64, 16)])
def test_model_matches_exact_reference(m, n, nrhs):
    a, z, x, b = pl.exact_case(np.random.default_rng(m + n + nrhs), m, n, nrhs)
    want = pl.pack_d(pl.d_exact(a, z, x, b), n)
    assert np.array_equal(pl.model_pass(a, z, x, b), want)
    d = pl.unpack_d(want, n)
    assert np.array_equal(d[:n, :nrhs], pl.d_exact(a, z, x, b)) and not d[n:].any() and not d[:, nrhs:].any()
    assert np.array_equal(pl.model_pass(a, z, np.zeros_like(x), b), pl.pack_d(pl.d_exact(a, z, None, b), n))


@pytest.mark.parametrize("defect", ["x_sign", "drop_tail_row", "swap_ti"])
@pytest.mark.parametrize("m,n,nrhs", [(33, 17, 1), (100, 64, 16)])
def test_exact_check_bites(m, n, nrhs, defect):
    a, z, x, b = pl.exact_case(np.random.default_rng(7 * m + n), m, n, nrhs)
    want = pl.pack_d(pl.d_exact(a, z, x, b), n)
    assert not np.array_equal(pl.model_pass(a, z, x, b, defect), want)


def test_layouts():
    x = np.arange(1.0, 7.0).reshape(3, 2)
    v = pl.pad_x(x, 3)
    assert v.shape == (256,) and v[0] == 1.0 and v[16 + 2] == 6.0 and v[2 * 16] == 0.0
    assert np.array_equal(pl.unpad_x(v, 3)[:3, :2], x)
    d = np.arange(1.0, 1.0 + 17 * 2).reshape(17, 2)
    w = pl.pack_d(d, 17)
    # D[5][1]: tile 0, row 5 = lq 1 + 4 * reg 1, lane 16 * 1 + 1;  D[16][0]: tile 1, register 0, lane 0
    assert w.shape == (512,) and w[(0 * 4 + 1) * 64 + 17] == d[5, 1] and w[256] == d[16, 0]
    assert np.array_equal(pl.unpack_d(w, 17)[:17, :2], d)


def test_explicit_inverse_and_reference_solve():
    rng = np.random.default_rng(2)
    a, b = rng.standard_normal((300, 9)), rng.standard_normal((300, 4))
    r = pl.householder_r(a)
    assert np.all(np.diag(r) > 0) and np.abs(pl.explicit_inverse(r) @ r - np.eye(9)).max() < 1e-13
    x = pl.lstsq_ld(a, b)
    assert pl.normal_residual(a, b, x) < 1e-17                   # (longdouble: far below fp64 rounding)
    assert pl.rel_err(np.linalg.lstsq(a, b, rcond=None)[0], x) < 1e-14


@functools.lru_cache(maxsize=None)
def model_figures(case):
    """(error of refine 0 .. 4, error of numpy's lstsq), all against the longdouble Householder solve"""
    _, m, n, nrhs, cond, kind = case
    a, b = pl.accuracy_input(m, n, nrhs, cond, kind)
    ref = pl.lstsq_ld(a, b)
    errs = [pl.rel_err(pl.model_lstsq(a, b, k)[0], ref) for k in (0, 1, 2, 3, 4)]
    return errs, pl.rel_err(np.linalg.lstsq(a, b, rcond=None)[0], ref)


# the factor of the GPU test's assertion (tests/test_gpu_f64_lstsq.py says how it was fixed); the model's largest ratio is 0.62
# (profiles/fp64_lstsq_accuracy.md)
MODEL_FACTOR = 2.0


@pytest.mark.parametrize("case", pl.accuracy_cases(), ids=lambda c: c[0])
def test_model_meets_the_accuracy_check(case):
    (e0, e1, e2, e3, e4), lapack = model_figures(case)
    n = case[2]
    print("model %-32s refine 0 %.3e  1 %.3e  2 %.3e  3 %.3e  4 %.3e  lapack %.3e  ratio(refine 1) %.3g  floor %.3e"
          % (case[0], e0, e1, e2, e3, e4, lapack, e1 / lapack if lapack > 0 else float(e1 > 0), pl.floor_of(n)))
    assert e1 <= max(MODEL_FACTOR * lapack, pl.floor_of(n))
    assert e2 <= 2.0 * max(e1, pl.floor_of(n))
    assert e3 <= 2.0 * max(e2, pl.floor_of(n)) and e4 <= 2.0 * max(e2, pl.floor_of(n))      # (the GPU test's rule for refine 3 and 4)


def test_accuracy_check_bites():
    """a correction formed from B + A X doubles the error instead of removing it: far outside the band"""
    case = [c for c in pl.accuracy_cases() if c[0].startswith("cond1e+04") and c[5] == "gaussian"][0]
    _, m, n, nrhs, cond, kind = case
    a, b = pl.accuracy_input(m, n, nrhs, cond, kind)
    ref = pl.lstsq_ld(a, b)
    lapack = pl.rel_err(np.linalg.lstsq(a, b, rcond=None)[0], ref)
    bad = pl.rel_err(pl.model_lstsq(a, b, 1, defect="x_sign")[0], ref)
    assert bad > 64.0 * max(lapack, pl.floor_of(n))


# ---- the scaling tests of the entry (tests/test_gpu_f64_lstsq_scale.py): ranges, the model's own covariance, a seeded defect ------------------
from tests import pass_refs_f64_scale as ps

_SCALE_IDS = ["%dx%dx%d" % s for s in pl.SCALE_SHAPES]
_UNSHIFTED = ("gauss",) + ps.GRADED_LADDER_ROWS


def _graded_names(n):
    return _UNSHIFTED if n > 1 else ("gauss",)


@functools.lru_cache(maxsize=None)
def _trace(m, n, nrhs, name):
    a, b = pl.scale_case(m, n, nrhs, name)
    return pl.model_trace(a, b, max(pl.SCALE_REFINES))


def test_model_trace_is_the_model():
    a, b = pl.scale_case(300, 17, 3, "cond1e6")
    for refine in (0, 2, 4):
        t = pl.model_trace(a, b, refine)
        x, r = pl.model_lstsq(a, b, refine)
        assert pl.same_bits(t[0], x) and pl.same_bits(t[1], r) and len(t[4]) == refine + 1 and pl.same_bits(t[5][-1], x)


def test_scale_x_is_exact_and_says_so_when_it_is_not():
    x = np.random.default_rng(3).standard_normal((5, 3))
    y = pl.scale_x(x, np.array([1, -2, 300, 0, -400]), np.array([0, 401, -400]))
    assert y[2, 1] == np.ldexp(x[2, 1], 101) and y[4, 2] == x[4, 2] and pl.same_bits(pl.scale_x(x, 3, 3), x)
    with pytest.raises(AssertionError, match="left the normal range"):
        pl.scale_x(x, 700, -400)


@pytest.mark.parametrize("m,n,nrhs", pl.SCALE_SHAPES, ids=_SCALE_IDS)
def test_covariance_exponents_keep_every_intermediate_in_range(m, n, nrhs):
    """Z, the residual, D = (A Z)^T (B - A X) and X of every pass -- the correction passes of the consistent columns carry a residual
    and a D of rounding size -- for every (input, k, j) of the uniform section, the graded exponents of A and the per-column exponents
    of B: the non-zero magnitudes stay inside [2^-1000, 2^1000], taken in longdouble from the unscaled model's trace"""
    lo, hi, worst = np.inf, -np.inf, None
    todo = [(kind, k, j) for kind in ps.UNIFORM_INPUTS for k, j in pl.uniform_pairs()]
    todo += [(name, ps.graded_k(m, n), 0) for name in _graded_names(n)]
    todo += [(kind, 0, pl.b_exponents(m, n, nrhs)) for kind in ps.UNIFORM_INPUTS]
    for name, k, j in todo:
        a, b = pl.scale_case(m, n, nrhs, name)
        ps.scale_columns(a, np.broadcast_to(np.asarray(k, dtype=np.int64), (n,)))            # (exact: asserted there)
        ps.scale_columns(b, np.broadcast_to(np.asarray(j, dtype=np.int64), (nrhs,)))
        for what, (l, h) in pl.scaled_spans(_trace(m, n, nrhs, name), k, j).items():
            if l < lo:
                lo, worst = l, (name, what, np.min(k), np.max(j))
            hi = max(hi, h)
            assert -pl.RANGE_LOG2 <= l and h <= pl.RANGE_LOG2, (name, what, k, j, l, h)
    print("%d x %d, nrhs %d: log2 of the non-zero intermediates from %.1f to %.1f (lowest: %s)" % (m, n, nrhs, lo, hi, worst))
    jb = pl.b_exponents(m, n, nrhs)
    assert nrhs < 2 or (jb.min() == -pl.B_SPAN and jb.max() == pl.B_SPAN)


def _scaled_model(m, n, nrhs, name, k, j, refine, round_d=None):
    a, b = pl.scale_case(m, n, nrhs, name)
    ak = ps.scale_columns(a, np.broadcast_to(np.asarray(k, dtype=np.int64), (n,)))
    bj = ps.scale_columns(b, np.broadcast_to(np.asarray(j, dtype=np.int64), (nrhs,)))
    t = pl.model_trace(ak, bj, refine, round_d)
    return t[0], t[1]


@pytest.mark.parametrize("m,n,nrhs", pl.SCALE_SHAPES, ids=_SCALE_IDS)
def test_model_is_bitwise_covariant(m, n, nrhs):
    """the model of the call (Householder R, explicit inverse, products) on the data of the GPU test: X' = diag(2^-k) X diag(2^j) and
    R' = R diag(2^k) bit for bit -- the property the GPU test asserts is one that fp64 arithmetic of this kind has"""
    refine = max(pl.SCALE_REFINES)
    todo = [(kind, k, j) for kind in ps.UNIFORM_INPUTS for k, j in pl.uniform_pairs()]
    todo += [(name, ps.graded_k(m, n), 0) for name in _graded_names(n)]
    todo += [(kind, 0, pl.b_exponents(m, n, nrhs)) for kind in ps.UNIFORM_INPUTS]
    for name, k, j in todo:
        x0, r0 = _trace(m, n, nrhs, name)[:2]
        x, r = _scaled_model(m, n, nrhs, name, k, j, refine)
        assert pl.same_bits(x, pl.scale_x(x0, k, j)), (name, k, j, "X")
        assert pl.same_bits(r, ps.scale_columns(r0, np.broadcast_to(np.asarray(k, dtype=np.int64), (n,)))), (name, k, j, "R")


@pytest.mark.parametrize("m,n,nrhs", [(1029, 51, 5), (100, 7, 1)])
def test_covariance_check_bites_on_a_narrowed_d(m, n, nrhs):
    """the seeded defect: D rounded to float32.  At k = 401 the check fails as soon as B moves too -- D does not depend on k at all
    (A Z keeps its bits), so it is the pairs (401, -400) and (401, 401) that leave float's range: D is zero or infinite there.  On the
    unscaled data the correction pass repairs what the narrowed D of the pass before it lost, and the accuracy rule is met: inputs of
    magnitude 1 cannot show this defect, which is why the scaled pairs exist."""
    a, b = pl.scale_case(m, n, nrhs, "gauss")
    x0 = pl.model_trace(a, b, 1, np.float32)[0]
    for j in (-400, 401):
        x = _scaled_model(m, n, nrhs, "gauss", 401, j, 1, np.float32)[0]
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            want = np.ldexp(x0, j - 401)
        assert not pl.same_bits(x, want), j
    ref = pl.lstsq_ld(a, b)
    lapack = pl.rel_err(np.linalg.lstsq(a, b, rcond=None)[0], ref)
    assert pl.rel_err(x0, ref) <= max(MODEL_FACTOR * lapack, pl.floor_of(n))


@pytest.mark.parametrize("m,n,nrhs", pl.SCALE_SHAPES, ids=_SCALE_IDS)
def test_model_meets_the_accuracy_rule_on_the_scale_inputs(m, n, nrhs):
    """the rule of tests/test_gpu_f64_lstsq.py, on the consistent and on the Gaussian columns separately, where cond <= 1e6"""
    for kind in ("gauss", "cond1e6") + ps.GRADED_LADDER_ROWS[:len(_graded_names(n)) - 1]:
        a, b = pl.scale_case(m, n, nrhs, kind)
        ref = pl.lstsq_ld(a, b)
        xl = np.linalg.lstsq(a, b, rcond=None)[0]
        x = pl.model_lstsq(a, b, 1)[0]
        for group, cols in pl.rhs_groups(nrhs):
            err, lapack = pl.column_err(x, ref, cols), pl.column_err(xl, ref, cols)
            print("model %d x %d %-14s %-10s columns: refine 1 %.3e  lapack %.3e  ratio %.3g" % (m, n, kind, group, err, lapack, err / lapack))
            assert err <= max(MODEL_FACTOR * lapack, pl.floor_of(n)), (kind, group, err, lapack)


@pytest.mark.parametrize("m,n,nrhs", pl.RANGE_SHAPES, ids=["%dx%dx%d" % s for s in pl.RANGE_SHAPES])
@pytest.mark.parametrize("kind", pl.RHS_KINDS)
def test_range_exponents_of_b(m, n, nrhs, kind):
    """section 2: each chosen j, from the data.  Inside: the scaled column's norm lies in the documented range, with less than 2^16 to
    spare at its end, and the model meets the accuracy rule on the rescaled column.  Beyond: the norm lies outside; the entries of B are
    still normal, finite and exactly scaled (scale_columns asserts it), so the test's own rescaling is exact.  The figures say what
    leaves the range: u ||b|| (the residual of a consistent system) is subnormal at the low end, ||b||^2 overflows at the high end."""
    a, b = pl.range_case(m, n, nrhs, kind)
    c = pl.RANGE_COLUMN
    lo, hi = pl.b_range_log2(a)
    norm = float(np.log2(np.linalg.norm(b[:, c])))
    ref = pl.lstsq_ld(a, b)
    lapack = pl.column_err(np.linalg.lstsq(a, b, rcond=None)[0], ref, [c])
    print("%d x %d %s: documented log2 ||b|| in [%.1f, %.1f], log2 ||b_c|| = %.1f" % (m, n, kind, lo, hi, norm))
    for j, inside in [(j, True) for j in pl.RANGE_J_INSIDE] + [(j, False) for j in pl.RANGE_J_BEYOND]:
        bj = pl.scale_one_column(b, c, j)
        assert np.all(np.isfinite(bj)) and np.all((bj[:, c] == 0) | (np.abs(bj[:, c]) >= np.finfo(np.float64).tiny))
        assert (lo <= norm + j <= hi) == inside, (j, norm + j, lo, hi)
        if inside:
            assert min(norm + j - lo, hi - (norm + j)) <= 16.0, (j, "not at an end of the range")
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            x = pl.model_lstsq(a, bj, 1)[0]
            tiny_res = float(np.ldexp(np.linalg.norm(b[:, c]) * pl.U, j))
            sq = np.float64(np.ldexp(np.linalg.norm(b[:, c]), j)) ** 2
            xc = np.ldexp(x[:, c], -j)
        finite = bool(np.all(np.isfinite(x[:, c])))
        err = pl.rel_err(xc[:, None], ref[:, [c]]) if finite else float("nan")
        others = [i for i in range(nrhs) if i != c]
        print("  j %5d (%s): u ||b_c|| 2^j = %.3e  (||b_c|| 2^j)^2 = %.3e  model: column finite %s, err after rescaling %.3e (lapack %.3e)"
              % (j, "inside" if inside else "beyond", tiny_res, sq, finite, err, lapack))
        assert pl.same_bits(x[:, others], pl.model_lstsq(a, b, 1)[0][:, others]), "the model's other columns moved"
        if inside:
            assert finite and err <= max(MODEL_FACTOR * lapack, pl.floor_of(n)), (j, err, lapack)
        elif j < 0:
            assert tiny_res < np.finfo(np.float64).tiny
        else:
            assert np.isinf(sq)


@pytest.mark.parametrize("m,n,nrhs", pl.DEPENDENT_SHAPES, ids=["%dx%dx%d" % s for s in pl.DEPENDENT_SHAPES])
def test_min_residual_of_the_dependent_cases(m, n, nrhs):
    """pivoting the dependent columns out leaves a full-rank matrix whose least-squares residual is the minimum over all of A's range:
    zero to rounding for B = A X*, and no column of the full A improves it (A^T of the residual vanishes to rounding)"""
    for name, a, j0 in ps.dependent_matrices(m, n):
        keep = pl.independent_columns(name, n, j0)
        assert np.linalg.matrix_rank(a[:, keep]) == keep.size
        b = pl.scale_rhs(a, nrhs, ps.shape_seed(m, n, 19))
        al, bl = a.astype(pl.LD), b.astype(pl.LD)
        e = bl - al[:, keep] @ pl.lstsq_ld(a[:, keep], b)
        g = al.T @ e
        rel = float(np.sqrt(np.sum(g * g)) / (np.sqrt(np.sum(al * al)) * np.sqrt(np.sum(bl * bl))))
        print("%d x %d %s: min ||B - A X||_F %.3e (consistent columns %.3e)  ||At e||_F / (||A||_F ||B||_F) %.3e"
              % (m, n, name, pl.min_residual_ld(a, b, keep), float(np.sqrt(np.sum(e[:, 0::2] ** 2))), rel))
        assert rel <= 1e-15
        assert float(np.sqrt(np.sum(e[:, 0::2] ** 2))) <= 1e-11 * float(np.sqrt(np.sum(bl[:, 0::2] ** 2)))


def test_stagnation_rule_keeps_later_refinements_from_redrawing_the_error():
    """300 x 17, cond 1e6, consistent B with 3 right-hand sides, 60 fresh matrices: with every correction applied err_3 or err_4 ends
    more than twice above err_2 on some of them (the GPU test's rule for refine 3 and 4 fails by rounding noise alone); under the
    stagnation rule of lsq_update_f64_kernel it does on none.  refine <= 1 does not see the rule."""
    from tests import pass_refs_f64_r as p64r
    m, n, nrhs, cond = 300, 17, 3, 1e6
    worst = {}
    for defect in ("no_stagnation_rule", None):
        ratios = []
        for seed in range(60):
            a = p64r.cond_matrix(m, n, cond, seed + 5000)
            b = a @ np.random.default_rng(seed + 9).standard_normal((n, nrhs))
            ref = pl.lstsq_ld(a, b)
            e = {k: pl.rel_err(pl.model_lstsq(a, b, k, defect)[0], ref) for k in (2, 3, 4)}
            ratios += [e[3] / max(e[2], pl.floor_of(n)), e[4] / max(e[2], pl.floor_of(n))]
            if seed < 4:
                assert pl.same_bits(pl.model_lstsq(a, b, 1, defect)[0], pl.model_lstsq(a, b, 1, "no_stagnation_rule")[0])
        worst[defect] = (max(ratios), sum(r > 2.0 for r in ratios))
        print("%s: largest err_3 / err_2, err_4 / err_2 %.2f, %d of %d above 2" % (defect or "with the rule", worst[defect][0], worst[defect][1], len(ratios)))
    assert worst["no_stagnation_rule"][1] >= 1 and worst[None][1] == 0


def test_stagnation_step():
    d1 = np.array([[8.0, 8.0, 8.0, np.nan], [-1.0, 1.0, 0.0, 1.0]])
    x, st = pl.stagnation_step(None, d1.copy(), d1, None, 0)
    assert np.array_equal(st, [8.0, 8.0, 8.0, 1.0])
    d2 = np.array([[4.0, 4.5, 1.0, 0.25], [0.0, 0.0, 0.0, 0.0]])
    one = np.ones_like(d2)
    x2, st2 = pl.stagnation_step(np.zeros_like(d2), one, d2, st, 2)              # 4 <= 8 / 2 applies, 4.5 does not and stops
    assert np.array_equal(x2[0], [1.0, 0.0, 1.0, 1.0]) and np.array_equal(st2, [4.0, -1.0, 1.0, 0.25])
    x3, st3 = pl.stagnation_step(x2, one, d2 / 4, st2, 3)                        # a stopped column stays stopped
    assert np.array_equal(x3[0], [2.0, 0.0, 2.0, 2.0]) and st3[1] == -1.0
    x4, _ = pl.stagnation_step(x2, one, d2 * 8, st2, 1)                          # the first correction is always applied
    assert np.array_equal(x4[0], [2.0, 1.0, 2.0, 2.0])

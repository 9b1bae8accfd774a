"""CPU check of tests/pass_refs_f64_scale.py: the generators are exact and deterministic; every exponent the covariance tests use keeps
the Gram matrix inside [2^-1000, 2^1000] (from the generated data); every out-of-range exponent does what its test says it does to
A^T A in numpy's fp64; Householder QR on the unscaled Gaussian inputs meets the header's bands under ext_metrics, so the conditions the
GPU tests impose are ones the measure itself can meet."""
import numpy as np
import pytest

from tests import pass_refs_f64 as p64
from tests import pass_refs_f64_scale as ps

ALL_SHAPES = tuple(dict.fromkeys(ps.NARROW_SHAPES + ps.WIDE_SHAPES + ps.DIST_SHAPES))


def _same_bits(x, y):
    return np.array_equal(np.ascontiguousarray(x).view(np.int64), np.ascontiguousarray(y).view(np.int64))


# ---- generators ------------------------------------------------------------------------------------------------------------------------------
def test_scale_columns_is_exact_and_says_so_when_it_is_not():
    rng = np.random.default_rng(1)
    a = p64.full_mantissa64(rng, (33, 5))
    k = np.array([-400, -1, 0, 1, 401])
    b = ps.scale_columns(a, k)
    m0, e0 = np.frexp(a)
    m1, e1 = np.frexp(b)
    assert _same_bits(m0, m1) and np.array_equal(e1 - e0, np.broadcast_to(k, a.shape))   # same significands, exponents moved by k_j
    assert _same_bits(ps.scale_uniform(a, 7), a * 128.0)
    z = a.copy(); z[:, 2] = 0.0; z[0, 0] = -0.0
    assert _same_bits(ps.scale_columns(z, k)[:, 2], z[:, 2]) and np.signbit(ps.scale_columns(z, k)[0, 0])
    with pytest.raises(AssertionError, match="left the normal range"):
        ps.scale_uniform(a, -1060)                          # subnormal results lose bits
    with pytest.raises(AssertionError, match="left the normal range"):
        ps.scale_uniform(a, 1030)                           # overflow
    with pytest.raises(AssertionError):
        ps.scale_columns(a, np.array([1.0, 2.0, 3.0, 4.0, 5.0]))


@pytest.mark.parametrize("n", [1, 2, 3, 7, 64, 200])
def test_graded_exponents(n):
    span = ps.GRADED_SPAN
    k = ps.graded_exponents(np.random.default_rng(n), n, span)
    assert k.shape == (n,) and np.issubdtype(k.dtype, np.integer)
    assert np.all(np.abs(k) <= span)
    if n >= 2:
        assert k.min() == -span and k.max() == span
    if n >= 3:
        assert np.any(k % 2 == 0) and np.any(k % 2 != 0)
    assert np.array_equal(k, ps.graded_exponents(np.random.default_rng(n), n, span)), "not deterministic"
    if n >= 64:                                              # random order: the extremes are not left where they were put
        ks = [ps.graded_exponents(np.random.default_rng(s), n, span) for s in range(8)]
        assert len({int(np.argmin(x)) for x in ks}) > 1 and len({int(np.argmax(x)) for x in ks}) > 1
    m, nn = ps.NARROW_SHAPES[0]
    assert np.array_equal(ps.graded_k(m, nn), ps.graded_k(m, nn))


@pytest.mark.parametrize("m,n", [(100, 7), (65, 4), (300, 51)])
def test_dependent_cases(m, n):
    cases = ps.dependent_cases(np.random.default_rng(5), m, n)
    again = ps.dependent_cases(np.random.default_rng(5), m, n)
    base = np.random.default_rng(5).standard_normal((m, n))
    assert [c[0] for c in cases] == list(ps.DEPENDENT_NAMES)
    j0 = n // 2
    for (name, a, j), (_, a2, _) in zip(cases, again):
        assert j == j0 and a.shape == (m, n) and _same_bits(a, a2)
        assert np.linalg.matrix_rank(a[:, :j0]) == j0           # j0 leading independent columns
        touched = np.zeros(n, bool)
        touched[j0 if name != ps.DEPENDENT_NAMES[3] else slice(j0, n)] = True
        assert _same_bits(a[:, ~touched], base[:, ~touched]), "a column outside the modification changed"
    a, b, c, d = (x[1] for x in cases)
    assert _same_bits(a[:, j0], a[:, j0 - 1])
    assert np.all(b[:, j0] == 0.0) and not np.signbit(b[:, j0]).any()
    assert _same_bits(c[:, j0], c[:, 0] + c[:, 1])
    exact = c[:, 0].astype(p64.LD) + c[:, 1].astype(p64.LD)
    assert np.any(exact != c[:, j0].astype(p64.LD)), "case c is meant to be dependent to rounding only"
    for j in range(j0, n):
        assert _same_bits(d[:, j], d[:, 0])
    # the rank the names promise: a, b, d exactly deficient; c full rank in exact arithmetic but with cond ~ 1 / u
    sv = [np.linalg.svd(x, compute_uv=False) for x in (a, b, c, d)]
    assert sv[0][-1] <= 1e-13 * sv[0][0] and sv[1][-1] <= 1e-13 * sv[1][0] and sv[3][j0] <= 1e-13 * sv[3][0]
    assert sv[2][-1] <= 1e-13 * sv[2][0] and sv[2][-2] > 1e-3 * sv[2][0]


def test_dependent_cases_one_column():
    (name, a, j0), = ps.dependent_cases(np.random.default_rng(5), 65, 1)
    assert name == "unmodified" and j0 == 1 and _same_bits(a, np.random.default_rng(5).standard_normal((65, 1)))


def test_shared_inputs_are_deterministic_and_read_only():
    m, n = 100, 7
    for get in (lambda: ps.gaussian(m, n), lambda: ps.cond_matrix(m, n, 1e6), lambda: ps.graded_inputs(m, n)[1][1],
                lambda: ps.dependent_matrices(m, n)[0][1]):
        x = get()
        assert x is get() and not x.flags.writeable
    assert _same_bits(ps.gaussian(m, n), np.random.default_rng(ps.shape_seed(m, n)).standard_normal((m, n)))
    c = np.linalg.cond(ps.cond_matrix(m, n, 1e6))
    assert 0.99e6 <= c <= 1.01e6, c
    assert [x[0] for x in ps.graded_inputs(m, n)] == ["gauss"] + list(ps.GRADED_LADDER_ROWS)
    assert [x[0] for x in ps.graded_inputs(65, 1)] == ["gauss"]


def test_ext_metrics_against_known_defects():
    """an orthonormal Q with a prescribed defect: each measure returns what was put in, to longdouble rounding"""
    rng = np.random.default_rng(2)
    m, n = 200, 9
    q, _ = np.linalg.qr(rng.standard_normal((m, n)))
    r = np.triu(rng.standard_normal((n, n))) + 4.0 * np.eye(n)
    ql = q.astype(p64.LD)
    a = np.asarray(ql @ r.astype(p64.LD), np.float64)        # A = fl(Q R): residual at the level of u
    orth, res, cols = ps.ext_metrics(a, q, r)
    assert orth <= 1e-14 and res <= 2 * p64.U and cols.shape == (n,) and cols.max() <= 4 * p64.U
    q2 = q.copy(); q2[:, 3] *= 1.0 + 1e-9                    # diagonal entry 3 of Q^T Q - I becomes 2e-9
    orth2, _, cols2 = ps.ext_metrics(a, q2, r)
    assert abs(orth2 - 2e-9) <= 1e-12
    assert ps.ext_metrics(a, q2, r, lead=3)[0] <= 1e-14      # the leading block does not see column 3
    assert np.argmax(cols2) >= 3 and cols2[:3].max() <= 4 * p64.U      # columns 0 .. 2 do not use column 3 of Q
    a0 = a.copy(); a0[:, 4] = 0.0
    r0 = r.copy(); r0[:, 4] = 0.0
    assert ps.ext_metrics(a0, q, r0)[2].shape == (n - 1,)    # the zero column is skipped
    # differences far below fp64's reach: ||A - Q R|| of an A that is Q R rounded to fp64 is not zero, and is below u ||A||
    assert 0.0 < res


# ---- the ranges ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", ALL_SHAPES)
def test_covariance_exponents_keep_the_gram_matrix_normal_with_margin(m, n):
    """sections 3a and 3b: m max|a_j|^2 2^(2 k_j) and its reciprocal inside [2^-1000, 2^1000] for every column of every input at every
    exponent, from the generated data; and the scalings themselves are exact (scale_columns asserts it)"""
    seen = []
    for kind in ps.UNIFORM_INPUTS:
        a = ps.uniform_input(kind, m, n)
        for k in ps.UNIFORM_K:
            ps.scale_uniform(a, k)
            seen.append(ps.log2_gram_range(a, np.full(n, k)))
    kg = ps.graded_k(m, n)
    for name, a in ps.graded_inputs(m, n):
        ps.scale_columns(a, kg)
        seen.append(ps.log2_gram_range(a, kg))
    lo, hi = min(s[0] for s in seen), max(s[1] for s in seen)
    print("%d x %d: log2(m max|a_j|^2 2^(2 k_j)) from %.1f to %.1f" % (m, n, lo, hi))
    assert -1000.0 <= lo and hi <= 1000.0
    # the product of two columns' scales, the off-diagonal entries of G and the in-progress rows of R^-T (2^(k_i - k_j)), stays inside too
    assert 2 * (kg.max() - kg.min()) + 64 <= 2000


@pytest.mark.parametrize("m,n", ps.RANGE_SHAPES)
def test_out_of_range_exponents_do_leave_the_range(m, n):
    """section 3c in numpy's fp64.  k = 520: A^T A overflows.  k = 506: m 2^(2 k) reaches 2^1024 for m >= 4096 only -- at 4097 rows
    diagonal entries overflow, at 2063 rows (2063 2^1012 < 2^1024) A^T A stays finite within a factor 2 of the largest double and it
    is its trace that overflows.  k = -520: every entry of A^T A is subnormal, none zero.  k = -545: A^T A is all zero."""
    a = ps.gaussian(m, n)
    out = {}
    for k in ps.RANGE_K:
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            b = np.ldexp(a, k)
            out[k] = b.T @ b
    assert np.isinf(np.diag(out[520])).all()
    if m >= 4096:
        assert np.isinf(np.diag(out[506])).any()
    else:
        assert np.isfinite(out[506]).all() and out[506].max() > 2.0 ** 1023
        with np.errstate(over="ignore"):
            assert np.isinf(np.trace(out[506]))
    tiny = float(np.finfo(np.float64).tiny)
    assert np.all(out[-520] != 0.0) and np.all(np.abs(out[-520]) < tiny)
    assert np.all(out[-545] == 0.0)
    # and the inputs themselves are still exact scalings of A (the entries of A do not leave the range, only their products do)
    for k in ps.RANGE_K:
        ps.scale_uniform(a, k)


# ---- the reference meets the conditions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", ALL_SHAPES)
def test_householder_meets_the_bands_under_ext_metrics(m, n):
    a = ps.gaussian(m, n)
    q, r = np.linalg.qr(a)
    orth, res, cols = ps.ext_metrics(a, q, r)
    print("%d x %d Householder: ||QtQ-I||_F %.2e  residual %.2e  worst column %.2e" % (m, n, orth, res, cols.max()))
    orth_max, res_max = ps.bands(n, 1)                       # the tighter of the two bands
    assert orth <= orth_max / 10 and res <= res_max / 10 and cols.max() <= res_max / 10

"""Pure-numpy generators and measures for the scaling and dependent-column tests of the fp64 entries (tests/test_gpu_f64_scale.py):
exact power-of-two column scalings, graded exponent sets, matrices with exactly (and almost) dependent columns, the cases of every
section with their exponents, and the longdouble measures of a factorisation.  No GPU, no library, no torch:
tests/test_pass_refs_f64_scale.py checks all of it on the CPU.

Why powers of two: the fp64 ladder is products and sums (MFMA, FMA), v_rsq_f64 with one Newton step on pivots that scale by EVEN powers
of two, and verdicts taken on ratios of like-scaled quantities.  A -> A diag(2^k_j) multiplies every intermediate by an exact power of
two as long as nothing leaves the normal range, so an unshifted call returns the same bits of Q and R diag(2^k_j); the shift
s = shift_coef trace(G) follows a UNIFORM scaling only (tests/test_gpu_f64_scale.py states the two properties)."""
import functools

import numpy as np

from tests import pass_refs_f64 as p64

LD = p64.LD

# ---- the cases of tests/test_gpu_f64_scale.py (shapes, exponents), shared with the CPU check of their ranges -------------------------------
NARROW_SHAPES = ((4097, 64), (1029, 51), (100, 7), (65, 1))          # qr_f64, r_f64
WIDE_SHAPES = ((2063, 130), (4097, 200))                             # qr_f64_wide
DIST_SHAPES = ((4097, 64), (2063, 130))                              # tsqr_mi_qr_f64_dist_cb on one rank
UNIFORM_K = (-400, -1, 1, 401)                                       # section 3a
UNIFORM_INPUTS = ("gauss", "cond1e6", "cond1e12")                    # sweeps 1 (2 with reorth), 2, 103
GRADED_SPAN = 300                                                    # section 3b
GRADED_LADDER_ROWS = ("alone_max / 2", "2 alone_max", "max_scond / 4")   # pass_refs_f64.LADDER's rows on the CholeskyQR2 side
RANGE_SHAPES = ((4097, 64), (2063, 130))                             # section 3c
RANGE_K = (-545, -520, 506, 520)
DEPENDENT_SHAPES = ((4097, 64), (1029, 51), (2063, 130))             # section 3d
DEPENDENT_NAMES = ("a_copy_of_previous", "b_zero_column", "c_sum_of_two_rounded", "d_tail_copies_of_first")


def shape_seed(m, n, salt=0):
    return 1000003 * salt + 1009 * m + n


def _frozen(a):
    a.setflags(write=False)                                  # (shared between tests through the caches below: nobody changes them)
    return a


@functools.lru_cache(maxsize=None)
def gaussian(m, n):
    return _frozen(np.random.default_rng(shape_seed(m, n)).standard_normal((m, n)))


@functools.lru_cache(maxsize=None)
def cond_matrix(m, n, cond):
    """tests/test_gpu_f64.py's _cond_matrix: U diag(logspace(0, -log10 cond)) V^T"""
    rng = np.random.default_rng(shape_seed(m, n, int(round(np.log10(cond)))))
    u, _ = np.linalg.qr(rng.standard_normal((m, n)))
    v, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return _frozen((u * np.logspace(0.0, -np.log10(cond), n)) @ v.T)


def uniform_input(kind, m, n):
    if kind == "gauss":
        return gaussian(m, n)
    assert kind.startswith("cond"), kind
    return cond_matrix(m, n, float(kind[4:]))


@functools.lru_cache(maxsize=None)
def graded_inputs(m, n):
    """[(name, A)] of section 3b: Gaussian, and for n > 1 (S = 1 for one column) the ladder matrices on the CholeskyQR2 side"""
    out = [("gauss", gaussian(m, n))]
    if n > 1:
        for name, target, _, _ in p64.ladder_targets(m, n):
            if name in GRADED_LADDER_ROWS:
                out.append((name, _frozen(p64.ladder_matrix(m, n, target, n)[0])))
        assert len(out) == 1 + len(GRADED_LADDER_ROWS)
    return tuple(out)


def graded_k(m, n):
    """the exponents section 3b uses at this shape"""
    return graded_exponents(np.random.default_rng(shape_seed(m, n, 3)), n, GRADED_SPAN)


# ---- exact scalings ------------------------------------------------------------------------------------------------------------------------
def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def scale_columns(a, k):
    """A diag(2^k_j), k integers (one per column), and the proof that it is exact: scaling back returns A's bits"""
    k = np.asarray(k)
    assert k.shape == (a.shape[1],) and np.issubdtype(k.dtype, np.integer), (k.shape, k.dtype)
    k = k.astype(np.int32)
    with np.errstate(over="ignore", under="ignore"):         # (a scaling that leaves the range is reported by the assertion below)
        out = np.ldexp(a, k[None, :])
        back = np.ldexp(out, -k[None, :])
    assert np.array_equal(_bits(back), _bits(a)), "the scaling rounded: an entry left the normal range"
    return out


def scale_uniform(a, k):
    return scale_columns(a, np.full(a.shape[1], k, dtype=np.int64))


def graded_exponents(rng, n, span):
    """n integers in [-span, span] in random order: both extremes present (n >= 2), odd and even values mixed (n >= 3)"""
    assert n >= 1 and span >= 1
    k = rng.integers(-span, span + 1, size=n)
    if n == 1:
        k[0] = -span
    else:
        k[0], k[1] = -span, span
    if n >= 3:
        k[2] = span - 1                                      # the other parity, whatever the draw gave
    k = rng.permutation(k).astype(np.int64)
    assert k.min() >= -span and k.max() <= span
    assert n < 2 or (k.min() == -span and k.max() == span)
    assert n < 3 or len(set(np.abs(k) % 2)) == 2
    return k


def log2_gram_range(a, k):
    """(lowest, highest) over the columns of log2(m max_i |a_ij|^2 2^(2 k_j)): where the diagonal of the Gram matrix of A diag(2^k) lies,
    taken in logarithms so that nothing overflows here"""
    m = a.shape[0]
    amax = np.abs(a).max(axis=0)
    assert np.all(amax > 0.0)
    v = np.log2(float(m)) + 2.0 * np.log2(amax) + 2.0 * np.asarray(k, dtype=np.float64)
    return float(v.min()), float(v.max())


# ---- dependent columns ---------------------------------------------------------------------------------------------------------------------
def dependent_cases(rng, m, n):
    """[(name, A, j0)]: one Gaussian m x n matrix with, at column j0 = n // 2,
      a_copy_of_previous      column j0 an exact copy of column j0 - 1
      b_zero_column           column j0 exactly zero
      c_sum_of_two_rounded    column j0 = fl(column 0 + column 1): dependent to rounding only, cond about 1 / u
      d_tail_copies_of_first  columns j0 .. n - 1 all copies of column 0
    j0 is the number of leading independent columns.  n == 1: the unmodified matrix alone, j0 = 1."""
    base = rng.standard_normal((m, n))
    if n == 1:
        return [("unmodified", base, 1)]
    j0 = n // 2
    assert j0 >= 2, "case c needs columns 0 and 1 in front of column j0"
    out = []
    a = base.copy(); a[:, j0] = a[:, j0 - 1]; out.append((DEPENDENT_NAMES[0], a, j0))
    a = base.copy(); a[:, j0] = 0.0; out.append((DEPENDENT_NAMES[1], a, j0))
    a = base.copy(); a[:, j0] = a[:, 0] + a[:, 1]; out.append((DEPENDENT_NAMES[2], a, j0))
    a = base.copy(); a[:, j0:] = a[:, :1]; out.append((DEPENDENT_NAMES[3], a, j0))
    return out


@functools.lru_cache(maxsize=None)
def dependent_matrices(m, n):
    return tuple((name, _frozen(a), j0) for name, a, j0 in dependent_cases(np.random.default_rng(shape_seed(m, n, 7)), m, n))


# ---- measures ------------------------------------------------------------------------------------------------------------------------------
def _fro(x):
    return np.sqrt(np.sum(x * x))


def ext_metrics(a, q, r, lead=None):
    """In longdouble: (||Q^T Q - I||_F, ||A - Q R||_F / ||A||_F, the per-column residuals ||a_j - Q r_j|| / ||a_j|| of the non-zero
    columns).  lead: the first measure on Q[:, :lead] only.  The caller rescales first (ldexp), so every operand is of order 1."""
    p64.require_longdouble()
    al, ql, rl = np.asarray(a, LD), np.asarray(q, LD), np.asarray(r, LD)
    ql_lead = ql if lead is None else ql[:, :lead]
    e = ql_lead.T @ ql_lead - np.eye(ql_lead.shape[1], dtype=LD)
    d = al - ql @ rl
    cn = np.sqrt(np.sum(al * al, axis=0))
    dn = np.sqrt(np.sum(d * d, axis=0))
    live = cn > 0
    return float(_fro(e)), float(_fro(d) / _fro(al)), np.asarray(dn[live] / cn[live], np.float64)


def bands(n, reorth):
    """include/tsqr_mi.h: (||Q^T Q - I||_F, residual) of tsqr_mi_qr_f64 / _wide / _dist for cond(A) <= 1e12"""
    return (1e-12 if reorth else 1e-11) * max(1.0, n / 64.0), 1e-13

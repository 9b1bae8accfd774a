"""Pure-numpy references for the tests of the fp64 least-squares entry (tsqr_mi_lstsq_f64): exact data with an asserted bit budget and
the exact result of one pass D = (A Z)^T (B - A X) (lsq_f64_kernel, tsqr_f64.hip) in the layout its partials leave in, a numpy model of
that pass with the defects the tests must catch, a numpy model of the whole call, the longdouble Householder solve the entry's tests
measure against and the test matrices.  No GPU, no library: tests/test_pass_refs_f64_lsq.py checks it on the CPU.  Notation as in
tests/pass_refs_f64_r.py."""
import numpy as np

from tests import pass_refs_f64 as p64
from tests import pass_refs_f64_r as p64r
from tests import pass_refs_f64_scale as ps

U = p64.U
LD = p64.LD
NRHS_MAX = 16
np_of = p64r.np_of


# ---- layouts ---------------------------------------------------------------------------------------------------------------------------
def pad_x(x, n):
    """n x nrhs X -> the NP x 16 column-major block (ld NP) the passes read, zero padded"""
    np_ = np_of(n)
    xp = np.zeros((np_, NRHS_MAX))
    xp[:n, :x.shape[1]] = x
    return np.ascontiguousarray(xp.T).reshape(-1)


def unpad_x(v, n):
    np_ = np_of(n)
    return np.asarray(v)[:np_ * NRHS_MAX].reshape(NRHS_MAX, np_).T.copy()


def _d_index(n):
    """(row, column) of D behind every element of the summed partial: tile t, register r, lane (li, lq) at (4 t + r) 64 + 16 lq + li
    holds D[16 t + lq + 4 r][li]"""
    e = np.arange(np_of(n) // 16 * 256)
    t, r, lane = e // 256, (e // 64) % 4, e % 64
    return 16 * t + (lane >> 4) + 4 * r, lane & 15


def pack_d(d, n):
    """n x nrhs D -> the NT tiles of 256 doubles of the summed partials (rows >= n and right-hand sides >= nrhs are zeros)"""
    dp = np.zeros((np_of(n), NRHS_MAX))
    dp[:d.shape[0], :d.shape[1]] = d
    i, j = _d_index(n)
    return dp[i, j]


def unpack_d(v, n):
    """the summed partials -> NP x 16"""
    dp = np.zeros((np_of(n), NRHS_MAX))
    i, j = _d_index(n)
    dp[i, j] = np.asarray(v)[:i.size]
    return dp


# ---- exact data -------------------------------------------------------------------------------------------------------------------------
AMAX = 3


def exact_case(rng, m, n, nrhs):
    """(A, Z, X, B): A, X, B integers in [-3, 3], Z unit upper triangular with entries in {-1, 0, 1}.  |A Z| <= 3 n <= 192 and
    |B - A X| <= 3 + 9 n <= 579 are integers, and every partial sum of D = (A Z)^T (B - A X), in any order and fused or not, is an
    integer of magnitude <= m 192 579: exact in fp64 while that is below 2^53 (asserted on the data at hand)."""
    assert n <= 64 and nrhs <= NRHS_MAX
    a = rng.integers(-AMAX, AMAX + 1, size=(m, n)).astype(np.float64)
    z = np.triu(rng.integers(-1, 2, size=(n, n)), 1).astype(np.float64) + np.eye(n)
    x = rng.integers(-AMAX, AMAX + 1, size=(n, nrhs)).astype(np.float64)
    b = rng.integers(-AMAX, AMAX + 1, size=(m, nrhs)).astype(np.float64)
    q, res = a @ z, b - a @ x
    assert np.abs(q).max() <= AMAX * 64 and np.abs(res).max() <= AMAX + AMAX * AMAX * 64
    assert m * float(np.abs(q).max()) * max(float(np.abs(res).max()), 1.0) < 2.0 ** 53, "a partial sum could leave the exact range"
    return a, z, x, b


def d_exact(a, z, x, b):
    """(A Z)^T (B - A X) of exact_case data: plain fp64 products are exact (budget asserted there); x None: X = 0"""
    res = b if x is None else b - a @ x
    return (a @ z).T @ res


# ---- numpy model of one pass, with the defects the tests must catch ----------------------------------------------------------------------
def model_pass(a, z, x, b, defect=None):
    """fp64 model of lsq_f64_kernel + reduction -> the summed partials (pack_d): 16-row tiles of Q~ = A Z and of the residual, formed and
    consumed one after the other.  defects: 'x_sign' forms B + A X; 'drop_tail_row' leaves out the last row of A and B; 'swap_ti' stores
    the first two 16-row tiles of D in each other's place (n > 16)."""
    m, n = a.shape
    rows = m - 1 if defect == "drop_tail_row" else m
    d = np.zeros((n, b.shape[1]))
    for r0 in range(0, rows, 16):
        at, bt = a[r0:min(r0 + 16, rows)], b[r0:min(r0 + 16, rows)]
        res = bt + at @ x if defect == "x_sign" else bt - at @ x
        d += (at @ z).T @ res
    v = pack_d(d, n)
    if defect == "swap_ti":
        assert n > 16, "one tile cannot be swapped"
        v[:256], v[256:512] = v[256:512].copy(), v[:256].copy()
    return v


# ---- numpy model of the whole call ------------------------------------------------------------------------------------------------------
def householder_r(a):
    """numpy's Householder R with a positive diagonal"""
    n = a.shape[1]
    r = np.linalg.qr(a, mode="r").reshape(n, n)
    return np.where(np.diag(r) < 0, -1.0, 1.0)[:, None] * r


def explicit_inverse(r):
    """Z = inverse(R) in fp64 by back substitution, column by column (upper triangular)"""
    n = r.shape[0]
    z = np.zeros((n, n))
    for j in range(n):
        z[j, j] = 1.0 / r[j, j]
        for i in range(j - 1, -1, -1):
            z[i, j] = -(r[i, i + 1:j + 1] @ z[i + 1:j + 1, j]) / r[i, i]
    return z


def stagnation_step(x, dx, d, state, p):
    """lsq_update_f64_kernel's stagnation rule for pass p (0-based) on fp64 arrays: right-hand side j takes its update dx[:, j] unless
    p >= 2 and max_k |D[k][j]| is above half of the pass before (or the column has stopped already); a column that is refused stops for
    good.  state: max |D| per column of the pass before, -1 once stopped (None before the first pass).  Returns (X, state)."""
    with np.errstate(invalid="ignore"):
        dm = np.fmax.reduce(np.abs(d), axis=0, initial=0.0)                  # (fmax: a NaN is skipped, as on the device)
        apply = np.ones(d.shape[1], bool) if p < 2 else (state >= 0.0) & ~(dm > 0.5 * state)
    x = dx if x is None else np.where(apply[None, :], x + dx, x)
    return x, np.where(apply, dm, -1.0)


def model_lstsq(a, b, refine=1, defect=None):
    """fp64 model of the algorithm of tsqr_mi_lstsq_f64, tile-free: R from Householder QR, an explicit Z = inverse(R), Q~ = A Z,
    X_0 = Z (Q~^T B), then `refine` times X <- X + Z (Q~^T (B - A X)), from the second correction on under the stagnation rule
    (stagnation_step).  Returns (X, R).  defect 'x_sign': the correction is formed from B + A X (the model's own yardstick test);
    'no_stagnation_rule': every correction is applied."""
    r = householder_r(a)
    z = explicit_inverse(r)
    q = a @ z
    d = q.T @ b
    x, state = stagnation_step(None, z @ d, d, None, 0)
    for p in range(1, refine + 1):
        res = b + a @ x if defect == "x_sign" else b - a @ x
        d = q.T @ res
        x, state = stagnation_step(x, z @ d, d, state, 0 if defect == "no_stagnation_rule" else p)
    return x, r


# ---- the reference solve and the measures ------------------------------------------------------------------------------------------------
def lstsq_ld(a, b):
    """argmin ||A X - B||_F by Householder QR in longdouble (reflectors applied to [A B], back substitution)"""
    p64.require_longdouble()
    m, n = a.shape
    w = np.concatenate([a, b], axis=1).astype(LD)
    for j in range(n):
        v = w[j:, j].copy()
        alpha = np.sqrt(np.sum(v * v))
        if alpha == 0:
            continue
        if v[0] > 0:
            alpha = -alpha
        v[0] -= alpha
        vv = np.sum(v * v)
        if vv == 0:
            continue
        w[j:, j:] -= np.outer(v, (2 / vv) * (v @ w[j:, j:]))
    r, c = w[:n, :n], w[:n, n:]
    x = np.zeros((n, b.shape[1]), LD)
    for i in range(n - 1, -1, -1):
        x[i] = (c[i] - r[i, i + 1:] @ x[i + 1:]) / r[i, i]
    return x


def rel_err(x, x_ref):
    """||X - X_ref||_F / ||X_ref||_F in longdouble"""
    e = np.asarray(x, LD) - x_ref
    return float(np.sqrt(np.sum(e * e)) / np.sqrt(np.sum(x_ref * x_ref)))


def normal_residual(a, b, x):
    """||A^T (B - A X)||_F / (||A||_F ||B||_F) in longdouble"""
    al, bl = a.astype(LD), b.astype(LD)
    g = al.T @ (bl - al @ np.asarray(x, LD))
    return float(np.sqrt(np.sum(g * g)) / (np.sqrt(np.sum(al * al)) * np.sqrt(np.sum(bl * bl))))


# ---- the inputs of the entry's accuracy test (tests/test_gpu_f64_lstsq.py; the CPU test runs model_lstsq on the same) --------------------
SHAPES = ((1, 1, 1), (65, 64, 16), (1000, 7, 3), (9211, 51, 5), (4096, 64, 16))        # (m, n, nrhs), Gaussian A
CONDS = (1.0, 1e4, 1e6)                                                                    # at 4096 x 64, nrhs 16
RUNG_SHAPES = ((777, 33, 16), (300, 17, 3), (1029, 51, 5))     # NP != n, NT = 3, 2, 4: both conditioned rungs of the ladder behind f64r_zmul
RUNG_CONDS = (1e4, 1e6)
RHS_KINDS = ("consistent", "gaussian")
FLOOR_COEF = 4.0                                           # the absolute floor of the assertion: 4 n u ("a few n u")


def accuracy_cases():
    """(name, m, n, nrhs, cond or None, rhs kind) of every accuracy case"""
    out = []
    for m, n, nrhs in SHAPES:
        for kind in RHS_KINDS:
            out.append(("gauss_%dx%d_%s" % (m, n, kind), m, n, nrhs, None, kind))
    for cond in CONDS:
        for kind in RHS_KINDS:
            out.append(("cond%.0e_4096x64_%s" % (cond, kind), 4096, 64, 16, cond, kind))
    return out + rung_cases()


def rung_cases():
    """the cases at RUNG_SHAPES: cond 1e4 and 1e6 with a column tail (n = 16 k + 1, 51) and a ragged last row tile"""
    return [("cond%.0e_%dx%d_%s" % (cond, m, n, kind), m, n, nrhs, cond, kind)
            for m, n, nrhs in RUNG_SHAPES for cond in RUNG_CONDS for kind in RHS_KINDS]


def accuracy_input(m, n, nrhs, cond, kind):
    """(A, B): A Gaussian (cond None) or pass_refs_f64_r.cond_matrix; B = A X* with Gaussian X* ('consistent': a residual of rounding
    size) or Gaussian ('gaussian': a residual as large as B)"""
    seed = 7 * m + n + (0 if cond is None else int(np.log10(cond)) + 1)
    a = np.random.default_rng(seed).standard_normal((m, n)) if cond is None else p64r.cond_matrix(m, n, cond, seed)
    rng = np.random.default_rng(seed + 100003)
    b = a @ rng.standard_normal((n, nrhs)) if kind == "consistent" else rng.standard_normal((m, nrhs))
    return a, b


def floor_of(n):
    return FLOOR_COEF * n * U


# ---- the scaling, range and dependent-column tests of the entry (tests/test_gpu_f64_lstsq_scale.py) ---------------------------------------
# Generators and exact scalers: tests/pass_refs_f64_scale.py.  What scales how (the code is products, FMAs and MFMA accumulates behind a
# ladder that is itself covariant): A -> A diag(2^k_c), B -> B diag(2^j_c) gives Z' = diag(2^-k_c) Z, (A Z)' = A Z, residual' and
# D' = D diag(2^j_c), X' = diag(2^-k_c) X diag(2^j_c), R' = R diag(2^k_c) -- exactly, while nothing leaves the normal range.
SCALE_SHAPES = ((4097, 64, 16), (1029, 51, 5), (777, 33, 16), (300, 17, 3), (100, 7, 1), (65, 1, 1))     # NT 4, 4, 3, 2, 1, 1
SCALE_K = ps.UNIFORM_K                                     # A -> 2^k A
SCALE_J = (-400, 0, 401)                                   # B -> 2^j B
SCALE_REFINES = (0, 1, 2)
B_SPAN = 400                                               # B -> B diag(2^j_c), j_c in [-B_SPAN, B_SPAN]
RANGE_LOG2 = 1000.0                                        # every intermediate of a covariance case inside [2^-1000, 2^1000]
# The documented range of B (include/tsqr_mi.h): a non-zero column b of B is in contract when
#     2^B_LOW_LOG2 max(1, ||A||_F)  <=  ||b||_2  <=  2^B_HIGH_LOG2 min(1, sigma_min(A)).
# Above: the largest intermediates are |D| <= ||q|| ||b|| and |X| <= ||b|| / sigma_min (a row of A X is again of B's size).  Below: on
# a consistent system the correction passes carry a residual of u ||b|| / sqrt(m) per entry, D of u ||b|| and an update of
# u ||b|| / ||A||; with (m + n) cond(A) <= 2^43 roundings at the subnormal spacing 2^-1074 they stay below u of the result while
# ||b|| >= 2^(-1074 + 53 + 43 + margin) max(1, ||A||).
B_LOW_LOG2, B_HIGH_LOG2 = -960, 1000
RANGE_SHAPES = ((4097, 64, 5), (1029, 51, 5))              # Gaussian A; one column (RANGE_COLUMN) of B scaled by 2^j
RANGE_COLUMN = 2
RANGE_J_INSIDE = (-950, 985)                               # just inside each end (shown from the data on the CPU)
RANGE_J_BEYOND = (-1000, 1012)                             # beyond each end; the entries of B themselves stay normal and finite
DEPENDENT_SHAPES = ((4097, 64, 16), (1029, 51, 5))


def _frozen(a):
    a.setflags(write=False)
    return a


def scale_rhs(a, nrhs, seed):
    """m x nrhs right-hand sides for A: even columns consistent (A x*, x* Gaussian: a residual of rounding size, so that the correction
    passes carry u ||b||), odd columns Gaussian (a residual as large as b)"""
    rng = np.random.default_rng(seed)
    b = rng.standard_normal((a.shape[0], nrhs))
    xs = rng.standard_normal((a.shape[1], nrhs))
    b[:, 0::2] = (a @ xs)[:, 0::2]
    return b


_scale_cache = {}


def scale_case(m, n, nrhs, name):
    """(A, B) of a covariance case, shared and read-only: A = pass_refs_f64_scale.uniform_input(name) ('gauss', 'cond1e6', 'cond1e12') or
    the ladder matrix of that name (graded_inputs); B = scale_rhs on it"""
    key = (m, n, nrhs, name)
    if key not in _scale_cache:
        graded = dict(ps.graded_inputs(m, n))
        a = graded[name] if name in graded else ps.uniform_input(name, m, n)
        salt = 11 + sorted(set(ps.UNIFORM_INPUTS) | set(ps.GRADED_LADDER_ROWS) | {"gauss"}).index(name)
        _scale_cache[key] = (a, _frozen(scale_rhs(a, nrhs, ps.shape_seed(m, n, salt))))
    return _scale_cache[key]


def rhs_groups(nrhs):
    """the column sets the accuracy rule is applied to: the consistent and the Gaussian columns of scale_rhs, each on its own"""
    return [("consistent", np.arange(0, nrhs, 2))] + ([("gaussian", np.arange(1, nrhs, 2))] if nrhs > 1 else [])


def b_exponents(m, n, nrhs):
    """j_c of the per-column scaling of B: integers in [-B_SPAN, B_SPAN], both extremes present from two columns on"""
    return ps.graded_exponents(np.random.default_rng(ps.shape_seed(m, n, 5)), nrhs, B_SPAN)


def uniform_pairs():
    return [(k, j) for k in SCALE_K for j in SCALE_J]


def scale_x(x, k, j):
    """diag(2^-k_c) X diag(2^j_c), exact (asserted by scaling back); k, j: an integer or one integer per row / column"""
    x = np.asarray(x, np.float64)
    e = (-np.broadcast_to(np.asarray(k), (x.shape[0],))[:, None] + np.broadcast_to(np.asarray(j), (x.shape[1],))[None, :]).astype(np.int32)
    with np.errstate(over="ignore", under="ignore"):
        out = np.ldexp(x, e)
        back = np.ldexp(out, -e)
    assert np.array_equal(back.view(np.int64), np.ascontiguousarray(x).view(np.int64)), "the scaling rounded: an entry left the normal range"
    return out


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.int64), y.view(np.int64))


def model_trace(a, b, refine, round_d=None):
    """model_lstsq with its intermediates: (X, R, Z, [residual of every pass], [D of every pass], [X after every pass]).  round_d: the
    seeded defect of the covariance check -- D is rounded to that type (np.float32: a narrowed accumulate) before it is used."""
    r = householder_r(a)
    z = explicit_inverse(r)
    q = a @ z
    res_all, d_all, x_all = [], [], []
    x = None
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        state = None
        for p in range(refine + 1):
            res = b if x is None else b - a @ x
            d = q.T @ res
            if round_d is not None:
                d = d.astype(round_d).astype(np.float64)
            x, state = stagnation_step(x, z @ d, d, state, p)
            res_all.append(res); d_all.append(d); x_all.append(x)
    return x, r, z, res_all, d_all, x_all


def log2_span(x, row_exp=0, col_exp=0):
    """(lowest, highest) log2 of the non-zero magnitudes of diag(2^row_exp) x diag(2^col_exp), taken in longdouble (exponent range
    2^+-16383: nothing under test can leave it, so an fp64 underflow cannot hide here)"""
    p64.require_longdouble()
    x = np.asarray(x, LD)
    e = (np.broadcast_to(np.asarray(row_exp), (x.shape[0],))[:, None] + np.broadcast_to(np.asarray(col_exp), (x.shape[1],))[None, :])
    v = np.abs(np.ldexp(x, e.astype(np.int32)))
    v = v[v != 0]
    if v.size == 0:
        return 0.0, 0.0
    return float(np.log2(v.min())), float(np.log2(v.max()))


def scaled_spans(trace, k, j):
    """{name: (lowest, highest) log2} of Z, the residuals, D and X of every pass of the call on A diag(2^k) and B diag(2^j), from the
    trace of the unscaled model"""
    _, _, z, res_all, d_all, x_all = trace
    out = {"Z": log2_span(z, row_exp=-np.asarray(k))}
    for p, (res, d, x) in enumerate(zip(res_all, d_all, x_all)):
        out["residual%d" % p] = log2_span(res, col_exp=j)
        out["D%d" % p] = log2_span(d, col_exp=j)
        out["X%d" % p] = log2_span(x, row_exp=-np.asarray(k), col_exp=j)
    return out


def column_err(x, ref, cols):
    """rel_err on a set of columns"""
    return rel_err(np.asarray(x)[:, cols], ref[:, cols])


def b_range_log2(a):
    """(lowest, highest) log2 of the 2-norm of a non-zero column of B that include/tsqr_mi.h puts in contract for this A"""
    sv = np.linalg.svd(a, compute_uv=False)
    fro = float(np.sqrt(np.sum(sv * sv)))
    return B_LOW_LOG2 + np.log2(max(1.0, fro)), B_HIGH_LOG2 + np.log2(min(1.0, float(sv[-1])))


def range_case(m, n, nrhs, kind):
    """(A, B) of the range test: Gaussian A, B consistent or Gaussian (accuracy_input's kinds)"""
    key = ("range", m, n, nrhs, kind)
    if key not in _scale_cache:
        a = ps.gaussian(m, n)
        rng = np.random.default_rng(ps.shape_seed(m, n, 17))
        b = a @ rng.standard_normal((n, nrhs)) if kind == "consistent" else rng.standard_normal((m, nrhs))
        _scale_cache[key] = (a, _frozen(b))
    return _scale_cache[key]


def scale_one_column(b, col, j):
    k = np.zeros(b.shape[1], dtype=np.int64)
    k[col] = j
    return ps.scale_columns(b, k)


def independent_columns(name, n, j0):
    """the columns that remain when the dependent ones of pass_refs_f64_scale.dependent_cases are pivoted out"""
    return np.arange(j0) if name.startswith("d_") else np.array([c for c in range(n) if c != j0])


def min_residual_ld(a, b, keep):
    """min_X ||B - A X||_F in longdouble over the independent columns `keep` of A (the dependent ones add nothing to the range)"""
    al, bl = a[:, keep].astype(LD), b.astype(LD)
    e = bl - al @ lstsq_ld(a[:, keep], b)
    return float(np.sqrt(np.sum(e * e)))


def residual_ld(a, b, x):
    e = b.astype(LD) - a.astype(LD) @ np.asarray(x, LD)
    return float(np.sqrt(np.sum(e * e)))

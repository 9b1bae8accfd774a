"""Pure-numpy references for the tests of the fp64 least-squares entry (tsqr_mi_lstsq_f64): exact data with an asserted bit budget and
the exact result of one pass D = (A Z)^T (B - A X) (lsq_f64_kernel, tsqr_f64.hip) in the layout its partials leave in, a numpy model of
that pass with the defects the tests must catch, a numpy model of the whole call, the longdouble Householder solve the entry's tests
measure against and the test matrices.  No GPU, no library: tests/test_pass_refs_f64_lsq.py checks it on the CPU.  Notation as in
tests/pass_refs_f64_r.py."""
import numpy as np

from tests import pass_refs_f64 as p64
from tests import pass_refs_f64_r as p64r

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


def model_lstsq(a, b, refine=1, defect=None):
    """fp64 model of the algorithm of tsqr_mi_lstsq_f64, tile-free: R from Householder QR, an explicit Z = inverse(R), Q~ = A Z,
    X_0 = Z (Q~^T B), then `refine` times X <- X + Z (Q~^T (B - A X)).  Returns (X, R).  defect 'x_sign': the correction is formed from
    B + A X (the model's own yardstick test)."""
    r = householder_r(a)
    z = explicit_inverse(r)
    q = a @ z
    x = z @ (q.T @ b)
    for _ in range(refine):
        res = b + a @ x if defect == "x_sign" else b - a @ x
        x = x + z @ (q.T @ res)
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
    return out


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

"""Pure-numpy references for the passes of a rank-aware fp64 least-squares solve: the rank rule and Zeff of
lsq_rank_f64_kernel, the dense-Z pass and update (lsq_dense_f64_kernel, lsq_update_f64_kernel<ZDENSE>, tsqr_f64.hip) with the
defects the tests must catch, a numpy model of the whole solve, its test cases with their preconditions and the assertions the model
is held to (tests/test_pass_refs_f64_lsq_rank.py, CPU) and an entry built on these passes will be held to.  Built on
tests/pass_refs_f64_lsq.py and householder_qrcp of tests/pass_refs_f64_qrcp.py."""
import numpy as np

from tests import pass_refs_f64_lsq as pl
from tests import pass_refs_f64_qrcp as pq

U = pl.U
LD = pl.LD
np_of = pl.np_of


# ---- the rank rule and Zeff --------------------------------------------------------------------------------------------------------------
def rank_of(r, rcond):
    """the number of j with R_jj > rcond R_00"""
    d = np.diag(np.asarray(r, np.float64))
    return int(np.sum(d > rcond * d[0]))


def back_inverse(r11):
    """inverse(R11) by column-oriented back substitution in lsq_rank_f64_kernel's order: column j starts from e_j; step l = j .. 0 forms
    z_l = w_l / R_ll, then w_i <- w_i - R_il z_l for i < l (one rounding per term stands in for the fused multiply-add)"""
    k = r11.shape[0]
    z = np.zeros((k, k))
    for j in range(k):
        w = np.zeros(k)
        w[j] = 1.0
        for l in range(j, -1, -1):
            z[l, j] = w[l] / r11[l, l]
            w[:l] -= r11[:l, l] * z[l, j]
    return z


def zeff_of(r, p, k, defect=None):
    """n x n Zeff: Zeff[p[i]][j] = inverse(R[:k, :k])[i][j] for i <= j < k, zero elsewhere (the device pads it to NP x NP with zeros).
    defect 'no_perm': the rows are not permuted."""
    n = r.shape[0]
    z = np.zeros((n, n))
    rows = np.arange(k) if defect == "no_perm" else np.asarray(p)[:k]
    z[rows, :k] = back_inverse(np.asarray(r, np.float64)[:k, :k])
    return z


def pad_z(z):
    """n x n dense Z -> NP x NP column-major (ld NP), zero padded, flat"""
    n = z.shape[0]
    zp = np.zeros((np_of(n), np_of(n)))
    zp[:n, :n] = z
    return np.ascontiguousarray(zp.T).reshape(-1)


def unpad_z(v, n):
    np_ = np_of(n)
    return np.asarray(v)[:np_ * np_].reshape(np_, np_).T.copy()


def structure_ok(zp, p, k, n):
    """exact zeros of the NP x NP Zeff outside the permuted triangle (entries (p[i], j) with i <= j < k) and in the padding"""
    mask = np.zeros(zp.shape, bool)
    for i in range(k):
        mask[p[i], i:k] = True
    return not zp[~mask].any()


def inverse_residual(r, zp, p, k):
    """||R11 (P1^T Zeff)[:k, :k] - I||_F in longdouble"""
    r11 = np.asarray(r, LD)[:k, :k]
    z11 = np.asarray(zp, LD)[np.asarray(p)[:k], :k]
    e = r11 @ z11 - np.eye(k, dtype=LD)
    return float(np.sqrt(np.sum(e * e)))


def inverse_allowance(r, k):
    """4 x the same figure of scipy.linalg.solve_triangular on the same R11, or k 2^-53 if larger"""
    import scipy.linalg
    r11 = np.asarray(r, np.float64)[:k, :k]
    zs = scipy.linalg.solve_triangular(r11, np.eye(k))
    e = r11.astype(LD) @ zs.astype(LD) - np.eye(k, dtype=LD)
    return max(4.0 * float(np.sqrt(np.sum(e * e))), k * U)


# ---- exact data of the dense pass -----------------------------------------------------------------------------------------------------------
def exact_dense_case(rng, m, n, nrhs, upper=False):
    """(A, Z, X, B): pass_refs_f64_lsq.exact_case with a DENSE Z in {-1, 0, 1} (upper: upper triangular, not unit).  |A Z| <= 3 n <= 192,
    |B - A X| <= 3 + 9 n <= 579; every partial sum of D is an integer below 2^53 (asserted on the data at hand)."""
    assert n <= 64 and nrhs <= pl.NRHS_MAX
    a = rng.integers(-pl.AMAX, pl.AMAX + 1, size=(m, n)).astype(np.float64)
    z = rng.integers(-1, 2, size=(n, n)).astype(np.float64)
    if upper:
        z = np.triu(z)
    x = rng.integers(-pl.AMAX, pl.AMAX + 1, size=(n, nrhs)).astype(np.float64)
    b = rng.integers(-pl.AMAX, pl.AMAX + 1, size=(m, nrhs)).astype(np.float64)
    q, res = a @ z, b - a @ x
    assert np.abs(q).max() <= pl.AMAX * 64 and np.abs(res).max() <= pl.AMAX + pl.AMAX * pl.AMAX * 64
    assert m * max(float(np.abs(q).max()), 1.0) * max(float(np.abs(res).max()), 1.0) < 2.0 ** 53, "a partial sum could leave the exact range"
    return a, z, x, b


def tri_skip(z):
    """Z as the triangular form of the pass sees it: output tile jt (columns 16 jt .. 16 jt + 15) takes rows k < 16 (jt + 1) only"""
    n = z.shape[0]
    k, j = np.arange(n)[:, None], np.arange(n)[None, :]
    return np.where(k < 16 * (j // 16 + 1), z, 0.0)


def model_dense_pass(a, z, x, b, defect=None):
    """fp64 model of the dense pass + reduction -> the summed partials (pack_d).  defect 'tri_skip': the triangular form's k-block skip
    is left on"""
    zz = tri_skip(z) if defect == "tri_skip" else z
    return pl.model_pass(a, zz, np.zeros((a.shape[1], b.shape[1])) if x is None else x, b)


# ---- numpy model of the whole call ------------------------------------------------------------------------------------------------------
def model_lstsq_rank(a, b, rcond, refine=1, defect=None, trace=None, r0=None):
    """fp64 model of the rank-aware solve, tile-free: R0 from Householder QR, householder_qrcp in fp64 (the kernel's conventions), the
    rank rule, Zeff, then refine + 1 passes X <- X + Zeff (A Zeff)^T (B - A X) under pass_refs_f64_lsq.stagnation_step.
    Returns (X, R, p, rank).  defects: 'no_perm' (Zeff without the permutation), 'rank_plus' / 'rank_minus' (rank off by one),
    'dropped_row' (the first dropped row of X is left at a rounding-size non-zero; nothing at full rank), 'tri_skip' (the dense pass
    keeps the triangular skip).  trace: a list that receives max |D| of every pass."""
    n = a.shape[1]
    r0 = pl.householder_r(a) if r0 is None else r0          # (r0: another R0: tools/lstsq_rank_contraction.py)
    r, _, p = pq.householder_qrcp(r0, dtype=np.float64)
    k = rank_of(r, rcond)
    if defect == "rank_plus":
        k = min(k + 1, n) if k < n else k - 1
    elif defect == "rank_minus":
        k = k - 1 if k > 1 else k + 1
    z = zeff_of(r, p, k, defect)
    zq = tri_skip(z) if defect == "tri_skip" else z
    q = a @ zq
    x, state = None, None
    for t in range(refine + 1):
        d = q.T @ (b if x is None else b - a @ x)
        if trace is not None:
            trace.append(float(np.abs(d).max()))
        x, state = pl.stagnation_step(x, z @ d, d, state, t)
    if defect == "dropped_row" and k < n:
        x = x.copy()
        x[p[k]] += 2.0 ** -60
    return x, r, p, k


# ---- the cases of the end-to-end test ----------------------------------------------------------------------------------------------------
# (name, m, n, nrhs, rcond or None = the default max(m, n) eps, expected rank, row-major A, row-major B, reorth)
CASES = (
    ("copied_4096x16", 4096, 16, 5, 1e-8, 15, 0, 0, 0),
    ("rank32_1029x51", 1029, 51, 5, 1e-6, 32, 1, 0, 1),
    ("rank1_777x33", 777, 33, 16, 1e-8, 1, 0, 1, 0),
    ("rank40_4097x64", 4097, 64, 16, 1e-7, 40, 1, 1, 0),
    ("full_300x17", 300, 17, 1, None, 17, 0, 0, 1),
    ("tail3_100x7", 100, 7, 5, 1e-8, 4, 1, 1, 1),
    ("one_65x1", 65, 1, 16, None, 1, 0, 1, 0),
)
# (n = 1 takes 16 right-hand sides, not one: the sensitivity of a least-squares solution to rounding is u / cos(b, range A) per column,
# and with one Gaussian column both errors of the comparison are single numbers -- LAPACK's can land a factor 5 under that figure by
# chance.  Over 16 columns the Frobenius ratio is an average.  nrhs = 1 is covered at 300 x 17.)
RHS_KINDS = ("gaussian", "consistent")


def rcond_of(rcond, m, n):
    return max(m, n) * 2.0 ** -52 if rcond is None else rcond


_cache = {}


def case_matrix(name):
    """A of a case, shared and read-only"""
    if name in _cache:
        return _cache[name]
    _, m, n = next(c[:3] for c in CASES if c[0] == name)
    rng = np.random.default_rng(sum(ord(c) for c in name))
    g = rng.standard_normal
    if name.startswith("copied"):
        a = g((m, n))
        a[:, 11] = a[:, 4]
    elif name.startswith("rank32"):
        a = g((m, 32)) @ g((32, n)) + 1e-10 * g((m, n))
    elif name.startswith("rank1_"):
        a = g((m, 1)) @ g((1, n))
    elif name.startswith("rank40"):
        # 40 singular values 1 .. 1e-4 plus a Gaussian noise matrix of Frobenius norm 1e-11.  (Entries of 1e-11 each would put the
        # trailing pivots at 6e-9 of R_00, above the 1e-3 rcond = 1e-10 that the precondition asks for.)
        u, _ = np.linalg.qr(g((m, 40)))
        v, _ = np.linalg.qr(g((n, n)))
        e = g((m, n))
        a = (u * np.logspace(0, -4, 40)) @ v[:40] + 1e-11 * e / np.linalg.norm(e)
    elif name.startswith("tail3"):
        a = g((m, 4))
        a = np.concatenate([a, a[:, [3, 3, 3]]], axis=1)
    else:
        a = g((m, n))
    _cache[name] = pl._frozen(np.ascontiguousarray(a))
    return _cache[name]


def case_rhs(name, kind):
    key = (name, kind)
    if key not in _cache:
        a = case_matrix(name)
        nrhs = next(c[3] for c in CASES if c[0] == name)
        rng = np.random.default_rng(sum(ord(c) for c in name) + 977)
        b = rng.standard_normal((a.shape[0], nrhs)) if kind == "gaussian" else a @ rng.standard_normal((a.shape[1], nrhs))
        _cache[key] = pl._frozen(b)
    return _cache[key]


def precondition(name):
    """asserts that scipy.linalg.qr(pivoting=True) of A has |R_jj| / |R_00| >= 1e3 rcond for j < k_expected and <= 1e-3 rcond beyond:
    no case can pass by landing on the threshold.  Returns (lowest leading ratio, highest trailing ratio)."""
    import scipy.linalg
    key = ("pre", name)
    if key not in _cache:
        _, m, n, _, rcond, k = next(c[:6] for c in CASES if c[0] == name)
        rc = rcond_of(rcond, m, n)
        d = np.abs(np.diag(scipy.linalg.qr(case_matrix(name), mode="r", pivoting=True)[0][:n, :n]))
        lead, trail = float((d[:k] / d[0]).min()), float((d[k:] / d[0]).max()) if k < n else 0.0
        assert lead >= 1e3 * rc and trail <= 1e-3 * rc, (name, lead, trail, rc)
        _cache[key] = (lead, trail)
    return _cache[key]


def yardstick(name, kind, p, k):
    """(X*, LAPACK's error) on the retained columns: X* = lstsq_ld(A[:, p[:k]], B), and rel_err of numpy.linalg.lstsq on the same
    sub-matrix against it; shared among the tests of one (case, kind, p, k)"""
    key = ("yard", name, kind, tuple(int(i) for i in p[:k]))
    if key not in _cache:
        a, b = case_matrix(name), case_rhs(name, kind)
        sub = a[:, np.asarray(p)[:k]]
        ref = pl.lstsq_ld(sub, b)
        _cache[key] = (ref, pl.rel_err(np.linalg.lstsq(sub, b, rcond=None)[0], ref))
    return _cache[key]


def figures(name, kind, x, p, k):
    """{err, lapack, bound, zero_rows} of a result of a case"""
    n = case_matrix(name).shape[1]
    p = np.asarray(p)
    ref, lap = yardstick(name, kind, p, k)
    x = np.asarray(x, np.float64).reshape(n, -1)
    return {"err": pl.rel_err(x[p[:k]], ref), "lapack": lap, "bound": max(2.0 * lap, pl.floor_of(n)),
            "zero_rows": not x[p[k:]].any()}


def check(name, kind, x, p, k):
    """the assertions of a refine = 1 result: the rank is the expected one, p is a permutation, rows p[k:] of X are exact zeros,
    rel_err(X[p[:k]], X*) <= max(2 x LAPACK's, floor_of(n)).  Returns figures()."""
    _, m, n, _, _, k_expected = next(c[:6] for c in CASES if c[0] == name)
    precondition(name)
    assert k == k_expected, (name, "rank", k, k_expected)
    assert sorted(int(i) for i in p) == list(range(n)), (name, "jpvt is no permutation")
    f = figures(name, kind, x, p, k)
    assert f["zero_rows"], (name, kind, "a dropped row of X is not zero")
    assert f["err"] <= f["bound"], (name, kind, f)
    return f

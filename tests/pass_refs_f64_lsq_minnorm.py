"""Pure-numpy references for the minimum-norm form of the rank-aware fp64 least-squares entry (tsqr_mi_lstsq_minnorm_f64;
lsq_zg_f64_kernel and lsq_minnorm_f64_kernel, lsq_rank_f64.hip): Zg, a model of the update factor Zmn = P pinv(S) in
the kernel's order of operations with the defects the tests must catch, a model of the whole solve, an extended-precision minimum-norm
reference, LAPACK's yardstick on the same projected problem, the assertions a result is held to, and the data and measures of the
kernel's GPU test.  Built on tests/pass_refs_f64_lsq_rank.py and tests/pass_refs_f64_lsq_rank_step.py, whose cases, right-hand sides and
precondition() are used as they are.  No GPU, no library: tests/test_pass_refs_f64_lsq_minnorm.py checks it on the CPU."""
import numpy as np

from tests import pass_refs_f64_lsq as pl
from tests import pass_refs_f64_lsq_rank as pk
from tests import pass_refs_f64_lsq_rank_step as ps
from tests import pass_refs_f64_qrcp as pq

U = pk.U
LD = pk.LD
CASES = pk.CASES
RHS_KINDS = pk.RHS_KINDS


# ---- extended precision --------------------------------------------------------------------------------------------------------------------
def qr_ld(y):
    """(Q, R) of a full-column-rank y in longdouble: classical Gram-Schmidt, each column orthogonalised twice"""
    y = np.asarray(y, LD)
    m, k = y.shape
    q, r = np.zeros((m, k), LD), np.zeros((k, k), LD)
    for j in range(k):
        v = y[:, j].copy()
        for _ in range(2):
            c = q[:, :j].T @ v
            v -= q[:, :j] @ c
            r[:j, j] += c
        r[j, j] = np.sqrt(v @ v)
        q[:, j] = v / r[j, j]
    return q, r


def minnorm_ld(a, b, cols):
    """X*, the minimum-norm solution of the problem truncated at the columns cols, in longdouble: Q1 from a QR of A[:, cols], S = Q1^T A
    (k x n, full row rank), S^T = Qs Rs, X* = Qs Rs^-T Q1^T B -- the least-norm solution of S X = Q1^T B"""
    q1, _ = qr_ld(np.asarray(a, LD)[:, list(cols)])
    s, c = q1.T @ np.asarray(a, LD), q1.T @ np.asarray(b, LD).reshape(len(a), -1)
    qs, rs = qr_ld(s.T)
    y = np.zeros_like(c)
    for i in range(rs.shape[0]):
        y[i] = (c[i] - rs[:i, i] @ y[:i]) / rs[i, i]
    return qs @ y


# ---- Zg and the update factor ---------------------------------------------------------------------------------------------------------------
def zg_of(zeff, p, k):
    """Zeff with column j = k .. n - 1 set to the unit vector e_p[j] (lsq_zg_f64_kernel)"""
    z = np.array(zeff, np.float64)
    for j in range(k, z.shape[0]):
        z[p[j], j] = 1.0
    return z


def s12_of(g, k):
    """(Rc, S12 = Rc^-T G12) by the kernel's right-looking Cholesky of G[:k, :k] with the columns k .. n - 1 of its rows carried along;
    (None, None) on a bad pivot"""
    n = g.shape[0]
    w = np.asarray(g, np.float64)[:k].copy()
    w[:, :k] = np.triu(w[:, :k])
    for p in range(k):
        d = w[p, p]
        if not (d > 0.0) or not np.isfinite(d):
            return None, None
        rpp = np.sqrt(d)
        w[p, p + 1:] = w[p, p + 1:] / rpp
        w[p, p] = rpp
        for i in range(p + 1, k):
            w[i, i:] -= w[p, i] * w[p, i:]
    return w[:, :k], w[:, k:n]


def zmn_of(g, zeff, p, k, defect=None, r=None):
    """(Zmn n x n, verdict) of lsq_minnorm_f64_kernel: g the n x n Gram matrix on Zg (G11 = g[:k, :k], G12 = g[:k, k:]; nothing else is
    read), zeff the n x n Zeff behind the step.  T = P1^T Zeff, M = T S12, C = I + M M^T = Uc^T Uc, Ui = inverse(Uc), V = Ui (Ui^T T),
    rows p[:k] of Zmn are V and rows p[k:] are M^T V.  Verdict 1: a pivot of G11; 2: a pivot of C; both leave Zmn = 0.  defects:
    'r12_from_r' takes M = inverse(R11) R12 from the pivoted R (r) instead of G12; 'no_perm' leaves the rows unpermuted; 'basic' drops
    the rows M^T V (the basic solution)."""
    n = zeff.shape[0]
    p = np.asarray(p)
    out = np.zeros((n, n))
    if k == 0:
        return out, 0
    rc, s12 = s12_of(g, k)
    if rc is None:
        return out, 1
    t = np.triu(np.asarray(zeff, np.float64)[p[:k], :k])
    mm = t @ s12
    if defect == "r12_from_r":
        rr = np.asarray(r, np.float64)
        mm = pk.back_inverse(rr[:k, :k]) @ rr[:k, k:]
    uc = ps.chol_upper(np.eye(k) + mm @ mm.T)
    if uc is None:
        return out, 2
    ui = pk.back_inverse(uc)
    v = ui @ (ui.T @ t)
    rows = np.arange(n) if defect == "no_perm" else p
    out[rows[:k], :k] = v
    if defect != "basic":
        out[rows[k:], :k] = mm.T @ v
    return out, 0


def model_lstsq_minnorm(a, b, rcond, refine=1, defect=None, r0=None):
    """fp64 model of the entry, tile-free: pass_refs_f64_lsq_rank_step.model_lstsq_rank_step with the Gram matrix taken on Zg, Zmn behind
    the step, and Zmn as the factor of the update.  r0: the R0 the pivoted QR starts from (the tests pass ladder_r0_model's, which is
    inconsistent behind an exactly copied column: defect 'r12_from_r' reads it there, the sound path does not; None: Householder's).
    Returns (X, R, p, rank, Zeff, Zmn)."""
    n = a.shape[1]
    r0 = pl.householder_r(a) if r0 is None else r0
    r, _, p = pq.householder_qrcp(r0, dtype=np.float64)
    p = np.asarray(p)
    k = pk.rank_of(r, rcond)
    z = pk.zeff_of(r, p, k)
    q = a @ zg_of(z, p, k)
    g = q.T @ q
    z, verdict = ps.step_of(z, g, k)
    assert verdict == 0, "the Cholesky step of the model met a bad pivot"
    zmn, verdict = zmn_of(g, z, p, k, defect, r)
    assert verdict == 0, "the Cholesky factorisation of C in the model met a bad pivot"
    q = a @ z
    x, state = None, None
    for t in range(refine + 1):
        d = q.T @ (b if x is None else b - a @ x)
        x, state = pl.stagnation_step(x, zmn @ d, d, state, t)
    return x, r, p, k, z, zmn


# ---- the yardstick and the assertions of a result ---------------------------------------------------------------------------------------------
_cache = {}


def yardstick(name, kind, p, k):
    """(X*, LAPACK's error): X* = minnorm_ld(A, B, p[:k]), and rel_err against it of numpy.linalg.lstsq on the same projected problem
    (Q1^T A, Q1^T B), Q1 from numpy.linalg.qr(A[:, p[:k]]); shared among the tests of one (case, kind, p, k)"""
    key = (name, kind, tuple(int(i) for i in np.asarray(p)[:k]))
    if key not in _cache:
        a, b = pk.case_matrix(name), pk.case_rhs(name, kind)
        ref = pl._frozen(np.asarray(minnorm_ld(a, b, np.asarray(p)[:k]), np.float64))
        q1, _ = np.linalg.qr(a[:, np.asarray(p)[:k]])
        lap = np.linalg.lstsq(q1.T @ a, q1.T @ b, rcond=None)[0]
        _cache[key] = (ref, pl.rel_err(lap, ref))
    return _cache[key]


def figures(name, kind, x, p, k):
    """{err, lapack, bound} of a result of a case"""
    n = pk.case_matrix(name).shape[1]
    ref, lap = yardstick(name, kind, p, k)
    return {"err": pl.rel_err(np.asarray(x, np.float64).reshape(n, -1), ref), "lapack": lap, "bound": max(2.0 * lap, pl.floor_of(n))}


def check(name, kind, x, p, k):
    """the assertions of a refine = 1 result: precondition(), the expected rank, p a permutation,
    rel_err(X, X*) <= max(2 x LAPACK's, floor_of(n)).  Returns figures()."""
    _, m, n, _, _, k_expected = next(c[:6] for c in CASES if c[0] == name)
    pk.precondition(name)
    assert k == k_expected, (name, "rank", k, k_expected)
    assert sorted(int(i) for i in p) == list(range(n)), (name, "jpvt is no permutation")
    f = figures(name, kind, x, p, k)
    assert f["err"] <= f["bound"], (name, kind, f)
    return f


# ---- the data of the kernel's test ----------------------------------------------------------------------------------------------------------
FACTOR_SHAPES = ((1, 1), (7, 4), (16, 15), (17, 17), (33, 1), (51, 32), (64, 40), (16, 0))     # (n, k)


def factor_case(n, k, seed=0):
    """-> (G n x n in fp64, Zeff n x n behind the step, p): a Gaussian A (m = 4 n + 3 rows), R and p from Householder QR with column
    pivoting, the rank SET to k (S = Q1^T A P and its pseudo-inverse are defined for any k), Zeff = zeff_of(R, p, k), G the Gram matrix
    of A Zg formed in longdouble and rounded once, Zeff <- step_of(Zeff, G, k): what the kernel is handed in the entry, up to the
    rounding of the Gram pass."""
    rng = np.random.default_rng(7000 * n + 10 * k + seed)
    a = rng.standard_normal((4 * n + 3, n))
    r, _, p = pq.householder_qrcp(pl.householder_r(a), dtype=np.float64)
    p = np.asarray(p)
    zeff = pk.zeff_of(r, p, k)
    q = a.astype(LD) @ zg_of(zeff, p, k).astype(LD)
    g = np.asarray(q.T @ q, np.float64)
    g = (g + g.T) / 2
    zeff, verdict = ps.step_of(zeff, g, k)
    assert verdict == 0
    return g, zeff, p


def s_of_inputs(g, zeff, p, k, dtype=LD):
    """S = R11' [I M] = [inverse(T) | Rc^-T G12] (k x n, in the pivoted column order) from the kernel's inputs, in dtype: G11 = Rc^T Rc by
    numpy's Cholesky of the dtype's nearest (longdouble: a Cholesky written out), T = P1^T Zeff"""
    n = g.shape[0]
    g = np.asarray(g, dtype)
    t = np.triu(np.asarray(zeff, dtype)[np.asarray(p)[:k], :k])
    if dtype is LD:
        rc = np.zeros((k, k), LD)
        w = g[:k, :k].copy()
        for i in range(k):
            rc[i, i:] = w[i, i:] / np.sqrt(w[i, i])
            w[i + 1:, i + 1:] -= np.outer(rc[i, i + 1:], rc[i, i + 1:])
        tinv, s12 = np.zeros((k, k), LD), np.zeros((k, n - k), LD)
        for j in range(k):                             # inverse(T) by back substitution, T upper triangular
            e = np.zeros(k, LD)
            e[j] = 1
            for i in range(k - 1, -1, -1):
                tinv[i, j] = (e[i] - t[i, i + 1:] @ tinv[i + 1:, j]) / t[i, i]
        for i in range(k):                             # Rc^T S12 = G12 by forward substitution
            s12[i] = (g[i, k:n] - rc[:i, i] @ s12[:i]) / rc[i, i]
    else:
        import scipy.linalg
        rc = np.linalg.cholesky(g[:k, :k]).T
        tinv = scipy.linalg.solve_triangular(t, np.eye(k))
        s12 = scipy.linalg.solve_triangular(rc, g[:k, k:n], trans="T")
    return np.concatenate([tinv, s12], axis=1)


def factor_residuals(s_ld, zmn, p, k):
    """(||S P^T Zmn - I_k||_F, ||(I - pinv(S) S) P^T Zmn||_F) in longdouble; the projector from a QR of S^T"""
    zp = np.asarray(zmn, LD)[np.asarray(p), :k]
    e = s_ld @ zp - np.eye(k, dtype=LD)
    qs, _ = qr_ld(s_ld.T)
    f = zp - qs @ (qs.T @ zp)
    return float(np.sqrt(np.sum(e * e))), float(np.sqrt(np.sum(f * f)))


def factor_allowance(g, zeff, p, k):
    """per residual: 2 x the same figure of numpy.linalg.pinv in fp64 on the same inputs (S formed in fp64 by LAPACK), or
    k cond(C) 2^-53 if larger, C = I + M M^T"""
    n = g.shape[0]
    s_ld = s_of_inputs(g, zeff, p, k)
    s64 = s_of_inputs(g, zeff, p, k, np.float64)
    zy = np.zeros((n, n))
    zy[np.asarray(p), :k] = np.linalg.pinv(s64)
    yard = factor_residuals(s_ld, zy, p, k)
    mm = np.asarray(np.asarray(zeff, LD)[np.asarray(p)[:k], :k] @ s_ld[:, k:], np.float64)
    floor = k * np.linalg.cond(np.eye(k) + mm @ mm.T) * U
    return tuple(max(2.0 * y, floor) for y in yard), yard, floor


def structure_ok(zp, k, n):
    """exact zeros of the NP x NP Zmn in the columns >= k and in the padding rows"""
    return not zp[:, k:].any() and not zp[n:].any()

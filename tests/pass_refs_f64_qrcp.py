"""References for the pivoting pass of the fp64 pivoted QR entry (tsqr_mi_qrcp_f64), evaluated in np.longdouble (64-bit mantissa on x86):

  householder_qrcp  Householder QR with column pivoting of a square matrix with qrcp_r_f64_kernel's conventions -- the squared norms of
                    the remaining part of every remaining column summed afresh at every step (never downdated), the largest wins and the
                    lowest index on a tie, dlarfg's reflector, a zero column gives H_k = I, and a negative R_kk is made positive by
                    negating row k of R and column k of H -- in any dtype: longdouble is the reference, float64 a model of the kernel;
  figures           the pass-level error figures of a factorisation R0 P = H R and its structure;
  lapack_figures    the same figures for scipy.linalg.qr(pivoting=True) (LAPACK dgeqp3) on the same R0;
  allowance         pass_refs_f64_svd's: max(4 x LAPACK's figure, n 2^-53);
  pivot_slack       the largest of sum_{i=k..j} R_ij^2 / R_kk^2 - 1 over j > k: how far R is from the Businger-Golub property;
  r_of_cond         pass_refs_f64_svd's graded upper triangular test matrix;
  r_of_rank         an upper triangular factor of exact rank r (its rows from r on are exact zeros);
  r_of_rank_rounded the same rank-r product behind an orthogonal transform, re-triangularised: rank r up to rounding, nothing zeroed;
  separated         a matrix whose candidate norms are separated by a fixed ratio at every step, so that every correct implementation
                    takes the same pivots.

tests/test_pass_refs_f64_qrcp.py checks the reference against scipy.linalg.qr(pivoting=True)."""
import numpy as np

from tests import pass_refs_f64 as p64
from tests import pass_refs_f64_svd as ps

LD = np.longdouble
U = p64.U
allowance = ps.allowance
r_of_cond = ps.r_of_cond
fro = ps.fro


def householder_qrcp(r0, dtype=LD):
    """-> (R, H, p) with r0[:, p] = H R in dtype: R upper triangular (exact zeros below), diag(R) >= 0, H n x n orthogonal, p the
    0-based pivots"""
    m = np.array(r0, dtype=dtype)
    n = m.shape[0]
    g = np.eye(n, dtype=dtype)                               # accumulates H^T by the same column operation
    p = np.arange(n)
    zero, one = dtype(0), dtype(1)
    for k in range(n):
        norms = np.sum(m[k:, k:] * m[k:, k:], axis=0)        # afresh, from the entries as they stand
        piv = k + int(np.argmax(norms))                      # (argmax returns the first of equal maxima: the lowest index)
        if piv != k:
            m[:, [k, piv]] = m[:, [piv, k]]
            p[[k, piv]] = p[[piv, k]]
        x = m[k:, k].copy()
        alpha, s2 = x[0], np.sum(x[1:] * x[1:])
        beta = alpha
        if s2 > 0:
            beta = -np.copysign(np.sqrt(alpha * alpha + s2), alpha)
            tau = (beta - alpha) / beta
            v = x / (alpha - beta)
            v[0] = one
            for mat, first in ((m, k + 1), (g, 0)):
                d = v @ mat[k:, first:]
                mat[k:, first:] -= np.outer(tau * v, d)
        m[k, k] = beta
        m[k + 1:, k] = zero
        if beta < 0:
            m[k, k:] = -m[k, k:]
            g[k, :] = -g[k, :]
    return m, g.T.copy(), p


def figures(r0, r, h, p):
    """residual ||R0 P - H R||_F / ||R0||_F (0 for a zero R0) and h_orth ||H^T H - I||_F in longdouble, and the structure: upper (R is
    exactly upper triangular), diag_ok (diag(R) >= 0 and non-increasing), perm (p is a permutation of 0 .. n - 1)"""
    r0l, rl, hl = (np.asarray(x, LD) for x in (r0, r, h))
    n = rl.shape[0]
    p = np.asarray(p)
    perm = sorted(int(i) for i in p) == list(range(n))
    d = np.diag(np.asarray(r, np.float64))
    norm0 = fro(r0l)
    res = fro(r0l[:, p] - p64.matmul_ld(hl, rl)) if perm else float("inf")
    return {"residual": res / norm0 if norm0 > 0 else res,
            "h_orth": fro(p64.matmul_ld(hl.T, hl) - np.eye(n, dtype=LD)),
            "upper": bool(np.array_equal(np.asarray(r), np.triu(np.asarray(r)))),
            "diag_ok": bool(np.all(d >= 0) and np.all(np.diff(d) <= 0)),
            "perm": perm}


def lapack_figures(r0):
    """figures() of scipy.linalg.qr(pivoting=True) on the same matrix (|diag R| is what LAPACK orders: its signs are made positive)"""
    import scipy.linalg
    h, r, p = scipy.linalg.qr(np.asarray(r0, np.float64), pivoting=True)
    sign = np.where(np.diag(r) < 0, -1.0, 1.0)
    return figures(r0, r * sign[:, None], h * sign[None, :], p)


def pivot_slack(r):
    """max over k < j of sum_{i=k..j} R_ij^2 / R_kk^2 - 1 (longdouble; -inf for n = 1; a zero R_kk with a non-zero tail gives inf)"""
    rl = np.asarray(r, LD)
    n = rl.shape[0]
    worst = -np.inf
    for k in range(n - 1):
        tails = np.array([np.sum(rl[k:j + 1, j] ** 2) for j in range(k + 1, n)], dtype=LD)
        dk = rl[k, k] ** 2
        if dk > 0:
            worst = max(worst, float(np.max(tails) / dk - 1))
        elif np.max(tails) > 0:
            worst = np.inf
    return worst


def r_of_rank(n, rank, seed):
    """an upper triangular n x n R0 of exact rank `rank`: the R of numpy's QR of a Gaussian rank-`rank` product B C (n x rank, rank x
    n) with the rows from `rank` on -- rounding of that QR, 1e-16 of the rest -- set to exact zeros"""
    rng = np.random.default_rng(seed)
    _, r = np.linalg.qr(rng.standard_normal((n, rank)) @ rng.standard_normal((rank, n)))
    r = np.triu(r * np.where(np.diag(r) < 0, -1.0, 1.0)[:, None])
    r[rank:, :] = 0.0
    return r


def r_of_rank_rounded(n, rank, seed):
    """r_of_rank's rank-`rank` product multiplied by a Haar-like orthogonal matrix from the left and made triangular again by numpy's
    QR, nothing zeroed: an upper triangular R0 that has rank `rank` up to the rounding of that product and QR, its rows from `rank`
    on at 1e-16 of the rest instead of exact zeros -- the trailing pivots of a pivoted QR are then finite numbers at rounding level"""
    rng = np.random.default_rng(seed)
    low = rng.standard_normal((n, rank)) @ rng.standard_normal((rank, n))
    w, _ = np.linalg.qr(rng.standard_normal((n, n)))
    _, r = np.linalg.qr(w @ low)
    return np.triu(r * np.where(np.diag(r) < 0, -1.0, 1.0)[:, None])


def separated(n, seed, ratio=0.75):
    """the upper triangular factor (numpy's QR) of a matrix with orthogonal columns of lengths ratio^0 .. ratio^(n-1) in a shuffled
    order: at every step of a pivoted QR the largest remaining column norm exceeds the second largest by 1 / ratio, up to rounding,
    so the pivots cannot depend on rounding.  The caller asserts the separation with candidate_gaps()."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    cols = q * (ratio ** np.arange(n))                       # orthogonal columns of graded length: the norms never mix
    shuffled = cols[:, rng.permutation(n)]
    _, r = np.linalg.qr(shuffled)
    return np.triu(r * np.where(np.diag(r) < 0, -1.0, 1.0)[:, None])


def candidate_gaps(r0):
    """for every step of the longdouble reference on r0: second largest / largest candidate norm (squared) -- 1.0 means a tie"""
    m = np.array(r0, dtype=LD)
    n = m.shape[0]
    gaps = []
    for k in range(n - 1):
        norms = np.sum(m[k:, k:] * m[k:, k:], axis=0)
        order = np.argsort(-norms, kind="stable")
        gaps.append(float(norms[order[1]] / norms[order[0]]) if norms[order[0]] > 0 else 1.0)
        piv = k + int(order[0])
        m[:, [k, piv]] = m[:, [piv, k]]
        x = m[k:, k].copy()
        s2 = np.sum(x[1:] * x[1:])
        if s2 > 0:
            beta = -np.copysign(np.sqrt(x[0] * x[0] + s2), x[0])
            tau = (beta - x[0]) / beta
            v = x / (x[0] - beta)
            v[0] = 1
            m[k:, k + 1:] -= np.outer(tau * v, v @ m[k:, k + 1:])
    return gaps

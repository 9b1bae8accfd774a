"""Pure-numpy references for the CholeskyQR step of the rank-aware fp64 least-squares entry (lsq_rank_step_f64_kernel and
gramq_dense_f64_kernel, lsq_rank_f64.hip): a model of the step in the kernel's order of operations, a model of the
whole solve with the step on an R0 as the R-only ladder leaves it (tools/lstsq_rank_contraction.ladder_r0_model), the data of the step's
GPU test and its measure.  Built on tests/pass_refs_f64_lsq_rank.py.  No GPU, no library: tests/test_pass_refs_f64_lsq_rank_step.py
checks it on the CPU."""
import numpy as np

from tests import pass_refs as pr
from tests import pass_refs_f64_lsq as pl
from tests import pass_refs_f64_lsq_rank as pk
from tests import pass_refs_f64_qrcp as pq

U = pk.U
LD = pk.LD


# ---- the step ------------------------------------------------------------------------------------------------------------------------------
def chol_upper(g):
    """Rc with G = Rc^T Rc by right-looking Cholesky on the upper triangle, the kernel's order: step p divides row p by sqrt(g_pp), then
    entry (i, j), p < i <= j, takes one update (one rounding per term stands in for the fused multiply-add).  None when a pivot is not
    positive or not finite: the kernel's verdict 1."""
    k = g.shape[0]
    m = np.triu(np.asarray(g, np.float64)).copy()
    for p in range(k):
        d = m[p, p]
        if not (d > 0.0) or not np.isfinite(d):
            return None
        rpp = np.sqrt(d)
        m[p, p + 1:] = m[p, p + 1:] / rpp
        m[p, p] = rpp
        for i in range(p + 1, k):
            m[i, i:] -= m[p, i] * m[p, i:]
    return m


def step_of(zeff, g1, k, defect=None):
    """(Zeff inverse(Rc), verdict) for the n x n Zeff of pass_refs_f64_lsq_rank.zeff_of and G1 = (A Zeff)^T (A Zeff), of which only the
    leading k x k block is read: inverse(Rc) by back_inverse, the product column by column over l = 0 .. j.  Columns >= k are written
    as zeros; verdict 1 (and k = 0) leaves Zeff = 0.  defects: 'left_out' returns Zeff as it came; 'transposed' multiplies by
    inverse(Rc)^T; 'dense_rows' adds a rounding-size number to a zero row."""
    n = zeff.shape[0]
    if defect == "left_out":
        return zeff.copy(), 0
    out = np.zeros((n, n))
    if k == 0:
        return out, 0
    rc = chol_upper(np.asarray(g1, np.float64)[:k, :k])
    if rc is None:
        return out, 1
    zi = pk.back_inverse(rc)
    if defect == "transposed":
        zi = zi.T.copy()
    for j in range(k):
        s = np.zeros(n)
        for l in range(j + 1) if defect != "transposed" else range(k):
            s = s + zeff[:, l] * zi[l, j]
        out[:, j] = s
    if defect == "dense_rows":
        zero = np.flatnonzero(~out.any(axis=1))
        if zero.size:
            out[zero[0], 0] = 2.0 ** -60
    return out, 0


def model_lstsq_rank_step(a, b, rcond, refine=1, defect=None, r0=None):
    """fp64 model of the entry, tile-free: pass_refs_f64_lsq_rank.model_lstsq_rank with the step between Zeff and the passes.  r0: the R0
    the pivoted QR starts from (the tests pass ladder_r0_model's; None: Householder's).  Returns (X, R, p, rank, Zeff after the step)."""
    r0 = pl.householder_r(a) if r0 is None else r0
    r, _, p = pq.householder_qrcp(r0, dtype=np.float64)
    k = pk.rank_of(r, rcond)
    z = pk.zeff_of(r, p, k)
    q = a @ z
    z, verdict = step_of(z, q.T @ q, k, defect)
    assert verdict == 0, "the Cholesky step of the model met a bad pivot"
    q = a @ z
    x, state = None, None
    for t in range(refine + 1):
        d = q.T @ (b if x is None else b - a @ x)
        x, state = pl.stagnation_step(x, z @ d, d, state, t)
    return x, r, p, k, z


# ---- the data of the step kernel's test ----------------------------------------------------------------------------------------------------
STEP_SHAPES = ((1, 1), (16, 15), (33, 1), (51, 32), (64, 40), (64, 64))     # (n, k)
STEP_EPS = (0.0, 1e-8, 2e-2)


def step_case(n, k, eps, seed=0):
    """-> (Zeff n x n, G1 n x n in fp64 with zeros outside [:k, :k], p, R11 in fp64, Q^T Q in longdouble).  The retained columns are
    A P1 = Q R11 EXACTLY (never rounded): Q (m x k, m = 4 n + 3) = orth + eps noise with ||noise||_2 = 1, R and p from Householder QR
    with column pivoting of a Gaussian matrix, Zeff = zeff_of(R, p, k).  The true Gram matrix of the columns is R11^T (Q^T Q) R11, so
    (A Zeff)^T (A Zeff) = T^T (Q^T Q) T with T = R11 (P1^T Zeff)[:k, :k], formed in longdouble and rounded once: what the Gram pass hands to
    the step, up to its own rounding."""
    rng = np.random.default_rng(1000 * n + 10 * k + seed)
    m = 4 * n + 3
    r, _, p = pq.householder_qrcp(pl.householder_r(rng.standard_normal((m, n))), dtype=np.float64)
    p = np.asarray(p)
    zeff = pk.zeff_of(r, p, k)
    orth, _ = np.linalg.qr(rng.standard_normal((m, k)))
    noise = rng.standard_normal((m, k))
    q = orth.astype(LD) + LD(eps) * (noise / np.linalg.norm(noise, 2)).astype(LD)
    qtq = q.T @ q
    r11 = np.asarray(r, np.float64)[:k, :k]
    t = r11.astype(LD) @ zeff[p[:k], :k].astype(LD)
    g1 = np.zeros((n, n))
    g1[:k, :k] = np.asarray(t.T @ qtq @ t, np.float64)
    g1[:k, :k] = (g1[:k, :k] + g1[:k, :k].T) / 2
    return zeff, g1, p, r11, qtq


def step_residual(zout, p, k, r11, qtq):
    """||Zout^T G Zout - I_k||_F in longdouble for the true Gram matrix G = P1 R11^T (Q^T Q) R11 P1^T of the columns, in its factored
    form: T^T (Q^T Q) T with T = R11 (P1^T Zout)[:k, :k]"""
    t = r11.astype(LD) @ np.asarray(zout, LD)[np.asarray(p)[:k], :k]
    e = t.T @ qtq @ t - np.eye(k, dtype=LD)
    return float(np.sqrt(np.sum(e * e)))


def step_allowance(zeff, g1, p, k, r11, qtq):
    """4 x step_residual of numpy's Cholesky and scipy.linalg.solve_triangular on the same data, or k 2^-53 if larger"""
    import scipy.linalg
    rc = np.linalg.cholesky(g1[:k, :k]).T
    zout = np.zeros_like(zeff)
    zout[:, :k] = zeff[:, :k] @ scipy.linalg.solve_triangular(rc, np.eye(k))
    return max(4.0 * step_residual(zout, p, k, r11, qtq), k * U)


def pack_g(g, n):
    """n x n symmetric G -> the summed tiles the step kernel reads (pass_refs.pack_tiles, fp64 layout)"""
    return pr.pack_tiles(g, n, False)


# ---- exact data of the dense Gram pass ----------------------------------------------------------------------------------------------------
def exact_dense_gram_case(rng, m, n, upper=False):
    """(A, Z): A integers in [-3, 3], Z DENSE in {-1, 0, 1} (upper: upper triangular, not unit), as pass_refs_f64_lsq_rank.exact_dense_case.
    |A Z| <= 3 n <= 192 and every partial sum of (A Z)^T (A Z) is an integer below m 192^2 < 2^53 (asserted on the data at hand)."""
    assert n <= 64
    a = rng.integers(-pl.AMAX, pl.AMAX + 1, size=(m, n)).astype(np.float64)
    z = rng.integers(-1, 2, size=(n, n)).astype(np.float64)
    if upper:
        z = np.triu(z)
    q = a @ z
    assert np.abs(q).max() <= pl.AMAX * 64 and m * max(float(np.abs(q).max()), 1.0) ** 2 < 2.0 ** 53, "a partial sum could leave the exact range"
    return a, z


def gram_dense_exact(a, z):
    q = a @ z
    return q.T @ q

"""References for the passes of the fp64 SVD entry (tsqr_mi_svd_f64), evaluated in np.longdouble (64-bit mantissa on x86):

  jacobi_svd     one-sided (Hestenes) Jacobi on a square or tall matrix, cyclic by rows, run until a sweep rotates nothing at the
                 threshold of the working precision -- the singular values and vectors the GPU passes are held against;
  qr_jacobi_svd  a whole tall matrix: a QR in extended precision (numpy's Householder R as a preconditioner, then two CholeskyQR steps in
                 longdouble with pass_refs_f64's chol_ld / trinv_ld / matmul_ld), then jacobi_svd on R and U = Q W;
  figures        the four pass-level error figures of a factorisation M = W diag(s) V^T against the reference singular values;
  allowance      the bound of a figure: max(4 x the same figure of numpy.linalg.svd on the same data, n 2^-53);
  kernel_model   svd_r_f64_kernel's algorithm step by step in fp64 numpy -- the scaling, the round-robin order, the rotations, and the
                 end with or without dividing out the norm drift of the rotation product -- the source of the model figures that the
                 kernel's comment and DESIGN.md quote.

tests/test_pass_refs_f64_svd.py checks the two references against numpy.linalg.svd."""
import numpy as np

from tests import pass_refs_f64 as p64

LD = np.longdouble
U = p64.U


def jacobi_svd(mat, dtype=LD, max_sweeps=60):
    """-> (s descending, W (rows x n, orthonormal columns), V (n x n), sweeps) with mat = W diag(s) V^T, all in dtype"""
    m = np.array(mat, dtype=dtype)
    n = m.shape[1]
    v = np.eye(n, dtype=dtype)
    tol = dtype(np.sqrt(n)) * np.finfo(dtype).eps / 2
    one = dtype(1)
    sweeps = 0
    for sweeps in range(1, max_sweeps + 1):
        rotated = False
        for p in range(n - 1):
            for q in range(p + 1, n):
                app, aqq, apq = m[:, p] @ m[:, p], m[:, q] @ m[:, q], m[:, p] @ m[:, q]
                if not abs(apq) > tol * np.sqrt(app) * np.sqrt(aqq):
                    continue
                zeta = (aqq - app) / (2 * apq)
                t = np.copysign(one, zeta) / (abs(zeta) + np.sqrt(one + zeta * zeta))
                if t == 0:
                    continue
                c = one / np.sqrt(one + t * t)
                s = c * t
                for x in (m, v):
                    xp, xq = x[:, p].copy(), x[:, q].copy()
                    x[:, p], x[:, q] = c * xp - s * xq, s * xp + c * xq
                rotated = True
        if not rotated:
            break
    else:
        raise AssertionError("the reference Jacobi iteration did not converge")
    sig = np.sqrt(np.sum(m * m, axis=0))
    order = np.argsort(-sig, kind="stable")
    sig, m, v = sig[order], m[:, order], v[:, order]
    w = np.where(sig > 0, m / np.where(sig > 0, sig, one), 0)
    return sig, w, v, sweeps


def qr_ld(a):
    """(Q, R) of a tall matrix in longdouble, R upper triangular with a positive diagonal: A inverse(R0) with R0 numpy's Householder R
    (orthonormal to cond(A) u: Householder QR is backward stable), then two CholeskyQR steps on it in extended precision, each
    multiplying R on the left -- nothing of A is dropped, and Q is orthonormal to the extended precision"""
    al = np.asarray(a, LD)
    r0 = np.linalg.qr(np.asarray(a, np.float64))[1]
    r = np.triu(r0 * np.where(np.diag(r0) < 0, -1.0, 1.0)[:, None]).astype(LD)
    q = p64.matmul_ld(al, p64.trinv_ld(r))
    for _ in range(2):
        r2 = p64.chol_ld(p64.matmul_ld(q.T, q))
        q = p64.matmul_ld(q, p64.trinv_ld(r2))
        r = np.triu(p64.matmul_ld(r2, r))
    return q, r


def qr_jacobi_svd(a):
    """-> (s, U, V) of the tall matrix a in longdouble: extended-precision QR, Jacobi on R, U = Q W"""
    q, r = qr_ld(a)
    s, w, v, _ = jacobi_svd(r)
    return s, p64.matmul_ld(q, w), v


def fro(x):
    return float(np.sqrt(np.sum(np.asarray(x, LD) ** 2)))


def figures(mat, s, w, v, s_ref):
    """the four figures of mat = w diag(s) v^T: E_sigma = max_j |s_j - s*_j| / s*_1, ||w^T w - I||_F, ||v^T v - I||_F,
    ||mat - w diag(s) v^T||_F / ||mat||_F, evaluated in longdouble"""
    mat, s, w, v, s_ref = (np.asarray(x, LD) for x in (mat, s, w, v, s_ref))
    n = s.size
    eye = np.eye(n, dtype=LD)
    return {"sigma": float(np.max(np.abs(s - s_ref)) / s_ref[0]),
            "w_orth": fro(p64.matmul_ld(w.T, w) - eye),
            "v_orth": fro(p64.matmul_ld(v.T, v) - eye),
            "residual": fro(mat - p64.matmul_ld(w * s, v.T)) / fro(mat)}


def lapack_figures(mat, s_ref):
    """the same figures for numpy.linalg.svd (LAPACK gesdd) on the same matrix"""
    w, s, vh = np.linalg.svd(np.asarray(mat, np.float64), full_matrices=False)
    return figures(mat, s, w, vh.T, s_ref)


def allowance(lapack_figure, n):
    """what a figure may reach: four times LAPACK's on the same data -- a different but equally valid rounding order -- and never
    below n 2^-53, so that a lucky exact LAPACK result does not make the bound zero"""
    return max(4.0 * lapack_figure, n * U)


def r_of_cond(n, cond, seed):
    """an upper triangular n x n R (positive diagonal) with singular values graded geometrically from 1 down to 1 / cond: the R of
    numpy's QR of U diag(s) V^T with Haar-like U, V"""
    rng = np.random.default_rng(seed)
    u, _ = np.linalg.qr(rng.standard_normal((n, n)))
    v, _ = np.linalg.qr(rng.standard_normal((n, n)))
    s = np.ones(1) if n == 1 else cond ** (-np.arange(n) / (n - 1.0))
    _, r = np.linalg.qr((u * s) @ v.T)
    return np.triu(r * np.where(np.diag(r) < 0, -1.0, 1.0)[:, None])


def kernel_model(r, transpose=True, renormalise=True, max_sweeps=30):
    """svd_r_f64_kernel in fp64 numpy -> (s, W, V, sweeps, J): M = R^T (or R) scaled to max |m_ij| in [1, 2), round-robin pairs (the
    circle method on n rounded up to even), dgesvj's criterion, the cap of 30 sweeps.  renormalise: the kernel's end -- sigma_j =
    ||m_j|| / ||j_j||, J <- J diag(||j_j||)^-1; without it sigma_j = ||m_j|| and J as accumulated.  J is returned as accumulated,
    in the sorted order.  The sums are numpy's, not the kernel's butterfly: figures agree in size, not in bits."""
    n = r.shape[0]
    m = np.array(r.T if transpose else r, np.float64)
    j = np.eye(n)
    ex = int(np.floor(np.log2(np.abs(m).max())))
    m = np.ldexp(m, -ex)
    ne = (n + 1) & ~1
    nsteps, tol = ne - 1, np.sqrt(n) * U
    sweeps = 0
    for sweeps in range(1, max_sweeps + 1):
        rotated = False
        for st in range(nsteps):
            for k in range(ne // 2):
                c0, c1 = (st, ne - 1) if k == 0 else ((st + k) % nsteps, (st - k + nsteps) % nsteps)
                p, q = min(c0, c1), max(c0, c1)
                if q >= n:
                    continue
                mp, mq = m[:, p].copy(), m[:, q].copy()
                app, aqq, apq = mp @ mp, mq @ mq, mp @ mq
                if not abs(apq) > tol * (np.sqrt(app) * np.sqrt(aqq)):
                    continue
                zeta = (aqq - app) / (2 * apq)
                t = np.copysign(1.0, zeta) / (abs(zeta) + np.sqrt(1 + zeta * zeta))
                if t == 0:
                    continue
                c = 1 / np.sqrt(1 + t * t)
                s = c * t
                m[:, p], m[:, q] = c * mp - s * mq, s * mp + c * mq
                jp, jq = j[:, p].copy(), j[:, q].copy()
                j[:, p], j[:, q] = c * jp - s * jq, s * jp + c * jq
                rotated = True
        if not rotated:
            break
    mnorm, jnorm = np.sqrt((m * m).sum(0)), np.sqrt((j * j).sum(0))
    sig = mnorm / jnorm if renormalise else mnorm
    order = np.argsort(-sig, kind="stable")
    x = (m / np.where(mnorm > 0, mnorm, 1.0))[:, order]
    jo = j[:, order]
    jout = jo / jnorm[order] if renormalise else jo
    w, v = (jout, x) if transpose else (x, jout)
    return np.ldexp(sig[order], ex), w, v, sweeps, jo

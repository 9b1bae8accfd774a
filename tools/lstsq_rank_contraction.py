"""The contraction of the rank-aware least-squares solve on an R0 as the R-only ladder leaves it, on the CPU, on
the seven cases of tests/pass_refs_f64_lsq_rank.py, Gaussian B.  No GPU, no library: numpy alone.

  ladder_r0_model  an fp64 model of tsqr_mi_r_f64's ladder as far as it matters here: every sweep forms the Gram matrix of A Z_acc FROM A
                   (Q is never stored), factors it by Cholesky, and factors G + s I instead, s = 11 u (m n + n (n + 1)) trace(G), when a
                   pivot is not positive or the smallest pivot ratio r_jj^2 / g_jj is below 2^-40; one more sweep after a plain first
                   one, two more after the last shifted one, six at most.  A MODEL of the ladder, not the ladder.
  plain            the solve as the passes stand: pivoted QR of R0, rank, Zeff = P1 inverse(R11), X <- X + Zeff (A Zeff)^T (B - A X).
  with the step    one CholeskyQR step on the retained columns in front of the passes: G1 = (A Zeff)^T (A Zeff), G1 = Rc^T Rc,
                   Zeff <- Zeff inverse(Rc) -- what an entry still needs (not built on the device).

Per case it prints ||Q1^T Q1 - I||_2 of Q1 = A Zeff, the factor by which a pass reduces the error, and the error against the
extended-precision solve on the retained columns after 1 .. 4 passes, next to the bound max(2 x LAPACK's error, 4 n u).  On the copied
interior column the plain solve contracts by about 2e-2 only: the image of the dependent column under Z_acc is rounding noise drawn
afresh in every sweep, so R0 is inconsistent in the columns behind it.  profiles/fp64_lstsq_rank_accuracy.md holds the output."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import pass_refs_f64_lsq_rank as pk               # noqa: E402
from tests import pass_refs_f64_qrcp as pq                   # noqa: E402

U = pk.U


def ladder_r0_model(a):
    """-> (R0, sweeps, index of the last shifted sweep or -1)"""
    m, n = a.shape

    def chol(g, shift):
        try:
            r = np.linalg.cholesky(g + shift * np.eye(n)).T
        except np.linalg.LinAlgError:
            return None, 0.0
        return r, float((np.diag(r) ** 2 / np.diag(g + shift * np.eye(n))).min())
    zacc, r0, k, last = np.eye(n), np.eye(n), 0, -1
    while k < 6:
        q = a @ zacc
        g = q.T @ q
        r, ratio = chol(g, 0.0)
        if r is None or ratio < 2.0 ** -40:
            r, _ = chol(g, 11 * U * (m * n + n * (n + 1)) * np.trace(g))
            last = k
        r0, zacc, k = r @ r0, zacc @ np.linalg.inv(r), k + 1
        if k >= max(2, last + 3):
            break
    return r0, k, last


def solve(name, a, b, r, p, k, step):
    """-> (contraction, [error after 1 .. 4 passes])"""
    z = pk.zeff_of(r, p, k)
    if step:
        q = a @ z[:, :k]
        rc = np.linalg.cholesky(q.T @ q).T
        z[:, :k] = z[:, :k] @ np.linalg.inv(rc)
    q = a @ z
    c = float(np.linalg.norm(q[:, :k].T @ q[:, :k] - np.eye(k), 2))
    x, errs = None, []
    for _ in range(4):
        d = q.T @ (b if x is None else b - a @ x)
        x = z @ d if x is None else x + z @ d
        f = pk.figures(name, "gaussian", x, p, k)
        assert f["zero_rows"]
        errs.append(f["err"])
    return c, errs, f["bound"]


def main():
    for name, m, n, nrhs, rcond, k_expected in (c[:6] for c in pk.CASES):
        a, b = np.array(pk.case_matrix(name)), np.array(pk.case_rhs(name, "gaussian"))
        r0, sweeps, last = ladder_r0_model(a)
        r, _, p = pq.householder_qrcp(r0, dtype=np.float64)
        k = pk.rank_of(r, pk.rcond_of(rcond, m, n))
        assert k == k_expected, (name, k)
        for step in (False, True):
            c, errs, bound = solve(name, a, b, r, p, k, step)
            print("%-16s sweeps %d last shifted %2d rank %2d %-13s contraction %.1e errors %s bound %.1e %s"
                  % (name, sweeps, last, k, "with the step" if step else "plain", c, " ".join("%.1e" % e for e in errs), bound,
                     "inside after 2 passes" if errs[1] <= bound else "OUTSIDE after 2 passes"))
    return 0


if __name__ == "__main__":
    sys.exit(main())

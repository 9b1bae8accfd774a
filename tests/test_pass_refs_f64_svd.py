"""The references of tests/pass_refs_f64_svd.py against numpy.linalg.svd: the extended-precision Jacobi SVD and the QR-then-Jacobi SVD
of a whole matrix must agree with LAPACK to LAPACK's own accuracy (a few n u relative to the largest singular value), be orthonormal
and reproduce the matrix far below fp64 rounding -- on n = 1, 2, 17, 64, a matrix with repeated singular values and one of cond 1e12."""
import numpy as np
import pytest

from tests import pass_refs_f64 as p64
from tests import pass_refs_f64_svd as ps

LD = np.longdouble
NS = (1, 2, 17, 64)


def setup_module(module):
    p64.require_longdouble()


def check_reference(mat, s, w, v):
    n = mat.shape[1]
    s64 = np.linalg.svd(mat, compute_uv=False)
    assert np.all(np.diff(np.asarray(s, np.float64)) <= 0) and np.all(s >= 0)
    assert np.max(np.abs(np.asarray(s, np.float64) - s64)) <= 8 * n * p64.U * s64[0], "singular values against LAPACK"
    f = ps.figures(mat, s, w, v, s)
    assert f["w_orth"] <= 1e-17 * n and f["v_orth"] <= 1e-17 * n and f["residual"] <= 1e-17 * n, f


@pytest.mark.parametrize("n", NS)
def test_jacobi_reference_against_lapack(n):
    rng = np.random.default_rng(n)
    for mat in (rng.standard_normal((n, n)), ps.r_of_cond(n, 1e12, n), ps.r_of_cond(n, 1e6, 3 * n)):
        s, w, v, sweeps = ps.jacobi_svd(mat)
        assert sweeps <= 30
        check_reference(mat, s, w, v)


def test_jacobi_reference_repeated_singular_values():
    rng = np.random.default_rng(5)
    n = 17
    u, _ = np.linalg.qr(rng.standard_normal((n, n)))
    v, _ = np.linalg.qr(rng.standard_normal((n, n)))
    sv = np.array([3.0] * 5 + [1.0] * 7 + [0.25] * 5)
    mat = (u * sv) @ v.T
    s, w, vv, _ = ps.jacobi_svd(mat)
    check_reference(mat, s, w, vv)
    assert np.max(np.abs(np.asarray(s, np.float64) - sv)) <= 1e-14
    s, w, vv, sweeps = ps.jacobi_svd(np.eye(4))
    assert sweeps == 1 and np.array_equal(np.asarray(s, np.float64), np.ones(4)) and np.array_equal(np.asarray(w, np.float64), np.eye(4))


@pytest.mark.parametrize("n", NS)
def test_qr_jacobi_reference_against_lapack(n):
    rng = np.random.default_rng(100 + n)
    m = 3 * n + 5
    mats = [rng.standard_normal((m, n))]
    if n > 1:
        uu, _, vt = np.linalg.svd(rng.standard_normal((m, n)), full_matrices=False)
        mats.append((uu * np.geomspace(1.0, 1e-12, n)) @ vt)
    for mat in mats:
        q, r = ps.qr_ld(mat)
        assert np.all(np.diag(r) > 0) and np.array_equal(r, np.triu(r))
        assert ps.fro(p64.matmul_ld(q.T, q) - np.eye(n)) <= 1e-17 * n
        assert ps.fro(mat - p64.matmul_ld(q, r)) <= 1e-17 * n * ps.fro(mat)
        s, u, v = ps.qr_jacobi_svd(mat)
        check_reference(mat, s, u, v)


def test_allowance_has_a_floor_and_follows_lapack():
    assert ps.allowance(0.0, 64) == 64 * p64.U
    assert ps.allowance(1e-14, 64) == 4e-14
    r = ps.r_of_cond(17, 1e6, 1)
    assert np.array_equal(r, np.triu(r)) and np.all(np.diag(r) > 0)
    assert 0.5e6 < np.linalg.cond(r) < 2e6


def test_kernel_model_norm_drift_and_triangle_choice():
    """What the kernel's end and its choice of triangle rest on, in the fp64 model of the kernel at n = 64, cond 1e6: nearly all of
    ||J^T J - I||_F of the accumulated rotations sits on the diagonal (the norm drift); without dividing it out the figures of W miss
    max(4 x LAPACK, n 2^-53), with it all four are inside; and the columns of R^T need fewer sweeps than those of R."""
    n = 64
    r = ps.r_of_cond(n, 1e6, 7 * n)
    s_ref = ps.jacobi_svd(r)[0]
    lapack = ps.lapack_figures(r, s_ref)
    s, w, v, sweeps, jacc = ps.kernel_model(r, transpose=True, renormalise=True)
    e = p64.matmul_ld(jacc.T, jacc) - np.eye(n)
    diag, total = ps.fro(np.diag(np.diag(e))), ps.fro(e)
    off = float(np.sqrt(total ** 2 - diag ** 2))
    print("model n 64 cond 1e6: %d sweeps, ||J^T J - I||_F %.2e (diagonal %.2e, off the diagonal %.2e)" % (sweeps, total, diag, off))
    assert diag > 3 * off, "the norm drift no longer dominates: the kernel's end needs another look"
    assert total > ps.allowance(lapack["w_orth"], n), "the accumulated rotations are inside the allowance without the renormalisation"
    f = ps.figures(r, s, w, v, s_ref)
    for key in f:
        assert f[key] <= ps.allowance(lapack[key], n), (key, f[key], lapack[key])
    sweeps_r = ps.kernel_model(r, transpose=False)[3]
    print("model n 64 cond 1e6: sweeps on R^T %d, on R %d" % (sweeps, sweeps_r))
    assert sweeps < sweeps_r <= 30

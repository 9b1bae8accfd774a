"""Pure-numpy references for the tests of the R-only fp64 entry (tsqr_mi_r_f64): exact data with an asserted bit budget and the per-entry
bound of the pass that takes the Gram matrix of A Z without storing A Z (gramq_f64_kernel, tsqr_f64.hip), a numpy model of that pass with
the defects the tests must catch, the operand of the Z product, and the two longdouble measures of an R factor that the entry's tests
assert.  No GPU, no library: tests/test_pass_refs_f64_r.py checks it on the CPU.  Notation as in tests/pass_refs_f64.py."""
import numpy as np

from tests import pass_refs as pr
from tests import pass_refs_f64 as p64

U = p64.U
LD = p64.LD


def np_of(n):
    return 16 * pr.ntiles(n)


def pad_z(z, n):
    """n x n upper-triangular Z -> the NP x NP column-major block (ld NP) chol_f64_kernel leaves, zero padded"""
    np_ = np_of(n)
    zp = np.zeros((np_, np_))
    zp[:n, :n] = z
    return np.ascontiguousarray(zp.T).reshape(-1)


def unpad_z(v, n):
    np_ = np_of(n)
    return np.asarray(v)[:np_ * np_].reshape(np_, np_).T.copy()


# ---- exact data ----------------------------------------------------------------------------------------------------------------------
AMAX = 3


def exact_pair(rng, m, n):
    """(A, Z): A integers in [-3, 3], Z unit upper triangular with entries in {-1, 0, 1}.  Every entry of A Z is an integer of magnitude
    <= 3 n <= 192, every Gram entry an integer below m 192^2: exact in fp64, fused or not, in any order, while m 192^2 < 2^53."""
    assert n <= 64 and m * (AMAX * 64) ** 2 < 1 << 53, (m, n)
    a = rng.integers(-AMAX, AMAX + 1, size=(m, n)).astype(np.float64)
    z = np.triu(rng.integers(-1, 2, size=(n, n)), 1).astype(np.float64) + np.eye(n)
    q = a @ z
    assert np.abs(q).max() <= AMAX * 64 and m * float(np.abs(q).max()) ** 2 < 2.0 ** 53
    return a, z


def gramq_exact(a, z):
    """(A Z)^T (A Z) of exact_pair data: plain fp64 products are exact (budget asserted there)"""
    q = a @ z
    return q.T @ q


# ---- dense data ------------------------------------------------------------------------------------------------------------------------
def mixed_triangular(rng, n):
    """upper triangular, Gaussian entries, column scales from 1e-6 to 1e6 in random order"""
    s = 10.0 ** rng.permutation(np.linspace(-6.0, 6.0, n))
    return np.triu(rng.standard_normal((n, n))) * s[None, :]


def gramq_bound(a, z):
    """|G^ - G| <= 1.01 (m + 2 n + 16) u P per entry, P = (|A| |Z|)^T (|A| |Z|).  To first order: every entry of Q = A Z is a chain of at
    most n products, gamma_n |A| |Z|, and enters each Gram product twice (2 n u); the sum over the rows is m terms in MFMA chains, the
    workgroup sum and the fixed reduction tree (m + 16 covers every split of the m terms over waves: the depth never exceeds the number
    of terms plus the tree); P dominates |Q|^T |Q|."""
    m, n = a.shape
    p = np.abs(a) @ np.abs(z)
    return 1.01 * (m + 2 * n + 16) * U * (p.T @ p)


def gramq_ld(a, z, rows=None):
    """(A Z)^T (A Z) in longdouble (rows: only these rows of the result)"""
    q = p64.matmul_ld(a, z)
    left = q if rows is None else q[:, rows]
    return left.T @ q


# ---- numpy model of the pass, with the defects the tests must catch ---------------------------------------------------------------------
def model_gramq(a, z, defect=None):
    """fp64 model of gramq_f64_kernel + reduction -> the tile array (pass_refs.pack_tiles, f64 layout): 16-row tiles of Q = A Z, formed
    and consumed one after the other.  defects: 'drop_tile' leaves out the (ragged or not) last row tile; 'transposed_tile' stores the
    first off-diagonal tile transposed (n > 16); 'stale_z' uses Z's strict upper part only (the unit diagonal dropped)."""
    m, n = a.shape
    zz = np.triu(z, 1) if defect == "stale_z" else z
    g = np.zeros((n, n))
    nt = -(-m // 16)
    for t in range(nt):
        if defect == "drop_tile" and t == nt - 1:
            continue
        q = a[16 * t: 16 * t + 16] @ zz
        g += q.T @ q
    np_ = np_of(n)
    gp = np.zeros((np_, np_))
    gp[:n, :n] = g
    if defect == "transposed_tile":
        assert np_ > 16, "a lone diagonal tile is symmetric: the defect needs n > 16"
        gp[:16, 16:32] = gp[:16, 16:32].T.copy()
    r, c = pr._tile_index(n, False)
    return gp[r, c]


# ---- measures of an R factor (the entry's tests) ----------------------------------------------------------------------------------------
def orth_of_r(a, r):
    """||Q~^T Q~ - I||_F in longdouble, Q~ = A inverse(R) by substitution (column j of Q~ from the columns before it)"""
    p64.require_longdouble()
    m, n = a.shape
    al, rl = a.astype(LD), np.asarray(r, LD)
    q = np.zeros((m, n), LD)
    for j in range(n):
        q[:, j] = (al[:, j] - q[:, :j] @ rl[:j, j]) / rl[j, j]
    e = q.T @ q - np.eye(n, dtype=LD)
    return float(np.sqrt(np.sum(e * e)))


def gram_ld(a):
    p64.require_longdouble()
    al = a.astype(LD)
    return al.T @ al


def gram_residual_of_r(ata_ld, r):
    """||R^T R - A^T A||_F / ||A^T A||_F in longdouble"""
    rl = np.asarray(r, LD)
    e = rl.T @ rl - ata_ld
    return float(np.sqrt(np.sum(e * e)) / np.sqrt(np.sum(ata_ld * ata_ld)))


def cond_matrix(m, n, cond, seed):
    """A = U diag(sigma) V^T in fp64: U, V with orthonormal columns (Householder QR of Gaussian matrices), sigma geometric 1 .. 1 / cond"""
    rng = np.random.default_rng(seed)
    u, _ = np.linalg.qr(rng.standard_normal((m, n)))
    v, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return (u * np.geomspace(1.0, 1.0 / cond, n)) @ v.T

"""Pure-numpy references for the per-pass tests of the fp64 entries (tests/test_gpu_f64_passes.py): the wide block store's layout, exact
data with asserted bit budgets, extended-precision references and the error bounds of each pass, derived from the kernels' operation
order (tsqr_f64.hip, tsqr_f64_wide.hip, chol_body16 in tsqr_kernels.hip).  No GPU, no library: tests/test_pass_refs_f64.py checks all
of it on the CPU, and shows with seeded defects that every bound bites.

Notation: u = 2^-53; gamma_k = k u / (1 - k u); |X| is the entrywise absolute value.  The narrow path's tile order is
pass_refs.pack_tiles(..., f32_layout=False)."""
import numpy as np

from tests import pass_refs as pr

U = 2.0 ** -53
LD = np.longdouble


def require_longdouble():
    """the extended-precision references need a 64-bit significand (x86 long double); no silent fall-back to fp64"""
    eps = float(np.finfo(LD).eps)
    assert eps <= 2.0 ** -63, "np.longdouble has eps %.3g here: not an extended-precision type, the references would be fp64" % eps


def gamma(k):
    return k * U / (1.0 - k * U)


# ---- the wide block store ------------------------------------------------------------------------------------------------------------
def nblocks(n):
    return (n + 63) // 64


def wpair(i, j):
    return j * (j + 1) // 2 + i


def npairs(n):
    nb = nblocks(n)
    return nb * (nb + 1) // 2


def pack_blocks(x, n):
    """n x n matrix -> its upper block pairs (I <= J): pair p = J (J + 1) / 2 + I, X[64 I + r][64 J + c] at 4096 p + 64 c + r; rows and
    columns >= n are zeros.  Blocks below the block diagonal are not stored."""
    nb = nblocks(n)
    xp = np.zeros((64 * nb, 64 * nb), x.dtype)
    xp[:n, :n] = x
    out = np.zeros(npairs(n) * 4096, x.dtype)
    for j in range(nb):
        for i in range(j + 1):
            p = wpair(i, j)
            out[4096 * p: 4096 * (p + 1)] = xp[64 * i: 64 * i + 64, 64 * j: 64 * j + 64].T.reshape(-1)
    return out


def unpack_blocks(v, n, symmetric=False):
    """block store -> 64 nb x 64 nb matrix; the blocks below the block diagonal are zero, or the transposes of their mirrors"""
    nb = nblocks(n)
    v = np.asarray(v)
    assert v.shape == (npairs(n) * 4096,)
    x = np.zeros((64 * nb, 64 * nb), v.dtype)
    for j in range(nb):
        for i in range(j + 1):
            p = wpair(i, j)
            blk = v[4096 * p: 4096 * (p + 1)].reshape(64, 64).T
            x[64 * i: 64 * i + 64, 64 * j: 64 * j + 64] = blk
            if symmetric and i < j:
                x[64 * j: 64 * j + 64, 64 * i: 64 * i + 64] = blk.T
    return x


# ---- exact data ----------------------------------------------------------------------------------------------------------------------
def kmax_for(m):
    """largest integer magnitude with m kmax^2 < 2^53: 2^20 - 1 up to m = 2^13, 2^16 - 1 up to 2^20, 2^15 - 1 up to 2^23"""
    if m <= 1 << 13:
        return (1 << 20) - 1
    if m <= 1 << 20:
        return (1 << 16) - 1
    assert m <= 1 << 23
    return (1 << 15) - 1


def assert_gram_budget(kmax, m):
    """A = k 2^e_j, integer |k| <= kmax: every partial sum of a column pair is an integer multiple of 2^(e_i + e_j) below m kmax^2.
    With m kmax^2 < 2^53 every product and every partial sum is exact in fp64 -- in any order, fused or not."""
    assert m * kmax * kmax < 1 << 53, (m, kmax)


def exact_ints64(rng, m, n, kmax=None, exps=(-3, 3)):
    """float64 m x n, entries k 2^e_j with |k| <= kmax, most of them with all their bits in use, a fifth anywhere in [-kmax, kmax]"""
    kmax = kmax or kmax_for(m)
    assert_gram_budget(kmax, m)
    top = 1 << (pr.int_bits(kmax) - 1)
    k = rng.integers(top, kmax + 1, size=(m, n))
    k = np.where(rng.random((m, n)) < 0.2, rng.integers(-kmax, kmax + 1, size=(m, n)), k)
    k = k * rng.choice(np.array([-1, 1]), size=(m, n))
    e = rng.integers(exps[0], exps[1] + 1, size=n)
    return k.astype(np.float64) * np.exp2(e)[None, :]


def gram_exact(a):
    """A^T A of exact_ints64 data: a plain fp64 matmul is exact (assert_gram_budget), whatever order BLAS takes"""
    return a.T @ a


def exact_inverse_pair64(rng, n, split, bmax=(1 << 20) - 1, scale_exp=8):
    """R = D [[I, B], [0, I]] and its exact inverse Z = [[I, -B], [0, I]] D^-1 in fp64: B integers |b| <= bmax, D powers of two.
    With integer A, |a| <= amax, every entry of A Z is (a_j - sum_i a_i b_ij) / d_j: exact while amax (1 + split bmax) < 2^53."""
    b = rng.integers(-bmax, bmax + 1, size=(split, n - split)).astype(np.float64)
    d = np.exp2(rng.integers(-scale_exp, scale_exp + 1, size=n).astype(np.float64))
    uu = np.eye(n)
    uu[:split, split:] = b
    zi = np.eye(n)
    zi[:split, split:] = -b
    r = d[:, None] * uu
    z = zi / d[None, :]
    assert np.array_equal(r @ z, np.eye(n))
    return r, z


def assert_apply_budget(amax, split, bmax):
    assert amax * (1 + split * bmax) < 1 << 53, (amax, split, bmax)


def full_mantissa64(rng, size, spread=20):
    """float64 values with all 53 significand bits in use (lowest bit set), exponents uniform in [-spread, spread], random sign"""
    mant = rng.integers(1 << 52, 1 << 53, size=size) | 1
    e = rng.integers(-spread, spread + 1, size=size)
    s = rng.choice(np.array([-1.0, 1.0]), size=size)
    return s * np.ldexp(mant.astype(np.float64), e - 52)


def single_entry_rows64(rng, m, n):
    """m x n with exactly one non-zero (full mantissa) per row: every entry of A Z is ONE product, expected fl64(a z)"""
    a = np.zeros((m, n))
    a[np.arange(m), rng.integers(0, n, size=m)] = full_mantissa64(rng, m, 6)
    return a


def fl64_products(a, z):
    """correctly rounded a z for single_entry_rows64 data: one IEEE fp64 multiplication per entry (correctly rounded by definition;
    the zeros of the other columns add exactly), cross-checked against the 64-bit longdouble product to within half an fp64 ulp"""
    require_longdouble()
    cols = np.argmax(a != 0, axis=1)
    av = a[np.arange(a.shape[0]), cols]
    q = av[:, None] * z[cols, :]
    p = av.astype(LD)[:, None] * z[cols, :].astype(LD)
    assert np.all(np.abs(p - q.astype(LD)) <= (np.spacing(np.abs(q)) / 2).astype(LD) * (1 + LD(2) ** -10))
    return q


def int_triangular(rng, n, kmax=(1 << 20) - 1):
    """upper-triangular integer factor, |k| <= kmax: products of two such factors are exact in fp64 while n kmax^2 < 2^53"""
    assert n * kmax * kmax < 1 << 53
    return np.triu(rng.integers(-kmax, kmax + 1, size=(n, n))).astype(np.float64)


def spd(n, cond, seed, m=None):
    """(G, A): A with singular values 1 .. 1 / cond and a column scaling in [0.5, 2) (S must not care), G = A^T A in fp64"""
    rng = np.random.default_rng(seed)
    m = m or max(4 * n, 256)
    a = rng.standard_normal((m, n))
    uu, _, vt = np.linalg.svd(a, full_matrices=False)
    a = (uu * np.geomspace(1.0, 1.0 / cond, n)) @ vt
    a *= rng.uniform(0.5, 2.0, n)
    return a.T @ a, a


# ---- extended-precision references ----------------------------------------------------------------------------------------------------
def matmul_ld(x, y):
    require_longdouble()
    return x.astype(LD) @ y.astype(LD)


def chol_ld(g):
    """upper Cholesky factor of g in longdouble (plain right-looking loop)"""
    require_longdouble()
    a = np.array(g, dtype=LD)
    n = a.shape[0]
    r = np.zeros((n, n), LD)
    for k in range(n):
        r[k, k] = np.sqrt(a[k, k])
        r[k, k + 1:] = a[k, k + 1:] / r[k, k]
        a[k + 1:, k + 1:] -= np.outer(r[k, k + 1:], r[k, k + 1:])
    return r


def trinv_ld(r):
    require_longdouble()
    n = r.shape[0]
    z = np.zeros((n, n), LD)
    for j in range(n):
        z[j, j] = LD(1) / r[j, j]
        for i in range(j - 1, -1, -1):
            z[i, j] = -(r[i, i + 1: j + 1] @ z[i + 1: j + 1, j]) / r[i, i]
    return z


def scond_ref(g):
    """(S, smallest pivot ratio) of G in longdouble: S = ||D inverse(R)||_F^2 / n, D = diag(sqrt(g_jj)); ratio = min r_jj^2 / g_jj"""
    r = chol_ld(g)
    z = trinv_ld(r)
    d = np.diag(np.asarray(g, LD))
    s = np.sum(d[:, None] * z * z) / g.shape[0]
    return float(s), float(np.min(np.diag(r) ** 2 / d))


# ---- the acceptance rule (CholArgs64, tsqr_f64.hip) -----------------------------------------------------------------------------------
def rule(m, n):
    """(max_scond, alone_max, shift_coef) as the launches compute them: fp64 arithmetic, the two bounds rounded to fp32"""
    mn = float(m) * float(n) + float(n) * float(n + 1)
    return (float(np.float32(1.0 / (64.0 * n * U * mn))), float(np.float32(1e-12 / (4.0 * n * U))), 11.0 * U * mn)


# ---- bounds -----------------------------------------------------------------------------------------------------------------------------
def reduce_depth(nparts):
    """gram_reduce1_kernel: additions on the longest path of one entry.  Thread (e, s) adds partials s, s + 16, ... into four rotating
    accumulators (the first 512 partials) and the rest into the first: at most ceil(nparts / 16) additions on one accumulator; then
    (s0 + s1) + (s2 + s3): 2; then the pairwise tree over sixteen s-sums: 4."""
    return -(-nparts // 16) + 6


def gram_path_narrow(m, nwaves=None):
    """gram_f64_kernel: a wave owns ceil(nch / nwaves) chunks of 64 rows (interleaved); every row is one term of an MFMA chain
    (v_mfma_f64_16x16x4_f64: four terms a step, each counted as a product rounding plus an addition whether the unit fuses or not);
    the workgroup sum adds the four waves in two levels; the reduction sums the workgroups' partials (reduce_depth)."""
    nch = -(-m // 64)
    if nwaves is None:
        cpw = max(1, -(-nch // 2048))
        nwaves = -(-nch // cpw)
    chunks = -(-nch // nwaves)
    return 64 * chunks + 1 + 2 + reduce_depth((nwaves + 3) // 4)


def gram_path_wide(nch, cps):
    """gram_wide_f64_kernel: a wave owns one slice of cps chunks of 16 rows; the slices' partials go through the reduction"""
    return 16 * cps + 1 + reduce_depth(-(-nch // cps))


def gram_bound(a, path):
    """per entry |dG_ij| <= gamma_path sum_k |a_ki a_kj| (Higham, Accuracy and Stability, section 3.1: any order of `path` roundings)"""
    aa = np.abs(a)
    return gamma(path) * (aa.T @ aa)


# v_rsq_f64: "Precision is (2**29) ULP" (AMD Instinct MI300 / CDNA3 instruction set architecture reference guide, V_RSQ_F64; the same
# statement in the Vega and CDNA1/2 guides): a relative error of at most 2^29 2^-52 = 2^-23.
E0_RSQ = 2.0 ** -23
# One Newton step y' = y + (y / 2)(1 - p y^2) on y = (1 + e) / sqrt(p) leaves -(3/2) e^2 - e^3 / 2; as chol_section4 evaluates it,
# fma(0.5 y, fma(-fl(p y), y, 1), y): fl(p y) perturbs the residual by u (half of it reaches y'), the inner fma rounds a quantity of size
# <= 3 e0 (negligible), the outer fma rounds once: e_rsq <= 1.5 e0^2 + 2 u = 2.15e-14, about 190 u.
E_RSQ = 1.5 * E0_RSQ ** 2 + 2 * U


def chol_bounds(r, z, n):
    """chol_body16 in fp64 on an n x n block.  Row k of R is (row k of the Schur complement) * y_k and r_kk = p_k y_k, with
    y_k = (1 + d_k) / sqrt(p_k), |d_k| <= e_rsq; the trailing update uses the computed rows, so column sums telescope as in any
    Cholesky (gamma_(n+1): at most n - 1 fused updates, one scaling) except for term k = i of entry (i, j): r_ii r_ij = (1 + d_i)^2 g'_ij.
        |G - R^T R| <= (gamma_(n+1) + 2 e_rsq) |R^T| |R|
    M = R^-T comes from the same row operations on the identity (forward substitution with y_k in place of 1 / r_kk = y_k (1 + d_k)^-2):
        |Z R - I| <= (gamma_(n+1) + 2 e_rsq) |Z| |R|.
    Returns the two bound matrices."""
    c = gamma(n + 1) + 2 * E_RSQ
    ar, az = np.abs(r), np.abs(z)
    return c * (ar.T @ ar), c * (az @ ar)


def pivot_error(r, z):
    """d_k from the outputs: z_kk = y_k and r_kk = p_k y_k, so z_kk r_kk = (1 + d_k)^2 up to two roundings"""
    require_longdouble()
    return np.asarray((np.diag(z).astype(LD) * np.diag(r).astype(LD) - 1) / 2, np.float64)


def chain_bounds(r, z, n):
    """The blocked right-looking chain (cholw_diag / row / update kernels), nb = ceil(n / 64) blocks, 64-term block products on the MFMA.
    Diagonal blocks are chol_bounds.  Off the diagonal R_kJ = Z_kk^T G'_kJ is a PRODUCT with the block inverse, not a solve:
        R_kk^T R_kJ - G'_kJ = (Z_kk R_kk - I)^T G'_kJ + R_kk^T dP,  |dP| <= gamma_64 |Z_kk^T| |G'_kJ|,
    and with |G'_kJ| <= |R_kk^T| |R_kJ| (1 + small):
        |G - R^T R|_(I,J) <= gamma_(n + nb + 1) (|R^T| |R|)_(I,J)  [the Schur updates: (I) block products of 64 terms, each subtracted]
                             + (2 gamma_65 + 2 e_rsq) |R_II^T| |Z_II^T| |R_II^T| |R_IJ|            (I < J)
                             + (gamma_65 + 2 e_rsq) |R_II^T| |R_II|                                 (I = J).
    Z_Ik = -T_Ik Z_kk with T_Ik = sum_K Z_IK R_Kk accumulated over the steps:
        (Z R)_Ik = T_Ik (I - Z_kk R_kk) + rounding of T (gamma_(n + nb)) and of the product (gamma_64 |T_Ik| |Z_kk| |R_kk|), |T| <= |Z| |R|:
        |Z R - I|_(I,k) <= gamma_(n + nb + 1) (|Z| |R|)_(I,k) + (2 gamma_65 + 2 e_rsq) (|Z| |R|)_(I,k)^- |Z_kk| |R_kk|        (I < k)
    where ^- leaves block K = k out of the product.  First order; a factor 1.01 covers the rest.  r, z: n x n."""
    nb = nblocks(n)
    ar, az = np.abs(r), np.abs(z)
    c0 = gamma(n + nb + 1)
    c1 = 2 * gamma(65) + 2 * E_RSQ
    bg = c0 * (ar.T @ ar)
    bz = c0 * (az @ ar)
    for k in range(nb):
        s = slice(64 * k, min(n, 64 * k + 64))
        rkk, zkk = ar[s, s], az[s, s]
        bg[s, s] += (gamma(65) + 2 * E_RSQ) * (rkk.T @ rkk)
        bz[s, s] += (gamma(65) + 2 * E_RSQ) * (zkk @ rkk)
        if 64 * k + 64 < n:
            t = slice(64 * k + 64, n)
            bg[s, t] += c1 * (rkk.T @ zkk.T @ rkk.T @ ar[s, t])
        if k > 0:
            up = slice(0, 64 * k)
            bz[up, s] += c1 * ((az[up, up] @ ar[up, s]) @ zkk @ rkk)
    bg = np.triu(bg) + np.triu(bg, 1).T
    return 1.01 * bg, 1.01 * bz


def apply_bound(a, z):
    """Q = A Z on the fp64 MFMA: entry (r, j) is a chain of at most n products (zero blocks of Z skipped): gamma_(n+1) |A| |Z|"""
    return gamma(a.shape[1] + 1) * (np.abs(a) @ np.abs(z))


def rmul_bound(r2, r1):
    """R2 R1: each entry a chain of at most n fp64 products (wide: block sums added once more): gamma_(n + nb + 1) |R2| |R1|"""
    n = r1.shape[0]
    return gamma(n + nblocks(n) + 1) * (np.abs(r2) @ np.abs(r1))


# ---- numpy models of the passes, with the defects the tests must catch ------------------------------------------------------------------
def model_gram(a, chunk=64, defect=None):
    """fp64 model of a Gram pass: chunks of `chunk` rows summed in order.  defects: 'tail' drops the rows of the ragged last chunk,
    'fp32' rounds one chunk's partial to fp32"""
    m, n = a.shape
    g = np.zeros((n, n))
    nch = -(-m // chunk)
    for ch in range(nch):
        rows = a[ch * chunk: min(m, ch * chunk + chunk)]
        if defect == "tail" and rows.shape[0] < chunk:
            continue
        part = rows.T @ rows
        if defect == "fp32" and ch == nch // 2:
            part = part.astype(np.float32).astype(np.float64)
        g += part
    return g


def model_chol(g, newton=True, seed_err=E0_RSQ, shift=0.0, nreal=None):
    """fp64 model of chol_body16: rows scaled by y = rsq(pivot); newton=False keeps a seed of relative error seed_err (the defect).
    shift is added to the diagonal entries < nreal (a defect when nreal exceeds the true column count).  Returns R, Z."""
    n = g.shape[0]
    a = g.copy()
    nreal = n if nreal is None else nreal
    a[np.arange(nreal), np.arange(nreal)] += shift
    r = np.zeros((n, n))
    m = np.eye(n)
    for k in range(n):
        if a[k, k] == 0.0 and not np.any(a[k]):              # a padded row (columns >= the real count): not live, R and Z rows stay zero
            m[k] = 0.0
            continue
        y = 1.0 / np.sqrt(a[k, k])
        if not newton:
            y *= 1.0 + seed_err * (1 if k % 2 else -1)
        r[k, k:] = a[k, k:] * y
        m[k] = m[k] * y
        lk = r[k, k + 1:]
        a[k + 1:, k + 1:] -= np.outer(lk, r[k, k + 1:])
        m[k + 1:] -= np.outer(lk, m[k])
    return r, m.T


def padding_is_zero(x, n):
    """rows and columns >= n of a block-padded n x n quantity are exact zeros (what the block store promises for R and Z)"""
    return bool(np.all(x[n:, :] == 0) and np.all(x[:, n:] == 0))


def model_s(g, z, nb_offdiag=True):
    """S = sum_ij g_ii z_ij^2 / n summed per 64 x 64 block pair; nb_offdiag=False drops the off-diagonal block pairs (the defect)"""
    n = g.shape[0]
    t = np.diag(g)[:, None] * z * z
    if not nb_offdiag:
        keep = (np.arange(n)[:, None] // 64) == (np.arange(n)[None, :] // 64)
        t = t * keep
    return float(np.sum(t) / n)


# ---- the shift ------------------------------------------------------------------------------------------------------------------------------
def shift_residual(g, s, r, nreal=None):
    """|G + s I_(< nreal) - R^T R| in longdouble: the backward residual of the shifted factorisation.  s = shift_coef trace(G) is about
    1e-8 n times a diagonal entry while the bounds of chol_bounds / chain_bounds are about 1e-13 times it, so a wrong coefficient, a
    trace over part of the diagonal, or a shift that misses some diagonal entries shows on the diagonal at 1e4 times the bound and more."""
    require_longdouble()
    n = g.shape[0]
    nreal = n if nreal is None else nreal
    gs = np.array(g, dtype=LD)
    gs[np.arange(nreal), np.arange(nreal)] += LD(s)
    return np.asarray(np.abs(gs - matmul_ld(r.T, r)), np.float64)


# ---- matrices with a prescribed scaled conditioning (the ladder tests through the public entries) ------------------------------------------
def s_of(b):
    """S_ref = mean(1 / sigma_i(B D^-1)^2), D the column norms of B: ||D inverse(R)||_F^2 / n of B's R factor"""
    sv = np.linalg.svd(b / np.linalg.norm(b, axis=0), compute_uv=False)
    return float(np.mean(1.0 / sv ** 2))


def ladder_matrix(m, n, s_target, seed):
    """m x n matrix A = U diag(sigma) V^T, sigma geometric from 1 to 1 / c, with c found by bisection so that S_ref(A) = s_target
    (relative 1e-6).  U has orthonormal columns, so S_ref(A) = S_ref(diag(sigma) V^T): the search runs on n x n matrices.
    Returns (A, S_ref of the n x n core)."""
    assert s_target > 1.0
    rng = np.random.default_rng(seed)
    u, _ = np.linalg.qr(rng.standard_normal((m, n)))
    v, _ = np.linalg.qr(rng.standard_normal((n, n)))
    core = lambda logc: np.geomspace(1.0, 10.0 ** -logc, n)[:, None] * v.T
    lo, hi = 0.0, 1.0
    while s_of(core(hi)) < s_target:
        hi *= 2.0
        assert hi <= 16.0, "S target out of reach in fp64"
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if s_of(core(mid)) < s_target:
            lo = mid
        else:
            hi = mid
    b = core(0.5 * (lo + hi))
    s = s_of(b)
    assert abs(s - s_target) <= 1e-6 * s_target, (s, s_target)
    return u @ b, s


LADDER = (("alone_max / 2", 1, 2), ("2 alone_max", 2, 2), ("max_scond / 4", 2, 2), ("4 max_scond", 103, 103))


def ladder_targets(m, n):
    """S_ref on both sides of both thresholds of rule(m, n) with the margins 2 and 4, and the sweep counts of the header
    (reorth = 0, reorth = 1): one sweep below alone_max, CholeskyQR2 up to max_scond, shifted CholeskyQR3 (103) beyond"""
    mx, al, _ = rule(m, n)
    assert 2 * al < mx / 4, "the thresholds are too close for four separate cases"
    return [(name, t, s0, s1) for (name, s0, s1), t in zip(LADDER, (al / 2, 2 * al, mx / 4, 4 * mx))]

"""Pure-numpy references for the per-pass tests (tests/test_gpu_passes.py): the Gram-tile layouts, the exact-data generators with
their bit budgets, and the error bounds of each pass.  No GPU, no library: tests/test_pass_refs.py checks all of it on the CPU.

Notation: u = 2^-24 (fp32 unit roundoff), u64 = 2^-53, u16 = 2^-11; |X| is the entrywise absolute value."""
import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53
U16 = 2.0 ** -11
KSTEP = 32                      # rows of one fp32 MFMA chain of the bf16-split Gram pass (gram_bf16_kernel / gram_blk_kernel)


# ---- Gram tiles ---------------------------------------------------------------------------------------------------------------------
def ntiles(n):
    return (n + 15) // 16


def gram_elems(n):
    """doubles of the summed tiles (tsqr_mi_gram_elems): upper-triangle tile pairs x 256"""
    nt = ntiles(n)
    return nt * (nt + 1) // 2 * 256


def _tile_index(n, f32_layout):
    """(row, column) of every element of the tile array: tile pairs (ti <= tj) in order, then (reg, lane) -- the MFMA accumulator order
    (f32 C/D layout: row = 4 (lane >> 4) + reg; f64: row = (lane >> 4) + 4 reg; column = lane & 15)"""
    lanes = np.arange(64)
    rows, cols = [], []
    nt = ntiles(n)
    for ti in range(nt):
        for tj in range(ti, nt):
            for reg in range(4):
                r = (4 * (lanes >> 4) + reg) if f32_layout else ((lanes >> 4) + 4 * reg)
                rows.append(16 * ti + r)
                cols.append(16 * tj + (lanes & 15))
    return np.concatenate(rows), np.concatenate(cols)


def pack_tiles(g, n, f32_layout):
    """n x n matrix -> tile array (what a Gram kernel leaves in gsum); the diagonal tiles carry both triangles, entries beyond n are 0"""
    np_ = 16 * ntiles(n)
    gp = np.zeros((np_, np_))
    gp[:n, :n] = g
    r, c = _tile_index(n, f32_layout)
    return gp[r, c]


def unpack_tiles(v, n, f32_layout):
    """tile array -> NP x NP matrix (NP = 16 ceil(n / 16)).  The tiles on and above the diagonal are taken as they are (both triangles
    of a diagonal tile: an MFMA accumulator computes both), the tiles below the diagonal are the transposes of their mirrors."""
    v = np.asarray(v)
    assert v.shape == (gram_elems(n),)
    np_ = 16 * ntiles(n)
    g = np.full((np_, np_), np.nan)
    r, c = _tile_index(n, f32_layout)
    g[r, c] = v
    low = (r // 16) != (c // 16)
    g[c[low], r[low]] = v[low]
    return g


# ---- exact-data generators ----------------------------------------------------------------------------------------------------------
def int_bits(kmax):
    """significant bits of the integers |k| <= kmax"""
    return int(kmax).bit_length()


def gram_exact_budget(kmax, m, chain=KSTEP):
    """A = k 2^e with integer |k| <= kmax (one exponent per column): every product a_ki a_kj is an integer of at most 2 int_bits(kmax)
    bits times 2^(e_i + e_j).  The bf16-split pass sums `chain` products of a column pair in one fp32 MFMA chain and the chain results
    in fp64; the fp64 pass sums all m in fp64.  Every partial sum is then an integer multiple of 2^(e_i + e_j), and it is exact when
    its magnitude stays below 2^24 (fp32 chain) / 2^53 (fp64 totals).  Returns (chain bits, total bits) of the integer sums: exact
    Gram matrices in ANY summation order need chain bits <= 24 and total bits <= 53."""
    chain_max = chain * kmax * kmax
    total_max = max(m, 1) * kmax * kmax
    return int(chain_max).bit_length(), int(total_max).bit_length()


def exact_ints(rng, m, n, kmax=511, exps=(-3, 3)):
    """float32 m x n, entries k 2^e_j: |k| <= kmax, most of them with all int_bits(kmax) bits (for kmax = 511: nine bits, so that the
    bf16 split has a non-zero mid part and the hm / mh / mm products take part), some zeros; e_j per column in [exps]"""
    top = 1 << (int_bits(kmax) - 1)
    k = rng.integers(top, kmax + 1, size=(m, n))
    k = np.where(rng.random((m, n)) < 0.2, rng.integers(-kmax, kmax + 1, size=(m, n)), k)
    k *= rng.choice(np.array([-1, 1]), size=(m, n))
    e = rng.integers(exps[0], exps[1] + 1, size=n)
    return (k * np.exp2(e)[None, :]).astype(np.float32)


def full_mantissa(rng, size, spread=20):
    """float32 values with all 24 significand bits in use (lowest bit set) and exponents uniform in [-spread, spread], random sign"""
    mant = rng.integers(1 << 23, 1 << 24, size=size) | 1
    e = rng.integers(-spread, spread + 1, size=size)
    s = rng.choice(np.array([-1.0, 1.0]), size=size)
    return (s * mant * np.exp2(e - 23.0)).astype(np.float32)


def isolated_rows(rng, m, n, stretch=64, spread=20):
    """float32 m x n, zero except ONE row per `stretch`-row stretch (rows [stretch s, stretch s + stretch)) -- so no 32-row K-step
    holds two non-zero rows and every fp32 MFMA chain of the bf16-split pass carries one product per entry; full mantissas"""
    a = np.zeros((m, n), np.float32)
    starts = np.arange(0, m, stretch)
    rows = starts + rng.integers(0, stretch, size=starts.size)
    rows = np.minimum(rows, m - 1)
    a[rows, :] = full_mantissa(rng, (rows.size, n), spread)
    return a


def single_entry_rows(rng, m, n, spread=6):
    """float32 m x n with exactly one non-zero (full mantissa) per row, in a random column: every entry of A Z is ONE product a z"""
    a = np.zeros((m, n), np.float32)
    cols = rng.integers(0, n, size=m)
    a[np.arange(m), cols] = full_mantissa(rng, m, spread)
    return a


def exact_inverse_pair(rng, n, split, bmax=63, scale_exp=2, b_full=False):
    """R = D [[I, B], [0, I]] (blocks split after `split` rows / columns, D = diag of powers of two, 2^-scale_exp .. 2^scale_exp) and
    its EXACT inverse [[I, -B], [0, I]] D^-1.  B: integers |b| <= bmax (b_full: full-mantissa fp32 values instead).  Returns float32 R
    and float64 Z (Z is representable in fp32: every entry is -b_ij / d_i, 1 / d_i or 0)."""
    b = (full_mantissa(rng, (split, n - split), spread=3).astype(np.float64) if b_full
         else rng.integers(-bmax, bmax + 1, size=(split, n - split)).astype(np.float64))
    d = np.exp2(rng.integers(-scale_exp, scale_exp + 1, size=n).astype(np.float64))
    u = np.eye(n)
    u[:split, split:] = b
    zi = np.eye(n)
    zi[:split, split:] = -b
    r = d[:, None] * u
    z = zi / d[None, :]
    assert np.array_equal(r @ z, np.eye(n))
    return r.astype(np.float32), z


def random_triangular(rng, n, cond):
    """float32 upper-triangular n x n with 2-norm condition number near `cond` (R factor of a matrix with geometric singular values)"""
    mm = max(2 * n, 8)
    x = rng.standard_normal((mm, n))
    uu, _, vt = np.linalg.svd(x, full_matrices=False)
    a = (uu * np.geomspace(1.0, 1.0 / cond, n)) @ vt
    r = np.linalg.qr(a, mode="r")
    return r.astype(np.float32)


# ---- bounds ---------------------------------------------------------------------------------------------------------------------------
C_SPLIT_PRODUCT = 10.0


def gram_l2_isolated_bound(a):
    """Level 2 (bf16 split, six products, fp32 chain per 32-row K-step, fp64 totals) on isolated_rows() data, per entry:
        |dG_ij| <= 10 u sum_k |a_ki a_kj| + (m / 32 + 64) u64 sum_k |a_ki a_kj|.
    Derivation, for one product x = a b of one chain: a = h + m + l exactly (RNE bf16 split of a normal fp32: |m| <= 2^-8 |a|,
    |l| <= 2^-16 |a|; allow 2u for a split that is not exact); the six bf16 products are exact in fp32; the three dropped ones,
    ml + lm + ll, are <= (2 2^-24 + 2^-32) |x|; the chain starts from zero and makes five fp32 additions, each <= u (1 + 2^-6) |x|
    (every partial sum is below (1 + 2^-6) |x|).  2.01 + 2 + 5.1 < 10.  The chain results then go into fp64 totals and a fixed tree
    of fp64 sums: fewer than m / 32 + 64 additions on any path, each <= u64 times the sum of magnitudes."""
    aa = np.abs(a.astype(np.float64))
    s = aa.T @ aa
    return (C_SPLIT_PRODUCT * U32 + (a.shape[0] / KSTEP + 64) * U64) * s


def gram_l2_dense_bound(a):
    """Level 2 on dense data, normwise: ||dG||_F <= (4 + 6 * 32) u || |A|^T |A| ||_F + (m / 32 + 64) u64 (same).
    Per chain of a column pair: 32 rows x 6 products = 192 terms added in fp32 in some order (gamma_192 <= 192 u (1 + small)) plus the
    split and dropped terms (<= 4 u per product), on |a_ki a_kj|; the fp64 totals as in gram_l2_isolated_bound."""
    aa = np.abs(a.astype(np.float64))
    s = np.linalg.norm(aa.T @ aa)
    return ((4 + 6 * KSTEP) * U32 * 1.01 + (a.shape[0] / KSTEP + 64) * U64) * s


def gram_l1_bound(a):
    """Level 1 (fp64 MFMA, fp64 totals), per entry: the products of two fp32 values are exact in fp64; every entry is a sum of m
    products formed through MFMA chains, an LDS tree and the fixed reduction tree -- fewer than m + 64 additions on any path, so
    |dG_ij| <= (m + 64) u64 sum_k |a_ki a_kj| (first order; m u64 << 1 here)."""
    aa = np.abs(a.astype(np.float64))
    return (a.shape[0] + 64) * U64 * 1.01 * (aa.T @ aa)


C_ENGINE1 = 8.0


def apply_single_product_bound(engine, q_exact):
    """One product per entry (single_entry_rows A, any Z), relative to |a z|:
      engine 0 (exact fp32 FMA chain): the one non-zero product is rounded once and zeros add exactly -> 0 (bit-exact fl32(a z));
      engine 1 (bf16x3, six products): as gram_l2_isolated_bound for one chain but the split of both operands is exact (normal fp32):
        dropped terms 2.01 u + five fp32 additions 5.1 u < 8 u;
      engine 2 (fp16 operands, one product): fl16(a) fl16(z) = a z (1 + d1)(1 + d2), |d| <= u16 = 2^-11, the product is exact in fp32
        (11 + 11 bits), the chain adds zeros: <= (2 u16 + u16^2) |a z| + u for the final fp32 rounding (operands in the fp16 normal
        range)."""
    q = np.abs(q_exact)
    if engine == 0:
        return np.zeros_like(q)
    if engine == 1:
        return C_ENGINE1 * U32 * q
    return (2 * U16 + U16 * U16 + U32) * q


def apply_general_bound(engine, a, z, cond):
    """Q = A Z with Z = inverse(R) formed by trinv_kernel (fp64, rounded to fp32) and the engine's product, normwise against the fp64
    product with the exact inverse of the fp32 R:
      Z: fp64 elimination (<= n cond u64 |Z| to first order) + one rounding to fp32 (u |Z|);
      product: engine 0 an fp32 FMA chain of n terms (gamma_n), engine 1 the same with < 8 u per product (apply_single_product_bound),
      engine 2 fp16 operands (2 u16 + u16^2 per product, up to n u of fp32 chain, and 2^-25 per |a| for a z entry below the fp16
      normal range);
    so ||dQ||_F <= c_e || |A| |Z| ||_F (+ the fp16 underflow term), c_0 = (n + 1) u + n cond u64, c_1 = c_0 + 8 u, c_2 = 2 u16 + ...,
    times 1.01 for the second-order terms."""
    n = a.shape[1]
    aa, zz = np.abs(a.astype(np.float64)), np.abs(z)
    s = np.linalg.norm(aa @ zz)
    c = (n + 1) * U32 + n * cond * U64
    if engine == 1:
        c += C_ENGINE1 * U32
    if engine == 2:
        c += 2 * U16 + U16 * U16
        return 1.01 * c * s + 2.0 ** -25 * n * np.linalg.norm(aa)
    return 1.01 * c * s


def ulp32(x):
    """spacing of fp32 at |x| (one unit in the last place of the fp32 value nearest to x)"""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def rmul_bound(r2, r1):
    """R2 R1 with fp64 accumulation, rounded once to fp32, per entry:
        |P - P_exact| <= 1/2 ulp32(P_exact) (the final rounding) + n u64 sum_k |r2_ik r1_kj| (the fp64 sums: products of two fp32
    values are exact in fp64).  The reference P64 (numpy fp64 matmul) carries the same n u64 term, and ulp32(P64) can be one binade
    smaller than ulp32(P_exact), so against P64: <= ulp32(P64) + 2 n u64 sum_k |r2_ik r1_kj| -- "within 1 fp32 ulp", with room for
    the summation error of both sides.  Any fp32 accumulation leaves ulps after a few terms."""
    n = r1.shape[0]
    p = r2.astype(np.float64) @ r1.astype(np.float64)
    s = np.abs(r2.astype(np.float64)) @ np.abs(r1.astype(np.float64))
    return ulp32(p) + 2 * n * U64 * s


C_HOUSEHOLDER = 8.0


def local_r_backward_bound(a):
    """Householder TSQR is backward stable: R is the exact R factor of A + dA with ||dA||_F <= c n u ||A||_F (fp32 reflectors applied
    to <= 64 + NP rows per fold, errors of the folds along a chain and the tree adding up in norm), so
    ||R^T R - A^T A||_F = ||A^T dA + dA^T A + dA^T dA||_F <= (2 c n u + (c n u)^2) ||A||_F^2, c = 8 -- independent of cond(A)."""
    n = a.shape[1]
    e = C_HOUSEHOLDER * n * U32
    return (2 * e + e * e) * np.linalg.norm(a.astype(np.float64)) ** 2


def local_r_forward_bound(a, cond):
    """Sign-normalised R against LAPACK's fp64 R: the perturbation of the R factor under dA is ||dR||_F <= sqrt(2) cond(A) ||dA||_F
    (first order), with ||dA||_F from local_r_backward_bound and LAPACK's own error (fp64) negligible"""
    n = a.shape[1]
    return np.sqrt(2) * 1.01 * max(cond, 1.0) * C_HOUSEHOLDER * n * U32 * np.linalg.norm(a.astype(np.float64))


# =========================================================================================================================================
# The one-panel path, 64 < n <= 128 (tsqr_wide.hip): gram_wide_kernel, chol_wide_kernel, the apply_wide instances
# =========================================================================================================================================
WIDE_TILES = 36
WIDE_ELEMS = WIDE_TILES * 256


def _tri4(ti, tj):
    return ti * 4 - (ti * (ti - 1)) // 2 + (tj - ti)


def wide_tile(ti, tj):
    """destination of the tile pair (ti <= tj) of a 128 x 128 Gram matrix (wide_tile, tsqr_wide.hip):
    [G11: 10 tiles in the NT = 4 triangle order][G22: 10 tiles, the same order][G12: 16 tiles row-major]"""
    assert 0 <= ti <= tj < 8
    if tj < 4:
        return _tri4(ti, tj)
    return 10 + _tri4(ti - 4, tj - 4) if ti >= 4 else 20 + ti * 4 + (tj - 4)


def _wide_index():
    """(row, column) of every element of the 36-tile array: element (reg, lane) of a tile sits at tile * 256 + reg * 64 + lane and is
    G[16 ti + 4 (lane >> 4) + reg][16 tj + (lane & 15)] -- the f32 MFMA accumulator layout (gram_wide_body stores acc[t][r] of lane l at
    (dst * 4 + r) * 64 + l; chol_wide_kernel reads the diagonal at reg = c & 3, lane = 16 (c >> 2) + c)"""
    lanes = np.arange(64)
    rows = np.zeros(WIDE_ELEMS, np.int64)
    cols = np.zeros(WIDE_ELEMS, np.int64)
    for ti in range(8):
        for tj in range(ti, 8):
            t = wide_tile(ti, tj)
            for reg in range(4):
                sl = slice(t * 256 + reg * 64, t * 256 + reg * 64 + 64)
                rows[sl] = 16 * ti + 4 * (lanes >> 4) + reg
                cols[sl] = 16 * tj + (lanes & 15)
    return rows, cols


def pack_wide_tiles(g, n):
    """n x n matrix (64 < n <= 128) -> the 36 x 256 doubles gram_wide_kernel + the reduction leave: tiles on and above the diagonal,
    both triangles of a diagonal tile, entries beyond n zero"""
    assert 64 < n <= 128 and g.shape == (n, n)
    gp = np.zeros((128, 128))
    gp[:n, :n] = g
    r, c = _wide_index()
    return gp[r, c]


def unpack_wide_tiles(v):
    """36 x 256 doubles -> 128 x 128 matrix; tiles below the diagonal are the transposes of their mirrors"""
    v = np.asarray(v)
    assert v.shape == (WIDE_ELEMS,)
    g = np.full((128, 128), np.nan)
    r, c = _wide_index()
    g[r, c] = v
    low = (r // 16) != (c // 16)
    g[c[low], r[low]] = v[low]
    return g


def exact_wide_pair(rng, n, split, k=3, col_budget=24):
    """The 128-column exact inverse pair for the factorisation AND the apply pass: R = 2^k [[I, B], [0, I]] (B: split x (n - split), the
    split anywhere in 1 .. n - 1: inside the first 64-column block, on column 64 or inside the second block), Z = 2^-k [[I, -B], [0, I]],
    G = R^T R = 4^k [[I, B], [B^T, I + B^T B]].  B holds integers |b| <= 2 with sum_i b_ij^2 <= col_budget per column, so that
      * every fp64 operation of a Cholesky factorisation of G by rows is exact (integers below 2^53 times powers of two; pivots are
        powers of four, whose reciprocal square roots are powers of two),
      * the verdict of chol_wide_kernel is known in closed form: the smallest pivot ratio r_jj^2 / g_jj = 1 / (1 + max_j sum_i b_ij^2)
        (> 2^-5 for col_budget <= 30) and S = ||D Z||_F^2 / n with D = diag(sqrt(g_jj)) = 1 + 2 ||B||_F^2 / n.
    Returns float64 (R, Z, G, B)."""
    assert 0 < split < n
    b = rng.integers(-2, 3, size=(split, n - split)).astype(np.float64)
    b[rng.random(b.shape) < 0.5] = 0.0
    for j in range(b.shape[1]):
        while np.sum(b[:, j] ** 2) > col_budget:
            nz = np.flatnonzero(b[:, j])
            b[rng.choice(nz), j] = 0.0
    return wide_pair_from_b(b, n, k) + (b,)


def wide_pair_from_b(b, n, k=3):
    """(R, Z, G) of exact_wide_pair for a given integer block B (split = its row count)"""
    split = b.shape[0]
    assert b.shape == (split, n - split)
    u = np.eye(n)
    u[:split, split:] = b
    zi = np.eye(n)
    zi[:split, split:] = -b
    r = u * 2.0 ** k
    z = zi * 2.0 ** -k
    g = r.T @ r
    assert np.array_equal(r @ z, np.eye(n)) and np.array_equal(z.T @ g @ z, np.eye(n))
    return r, z, g


def exact_wide_verdict(b, n):
    """(smallest pivot ratio, S) of exact_wide_pair's G in closed form (see there)"""
    return 1.0 / (1.0 + float(np.max(np.sum(b * b, axis=0)))), 1.0 + 2.0 * float(np.sum(b * b)) / n


def wide_scond_threshold(rows, floor=4.0):
    """the bound on S of the bf16-split level as chol_wide_kernel evaluates it (fp32): min(128, max(floor, 0.12 sqrt(rows)))"""
    f = np.float32
    return float(min(f(128.0), max(f(floor), f(0.12) * np.sqrt(f(rows)))))


def zw_of(z, n):
    """n x n Z -> the 128 x 128 fp32 operand of the apply_wide instances as chol_wide_kernel leaves it: zw[K * 128 + j] = Z[j][K] (column
    K of Z contiguous, ld 128), zero beyond n"""
    zp = np.zeros((128, 128), np.float32)
    zp[:n, :n] = z
    return np.ascontiguousarray(zp.T).reshape(-1)


def apply_wide_exact_budget(amax, bmax, split, k):
    """Q = A Z, A integers |a| <= amax, Z = 2^-k [[I, -B], [0, I]], |b| <= bmax: every product is an integer times 2^-k and a column of Q
    sums at most split + 1 of them, |q| 2^k <= amax (1 + split bmax).  Exact in every engine when the operands are exact in bf16 and fp16
    (amax, bmax < 2^8 .. 2^11: asserted as <= 255) and every partial sum stays below 2^24 units (fp32 accumulators; the bf16x3 engine's
    mid / low images of such operands are zero).  Returns the bits of the largest partial sum."""
    assert amax <= 255 and bmax <= 255
    return int(amax * (1 + split * bmax)).bit_length()


# ---- chol_wide_kernel against a longdouble factorisation --------------------------------------------------------------------------------
def _up(x):
    """upper triangle with half the diagonal: the first-order map dG -> dR R^-1 of the Cholesky factor (dR = up(Z^T dG Z) R)"""
    return np.triu(x, 1) + 0.5 * np.diag(np.diag(x))


def chol_wide_bounds(r, z, n):
    """Entrywise bounds on |R_gpu - R|, |Z_gpu - Z| for chol_wide_kernel, R = chol(G) and Z = inverse(R) of the SAME doubles in longdouble
    (passed here rounded to float64), n1 = 64, n2 = n - 64.  Form: half an fp32 ulp (the one rounding on the way out) plus an fp64 term.

    The fp64 term follows the kernel block by block; u = 2^-53, g_k = k u / (1 - k u), e = pass_refs_f64.E_RSQ (the v_rsq_f64 + Newton pivot
    scaling), c = g_65 + 2 e (pass_refs_f64.chol_bounds for a 64-column block: |G - R^T R| <= c |R^T| |R|, |Z R - I| <= c |Z| |R|):
      F11 = up(|Z11^T| c |R11^T| |R11| |Z11|) |R11|                       first-order perturbation of a Cholesky factor under dG
      H11 = |Z11| F11 |Z11| + c |Z11| |R11| |Z11|                         its inverse: the factor's error plus the inverse's residual
      F12 = H11^T |G12| + g_65 |Z11^T| |G12|                              R12 = Z11^T G12 is a 64-term fp64 MFMA product with the inverse
      E22 = 2 F12^T |R12| + g_66 (|G22| + |R12^T| |R12|)                  G22' = G22 - R12^T R12 (64-term product, one subtraction)
      F22 = up(|Z22^T| (E22 + c |R22^T| |R22|) |Z22|) |R22|,  H22 as H11
      dT  = F12 |Z22| + |R12| H22 + g_65 |R12| |Z22|                      T = R12 Z22
      H12 = H11 |T| + |Z11| dT + g_65 |Z11| |T|                           Z12 = -Z11 T
    each times 1.1 for the second-order terms.  Dependence on n and on the conditioning: every term is c or g_65 (about 65 u .. 500 u:
    the block size, not n) times chained products of |R| and |Z| factors, a worst case that grows far faster than cond_2(G): measured
    on the NumPy model (tests/test_pass_refs.py), the fp64 term stays below 0.05 ulp32 on the entries of R that are not tiny at
    cond(A) = 2, passes one ulp from cond(A) of about 4 at n = 128, and still separates the fp64 arithmetic from an fp32 Schur complement
    or Z12 (n2 u32 |R12^T| |R12| in G22') by a factor of 8 .. 800 up to cond(A) = 30.  That is the conditioning this bound covers
    (WIDE_CHOL_GENERAL).  It does NOT cover cond(A) = 1e3: there even the normwise first-order bound of an fp64 Cholesky factor,
    ||dR||_F <= 2^-1/2 cond_2(G) eps ||R||_2 with eps = c n for the backward error (Higham, Accuracy and Stability, theorem 10.8),
    is 0.7 x 1e6 x 128 x 5.8e-14 = 5e-6 ||R||_2, eighty times the fp32 rounding 2^-24 -- no rigorous bound tells fp64 from fp32 there, and
    at cond(A) = 1e2 it is 5e-8 ||R||_2, level with it.  Returns (bound on R, bound on Z), n x n each."""
    from tests import pass_refs_f64 as p64
    n1, n2 = 64, n - 64
    r = np.asarray(r, np.float64)
    z = np.asarray(z, np.float64)
    ar, az = np.abs(r), np.abs(z)
    r11, r12, r22 = ar[:n1, :n1], ar[:n1, n1:], ar[n1:, n1:]
    z11, z22 = az[:n1, :n1], az[n1:, n1:]
    g = ar.T @ ar                                           # >= |G| entrywise (G = R^T R)
    g12, g22 = g[:n1, n1:], g[n1:, n1:]
    c = p64.gamma(65) + 2 * p64.E_RSQ
    g65, g66 = p64.gamma(65), p64.gamma(66)
    f11 = _up(z11.T @ (c * (r11.T @ r11)) @ z11) @ r11
    h11 = z11 @ f11 @ z11 + c * (z11 @ r11 @ z11)
    f12 = h11.T @ g12 + g65 * (z11.T @ g12)
    e22 = 2 * (f12.T @ r12) + g66 * (g22 + r12.T @ r12)
    f22 = _up(z22.T @ (e22 + c * (r22.T @ r22)) @ z22) @ r22
    h22 = z22 @ f22 @ z22 + c * (z22 @ r22 @ z22)
    t = r12 @ z22
    dt = f12 @ z22 + r12 @ h22 + g65 * (r12 @ z22)
    h12 = h11 @ t + z11 @ dt + g65 * (z11 @ t)
    fr = np.zeros((n, n))
    fz = np.zeros((n, n))
    fr[:n1, :n1], fr[:n1, n1:], fr[n1:, n1:] = f11, f12, f22
    fz[:n1, :n1], fz[:n1, n1:], fz[n1:, n1:] = h11, h12, h22
    fr *= 1.1
    fz *= 1.1
    return 0.5 * ulp32(ar + fr) + fr, 0.5 * ulp32(az + fz) + fz


def model_chol_wide(g, n, schur32=False, z12_32=False):
    """NumPy emulation of chol_wide_kernel's intended arithmetic on the n x n fp64 matrix g: fp64 Cholesky of G11 by rows, Z11 by
    substitution, R12 = Z11^T G12, G22' = G22 - R12^T R12, the second block likewise, Z12 = -Z11 (R12 Z22), all in fp64, R and Z rounded
    once to fp32.  schur32 / z12_32: the shortcut -- that product accumulated in fp32.  Returns float32 (R, Z)."""
    def chol_inv(a):
        a = np.array(a, np.float64)
        k = a.shape[0]
        rr = np.zeros((k, k))
        for i in range(k):
            y = 1.0 / np.sqrt(a[i, i])
            rr[i, i:] = a[i, i:] * y
            a[i + 1:, i + 1:] -= np.outer(rr[i, i + 1:], rr[i, i + 1:])
        return rr, np.linalg.solve(rr, np.eye(k))
    n1 = 64
    r11, z11 = chol_inv(g[:n1, :n1])
    r12 = z11.T @ g[:n1, n1:]
    if schur32:
        s = (r12.astype(np.float32).T @ r12.astype(np.float32)).astype(np.float64)
    else:
        s = r12.T @ r12
    r22, z22 = chol_inv(g[n1:, n1:] - s)
    if z12_32:
        z12 = -(z11.astype(np.float32) @ (r12 @ z22).astype(np.float32)).astype(np.float64)
    else:
        z12 = -z11 @ (r12 @ z22)
    r = np.zeros((n, n))
    z = np.zeros((n, n))
    r[:n1, :n1], r[:n1, n1:], r[n1:, n1:] = r11, r12, r22
    z[:n1, :n1], z[:n1, n1:], z[n1:, n1:] = np.triu(z11), z12, np.triu(z22)
    return r.astype(np.float32), z.astype(np.float32)


def well_conditioned(rng, m, n, cond):
    """float32 m x n with singular values geometric in [1 / cond, 1] and random singular vectors"""
    x = rng.standard_normal((m, n))
    uu, _, vt = np.linalg.svd(x, full_matrices=False)
    return ((uu * np.geomspace(1.0, 1.0 / cond, n)) @ vt).astype(np.float32)


# the shapes of tests/test_gpu_wide_passes.py (the budget assertions of tests/test_pass_refs.py run over the same lists)
WIDE_GRAM_M = [1, 63, 64, 65, 129, 193, 485]
WIDE_GRAM_N = [65, 80, 97, 113, 127, 128]
WIDE_CHOL_CASES = [(n, s) for n in (65, 80, 112, 128) for s in (50, 64, 80) if s < n]
# chol_wide_kernel against longdouble, (n, cond(A)): the conditioning chol_wide_bounds covers (its docstring: why not 1e3).  At every one
# of these the NumPy model with an fp32 Schur complement or Z12 misses the bound (tests/test_pass_refs.py); cond(A) = 1 (G = I, R12 = 0)
# would not see either.
WIDE_CHOL_GENERAL = [(128, 2.0), (80, 2.0), (128, 4.0), (128, 10.0), (80, 10.0), (128, 30.0)]
WIDE_APPLY_M = [1, 63, 65, 129, 323, 449]
WIDE_APPLY_N = [65, 80, 100, 113, 128]
WIDE_APPLY_SPLITS = [17, 64, 70, 100]


# =========================================================================================================================================
# Panel coupling (cross_kernel, cross_reduce_multi_kernel, cross_finish_kernel, the update instance) and the half-typed path
# =========================================================================================================================================
def cross_exact_budget(kmax, m, rows_per_wg):
    """X, Y integers |k| <= kmax.  cross_kernel keeps ONE fp32 MFMA chain per wave over all the rows of the wave (cpw chunks of 64 rows:
    not one 32-row K-step), and wg_sum4_store then adds the four waves of a workgroup in fp32; the workgroups' partials are summed in
    fp64.  Every fp32 partial sum is an integer, exact while the rows one workgroup sums (rows_per_wg = 4 x cpw x 64, from the plan entry)
    times kmax^2 stay below 2^24; the fp64 totals need m kmax^2 < 2^53.  Returns (workgroup bits, total bits): exact S needs <= 24, <= 53."""
    return int(min(m, rows_per_wg) * kmax * kmax).bit_length(), int(m * kmax * kmax).bit_length()


C_CROSS_ISOLATED = 14.1


def cross_isolated_bound(x, y, m, nblocks):
    """isolated_rows data with one non-zero row per wave's range (stretch = cpw x 64 rows, X and Y non-zero in the same rows): a wave's
    chain holds ONE product per entry -- 10 u as in gram_l2_isolated_bound --, three fp32 additions join the four waves (each <= u
    (1 + 2^-6) times the sum of magnitudes: 3.1 u), the fp64 sum of the nblocks partials adds (nblocks / 16 + 8) u64, and R receives the
    sum rounded once to fp32 (u): |dS_ij| <= (14.1 u + (nblocks / 16 + 8) u64) sum_k |x_ki y_kj|."""
    s = np.abs(x.astype(np.float64)).T @ np.abs(y.astype(np.float64))
    return (C_CROSS_ISOLATED * U32 + (nblocks / 16 + 8) * U64) * s


def half_exact_budget(kmax, exps, m, chain=64):
    """halves k 2^e_j, |k| <= kmax: representable when int_bits(kmax) <= 11 (the fp16 significand) and kmax 2^max(e) <= 65504, normal when
    2^min(e) >= 2^-14.  gram_h_kernel keeps one fp32 MFMA chain per 64-row chunk (products of halves are exact in fp32) and fp64 totals:
    chain kmax^2 < 2^24, m kmax^2 < 2^53.  Returns (significand bits, chain bits, total bits, largest magnitude)."""
    assert exps[0] >= -14
    return int_bits(kmax), int(chain * kmax * kmax).bit_length(), int(max(m, 1) * kmax * kmax).bit_length(), kmax * 2.0 ** exps[1]


def exact_halves(rng, m, n, kmax=511, exps=(-3, 3)):
    """exact_ints cast to float16, with the budget of an 11-bit significand asserted (half_exact_budget): the cast is exact"""
    sig, chain, total, big = half_exact_budget(kmax, exps, m)
    assert sig <= 11 and chain <= 24 and total <= 53 and big <= 65504
    a = exact_ints(rng, m, n, kmax, exps)
    h = a.astype(np.float16)
    assert np.array_equal(h.astype(np.float32), a)
    return h


CROSS_M = [1, 65, 129, 1000, 4097]
CROSS_NY = [1, 17, 64, 65, 130, 197]
HALF_GRAM_M = [64, 65, 127, 4097, 9211]
HALF_N = [17, 33, 48, 64]

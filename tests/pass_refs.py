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

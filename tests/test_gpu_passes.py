"""Each pass of the engine on its own, through the staged C entry points (include/tsqr_mi.h), against exact or fp64 references:

  tsqr_mi_gram_f32      (levels 2 and 1: bf16x3-split and fp64 Gram tiles)  exact data bit for bit, isolated products per entry, dense
  tsqr_mi_apply_rinv_f32 (trinv_kernel + apply engines 0 / 1 / 2)            exact inverses, single products, general R
  tsqr_mi_chol_f32 + tsqr_mi_apply_z_f32                                    chained
  tsqr_mi_rmul_f32      (rmul64_kernel, rmul_kernel)                         within one fp32 ulp of the exact product
  tsqr_mi_local_r_f32   (Householder fold)                                   backward stability, LAPACK, triangular shape
and the padding / alignment contract of the staged entries and of mtk::qr::qr: NaN in the leading-dimension padding and behind the
last column changes nothing, padding of the outputs keeps its sentinels, unaligned base pointers give the aligned results.

Bounds and generators: tests/pass_refs.py (derivations in the docstrings).  Every bounded check prints max(measured / bound)."""
import numpy as np
import pytest

from tests import pass_refs as pr

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT = -777.0                                   # sentinel in the padding of outputs


@pytest.fixture(scope="module")
def env(bq):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return bq, bq.lib(), torch


def _st(torch):
    return torch.cuda.current_stream().cuda_stream


def report(what, measured, bound):
    """max(measured / bound) over the entries (0 / 0 counts as 0); printed, and it must not exceed 1"""
    measured, bound = np.broadcast_arrays(np.asarray(measured, np.float64), np.asarray(bound, np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(measured == 0, 0.0, measured / bound)
    worst = float(np.max(ratio)) if ratio.size else 0.0
    print("%-58s max(measured / bound) = %.3g" % (what, worst))
    assert worst <= 1.0, what
    return worst


# ---- column-major operands in device memory -------------------------------------------------------------------------------------------
def upload(torch, a, ld, pad=0.0, offset=0, slack=16, dtype=np.float32):
    """m x n host matrix -> 1-D device pool holding it column-major with leading dimension ld at element `offset`; everything else of
    the pool (rows m .. ld - 1, `slack` elements behind the last column, the offset) is `pad`.  slack = 0 puts A at the pool's tail.
    Returns (pool, address of A)."""
    m, n = a.shape
    host = np.full(offset + (n - 1) * ld + m + slack, pad, dtype)
    for j in range(n):
        host[offset + j * ld: offset + j * ld + m] = a[:, j]
    pool = torch.from_numpy(host).cuda()
    return pool, pool.data_ptr() + offset * host.itemsize


def download(pool, m, n, ld, offset=0):
    host = pool.cpu().numpy()
    return np.stack([host[offset + j * ld: offset + j * ld + m] for j in range(n)], axis=1)


def out_pool(torch, m, n, ld, offset=0, fill=NAN, dtype=None):
    dtype = dtype or torch.float32
    pool = torch.full((offset + (n - 1) * ld + m,), fill, dtype=dtype, device="cuda")
    return pool, pool.data_ptr() + offset * pool.element_size()


def padding_of(pool, m, n, ld, offset=0):
    """the pool's elements outside the m x n block"""
    host = pool.cpu().numpy().copy()
    mask = np.ones(host.size, bool)
    for j in range(n):
        mask[offset + j * ld: offset + j * ld + m] = False
    return host[mask]


# ---- the staged calls -----------------------------------------------------------------------------------------------------------------
def gram(env, a_ptr, lda, m, n, level):
    """tsqr_mi_gram_f32 -> NP x NP Gram matrix (unpacked tiles; level 2: f32 accumulator layout, level 1: f64)"""
    bq, L, torch = env
    bf = bq.buffer(bq.compute_mode.fp32_tc_cor)
    bf.allocate(m, n)
    gs = torch.full((pr.gram_elems(n),), NAN, dtype=torch.float64, device="cuda")
    rc = L.tsqr_mi_gram_f32(level, gs.data_ptr(), a_ptr, lda, m, n, bf.dwq.data_ptr(), bf.dwr.data_ptr(), _st(torch))
    assert rc == 0, bq.last_error()
    torch.cuda.synchronize()
    return pr.unpack_tiles(gs.cpu().numpy(), n, level == 2)


def apply_rinv(env, mode, q_ptr, ldq, a_ptr, lda, r_ptr, ldr, m, n):
    bq, L, torch = env
    bf = bq.buffer(mode)
    bf.allocate(m, n)
    rc = L.tsqr_mi_apply_rinv_f32(int(mode), q_ptr, ldq, a_ptr, lda, r_ptr, ldr, m, n, bf.dwq.data_ptr(), _st(torch))
    assert rc == 0, bq.last_error()
    torch.cuda.synchronize()


def padded_exact(g, n):
    np_ = 16 * pr.ntiles(n)
    out = np.zeros((np_, np_))
    out[:n, :n] = g
    return out


ENGINES = {0: "fp32_notc", 1: "fp32_tc_cor", 2: "fp32_tc_nocor"}


def dev_exact_ints(torch, m, n, seed, kmax=511, exps=(-3, 3)):
    """pass_refs.exact_ints on the device (the same distribution; for the row counts where a host generator would dominate the time)"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    top = 1 << (pr.int_bits(kmax) - 1)
    k = torch.randint(top, kmax + 1, (n, m), generator=g, device="cuda", dtype=torch.int32)
    k2 = torch.randint(-kmax, kmax + 1, (n, m), generator=g, device="cuda", dtype=torch.int32)
    k = torch.where(torch.rand(n, m, generator=g, device="cuda") < 0.2, k2, k)
    k = k * (torch.randint(0, 2, (n, m), generator=g, device="cuda", dtype=torch.int32) * 2 - 1)
    e = torch.randint(exps[0], exps[1] + 1, (n, 1), generator=g, device="cuda").float()
    return k.float() * torch.exp2(e)                                   # n x m: column-major m x n with ld = m


# =========================================================================================================================================
# 1. Gram pass
# =========================================================================================================================================
GRAM_EXACT = [(1, 1), (31, 7), (32, 16), (33, 17), (127, 33), (128, 51), (129, 63), (33, 64), (4097, 64), (9211, 51), (4097, 1),
              (129, 47)]


@pytest.mark.parametrize("m,n", GRAM_EXACT)
@pytest.mark.parametrize("level", [2, 1])
def test_gram_exact_integers_bit_for_bit(env, m, n, level):
    """A = k 2^e_j, |k| <= 511 (nine bits: the bf16 split has a mid part): a 32-row fp32 chain stays below 2^23 and the fp64 totals below
    2^53 (pass_refs.gram_exact_budget), so A^T A is exact in any summation order -- both levels must give it in every entry of every
    tile, the zero padding beyond column n included.  lda = m + 3 (odd: the chunk kernel for n = 64)."""
    bq, L, torch = env
    assert all(b <= lim for b, lim in zip(pr.gram_exact_budget(511, m), (24, 53)))
    a = pr.exact_ints(np.random.default_rng(1000 * m + n), m, n)
    pool, ap = upload(torch, a, m + 3)
    g = gram(env, ap, m + 3, m, n, level)
    ref = padded_exact(a.astype(np.float64).T @ a.astype(np.float64), n)
    assert np.array_equal(g, ref), np.argwhere(g != ref)[:5]


@pytest.mark.parametrize("m,ld_pad", [(128 * 33, 0), (128 * 33, 1), (1 << 20, 0), (1 << 20, 4), (1 << 20, 1), ((1 << 20) + 128, 0),
                                      (3 << 20, 0)])
@pytest.mark.parametrize("level", [2, 1])
def test_gram_exact_integers_large(env, m, ld_pad, level):
    """the same exact check on the dispatch branches of the 64-column Gram pass: gram_blk_kernel (m % 128 == 0, m <= 2^20, ld % 4 == 0,
    aligned) against the chunk kernel on the same m with ld = m + 1, beyond 2^20 rows, and 3 x 2^20 rows (fp64 totals above 2^32;
    every partial sum is still an integer below 2^41).  Data and fp64 reference on the device (exact as well)."""
    bq, L, torch = env
    n = 64
    assert all(b <= lim for b, lim in zip(pr.gram_exact_budget(511, m), (24, 53)))
    at = dev_exact_ints(torch, m, n, seed=m + ld_pad)
    ld = m + ld_pad
    if ld_pad:
        buf = torch.full((n, ld), NAN, device="cuda")                   # (NaN padding: read nowhere)
        buf[:, :m] = at
    else:
        buf = at
    g = gram(env, buf.data_ptr(), ld, m, n, level)
    a64 = at.double()
    ref = (a64 @ a64.T).cpu().numpy()
    del a64
    assert np.array_equal(g, ref), np.argwhere(g != ref)[:5]


@pytest.mark.parametrize("m,n", [(33, 17), (4097, 64), (9211, 51), (1 << 20, 64), (65, 7)])
@pytest.mark.parametrize("level", [2, 1])
def test_gram_isolated_products(env, m, n, level):
    """full 24-bit mantissas over +-20 binades, one non-zero row per 64-row stretch: every fp32 chain of level 2 holds ONE product per
    entry, so the per-entry bound of pass_refs.gram_l2_isolated_bound holds deterministically (a two-term split errs near 2^-16);
    level 1 within pass_refs.gram_l1_bound (the fp64 reference carries an error of the same kind: the check allows both)."""
    bq, L, torch = env
    a = pr.isolated_rows(np.random.default_rng(m + 7 * n), m, n)
    pool, ap = upload(torch, a, m)
    g = gram(env, ap, m, m, n, level)[:n, :n]
    nz = a[np.any(a != 0, axis=1)].astype(np.float64)
    ref = nz.T @ nz
    err = np.abs(g - ref)
    if level == 2:
        report("gram L2 isolated m=%d n=%d" % (m, n), err, pr.gram_l2_isolated_bound(a))
    else:
        report("gram L1 isolated m=%d n=%d" % (m, n), err, 2 * pr.gram_l1_bound(a))


@pytest.mark.parametrize("m,n", [(4097, 33), (1 << 20, 64)])
@pytest.mark.parametrize("level", [2, 1])
def test_gram_dense_same_sign(env, m, n, level):
    """U(0.5, 1) entries (same sign: no cancellation to hide a rounding), normwise against the fp64 product: level 2 within
    pass_refs.gram_l2_dense_bound, level 1 within the fp64-accumulation bound (reference error allowed for as above)"""
    bq, L, torch = env
    gen = torch.Generator(device="cuda")
    gen.manual_seed(m + n)
    at = torch.rand(n, m, generator=gen, device="cuda") * 0.5 + 0.5
    g = gram(env, at.data_ptr(), m, m, n, level)[:n, :n]
    a = at.cpu().numpy().T
    ref = (at.double() @ at.double().T).cpu().numpy()
    if level == 2:
        report("gram L2 dense m=%d n=%d" % (m, n), np.linalg.norm(g - ref), pr.gram_l2_dense_bound(a))
    else:
        report("gram L1 dense m=%d n=%d" % (m, n), np.abs(g - ref), 2 * pr.gram_l1_bound(a))


# =========================================================================================================================================
# 2. Apply pass and triangular inverse
# =========================================================================================================================================
APPLY_SHAPES = [(1, 7, 3), (33, 17, 16), (127, 33, 32), (129, 64, 32), (4097, 64, 23), (9211, 51, 40), (65, 16, 5), (128, 1, 0)]


def _apply_case(env, mode, a, r, inplace, ld_pad=3):
    bq, L, torch = env
    m, n = a.shape
    ld = m + ld_pad
    ldr = n + 2
    rpool, rp = upload(torch, r, ldr, pad=SENT)
    apool, ap = upload(torch, a, ld, pad=NAN)
    if inplace:
        apply_rinv(env, mode, ap, ld, ap, ld, rp, ldr, m, n)
        q, qpad = download(apool, m, n, ld), padding_of(apool, m, n, ld)
    else:
        qpool, qp = out_pool(torch, m, n, ld, fill=SENT)
        apply_rinv(env, mode, qp, ld, ap, ld, rp, ldr, m, n)
        q, qpad = download(qpool, m, n, ld), padding_of(qpool, m, n, ld)
        assert np.array_equal(download(apool, m, n, ld), a)           # A is only read
        assert np.isnan(padding_of(apool, m, n, ld)).all()
        assert np.all(qpad == SENT)                                     # nothing written outside the m x n block of Q
    assert np.all(padding_of(rpool, n, n, ldr) == SENT)
    return q


@pytest.mark.parametrize("m,n,split", APPLY_SHAPES)
@pytest.mark.parametrize("engine", [0, 1, 2])
@pytest.mark.parametrize("inplace", [False, True])
def test_apply_exact_inverse_small_integers(env, m, n, split, engine, inplace):
    """R = 2^3 [[I, B], [0, I]] (split at a tile boundary and away from one), B and A integers of at most six bits (exact in bf16 and
    fp16): inverse(R) = 2^-3 [[I, -B], [0, I]] is exact in fp64 and fp32, every product and every partial sum of Q = A inverse(R) is a
    multiple of 2^-3 below 2^18 -- all three engines must give Q exactly, out of place and with q == a."""
    bq, L, torch = env
    rng = np.random.default_rng(m * 7 + n + engine)
    if split == 0:
        r, z = np.eye(n, dtype=np.float32), np.eye(n)
    else:
        r, z = pr.exact_inverse_pair(rng, n, split, bmax=63, scale_exp=0)
    r, z = r * np.float32(8.0), z / 8.0
    a = pr.exact_ints(rng, m, n, kmax=63, exps=(0, 0))
    q = _apply_case(env, bq.compute_mode[ENGINES[engine]], a, r, inplace)
    ref = a.astype(np.float64) @ z
    assert np.array_equal(q, ref), np.argwhere(q != ref)[:5]


@pytest.mark.parametrize("m,n,split", [(129, 64, 32), (4097, 64, 23), (9211, 51, 40), (33, 17, 16), (127, 7, 3), (4096, 33, 20)])
@pytest.mark.parametrize("engine", [0, 1, 2])
def test_apply_single_products(env, m, n, split, engine):
    """one non-zero (full mantissa) per row of A and a full-mantissa B: every Q_ij is ONE product a z.  Engine 0 must give fl32(a z) bit
    for bit, engines 1 and 2 stay within pass_refs.apply_single_product_bound (bf16x3: < 8 u; fp16 operands: 2 u16)."""
    bq, L, torch = env
    rng = np.random.default_rng(m + n + 100 * engine)
    r, z = pr.exact_inverse_pair(rng, n, split, b_full=True)
    a = pr.single_entry_rows(rng, m, n, spread=6)
    q = _apply_case(env, bq.compute_mode[ENGINES[engine]], a, r, inplace=False)
    exact = a.astype(np.float64) @ z                                    # one product per entry: exact in fp64
    if engine == 0:
        want = exact.astype(np.float32)                                 # the one rounding of an fp32 FMA
        assert np.array_equal(q, want), np.argwhere(q != want)[:5]
    else:
        report("apply engine %d single products m=%d n=%d" % (engine, m, n), np.abs(q - exact), pr.apply_single_product_bound(engine, exact))


GENERAL = [(e, c) for e in (0, 1, 2) for c in (1.0, 1e3, 1e6) if not (e == 2 and c > 1e3)]


@pytest.mark.parametrize("engine,cond", GENERAL)
@pytest.mark.parametrize("n", [64, 33, 17, 7])
def test_apply_general_triangular(env, engine, cond, n):
    """random R of 2-norm condition 1 .. 1e6: Q against the fp64 product with the exact inverse of the fp32 R, normwise within
    pass_refs.apply_general_bound -- it covers trinv_kernel (fp64 elimination; an fp32 inverse would miss it by cond x) and the
    engine's product.  (fp16 operands: cond <= 1e3, the range the fp32_tc_nocor mode is meant for.)"""
    bq, L, torch = env
    m = 4097
    rng = np.random.default_rng(int(cond) + n + engine)
    r = pr.random_triangular(rng, n, cond)
    a = rng.uniform(-1, 1, (m, n)).astype(np.float32)
    q = _apply_case(env, bq.compute_mode[ENGINES[engine]], a, r, inplace=bool(n % 2))
    z = np.linalg.inv(r.astype(np.float64))
    ref = a.astype(np.float64) @ z
    report("apply engine %d general R n=%d cond=%.0e" % (engine, n, cond), np.linalg.norm(q - ref),
           pr.apply_general_bound(engine, a, z, np.linalg.cond(r.astype(np.float64))))


def test_apply_large_out_of_place_exact(env):
    """one out-of-place call of 2^20 x 64 (256 MiB: the apply pass measures its block shares inside this call) with the exact small-integer
    data of test_apply_exact_inverse_small_integers, engine 1 (the engine of the measured shares) and engine 0: exact Q"""
    bq, L, torch = env
    m, n = 1 << 20, 64
    r, z = pr.exact_inverse_pair(np.random.default_rng(5), n, 40, bmax=63, scale_exp=0)
    r, z = r * np.float32(8.0), z / 8.0
    at = dev_exact_ints(torch, m, n, seed=9, kmax=63, exps=(0, 0))
    rt = torch.from_numpy(np.ascontiguousarray(r.T)).cuda()
    ref = (torch.from_numpy(z).cuda().T @ at.double()).float()         # exact (products and sums below 2^18 x 2^-3), n x m
    for engine in (1, 0):
        q = torch.full((n, m), NAN, device="cuda")
        apply_rinv(env, bq.compute_mode[ENGINES[engine]], q.data_ptr(), m, at.data_ptr(), m, rt.data_ptr(), n, m, n)
        assert torch.equal(q, ref), engine


@pytest.mark.parametrize("m,n,level", [(9211, 51, 2), (9211, 51, 1), (1 << 16, 64, 2), (4097, 17, 1)])
@pytest.mark.parametrize("engine", [0, 1])
def test_chol_then_apply_z(env, m, n, level, engine):
    """tsqr_mi_gram_f32 -> tsqr_mi_chol_f32 -> tsqr_mi_apply_z_f32: Q against fp64 A inverse(R_returned).  The apply uses the fp64
    inverse of the fp64 Cholesky factor (rounded to fp32) while R_returned is that factor rounded: the difference, A inverse(R64) -
    A inverse(R32) ~ Q dR Z with |dR| <= u |R|, adds u || |Q| |R| |Z| ||_F to pass_refs.apply_general_bound."""
    bq, L, torch = env
    rng = np.random.default_rng(m + n + level)
    a = rng.uniform(-1, 1, (m, n)).astype(np.float32)
    mode = bq.compute_mode[ENGINES[engine]]
    bf = bq.buffer(mode)
    bf.allocate(m, n)
    at = torch.from_numpy(np.ascontiguousarray(a.T)).cuda()
    gs = torch.full((pr.gram_elems(n),), NAN, dtype=torch.float64, device="cuda")
    r = torch.full((n, n + 1), SENT, device="cuda")
    st = _st(torch)
    import ctypes
    assert L.tsqr_mi_gram_f32(level, gs.data_ptr(), at.data_ptr(), m, m, n, bf.dwq.data_ptr(), bf.dwr.data_ptr(), st) == 0
    status = ctypes.c_uint(77)
    assert L.tsqr_mi_chol_f32(level, r.data_ptr(), n + 1, gs.data_ptr(), m, n, bf.dwq.data_ptr(), ctypes.byref(status), st) == 0
    assert status.value == 0
    q = torch.full((n, m), NAN, device="cuda")
    assert L.tsqr_mi_apply_z_f32(int(mode), q.data_ptr(), m, at.data_ptr(), m, m, n, bf.dwq.data_ptr(), st) == 0
    torch.cuda.synchronize()
    rh = r.cpu().numpy()
    assert np.all(rh[:, n] == SENT)
    R = rh[:, :n].T.astype(np.float64)
    assert np.all(np.tril(R, -1) == 0.0)
    z = np.linalg.inv(R)
    ref = a.astype(np.float64) @ z
    qh = q.cpu().numpy().T.astype(np.float64)
    cond = np.linalg.cond(R)
    bound = pr.apply_general_bound(engine, a, z, cond) + pr.U32 * np.linalg.norm(np.abs(ref) @ np.abs(R) @ np.abs(z))
    report("gram L%d -> chol -> apply_z engine %d m=%d n=%d" % (level, engine, m, n), np.linalg.norm(qh - ref), bound)


# =========================================================================================================================================
# 3. R product
# =========================================================================================================================================
@pytest.mark.parametrize("n", [1, 7, 16, 64, 65, 128, 200, 1024])
def test_rmul_within_one_ulp(env, n):
    """r <- r2 r with fp64 accumulation (rmul64_kernel for n <= 64, rmul_kernel above): every entry within 1 fp32 ulp of the exact
    product plus the n u64 summation allowance (pass_refs.rmul_bound) on same-sign full-mantissa factors, where fp32 accumulation
    drifts by ulps.  ldr = n + 3, ldr2 = n + 5: the padding rows of r keep their sentinel; the lower triangles of both inputs are NaN
    (only the upper triangles are read) and the result has exact zeros below the diagonal."""
    bq, L, torch = env
    rng = np.random.default_rng(n)
    r1 = np.triu(rng.uniform(0.5, 1.0, (n, n))).astype(np.float32)
    r2 = np.triu(rng.uniform(0.5, 1.0, (n, n))).astype(np.float32)
    low = np.tril(np.ones((n, n), bool), -1)
    r1_in, r2_in = r1.copy(), r2.copy()
    r1_in[low] = np.nan
    r2_in[low] = np.nan
    ldr, ldr2 = n + 3, n + 5
    rpool, rp = upload(torch, r1_in, ldr, pad=SENT, slack=0)
    r2pool, r2p = upload(torch, r2_in, ldr2, pad=NAN, slack=0)
    wq = torch.empty(n * n, device="cuda")
    assert L.tsqr_mi_rmul_f32(rp, ldr, r2p, ldr2, n, wq.data_ptr(), _st(torch)) == 0
    torch.cuda.synchronize()
    p = download(rpool, n, n, ldr).astype(np.float64)
    assert np.all(padding_of(rpool, n, n, ldr) == SENT)
    assert np.all(p[low] == 0.0)
    exact = r2.astype(np.float64) @ r1.astype(np.float64)
    report("rmul n=%d" % n, np.abs(p - exact), pr.rmul_bound(r2, r1))


# =========================================================================================================================================
# 4. Householder local R
# =========================================================================================================================================
@pytest.mark.parametrize("n", [64, 33])
@pytest.mark.parametrize("mk", ["1", "n-1", "n", "65", "4097", "2^18"])
def test_local_r(env, n, mk):
    """tsqr_mi_local_r_f32: ||R^T R - A^T A||_F within the cond-independent backward bound (pass_refs.local_r_backward_bound), exact
    zeros below the diagonal, ldr padding untouched; for m >= n the sign-normalised R against LAPACK's fp64 R on a well-conditioned A
    (pass_refs.local_r_forward_bound)."""
    bq, L, torch = env
    m = {"1": 1, "n-1": n - 1, "n": n, "65": 65, "4097": 4097, "2^18": 1 << 18}[mk]
    rng = np.random.default_rng(m + n)
    a = rng.uniform(-1, 1, (m, n)).astype(np.float32)
    bf = bq.buffer(bq.compute_mode.fp32_notc)
    bf.allocate(max(m, n), n)
    apool, ap = upload(torch, a, m + 1, pad=NAN)
    ldr = n + 2
    rpool, rp = out_pool(torch, n, n, ldr, fill=SENT)
    assert L.tsqr_mi_local_r_f32(rp, ldr, ap, m + 1, m, n, bf.dwq.data_ptr(), bf.dwr.data_ptr(), _st(torch)) == 0
    torch.cuda.synchronize()
    R = download(rpool, n, n, ldr).astype(np.float64)
    assert np.all(padding_of(rpool, n, n, ldr) == SENT)
    assert np.all(np.isfinite(R)) and np.all(np.tril(R, -1) == 0.0)
    a64 = a.astype(np.float64)
    report("local R backward m=%d n=%d" % (m, n), np.linalg.norm(R.T @ R - a64.T @ a64), pr.local_r_backward_bound(a))
    if m >= n:
        ref = np.linalg.qr(a64, mode="r")
        s_gpu, s_ref = np.sign(np.diag(R)), np.sign(np.diag(ref))
        s_gpu[s_gpu == 0] = 1
        s_ref[s_ref == 0] = 1
        cond = np.linalg.cond(a64)
        report("local R vs LAPACK m=%d n=%d cond=%.1f" % (m, n, cond), np.linalg.norm(s_gpu[:, None] * R - s_ref[:, None] * ref),
               pr.local_r_forward_bound(a, cond))


# =========================================================================================================================================
# 5. Poisoned padding and unaligned operands
# =========================================================================================================================================
def _qr_call(env, a, mode, lda, ldq, ldr, pad, a_off=0, q_off=0, half=False, slack=16):
    """bq.qr on A (padding `pad`) -> (q, r, Q pool padding, R padding)"""
    bq, L, torch = env
    m, n = a.shape
    tdt = torch.float16 if half else torch.float32
    apool, ap = upload(torch, a, lda, pad=pad, offset=a_off, slack=slack, dtype=np.float16 if half else np.float32)
    qpool, qp = out_pool(torch, m, n, ldq, offset=q_off, fill=SENT, dtype=tdt)
    rpool = torch.full((n * ldr,), SENT, dtype=tdt, device="cuda")
    rpool.view(n, ldr)[:, :n] = 0                                       # the caller pre-zeros R (reference src/test.cu:129)
    bf = bq.buffer(mode)
    bf.allocate(m, n)
    # (bq.qr takes tensors; pass views that start at the carved addresses)
    qv = qpool[q_off:]
    av = apool[a_off:]
    st = bq.qr(qv, ldq, rpool, ldr, av, lda, m, n, bf)
    assert st == bq.success_factorization
    torch.cuda.synchronize()
    assert av.data_ptr() == ap and qv.data_ptr() == qp
    q = download(qpool, m, n, ldq, q_off)
    r = download(rpool, n, n, ldr)
    return q, r, padding_of(qpool, m, n, ldq, q_off), padding_of(rpool, n, n, ldr)


QR_CASES = [(4097, 64, "fp32_tc_cor"), (4096, 64, "fp32_notc"), (3000, 100, "fp32_tc_cor"), (5000, 200, "fp32_notc"),
            (4096, 64, "fp16_notc"), (2000, 33, "fp16_tc_nocor")]


@pytest.mark.parametrize("m,n,mode", QR_CASES)
def test_qr_nan_padding_changes_nothing(env, m, n, mode):
    """mtk::qr::qr (one panel, the n = 100 one-panel path, 128-column blocks, the fp16 entry): NaN in A's padding rows (m .. lda - 1) and
    behind its last column gives the same Q and R bit for bit as zero padding; Q's ldq padding and R's ldr padding keep their sentinels."""
    bq, L, torch = env
    md = bq.compute_mode[mode]
    half = md in bq.FP16_MODES
    a = np.random.default_rng(m + n).uniform(-1, 1, (m, n)).astype(np.float16 if half else np.float32)
    lda = m + (8 if half else 5)
    outs = [_qr_call(env, a, md, lda, m + 3, n + 2, pad, half=half) for pad in (0.0, NAN)]
    (q0, r0, qp0, rp0), (q1, r1, qp1, rp1) = outs
    assert np.isfinite(q0.astype(np.float32)).all()
    assert np.array_equal(q0, q1) and np.array_equal(r0, r1)
    for p in (qp0, qp1, rp0, rp1):
        assert np.all(p == SENT)


@pytest.mark.parametrize("m,n", [(4097, 64), (4096, 64), (129, 17), (33, 7)])
@pytest.mark.parametrize("level", [2, 1])
def test_gram_nan_padding_changes_nothing(env, m, n, level):
    bq, L, torch = env
    a = np.random.default_rng(m + n).uniform(-1, 1, (m, n)).astype(np.float32)
    g = []
    for pad in (0.0, NAN):
        pool, ap = upload(torch, a, m + 4, pad=pad)
        g.append(gram(env, ap, m + 4, m, n, level))
    assert np.array_equal(g[0], g[1])


@pytest.mark.parametrize("m,n", [(4097, 64), (129, 17), (33, 7), (100, 51)])
@pytest.mark.parametrize("engine", [0, 1, 2])
def test_apply_and_local_r_nan_padding_changes_nothing(env, m, n, engine):
    """tsqr_mi_apply_rinv_f32 and tsqr_mi_local_r_f32 with NaN around A and in R's lower triangle / ldr padding: the same bits as with
    zeros there"""
    bq, L, torch = env
    rng = np.random.default_rng(m + n + engine)
    a = rng.uniform(-1, 1, (m, n)).astype(np.float32)
    r = pr.random_triangular(rng, n, 10.0)
    outs = []
    for pad in (0.0, NAN):
        rr = r.copy()
        rr[np.tril(np.ones((n, n), bool), -1)] = pad
        rpool, rp = upload(torch, rr, n + 3, pad=pad)
        apool, ap = upload(torch, a, m + 5, pad=pad)
        qpool, qp = out_pool(torch, m, n, m + 2, fill=SENT)
        apply_rinv(env, bq.compute_mode[ENGINES[engine]], qp, m + 2, ap, m + 5, rp, n + 3, m, n)
        assert np.all(padding_of(qpool, m, n, m + 2) == SENT)
        outs.append(download(qpool, m, n, m + 2))
        if engine == 0:
            bf = bq.buffer(bq.compute_mode.fp32_notc)
            bf.allocate(m, n)
            lpool, lp = out_pool(torch, n, n, n + 1, fill=SENT)
            assert L.tsqr_mi_local_r_f32(lp, n + 1, ap, m + 5, m, n, bf.dwq.data_ptr(), bf.dwr.data_ptr(), _st(torch)) == 0
            torch.cuda.synchronize()
            assert np.all(padding_of(lpool, n, n, n + 1) == SENT)
            outs.append(download(lpool, n, n, n + 1))
    half = len(outs) // 2
    for x, y in zip(outs[:half], outs[half:]):
        assert np.isfinite(x).all() and np.array_equal(x, y)


@pytest.mark.parametrize("off", [1, 2, 3])
def test_unaligned_staged_exact(env, off):
    """A carved from a NaN pool at a base offset of 1, 2, 3 floats and placed at the pool's tail, Q at the same offset in a sentinel
    pool: with the exact data of sections 1 and 2 the results are exact -- the Gram pass of a 64-column m % 128 == 0 matrix then takes
    the chunk kernel instead of gram_blk_kernel (16-byte alignment check), and the apply engines read and write unaligned columns."""
    bq, L, torch = env
    rng = np.random.default_rng(off)
    m, n = 4096, 64
    a = pr.exact_ints(rng, m, n)
    pool, ap = upload(torch, a, m, pad=NAN, offset=off, slack=0)
    ref = padded_exact(a.astype(np.float64).T @ a.astype(np.float64), n)
    for level in (2, 1):
        assert np.array_equal(gram(env, ap, m, m, n, level), ref), level
    r, z = pr.exact_inverse_pair(rng, n, 23, bmax=63, scale_exp=0)
    r, z = r * np.float32(8.0), z / 8.0
    b = pr.exact_ints(rng, 1000, n, kmax=63, exps=(0, 0))
    bpool, bp = upload(torch, b, 1001, pad=NAN, offset=off, slack=0)
    rpool, rp = upload(torch, r, n + 1, pad=NAN, offset=off, slack=0)
    for engine in (0, 1, 2):
        qpool, qp = out_pool(torch, 1000, n, 1001, offset=off, fill=SENT)
        apply_rinv(env, bq.compute_mode[ENGINES[engine]], qp, 1001, bp, 1001, rp, n + 1, 1000, n)
        assert np.array_equal(download(qpool, 1000, n, 1001, off), b.astype(np.float64) @ z), engine
        assert np.all(padding_of(qpool, 1000, n, 1001, off) == SENT)


@pytest.mark.parametrize("m,n,mode", QR_CASES)
def test_unaligned_qr_matches_aligned(env, m, n, mode):
    """mtk::qr::qr with A and Q carved at base offsets of 1, 2, 3 floats (1 half for the fp16 entry), A at a NaN pool's tail: the same
    bits as the call on an aligned copy with the same leading dimensions (odd lda, so that both take the same Gram kernel / the fp16
    conversion path)"""
    bq, L, torch = env
    md = bq.compute_mode[mode]
    half = md in bq.FP16_MODES
    a = np.random.default_rng(m * 3 + n).uniform(-1, 1, (m, n)).astype(np.float16 if half else np.float32)
    lda, ldq = m + 1, m + 3
    q0, r0, _, _ = _qr_call(env, a, md, lda, ldq, n, 0.0, half=half)
    for off in ((1,) if half else (1, 2, 3)):
        q1, r1, qpad, _ = _qr_call(env, a, md, lda, ldq, n, NAN, a_off=off, q_off=off, half=half, slack=0)
        assert np.array_equal(q0, q1) and np.array_equal(r0, r1), off
        assert np.all(qpad == SENT)

"""CPU tests of the per-pass references (tests/pass_refs.py): the Gram-tile layouts round-trip, the exact-data generators keep their
bit budgets, and the bounds are what their derivations say on data where the answer is known."""
import numpy as np
import pytest

from tests import pass_refs as pr


@pytest.mark.parametrize("n", [1, 7, 16, 17, 33, 51, 63, 64])
@pytest.mark.parametrize("f32_layout", [True, False])
def test_tile_unpack_inverts_pack(n, f32_layout):
    rng = np.random.default_rng(n)
    g = rng.standard_normal((n, n))
    g = g + g.T
    v = pr.pack_tiles(g, n, f32_layout)
    assert v.shape == (pr.gram_elems(n),)
    back = pr.unpack_tiles(v, n, f32_layout)
    np_ = 16 * pr.ntiles(n)
    want = np.zeros((np_, np_))
    want[:n, :n] = g
    assert np.array_equal(back, want)
    assert np.array_equal(pr.pack_tiles(back[:n, :n], n, f32_layout), v)


def test_tile_layouts_differ_and_match_the_chol_test_packing():
    """the f32 and f64 accumulator layouts put the same element in different places (row 4 (lane >> 4) + reg against (lane >> 4) + 4 reg);
    pack_tiles is the one of tests/test_gpu_chol.py"""
    n = 32
    g = np.arange(n * n, dtype=np.float64).reshape(n, n)
    a, b = pr.pack_tiles(g, n, True), pr.pack_tiles(g, n, False)
    assert not np.array_equal(a, b) and np.array_equal(np.sort(a), np.sort(b))
    assert a[1] == g[0, 1] and a[64] == g[1, 0] and b[64] == g[4, 0]      # (reg 1, lane 0): row 1 (f32) / row 4 (f64)
    assert pr.unpack_tiles(a, n, True)[1, 0] == g[1, 0]                  # a diagonal tile keeps its own lower triangle
    assert pr.unpack_tiles(a, n, True)[16, 0] == g[0, 16]                 # an off-diagonal tile's mirror is its transpose


def test_gram_exact_budget():
    assert pr.int_bits(511) == 9 and pr.int_bits(63) == 6
    chain, total = pr.gram_exact_budget(511, 3 << 20)
    assert chain <= 24 and total <= 53
    assert pr.gram_exact_budget(2047, 1)[0] > 24                          # 11-bit integers would overflow a 32-row fp32 chain


@pytest.mark.parametrize("m,n", [(1, 1), (129, 17), (4097, 64)])
def test_exact_ints_bit_budget(m, n):
    rng = np.random.default_rng(m)
    a = pr.exact_ints(rng, m, n)
    assert a.dtype == np.float32
    for j in range(n):                                                    # every column: integers |k| <= 511 times one power of two
        col = a[:, j].astype(np.float64)
        if not np.any(col):
            continue
        assert any(np.all(col / 2.0 ** e == np.round(col / 2.0 ** e)) and np.abs(col / 2.0 ** e).max() <= 511 for e in range(-3, 4)), j
    if m * n >= 1000:
        # most entries use all nine bits: the bf16 split (eight bits) of such an entry leaves a non-zero mid part
        x = a[a != 0].astype(np.float64)
        hi = np.round(np.frexp(x)[0] * 2 ** 8) / 2 ** 8 * np.exp2(np.frexp(x)[1])
        assert np.mean(x != hi) > 0.3


def test_exact_ints_gram_is_exact_in_fp64_any_order():
    rng = np.random.default_rng(3)
    a = pr.exact_ints(rng, 3000, 17).astype(np.float64)
    g1 = a.T @ a
    g2 = sum(a[k:k + 32].T @ a[k:k + 32] for k in range(0, 3000, 32))
    g3 = (a[::-1].T @ a[::-1])
    assert np.array_equal(g1, g2) and np.array_equal(g1, g3)


def test_full_mantissa_and_isolated_rows():
    rng = np.random.default_rng(4)
    x = pr.full_mantissa(rng, 10000, spread=20)
    bits = x.view(np.uint32)
    assert np.all(bits & 1 == 1)                                          # lowest significand bit set: 24 bits in use
    ex = np.frexp(x.astype(np.float64))[1] - 1
    assert ex.min() >= -20 and ex.max() <= 20 and ex.max() - ex.min() >= 30
    for m in (1, 33, 127, 4097):
        a = pr.isolated_rows(rng, m, 7)
        nzrow = np.any(a != 0, axis=1)
        for k in range(0, m, 32):                                         # at most one non-zero row per 32-row K-step
            assert nzrow[k:k + 32].sum() <= 1
        assert nzrow.sum() == (m + 63) // 64


def test_single_entry_rows():
    a = pr.single_entry_rows(np.random.default_rng(5), 500, 33)
    assert np.all((a != 0).sum(axis=1) == 1)


@pytest.mark.parametrize("n,split", [(64, 32), (64, 23), (17, 16), (51, 40), (2, 1)])
@pytest.mark.parametrize("b_full", [False, True])
def test_exact_inverse_pair(n, split, b_full):
    r, z = pr.exact_inverse_pair(np.random.default_rng(n + split), n, split, b_full=b_full)
    assert np.array_equal(r.astype(np.float64) @ z, np.eye(n))
    assert np.array_equal(z.astype(np.float32).astype(np.float64), z)   # Z is an fp32 matrix
    assert np.array_equal(np.triu(r), r)
    if not b_full:                                                        # small integers: exact in fp16 as well
        assert np.array_equal(z.astype(np.float16).astype(np.float64), z)


def test_random_triangular_condition():
    for cond in (1.0, 1e3, 1e6):
        r = pr.random_triangular(np.random.default_rng(6), 64, cond)
        c = np.linalg.cond(r.astype(np.float64))
        assert np.array_equal(np.triu(r), r) and cond / 3 <= c <= cond * 3


def _split3(x):
    """RNE bf16 split of float32 values, as the kernels do it"""
    def bf(v):
        b = v.astype(np.float32).view(np.uint32).astype(np.uint64)
        b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
        return b.astype(np.uint32).view(np.float32)
    h = bf(x)
    r1 = (x - h).astype(np.float32)
    m = bf(r1)
    r2 = (r1 - m).astype(np.float32)
    return h, m, bf(r2)


def _six_products(a, b):
    """one fp32 chain of the six products, smallest first (mm hl lh hm mh hh), rounded after every addition"""
    ah, am, al = _split3(a)
    bh, bm, bl = _split3(b)
    acc = np.float32(0)
    for x, y in ((am, bm), (ah, bl), (al, bh), (ah, bm), (am, bh), (ah, bh)):
        acc = np.float32(acc + np.float32(x.astype(np.float64) * y.astype(np.float64)))
    return acc


def test_split_product_bound_holds_and_two_terms_break_it():
    """the per-product constant of gram_l2_isolated_bound / apply_single_product_bound on a CPU model of the chain, and a split without
    its hl / lh terms -- the kind of bug the GPU tests are for -- exceeds it by orders of magnitude"""
    rng = np.random.default_rng(7)
    a, b = pr.full_mantissa(rng, 20000, 20), pr.full_mantissa(rng, 20000, 20)
    exact = a.astype(np.float64) * b.astype(np.float64)
    six = _six_products(a, b).astype(np.float64)
    worst = np.max(np.abs(six - exact) / np.abs(exact)) / pr.U32
    assert worst <= pr.C_ENGINE1 / 4                                      # (the model measures < 2 u: the bound sits 4x above)
    ah, am, al = _split3(a)
    bh, bm, bl = _split3(b)
    two = np.float32(np.float32(am * bm) + np.float32(ah * bm)) + np.float32(am * bh) + np.float32(ah * bh)
    worst2 = np.max(np.abs(two.astype(np.float64) - exact) / np.abs(exact)) / pr.U32
    assert worst2 > 10 * pr.C_SPLIT_PRODUCT                              # (errors near 2^-16, the size of h l)


def test_gram_bounds_cover_rounding_models():
    rng = np.random.default_rng(8)
    a = rng.uniform(0.5, 1.0, (4096, 16)).astype(np.float32)
    exact = a.astype(np.float64).T @ a.astype(np.float64)
    # fp32 totals over all rows: far outside the level-2 dense bound
    f32 = a.T @ a
    assert np.linalg.norm(f32 - exact) > 0 and np.all(pr.gram_l1_bound(a) < 1e-9 * exact)
    assert pr.gram_l2_dense_bound(a) < 200 * pr.U32 * np.linalg.norm(exact)
    # fp32 rounding of the level-1 result: beyond the level-1 bound
    assert np.any(np.abs(exact.astype(np.float32) - exact) > pr.gram_l1_bound(a))


def test_rmul_bound_separates_fp64_and_fp32_accumulation():
    rng = np.random.default_rng(9)
    n = 200
    r2 = np.triu(rng.uniform(0.5, 1.0, (n, n))).astype(np.float32)
    r1 = np.triu(rng.uniform(0.5, 1.0, (n, n))).astype(np.float32)
    good = (r2.astype(np.float64) @ r1.astype(np.float64)).astype(np.float32)
    bound = pr.rmul_bound(r2, r1)
    exact = r2.astype(np.float64) @ r1.astype(np.float64)
    assert np.all(np.abs(good - exact) <= bound)
    bad = np.zeros((n, n), np.float32)                                    # fp32 accumulation, k ascending
    for k in range(n):
        bad = (bad + np.outer(r2[:, k], r1[k, :])).astype(np.float32)
    assert np.any(np.abs(bad - exact) > bound)


def test_ulp32():
    assert pr.ulp32(1.0) == 2.0 ** -23 and pr.ulp32(-3.0) == 2.0 ** -22 and pr.ulp32(0.0) > 0


def test_apply_bounds_shape():
    rng = np.random.default_rng(10)
    a = rng.standard_normal((100, 16)).astype(np.float32)
    z = np.triu(rng.standard_normal((16, 16)))
    b0, b1, b2 = (pr.apply_general_bound(e, a, z, 10.0) for e in (0, 1, 2))
    assert 0 < b0 < b1 < b2
    q = a.astype(np.float64) @ z
    assert np.all(pr.apply_single_product_bound(0, q) == 0)
    assert np.all(pr.apply_single_product_bound(1, q) <= 8 * pr.U32 * np.abs(q))


def test_local_r_bounds():
    rng = np.random.default_rng(11)
    a = rng.standard_normal((1000, 64)).astype(np.float32)
    r = np.linalg.qr(a.astype(np.float64), mode="r").astype(np.float32).astype(np.float64)
    d = r.T @ r - a.astype(np.float64).T @ a.astype(np.float64)
    assert np.linalg.norm(d) <= pr.local_r_backward_bound(a)             # rounding R to fp32 alone is far inside it


# =========================================================================================================================================
# The one-panel path (64 < n <= 128)
# =========================================================================================================================================
@pytest.mark.parametrize("n", [65, 80, 97, 113, 127, 128])
def test_wide_tile_unpack_inverts_pack(n):
    rng = np.random.default_rng(n)
    g = rng.standard_normal((n, n))
    g = g + g.T
    v = pr.pack_wide_tiles(g, n)
    assert v.shape == (36 * 256,)
    want = np.zeros((128, 128))
    want[:n, :n] = g
    back = pr.unpack_wide_tiles(v)
    assert np.array_equal(back, want)
    assert np.array_equal(pr.pack_wide_tiles(back[:n, :n], n), v)


def test_wide_tile_order_is_the_kernels():
    """[G11: 10][G22: 10][G12: 16 row-major]; the first ten tiles are pack_tiles' NT = 4 array of G11 (a chol_body16 input), the next ten
    that of G22; the diagonal element (c, c) of diagonal tile d sits where chol_wide_kernel reads it"""
    assert [pr.wide_tile(t, t) for t in range(8)] == [0, 4, 7, 9, 10, 14, 17, 19]
    assert pr.wide_tile(0, 4) == 20 and pr.wide_tile(3, 7) == 35 and pr.wide_tile(1, 6) == 26
    assert sorted(pr.wide_tile(i, j) for i in range(8) for j in range(i, 8)) == list(range(36))
    g = np.arange(128.0 * 128).reshape(128, 128)
    g = g + g.T
    v = pr.pack_wide_tiles(g, 128)
    assert np.array_equal(v[:2560], pr.pack_tiles(g[:64, :64], 64, True))
    assert np.array_equal(v[2560:5120], pr.pack_tiles(g[64:, 64:], 64, True))
    for blk in (0, 1):
        for j in range(64):
            d, cc = j >> 4, j & 15
            e = (2560 if blk else 0) + pr._tri4(d, d) * 256 + (cc & 3) * 64 + 16 * (cc >> 2) + cc
            assert v[e] == g[64 * blk + j, 64 * blk + j]
    e = 5120 + (2 * 4 + 1) * 256 + 3 * 64 + 37                               # G12 tile (2, 5), reg 3, lane 37: row 4 * 2 + 3, column 5
    assert v[e] == g[32 + 11, 64 + 16 + 5]


@pytest.mark.parametrize("n,split", pr.WIDE_CHOL_CASES + [(n, s) for n in pr.WIDE_APPLY_N for s in pr.WIDE_APPLY_SPLITS if s < n])
def test_exact_wide_pair_is_an_exact_inverse_with_a_closed_form_verdict(n, split):
    rng = np.random.default_rng(n + split)
    r, z, g, b = pr.exact_wide_pair(rng, n, split)
    assert np.array_equal(r @ z, np.eye(n)) and np.array_equal(r.T @ r, g)
    assert np.array_equal(r.astype(np.float32), r) and np.array_equal(z.astype(np.float32), z)
    assert np.max(np.abs(g)) * n < 2.0 ** 53
    from tests import pass_refs_f64 as p64
    if np.finfo(np.longdouble).eps < 2.0 ** -60:
        s_ref, ratio_ref = p64.scond_ref(g)
        ratio, s = pr.exact_wide_verdict(b, n)
        assert abs(s_ref - s) <= 1e-12 * s and abs(ratio_ref - ratio) <= 1e-12 * ratio
        assert ratio > 2.0 ** -5
    zw = pr.zw_of(z, n).reshape(128, 128)
    assert np.array_equal(zw[:n, :n].T, z) and np.all(zw[n:] == 0) and np.all(zw[:, n:] == 0)
    # the model of the intended arithmetic reproduces R and Z exactly on this data
    rm, zm = pr.model_chol_wide(g, n)
    assert np.array_equal(rm, r) and np.array_equal(zm, z)


def test_wide_budgets_hold_for_the_gpu_shapes():
    for m in pr.WIDE_GRAM_M + [337]:
        chain, total = pr.gram_exact_budget(511, m)
        assert chain <= 24 and total <= 53
    for split in pr.WIDE_APPLY_SPLITS:
        assert pr.apply_wide_exact_budget(63, 2, split, 3) <= 24
    assert pr.wide_scond_threshold(1000) == 4.0 and pr.wide_scond_threshold(1 << 20) == float(np.float32(0.12) * np.float32(1024.0))
    assert pr.wide_scond_threshold(1 << 30) == 128.0


@pytest.mark.parametrize("n,cond", pr.WIDE_CHOL_GENERAL)
def test_chol_wide_bounds_hold_for_fp64_and_fail_for_fp32_shortcuts(n, cond):
    """the bound against a longdouble factorisation holds for the NumPy model of the intended arithmetic (all products in fp64) and is
    missed by a Schur complement or a Z12 accumulated in fp32 -- by more than a factor of 4 at every case (measured: 8 .. 800, printed;
    of the order of n at cond(A) = 2 and 4).  Only at cond(A) <= 2 does the fp64 term stay far below the ulp term (asserted: below 0.05
    ulp32 on the entries that are not tiny); at cond(A) = 10 and 30 the bound is several ulps wide on the smaller entries and what it still
    guarantees is this separation from the fp32 shortcuts.  The cases are those of the GPU test, pass_refs.WIDE_CHOL_GENERAL: cond(A)
    2 .. 30, the conditioning chol_wide_bounds covers (its docstring says why not 1e3)."""
    from tests import pass_refs_f64 as p64
    p64.require_longdouble()
    rng = np.random.default_rng(int(cond) + n)
    a = pr.well_conditioned(rng, 4 * n, n, cond).astype(np.float64)
    g = pr.unpack_wide_tiles(pr.pack_wide_tiles(a.T @ a, n))[:n, :n]
    r = p64.chol_ld(g)
    z = p64.trinv_ld(r)
    r64, z64 = np.asarray(r, np.float64), np.asarray(z, np.float64)
    br, bz = pr.chol_wide_bounds(r64, z64, n)
    up = np.triu(np.ones((n, n), bool))
    big = up & (np.abs(r64) > 1e-3 * np.max(np.abs(r64)))
    if cond <= 2.0:
        assert np.max((br - 0.5 * pr.ulp32(r64))[big] / pr.ulp32(r64)[big]) < 0.05       # the fp64 term: far below the ulp term
    worst = {}
    for name, kw in (("fp64", {}), ("schur32", {"schur32": True}), ("z12_32", {"z12_32": True})):
        rm, zm = pr.model_chol_wide(g, n, **kw)
        er = np.abs(rm.astype(np.longdouble) - r).astype(np.float64)
        ez = np.abs(zm.astype(np.longdouble) - z).astype(np.float64)
        worst[name] = (float(np.max(er[up] / br[up])), float(np.max(ez[up] / bz[up])))
    print("chol wide model n=%d cond=%g: max(err / bound) on (R, Z) fp64 %s, fp32 Schur %s, fp32 Z12 %s"
          % (n, cond, *("(%.3g, %.3g)" % worst[k] for k in ("fp64", "schur32", "z12_32"))))
    assert worst["fp64"][0] <= 1.0 and worst["fp64"][1] <= 1.0, worst
    assert worst["schur32"][0] > 4.0, worst                                    # R22 (and Z22, Z12) carry the fp32 Schur error
    assert worst["z12_32"][1] > 4.0 and worst["z12_32"][0] <= 1.0, worst       # only Z12 is touched


def test_coupling_and_half_budgets_hold_for_the_gpu_shapes():
    """cross_kernel with the default plan (cpw = 1 up to 2048 chunks: a workgroup sums 256 rows in fp32) and with three waves asked for at
    4097 rows (cpw = 22: one workgroup sums all 4097 rows in fp32, still below 2^24 with |k| <= 63 -- 4228 rows would not be); half operands"""
    for m in pr.CROSS_M:
        wg, total = pr.cross_exact_budget(63, m, 256)
        assert wg <= 24 and total <= 53
    assert pr.cross_exact_budget(63, 4097, 4 * 22 * 64)[0] <= 24 and pr.cross_exact_budget(63, 4228, 4 * 22 * 64)[0] > 24
    for m in pr.HALF_GRAM_M:
        sig, chain, total, big = pr.half_exact_budget(511, (-3, 3), m)
        assert sig <= 11 and chain <= 24 and total <= 53 and big <= 65504
    assert pr.half_exact_budget(2047, (0, 0), 64)[1] > 24                      # eleven-bit integers overrun a 64-row chain
    h = pr.exact_halves(np.random.default_rng(0), 127, 33)
    assert h.dtype == np.float16 and np.max(np.abs(h.astype(np.float64))) <= 511 * 8


def test_cross_isolated_bound_sees_a_dropped_product():
    """NumPy emulation of one isolated product per entry: the exact product rounded to fp32 lies within the bound; with the mid x mid term of
    the bf16 split dropped (about 2^-16 relative) it does not"""
    rng = np.random.default_rng(3)
    x = pr.isolated_rows(rng, 256, 64)
    y = np.zeros((256, 17), np.float32)
    y[np.any(x != 0, axis=1)] = pr.full_mantissa(rng, (4, 17), 6)
    exact = x.astype(np.float64).T @ y.astype(np.float64)
    bound = pr.cross_isolated_bound(x, y, 256, 1)

    def mid(v):
        v = v.astype(np.float64)
        hi = (v.astype(np.float32).view(np.uint32) & 0xffff0000).view(np.float32).astype(np.float64)
        r = v - hi
        return (r.astype(np.float32).view(np.uint32) & 0xffff0000).view(np.float32).astype(np.float64)
    ok = np.abs(exact.astype(np.float32).astype(np.float64) - exact)
    assert np.all(ok <= bound)
    dropped = np.abs(mid(x).T @ mid(y))
    assert np.max(dropped / np.maximum(bound, 1e-300)) > 4.0

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

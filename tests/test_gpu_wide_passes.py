"""Each pass of three kernel families of the fp32 engine on its own, through the test library's entries of
tsqr_gpu_amd/csrc/selftest_f32.hip (the product's kernels with the product's launch arithmetic, f32_plan.h), against exact data bit for
bit or extended-precision references.  The one-panel path (64 < n <= 128), tsqr_selftest_w_*:

  gram_wide_kernel<true> / <false> + gram_reduce1_kernel    all 36 tiles of A^T A, every split of the rows over the two forms
  chol_wide_kernel                                          R, the 128 x 128 Z, the verdict words
  apply_wide_f32_kernel, apply_wide_kernel<1>, <2>          Q = A Z, out of place and in place
the panel coupling (n > 64), tsqr_selftest_cross / _update:
  cross_kernel + cross_reduce_multi_kernel (fused finish)   the block row of R and the operands -S_j, grouped launches, ragged last panel
  the same without the finish + cross_finish_kernel         the same bits
  apply_wg_kernel<E, 4, true, 128> with multi_cols          Y_j - X S_j for every trailing panel
and the native half-typed path (16 < n <= 64), tsqr_selftest_h_*:
  gram_h_kernel<NT>                                         A^T A of half operands
  apply_wg_h_kernel<E, NT, ROWS>                            Q rounded to nearest even, the half-typed R with its overflow to inf

Operands carry NaN in the leading-dimension padding and behind the last column, outputs a sentinel in their padding.  A partition
override is an argument of the entry.  Bounds, generators and their derivations: tests/pass_refs.py.  Every bounded check prints
max(measured / bound)."""
import ctypes
import os

import numpy as np
import pytest

from tests import pass_refs as pr
from tests import pass_refs_f64 as p64
from tests.test_gpu_passes import download, out_pool, padding_of, report, upload

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
SENT = -777.0
c_sz, c_p, c_i = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int
NELEM = pr.WIDE_ELEMS
BIG_M = 1 << 20                                  # row count handed to chol_wide_kernel when the bound on S should be out of the way (122.88)


@pytest.fixture(scope="module")
def st():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    L = ctypes.CDLL(os.path.join(ROOT, "tsqr_gpu_amd", "csrc", "libtsqr_selftest.so"))
    sig = {
        "tsqr_selftest_w_plan": [c_sz, c_i, c_sz, c_p],
        "tsqr_selftest_w_gram": [c_p, c_p, c_sz, c_sz, c_i, c_p, c_sz, c_i],
        "tsqr_selftest_w_chol": [c_p, c_sz, c_p, c_p, c_p, c_p, c_p, c_sz, c_i, c_p, c_sz],
        "tsqr_selftest_w_apply": [c_i, c_p, c_sz, c_p, c_sz, c_sz, c_i, c_p, c_p, c_i],
        "tsqr_selftest_cross_plan": [c_sz, c_i, c_p],
        "tsqr_selftest_cross": [c_p, c_sz, c_p, c_p, c_p, c_sz, c_p, c_sz, c_sz, c_i, c_p, c_sz, c_i, c_i],
        "tsqr_selftest_update": [c_i, c_p, c_sz, c_p, c_sz, c_sz, c_p, c_i, c_i],
        "tsqr_selftest_h_gram": [c_p, c_p, c_sz, c_sz, c_i, c_p, c_sz, c_i],
        "tsqr_selftest_h_apply": [c_i, c_p, c_sz, c_p, c_sz, c_sz, c_i, c_p, c_p, c_p, c_sz, c_i],
    }
    for name, args in sig.items():
        getattr(L, name).restype = c_i
        getattr(L, name).argtypes = args
    return L, torch


def plan(L, m, n, lda):
    out = (ctypes.c_longlong * 10)()
    assert L.tsqr_selftest_w_plan(m, n, lda, ctypes.cast(out, c_p)) == 0
    return dict(zip("nfull nrest wgs_fast wgs_rest part gsum max_wgs blk128 blk64 chol_scratch".split(), out))


# =========================================================================================================================================
# 1. gram_wide_kernel
# =========================================================================================================================================
def gram_wide(st, a, lda, offset=0, wgs_over=0):
    """-> 128 x 128 Gram matrix from the summed tiles; checks the row count word, the sentinels behind the partials and the sums"""
    L, torch = st
    m, n = a.shape
    pool, ap = upload(torch, a, lda, pad=NAN, offset=offset)
    p = plan(L, m, n, lda)
    nparts = (min(p["wgs_fast"], wgs_over) + min(p["wgs_rest"], wgs_over)) if wgs_over else p["wgs_fast"] + p["wgs_rest"]
    cap = nparts * NELEM
    part = torch.full((cap + 64,), SENT, dtype=torch.float64, device="cuda")
    gs = torch.full((NELEM + 1 + 8,), SENT, dtype=torch.float64, device="cuda")
    rc = L.tsqr_selftest_w_gram(gs.data_ptr(), ap, lda, m, n, part.data_ptr(), cap, wgs_over)
    assert rc == 0, rc
    g = gs.cpu().numpy()
    assert g[NELEM] == float(m) and np.all(g[NELEM + 1:] == SENT)
    assert np.all(part[cap:].cpu().numpy() == SENT)           # nothing behind part_cap
    return pr.unpack_wide_tiles(g[:NELEM]), p


def padded128(g):
    out = np.zeros((128, 128))
    out[:g.shape[0], :g.shape[1]] = g
    return out


@pytest.mark.parametrize("m", pr.WIDE_GRAM_M)
def test_gram_wide_exact_bit_for_bit(st, m):
    """A = k 2^e_j, |k| <= 511: a chain is one 32-row K-step per block (pass_refs.gram_exact_budget asserted), so all 36 tiles equal A^T A
    bit for bit and the entries beyond n are exact zeros.  n = 128: the fast form alone (m = 64), the fast form plus a ragged rest,
    the general form alone (m < 64); n < 128: the general form alone.  lda = m + 3 and lda = m; for n = 128 also a base offset of one
    float (the fast form is not gated on alignment)."""
    L, torch = st
    assert all(b <= lim for b, lim in zip(pr.gram_exact_budget(511, m), (24, 53)))
    for n in pr.WIDE_GRAM_N:
        a = pr.exact_ints(np.random.default_rng(1000 * m + n), m, n)
        ref = padded128(a.astype(np.float64).T @ a.astype(np.float64))
        for lda, off in [(m + 3, 0), (m, 0)] + ([(m + 3, 1), (m + (-m) % 4, 1)] if n == 128 else []):
            g, p = gram_wide(st, a, lda, off)
            assert p["nfull"] == (m // 64 if n == 128 else 0) and p["nfull"] + p["nrest"] == -(-m // 64)
            assert np.array_equal(g, ref), (m, n, lda, off, np.argwhere(g != ref)[:5])


@pytest.mark.parametrize("wgs_over", [0, 1, 2])
@pytest.mark.parametrize("n", [128, 100])
def test_gram_wide_exact_workgroup_override(st, n, wgs_over):
    """m = 485 (seven full blocks and a ragged one): one workgroup takes all seven blocks of the fast form -- the X / Y register
    rotation and both image buffers, an odd count --, two workgroups take four and three; n = 100: eight blocks of the general form"""
    m = 485
    a = pr.exact_ints(np.random.default_rng(n + wgs_over), m, n)
    g, p = gram_wide(st, a, m + 3, 0, wgs_over)
    assert (p["nfull"], p["nrest"]) == ((7, 1) if n == 128 else (0, 8))
    ref = padded128(a.astype(np.float64).T @ a.astype(np.float64))
    assert np.array_equal(g, ref), np.argwhere(g != ref)[:5]


@pytest.mark.parametrize("m,n", [(337, 128), (337, 100)])
def test_gram_wide_isolated_products(st, m, n):
    """full 24-bit mantissas, one non-zero row per 64-row stretch: every fp32 chain holds ONE product per entry, so the per-entry bound of
    pass_refs.gram_l2_isolated_bound holds deterministically -- a dropped correction product of the split errs near 2^-16"""
    a = pr.isolated_rows(np.random.default_rng(m + 7 * n), m, n)
    g, _ = gram_wide(st, a, m + 3)
    assert np.all(g[n:] == 0) and np.all(g[:, n:] == 0)
    nz = a[np.any(a != 0, axis=1)].astype(np.float64)
    report("gram wide isolated m=%d n=%d" % (m, n), np.abs(g[:n, :n] - nz.T @ nz), pr.gram_l2_isolated_bound(a))


def test_gram_wide_refuses_what_does_not_fit(st):
    """-100 before any launch: partials that do not fit part_cap (the buffer keeps its sentinel), lda < m, n outside 65 .. 128"""
    L, torch = st
    m, n = 193, 128
    a = np.ones((m, n), np.float32)
    pool, ap = upload(torch, a, m)
    part = torch.full((4 * NELEM,), SENT, dtype=torch.float64, device="cuda")
    gs = torch.full((NELEM + 1,), SENT, dtype=torch.float64, device="cuda")
    assert L.tsqr_selftest_w_gram(gs.data_ptr(), ap, m, m, n, part.data_ptr(), 4 * NELEM - 1, 0) == -100
    assert L.tsqr_selftest_w_gram(gs.data_ptr(), ap, m - 1, m, n, part.data_ptr(), 4 * NELEM, 0) == -100
    for bad_n in (64, 129, 0):
        assert L.tsqr_selftest_w_gram(gs.data_ptr(), ap, m, m, bad_n, part.data_ptr(), 4 * NELEM, 0) == -100
    assert L.tsqr_selftest_w_gram(gs.data_ptr(), ap, m, 0, n, part.data_ptr(), 4 * NELEM, 0) == -100
    torch.cuda.synchronize()
    assert np.all(part.cpu().numpy() == SENT) and np.all(gs.cpu().numpy() == SENT)


# =========================================================================================================================================
# 2. chol_wide_kernel
# =========================================================================================================================================
def chol_wide(st, tiles, m, n, prev=None, ldr=None):
    """-> (R n x n, Z 128 x 128 [row, column], status[3] words, host words, R pool padding)"""
    L, torch = st
    ldr = ldr or n + 3
    gs = torch.from_numpy(np.concatenate([tiles, [float(m)]])).cuda()
    rpool, rp = out_pool(torch, n, n, ldr, fill=SENT)
    zw = torch.full((128 * 128 + 16,), SENT, device="cuda")
    status = torch.full((16,), 77, dtype=torch.int32, device="cuda")
    host = torch.full((16,), 77, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(plan(L, m, n, m)["chol_scratch"], device="cuda")
    prev_t = None if prev is None else torch.tensor([prev, 0, 0, 0], dtype=torch.int32, device="cuda")
    rc = L.tsqr_selftest_w_chol(rp, ldr, zw.data_ptr(), status.data_ptr(), host.data_ptr(), None if prev is None else prev_t.data_ptr(),
                                gs.data_ptr(), m, n, scratch.data_ptr(), scratch.numel())
    assert rc == 0, rc
    zh = zw.cpu().numpy()
    assert np.all(zh[128 * 128:] == SENT)
    sw = status.cpu().numpy().view(np.uint32)
    hw = host.cpu().numpy().view(np.uint32)
    assert np.all(sw[3:] == 77) and np.all(hw[3:] == 77) and np.array_equal(sw[:3], hw[:3])
    return download(rpool, n, n, ldr), zh[:128 * 128].reshape(128, 128).T, sw[:3], padding_of(rpool, n, n, ldr)


def f32_of(word):
    return float(np.array([word], np.uint32).view(np.float32)[0])


@pytest.mark.parametrize("n,split", pr.WIDE_CHOL_CASES)
def test_chol_wide_exact_bit_for_bit(st, n, split):
    """G = R^T R, R = 2^3 [[I, B], [0, I]] with small integers (pass_refs.exact_wide_pair: every fp64 operation of the factorisation is
    exact), the split inside the first block, on column 64 and inside the second: R and the 128 x 128 Z bit for bit, exact zeros in the
    strict lower triangle and beyond n, the ldr padding intact, accepted, and the verdict words equal to their closed forms"""
    rng = np.random.default_rng(n * 131 + split)
    r, z, g, b = pr.exact_wide_pair(rng, n, split)
    rg, zg, sw, rpad = chol_wide(st, pr.pack_wide_tiles(g, n), BIG_M, n)
    assert np.all(rpad == SENT)
    assert np.array_equal(rg, r), np.argwhere(rg != r)[:5]
    assert np.array_equal(zg, padded128(z)), np.argwhere(zg != padded128(z))[:5]
    ratio, s = pr.exact_wide_verdict(b, n)
    assert sw[0] == 0
    assert f32_of(sw[1]) == float(np.float32(ratio)) and abs(f32_of(sw[2]) - s) <= pr.ulp32(s)


@pytest.mark.parametrize("n,cond", pr.WIDE_CHOL_GENERAL)
def test_chol_wide_against_longdouble(st, n, cond):
    """G = A^T A (fp64) of a random fp32 A, packed through pass_refs.pack_wide_tiles: R and Z within pass_refs.chol_wide_bounds of a
    longdouble factorisation of the same doubles (half an fp32 ulp plus the fp64 term, over the conditioning that bound covers, cond(A) 2 .. 30: the NumPy model with an
    fp32 Schur complement or Z12 misses it by a factor of 8 .. 800, tests/test_pass_refs.py), exact zeros below the diagonal and beyond n.  The verdict words against longdouble:
    the kernel forms the ratio as 1 / (g_jj z_jj^2) and S as a sum of n (n + 1) / 2 fp64 terms, then rounds each to fp32 -- one fp32 ulp
    covers the rounding, 1e-10 relative the fp64 sums and the (1 + d)^4 of the pivot scaling.  (R and Z reach max(measured / bound) = 1 to
    three digits: the bound is half an ulp plus a small term and some entry rounds by nearly half an ulp; report() asserts
    worst <= 1.0, so a result exactly on the bound passes.)"""
    p64.require_longdouble()
    rng = np.random.default_rng(int(cond) + n)
    a = pr.well_conditioned(rng, 4 * n, n, cond).astype(np.float64)
    g = a.T @ a
    g = np.triu(g) + np.triu(g, 1).T
    rg, zg, sw, rpad = chol_wide(st, pr.pack_wide_tiles(g, n), BIG_M, n)
    assert np.all(rpad == SENT) and sw[0] == 0
    r = p64.chol_ld(g)
    z = p64.trinv_ld(r)
    br, bz = pr.chol_wide_bounds(np.asarray(r, np.float64), np.asarray(z, np.float64), n)
    up = np.triu(np.ones((n, n), bool))
    assert np.all(rg[~up] == 0) and np.all(zg[:n, :n][~up] == 0) and np.all(zg[n:] == 0) and np.all(zg[:, n:] == 0)
    er = np.abs(rg.astype(np.longdouble) - r).astype(np.float64)
    ez = np.abs(zg[:n, :n].astype(np.longdouble) - z).astype(np.float64)
    report("chol wide R n=%d cond=%g" % (n, cond), er[up], br[up])
    report("chol wide Z n=%d cond=%g" % (n, cond), ez[up], bz[up])
    s_ref, ratio_ref = p64.scond_ref(g)
    report("chol wide pivot ratio n=%d cond=%g" % (n, cond), abs(f32_of(sw[1]) - min(ratio_ref, 1.0)), pr.ulp32(ratio_ref) + 1e-10 * ratio_ref)
    report("chol wide S n=%d cond=%g" % (n, cond), abs(f32_of(sw[2]) - s_ref), pr.ulp32(s_ref) + 1e-10 * s_ref)


def _b_with(split, n, col, colsum, ones_elsewhere=0):
    """B (split x (n - split)) with `colsum` ones in column `col` and `ones_elsewhere` further ones spread four to a column"""
    b = np.zeros((split, n - split))
    b[:colsum, col] = 1.0
    k = 0
    for j in range(n - split):
        for i in range(4):
            if j != col and k < ones_elsewhere:
                b[split - 1 - i, j] = 1.0
                k += 1
    assert k == ones_elsewhere
    return b


def test_chol_wide_pivot_verdicts(st):
    """pivot ratio r_jj^2 / g_jj = 1 / (1 + sum_i b_ij^2) (pass_refs.exact_wide_pair) against the threshold 2^-5, at a row count where S
    is out of the way: 1/25 accepted; 1/36 in a column of the FIRST block (split 50, column 55: the first factorisation rejects, words
    [1] and [2] are zero); 1/36 in a column of the second block, whose own factorisation -- on the Schur complement, diagonal 4^k --
    sees ratio 1: only the verdict over both blocks, on the ORIGINAL diagonal of G, rejects, and reports 1/36 and S"""
    n = 128
    for split, col, colsum, want in [(50, 5, 24, 0), (50, 5, 35, 1), (64, 7, 24, 0), (64, 7, 35, 2)]:
        b = _b_with(split, n, col, colsum)
        r, z, g = pr.wide_pair_from_b(b, n)
        rg, zg, sw, _ = chol_wide(st, pr.pack_wide_tiles(g, n), BIG_M, n)
        ratio, s = pr.exact_wide_verdict(b, n)
        if want == 1:
            assert list(sw) == [1, 0, 0], (split, colsum, sw)
        else:
            assert sw[0] == (1 if want else 0), (split, colsum, sw)
            assert f32_of(sw[1]) == float(np.float32(ratio)) and f32_of(sw[2]) == float(np.float32(s))
            assert np.array_equal(rg, r) and np.array_equal(zg, padded128(z))


def test_chol_wide_scond_threshold(st):
    """S = 1 + 2 ||B||_F^2 / n in closed form, rows = 1000 where the bound min(128, max(4, 0.12 sqrt(rows))) is 4: ||B||_F^2 = 191
    (S = 3.984) and 192 (S = 4 exactly: the rule is S <= bound) are accepted, 193 (S = 4.016) is rejected; with rows = 2^20 (bound 122.88)
    the same matrix is accepted"""
    n, split = 128, 64
    assert pr.wide_scond_threshold(1000) == 4.0
    for ones, rows, want in [(191, 1000, 0), (192, 1000, 0), (193, 1000, 1), (193, BIG_M, 0)]:
        b = _b_with(split, n, 0, 2, ones - 2)
        assert np.sum(b * b) == ones
        r, z, g = pr.wide_pair_from_b(b, n)
        rg, zg, sw, _ = chol_wide(st, pr.pack_wide_tiles(g, n), rows, n)
        ratio, s = pr.exact_wide_verdict(b, n)
        assert s == 1.0 + 2.0 * ones / n
        assert sw[0] == want and f32_of(sw[1]) == float(np.float32(ratio)) and f32_of(sw[2]) == float(np.float32(s)), (ones, rows, sw)


def test_chol_wide_previous_rejection_and_refusals(st):
    """a non-zero prev_status gives the reject words without reading G (NaN tiles) and writes neither R nor Z; the entry refuses ldr < n,
    n outside 65 .. 128 and a short scratch buffer"""
    L, torch = st
    n = 100
    rg, zg, sw, rpad = chol_wide(st, np.full(NELEM, NAN), 1000, n, prev=1)
    assert list(sw) == [1, 0, 0] and np.all(rg == SENT) and np.all(zg == SENT) and np.all(rpad == SENT)
    buf = torch.zeros(128 * 128 + 9000, device="cuda")
    gs = torch.zeros(NELEM + 1, dtype=torch.float64, device="cuda")
    w = torch.zeros(16, dtype=torch.int32, device="cuda")
    args = lambda ldr, nn, sc: (buf.data_ptr(), ldr, buf.data_ptr(), w.data_ptr(), None, None, gs.data_ptr(), 1000, nn, buf.data_ptr(), sc)
    assert L.tsqr_selftest_w_chol(*args(99, 100, 8224)) == -100
    assert L.tsqr_selftest_w_chol(*args(128, 64, 8224)) == -100
    assert L.tsqr_selftest_w_chol(*args(130, 129, 8224)) == -100
    need = plan(L, 1000, 100, 1000)["chol_scratch"]
    assert need == 8224 and L.tsqr_selftest_w_chol(*args(128, 100, need - 1)) == -100


# =========================================================================================================================================
# 3. apply_wide_f32_kernel, apply_wide_kernel<1>, apply_wide_kernel<2>
# =========================================================================================================================================
def apply_wide(st, engine, a, zw, inplace, wgs_over=0, skip=None, lda=None, ldq=None):
    """-> Q (m x n); out of place with ldq != lda (both odd by default), A read only and its NaN padding intact, Q's padding sentinel"""
    L, torch = st
    m, n = a.shape
    lda = lda or m + (3 if m % 2 == 0 else 4)
    ldq = lda if inplace else (ldq or lda + 2)
    apool, ap = upload(torch, a, lda, pad=SENT if inplace else NAN)
    zt = torch.from_numpy(zw).cuda()
    skip_t = None if skip is None else torch.tensor([skip, 0, 0, 0], dtype=torch.int32, device="cuda")
    if inplace:
        qpool, qp = apool, ap
    else:
        qpool, qp = out_pool(torch, m, n, ldq, fill=SENT)
    rc = L.tsqr_selftest_w_apply(engine, qp, ldq, ap, lda, m, n, zt.data_ptr(), None if skip is None else skip_t.data_ptr(), wgs_over)
    assert rc == 0, rc
    assert np.all(padding_of(qpool, m, n, ldq) == SENT)
    if not inplace:
        assert np.array_equal(download(apool, m, n, lda), a) and np.isnan(padding_of(apool, m, n, lda)).all()
    return download(qpool, m, n, ldq)


def _exact_apply_operands(rng, m, n, split):
    assert pr.apply_wide_exact_budget(63, 2, split, 3) <= 24
    _, z, _, _ = pr.exact_wide_pair(rng, n, split)
    a = pr.exact_ints(rng, m, n, kmax=63, exps=(0, 0))
    return a, z, a.astype(np.float64) @ z


@pytest.mark.parametrize("m", pr.WIDE_APPLY_M)
@pytest.mark.parametrize("engine", [0, 1, 2])
def test_apply_wide_exact(st, engine, m):
    """A integers |a| <= 63, Z = 2^-3 [[I, -B], [0, I]] handed over in chol_wide_kernel's zw layout (ld 128): every product and partial sum
    is exact in all three engines (pass_refs.apply_wide_exact_budget) -- Q bit for bit, out of place (ldq != lda, both odd) and in place;
    the splits fall inside the first block, on column 64 and inside the second"""
    for n in pr.WIDE_APPLY_N:
        for split in pr.WIDE_APPLY_SPLITS:
            if split >= n:
                continue
            a, z, ref = _exact_apply_operands(np.random.default_rng(m * 7 + n + split + engine), m, n, split)
            for inplace in (False, True):
                q = apply_wide(st, engine, a, pr.zw_of(z, n), inplace)
                assert np.array_equal(q, ref), (n, split, inplace, np.argwhere(q != ref)[:5])


@pytest.mark.parametrize("wgs_over", [0, 1, 2])
@pytest.mark.parametrize("engine", [0, 1, 2])
def test_apply_wide_exact_workgroup_override(st, engine, wgs_over):
    """m = 449: four 128-row blocks (eight 64-row blocks for the fp32 kernel) on one workgroup -- the block loop with both prefetch
    registers in use --, on two, and on the product's grid"""
    L, torch = st
    m = 449
    p = plan(L, m, 128, m)
    assert (p["blk128"], p["blk64"]) == (4, 8)
    for n, split in [(128, 70), (100, 17)]:
        a, z, ref = _exact_apply_operands(np.random.default_rng(n + engine + wgs_over), m, n, split)
        for inplace in (False, True):
            q = apply_wide(st, engine, a, pr.zw_of(z, n), inplace, wgs_over)
            assert np.array_equal(q, ref), (n, inplace, np.argwhere(q != ref)[:5])


@pytest.mark.parametrize("engine", [0, 1, 2])
def test_apply_wide_skips_on_rejection_and_refuses_bad_shapes(st, engine):
    """a non-zero skip_status leaves Q entirely sentinel; ld < m, n outside 65 .. 128 and an unknown engine are refused"""
    L, torch = st
    a, z, _ = _exact_apply_operands(np.random.default_rng(engine), 129, 100, 17)
    q = apply_wide(st, engine, a, pr.zw_of(z, 100), False, skip=1)
    assert np.all(q == SENT)
    buf = torch.zeros(129 * 128 + 128 * 128, device="cuda")
    p = buf.data_ptr()
    assert L.tsqr_selftest_w_apply(engine, p, 128, p, 129, 129, 100, p, None, 0) == -100
    assert L.tsqr_selftest_w_apply(engine, p, 129, p, 128, 129, 100, p, None, 0) == -100
    assert L.tsqr_selftest_w_apply(engine, p, 129, p, 129, 129, 64, p, None, 0) == -100
    assert L.tsqr_selftest_w_apply(engine, p, 129, p, 129, 129, 129, p, None, 0) == -100
    assert L.tsqr_selftest_w_apply(3, p, 129, p, 129, 129, 100, p, None, 0) == -100
    assert L.tsqr_selftest_w_apply(engine, p, 129, p, 129, 129, 100, p, None, -1) == -100


@pytest.mark.parametrize("n", [128, 100])
@pytest.mark.parametrize("engine", [0, 1, 2])
def test_apply_wide_single_products(st, engine, n):
    """one non-zero (full mantissa) per row of A, in column i mod n (every row k of Z is met in three different row positions), times a
    dense full-mantissa upper-triangular Z: every Q_ij is ONE product a z.  Engine 0 must give fl32(a z) bit for bit -- in every (k, j)
    slot of its compact triangular Z --, engines 1 and 2 stay within pass_refs.apply_single_product_bound"""
    m = 449
    rng = np.random.default_rng(n + 10 * engine)
    a = np.zeros((m, n), np.float32)
    a[np.arange(m), np.arange(m) % n] = pr.full_mantissa(rng, m, 6)
    z = np.triu(pr.full_mantissa(rng, (n, n), 3)).astype(np.float64)
    q = apply_wide(st, engine, a, pr.zw_of(z, n), False)
    exact = a.astype(np.float64) @ z                                    # one product per entry: exact in fp64
    if engine == 0:
        want = exact.astype(np.float32)
        assert np.array_equal(q, want), np.argwhere(q != want)[:5]
    else:
        report("apply wide engine %d single products n=%d" % (engine, n), np.abs(q - exact), pr.apply_single_product_bound(engine, exact))


# =========================================================================================================================================
# 4. Panel coupling: cross_kernel, cross_reduce_multi_kernel, cross_finish_kernel, the update instance
# =========================================================================================================================================
def cross_plan(L, m, nwaves_over=0):
    out = (ctypes.c_longlong * 7)()
    assert L.tsqr_selftest_cross_plan(m, nwaves_over, ctypes.cast(out, c_p)) == 0
    return dict(zip("nch cpw nwaves nblocks rows_per_wg gstride part".split(), out))


def cross(st, x, y, fused, slots_panels=None, nwaves_over=0):
    """-> (R block row 64 x ny_total, S_neg list of 64 x 64 [row, column] per trailing panel, the plan).  slots_panels: the trailing panels
    the partial buffer holds workgroup partials for (None: all of them -- one launch)"""
    L, torch = st
    m, ny = y.shape
    ntr = -(-ny // 64)
    p = cross_plan(L, m, nwaves_over)
    xpool, xp = upload(torch, x, m + 3, pad=NAN)
    ypool, yp = upload(torch, y, m + 5, pad=NAN)
    ldr = 64 + 3
    rpool, rp = out_pool(torch, 64, ny, ldr, fill=SENT)
    zneg = torch.full((ntr * 4096 + 16,), SENT, device="cuda")
    gm = torch.full((ntr * p["gstride"] + 16,), SENT, dtype=torch.float64, device="cuda")
    cap = (slots_panels or ntr) * p["nblocks"] * p["part"]
    part = torch.full((cap + 16,), SENT, dtype=torch.float64, device="cuda")
    rc = L.tsqr_selftest_cross(rp, ldr, zneg.data_ptr(), gm.data_ptr(), xp, m + 3, yp, m + 5, m, ny, part.data_ptr(), cap, fused, nwaves_over)
    assert rc == 0, rc
    assert np.all(padding_of(rpool, 64, ny, ldr) == SENT)
    zh = zneg.cpu().numpy()
    assert np.all(zh[ntr * 4096:] == SENT) and np.all(part[cap:].cpu().numpy() == SENT) and np.all(gm[ntr * p["gstride"]:].cpu().numpy() == SENT)
    return download(rpool, 64, ny, ldr), [zh[4096 * j: 4096 * (j + 1)].reshape(64, 64).T for j in range(ntr)], p


def check_cross(r, sneg, want, ny):
    """R block row == want (64 x ny) and slice j of zneg == -want's panel j, exact zeros in the columns beyond a ragged last panel"""
    assert np.array_equal(r, want), np.argwhere(r != want)[:5]
    for j, sj in enumerate(sneg):
        w = min(64, ny - 64 * j)
        ref = np.zeros((64, 64), np.float32)
        ref[:, :w] = -want[:, 64 * j: 64 * j + w]
        assert np.array_equal(sj, ref), (j, np.argwhere(sj != ref)[:5])
        assert not np.any(np.signbit(sj[:, w:]))                      # +0, as cross_finish_kernel and the fused finish write it


@pytest.mark.parametrize("m", pr.CROSS_M)
def test_cross_exact_fused_and_two_launch_forms(st, m):
    """X, Y integers |k| <= 63: the budget of pass_refs.cross_exact_budget asserted from the plan entry (a workgroup sums rows_per_wg
    rows in fp32), then the R block row equals fl32(X^T Y), every 64 x 64 slice of zneg equals -S with exact zeros beyond a ragged last
    panel, sentinels intact, and the fused (one-GPU) and two-launch (row-partitioned) forms give the same bits.  ny_total = 130 and 197
    also with partials for two panels only: grouped launches, the last group with one ragged panel (130: 2 + 1; 197: 2 + 2)."""
    L, torch = st
    rng = np.random.default_rng(m)
    x = pr.exact_ints(rng, m, 64, kmax=63, exps=(0, 0))
    for ny in pr.CROSS_NY:
        y = pr.exact_ints(rng, m, ny, kmax=63, exps=(0, 0))
        want = (x.astype(np.float64).T @ y.astype(np.float64)).astype(np.float32)
        for slots in ([None, 2] if ny > 128 else [None]):
            outs = []
            for fused in (1, 0):
                r, sneg, p = cross(st, x, y, fused, slots)
                assert all(b <= lim for b, lim in zip(pr.cross_exact_budget(63, m, p["rows_per_wg"]), (24, 53)))
                check_cross(r, sneg, want, ny)
                outs.append((r, sneg))
            assert np.array_equal(outs[0][0], outs[1][0]) and all(np.array_equal(a, b) for a, b in zip(outs[0][1], outs[1][1]))


@pytest.mark.parametrize("nwaves_over", [1, 3, 5])
def test_cross_exact_wave_override(st, nwaves_over):
    """4097 rows on one, three and five waves (cpw = 65, 22, 13: several chunks per wave, waves of the last workgroup without a chunk, a
    ragged last chunk); the budget from the plan still holds (all 4097 rows in one fp32 sum stay below 2^24)"""
    m, ny = 4097, 70
    rng = np.random.default_rng(nwaves_over)
    x = pr.exact_ints(rng, m, 64, kmax=63, exps=(0, 0))
    y = pr.exact_ints(rng, m, ny, kmax=63, exps=(0, 0))
    want = (x.astype(np.float64).T @ y.astype(np.float64)).astype(np.float32)
    for fused in (1, 0):
        r, sneg, p = cross(st, x, y, fused, None, nwaves_over)
        assert p["nwaves"] <= nwaves_over and p["cpw"] == -(-65 // nwaves_over)
        assert all(b <= lim for b, lim in zip(pr.cross_exact_budget(63, m, p["rows_per_wg"]), (24, 53)))
        check_cross(r, sneg, want, ny)


def test_cross_isolated_products(st):
    """one non-zero row (full mantissas) per wave's range, taken from the plan (cpw chunks of 64 rows), X and Y in the same rows: every
    wave's chain holds one product per entry -- within pass_refs.cross_isolated_bound; a dropped product of the split errs near 2^-16"""
    L, torch = st
    m, ny = 1000, 70
    p = cross_plan(L, m)
    rng = np.random.default_rng(11)
    x = pr.isolated_rows(rng, m, 64, stretch=64 * p["cpw"], spread=6)
    rows = np.flatnonzero(np.any(x != 0, axis=1))
    y = np.zeros((m, ny), np.float32)
    y[rows] = pr.full_mantissa(rng, (rows.size, ny), 6)
    r, sneg, p = cross(st, x, y, 1)
    exact = x[rows].astype(np.float64).T @ y[rows].astype(np.float64)
    report("cross isolated m=%d ny=%d" % (m, ny), np.abs(r - exact), pr.cross_isolated_bound(x, y, m, p["nblocks"]))
    assert np.array_equal(sneg[0], -r[:, :64])


@pytest.mark.parametrize("engine", [0, 1, 2])
def test_update_exact(st, engine):
    """Y_j - X S_j for every trailing panel with the last one ragged (ny_total = 150: 64 + 64 + 22), X integers |x| <= 63, S integers
    |s| <= 7, Y integers |y| <= 63: every product and sum is an integer below 2^24, exact in the three engines.  wgs_over = 6 on m = 449
    (four 128-row blocks): two workgroups per panel, the grid really splits over the panels; 0: the product's grid.  Two further columns
    behind ny_total keep their sentinel, as does the leading-dimension padding."""
    L, torch = st
    m, ny, extra = 449, 150, 2
    rng = np.random.default_rng(engine)
    x = pr.exact_ints(rng, m, 64, kmax=63, exps=(0, 0))
    y = pr.exact_ints(rng, m, ny, kmax=63, exps=(0, 0))
    sm = rng.integers(-7, 8, size=(64, ny)).astype(np.float64)
    assert int(63 * (1 + 64 * 7)).bit_length() <= 24
    zneg = np.zeros((3, 64, 64), np.float32)                            # slice j: zneg[j][column][row] = -S_j[row][column]
    for j in range(3):
        w = min(64, ny - 64 * j)
        zneg[j, :w, :] = -sm[:, 64 * j: 64 * j + w].T
    want = y.astype(np.float64) - x.astype(np.float64) @ sm
    for wgs_over in (6, 0):
        xpool, xp = upload(torch, x, m + 3, pad=NAN)
        ypad = np.concatenate([y, np.full((m, extra), SENT, np.float32)], axis=1)
        ypool, yp = upload(torch, ypad, m + 5, pad=SENT)
        zt = torch.from_numpy(zneg.reshape(-1)).cuda()
        rc = L.tsqr_selftest_update(engine, yp, m + 5, xp, m + 3, m, zt.data_ptr(), ny, wgs_over)
        assert rc == 0, rc
        got = download(ypool, m, ny + extra, m + 5)
        assert np.array_equal(got[:, :ny], want), np.argwhere(got[:, :ny] != want)[:5]
        assert np.all(got[:, ny:] == SENT) and np.all(padding_of(ypool, m, ny + extra, m + 5) == SENT)
        assert np.array_equal(download(xpool, m, 64, m + 3), x)
    assert L.tsqr_selftest_update(engine, yp, m - 1, xp, m + 3, m, zt.data_ptr(), ny, 0) == -100
    assert L.tsqr_selftest_update(3, yp, m + 5, xp, m + 3, m, zt.data_ptr(), ny, 0) == -100
    assert L.tsqr_selftest_update(engine, yp, m + 5, xp, m + 3, m, zt.data_ptr(), 0, 0) == -100


# =========================================================================================================================================
# 5. Native half-typed path: gram_h_kernel, apply_wg_h_kernel
# =========================================================================================================================================
def up16(torch, a, ld, pad=NAN):
    return upload(torch, a.astype(np.float16), ld, pad=pad, dtype=np.float16)


@pytest.mark.parametrize("m", pr.HALF_GRAM_M)
def test_half_gram_exact_bit_for_bit(st, m):
    """half operands k 2^e_j, |k| <= 511 (pass_refs.exact_halves: the budget for an 11-bit significand and a 64-row chain asserted),
    lda the next multiple of 8 above m with NaN halves in the padding: G bit for bit, zeros beyond n; also on one and three waves"""
    L, torch = st
    lda = m + 8 - m % 8
    for n in pr.HALF_N:
        a = pr.exact_halves(np.random.default_rng(100 * m + n), m, n)
        ref = a.astype(np.float64).T @ a.astype(np.float64)
        pool, ap = up16(torch, a, lda)
        ntri = pr.gram_elems(n) // 256
        for nwaves_over in (0, 1, 3):
            p = cross_plan(L, m, nwaves_over)                              # (the same gram_plan: the wave count does not depend on n)
            cap = p["nblocks"] * ntri * 256
            part = torch.full((cap + 16,), SENT, dtype=torch.float64, device="cuda")
            gs = torch.full((ntri * 256 + 1 + 8,), SENT, dtype=torch.float64, device="cuda")
            rc = L.tsqr_selftest_h_gram(gs.data_ptr(), ap, lda, m, n, part.data_ptr(), cap, nwaves_over)
            assert rc == 0, rc
            g = gs.cpu().numpy()
            assert g[ntri * 256] == float(m) and np.all(g[ntri * 256 + 1:] == SENT) and np.all(part[cap:].cpu().numpy() == SENT)
            gg = pr.unpack_tiles(g[:ntri * 256], n, True)
            want = np.zeros_like(gg)
            want[:n, :n] = ref
            assert np.array_equal(gg, want), (n, nwaves_over, np.argwhere(gg != want)[:5])
        assert L.tsqr_selftest_h_gram(gs.data_ptr(), ap, lda, m, n, part.data_ptr(), cap - 1, 3) == -100
        assert L.tsqr_selftest_h_gram(gs.data_ptr(), ap, lda + 4, m, n, part.data_ptr(), cap, 3) == -100
        assert L.tsqr_selftest_h_gram(gs.data_ptr(), ap + 2, lda, m, n, part.data_ptr(), cap, 3) == -100
        assert L.tsqr_selftest_h_gram(gs.data_ptr(), ap, lda, m, 16, part.data_ptr(), cap, 3) == -100


@pytest.mark.parametrize("wgs_over", [0, 1, 2])
@pytest.mark.parametrize("engine", [1, 2])
def test_half_apply_rounds_to_nearest_even(st, engine, wgs_over):
    """A integers |a| <= 63 (halves), Z = 2^-3 [[I, -B], [0, I]] with |b| <= 63: Q 2^3 = a_j - sum_i a_i b_ij is an integer of up to 17
    bits -- exact in the fp32 accumulator (below 2^24) but NOT always representable in fp16, and below 65504 / 8 x 8 in magnitude: Q must
    equal np.float16(exact), round to nearest even of the exactly computed value; a truncating narrowing differs in about half the
    entries.  m = 449 on the product's grid, one and two workgroups; out of place, ldq != lda (multiples of 4), NaN / sentinel padding.
    r16 must equal np.float16(r32) over the whole n x n block -- with an entry above 65504, which comes back as inf -- ldr16 padding intact."""
    L, torch = st
    m = 449
    for n, split in [(64, 20), (33, 16), (17, 5), (48, 23)]:
        rng = np.random.default_rng(n + engine + wgs_over)
        _, z = pr.exact_inverse_pair(rng, n, split, bmax=63, scale_exp=0)
        z = z / 8.0
        a = pr.exact_ints(rng, m, n, kmax=63, exps=(0, 0))
        exact = a.astype(np.float64) @ z
        assert int(63 * (1 + split * 63)).bit_length() <= 24 and np.max(np.abs(exact)) < 65504
        want = exact.astype(np.float16)
        assert np.any(want.astype(np.float64) != exact)                   # the rounding is exercised
        np_ = 16 * pr.ntiles(n)
        zp = np.zeros((np_, np_), np.float32)
        zp[:n, :n] = z
        zt = torch.from_numpy(np.ascontiguousarray(zp.T).reshape(-1)).cuda()
        lda, ldq, ldr16 = m + 3, m + 7, n + 3
        apool, ap = up16(torch, a, lda)
        qpool, qp = out_pool(torch, m, n, ldq, fill=SENT, dtype=torch.float16)
        r32 = pr.full_mantissa(rng, (n, n), 10)                             # packed, ld n: the kernel narrows every entry
        r32[0, 0], r32[n - 1, 1], r32[2, n - 1] = 65520.0, -1e6, 65504.0    # rounds up to inf, far beyond, the largest half
        rt = torch.from_numpy(np.ascontiguousarray(r32.T).reshape(-1)).cuda()   # column-major, ld n
        r16pool, r16p = out_pool(torch, n, n, ldr16, fill=SENT, dtype=torch.float16)
        rc = L.tsqr_selftest_h_apply(engine, qp, ldq, ap, lda, m, n, zt.data_ptr(), rt.data_ptr(), r16p, ldr16, wgs_over)
        assert rc == 0, rc
        q = download(qpool, m, n, ldq)
        assert np.array_equal(q, want), (n, np.argwhere(q != want)[:5])
        assert np.all(padding_of(qpool, m, n, ldq) == np.float16(SENT))
        assert np.array_equal(download(apool, m, n, lda), a.astype(np.float16))
        r16 = download(r16pool, n, n, ldr16)
        with np.errstate(over="ignore"):
            want16 = r32.astype(np.float16)
        assert np.isinf(want16[0, 0]) and np.isinf(want16[n - 1, 1]) and want16[2, n - 1] == np.float16(65504.0)
        assert np.array_equal(r16, want16), np.argwhere(r16 != want16)[:5]
        assert np.all(padding_of(r16pool, n, n, ldr16) == np.float16(SENT))
    assert L.tsqr_selftest_h_apply(engine, qp, ldq + 1, ap, lda, m, n, zt.data_ptr(), None, None, 0, 0) == -100
    assert L.tsqr_selftest_h_apply(0, qp, ldq, ap, lda, m, n, zt.data_ptr(), None, None, 0, 0) == -100
    assert L.tsqr_selftest_h_apply(engine, qp, ldq, ap, lda, m, 16, zt.data_ptr(), None, None, 0, 0) == -100

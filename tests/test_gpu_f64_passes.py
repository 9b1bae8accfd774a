"""Each pass of the fp64 entries on its own, through the test library's tsqr_selftest_f64_* entries (tsqr_gpu_amd/csrc/selftest_f64.hip:
the product's kernels launched with the product's plan, f64_plan.h), against exact data bit for bit or extended-precision references:

  n <= 64       gram_f64_kernel + gram_reduce1_kernel, chol_f64_kernel, apply_f64_kernel<NT>, trimul_f64_kernel
  64 < n <= 1024 gram_wide_f64_kernel + reduction, the blocked Cholesky chain (plain, shifted, both as the product enqueues them),
                apply_wide_f64_kernel, rcopy_wide_f64_kernel, rsave_ + rmul_wide_f64_kernel

Operands carry NaN in the leading-dimension padding and behind the last column, outputs a sentinel in their padding, base pointers are
offset by one double (8-byte, not 16-byte aligned) with odd leading dimensions next to aligned ones.  Bounds, generators and their
derivations: tests/pass_refs_f64.py.  Every bounded check prints max(measured / bound)."""
import ctypes
import os

import numpy as np
import pytest

from tests import pass_refs as pr
from tests import pass_refs_f64 as p64
from tests.test_gpu_passes import download, padding_of, report, upload

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
SENT = -777.0
LD = np.longdouble
c_sz, c_p, c_i = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int


@pytest.fixture(scope="module")
def st():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    L = ctypes.CDLL(os.path.join(ROOT, "tsqr_gpu_amd", "csrc", "libtsqr_selftest.so"))
    sig = {
        "tsqr_selftest_f64_plan": [c_sz, c_sz, c_p], "tsqr_selftest_f64w_plan": [c_sz, c_sz, c_p],
        "tsqr_selftest_f64_gram": [c_p, c_p, c_sz, c_sz, c_i, c_p, c_sz, c_i],
        "tsqr_selftest_f64_chol": [c_p, c_sz, c_p, c_p, c_p, c_p, c_sz, c_i, c_i],
        "tsqr_selftest_f64_apply": [c_p, c_sz, c_p, c_sz, c_sz, c_i, c_p, c_i],
        "tsqr_selftest_f64_rmul": [c_p, c_sz, c_p, c_i],
        "tsqr_selftest_f64w_gram": [c_p, c_p, c_sz, c_sz, c_i, c_p, c_sz, c_sz],
        "tsqr_selftest_f64w_chain": [c_p, c_sz, c_i, c_i, c_p],
        "tsqr_selftest_f64w_apply": [c_p, c_sz, c_p, c_sz, c_sz, c_i, c_p],
        "tsqr_selftest_f64w_rcopy": [c_p, c_sz, c_p, c_i],
        "tsqr_selftest_f64w_rmul": [c_p, c_sz, c_p, c_p, c_i],
    }
    for name, args in sig.items():
        getattr(L, name).restype = c_i
        getattr(L, name).argtypes = args
    return L, torch


def up64(torch, a, ld, offset=0, pad=NAN):
    return upload(torch, np.asarray(a, np.float64), ld, pad=pad, offset=offset, slack=16, dtype=np.float64)


def dev(torch, v):
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).cuda()


def narrow_plan(L, m, n):
    out = (ctypes.c_longlong * 8)()
    assert L.tsqr_selftest_f64_plan(m, n, ctypes.cast(out, c_p)) == 0
    return list(out)


def wide_plan(L, m, n):
    out = (ctypes.c_longlong * 20)()
    assert L.tsqr_selftest_f64w_plan(m, n, ctypes.cast(out, c_p)) == 0
    keys = "nb npairs ngroups nslices cps nch bs o_gs o_w o_rw o_zw o_ta o_rc o_zd o_sb o_bst o_status wq wr cap".split()
    return dict(zip(keys, out))


# =========================================================================================================================================
# n <= 64
# =========================================================================================================================================
def gram_narrow(st, a, lda, offset, nwaves=0):
    L, torch = st
    m, n = a.shape
    pool, ap = up64(torch, a, lda, offset)
    ntri = pr.gram_elems(n) // 256
    nblocks = (nwaves + 3) // 4 if nwaves else narrow_plan(L, m, n)[4]
    cap = nblocks * ntri * 256
    part = torch.full((cap + 8,), SENT, dtype=torch.float64, device="cuda")
    gs = torch.full((ntri * 256 + 1 + 8,), SENT, dtype=torch.float64, device="cuda")
    rc = L.tsqr_selftest_f64_gram(gs.data_ptr(), ap, lda, m, n, part.data_ptr(), cap, nwaves)
    assert rc == 0, rc
    g = gs.cpu().numpy()
    assert g[ntri * 256] == float(m) and np.all(g[ntri * 256 + 1:] == SENT) and np.all(part[cap:].cpu().numpy() == SENT)
    return pr.unpack_tiles(g[:ntri * 256], n, False)


def padded(g, np_):
    out = np.zeros((np_, np_))
    out[:g.shape[0], :g.shape[1]] = g
    return out


GRAM_M = [1, 63, 64, 65, 127, 129, 4097, 9211]
GRAM_N = [1, 7, 16, 17, 33, 48, 51, 63, 64]


@pytest.mark.parametrize("m", GRAM_M)
def test_gram_exact_bit_for_bit(st, m):
    """exact integers (pass_refs_f64.exact_ints64, m kmax^2 < 2^53 asserted): the summed tiles equal A^T A bit for bit, the tiles of
    columns >= n are exact zeros; base pointer 8-byte aligned only and lda odd for odd n, aligned for even n"""
    for n in GRAM_N:
        a = p64.exact_ints64(np.random.default_rng(1000 * m + n), m, n)
        odd = n & 1
        g = gram_narrow(st, a, m + 3 if odd else m + (-m) % 2, odd)
        assert np.array_equal(g, padded(p64.gram_exact(a), g.shape[0])), (m, n)


@pytest.mark.parametrize("nwaves", [1, 3, 5])
@pytest.mark.parametrize("m,n", [(65, 17), (333, 64), (1029, 33)])
def test_gram_exact_wave_override(st, m, n, nwaves):
    """one, three, five waves: several chunks per wave, waves of the last workgroup without a chunk, a ragged last chunk"""
    a = p64.exact_ints64(np.random.default_rng(m + n + nwaves), m, n)
    g = gram_narrow(st, a, m + 1, 1, nwaves)
    assert np.array_equal(g, padded(p64.gram_exact(a), g.shape[0]))


@pytest.mark.parametrize("m,n", [((1 << 17) + 64, 64), (1 << 20, 64), (1 << 23, 16)])
def test_gram_exact_product_plan_large(st, m, n):
    """the product's plan where a wave takes two and more chunks; data generated on the device (integers, budget asserted)"""
    L, torch = st
    kmax = p64.kmax_for(m)
    p64.assert_gram_budget(kmax, m)
    gen = torch.Generator(device="cuda").manual_seed(m + n)
    a = torch.randint(-kmax, kmax + 1, (n, m), generator=gen, device="cuda", dtype=torch.int32).double()
    ntri = pr.gram_elems(n) // 256
    plan = narrow_plan(L, m, n)
    part = torch.empty(plan[6], dtype=torch.float64, device="cuda")
    gs = torch.full((ntri * 256 + 1,), SENT, dtype=torch.float64, device="cuda")
    assert L.tsqr_selftest_f64_gram(gs.data_ptr(), a.data_ptr(), m, m, n, part.data_ptr(), plan[6], 0) == 0
    ref = torch.zeros(n, n, dtype=torch.float64, device="cuda")
    for r0 in range(0, m, 1 << 18):                      # exact in any order: torch's fp64 product is a reference
        blk = a[:, r0:r0 + (1 << 18)]
        ref += blk @ blk.T
    g = pr.unpack_tiles(gs.cpu().numpy()[:ntri * 256], n, False)
    assert np.array_equal(g, padded(ref.cpu().numpy(), g.shape[0]))


@pytest.mark.parametrize("kind", ["gauss", "same_sign"])
@pytest.mark.parametrize("m,n", [(4097, 33), (1 << 20, 64)])
def test_gram_dense_bound(st, m, n, kind):
    """dense data against longdouble, per entry.  4097 x 33: one chunk per wave, a ragged last chunk.  2^20 x 64: eight chunks per wave in
    one MFMA chain and 512 partials through the reduction; the longdouble product is taken for six rows of G, one or two in each row of tiles"""
    rng = np.random.default_rng(7)
    a = rng.standard_normal((m, n)) if kind == "gauss" else rng.uniform(0.5, 1.5, (m, n))
    g = gram_narrow(st, a, m + 3, 1)[:n, :n]
    rows = np.arange(n) if m * n * n <= 1 << 28 else np.array([0, 15, 16, 31, 47, 63])
    err = np.asarray(g[rows].astype(LD) - p64.matmul_ld(a[:, rows].T, a), np.float64)
    path = p64.gram_path_narrow(m)
    report("gram_f64 %s %d x %d, path %d" % (kind, m, n, path), np.abs(err), p64.gram_bound(a, path)[rows])


def chol_narrow(st, g, n, m=1 << 20, first=1, ldr=None):
    L, torch = st
    NP = 16 * pr.ntiles(n)
    ldr = ldr or n + 3
    gs = dev(torch, pr.pack_tiles(g, n, False))
    r = torch.full((n * ldr,), SENT, dtype=torch.float64, device="cuda")
    z = torch.full((NP * NP + 8,), SENT, dtype=torch.float64, device="cuda")
    status = torch.full((8,), 77, dtype=torch.int32, device="cuda")
    hw = torch.full((8,), 77, dtype=torch.int32, device="cuda")
    assert L.tsqr_selftest_f64_chol(r.data_ptr(), ldr, z.data_ptr(), status.data_ptr(), hw.data_ptr(), gs.data_ptr(), m, n, first) == 0
    rh = r.cpu().numpy().reshape(n, ldr)
    assert np.all(rh[:, n:] == SENT), "R's padding was written"
    zh = z.cpu().numpy()
    assert np.all(zh[NP * NP:] == SENT)
    s, h = status.cpu().numpy().view(np.uint32), hw.cpu().numpy().view(np.uint32)
    assert np.array_equal(s[:4], h[:4]) and np.all(s[4:] == 77) and np.all(h[4:] == 77)
    words = (int(s[0]), float(s[1:2].view(np.float32)[0]), float(s[2:3].view(np.float32)[0]), int(s[3]))
    return rh[:, :n].T.copy(), zh[:NP * NP].reshape(NP, NP).T.copy(), words


@pytest.mark.parametrize("n", [64, 51, 48, 33, 17, 16, 5, 1])
def test_chol_residual_bounds_and_pivot_error(st, n):
    """|G - R^T R| and |Z R - I| per entry (pass_refs_f64.chol_bounds) for cond(G) 1 .. 1e6 (cond(A) 1 .. 1e3) with column scaling; R's strict lower triangle
    and Z's padding exact zeros; S and the pivot ratio against longdouble where S <= 100; the measured pivot error d is printed"""
    worst_d = 0.0
    for cond in (1.0, 30.0, 1e3):
        g, _ = p64.spd(n, cond, 10 * n + int(np.log10(cond)))
        R, Z, (v, ratio, scond, _) = chol_narrow(st, g, n)
        assert v == 0
        assert np.all(np.tril(R, -1) == 0.0) and np.all(np.tril(Z, -1) == 0.0) and np.all(Z[n:, :] == 0.0) and np.all(Z[:, n:] == 0.0)
        bg, bz = p64.chol_bounds(R, Z[:n, :n], n)
        eg = np.asarray(g.astype(LD) - p64.matmul_ld(R.T, R), np.float64)
        ez = np.asarray(p64.matmul_ld(Z[:n, :n], R) - np.eye(n), np.float64)
        report("chol_f64 n %d cond %.0e  |G - RtR|" % (n, cond), np.abs(np.triu(eg)), np.triu(bg) + np.tril(np.ones_like(bg), -1))
        report("chol_f64 n %d cond %.0e  |Z R - I|" % (n, cond), np.abs(ez), bz + (bz == 0))
        worst_d = max(worst_d, float(np.abs(p64.pivot_error(R, Z[:n, :n])).max()))
        s_ref, ratio_ref = p64.scond_ref(g)
        if s_ref <= 100:
            assert abs(scond - s_ref) <= 1e-4 * s_ref and abs(ratio - ratio_ref) <= 1e-5 * ratio_ref
    print("chol_f64 n %d: largest pivot error d = max |z_kk r_kk - 1| / 2 = %.3g (e_rsq bound %.3g, u = %.3g)" % (n, worst_d, p64.E_RSQ, p64.U))
    assert worst_d <= p64.E_RSQ + 2 * p64.U


def test_chol_verdicts_thresholds_and_shift(st):
    n = 64
    g, _ = p64.spd(n, 3.0, 1)
    assert chol_narrow(st, g, n)[2][0] == 0
    for bad in (np.nan, np.inf):
        gb = g.copy(); gb[3, 3] = bad
        assert chol_narrow(st, gb, n)[2][0] == 1
    m = 1 << 18
    max_scond, alone_max, coef = p64.rule(m, n)
    for gd in ("dependent", "zero"):
        g2 = g.copy()
        if gd == "dependent":
            g2[:, 7] = g2[:, 6]; g2[7, :] = g2[6, :]
        else:
            g2[:, 9] = 0.0; g2[9, :] = 0.0
        R, Z, (v, _, _, one) = chol_narrow(st, g2, n, m=m)
        assert v == 2 and one == 0 and np.all(np.isfinite(R)) and np.all(np.isfinite(Z))
        s = coef * np.trace(g2)
        # the backward residual of the SHIFTED matrix: s is ~1e-8 n of a diagonal entry, the bound ~1e-13 of it -- a wrong coefficient,
        # trace or set of shifted entries is far outside (tests/test_pass_refs_f64.py::test_shift_check_bites)
        report("chol_f64 shifted (%s)  |G + sI - RtR|" % gd, np.triu(p64.shift_residual(g2, s, R)),
               np.triu(p64.chol_bounds(R, Z, n)[0]) + np.tril(np.ones((n, n)), -1))
    # thresholds: S on either side of alone_max (word [3]) and of max_scond (verdict) -- S_ref from longdouble, margins 2 and 4
    seen = set()
    for cond in (10.0, 300.0, 1e5, 1e7):
        g3, _ = p64.spd(n, cond, int(cond) % 1000 + 5)
        s_ref, _ = p64.scond_ref(g3)
        for mm in (4096, 1 << 23):
            mx, al, _ = p64.rule(mm, n)
            if al / 2 <= s_ref <= 2 * al or mx / 4 <= s_ref <= 4 * mx:
                continue
            v, _, scond, one = chol_narrow(st, g3, n, m=mm)[2]
            assert v == (0 if s_ref <= mx else 2), (cond, mm, s_ref, mx)
            assert one == (1 if s_ref <= min(al, mx) else 0), (cond, mm, s_ref, al)
            seen.add((v, one))
            if v == 0 and s_ref <= 100:
                assert abs(scond - s_ref) <= 1e-4 * s_ref
    assert seen == {(0, 1), (0, 0), (2, 0)}, seen         # every outcome was reached: no side of a threshold went untested
    # a later sweep (first = 0): no bound on S, never accepted alone
    g4, _ = p64.spd(n, 1e5, 9)
    assert chol_narrow(st, g4, n, m=1 << 23, first=1)[2][0] == 2
    v, _, _, one = chol_narrow(st, g4, n, m=1 << 23, first=0)[2]
    assert v == 0 and one == 0


def floor_matrix(n, target):
    """SPD G = R^T R (longdouble, rounded to fp64) whose LAST pivot ratio r_nn^2 / g_nn is `target`, every other one that of a
    well-conditioned matrix: R is the factor of spd(n, 3) with its last diagonal entry set from r_nn^2 = target c / (1 - target),
    c the squared norm of the rest of the last column"""
    g0, _ = p64.spd(n, 3.0, 1)
    r = p64.chol_ld(g0)
    c = np.sum(r[:n - 1, n - 1] ** 2)
    r[n - 1, n - 1] = np.sqrt(LD(target) * c / (LD(1) - LD(target)))
    return np.asarray(r.T @ r, np.float64)                 # (longdouble product, symmetric term by term, rounded once)


@pytest.mark.parametrize("n", [64, 17])
def test_chol_pivot_floor_of_every_plain_factorisation(st, n):
    """F64_MIN_PIVOT_RATIO = 2^-40 (CholArgs64): a later sweep (first = 0, no bound on S) whose smallest pivot ratio is 1.5 times above
    the floor is accepted, one 1.5 times below it is factored shifted -- at the smallest and the largest row count alike: the floor does
    not depend on the shape.  (The kernel's pivot carries about n u / ratio = 1 % of rounding at the floor: the margin 1.5 is a
    condition.)  The ratios are checked in longdouble first."""
    floor = 2.0 ** -40
    for factor, want in ((1.5, 0), (1.0 / 1.5, 2)):
        g = floor_matrix(n, factor * floor)
        ratio_ref = p64.scond_ref(g)[1]
        assert abs(ratio_ref - factor * floor) <= 0.02 * factor * floor, (ratio_ref, factor * floor)
        for m in (4096, 1 << 23):
            v, ratio, _, one = chol_narrow(st, g, n, m=m, first=0)[2]
            print("n %d m %d: pivot ratio %.3g (longdouble %.3g, floor %.3g): verdict %d" % (n, m, ratio, ratio_ref, floor, v))
            assert v == want and one == 0, (n, m, factor, v)
            if want == 0:
                assert abs(ratio - ratio_ref) <= 0.05 * ratio_ref


def apply_narrow(st, a, z, ld_pad, offset, wgs=0, in_place=False):
    L, torch = st
    m, n = a.shape
    NP = 16 * pr.ntiles(n)
    zp = dev(torch, padded(z, NP).T.reshape(-1))
    lda = m + ld_pad
    apool, ap = up64(torch, a, lda, offset)
    if in_place:
        assert L.tsqr_selftest_f64_apply(ap, lda, ap, lda, m, n, zp.data_ptr(), wgs) == 0
        pad = padding_of(apool, m, n, lda, offset)
        assert np.all(np.isnan(pad)), "in place: the padding of A was written"
        return download(apool, m, n, lda, offset)
    ldq = m + ld_pad + 2
    qpool, qp = up64(torch, np.full((m, n), SENT), ldq, offset, pad=SENT)
    assert L.tsqr_selftest_f64_apply(qp, ldq, ap, lda, m, n, zp.data_ptr(), wgs) == 0
    assert np.all(padding_of(qpool, m, n, ldq, offset) == SENT), "Q's padding was written"
    return download(qpool, m, n, ldq, offset)


@pytest.mark.parametrize("n,split", [(64, 32), (51, 17), (33, 16), (16, 5), (7, 3)])
def test_apply_exact_bit_for_bit(st, n, split):
    """integer A times an exact inverse pair (budget asserted): bit for bit for every m mod 32 tail, unaligned and aligned operands, in
    place equal to out of place, one and three workgroups striding many blocks, and the product's grid"""
    rng = np.random.default_rng(n)
    amax = bmax = (1 << 20) - 1
    p64.assert_apply_budget(amax, split, bmax)
    _, z = p64.exact_inverse_pair64(rng, n, split, bmax)
    base = 32 * -(-n // 32)                              # m = 32 k + tail >= n for every tail and every NT
    for m in [base + t for t in (0, 1, 15, 16, 17, 31)] + [1000 + 15, 4097]:
        a = rng.integers(-amax, amax + 1, size=(m, n)).astype(np.float64)
        ref = a @ z
        assert np.array_equal(ref.astype(LD), p64.matmul_ld(a, z))
        for wgs in (0, 1, 3):
            odd = (m + wgs) & 1
            q = apply_narrow(st, a, z, 3 if odd else (-m) % 2, odd, wgs)
            assert np.array_equal(q, ref), (m, n, wgs)
            assert np.array_equal(apply_narrow(st, a, z, 3 if odd else (-m) % 2, odd, wgs, in_place=True), ref), (m, n, wgs, "in place")


def test_apply_single_products_and_general_bound(st):
    rng = np.random.default_rng(3)
    n, m = 64, 1055
    a1 = p64.single_entry_rows64(rng, m, n)
    z1 = np.triu(p64.full_mantissa64(rng, (n, n), 3))
    assert np.array_equal(apply_narrow(st, a1, z1, 3, 1), p64.fl64_products(a1, z1))   # one product per entry: fl64(a z)
    for cond in (1.0, 1e4, 1e8):
        z = np.linalg.inv(np.triu(pr.random_triangular(rng, n, cond).astype(np.float64)))
        a = rng.standard_normal((m, n))
        q = apply_narrow(st, a, z, 1, 1)
        report("apply_f64 cond %.0e" % cond, np.abs(np.asarray(q.astype(LD) - p64.matmul_ld(a, z), np.float64)), p64.apply_bound(a, z))


def test_apply_product_grid_large(st):
    """2^20 x 64 with the product's persistent grid: every wave strides over many 32-row blocks"""
    L, torch = st
    m, n, amax = 1 << 20, 64, (1 << 20) - 1
    _, z = p64.exact_inverse_pair64(np.random.default_rng(1), n, 32)
    gen = torch.Generator(device="cuda").manual_seed(2)
    a = torch.randint(-amax, amax + 1, (n, m), generator=gen, device="cuda", dtype=torch.int32).double()
    zd = dev(torch, z.T.reshape(-1))
    q = torch.empty_like(a)
    assert L.tsqr_selftest_f64_apply(q.data_ptr(), m, a.data_ptr(), m, m, n, zd.data_ptr(), 0) == 0
    assert torch.equal(q, (a.T @ dev(torch, z)).T.contiguous())
    assert L.tsqr_selftest_f64_apply(a.data_ptr(), m, a.data_ptr(), m, m, n, zd.data_ptr(), 0) == 0
    assert torch.equal(a, q)


@pytest.mark.parametrize("n", [1, 7, 16, 17, 63, 64])
def test_rmul(st, n):
    L, torch = st
    rng = np.random.default_rng(n)
    for kind in ("int", "general"):
        r2, r1 = (p64.int_triangular(rng, n), p64.int_triangular(rng, n)) if kind == "int" else \
            (np.triu(rng.standard_normal((n, n))), np.triu(rng.standard_normal((n, n))))
        ldr = n + 3
        rpool, rp = up64(torch, r1 + np.tril(np.full((n, n), NAN), -1), ldr, 1, pad=SENT)   # NaN below the diagonal: never read
        r2d = dev(torch, padded(r2, 64).T.reshape(-1))
        assert L.tsqr_selftest_f64_rmul(rp, ldr, r2d.data_ptr(), n) == 0
        out = download(rpool, n, n, ldr, 1)
        assert np.all(padding_of(rpool, n, n, ldr, 1) == SENT) and np.all(np.tril(out, -1) == 0.0)
        if kind == "int":
            assert np.array_equal(out, r2 @ r1)
        else:
            report("rmul_f64 n %d" % n, np.abs(np.asarray(out.astype(LD) - p64.matmul_ld(r2, r1), np.float64)), p64.rmul_bound(r2, r1) + np.tril(np.ones((n, n)), -1))


# =========================================================================================================================================
# 64 < n <= 1024
# =========================================================================================================================================
def gram_wide(st, a, lda, offset, cps=0):
    L, torch = st
    m, n = a.shape
    pl = wide_plan(L, m, n)
    nslices = -(-pl["nch"] // cps) if cps else pl["nslices"]
    cap = nslices * pl["bs"]
    pool, ap = up64(torch, a, lda, offset)
    part = torch.full((cap + 8,), SENT, dtype=torch.float64, device="cuda")
    gs = torch.full((pl["bs"] + 1 + 8,), SENT, dtype=torch.float64, device="cuda")
    assert L.tsqr_selftest_f64w_gram(gs.data_ptr(), ap, lda, m, n, part.data_ptr(), cap, cps) == 0
    g = gs.cpu().numpy()
    assert g[pl["bs"]] == float(m) and np.all(g[pl["bs"] + 1:] == SENT) and np.all(part[cap:].cpu().numpy() == SENT)
    return g[:pl["bs"]]


@pytest.mark.parametrize("n", [65, 79, 100, 128, 129, 200])
def test_wide_gram_exact_slices(st, n):
    """slices of 1, 2, 3 and 4 chunks (both register sets, every exit of the rotation) with a ragged last slice and 16-row chunk tails
    (m mod 16 = 1, 15), then the product's plan: every block pair bit for bit, rows and columns >= n of the block store exact zeros"""
    for m, cps in ((209, 1), (209, 2), (223, 3), (209, 4), (225, 4), (200, 0), (1100 if n < 200 else 1101, 0)):
        a = p64.exact_ints64(np.random.default_rng(100 * n + m + cps), m, n)
        odd = (m + cps) & 1
        v = gram_wide(st, a, m + 3 if odd else m + (-m) % 2, odd, cps)
        assert np.array_equal(v, p64.pack_blocks(p64.gram_exact(a), n)), (m, n, cps)


@pytest.mark.parametrize("m,n", [(200, 65), (1100, 1024), (65536, 128), (1 << 16, 1024), (4097, 640), (2063, 1000)])
def test_wide_gram_exact_product_plan(st, m, n):
    L, torch = st
    kmax = p64.kmax_for(m)
    p64.assert_gram_budget(kmax, m)
    gen = torch.Generator(device="cuda").manual_seed(m + n)
    lda = m + 3
    a = torch.full((n, lda), NAN, dtype=torch.float64, device="cuda")
    a[:, :m] = torch.randint(-kmax, kmax + 1, (n, m), generator=gen, device="cuda", dtype=torch.int32).double()
    pl = wide_plan(L, m, n)
    part = torch.empty(pl["wr"], dtype=torch.float64, device="cuda")
    gs = torch.full((pl["bs"] + 1,), SENT, dtype=torch.float64, device="cuda")
    assert L.tsqr_selftest_f64w_gram(gs.data_ptr(), a.data_ptr(), lda, m, n, part.data_ptr(), pl["wr"], 0) == 0
    ref = (a[:, :m] @ a[:, :m].T).cpu().numpy()
    assert np.array_equal(gs.cpu().numpy()[:pl["bs"]], p64.pack_blocks(ref, n))


def chain(st, g, n, m, mode, pre_status=None, wq_in=None):
    """the blocked Cholesky step on G (n x n, fp64): returns R, Z (64 nb square), the four status words, the host words, the work space"""
    L, torch = st
    pl = wide_plan(L, m, n)
    wq = np.full(pl["wq"], SENT) if wq_in is None else wq_in.copy()
    wq[pl["o_gs"]: pl["o_gs"] + pl["bs"]] = p64.pack_blocks(g, n)
    sw = wq[pl["o_status"]: pl["o_status"] + 8].view(np.uint32)
    if pre_status is not None:
        sw[:4] = pre_status
    wd = dev(torch, wq)
    hw = torch.full((8,), 77, dtype=torch.int32, device="cuda")
    assert L.tsqr_selftest_f64w_chain(wd.data_ptr(), m, n, mode, hw.data_ptr()) == 0
    out = wd.cpu().numpy()
    R = p64.unpack_blocks(out[pl["o_rw"]: pl["o_rw"] + pl["bs"]], n)
    Z = p64.unpack_blocks(out[pl["o_zw"]: pl["o_zw"] + pl["bs"]], n)
    s = out[pl["o_status"]: pl["o_status"] + 8].view(np.uint32)[:4].copy()
    return R, Z, s, hw.cpu().numpy().view(np.uint32)[:4].copy(), out, pl


def words(s):
    return int(s[0]), float(s[1:2].view(np.float32)[0]), float(s[2:3].view(np.float32)[0]), int(s[3])


@pytest.mark.parametrize("n", [65, 79, 100, 128, 200, 640, 1000, 1024])
def test_wide_chain_plain_bounds_and_skipped_shift(st, n):
    """plain chain on SPD matrices of cond(G) 1 .. 1e6 (cond(A) 1 .. 1e3): both residuals over all n columns (pass_refs_f64.chain_bounds), exact zeros outside
    the n columns, S and the pivot ratio against longdouble; then plain + shifted as the product enqueues them with verdict 0: the
    shifted chain changes nothing -- R, Z and the four words bit for bit -- and copies the words to the host words"""
    m = 1 << 14
    for cond in ((1.0, 30.0, 1e3) if n <= 200 else (30.0,)):
        g, _ = p64.spd(n, cond, n + int(np.log10(cond)), m=2 * n)
        R, Z, s, _, _, _ = chain(st, g, n, m, 0)
        v, ratio, scond, one = words(s)
        assert v == 0, (n, cond, v)
        assert np.all(R[n:, :] == 0) and np.all(R[:, n:] == 0) and np.all(Z[n:, :] == 0) and np.all(Z[:, n:] == 0)
        Rn, Zn = R[:n, :n], Z[:n, :n]
        assert np.all(np.tril(Rn, -1) == 0.0) and np.all(np.tril(Zn, -1) == 0.0)
        bg, bz = p64.chain_bounds(Rn, Zn, n)
        eg = np.asarray(g.astype(LD) - p64.matmul_ld(Rn.T, Rn), np.float64)
        ez = np.asarray(p64.matmul_ld(Zn, Rn) - np.eye(n), np.float64)
        report("wide chain n %d cond %.0e  |G - RtR|" % (n, cond), np.abs(np.triu(eg)), np.triu(bg) + np.tril(np.ones_like(bg), -1))
        report("wide chain n %d cond %.0e  |Z R - I|" % (n, cond), np.abs(ez), bz + (bz == 0))
        print("wide chain n %d cond %.0e: pivot error d %.3g" % (n, cond, np.abs(p64.pivot_error(Rn, Zn)).max()))
        s_ref, ratio_ref = p64.scond_ref(g)
        if s_ref <= 100:
            assert abs(scond - s_ref) <= 1e-4 * s_ref and abs(ratio - ratio_ref) <= 1e-5 * ratio_ref, (scond, s_ref, ratio, ratio_ref)
            mx, al, _ = p64.rule(m, n)
            assert one == (1 if s_ref <= al else 0)
        R2, Z2, s2, h2, _, _ = chain(st, g, n, m, 2)
        assert np.array_equal(R, R2) and np.array_equal(Z, Z2) and np.array_equal(s, s2) and np.array_equal(s2, h2)


@pytest.mark.parametrize("n", [79, 128, 200])
def test_wide_chain_shifted(st, n):
    """plain verdict 1 (dependent columns in the last block, a zero column in the first): the shifted chain factors G + s I, s from the
    documented formula on the diagonal entries < n only -- the backward residual of G + s I against chain_bounds, rows and columns >= n
    exact zeros -- verdict 2, word [3] 0; the shifted chain alone (after a rejected plain chain: the same bits; after an accepted
    one: it skips itself); NaN or Inf in any block: verdict 1"""
    m = 1 << 14
    g, _ = p64.spd(n, 3.0, n, m=2 * n)
    g[:, n - 1] = g[:, n - 2]; g[n - 1, :] = g[n - 2, :]
    g[:, 5] = 0.0; g[5, :] = 0.0
    R, Z, s, h, _, _ = chain(st, g, n, m, 2)
    assert words(s)[0] == 2 and words(s)[3] == 0 and np.array_equal(s, h)
    assert np.all(R[n:, :] == 0) and np.all(R[:, n:] == 0) and np.all(Z[n:, :] == 0) and np.all(Z[:, n:] == 0)
    sh = p64.rule(m, n)[2] * np.trace(g)
    Rn, Zn = R[:n, :n], Z[:n, :n]
    report("wide chain n %d shifted  |G + sI - RtR|" % n, np.triu(p64.shift_residual(g, sh, Rn)),
           np.triu(p64.chain_bounds(Rn, Zn, n)[0]) + np.tril(np.ones((n, n)), -1))
    # (d) the shifted chain alone on the work space the plain chain left, and with a plain verdict of 0 in the status slot
    _, _, s0, _, wq0, pl = chain(st, g, n, m, 0)
    assert words(s0)[0] == 1
    R1, Z1, s1, h1, _, _ = chain(st, g, n, m, 1, wq_in=wq0)
    assert np.array_equal(R1, R) and np.array_equal(Z1, Z) and np.array_equal(s1, s) and np.array_equal(h1, s)
    accepted = np.array([0, 0x3f800000, 0x3f800000, 1], np.uint32)
    _, _, s2, h2, wq2, _ = chain(st, g, n, m, 1, pre_status=accepted)
    assert np.array_equal(s2, accepted) and np.array_equal(h2, accepted)          # nothing but the copy to the host words
    assert np.all(wq2[pl["o_w"]: pl["o_status"]] == SENT), "a skipped shifted chain wrote to the work space"
    assert np.all(np.isfinite(Z))
    g2, _ = p64.spd(n, 3.0, n + 1, m=2 * n)
    for (i, j, bad) in ((3, 3, np.nan), (n - 1, n - 1, np.inf), (2, n - 1, np.nan)):
        gb = g2.copy(); gb[i, j] = bad; gb[j, i] = bad
        _, _, sb, hb, _, _ = chain(st, gb, n, m, 2)
        assert words(sb)[0] == 1 and hb[0] == 1, (i, j, bad, sb)


@pytest.mark.parametrize("n,split", [(65, 33), (100, 40), (129, 70), (200, 100), (640, 300)])
def test_wide_apply_exact(st, n, split):
    """integer A times an exact inverse pair spanning several column blocks: bit for bit, m < 128 and every m mod 32 tail, in place"""
    L, torch = st
    rng = np.random.default_rng(n)
    amax = bmax = (1 << 20) - 1
    p64.assert_apply_budget(amax, split, bmax)
    _, z = p64.exact_inverse_pair64(rng, n, split, bmax)
    zw = dev(torch, p64.pack_blocks(z, n))
    for m in ([n + 1, 32 * 25, 32 * 25 + 1, 32 * 25 + 15, 32 * 25 + 16, 32 * 25 + 17, 32 * 25 + 31] if n <= 200 else [1055]):
        a = rng.integers(-amax, amax + 1, size=(m, n)).astype(np.float64)
        ref = a @ z
        odd = m & 1
        lda, ldq = m + (3 if odd else (-m) % 2), m + 5
        apool, ap = up64(torch, a, lda, odd)
        qpool, qp = up64(torch, np.full((m, n), SENT), ldq, odd, pad=SENT)
        assert L.tsqr_selftest_f64w_apply(qp, ldq, ap, lda, m, n, zw.data_ptr()) == 0
        assert np.array_equal(download(qpool, m, n, ldq, odd), ref), (m, n)
        assert np.all(padding_of(qpool, m, n, ldq, odd) == SENT)
        assert L.tsqr_selftest_f64w_apply(ap, lda, ap, lda, m, n, zw.data_ptr()) == 0
        assert np.array_equal(download(apool, m, n, lda, odd), ref), (m, n, "in place")
        assert np.all(np.isnan(padding_of(apool, m, n, lda, odd)))


@pytest.mark.parametrize("n", [65, 79, 100, 128, 200, 1000])
def test_wide_rcopy_and_rmul(st, n):
    L, torch = st
    rng = np.random.default_rng(n)
    ldr = n + 3
    bs = p64.npairs(n) * 4096
    for kind in ("int", "general"):
        if kind == "int":
            rw_m, r1 = p64.int_triangular(rng, n, (1 << 20) - 1), p64.int_triangular(rng, n, (1 << 20) - 1)
        else:
            rw_m, r1 = np.triu(rng.standard_normal((n, n))), np.triu(rng.standard_normal((n, n)))
        rw = dev(torch, p64.pack_blocks(rw_m, n))
        rpool, rp = up64(torch, np.full((n, n), SENT), ldr, 1, pad=SENT)
        assert L.tsqr_selftest_f64w_rcopy(rp, ldr, rw.data_ptr(), n) == 0
        assert np.array_equal(download(rpool, n, n, ldr, 1), rw_m) and np.all(padding_of(rpool, n, n, ldr, 1) == SENT)
        # the running R as the first sweep's rcopy left it: zeros below the diagonal.  rmul writes the block pairs I <= J only; inside
        # the diagonal blocks it never reads below the diagonal (NaN there) and writes exact zeros
        blockdiag = (np.arange(n)[:, None] // 64) == (np.arange(n)[None, :] // 64)
        rpool, rp = up64(torch, r1 + np.where(blockdiag, np.tril(np.full((n, n), NAN), -1), 0.0), ldr, 1, pad=SENT)
        rc = torch.full((bs + 8,), SENT, dtype=torch.float64, device="cuda")
        assert L.tsqr_selftest_f64w_rmul(rp, ldr, rw.data_ptr(), rc.data_ptr(), n) == 0
        out = download(rpool, n, n, ldr, 1)
        assert np.all(padding_of(rpool, n, n, ldr, 1) == SENT) and np.all(np.tril(out, -1) == 0.0) and np.all(rc[bs:].cpu().numpy() == SENT)
        if kind == "int":
            assert np.array_equal(out, rw_m @ r1)
        else:
            report("rmul_wide_f64 n %d" % n, np.abs(np.asarray(out.astype(LD) - p64.matmul_ld(rw_m, r1), np.float64)),
                   p64.rmul_bound(rw_m, r1) + np.tril(np.ones((n, n)), -1))

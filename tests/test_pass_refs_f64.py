"""CPU tests of tests/pass_refs_f64.py: the block-store layout round trip, the bit budgets of the exact generators, every bound on an
honest fp64 numpy model of its pass and -- so that the bound is known to bite -- on the same model with one seeded defect, and the
launch plans of the fp64 entries as the test library reports them (the definitions libtsqr_mi.so is built from; no GPU is touched)."""
import ctypes
import os

import numpy as np
import pytest

from tests import pass_refs as pr
from tests import pass_refs_f64 as p64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


def worst(measured, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(measured == 0, 0.0, np.abs(measured) / bound)
    return float(np.max(ratio))


def test_longdouble_is_extended():
    p64.require_longdouble()
    assert np.finfo(LD).eps <= 2.0 ** -63


@pytest.mark.parametrize("n", [65, 79, 100, 128, 129, 200, 1000, 1024])
def test_block_store_round_trip(n):
    rng = np.random.default_rng(n)
    x = np.triu(rng.standard_normal((n, n)))
    v = p64.pack_blocks(x, n)
    assert v.size == p64.npairs(n) * 4096
    back = p64.unpack_blocks(v, n)
    assert np.array_equal(back[:n, :n], x) and np.all(back[n:, :] == 0) and np.all(back[:, n:] == 0)
    i, j = n - 1, n - 1                                                   # pair p = J (J + 1) / 2 + I, element 4096 p + 64 c + r
    assert v[4096 * p64.wpair(i >> 6, j >> 6) + 64 * (j & 63) + (i & 63)] == x[i, j]
    assert v[4096 * p64.wpair(0, 1) + 64 * 0 + 5] == x[5, 64]
    g = x.T @ x
    assert np.array_equal(p64.unpack_blocks(p64.pack_blocks(g, n), n, symmetric=True)[:n, :n], g)


@pytest.mark.parametrize("m", [1, 65, 4097, 1 << 13, (1 << 13) + 1, 1 << 20, (1 << 20) + 1, 1 << 23])
def test_budget_is_asserted_and_used(m):
    kmax = p64.kmax_for(m)
    p64.assert_gram_budget(kmax, m)
    with pytest.raises(AssertionError):
        p64.assert_gram_budget(1 << 27, m)
    a = p64.exact_ints64(np.random.default_rng(m), min(m, 4097), 5, kmax=kmax)
    k = np.abs(a / np.exp2(np.floor(np.log2(np.abs(a).max(axis=0) / kmax) + 0.5)))
    assert np.mean(k >= (kmax + 1) // 2) > 0.7                            # most entries use all their bits


def test_exact_gram_is_order_independent():
    a = p64.exact_ints64(np.random.default_rng(3), 4097, 33)
    g = p64.gram_exact(a)
    assert np.array_equal(g, p64.model_gram(a, 64)) and np.array_equal(g, p64.model_gram(a[::-1], 16))
    assert np.array_equal(g.astype(LD), p64.matmul_ld(a.T, a))
    assert not np.array_equal(g, p64.model_gram(a, 64, defect="tail"))    # one dropped row
    assert not np.array_equal(g, p64.model_gram(a, 64, defect="fp32"))    # one fp32 conversion


def test_exact_apply_pair_and_single_products():
    rng = np.random.default_rng(5)
    n, split, amax, bmax = 48, 16, (1 << 20) - 1, (1 << 20) - 1
    p64.assert_apply_budget(amax, split, bmax)
    r, z = p64.exact_inverse_pair64(rng, n, split, bmax)
    a = rng.integers(-amax, amax + 1, size=(200, n)).astype(np.float64)
    q = a @ z
    assert np.array_equal(q.astype(LD), p64.matmul_ld(a, z)) and np.array_equal(q @ r, a)
    a1 = p64.single_entry_rows64(rng, 300, n)
    z1 = np.triu(p64.full_mantissa64(rng, (n, n), 3))
    q1 = p64.fl64_products(a1, z1)
    assert np.array_equal(q1, a1 @ z1)                                    # zeros add exactly: numpy's product is the rounded one too
    r2, r1 = p64.int_triangular(rng, 64), p64.int_triangular(rng, 64)
    assert np.array_equal((r2 @ r1).astype(LD), p64.matmul_ld(r2, r1))


@pytest.mark.parametrize("m,n,kind", [(4097, 33, "gauss"), (4097, 33, "same_sign"), (1000, 64, "gauss")])
def test_gram_bound_holds_and_defects_break_it(m, n, kind):
    rng = np.random.default_rng(m + n)
    a = rng.standard_normal((m, n)) if kind == "gauss" else rng.uniform(0.5, 1.5, (m, n))
    ref = p64.matmul_ld(a.T, a)
    bound = p64.gram_bound(a, p64.gram_path_narrow(m))
    ok = worst(np.asarray(p64.model_gram(a, 64).astype(LD) - ref, np.float64), bound)
    tail = worst(np.asarray(p64.model_gram(a, 64, "tail").astype(LD) - ref, np.float64), bound)
    f32 = worst(np.asarray(p64.model_gram(a, 64, "fp32").astype(LD) - ref, np.float64), bound)
    print("gram %s %dx%d: honest %.3g  tail dropped %.3g  one fp32 partial %.3g" % (kind, m, n, ok, tail, f32))
    assert ok <= 1.0 and tail > 1.0 and f32 > 1.0


@pytest.mark.parametrize("n,cond", [(64, 1e3), (51, 1e2), (17, 30.0), (1, 1.0)])
def test_chol_bounds_hold_and_a_bare_seed_breaks_them(n, cond):
    g, _ = p64.spd(n, cond, n)
    r, z = p64.model_chol(g)
    bg, bz = p64.chol_bounds(r, z, n)
    eg = np.asarray(g.astype(LD) - p64.matmul_ld(r.T, r), np.float64)
    ez = np.asarray(p64.matmul_ld(z, r) - np.eye(n), np.float64)
    ok = max(worst(eg, bg), worst(ez, bz))
    r0, z0 = p64.model_chol(g, newton=False)                              # v_rsq_f64's seed without its Newton step
    b0g, b0z = p64.chol_bounds(r0, z0, n)
    bad = max(worst(np.asarray(g.astype(LD) - p64.matmul_ld(r0.T, r0), np.float64), b0g),
              worst(np.asarray(p64.matmul_ld(z0, r0) - np.eye(n), np.float64), b0z))
    d = np.abs(p64.pivot_error(r0, z0)).max()
    print("chol n %d cond %.0e: honest %.3g  bare seed %.3g (d %.3g)" % (n, cond, ok, bad, d))
    assert ok <= 1.0 and bad > 1.0
    assert 0.5 * p64.E0_RSQ <= d <= 1.5 * p64.E0_RSQ and np.abs(p64.pivot_error(r, z)).max() <= 4 * p64.U
    assert 1.9e-14 < p64.E_RSQ < 2.2e-14


@pytest.mark.parametrize("n", [100, 200])
def test_chain_bounds_hold_on_the_honest_model(n):
    g, _ = p64.spd(n, 1e4, n)
    r, z = p64.model_chol(g)
    bg, bz = p64.chain_bounds(r, z, n)
    eg = np.asarray(g.astype(LD) - p64.matmul_ld(r.T, r), np.float64)
    ez = np.asarray(p64.matmul_ld(z, r) - np.eye(n), np.float64)
    assert max(worst(eg, bg), worst(ez, bz)) <= 1.0
    r0, z0 = p64.model_chol(g, newton=False)
    b0g, _ = p64.chain_bounds(r0, z0, n)
    assert worst(np.asarray(g.astype(LD) - p64.matmul_ld(r0.T, r0), np.float64), b0g) > 1.0


def test_s_against_longdouble_and_dropped_offdiagonal_terms():
    n = 200
    g, _ = p64.spd(n, 8.0, 11)
    s_ref, ratio_ref = p64.scond_ref(g)
    assert s_ref <= 100
    r, z = p64.model_chol(g)
    assert abs(p64.model_s(g, z) - s_ref) <= 1e-4 * s_ref
    assert abs(p64.model_s(g, z, nb_offdiag=False) - s_ref) > 1e-4 * s_ref          # the off-diagonal block pairs omitted
    assert abs(np.min(np.diag(r) ** 2 / np.diag(g)) - ratio_ref) <= 1e-5 * ratio_ref


@pytest.mark.parametrize("n", [64, 100])
def test_shift_check_bites(n):
    """The check the GPU tests apply to a shifted factorisation: |G + s I - R^T R| per entry against chol_bounds / chain_bounds, s from the
    documented formula, and exact zeros in rows and columns >= n.  The honest fp64 model passes; 10/11 of the shift, a trace taken over
    the first block only, a shift that misses one diagonal entry or the whole second block, and a shift on the padded diagonal entries
    >= n are all rejected."""
    m = 4096
    g, _ = p64.spd(n, 3.0, n)
    g[:, n - 1] = g[:, n - 2]; g[n - 1, :] = g[n - 2, :]                   # dependent columns: what sends the product to the shift
    s = p64.rule(m, n)[2] * np.trace(g)
    bound = lambda r, z: (p64.chol_bounds(r, z, n) if n <= 64 else p64.chain_bounds(r, z, n))[0]
    r, z = p64.model_chol(g, shift=s)
    ok = worst(p64.shift_residual(g, s, r), bound(r, z))
    bad = {}
    for name, kw in (("10/11 of the shift", dict(shift=s * 10 / 11)), ("2x the shift", dict(shift=2 * s)),
                     ("trace of the first block", dict(shift=p64.rule(m, n)[2] * np.trace(g[:min(n, 64), :min(n, 64)]) * (0.5 if n <= 64 else 1.0))),
                     ("first block only", dict(shift=s, nreal=min(n - 1, 64)))):
        r1, z1 = p64.model_chol(g, **kw)
        bad[name] = worst(p64.shift_residual(g, s, r1), bound(r1, z1))
    gm = g.copy(); gm[7, 7] -= s                                            # the shift missing on one diagonal entry
    r1, z1 = p64.model_chol(gm, shift=s)
    bad["one entry missed"] = worst(p64.shift_residual(g, s, r1), bound(r1, z1))
    print("shift check n %d: honest %.3g  %s" % (n, ok, "  ".join("%s %.3g" % kv for kv in bad.items())))
    assert ok <= 1.0 and all(not v <= 1.0 for v in bad.values())        # (NaN -- a breakdown in an unshifted block -- fails the check too)
    np_ = 64 * p64.nblocks(n) if n > 64 else 16 * pr.ntiles(n)
    if np_ > n:
        gp = np.zeros((np_, np_)); gp[:n, :n] = g
        rp, zp = p64.model_chol(gp, shift=s, nreal=n)
        assert p64.padding_is_zero(rp, n) and p64.padding_is_zero(zp, n) and np.array_equal(rp[:n, :n], r)
        rq, _ = p64.model_chol(gp, shift=s, nreal=np_)                      # the shift on the padded diagonal entries >= n
        assert not p64.padding_is_zero(rq, n)


@pytest.mark.parametrize("n", [16, 64, 128, 200])
def test_ladder_matrices_land_on_the_intended_side(n):
    """the matrices of the ladder tests (tests/test_gpu_f64.py, test_gpu_f64_wide.py): S of the fp64 model of the first sweep -- Gram
    matrix in fp64, chol_body16's row operations, S summed per block pair -- lies within 1/64 (the relative perturbation the
    CholeskyQR2 bound itself allows for G) of the prescribed S_ref, so a margin of 2 puts every case on its side of its threshold"""
    m = 4096
    mx, al, _ = p64.rule(m, n)
    for name, target, s0, s1 in p64.ladder_targets(m, n):
        a, s_ref = p64.ladder_matrix(m, n, target, n)
        assert abs(p64.s_of(a) - s_ref) <= 1e-6 * s_ref
        g = a.T @ a
        r, z = p64.model_chol(g)
        s_model = p64.model_s(g, z)
        assert abs(s_model - s_ref) <= s_ref / 64, (name, s_model, s_ref)
        sweeps = 1 if s_model <= al else (2 if s_model <= mx else 103)
        assert sweeps == s0 and (2 if s_model <= mx else 103) == s1, (name, s_model, al, mx)


def test_apply_and_rmul_bounds():
    rng = np.random.default_rng(9)
    a = rng.standard_normal((300, 64))
    z = np.linalg.inv(np.triu(pr.random_triangular(rng, 64, 1e8).astype(np.float64)))
    err = np.asarray((a @ z).astype(LD) - p64.matmul_ld(a, z), np.float64)
    assert worst(err, p64.apply_bound(a, z)) <= 1.0
    q32 = (a.astype(np.float32) @ z.astype(np.float32)).astype(np.float64)
    assert worst(np.asarray(q32.astype(LD) - p64.matmul_ld(a, z), np.float64), p64.apply_bound(a, z)) > 1.0
    r2, r1 = np.triu(rng.standard_normal((64, 64))), np.triu(rng.standard_normal((64, 64)))
    assert worst(np.asarray((r2 @ r1).astype(LD) - p64.matmul_ld(r2, r1), np.float64), p64.rmul_bound(r2, r1)) <= 1.0


# ---- the launch plans ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def libs():
    st = ctypes.CDLL(os.path.join(ROOT, "tsqr_gpu_amd", "csrc", "libtsqr_selftest.so"))
    mi = ctypes.CDLL(os.path.join(ROOT, "tsqr_gpu_amd", "csrc", "libtsqr_mi.so"))
    st.tsqr_selftest_f64_rule.restype = ctypes.c_int
    st.tsqr_selftest_f64_rule.argtypes = [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
    for f in (st.tsqr_selftest_f64_plan, st.tsqr_selftest_f64w_plan):
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(ctypes.c_longlong)]
    for name in ("tsqr_mi_working_r_size_f64", "tsqr_mi_working_r_size_f64_wide", "tsqr_mi_working_q_size_f64", "tsqr_mi_working_q_size_f64_wide"):
        getattr(mi, name).restype = ctypes.c_size_t
        getattr(mi, name).argtypes = [ctypes.c_size_t, ctypes.c_size_t]
    return st, mi


def _ms():
    return list(range(1, 5001)) + [(1 << 17) + 64, 1 << 20, 1 << 23]


def test_narrow_plan(libs):
    st, mi = libs
    out = (ctypes.c_longlong * 8)()
    for n in (1, 16, 17, 32, 33, 48, 49, 64):
        for m in _ms():
            if m < n:
                continue
            assert st.tsqr_selftest_f64_plan(m, n, out) == 0
            NT, ntri, nch, nwaves, nblocks, wq, wr, cap = list(out)
            assert NT == (n + 15) // 16 and ntri == NT * (NT + 1) // 2 and nch == -(-m // 64)
            assert 1 <= nwaves <= min(nch, cap) and nblocks == (nwaves + 3) // 4
            # the partition itself is gram_f64_kernel's loop `for (ch = gw; ch < nchunks; ch += nwaves)` over waves gw < nwaves (waves
            # gw >= nwaves of the last workgroup take nothing): modelled here -- every chunk belongs to exactly one wave, no wave is idle
            if m % 97 == 0 or m > 5000:
                owner = np.concatenate([np.arange(gw, nch, nwaves) for gw in range(nwaves)])
                assert np.array_equal(np.sort(owner), np.arange(nch)) and all(gw < nch for gw in range(nwaves))
            assert wr == nblocks * ntri * 256 == mi.tsqr_mi_working_r_size_f64(m, n)
            assert wq == mi.tsqr_mi_working_q_size_f64(m, n)
            assert p64.gram_path_narrow(m) == p64.gram_path_narrow(m, nwaves)


def test_wide_plan(libs):
    st, mi = libs
    out = (ctypes.c_longlong * 20)()
    for n in [64 * nb for nb in range(2, 17)] + [65, 129, 193, 961]:     # every nb = 2 .. 16, and ragged last blocks
        for m in _ms() + [(1 << 26) // n]:
            if m < n:
                continue
            assert st.tsqr_selftest_f64w_plan(m, n, out) == 0
            nb, npairs, ngroups, nslices, cps, nch, bs = list(out)[:7]
            offs = list(out)[7:18]
            wr, cap = out[18], out[19]
            assert nb == -(-n // 64) and npairs == nb * (nb + 1) // 2 and ngroups == -(-npairs // 4) and bs == npairs * 4096
            assert nch == -(-m // 16) and nslices * cps >= nch > (nslices - 1) * cps      # every chunk in exactly one slice, none empty
            assert wr == nslices * bs <= cap == 8 << 20
            assert wr == mi.tsqr_mi_working_r_size_f64_wide(m, n) and offs[-1] == mi.tsqr_mi_working_q_size_f64_wide(m, n)
            sizes = [bs + 64, bs, bs, bs, bs, bs, nb * 4096, nb * (nb + 1), nb * 2, 8]
            assert offs[0] == 0 and [b - a for a, b in zip(offs[:-1], offs[1:])] == sizes  # the regions do not overlap
            assert nb * nb + nb <= sizes[7] and 4 * nb * 4 <= sizes[8] * 8                # sb terms + ratios; bst words (4 per block)


def test_rule_of_the_library_is_the_documented_one(libs):
    """f64_rule (f64_plan.h: the one definition both entries and the test hooks call) against the formulas of CholArgs64 as
    pass_refs_f64.rule restates them: 64 n S u (mn + n(n+1)) <= 1, 4 n S u <= 1e-12, s = 11 u (mn + n(n+1)) trace(G); later sweeps
    have no bound on S and are never accepted alone"""
    st, _ = libs
    out = (ctypes.c_double * 3)()
    for n in (1, 16, 64, 65, 128, 200, 1024):
        for m in (n, 4096, 1 << 14, 1 << 20, 1 << 23):
            if m < n:
                continue
            assert st.tsqr_selftest_f64_rule(m, n, 1, out) == 0
            assert tuple(out) == p64.rule(m, n), (m, n, tuple(out), p64.rule(m, n))
            assert st.tsqr_selftest_f64_rule(m, n, 0, out) == 0
            assert out[0] == np.inf and out[1] == 0.0 and out[2] == p64.rule(m, n)[2]

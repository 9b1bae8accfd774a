"""The three kernels of the fp64 block orthogonalisation entry, each alone through its test-library hook: the cross-Gram pass with its
reduction (tsqr_selftest_f64_orth_gram), the projection update (tsqr_selftest_f64_orth_update) and the kernel that writes the caller's S
(tsqr_selftest_f64_orth_s).

Each result is compared with the same product evaluated in longdouble.  Allowance: twice the error of NumPy's fp64 evaluation on the
same data, or 4 2^-53 times the Frobenius norm of the product of the absolute values, whichever is larger.  Shapes: the table of
tests/pass_refs_f64_orth.py and the tile edges, in both layouts; the four layout pairs must agree bit for bit."""
import ctypes
import os

import numpy as np
import pytest

from tests import pass_refs_f64_orth as po
from tests.test_gpu_f64_orth import GUARD, padding_of, pool, unpool

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
c_p, c_i, c_z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
LD = np.longdouble
fro = lambda a: float(np.sqrt(np.sum(np.asarray(a, dtype=LD) ** 2)))
SHAPES = ["1003x130x17", "80x64x16-complete", "333x1x1", "2061x65x64-cond1e8", "1003x63x16", "1003x64x64", "33000x70x20-slices",
          "4096x1024x64-caps"]
PAIRS = [(0, 0), (0, 1), (1, 0), (1, 1)]


@pytest.fixture(scope="module")
def st(bq):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    bq.lib()
    L = ctypes.CDLL(os.path.join(ROOT, "tsqr_gpu_amd", "csrc", "libtsqr_selftest.so"))
    sig = {"tsqr_selftest_f64_orth_plan": [c_z, c_z, c_z, ctypes.POINTER(ctypes.c_longlong)],
           "tsqr_selftest_f64_orth_gram": [c_i, c_i, c_p, c_p, c_z, c_p, c_z, c_z, c_i, c_i, c_p, c_z],
           "tsqr_selftest_f64_orth_update": [c_i, c_i, c_p, c_z, c_p, c_z, c_p, c_z, c_i, c_i],
           "tsqr_selftest_f64_orth_s": [c_p, c_z, c_p, c_p, c_z, c_i, c_i, c_i]}
    for name, args in sig.items():
        getattr(L, name).restype, getattr(L, name).argtypes = c_i, args
    return L, torch


def np_of(n):
    return 16 * ((n + 15) // 16)


def pack_sw(s, n_pad):
    """a k x n matrix in the work layout: S[64 b + r][c] at b * 64 * NP + 64 c + r, zero padded"""
    k, n = s.shape
    kb = (k + 63) // 64
    full = np.zeros((kb * 64, n_pad))
    full[:k, :n] = s
    return np.ascontiguousarray(full.reshape(kb, 64, n_pad).transpose(0, 2, 1)).ravel()


def unpack_sw(sw, k, n):
    n_pad, kb = np_of(n), (k + 63) // 64
    return sw[:kb * 64 * n_pad].reshape(kb, n_pad, 64).transpose(0, 2, 1).reshape(kb * 64, n_pad)


def gram(st, v, x, v_row, x_row, extra=0):
    """-> the padded (64 kblocks) x NP matrix of V^T X and the word behind it; the operands are checked to be unwritten"""
    L, torch = st
    (m, k), n = v.shape, x.shape[1]
    plan = (ctypes.c_longlong * 6)()
    assert L.tsqr_selftest_f64_orth_plan(m, k, n, plan) == 0
    hv, ldv = pool(v, v_row, extra)
    hx, ldx = pool(x, x_row, extra)
    dv, dx = torch.from_numpy(hv).cuda(), torch.from_numpy(hx).cuda()
    nelem = ((k + 63) // 64) * 64 * np_of(n)
    sw = torch.full((nelem + 1 + 8,), GUARD, dtype=torch.float64, device="cuda")
    part = torch.full((plan[5] + 8,), GUARD, dtype=torch.float64, device="cuda")
    assert L.tsqr_selftest_f64_orth_gram(v_row, x_row, sw.data_ptr(), dv.data_ptr(), ldv, dx.data_ptr(), ldx, m, k, n, part.data_ptr(),
                                         plan[5]) == 0
    assert dv.cpu().numpy().tobytes() == hv.tobytes() and dx.cpu().numpy().tobytes() == hx.tobytes()
    out = sw.cpu().numpy()
    assert np.all(out[nelem + 1:] == GUARD) and np.all(part[plan[5]:].cpu().numpy() == GUARD)
    return unpack_sw(out, k, n), out[nelem]


@pytest.fixture(scope="module")
def gram_refs():
    """case -> (longdouble V^T X, allowance); computed once"""
    cache = {}

    def get(case):
        if case not in cache:
            v, x = po.make(case)
            exact = np.asarray(v, dtype=LD).T @ np.asarray(x, dtype=LD)
            allow = max(2.0 * fro(v.T @ x - exact), 4.0 * po.U * fro(np.abs(v).T @ np.abs(x)))
            cache[case] = (exact, allow)
        return cache[case]
    return get


@pytest.mark.parametrize("case", SHAPES)
def test_cross_gram_pass(st, gram_refs, case):
    v, x = po.make(case)
    (m, k), n = v.shape, x.shape[1]
    exact, allow = gram_refs(case)
    pairs = PAIRS if case != "4096x1024x64-caps" else [(0, 0), (1, 1)]
    first = None
    for v_row, x_row in pairs:
        full, rows = gram(st, v, x, v_row, x_row, extra=0 if (v_row, x_row) == (0, 0) else 3)
        assert rows == float(m)
        assert np.all(full[k:] == 0.0) and np.all(full[:, n:] == 0.0), "the padding of the work copy is not exact zeros"
        err = fro(full[:k, :n] - exact)
        print("GRAM %s layouts %d%d | error %.2e | allowance %.2e" % (case, v_row, x_row, err, allow))
        assert err <= allow
        first = full if first is None else first
        assert full.tobytes() == first.tobytes(), "layout pair (%d, %d) differs from (0, 0)" % (v_row, x_row)


def update(st, v, x, s, v_row, x_row, extra=0):
    L, torch = st
    (m, k), n = v.shape, x.shape[1]
    hv, ldv = pool(v, v_row, extra)
    hx, ldx = pool(x, x_row, extra)
    hs = np.concatenate([pack_sw(s, np_of(n)), np.full(8, GUARD)])
    dv, dx, ds = (torch.from_numpy(a).cuda() for a in (hv, hx, hs))
    assert L.tsqr_selftest_f64_orth_update(v_row, x_row, dx.data_ptr(), ldx, dv.data_ptr(), ldv, ds.data_ptr(), m, k, n) == 0
    assert dv.cpu().numpy().tobytes() == hv.tobytes() and ds.cpu().numpy().tobytes() == hs.tobytes()
    out = dx.cpu().numpy()
    assert np.all(padding_of(out, (m, n), x_row, ldx) == GUARD), "padding of x or memory behind it was written"
    return unpool(out, (m, n), x_row, ldx)


@pytest.mark.parametrize("case", SHAPES)
def test_projection_update(st, case):
    v, x = po.make(case)
    (m, k), n = v.shape, x.shape[1]
    s = np.random.default_rng(k + n).standard_normal((k, n))
    vl, xl, sl = (np.asarray(a, dtype=LD) for a in (v, x, s))
    exact = xl - vl @ sl
    allow = max(2.0 * fro((x - v @ s) - exact), 4.0 * po.U * fro(np.abs(x) + np.abs(v) @ np.abs(s)))
    pairs = PAIRS if case != "4096x1024x64-caps" else [(0, 0), (1, 1)]
    first = None
    for v_row, x_row in pairs:
        got = update(st, v, x, s, v_row, x_row, extra=0 if (v_row, x_row) == (0, 0) else 3)
        err = fro(got - exact)
        print("UPDATE %s layouts %d%d | error %.2e | allowance %.2e" % (case, v_row, x_row, err, allow))
        assert err <= allow
        first = got if first is None else first
        assert got.tobytes() == first.tobytes(), "layout pair (%d, %d) differs from (0, 0)" % (v_row, x_row)


@pytest.mark.parametrize("k,n", [(130, 17), (1, 1), (64, 64), (65, 16), (1024, 64)])
def test_s_kernel(st, k, n):
    L, torch = st
    rng = np.random.default_rng(100 * k + n)
    s1, s2 = rng.standard_normal((k, n)), rng.standard_normal((k, n))
    r1 = np.triu(rng.standard_normal((n, n)))
    hs, lds = pool(np.full((k, n), GUARD), False, 3)
    hr, ldr = pool(r1 + np.tril(np.full((n, n), GUARD), -1), False, 2)     # (below the diagonal: never read)
    ds, dr = torch.from_numpy(hs).cuda(), torch.from_numpy(hr).cuda()
    sw1, sw2 = (torch.from_numpy(pack_sw(s, np_of(n))).cuda() for s in (s1, s2))
    assert L.tsqr_selftest_f64_orth_s(ds.data_ptr(), lds, sw1.data_ptr(), None, 0, k, n, 0) == 0
    out = ds.cpu().numpy()
    assert unpool(out, (k, n), False, lds).tobytes() == s1.tobytes() and np.all(padding_of(out, (k, n), False, lds) == GUARD)
    assert L.tsqr_selftest_f64_orth_s(ds.data_ptr(), lds, sw2.data_ptr(), dr.data_ptr(), ldr, k, n, 1) == 0
    out = ds.cpu().numpy()
    assert np.all(padding_of(out, (k, n), False, lds) == GUARD) and dr.cpu().numpy().tobytes() == hr.tobytes()
    got = unpool(out, (k, n), False, lds)
    exact = np.asarray(s1, dtype=LD) + np.asarray(s2, dtype=LD) @ np.asarray(r1, dtype=LD)
    allow = max(2.0 * fro((s1 + s2 @ r1) - exact), 4.0 * po.U * fro(np.abs(s1) + np.abs(s2) @ np.abs(r1)))
    err = fro(got - exact)
    print("S %dx%d | error %.2e | allowance %.2e" % (k, n, err, allow))
    assert err <= allow

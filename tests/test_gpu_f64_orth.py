"""GPU tests of the fp64 block orthogonalisation entry (tsqr_mi_orth_f64 through blockqr.orth_f64 and orth_f64_tensor) on the cases of
tests/pass_refs_f64_orth.py, passes = 2 and reorth = 0 unless said otherwise.

Bounds: ||Q^T Q - I||_F <= 1e-11 and ||W - V S - Q R||_F / ||W||_F <= 1e-13 (the QR entry's own claims, restated), and
||V^T Q||_F <= max(2 x the NumPy model's on the same data, 4 max(k, n) 2^-53).  Every figure is evaluated in longdouble and printed next
to the model's; profiles/fp64_orth_accuracy.md has the table measured on the MI355X."""
import os
import subprocess

import numpy as np
import pytest

from abi_util import compile_and_link
from tests import pass_refs_f64_orth as po

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = -777.25
TAIL = 64


@pytest.fixture(scope="module")
def env(bq):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return bq, torch


def pool(a, row_major, extra):
    """(flat host buffer, ld) holding a in the layout, GUARD in the padding up to ld and in TAIL doubles behind the last row / column"""
    rows, cols = a.shape
    if row_major:
        ld = cols + extra
        buf = np.full((rows, ld), GUARD)
        buf[:, :cols] = a
    else:
        ld = rows + extra
        buf = np.full((cols, ld), GUARD)
        buf[:, :rows] = a.T
    return np.concatenate([buf.ravel(), np.full(TAIL, GUARD)]), ld


def unpool(flat, shape, row_major, ld):
    rows, cols = shape
    body = flat[:-TAIL]
    return body.reshape(rows, ld)[:, :cols].copy() if row_major else body.reshape(cols, ld)[:, :rows].T.copy()


def padding_of(flat, shape, row_major, ld):
    """everything of the pool that is not the operand"""
    rows, cols = shape
    body = flat[:-TAIL]
    pad = body.reshape(rows, ld)[:, cols:] if row_major else body.reshape(cols, ld)[:, rows:]
    return np.concatenate([pad.ravel(), flat[-TAIL:]])


def run(env, v, w, passes=2, reorth=False, v_row=False, w_row=False, extra=0):
    """-> (state, q, s, r, sweeps); checks that v is unwritten and that no padding of w, s, r or v and nothing behind them was touched"""
    bq, torch = env
    (m, k), n = v.shape, w.shape[1]
    hv, ldv = pool(v, v_row, extra)
    hw, ldw = pool(w, w_row, extra)
    hs, lds = pool(np.full((k, n), GUARD), False, extra)
    hr, ldr = pool(np.full((n, n), GUARD), False, extra)
    dv, dw, ds, dr = (torch.from_numpy(x).cuda() for x in (hv, hw, hs, hr))
    bf = bq.buffer_f64_orth()
    bf.allocate(m, k, n)
    st = bq.orth_f64(dw, ldw, ds, lds, dr, ldr, dv, ldv, m, k, n, bf, passes=passes, reorthogonalize=reorth, v_row_major=v_row,
                     w_row_major=w_row)
    sweeps = bq.last_sweeps_f64()
    ov, ow, os_, or_ = (t.cpu().numpy() for t in (dv, dw, ds, dr))
    assert ov.tobytes() == hv.tobytes(), "v was written"
    for flat, shape, rm, ld in ((ow, (m, n), w_row, ldw), (os_, (k, n), False, lds), (or_, (n, n), False, ldr)):
        assert np.all(padding_of(flat, shape, rm, ld) == GUARD), "padding or memory behind an operand was written"
    return st, unpool(ow, (m, n), w_row, ldw), unpool(os_, (k, n), False, lds), unpool(or_, (n, n), False, ldr), sweeps


@pytest.fixture(scope="module")
def results(env):
    """one column-major call per case with passes = 2, shared by the tests below; never modified"""
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = run(env, *po.make(case))
        return cache[case]
    return get


@pytest.mark.parametrize("case", list(po.CASES))
def test_bounds(env, results, case):
    v, w = po.make(case)
    st, q, s, r, sweeps = results(case)
    assert st == 0
    vq, qtq, res = po.figures(v, w, q, s, r)
    mvq, mqtq, mres = po.model_figures(case, 2)
    print("ORTH %s | sweeps %d | ||V^T Q|| %.2e (model %.2e, bound %.2e) | ||Q^T Q - I|| %.2e (model %.2e) | residual %.2e (model %.2e)"
          % (case, sweeps, vq, mvq, po.vq_bound(case), qtq, mqtq, res, mres))
    assert np.all(np.diag(r) >= 0.0) and np.all(np.tril(r, -1) == 0.0)
    assert qtq <= po.QTQ_BOUND
    assert res <= po.RESID_BOUND
    assert vq <= po.vq_bound(case)
    assert 2 <= sweeps % 100 <= 12


def test_more_than_one_sweep_on_the_ill_conditioned_block(results):
    assert results("2061x65x64-cond1e8")[4] % 100 > 2


@pytest.mark.parametrize("extra", [0, 5])
def test_all_four_layout_pairs_give_the_same_bits(env, results, extra):
    case = "1003x130x17-near-cond1e8"
    v, w = po.make(case)
    st0, q0, s0, r0, sw0 = results(case)
    for v_row in (False, True):
        for w_row in (False, True):
            st, q, s, r, sw = run(env, v, w, v_row=v_row, w_row=w_row, extra=extra)
            assert (st, sw) == (st0, sw0)
            for a, b in ((q, q0), (s, s0), (r, r0)):
                assert a.tobytes() == b.tobytes(), (v_row, w_row, extra)


@pytest.mark.parametrize("case", ["2061x65x64-cond1e8", "333x1x1"])
def test_layouts_agree_at_the_edges(env, results, case):
    v, w = po.make(case)
    st0, q0, s0, r0, sw0 = results(case)
    st, q, s, r, sw = run(env, v, w, v_row=True, w_row=True, extra=3)
    assert (st, sw) == (st0, sw0) and q.tobytes() == q0.tobytes() and s.tobytes() == s0.tobytes() and r.tobytes() == r0.tobytes()


def test_two_calls_give_the_same_bits(env, results):
    case = "33000x70x20-slices"
    st0, q0, s0, r0, sw0 = results(case)
    st, q, s, r, sw = run(env, *po.make(case))
    assert (st, sw) == (st0, sw0) and q.tobytes() == q0.tobytes() and s.tobytes() == s0.tobytes() and r.tobytes() == r0.tobytes()


@pytest.mark.parametrize("case", po.EPS_ONE)
def test_one_round_returns_s_and_r(env, case):
    v, w = po.make(case)
    st, q, s, r, sweeps = run(env, v, w, passes=1)
    assert st == 0
    vq, qtq, res = po.figures(v, w, q, s, r)
    print("ORTH1 %s | sweeps %d | ||V^T Q|| %.2e | ||Q^T Q - I|| %.2e | residual %.2e" % (case, sweeps, vq, qtq, res))
    assert res <= po.RESID_BOUND and qtq <= po.QTQ_BOUND
    assert np.all(np.diag(r) >= 0.0)


@pytest.mark.parametrize("where", ["v", "w"])
def test_nan_ends_in_state_three_without_a_fault(env, where):
    bq, torch = env
    v, w = (np.array(a) for a in po.make("1003x130x17"))
    (v if where == "v" else w)[501, 3] = np.nan
    st, q, s, r, sweeps = run(env, v, w)
    assert st == bq.error_not_finite
    torch.cuda.synchronize()
    # the device is still usable
    assert run(env, *po.make("333x1x1"))[0] == 0


def test_tensor_form(env, results):
    bq, torch = env
    case = "1003x130x17"
    v, w = po.make(case)
    _, q0, s0, r0, _ = results(case)
    tv, tw = torch.from_numpy(np.array(v)).cuda(), torch.from_numpy(np.array(w)).cuda()      # contiguous: row-major
    same = lambda q, s, r: (q.cpu().numpy().tobytes() == q0.tobytes() and np.ascontiguousarray(s.cpu().numpy()).tobytes() == s0.tobytes()
                            and np.ascontiguousarray(r.cpu().numpy()).tobytes() == r0.tobytes())
    keep = tw.clone()
    q, s, r = bq.orth_f64_tensor(tv, tw)
    assert q.shape == tw.shape and s.shape == (130, 17) and r.shape == (17, 17) and q.is_contiguous()
    assert same(q, s, r) and torch.equal(tw, keep), "row-major tensors"
    cv, cw = tv.t().contiguous().t(), tw.t().contiguous().t()                                 # column-major strides
    q, s, r = bq.orth_f64_tensor(cv, cw)
    assert q.stride() == cw.stride() and same(q, s, r) and torch.equal(cw, keep), "column-major tensors"
    q, s, r = bq.orth_f64_tensor(cv, tw)
    assert same(q, s, r), "mixed layouts"
    big_v = torch.full((1003, 200), GUARD, dtype=torch.float64, device="cuda")
    big_w = torch.full((1003, 64), GUARD, dtype=torch.float64, device="cuda")
    big_v[:, 7:137] = tv
    big_w[:, 3:20] = tw
    q, s, r = bq.orth_f64_tensor(big_v[:, 7:137], big_w[:, 3:20], overwrite_w=True)           # strided slices, used where they lie
    assert q.data_ptr() == big_w[:, 3:20].data_ptr() and same(q, s, r)
    assert torch.all(big_w[:, :3] == GUARD) and torch.all(big_w[:, 20:] == GUARD) and torch.all(big_v[:, :7] == GUARD)
    wide = torch.zeros((1003, 34), dtype=torch.float64, device="cuda")
    wide[:, ::2] = tw
    q, s, r = bq.orth_f64_tensor(tv, wide[:, ::2], overwrite_w=True)                          # neither layout: copied once
    assert same(q, s, r) and torch.equal(wide[:, ::2], keep)
    with pytest.raises(bq.OrthError) as e:
        bad = tw.clone()
        bad[7, 2] = float("inf")
        bq.orth_f64_tensor(tv, bad)
    assert e.value.state == bq.error_not_finite


def test_cpp_sample_runs_inside_the_bounds(bq):
    with compile_and_link(os.path.join(ROOT, "tests", "cpp", "sample_fp64_orth.cpp"), "sample_fp64_orth") as exe:
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "orth_fp64 ok" in out.stdout and out.stdout.count("state 0") == 2

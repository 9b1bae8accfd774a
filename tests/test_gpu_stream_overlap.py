"""GPU tests: the stream schedules of the batch entries on OVERLAPPING operands, against the blocking calls in the same order.

tsqr_mi_qr_f32_batch / tsqr_mi_qr_f16_batch promise the blocking calls' result bit for bit whatever the schedule (include/tsqr_mi.h).
With two calls in flight (or chained), call i + 1's speculative attempt is enqueued before call i is finished; when call i is REJECTED by
the bf16-split level its ladder runs after that attempt.  Operands of neighbouring calls that overlap then see the wrong order unless the
library finishes call i first (tsqr_gpu_amd/csrc/stream_order.h decides that).

Every batch below is carved out of ONE device pool (C columns of m elements, ld = m).  The whole pool is first filled with U(-1, 1): stale
memory that the conditioning check accepts is what turns a wrong order into wrong factors with state 0.  The reference runs the calls one
after the other as blocking qr() calls on a copy of the pool, each checked against numpy fp64; every schedule (loop depths 1, 2, 3) must
then leave the WHOLE pool bit for bit as the reference left it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 4
COND_BAD = 1e6
RES32, ORTH32, R32 = 5e-7, 5e-6, 5e-6                  # tests/test_gpu_parity.py's bands
RES16, ORTH16, R16 = 1e-3, 5e-3, 2e-3                  # tests/test_gpu_f16.py's bands
RES_BAD = 1e-4                                         # residual of a rejected (cond 1e6) call: its ladder's rungs (measured up to 3.3e-5, 9211 x 51)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


# ---- layouts: per call (q column, r element offset, a column) in the pool, the calls whose A region receives an input ----
def layout(name, m, n, k=K):
    """Returns (pool columns, [(qc, re, ac)] * k, input calls).  qc / ac: column offsets (elements qc * m); re: element offset of R (ld n)."""
    h = n // 2
    rcols = (k * n * n + m - 1) // m + 1                # room for k separate R factors behind the matrix columns
    sep_r = lambda c0: [c0 * m + i * n * n for i in range(k)]
    if name == "control":                               # disjoint regions
        c = 2 * k * n
        return c + rcols, [((k + i) * n, sep_r(c)[i], i * n) for i in range(k)], list(range(k))
    if name == "feed_forward":                          # a[i + 1] is q[i]
        c = (k + 1) * n
        return c + rcols, [((i + 1) * n, sep_r(c)[i], i * n) for i in range(k)], [0]
    if name == "feed_forward_mid":                      # q[0] is a[1]; a[2] is an input of its own; q[2] is a[3]
        c = 6 * n
        ops = [(n, 0, 0), (2 * n, 0, n), (4 * n, 0, 3 * n), (5 * n, 0, 4 * n)]
        return c + rcols, [(q, sep_r(c)[i], a) for i, (q, _, a) in enumerate(ops)], [0, 2]
    if name == "backward":                              # q[i + 1] is a[i]: every call writes over the previous call's input
        c = (k + 1) * n
        return c + rcols, [(k * n if i == 0 else (i - 1) * n, sep_r(c)[i], i * n) for i in range(k)], list(range(k))
    if name == "r_into_a":                              # r[i] lies inside a[i + 1] (from its second column on)
        c = 2 * k * n
        return c + rcols, [((k + i) * n, ((i + 1) * n * m + m + 16) if i + 1 < k else sep_r(c)[i], i * n) for i in range(k)], list(range(k))
    if name == "shared_outputs":                        # one Q and one R for every call
        c = (k + 1) * n
        return c + rcols, [(k * n, sep_r(c)[0], i * n) for i in range(k)], list(range(k))
    if name == "partial":                               # q[i] overlaps a[i + 1] by n / 2 columns only
        c = 2 * n * k + n
        return c + rcols, [(2 * n * (i + 1) - h, sep_r(c)[i], 2 * n * i) for i in range(k)], list(range(k))
    raise ValueError(name)


class Case:
    """One pool with its operand views, inputs written over the pre-filled data."""

    def __init__(self, torch, m, n, dtype, name, bad, seed):
        self.torch, self.m, self.n, self.dtype = torch, m, n, dtype
        cols, self.ops, inputs = layout(name, m, n)
        self.bad = bad
        rng = np.random.Generator(np.random.MT19937(seed))
        pool = rng.uniform(-1, 1, size=(cols, m)).astype(np.float32)
        for i in inputs:
            if i in bad:
                from oracle import ref_oracle as ro
                a = ro.matrix_with_cond(m, n, COND_BAD, seed=seed + 17 * i + 1)
            else:
                a = rng.uniform(-1, 1, size=(m, n))
            ac = self.ops[i][2]
            pool[ac:ac + n] = a.T
        self.pool = torch.from_numpy(pool.astype(np.float16 if dtype == "f16" else np.float32)).cuda()

    def views(self, pool):
        flat = pool.view(-1)
        m, n = self.m, self.n
        qs = [pool[qc:qc + n] for qc, _, _ in self.ops]
        rs = [flat[re:re + n * n] for _, re, _ in self.ops]
        as_ = [pool[ac:ac + n] for _, _, ac in self.ops]
        return qs, rs, as_

    def bits(self, pool):
        return pool.view(self.torch.int16 if self.dtype == "f16" else self.torch.int32)


def check_reference_call(bq, a64, q, r, cond, f16, rejected, engine):
    """one blocking call of the reference sequence against numpy fp64 (a64: the A it read, q / r: what it wrote)"""
    res_tol, orth_tol, r_tol = (RES16, ORTH16 * max(1.0, a64.shape[1] / 100), R16) if f16 else (RES_BAD if rejected else RES32, ORTH32, R32)
    scale = max(1.0, cond / 10)
    assert np.isfinite(q).all() and np.isfinite(r).all()
    assert np.abs(np.tril(r, -1)).max() == 0.0
    d = q @ r - a64
    assert np.sqrt((d * d).sum() / (a64 * a64).sum()) < res_tol
    g = q.T @ q - np.eye(q.shape[1])
    assert np.sqrt((g * g).sum()) < orth_tol * scale
    r64 = np.linalg.qr(a64, mode="r")
    assert np.abs(np.abs(r) - np.abs(r64)).max() <= r_tol * scale * np.abs(r64).max()
    if rejected:                                        # the case is about a call the bf16-split level turns down: make sure it did
        assert engine not in (3, 5), engine


def reference(bq, torch, case, mode, bf):
    """the blocking calls one after the other on a copy of the pool, each checked against fp64; returns the pool they leave"""
    pool = case.pool.clone()
    qs, rs, as_ = case.views(pool)
    m, n = case.m, case.n
    for i in range(K):
        a64 = as_[i].cpu().numpy().astype(np.float64).T.copy()
        st = bq.qr(qs[i], m, rs[i], n, as_[i], m, m, n, bf, mode=mode)
        assert st == 0
        q = qs[i].cpu().numpy().astype(np.float64).T
        r = rs[i].cpu().numpy().astype(np.float64).reshape(n, n).T
        check_reference_call(bq, a64, q, r, np.linalg.cond(a64), case.dtype == "f16", i in case.bad, bq.last_engine())
    torch.cuda.synchronize()
    return pool


def batch_at_depths(bq, torch, case, mode, bf, want, depths=(1, 2, 3)):
    for depth in depths:
        pool = case.pool.clone()
        qs, rs, as_ = case.views(pool)
        bq.set_loop_depth(depth)
        try:
            st, states = bq.qr_batch(qs, case.m, rs, case.n, as_, case.m, case.m, case.n, bf, mode=mode)
        finally:
            bq.set_loop_depth(3)
        assert st == 0 and states == [0] * K, (depth, st, states)
        assert torch.equal(case.bits(pool), case.bits(want)), "depth %d: the pool differs from the blocking calls'" % depth


SHAPES = {                                             # (m, n, dtype, mode): what schedule each one reaches
    "f32_32768x64": (1 << 15, 64, "f32", "fp32_tc_cor"),     # chained64 at depth 3, two in flight at depth 2
    "f32_9211x51": (9211, 51, "f32", "fp32_tc_cor"),         # two in flight only
    "f32_33280x128": (64 * 520, 128, "f32", "fp32_tc_cor"),  # chained128, the speculative one-panel path
    "f16_32768x64": (1 << 15, 64, "f16", "fp16_notc"),       # fp16 chained (gram_h)
    "f16_20000x48": (20000, 48, "f16", "fp16_notc"),         # fp16 stream without chaining
}
LAYOUTS = [("feed_forward", (0,)), ("feed_forward_mid", (2,)), ("backward", (0,)), ("backward", (1,)), ("r_into_a", (0,)),
           # shared outputs: the call rejected is the one before the last, so that its ladder would write last in the wrong order
           ("shared_outputs", (2,)), ("partial", (0,)), ("control", (1,))]
CASES = [("f32_32768x64",) + lay for lay in LAYOUTS]
CASES += [(s, name, bad) for s in ("f32_9211x51", "f32_33280x128", "f16_32768x64", "f16_20000x48")
          for name, bad in (("feed_forward", (0,)), ("backward", (0,)), ("shared_outputs", (2,)))]


@pytest.fixture(scope="module")
def buffers(bq):
    cache = {}

    def get(shape):
        if shape not in cache:
            m, n, _, mode = SHAPES[shape]
            bf = bq.buffer(bq.compute_mode[mode], False)
            bf.allocate(m, n)
            cache[shape] = bf
        return cache[shape]
    return get


@pytest.mark.parametrize("shape,name,bad", CASES, ids=["%s-%s-bad%s" % (s, l, "".join(map(str, b))) for s, l, b in CASES])
def test_batch_on_overlapping_operands(bq, torch_cuda, buffers, shape, name, bad):
    m, n, dtype, mode = SHAPES[shape]
    md = bq.compute_mode[mode]
    case = Case(torch_cuda, m, n, dtype, name, bad, seed=100 + 7 * len(name) + bad[0])
    bf = buffers(shape)
    want = reference(bq, torch_cuda, case, md, bf)
    batch_at_depths(bq, torch_cuda, case, md, bf, want)


@pytest.mark.parametrize("direction", ["forward", "backward"])
def test_public_submit_pair(bq, torch_cuda, buffers, direction):
    """tsqr_mi_qr_f32_submit twice, call 0 rejected.  forward: a[1] is q[0] (pre-filled with acceptable data); backward: q[1] is a[0].
    Finishing both must leave what the two blocking calls leave."""
    torch = torch_cuda
    m, n, _, mode = SHAPES["f32_32768x64"]
    md = bq.compute_mode[mode]
    case = Case(torch, m, n, "f32", "feed_forward" if direction == "forward" else "backward", (0,), seed=300)
    bf = buffers("f32_32768x64")
    want = case.pool.clone()
    qs, rs, as_ = case.views(want)
    for i in range(2):
        assert bq.qr(qs[i], m, rs[i], n, as_[i], m, m, n, bf) == 0
        if i == 0:
            assert bq.last_engine() not in (3, 5)
    pool = case.pool.clone()
    qs, rs, as_ = case.views(pool)
    t0 = bq.submit(qs[0], m, rs[0], n, as_[0], m, m, n, bf)
    t1 = bq.submit(qs[1], m, rs[1], n, as_[1], m, m, n, bf)
    assert bq.finish(t0) == 0 and bq.finish(t1) == 0
    # (calls 2 and 3 of the layout were not made: compare everything the two calls could touch -- the whole pool)
    assert torch.equal(case.bits(pool), case.bits(want))


def test_loop_in_place_rejected_matrix(bq, oracle, torch_cuda, buffers):
    """bind_loop with q == a on a matrix the bf16-split level rejects, at depths 1 / 2 / 3: the loop entries keep two calls in flight in
    place.  Call i rejected leaves A untouched, so attempt i + 1 sees that same matrix; then the ladder of call i writes its Q over A, and
    call i + 1 must factor that Q exactly as the blocking loop does."""
    torch = torch_cuda
    m, n = 1 << 15, 64
    bf = buffers("f32_32768x64")
    a = oracle.matrix_with_cond(m, n, COND_BAD, seed=400)
    res = []
    for depth in (1, 2, 3):
        d_a = torch.from_numpy(np.ascontiguousarray(a.T)).cuda()
        d_r = torch.zeros(n, n, dtype=torch.float32, device="cuda")
        bq.set_loop_depth(depth)
        try:
            assert bq.bind_loop(d_a, m, d_r, n, d_a, m, m, n, bf)(3) == 0
        finally:
            bq.set_loop_depth(3)
        res.append((d_a.view(torch.int32).cpu().numpy(), d_r.view(torch.int32).cpu().numpy()))
    for k in (1, 2):
        assert np.array_equal(res[0][0], res[k][0]) and np.array_equal(res[0][1], res[k][1]), "depth %d" % (k + 1)
    q = res[0][0].view(np.float32).T.astype(np.float64)
    assert oracle.orthogonality_fro(q) < 5e-6

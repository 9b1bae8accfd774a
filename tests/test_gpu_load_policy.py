"""GPU tests of the load policy of A (tsqr_mi_set_load_policy / tsqr_mi_get_load_policy, include/tsqr_mi.h): cache-allocating (1) or
streamed (2) loads in the two passes of a full 64-column call -- gram_blk_kernel<NT_A> and the plain 64-row apply kernel's NT_A instance.

A load policy does not touch the arithmetic, so every comparison below is BYTE FOR BYTE: Q (its whole buffer, padding included), R and the
verdict words the call leaves in the pinned words.  Every input is U(-1, 1) and every call must be accepted at the bf16-split level
(last_engine() == 3): a rejected Gram matrix would leave the two kernels, and the comparison would pass without running them."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODES = ["fp32_tc_cor", "fp32_notc"]
# 128 rows: one Gram block; 384: three; 131072: the smallest with nblk >= 2 * nwg in the Gram pass (the uneven old / young split) and a
# multiple of 16 x 256 apply blocks (the apply pass's share path can engage)
ELIGIBLE_ROWS = [128, 384, 4096, 65536, 131072]

_inputs = {}


def uniform(m, n):
    if (m, n) not in _inputs:
        _inputs[(m, n)] = np.random.default_rng(1000 * n + m % 997).uniform(-1.0, 1.0, size=(n, m)).astype(np.float32)   # column-major m x n
    return _inputs[(m, n)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture()
def policy(bq):
    """sets the policy for a test; the process's initial setting and the default loop depth are back afterwards"""
    L = bq.lib()
    yield L.tsqr_mi_set_load_policy
    L.tsqr_mi_set_load_policy(int(os.environ.get("TSQR_MI_LOAD_POLICY", "0")))
    bq.set_loop_depth(3)


def run(bq, torch, mode, m, n, lda, depth=0, a_shift=0):
    """One blocking call (depth 0) or three calls of the loop entry at loop depth `depth` -> (Q buffer, R, verdict words) as bytes."""
    md = bq.compute_mode[mode]
    a = uniform(m, n)
    store = torch.zeros(n * lda + a_shift, dtype=torch.float32, device="cuda")
    d_a = store[a_shift:]
    d_a[:n * lda].view(n, lda)[:, :m] = torch.from_numpy(a).cuda()
    d_q = torch.full((n * lda,), float("nan"), dtype=torch.float32, device="cuda")
    d_r = torch.zeros(n * n, dtype=torch.float32, device="cuda")
    bf = bq.buffer(md, False)
    bf.allocate(m, n)
    bf.hl.zero_()
    if depth == 0:
        st = bq.qr(d_q, lda, d_r, n, d_a, lda, m, n, bf)
    else:
        bq.set_loop_depth(depth)
        st = bq.bind_loop(d_q, lda, d_r, n, d_a, lda, m, n, bf)(3)
    torch.cuda.synchronize()
    assert st == 0 and bq.last_engine() == 3, (st, bq.last_engine())     # accepted at the bf16-split level: the two kernels ran
    assert np.array_equal(d_a[:n * lda].view(n, lda)[:, :m].cpu().numpy(), a)   # A untouched
    words = bf.hl.numpy().copy()
    verdicts = np.concatenate([words[0:3], words[4:7]])                  # (words 3 and 7 are completion words: sequence numbers)
    return d_q.cpu().numpy().tobytes(), d_r.cpu().numpy().tobytes(), verdicts.tobytes()


@pytest.mark.parametrize("pad", [0, 64])
@pytest.mark.parametrize("m", ELIGIBLE_ROWS)
@pytest.mark.parametrize("mode", MODES)
def test_streamed_loads_change_no_bit(bq, torch_cuda, policy, mode, m, pad):
    L = bq.lib()
    n, lda = 64, m + pad
    res = {}
    for p in (1, 2):
        policy(p)
        for depth in (0, 1, 2):
            res[p, depth] = run(bq, torch_cuda, mode, m, n, lda, depth)
            assert L.tsqr_mi_get_load_policy() == p                      # the call took the kernels the policy is about, with that policy
    for depth in (0, 1, 2):
        assert res[1, depth] == res[2, depth], "policy 1 against 2, depth %d" % depth
    for p in (1, 2):
        assert res[p, 1][:2] == res[p, 0][:2] and res[p, 2][:2] == res[p, 0][:2], "loop depths against the blocking call, policy %d" % p
        assert res[p, 1][2][:12] == res[p, 0][2][:12]                    # (the first half of the verdict words: every depth-1 call uses it)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("m,n,shift", [(4095, 64, 0), (4096, 63, 0), (4096, 64, 1)])
def test_other_shapes_keep_their_kernels(bq, torch_cuda, policy, mode, m, n, shift):
    """rows no multiple of 128, fewer than 64 columns, columns that are not 16-byte aligned: not gram_blk_kernel's operands -- a pinned
    streamed policy changes nothing for them and they do not show in the getter"""
    L = bq.lib()
    policy(1)
    run(bq, torch_cuda, mode, 128, 64, 128)                              # an eligible call: the getter now says 1
    assert L.tsqr_mi_get_load_policy() == 1
    lda = (m + 3) & ~3                                                   # (a leading dimension the block kernel would take)
    want = run(bq, torch_cuda, mode, m, n, lda, a_shift=shift)
    policy(2)
    got = run(bq, torch_cuda, mode, m, n, lda, a_shift=shift)
    assert L.tsqr_mi_get_load_policy() == 1
    assert got == want


def test_auto_rule_below_the_size_threshold(bq, torch_cuda, policy):
    """65536 x 64 is 16 MiB, far below the 128 MiB the auto rule measures at: cache-allocating loads without a measurement; a pinned
    streamed policy is honoured at that size"""
    L = bq.lib()
    policy(2)
    two = run(bq, torch_cuda, "fp32_tc_cor", 65536, 64, 65536)
    assert L.tsqr_mi_get_load_policy() == 2
    policy(0)
    auto = run(bq, torch_cuda, "fp32_tc_cor", 65536, 64, 65536)
    assert L.tsqr_mi_get_load_policy() == 1
    assert auto == two
    policy(7)                                                            # (an unknown value is the auto setting)
    run(bq, torch_cuda, "fp32_tc_cor", 65536, 64, 65536)
    assert L.tsqr_mi_get_load_policy() == 1

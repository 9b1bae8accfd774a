"""CPU tests of the operand check of the batch entries (blockqr.check_batch_operands, used by blockqr.bind_batch and by the
row-partitioned bind_batch): a wrong dtype, a tensor off the GPU, a leading dimension below the rows or a tensor too small for its operand
raises TypeError / ValueError before anything reaches the C side, which reads raw pointers.  Only CPU tensors are used here."""
import types

import pytest


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def trio(torch, m, n, ldq, ldr, lda, dtype=None, k=2):
    dtype = dtype or torch.float32
    return ([torch.zeros((n - 1) * ldq + m, dtype=dtype) for _ in range(k)], [torch.zeros((n - 1) * ldr + n, dtype=dtype) for _ in range(k)],
            [torch.zeros((n - 1) * lda + m, dtype=dtype) for _ in range(k)])


def test_wrong_inputs_raise(bq, torch):
    m, n = 100, 8
    qs, rs, as_ = trio(torch, m, n, m, n, m)
    # every size is exactly enough: the only complaint left is that CPU tensors are not on the GPU
    with pytest.raises(TypeError, match="not a GPU tensor"):
        bq.check_batch_operands(qs, m, rs, n, as_, m, m, n)
    with pytest.raises(TypeError, match="float16"):                 # dtype first: an fp32 tensor for an fp16 mode
        bq.check_batch_operands(qs, m, rs, n, as_, m, m, n, half=True)
    h = trio(torch, m, n, m, n, m, dtype=torch.float16)
    with pytest.raises(TypeError, match="float32"):
        bq.check_batch_operands(h[0], m, h[1], n, h[2], m, m, n)
    with pytest.raises(TypeError, match="float32"):                 # one wrong tensor among right ones
        bq.check_batch_operands(qs, m, rs, n, [as_[0], as_[1].double()], m, m, n)
    for ldq, ldr, lda in ((m - 1, n, m), (m, n - 1, m), (m, n, m - 1)):
        with pytest.raises(ValueError, match="smaller than"):
            bq.check_batch_operands(qs, ldq, rs, ldr, as_, lda, m, n)
    for short in range(3):                                          # one element short, in q, r or a
        t = list(trio(torch, m, n, m, n, m))
        t[short] = [t[short][0], t[short][1][:-1]]
        with pytest.raises(ValueError, match="elements"):
            bq.check_batch_operands(t[0], m, t[1], n, t[2], m, m, n)
    big = trio(torch, m, n, m + 4, n, m)                            # ld larger than the rows: (n - 1) ld + rows elements are needed
    with pytest.raises(ValueError, match="elements"):
        bq.check_batch_operands(big[0], m + 4, big[1], n, [a[:-1] for a in big[2]], m, m, n)
    with pytest.raises(ValueError, match="same number"):
        bq.check_batch_operands(qs, m, rs[:1], n, as_, m, m, n)


def test_bind_batch_checks_before_the_gpu(bq, torch):
    """both batch binders refuse CPU and mistyped tensors (nothing here may reach the library's compute entries)"""
    m, n = 64, 4
    qs, rs, as_ = trio(torch, m, n, m, n, m)
    bf = types.SimpleNamespace(mode=bq.compute_mode.fp32_tc_cor, reorthogonalize=False)
    with pytest.raises(TypeError):
        bq.bind_batch(qs, m, rs, n, as_, m, m, n, bf)
    bf16 = types.SimpleNamespace(mode=bq.compute_mode.fp16_notc, reorthogonalize=False)
    with pytest.raises(TypeError):
        bq.bind_batch(qs, m, rs, n, as_, m, m, n, bf16)
    from tsqr_gpu_amd import dist as tdist
    backend = types.SimpleNamespace(n=n, _check_block=lambda m_local: None)
    with pytest.raises(TypeError):
        tdist.HipBackend.bind_batch(backend, qs, m, rs, n, as_, m, m, False)
    with pytest.raises(ValueError):
        tdist.HipBackend.bind_batch(backend, qs, m - 1, rs, n, as_, m, m, False)

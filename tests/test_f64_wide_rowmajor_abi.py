"""CPU tests of the wide QR's layout entry (tsqr_mi_qr_f64_wide_lay): the symbol and its prototype, the order of the argument checks
that come before any HIP call, the forwarding of n <= 64 to tsqr_mi_qr_f64_lay, the unchanged column-major entry and work-space sizes,
the row-major operand rules behind qr_f64_wide(row_major=True), the argument errors of qr_f64_wide_tensor, and a C++ caller of the
layout arguments of mtk::qr::qr_fp64_wide (tests/cpp/sample_fp64_wide_rowmajor.cpp)."""
import ctypes
import inspect
import os
import subprocess

import pytest

from abi_util import compile_and_link, header_flat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COL, ROW = 0, 1


def test_symbol_prototype_and_hooks(bq):
    L = ctypes.CDLL(bq.LIB_PATH)
    flat = header_flat()
    assert hasattr(L, "tsqr_mi_qr_f64_wide_lay")
    assert "tsqr_mi_qr_f64_wide_lay" in bq.C_ABI_SYMBOLS
    assert ("int tsqr_mi_qr_f64_wide_lay(int a_layout, int q_layout, int reorth, double* q, size_t ldq, double* r, size_t ldr, double* a, "
            "size_t lda, size_t m, size_t n, void* wq, void* wr, void* stream);") in flat
    # the old entry's declaration stays as it was
    assert ("int tsqr_mi_qr_f64_wide(int reorth, double* q, size_t ldq, double* r, size_t ldr, double* a, size_t lda, size_t m, size_t n, "
            "void* wq, void* wr, void* stream);") in flat
    sel = ctypes.CDLL(os.path.join(ROOT, "tsqr_gpu_amd", "csrc", "libtsqr_selftest.so"))
    for name in ("tsqr_selftest_f64w_gram_lay", "tsqr_selftest_f64w_gram", "tsqr_selftest_f64w_apply_lay", "tsqr_selftest_f64w_apply"):
        assert hasattr(sel, name), name
    ci, vp, sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    assert bq.lib().tsqr_mi_qr_f64_wide_lay.argtypes == [ci, ci, ci, vp, sz, vp, sz, vp, sz, sz, sz, vp, vp, vp]
    import tsqr_gpu_amd
    assert tsqr_gpu_amd.qr_f64_wide_tensor is bq.qr_f64_wide_tensor


def test_argument_check_order_without_gpu(bq):
    # every check comes before any HIP call: null pointers are safe.  With null pointers q == a, so the in-place rule is the LAST check
    # a call can meet: one that passes equal layouts and leading dimensions would go on to the device and is not made here.
    L = bq.lib()
    z = ctypes.c_void_p(0)
    bad, unsupported = bq.error_invalid_matrix_size, bq.error_unsupported_mode
    m, n = 300, 100

    def qr(al, ql, ldq, lda, m=m, n=n, ldr=None, reorth=0):
        return L.tsqr_mi_qr_f64_wide_lay(al, ql, reorth, z, ldq, z, n if ldr is None else ldr, z, lda, m, n, z, z, z)

    # 1. a layout other than 0 or 1 -- before the sizes and before "unsupported"
    for lay in (2, -1, 7):
        assert qr(lay, COL, m, m) == bad and qr(COL, lay, m, m) == bad and qr(ROW, lay, n, n) == bad and qr(lay, ROW, n, n) == bad
    assert qr(2, COL, 2000, 2000, m=2000, n=1025) == bad
    # 2. leading dimensions: below m column-major, below n row-major (ld = n < m is fine there); ldr; n > m; empty
    assert qr(COL, COL, m - 1, m) == bad and qr(COL, COL, m, m - 1) == bad
    assert qr(ROW, ROW, n - 1, n) == bad and qr(ROW, ROW, n, n - 1) == bad
    assert qr(ROW, COL, m - 1, n) == bad and qr(ROW, COL, m, n - 1) == bad
    assert qr(COL, ROW, n - 1, m) == bad and qr(COL, ROW, n, m - 1) == bad
    assert qr(ROW, ROW, n, n, ldr=n - 1) == bad and qr(COL, COL, m, m, ldr=n - 1) == bad
    for (mm, nn) in [(80, 100), (0, 0), (0, 70), (70, 0)]:
        for lay in (COL, ROW):
            assert qr(lay, lay, max(mm, nn, 1), max(mm, nn, 1), m=mm, n=nn, ldr=max(nn, 1)) == bad
    # 3. n > 1024: state 2 with a text, in every layout pair, behind the size checks and in front of the in-place rule
    for al, ql, ldq, lda in ((ROW, ROW, 1025, 1025), (COL, COL, 2000, 2000), (ROW, COL, 2000, 1025), (COL, ROW, 1025, 2000)):
        assert qr(al, ql, ldq, lda, m=2000, n=1025, ldr=1025, reorth=1) == unsupported
        assert "n <= 1024" in bq.last_error()
    assert qr(ROW, ROW, 1025, 1026, m=2000, n=1025, ldr=1025) == unsupported      # (q == a with unequal strides: "unsupported" comes first)
    assert qr(ROW, ROW, 1024, 1025, m=2000, n=1025, ldr=1025) == bad and qr(ROW, ROW, 1025, 1024, m=2000, n=1025, ldr=1025) == bad
    # 4. q == a (here: both null) with different layouts or different leading dimensions
    assert qr(ROW, COL, m, m) == bad and qr(COL, ROW, m, m) == bad
    assert qr(ROW, ROW, n, n + 1) == bad and qr(COL, COL, m, m + 1) == bad
    assert L.tsqr_mi_last_sweeps_f64() == 0


def test_forwarding_for_one_panel_without_gpu(bq):
    """n <= 64: what tsqr_mi_qr_f64_lay rejects, the wide entry rejects with the same state"""
    L = bq.lib()
    z = ctypes.c_void_p(0)
    m, n = 100, 8
    cases = [(2, COL, m, m, n), (ROW, ROW, n - 1, n, n), (ROW, ROW, n, n - 1, n), (COL, ROW, n, m - 1, n), (ROW, COL, m - 1, n, n),
             (COL, COL, m, m, n - 1), (ROW, COL, m, m, n), (COL, ROW, m, m, n), (ROW, ROW, n, n + 1, n), (COL, COL, m, m + 1, n)]
    for al, ql, ldq, lda, ldr in cases:
        want = L.tsqr_mi_qr_f64_lay(al, ql, 0, z, ldq, z, ldr, z, lda, m, n, z, z, z)
        assert want == bq.error_invalid_matrix_size
        assert L.tsqr_mi_qr_f64_wide_lay(al, ql, 0, z, ldq, z, ldr, z, lda, m, n, z, z, z) == want, (al, ql, ldq, lda, ldr)
    # n = 64 is the last one-panel size, n = 65 the first wide one: the narrow entry stops there, the wide one does not (both calls end at
    # the in-place rule, which sits behind the "unsupported" check of either)
    assert L.tsqr_mi_qr_f64_lay(ROW, ROW, 0, z, 65, z, 65, z, 66, 100, 65, z, z, z) == bq.error_unsupported_mode
    assert L.tsqr_mi_qr_f64_wide_lay(ROW, ROW, 0, z, 65, z, 65, z, 66, 100, 65, z, z, z) == bq.error_invalid_matrix_size
    assert L.tsqr_mi_qr_f64_wide_lay(ROW, ROW, 0, z, 64, z, 64, z, 65, 100, 64, z, z, z) == bq.error_invalid_matrix_size


def test_old_entry_and_work_space_sizes_unchanged(bq):
    L = bq.lib()
    z = ctypes.c_void_p(0)
    for (m, n) in [(80, 100), (0, 0), (0, 70), (70, 0)]:
        assert L.tsqr_mi_qr_f64_wide(0, z, max(m, 1), z, max(n, 1), z, max(m, 1), m, n, z, z, z) == bq.error_invalid_matrix_size
    assert L.tsqr_mi_qr_f64_wide(1, z, 2000, z, 1025, z, 2000, 2000, 1025, z, z, z) == bq.error_unsupported_mode
    assert L.tsqr_mi_qr_f64_wide(0, z, 299, z, 100, z, 300, 300, 100, z, z, z) == bq.error_invalid_matrix_size
    assert L.tsqr_mi_qr_f64_wide(0, z, 300, z, 100, z, 100, 300, 100, z, z, z) == bq.error_invalid_matrix_size   # lda = n is row-major's rule only
    # one size for every layout: six block stores of npairs 64 x 64 blocks and a little more; partials capped at 8 Mi doubles
    nb = 4
    npairs = nb * (nb + 1) // 2
    bs = npairs * 4096
    assert L.tsqr_mi_working_q_size_f64_wide(1 << 18, 256) == 6 * bs + 64 + nb * 4096 + nb * (nb + 1) + 2 * nb + 8
    assert L.tsqr_mi_working_r_size_f64_wide(1 << 18, 256) <= 8 << 20
    assert L.tsqr_mi_working_r_size_f64_wide(1 << 18, 256) % bs == 0
    assert L.tsqr_mi_working_q_size_f64_wide(100, 8) == L.tsqr_mi_working_q_size_f64(100, 8)


def test_qr_f64_wide_row_major_applies_the_operand_rules(bq, monkeypatch):
    """qr_f64_wide(row_major=True) hands check_f64_operands the row-major rules (ld >= n, room for (m - 1) ld + n doubles) before
    anything is launched; CPU tensors are refused before that"""
    import torch
    assert inspect.signature(bq.qr_f64_wide).parameters["row_major"].default is False
    m, n = 300, 100
    a = torch.zeros(m, n, dtype=torch.float64)
    r = torch.zeros(n, n, dtype=torch.float64)
    with pytest.raises(TypeError):
        bq.qr_f64_wide(torch.zeros_like(a), n, r, n, a, n, m, n, bq.buffer_f64_wide(False), row_major=True)     # CPU tensors
    with pytest.raises(TypeError):
        bq.qr_f64_wide(torch.zeros_like(a), n, r, n, a.float(), n, m, n, bq.buffer_f64_wide(False), row_major=True)

    class FakeDev(torch.Tensor):
        """a float64 tensor that claims to live on the GPU at an address of the test's choosing, with no memory behind it: the checks
        run, and the call must end before a launch"""
        is_cuda = True

        def data_ptr(self):
            return self.addr

        def numel(self):
            return self.count

    def fake(addr, numel):
        t = torch.zeros(1, dtype=torch.float64).as_subclass(FakeDev)
        t.addr, t.count = addr, numel
        return t

    seen = []
    real = bq.check_f64_operands
    monkeypatch.setattr(bq, "check_f64_operands", lambda *args, **kw: (seen.append(kw.get("row_major")), real(*args, **kw))[1])
    base, far = 1 << 20, 1 << 26
    rr = fake(1 << 28, n * n)
    bf = bq.buffer_f64_wide(False)

    def call(ldq, lda, q, a_, r_=rr, ldr=n, row_major=True):
        return bq.qr_f64_wide(q, ldq, r_, ldr, a_, lda, m, n, bf, row_major=row_major)

    with pytest.raises(ValueError):
        call(n - 1, n, fake(far, m * n), fake(base, m * n))             # ldq < n
    with pytest.raises(ValueError):
        call(n, n - 1, fake(far, m * n), fake(base, m * n))             # lda < n
    with pytest.raises(ValueError):
        call(n + 3, n, fake(far, (m - 1) * (n + 3) + n - 1), fake(base, m * n))      # q one element short of (m - 1) ld + n
    with pytest.raises(ValueError):
        call(n, n, fake(base + 8, m * n), fake(base, m * n + 1))        # q overlaps a without being a
    with pytest.raises(ValueError):
        call(n + 3, n + 4, fake(base, m * (n + 4)), fake(base, m * (n + 4)))         # in place with ldq != lda
    with pytest.raises(ValueError):
        call(n, n, fake(far, m * n), fake(base, m * n), r_=fake(far + 8, n * n))  # r overlaps q
    with pytest.raises(ValueError):
        call(n, n, fake(far, m * n), fake(base, m * n), row_major=False)             # the same operands column-major: ld < m
    assert seen == [True] * 6 + [False]
    # operands that pass the rules (contiguous, and exactly the padded spans) reach the buffer check: nothing is allocated, nothing launched
    for ldq, lda, q, a_ in ((n, n, fake(far, m * n), fake(base, m * n)),
                            (n + 3, n + 5, fake(far, (m - 1) * (n + 3) + n), fake(base, (m - 1) * (n + 5) + n)),
                            (n + 3, n + 3, fake(base, m * (n + 3)), fake(base, m * (n + 3)))):
        with pytest.raises(RuntimeError, match="not allocated"):
            call(ldq, lda, q, a_)
    # sizes the entry refuses come back as states, through the _lay entry
    assert bq.qr_f64_wide(fake(far, 1), 1025, rr, 1025, fake(base, 1), 1025, 2000, 1025, bf, row_major=True) == bq.error_unsupported_mode
    assert bq.qr_f64_wide(fake(far, 1), 8, rr, 8, fake(base, 1), 8, 4, 8, bf, row_major=True) == bq.error_invalid_matrix_size


def test_qr_f64_wide_tensor_argument_errors(bq):
    import torch
    sig = inspect.signature(bq.qr_f64_wide_tensor)
    assert list(sig.parameters) == ["a", "reorth", "overwrite_a", "stream"]
    assert [sig.parameters[k].default for k in ("reorth", "overwrite_a", "stream")] == [False, False, None]
    a = torch.zeros(300, 100, dtype=torch.float64)
    with pytest.raises(TypeError):
        bq.qr_f64_wide_tensor(a)                               # a CPU tensor
    with pytest.raises(TypeError):
        bq.qr_f64_wide_tensor(a.float())                       # wrong dtype
    with pytest.raises(TypeError):
        bq.qr_f64_wide_tensor(a.numpy())                       # not a tensor
    if torch.cuda.is_available():                              # (the GPU box: the rank check sits behind the device check, as in qr_f64_tensor)
        with pytest.raises(ValueError):
            bq.qr_f64_wide_tensor(torch.zeros(100, dtype=torch.float64, device="cuda"))
        with pytest.raises(ValueError):
            bq.qr_f64_wide_tensor(torch.zeros(10, 4, 2, dtype=torch.float64, device="cuda"))
        with pytest.raises(TypeError):
            bq.qr_f64_wide_tensor(torch.zeros(300, 100, dtype=torch.float32, device="cuda"))


def test_cpp_layout_sample_compiles_links_and_runs(bq):
    src = os.path.join(ROOT, "tests", "cpp", "sample_fp64_wide_rowmajor.cpp")
    with compile_and_link(src, "sample_fp64_wide_rowmajor") as exe:
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "argument checks ok" in out.stdout

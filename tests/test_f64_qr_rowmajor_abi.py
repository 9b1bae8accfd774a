"""CPU tests of the full QR's layout entry (tsqr_mi_qr_f64_lay): the symbol and its prototype, the argument checks that come before any
HIP call, the unchanged column-major entry and work-space sizes, the row-major span and overlap rules of check_f64_operands, the
argument errors of qr_f64_tensor, and a C++ caller of the layout arguments of mtk::qr::qr_fp64 (tests/cpp/sample_fp64_qr_rowmajor.cpp)."""
import ctypes
import inspect
import os
import subprocess

import pytest

from abi_util import compile_and_link, header_flat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COL, ROW = 0, 1


def test_symbol_prototype_and_hook(bq):
    L = ctypes.CDLL(bq.LIB_PATH)
    flat = header_flat()
    assert hasattr(L, "tsqr_mi_qr_f64_lay")
    assert "tsqr_mi_qr_f64_lay" in bq.C_ABI_SYMBOLS
    assert ("int tsqr_mi_qr_f64_lay(int a_layout, int q_layout, int reorth, double* q, size_t ldq, double* r, size_t ldr, double* a, "
            "size_t lda, size_t m, size_t n, void* wq, void* wr, void* stream);") in flat
    # the old entry's declaration stays as it was
    assert ("int tsqr_mi_qr_f64(int reorth, double* q, size_t ldq, double* r, size_t ldr, double* a, size_t lda, size_t m, size_t n, "
            "void* wq, void* wr, void* stream);") in flat
    sel = ctypes.CDLL(os.path.join(ROOT, "tsqr_gpu_amd", "csrc", "libtsqr_selftest.so"))
    assert hasattr(sel, "tsqr_selftest_f64_apply_lay") and hasattr(sel, "tsqr_selftest_f64_apply")
    ci, vp, sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    assert bq.lib().tsqr_mi_qr_f64_lay.argtypes == [ci, ci, ci, vp, sz, vp, sz, vp, sz, sz, sz, vp, vp, vp]


def test_argument_checks_without_gpu(bq):
    # every check comes before any HIP call: null pointers are safe.  (With null pointers q == a, so a call that is to get past the
    # in-place rule passes equal layouts and leading dimensions; n = 65 shows that the size checks were passed: state 2 lies behind them.)
    L = bq.lib()
    z = ctypes.c_void_p(0)
    bad, unsupported = bq.error_invalid_matrix_size, bq.error_unsupported_mode
    m, n = 100, 8

    def qr(al, ql, ldq, lda, m=m, n=n, ldr=None, reorth=0):
        return L.tsqr_mi_qr_f64_lay(al, ql, reorth, z, ldq, z, n if ldr is None else ldr, z, lda, m, n, z, z, z)

    for lay in (2, -1, 7):
        assert qr(lay, COL, m, m) == bad and qr(COL, lay, m, m) == bad and qr(ROW, lay, n, n) == bad and qr(lay, ROW, n, n) == bad
    assert qr(2, COL, 100, 100, n=65) == bad                  # a layout error comes before "unsupported"
    # leading dimensions: below m column-major, below n row-major (lda = n < m is fine there)
    assert qr(COL, COL, m - 1, m) == bad and qr(COL, COL, m, m - 1) == bad
    assert qr(ROW, ROW, n - 1, n) == bad and qr(ROW, ROW, n, n - 1) == bad
    assert qr(ROW, COL, m - 1, n) == bad and qr(ROW, COL, m, n - 1) == bad
    assert qr(COL, ROW, n - 1, m) == bad and qr(COL, ROW, n, m - 1) == bad
    assert qr(ROW, ROW, n, n, ldr=n - 1) == bad and qr(COL, COL, m, m, ldr=n - 1) == bad
    for (mm, nn) in [(4, 8), (0, 0), (0, 4), (4, 0)]:
        for lay in (COL, ROW):
            assert qr(lay, lay, max(mm, nn, 1), max(mm, nn, 1), m=mm, n=nn, ldr=max(nn, 1)) == bad
    # n > 64: state 2 with a text, in every layout pair, reached only behind the size checks
    for al, ql, ldq, lda in ((ROW, ROW, 65, 65), (COL, COL, 100, 100), (ROW, COL, 100, 65), (COL, ROW, 65, 100)):
        assert qr(al, ql, ldq, lda, n=65, ldr=65, reorth=1) == unsupported
        assert "n <= 64" in bq.last_error()
    assert qr(ROW, ROW, 64, 65, n=65, ldr=65) == bad and qr(ROW, ROW, 65, 64, n=65, ldr=65) == bad
    # q == a (here: both null) with different layouts or different leading dimensions
    assert qr(ROW, COL, m, m) == bad and qr(COL, ROW, m, m) == bad
    assert qr(ROW, ROW, n, n + 1) == bad and qr(COL, COL, m, m + 1) == bad
    assert L.tsqr_mi_last_sweeps_f64() == 0


def test_old_entry_and_work_space_sizes_unchanged(bq):
    L = bq.lib()
    z = ctypes.c_void_p(0)
    for (m, n) in [(4, 8), (0, 0), (0, 4), (4, 0)]:
        assert L.tsqr_mi_qr_f64(0, z, max(m, 1), z, max(n, 1), z, max(m, 1), m, n, z, z, z) == bq.error_invalid_matrix_size
    assert L.tsqr_mi_qr_f64(1, z, 100, z, 65, z, 100, 100, 65, z, z, z) == bq.error_unsupported_mode
    assert L.tsqr_mi_qr_f64(0, z, 99, z, 8, z, 100, 100, 8, z, z, z) == bq.error_invalid_matrix_size
    assert L.tsqr_mi_qr_f64(0, z, 100, z, 8, z, 8, 100, 8, z, z, z) == bq.error_invalid_matrix_size      # lda = n is row-major's rule only
    # wq: [Z 4096][R 4096][16 tiles + 8][8] doubles; wr: the Gram plan's partials (64-row chunks on at most 2048 waves, 4 to a workgroup)
    assert L.tsqr_mi_working_q_size_f64(1 << 20, 64) == 4096 + 4096 + 16 * 256 + 8 + 8
    assert L.tsqr_mi_working_q_size_f64(100, 8) == L.tsqr_mi_working_q_size_f64(1 << 20, 64)
    assert L.tsqr_mi_working_r_size_f64(1 << 20, 64) == 512 * 10 * 256
    assert L.tsqr_mi_working_r_size_f64(100, 8) == 1 * 1 * 256
    assert L.tsqr_mi_working_r_size_f64(4097, 33) == 17 * 6 * 256
    assert L.tsqr_mi_working_q_size_f64(0, 8) == 0 and L.tsqr_mi_working_r_size_f64(8, 0) == 0


def test_check_f64_operands_row_major_span_and_overlap():
    from tsqr_gpu_amd import blockqr as bq
    m, n = 100, 8
    base = 1 << 20
    far = 1 << 24
    r = (base + (1 << 18), n * n)

    def chk(ldq, lda, q, a, r=r, ldr=n):
        return bq.check_f64_operands(m, n, ldq, ldr, lda, q, r, a, row_major=True)

    chk(n, n, (far, m * n), (base, m * n))                                          # contiguous
    chk(n + 3, n + 5, (far, (m - 1) * (n + 3) + n), (base, (m - 1) * (n + 5) + n))  # exactly the spans (m - 1) ld + n
    with pytest.raises(ValueError):
        chk(n + 3, n, (far, (m - 1) * (n + 3) + n - 1), (base, m * n))              # q one element short
    with pytest.raises(ValueError):
        chk(n, n + 5, (far, m * n), (base, (m - 1) * (n + 5) + n - 1))              # a one element short
    with pytest.raises(ValueError):
        chk(n - 1, n, (far, m * n), (base, m * n))                                  # ldq < n
    with pytest.raises(ValueError):
        chk(n, n - 1, (far, m * n), (base, m * n))                                  # lda < n
    with pytest.raises(ValueError):
        chk(n, n, (far, m * n), (base, m * n), ldr=n - 1)
    with pytest.raises(ValueError):
        bq.check_f64_operands(m, n, n, n, n, (far, m * n), r, (base, m * n))        # the same operands as column-major: ld < m
    # in place: the very operand with the same leading dimension; any other overlap of q and a is refused
    chk(n + 3, n + 3, (base, m * (n + 3)), (base, m * (n + 3)))
    with pytest.raises(ValueError):
        chk(n + 3, n + 4, (base, m * (n + 4)), (base, m * (n + 4)))
    with pytest.raises(ValueError):
        chk(n, n, (base + 8, m * n), (base, m * n + 1))
    span = 8 * ((m - 1) * (n + 3) + n)
    chk(n, n + 3, (base + span, m * n), (base, m * (n + 3)))                        # q begins where the span of a ends: apart
    with pytest.raises(ValueError):
        chk(n, n + 3, (base + span - 8, m * n), (base, m * (n + 3)))                # one double inside it
    # r apart from both
    chk(n, n + 3, (far, m * n), (base, m * (n + 3)), r=(base + span, n * n))
    with pytest.raises(ValueError):
        chk(n, n + 3, (far, m * n), (base, m * (n + 3)), r=(base + span - 8, n * n))
    with pytest.raises(ValueError):
        chk(n, n, (far, m * n), (base, m * n), r=(far + 8 * (m * n - 1), n * n))
    with pytest.raises(ValueError):
        chk(n, n, (far, m * n), (base, m * n), r=(far - 8 * n * n + 8, n * n))
    assert inspect.signature(bq.check_f64_operands).parameters["row_major"].default is False


def test_python_surfaces_are_checked_on_the_cpu(bq):
    import torch
    assert inspect.signature(bq.qr_f64).parameters["row_major"].default is False
    sig = inspect.signature(bq.qr_f64_tensor)
    assert [sig.parameters[k].default for k in ("reorth", "overwrite_a", "stream")] == [False, False, None]
    assert issubclass(bq.QrError, RuntimeError) and bq.QrError(3, "x").state == 3 and not issubclass(bq.QrError, bq.LstsqError)
    a = torch.zeros(100, 8, dtype=torch.float64)
    r = torch.zeros(8, 8, dtype=torch.float64)
    with pytest.raises(TypeError):
        bq.qr_f64(torch.zeros_like(a), 8, r, 8, a, 8, 100, 8, bq.buffer_f64(False), row_major=True)     # CPU tensors
    with pytest.raises(TypeError):
        bq.qr_f64_tensor(a)                                    # a CPU tensor
    with pytest.raises(TypeError):
        bq.qr_f64_tensor(a.float())                            # wrong dtype
    with pytest.raises(TypeError):
        bq.qr_f64_tensor(a.numpy())                            # not a tensor
    if torch.cuda.is_available():                              # (the GPU box: the rank check sits behind the device check)
        with pytest.raises(ValueError):
            bq.qr_f64_tensor(torch.zeros(100, dtype=torch.float64, device="cuda"))
        with pytest.raises(ValueError):
            bq.qr_f64_tensor(torch.zeros(10, 4, 2, dtype=torch.float64, device="cuda"))
        with pytest.raises(TypeError):
            bq.qr_f64_tensor(torch.zeros(100, 8, dtype=torch.float32, device="cuda"))


def test_cpp_layout_sample_compiles_links_and_runs(bq):
    src = os.path.join(ROOT, "tests", "cpp", "sample_fp64_qr_rowmajor.cpp")
    with compile_and_link(src, "sample_fp64_qr_rowmajor") as exe:
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "argument checks ok" in out.stdout

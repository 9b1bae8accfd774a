"""CPU tests of the fp64 pivoted QR entry (tsqr_mi_qrcp_f64): exported symbols and their signatures, work-space sizes, the argument
checks that come before any HIP call, the Python operand checks of qrcp_f64 and qrcp_f64_tensor, and a C++ caller of
mtk::qr::qrcp_fp64 (tests/cpp/sample_fp64_qrcp.cpp) that compiles and links."""
import ctypes
import os

import pytest

from abi_util import compile_and_link, header_flat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QRCP_SYMBOLS = ("tsqr_mi_qrcp_f64", "tsqr_mi_working_q_size_f64_qrcp", "tsqr_mi_working_r_size_f64_qrcp")
QRCP_BLOCK = 4096 + 8                  # H and the status words: what jobq = 1 adds to the QR entry's wq, for every m
COL, ROW = 0, 1


def test_qrcp_symbols_exported_with_the_stated_signatures(bq):
    L = ctypes.CDLL(bq.LIB_PATH)
    flat = header_flat()
    for sym in QRCP_SYMBOLS:
        assert hasattr(L, sym), sym
        assert sym in bq.C_ABI_SYMBOLS, sym
    assert "size_t tsqr_mi_working_q_size_f64_qrcp(size_t m, size_t n, int jobq);" in flat
    assert "size_t tsqr_mi_working_r_size_f64_qrcp(size_t m, size_t n, int jobq);" in flat
    assert ("int tsqr_mi_qrcp_f64(int a_layout, int q_layout, int jobq, int reorth, double* q, size_t ldq, double* r, size_t ldr, int* jpvt, "
            "double* a, size_t lda, size_t m, size_t n, void* wq, void* wr, void* stream);") in flat
    assert bq.qrcp_f64 and bq.buffer_f64_qrcp and bq.qrcp_f64_tensor and issubclass(bq.QrcpError, RuntimeError)
    import tsqr_gpu_amd
    assert tsqr_gpu_amd.qrcp_f64 is bq.qrcp_f64 and tsqr_gpu_amd.qrcp_f64_tensor is bq.qrcp_f64_tensor
    assert tsqr_gpu_amd.buffer_f64_qrcp is bq.buffer_f64_qrcp and tsqr_gpu_amd.QrcpError is bq.QrcpError
    T = ctypes.CDLL(os.path.join(ROOT, "tsqr_gpu_amd", "csrc", "libtsqr_selftest.so"))
    assert hasattr(T, "tsqr_selftest_f64_qrcp_r")


def test_qrcp_working_sizes(bq):
    L = bq.lib()
    ms = (1, 15, 64, 65, 1000, 4099, 9211, 1 << 16, 1 << 20, (1 << 20) + 1, 1 << 23)
    for n in (1, 7, 16, 17, 33, 51, 64):
        for m in ms:
            assert L.tsqr_mi_working_q_size_f64_qrcp(m, n, 0) == L.tsqr_mi_working_q_size_f64_r(m, n), (m, n)
            assert L.tsqr_mi_working_r_size_f64_qrcp(m, n, 0) == L.tsqr_mi_working_r_size_f64_r(m, n), (m, n)
            assert L.tsqr_mi_working_q_size_f64_qrcp(m, n, 1) == L.tsqr_mi_working_q_size_f64(m, n) + QRCP_BLOCK, (m, n)
            assert L.tsqr_mi_working_r_size_f64_qrcp(m, n, 1) == L.tsqr_mi_working_r_size_f64(m, n), (m, n)
    for m, n in ((0, 4), (4, 0), (0, 0)):
        for jobq in (0, 1):
            assert L.tsqr_mi_working_q_size_f64_qrcp(m, n, jobq) == 0 and L.tsqr_mi_working_r_size_f64_qrcp(m, n, jobq) == 0


def test_qrcp_invalid_arguments_without_gpu(bq):
    # every check comes before any HIP call: null pointers are safe
    L = bq.lib()
    z, some = ctypes.c_void_p(0), ctypes.c_void_p(64)
    INVALID, UNSUPPORTED = bq.error_invalid_matrix_size, bq.error_unsupported_mode

    def call(a_lay=COL, q_lay=COL, jobq=1, ldq=100, ldr=8, lda=100, m=100, n=8, q=z, a=z):
        return L.tsqr_mi_qrcp_f64(a_lay, q_lay, jobq, 0, q, ldq, z, ldr, z, a, lda, m, n, z, z, z)

    for jobq in (0, 1):
        for (m, n) in [(4, 8), (0, 0), (0, 4), (4, 0)]:
            assert call(jobq=jobq, m=m, n=n, ldq=max(m, 1), lda=max(m, 1), ldr=max(n, 1)) == INVALID, (jobq, m, n)
        assert call(jobq=jobq, lda=99) == INVALID                                  # lda < m
        assert call(jobq=jobq, a_lay=ROW, q_lay=ROW, lda=7, ldq=8) == INVALID      # row-major: lda < n
        assert call(jobq=jobq, ldr=7) == INVALID                                   # ldr < n
        assert call(jobq=jobq, a_lay=2) == INVALID and call(jobq=jobq, a_lay=-1) == INVALID
        assert call(jobq=jobq, m=100, n=65, ldr=65) == UNSUPPORTED
        assert "tsqr_mi_qrcp_f64" in bq.last_error() and "n <= 64" in bq.last_error()
    assert call(jobq=1, ldq=99) == INVALID                                         # ldq < m
    assert call(jobq=1, a_lay=ROW, q_lay=ROW, lda=8, ldq=7) == INVALID
    assert call(jobq=1, q_lay=2) == INVALID
    for jobq in (2, -1):
        assert call(jobq=jobq) == INVALID
    assert call(jobq=1, q=some, a=some, a_lay=ROW, q_lay=COL, lda=8, ldq=100) == INVALID     # q == a with two layouts
    assert call(jobq=1, q=some, a=some, lda=100, ldq=101) == INVALID                         # q == a with two strides
    assert L.tsqr_mi_last_sweeps_f64() == 0


def test_qrcp_f64_operand_checks(bq):
    import torch
    m, n = 100, 8
    bf = bq.buffer_f64_qrcp(False)      # (not allocated: every check below raises before the buffer is looked at)
    a64, q64 = torch.zeros(m * n, dtype=torch.float64), torch.zeros(m * n, dtype=torch.float64)
    r64, p32 = torch.zeros(n * n, dtype=torch.float64), torch.zeros(n, dtype=torch.int32)
    with pytest.raises(TypeError):
        bq.qrcp_f64(q64.float(), m, r64, n, p32, a64, m, m, n, bf)
    with pytest.raises(TypeError):
        bq.qrcp_f64(q64, m, r64.float(), n, p32, a64, m, m, n, bf)
    with pytest.raises(TypeError):
        bq.qrcp_f64(q64, m, r64, n, p32.long(), a64, m, m, n, bf)             # jpvt must be int32
    with pytest.raises(TypeError):
        bq.qrcp_f64(q64, m, r64, n, p32.numpy(), a64, m, m, n, bf)
    with pytest.raises(TypeError):
        bq.qrcp_f64(q64, m, r64, n, p32, a64, m, m, n, bf)                    # CPU tensors of the right type
    with pytest.raises(TypeError):
        bq.qrcp_f64_tensor(torch.zeros(m, n, dtype=torch.float64))
    with pytest.raises(TypeError):
        bq.qrcp_f64_tensor(torch.zeros(m, n))
    if torch.cuda.is_available():                                              # (the GPU box: the checks on device tensors)
        a, q = (torch.zeros(m * n, dtype=torch.float64, device="cuda") for _ in range(2))
        r, p = torch.zeros(n * n, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
        with pytest.raises(ValueError):
            bq.qrcp_f64(q[:-1], m, r, n, p, a, m, m, n, bf)
        with pytest.raises(ValueError):
            bq.qrcp_f64(q, m, r[:-1], n, p, a, m, m, n, bf)
        with pytest.raises(ValueError):
            bq.qrcp_f64(q, m, r, n - 1, p, a, m, m, n, bf)
        with pytest.raises(ValueError):
            bq.qrcp_f64(q, m, r, n, p[:-1], a, m, m, n, bf)
        with pytest.raises(ValueError):
            bq.qrcp_f64(q, m, a[:n * n], n, p, a, m, m, n, bf)                 # r overlaps a
        with pytest.raises(RuntimeError):
            bq.qrcp_f64(q, m, r, n, p, a, m, m, n, bf)                         # everything in order but the buffer
        assert bq.qrcp_f64(q, m, r, n, p, a, m, 4, 8, bf) == bq.error_invalid_matrix_size
        with pytest.raises(ValueError):
            bq.qrcp_f64_tensor(a)                                              # one-dimensional
        with pytest.raises(bq.QrcpError) as e:
            bq.qrcp_f64_tensor(a.view(n, m))                                   # n > m
        assert e.value.state == bq.error_invalid_matrix_size


def test_qrcp_f64_operand_checks_cpu_sizes(bq):
    # the size and overlap rules on plain numbers (the helper qrcp_f64 runs on the tensors' addresses)
    chk = bq.check_f64_qrcp_operands
    m, n = 100, 8
    ok = dict(q=(10 ** 6, m * n), r=(10 ** 5, n * n), jpvt=(2 * 10 ** 5, n), a=(10 ** 7, m * n))
    chk(m, n, m, n, m, **ok)
    chk(m, n, n + 2, n, n + 1, row_major=True, q=(10 ** 6, (m - 1) * (n + 2) + n), r=ok["r"], jpvt=ok["jpvt"], a=(10 ** 7, (m - 1) * (n + 1) + n))
    chk(m, n, m, n, m, q=None, r=ok["r"], jpvt=ok["jpvt"], a=ok["a"])                   # jobq = 0
    chk(m, n, m, n, m, q=ok["a"], r=ok["r"], jpvt=ok["jpvt"], a=ok["a"])                # in place
    for bad in (dict(q=(10 ** 6, m * n - 1)), dict(r=(10 ** 5, n * n - 1)), dict(jpvt=(2 * 10 ** 5, n - 1)), dict(a=(10 ** 7, m * n - 1)),
                dict(r=(10 ** 7 + 8, n * n)), dict(jpvt=(10 ** 6 + 8 * (m * n - 1), n)), dict(jpvt=(10 ** 5 + 8, n)),
                dict(q=(10 ** 7 + 8, m * n))):
        with pytest.raises(ValueError):
            chk(m, n, m, n, m, **dict(ok, **bad))
    with pytest.raises(ValueError):
        chk(m, n, m - 1, n, m, **ok)
    with pytest.raises(ValueError):
        chk(m, n, m, n - 1, m, **ok)
    with pytest.raises(ValueError):
        chk(m, n, m + 1, n, m, q=(10 ** 7, (n - 1) * (m + 1) + m), r=ok["r"], jpvt=ok["jpvt"], a=ok["a"])      # q == a with another stride


def test_cpp_qrcp_fp64_compiles_and_links(bq):
    with compile_and_link(os.path.join(ROOT, "tests", "cpp", "sample_fp64_qrcp.cpp"), "sample_fp64_qrcp") as exe:
        assert os.path.exists(exe)

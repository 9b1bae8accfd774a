"""CPU tests of the fp64 SVD entry (tsqr_mi_svd_f64): exported symbols and their signatures, work-space sizes, the argument checks that
come before any HIP call, the Python operand checks of svd_f64 and svd_f64_tensor, and a C++ caller of mtk::qr::svd_fp64
(tests/cpp/sample_fp64_svd.cpp) that compiles and links."""
import ctypes
import os

import pytest

from abi_util import compile_and_link, header_flat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SVD_SYMBOLS = ("tsqr_mi_svd_f64", "tsqr_mi_working_q_size_f64_svd", "tsqr_mi_working_r_size_f64_svd", "tsqr_mi_last_jacobi_sweeps_f64")
SVD_BLOCK = 4096 + 4096 + 8            # R, W and the status words: what jobu = 1 adds to the QR entry's wq, for every m
COL, ROW = 0, 1


def test_svd_symbols_exported_with_the_stated_signatures(bq):
    L = ctypes.CDLL(bq.LIB_PATH)
    flat = header_flat()
    for sym in SVD_SYMBOLS:
        assert hasattr(L, sym), sym
        assert sym in bq.C_ABI_SYMBOLS, sym
    assert "size_t tsqr_mi_working_q_size_f64_svd(size_t m, size_t n, int jobu);" in flat
    assert "size_t tsqr_mi_working_r_size_f64_svd(size_t m, size_t n, int jobu);" in flat
    assert ("int tsqr_mi_svd_f64(int a_layout, int u_layout, int jobu, int reorth, double* u, size_t ldu, double* s, double* v, size_t ldv, "
            "double* a, size_t lda, size_t m, size_t n, void* wq, void* wr, void* stream);") in flat
    assert "int tsqr_mi_last_jacobi_sweeps_f64(void);" in flat
    assert "#define TSQR_MI_ERROR_NO_CONVERGENCE 4" in flat
    assert bq.error_no_convergence == 4
    assert bq.svd_f64 and bq.buffer_f64_svd and bq.svd_f64_tensor and issubclass(bq.SvdError, RuntimeError)
    import tsqr_gpu_amd
    assert tsqr_gpu_amd.svd_f64 is bq.svd_f64 and tsqr_gpu_amd.svd_f64_tensor is bq.svd_f64_tensor


def test_svd_working_sizes(bq):
    L = bq.lib()
    ms = (1, 15, 64, 65, 1000, 4099, 9211, 1 << 16, 1 << 20, (1 << 20) + 1, 1 << 23)
    for n in (1, 7, 16, 17, 33, 51, 64):
        for m in ms:
            assert L.tsqr_mi_working_q_size_f64_svd(m, n, 0) == L.tsqr_mi_working_q_size_f64_r(m, n), (m, n)
            assert L.tsqr_mi_working_r_size_f64_svd(m, n, 0) == L.tsqr_mi_working_r_size_f64_r(m, n), (m, n)
            assert L.tsqr_mi_working_q_size_f64_svd(m, n, 1) == L.tsqr_mi_working_q_size_f64(m, n) + SVD_BLOCK, (m, n)
            assert L.tsqr_mi_working_r_size_f64_svd(m, n, 1) == L.tsqr_mi_working_r_size_f64(m, n), (m, n)
    for m, n in ((0, 4), (4, 0), (0, 0)):
        for jobu in (0, 1):
            assert L.tsqr_mi_working_q_size_f64_svd(m, n, jobu) == 0 and L.tsqr_mi_working_r_size_f64_svd(m, n, jobu) == 0


def test_svd_invalid_arguments_without_gpu(bq):
    # every check comes before any HIP call: null pointers are safe (v: a pointer that is never followed, so that ldv is looked at)
    L = bq.lib()
    z, some = ctypes.c_void_p(0), ctypes.c_void_p(64)
    INVALID, UNSUPPORTED = bq.error_invalid_matrix_size, bq.error_unsupported_mode

    def call(a_lay=COL, u_lay=COL, jobu=1, ldu=100, v=z, ldv=8, lda=100, m=100, n=8, u=z, a=z):
        return L.tsqr_mi_svd_f64(a_lay, u_lay, jobu, 0, u, ldu, z, v, ldv, a, lda, m, n, z, z, z)

    for jobu in (0, 1):
        for (m, n) in [(4, 8), (0, 0), (0, 4), (4, 0)]:
            assert call(jobu=jobu, m=m, n=n, ldu=max(m, 1), lda=max(m, 1), ldv=max(n, 1)) == INVALID, (jobu, m, n)
        assert call(jobu=jobu, lda=99) == INVALID                                  # lda < m
        assert call(jobu=jobu, a_lay=ROW, u_lay=ROW, lda=7, ldu=8) == INVALID      # row-major: lda < n
        assert call(jobu=jobu, v=some, ldv=7) == INVALID                           # ldv < n
        assert call(jobu=jobu, a_lay=2) == INVALID and call(jobu=jobu, a_lay=-1) == INVALID
        assert call(jobu=jobu, m=100, n=65, ldv=65) == UNSUPPORTED
        assert "tsqr_mi_svd_f64" in bq.last_error() and "n <= 64" in bq.last_error()
    assert call(jobu=1, ldu=99) == INVALID                                         # ldu < m
    assert call(jobu=1, a_lay=ROW, u_lay=ROW, lda=8, ldu=7) == INVALID
    assert call(jobu=1, u_lay=2) == INVALID
    for jobu in (2, -1):
        assert call(jobu=jobu) == INVALID
    assert call(jobu=1, u=some, a=some, a_lay=ROW, u_lay=COL, lda=8, ldu=100) == INVALID     # u == a with two layouts
    assert call(jobu=1, u=some, a=some, lda=100, ldu=101) == INVALID                         # u == a with two strides
    assert L.tsqr_mi_last_sweeps_f64() == 0 and L.tsqr_mi_last_jacobi_sweeps_f64() == 0


def test_svd_f64_operand_checks(bq):
    import torch
    m, n = 100, 8
    bf = bq.buffer_f64_svd(False)       # (not allocated: every check below raises before the buffer is looked at)
    a64, u64 = torch.zeros(m * n, dtype=torch.float64), torch.zeros(m * n, dtype=torch.float64)
    s64, v64 = torch.zeros(n, dtype=torch.float64), torch.zeros(n * n, dtype=torch.float64)
    with pytest.raises(TypeError):
        bq.svd_f64(u64.float(), m, s64, v64, n, a64, m, m, n, bf)
    with pytest.raises(TypeError):
        bq.svd_f64(u64, m, s64.float(), v64, n, a64, m, m, n, bf)
    with pytest.raises(TypeError):
        bq.svd_f64(u64, m, s64, v64.numpy(), n, a64, m, m, n, bf)
    with pytest.raises(TypeError):
        bq.svd_f64(u64, m, s64, v64, n, a64, m, m, n, bf)                     # CPU tensors of the right type
    with pytest.raises(TypeError):
        bq.svd_f64_tensor(torch.zeros(m, n, dtype=torch.float64))
    with pytest.raises(TypeError):
        bq.svd_f64_tensor(torch.zeros(m, n))
    if torch.cuda.is_available():                                              # (the GPU box: the checks on device tensors)
        a, u = (torch.zeros(m * n, dtype=torch.float64, device="cuda") for _ in range(2))
        s, v = torch.zeros(n, dtype=torch.float64, device="cuda"), torch.zeros(n * n, dtype=torch.float64, device="cuda")
        with pytest.raises(ValueError):
            bq.svd_f64(u[:-1], m, s, v, n, a, m, m, n, bf)
        with pytest.raises(ValueError):
            bq.svd_f64(u, m, s[:-1], v, n, a, m, m, n, bf)
        with pytest.raises(ValueError):
            bq.svd_f64(u, m, s, v, n - 1, a, m, m, n, bf)
        with pytest.raises(ValueError):
            bq.svd_f64(u, m, s, a[:n * n], n, a, m, m, n, bf)                  # v overlaps a
        with pytest.raises(RuntimeError):
            bq.svd_f64(u, m, s, v, n, a, m, m, n, bf)                          # everything in order but the buffer
        assert bq.svd_f64(u, m, s, v, n, a, m, 4, 8, bf) == bq.error_invalid_matrix_size
        with pytest.raises(ValueError):
            bq.svd_f64_tensor(a)                                               # one-dimensional
        with pytest.raises(bq.SvdError) as e:
            bq.svd_f64_tensor(a.view(n, m))                                    # n > m
        assert e.value.state == bq.error_invalid_matrix_size


def test_svd_f64_operand_checks_cpu_sizes(bq):
    # the size and overlap rules on plain numbers (the helper svd_f64 runs on the tensors' addresses)
    chk = bq.check_f64_svd_operands
    m, n = 100, 8
    ok = dict(u=(10 ** 6, m * n), s=(10 ** 5, n), v=(2 * 10 ** 5, n * n), a=(10 ** 7, m * n))
    chk(m, n, m, n, m, **ok)
    chk(m, n, n + 2, n, n + 1, row_major=True, u=(10 ** 6, (m - 1) * (n + 2) + n), s=ok["s"], v=ok["v"], a=(10 ** 7, (m - 1) * (n + 1) + n))
    chk(m, n, m, n, m, u=None, s=ok["s"], v=None, a=ok["a"])                            # jobu = 0 without V
    chk(m, n, m, n, m, u=ok["a"], s=ok["s"], v=ok["v"], a=ok["a"])                      # in place
    for bad in (dict(u=(10 ** 6, m * n - 1)), dict(s=(10 ** 5, n - 1)), dict(v=(2 * 10 ** 5, n * n - 1)), dict(a=(10 ** 7, m * n - 1)),
                dict(s=(10 ** 7 + 8, n)), dict(v=(10 ** 6 + 8 * (m * n - 1), n * n)), dict(s=(2 * 10 ** 5 + 8, n)),
                dict(u=(10 ** 7 + 8, m * n))):
        with pytest.raises(ValueError):
            chk(m, n, m, n, m, **dict(ok, **bad))
    with pytest.raises(ValueError):
        chk(m, n, m - 1, n, m, **ok)
    with pytest.raises(ValueError):
        chk(m, n, m, n - 1, m, **ok)
    with pytest.raises(ValueError):
        chk(m, n, m + 1, n, m, u=(10 ** 7, (n - 1) * (m + 1) + m), s=ok["s"], v=ok["v"], a=ok["a"])      # u == a with another stride


def test_cpp_svd_fp64_compiles_and_links(bq):
    with compile_and_link(os.path.join(ROOT, "tests", "cpp", "sample_fp64_svd.cpp"), "sample_fp64_svd") as exe:
        assert os.path.exists(exe)

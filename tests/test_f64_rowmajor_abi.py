"""CPU tests of the layout entries (tsqr_mi_r_f64_lay, tsqr_mi_lstsq_f64_lay): the symbols and constants, the argument checks that come
before any HIP call, the layout lstsq_f64 chooses for an operand (strides only: CPU tensors), the row-major span and overlap rules of
check_f64_r_operands, and a C++ caller of the layout arguments of mtk::qr::r_fp64 / lstsq_fp64 (tests/cpp/sample_fp64_rowmajor.cpp)."""
import ctypes
import os
import subprocess

import pytest

from abi_util import compile_and_link, header_flat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COL, ROW = 0, 1


def test_layout_symbols_and_constants(bq):
    L = ctypes.CDLL(bq.LIB_PATH)
    flat = header_flat()
    for sym in ("tsqr_mi_r_f64_lay", "tsqr_mi_lstsq_f64_lay"):
        assert hasattr(L, sym), sym
        assert sym in bq.C_ABI_SYMBOLS, sym
    assert "#define TSQR_MI_COL_MAJOR 0" in flat and "#define TSQR_MI_ROW_MAJOR 1" in flat
    assert (bq.COL_MAJOR, bq.ROW_MAJOR) == (0, 1)
    assert ("int tsqr_mi_r_f64_lay(int a_layout, int reorth, double* r, size_t ldr, const double* a, size_t lda, size_t m, size_t n, "
            "void* wq, void* wr, void* stream);") in flat
    assert ("int tsqr_mi_lstsq_f64_lay(int a_layout, int b_layout, int reorth, int refine, double* x, size_t ldx, double* r, size_t ldr, "
            "const double* a, size_t lda, const double* b, size_t ldb, size_t m, size_t n, size_t nrhs, void* wq, void* wr, void* stream);") in flat
    sel = ctypes.CDLL(os.path.join(ROOT, "tsqr_gpu_amd", "csrc", "libtsqr_selftest.so"))
    for hook in ("tsqr_selftest_f64_gram_lay", "tsqr_selftest_f64_gramq_lay", "tsqr_selftest_f64_lsq_lay"):
        assert hasattr(sel, hook), hook


def test_layout_argument_checks_without_gpu(bq):
    # every check comes before any HIP call: null pointers are safe
    L = bq.lib()
    z = ctypes.c_void_p(0)
    bad, unsupported = bq.error_invalid_matrix_size, bq.error_unsupported_mode
    m, n, nrhs = 100, 8, 3

    def r(lay, lda, m=m, n=n, ldr=None):
        return L.tsqr_mi_r_f64_lay(lay, 0, z, n if ldr is None else ldr, z, lda, m, n, z, z, z)

    def ls(al, bl, lda, ldb, m=m, n=n, nrhs=nrhs, refine=1):
        return L.tsqr_mi_lstsq_f64_lay(al, bl, 0, refine, z, n, z, n, z, lda, z, ldb, m, n, nrhs, z, z, z)

    for lay in (2, -1, 7):
        assert r(lay, m) == bad
        assert ls(lay, COL, m, m) == bad and ls(COL, lay, m, m) == bad and ls(ROW, lay, n, nrhs) == bad
    assert r(2, m, n=65) == bad                               # a layout error comes before "unsupported"
    # row-major: lda >= n is asked, not lda >= m.  A call whose sizes pass goes on to the GPU, which these tests must not touch; that
    # lda = n < m PASSES the size check shows on n = 65 and nrhs = 17: state 2 is only reached behind it
    assert r(ROW, n - 1) == bad
    assert r(ROW, 64, n=65) == bad and r(ROW, 65, n=65) == unsupported and r(COL, 65, n=65) == bad
    assert "n <= 64" in bq.last_error()
    assert r(ROW, n, ldr=n - 1) == bad
    assert ls(ROW, ROW, n - 1, nrhs) == bad and ls(ROW, ROW, n, nrhs - 1) == bad
    assert ls(ROW, COL, n, m - 1) == bad and ls(COL, ROW, m - 1, nrhs) == bad
    assert ls(ROW, ROW, 65, nrhs, n=65) == unsupported        # lda = n = 65 < m = 100 passed the size check
    assert ls(ROW, ROW, n, 17, nrhs=17) == unsupported        # ldb = nrhs = 17 < m likewise
    assert "nrhs <= 16" in bq.last_error()
    assert ls(ROW, ROW, n, 16, nrhs=17) == bad
    assert ls(ROW, ROW, n, nrhs, refine=5) == unsupported
    assert ls(COL, COL, m - 1, m) == bad and ls(COL, COL, n, nrhs) == bad          # column-major: the old rule, lda >= m
    assert ls(COL, COL, m, m, n=65) == unsupported
    for (mm, nn, kk) in [(4, 8, 1), (0, 4, 1), (4, 0, 1), (8, 4, 0)]:
        assert ls(ROW, ROW, max(nn, 1), max(kk, 1), m=mm, n=nn, nrhs=kk) == bad
    assert L.tsqr_mi_last_sweeps_f64() == 0


def test_wrapper_layout_choice_on_strides():
    import torch
    from tsqr_gpu_amd import blockqr as bq
    m, n = 7, 4
    cont = torch.arange(float(m * n), dtype=torch.float64).reshape(m, n)
    t, ld, lay = bq._operand_f64(cont)                          # contiguous: rows contiguous, read where it lies
    assert (t.data_ptr(), ld, lay) == (cont.data_ptr(), n, ROW)
    tr = torch.arange(float(m * n), dtype=torch.float64).reshape(n, m).t()        # m x n, columns contiguous
    t, ld, lay = bq._operand_f64(tr)
    assert (t.data_ptr(), ld, lay) == (tr.data_ptr(), m, COL)
    padded = torch.zeros(m, n + 3, dtype=torch.float64)[:, :n]                     # rows padded: stride(0) = n + 3
    t, ld, lay = bq._operand_f64(padded)
    assert (t.data_ptr(), ld, lay) == (padded.data_ptr(), n + 3, ROW)
    colpad = torch.zeros(n, m + 5, dtype=torch.float64)[:, :m].t()                 # columns padded: stride(1) = m + 5
    t, ld, lay = bq._operand_f64(colpad)
    assert (t.data_ptr(), ld, lay) == (colpad.data_ptr(), m + 5, COL)
    one = torch.zeros(m, 1, dtype=torch.float64)                                   # one contiguous column
    t, ld, lay = bq._operand_f64(one)
    assert t.data_ptr() == one.data_ptr() and (ld, lay) in ((m, COL), (1, ROW))
    strided_col = cont[:, 2:3]                                                     # one column of a row-major matrix: stride(0) = n
    t, ld, lay = bq._operand_f64(strided_col)
    assert (t.data_ptr(), ld, lay) == (strided_col.data_ptr(), n, ROW)
    vec = cont[:, 1].unsqueeze(1)                                                  # what lstsq_f64 makes of a one-dimensional b
    t, ld, lay = bq._operand_f64(vec)
    assert (t.data_ptr(), ld, lay) == (vec.data_ptr(), n, ROW)
    every_other = torch.zeros(m, 2 * n, dtype=torch.float64)[:, ::2]               # neither: copied once, column-major
    t, ld, lay = bq._operand_f64(every_other)
    assert t.data_ptr() != every_other.data_ptr() and (ld, lay) == (m, COL) and t.stride() == (1, m) and torch.equal(t, every_other)
    expanded = torch.zeros(1, n, dtype=torch.float64).expand(m, n)                 # stride(0) = 0 < n: rows overlap, copied
    t, ld, lay = bq._operand_f64(expanded)
    assert t.data_ptr() != expanded.data_ptr() and (ld, lay) == (m, COL)


def test_check_f64_r_operands_row_major_span():
    from tsqr_gpu_amd import blockqr as bq
    m, n = 100, 8
    base = 1 << 20
    r = (base + (1 << 16), n * n)
    chk = lambda lda, numel, r=r, ldr=n: bq.check_f64_r_operands(m, n, ldr, lda, r, (base, numel), row_major=True)
    chk(n, m * n)                                              # contiguous
    chk(n + 3, (m - 1) * (n + 3) + n)                          # exactly the span (m - 1) lda + n
    with pytest.raises(ValueError):
        chk(n + 3, (m - 1) * (n + 3) + n - 1)                  # one element short
    with pytest.raises(ValueError):
        chk(n - 1, m * n)                                      # lda < n
    with pytest.raises(ValueError):
        bq.check_f64_r_operands(m, n, n, n, r, (base, m * n))  # the same operand as column-major: lda < m
    with pytest.raises(ValueError):
        chk(n, m * n, ldr=n - 1)
    span = 8 * ((m - 1) * (n + 3) + n)
    chk(n + 3, m * (n + 3), r=(base + span, n * n))            # r begins where the span of a ends: apart
    with pytest.raises(ValueError):
        chk(n + 3, m * (n + 3), r=(base + span - 8, n * n))    # one double inside it
    with pytest.raises(ValueError):
        chk(n + 3, m * (n + 3), r=(base - 8 * n * n + 8, n * n))


def test_r_f64_row_major_keyword_is_checked_on_the_cpu(bq):
    import torch
    a = torch.zeros(100, 8, dtype=torch.float64)
    r = torch.zeros(8, 8, dtype=torch.float64)
    bf = bq.buffer_f64_r(False)
    with pytest.raises(TypeError):
        bq.r_f64(r, 8, a, 8, 100, 8, bf, row_major=True)       # CPU tensors
    import inspect
    sig = inspect.signature(bq.r_f64)
    assert sig.parameters["row_major"].default is False


def test_cpp_layout_sample_compiles_links_and_runs(bq):
    src = os.path.join(ROOT, "tests", "cpp", "sample_fp64_rowmajor.cpp")
    with compile_and_link(src, "sample_fp64_rowmajor") as exe:
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "argument checks ok" in out.stdout

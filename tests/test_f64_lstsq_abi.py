"""CPU tests of the fp64 least-squares entry (tsqr_mi_lstsq_f64): exported symbols and their signatures, work-space sizes, argument
checks that come before any HIP call, the Python operand checks of lstsq_f64, and a C++ caller of mtk::qr::lstsq_fp64 that compiles and
links (with hipcc, the way tests/test_f64_r_abi.py builds its sample)."""
import ctypes
import os

import pytest

from abi_util import compile_and_link, header_flat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ("tsqr_mi_lstsq_f64", "tsqr_mi_working_q_size_f64_lstsq", "tsqr_mi_working_r_size_f64_lstsq")


def test_lstsq_symbols_exported_with_the_stated_signatures(bq):
    L = ctypes.CDLL(bq.LIB_PATH)
    flat = header_flat()
    for sym in SYMBOLS:
        assert hasattr(L, sym), sym
        assert sym in bq.C_ABI_SYMBOLS, sym
    assert "size_t tsqr_mi_working_q_size_f64_lstsq(size_t m, size_t n, size_t nrhs);" in flat
    assert "size_t tsqr_mi_working_r_size_f64_lstsq(size_t m, size_t n, size_t nrhs);" in flat
    assert ("int tsqr_mi_lstsq_f64(int reorth, int refine, double* x, size_t ldx, double* r, size_t ldr, const double* a, size_t lda, "
            "const double* b, size_t ldb, size_t m, size_t n, size_t nrhs, void* wq, void* wr, void* stream);") in flat
    import tsqr_gpu_amd
    assert tsqr_gpu_amd.lstsq_f64 is bq.lstsq_f64
    sel = ctypes.CDLL(os.path.join(ROOT, "tsqr_gpu_amd", "csrc", "libtsqr_selftest.so"))
    assert hasattr(sel, "tsqr_selftest_f64_lsq") and hasattr(sel, "tsqr_selftest_f64_lsq_update")


def test_lstsq_working_sizes(bq):
    L = bq.lib()
    ms = (1, 15, 16, 17, 33, 1000, 4099, 9211, 1 << 16, 1 << 20, (1 << 20) + 1, 1 << 23)
    for n in (1, 7, 16, 17, 33, 51, 64):
        wqs = set()
        for m in ms:
            for nrhs in (1, 5, 16):
                wq, wr = L.tsqr_mi_working_q_size_f64_lstsq(m, n, nrhs), L.tsqr_mi_working_r_size_f64_lstsq(m, n, nrhs)
                wqs.add(wq)
                # the R-only entry's layout, X (64 x 16) and the summed D (4 tiles of 256 and the reduction's row count)
                assert wq >= L.tsqr_mi_working_q_size_f64_r(m, n) + 1024 + 1024 + 1, (m, n, nrhs, wq)
                assert wr >= L.tsqr_mi_working_r_size_f64_r(m, n), (m, n, nrhs, wr)
                # the passes run on the R-only entry's second plan: one partial of NT tiles per workgroup of four waves
                nt = (n + 15) // 16
                tiles = (m + 15) // 16
                tpw = max(1, (tiles + 2047) // 2048)
                nwaves = (tiles + tpw - 1) // tpw
                assert wr >= ((nwaves + 3) // 4) * nt * 256, (m, n, nrhs, wr)
                assert wr <= 512 * 10 * 256, (m, n, nrhs, wr)
        assert len(wqs) == 1, "wq depends on m or nrhs"
    for m, n, nrhs in ((0, 4, 1), (4, 0, 1), (4, 4, 0), (0, 0, 0)):
        assert L.tsqr_mi_working_q_size_f64_lstsq(m, n, nrhs) == 0 and L.tsqr_mi_working_r_size_f64_lstsq(m, n, nrhs) == 0


def test_lstsq_invalid_sizes_without_gpu(bq):
    # every check comes before any HIP call: null pointers are safe
    L = bq.lib()
    z = ctypes.c_void_p(0)

    def call(m, n, nrhs, ldx=None, ldr=None, lda=None, ldb=None, refine=1, reorth=0):
        return L.tsqr_mi_lstsq_f64(reorth, refine, z, max(n, 1) if ldx is None else ldx, z, max(n, 1) if ldr is None else ldr,
                                   z, max(m, 1) if lda is None else lda, z, max(m, 1) if ldb is None else ldb, m, n, nrhs, z, z, z)

    for (m, n, nrhs) in [(4, 8, 1), (0, 0, 1), (0, 4, 1), (4, 0, 1), (8, 4, 0)]:
        assert call(m, n, nrhs) == bq.error_invalid_matrix_size, (m, n, nrhs)
    assert call(100, 8, 3, ldx=7) == bq.error_invalid_matrix_size
    assert call(100, 8, 3, ldr=7) == bq.error_invalid_matrix_size
    assert call(100, 8, 3, lda=99) == bq.error_invalid_matrix_size
    assert call(100, 8, 3, ldb=99) == bq.error_invalid_matrix_size
    assert call(100, 65, 3, reorth=1) == bq.error_unsupported_mode
    assert "tsqr_mi_lstsq_f64" in bq.last_error() and "n <= 64" in bq.last_error()
    assert call(100, 8, 17) == bq.error_unsupported_mode
    assert "nrhs <= 16" in bq.last_error()
    assert call(100, 8, 3, refine=5) == bq.error_unsupported_mode
    assert "refine <= 4" in bq.last_error()
    assert call(100, 8, 3, refine=-1) == bq.error_unsupported_mode
    assert call(100, 65, 3, lda=99) == bq.error_invalid_matrix_size        # a size error comes first
    assert L.tsqr_mi_last_sweeps_f64() == 0


def test_lstsq_f64_operand_checks(bq):
    import torch
    a = torch.zeros(100, 8, dtype=torch.float64)
    b = torch.zeros(100, 3, dtype=torch.float64)
    with pytest.raises(TypeError):
        bq.lstsq_f64(a.float(), b)
    with pytest.raises(TypeError):
        bq.lstsq_f64(a, b.float())
    with pytest.raises(TypeError):
        bq.lstsq_f64(a.numpy(), b)
    with pytest.raises(TypeError):
        bq.lstsq_f64(a, b)                                     # CPU tensors of the right type
    if torch.cuda.is_available():                              # (the GPU box: shapes and states on device tensors; nothing is launched)
        a, b = a.cuda(), b.cuda()
        with pytest.raises(ValueError):
            bq.lstsq_f64(a, b[:99])
        with pytest.raises(ValueError):
            bq.lstsq_f64(a.reshape(-1), b)
        for bad, state in (((a[:4], b[:4]), bq.error_invalid_matrix_size),                          # 4 x 8: n > m
                           ((torch.zeros(100, 65, dtype=torch.float64, device="cuda"), b), bq.error_unsupported_mode),
                           ((a, torch.zeros(100, 17, dtype=torch.float64, device="cuda")), bq.error_unsupported_mode)):
            with pytest.raises(bq.LstsqError) as e:
                bq.lstsq_f64(*bad)
            assert e.value.state == state
        with pytest.raises(bq.LstsqError) as e:
            bq.lstsq_f64(a, b, refine=5)
        assert e.value.state == bq.error_unsupported_mode


def test_colmajor_helper_keeps_or_copies():
    import torch
    from tsqr_gpu_amd import blockqr as bq
    rowmajor = torch.arange(12.0, dtype=torch.float64).reshape(4, 3)
    c, ld = bq._colmajor_f64(rowmajor)
    assert ld == 4 and c.stride() == (1, 4) and torch.equal(c, rowmajor) and c.data_ptr() != rowmajor.data_ptr()
    colmajor = torch.arange(15.0, dtype=torch.float64).reshape(3, 5).t()[:4]     # 4 x 3, column stride 5
    c, ld = bq._colmajor_f64(colmajor)
    assert ld == 5 and c.data_ptr() == colmajor.data_ptr()
    one = torch.zeros(7, 1, dtype=torch.float64)
    c, ld = bq._colmajor_f64(one)
    assert ld == 7 and c.data_ptr() == one.data_ptr()


CPP_SAMPLE = r"""
#include <tsqr/blockqr.hpp>
#include <cstdio>
int main() {
	const std::size_t m = 1000, n = 24, nrhs = 3;
	mtk::qr::buffer_fp64_lstsq<false> bf;
	double *a = nullptr, *b = nullptr, *x = nullptr, *r = nullptr;
	if (hipMalloc(&a, sizeof(double) * m * n) != hipSuccess) return 0;   // (no GPU: compiled and linked is what the CPU test checks)
	(void)hipMalloc(&b, sizeof(double) * m * nrhs);
	(void)hipMalloc(&x, sizeof(double) * n * nrhs);
	(void)hipMalloc(&r, sizeof(double) * n * n);
	bf.allocate(m, n, nrhs);
	const double *ca = a, *cb = b;
	const mtk::qr::state_t st = mtk::qr::lstsq_fp64<false>(x, n, r, n, ca, m, cb, m, m, n, nrhs, bf);
	const mtk::qr::state_t st2 = mtk::qr::lstsq_fp64<false>(x, n, r, n, ca, m, cb, m, m, n, nrhs, bf, 2);
	std::printf("states %d %d, sweeps %d, %zu bytes of work space\n", st, st2, tsqr_mi_last_sweeps_f64(), bf.get_device_memory_size());
	bf.destroy();
	(void)hipFree(a); (void)hipFree(b); (void)hipFree(x); (void)hipFree(r);
	return 0;
}
"""


def test_cpp_lstsq_fp64_compiles_and_links(bq):
    with compile_and_link(CPP_SAMPLE, "sample_fp64_lstsq") as exe:
        assert os.path.exists(exe)

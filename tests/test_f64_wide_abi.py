"""CPU tests of the wide fp64 entry (tsqr_mi_qr_f64_wide, 1 <= n <= 1024): exported and declared symbols, work-space sizes (the cap of
the Gram partials included), argument checks that come before any HIP call, the Python operand checks of qr_f64_wide, and a C++ caller
of mtk::qr::qr_fp64_wide that compiles and links."""
import ctypes
import os

import pytest

from abi_util import compile_and_link

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WIDE_SYMBOLS = ("tsqr_mi_qr_f64_wide", "tsqr_mi_working_q_size_f64_wide", "tsqr_mi_working_r_size_f64_wide")
WR_CAP = 8 << 20


def test_f64_wide_symbols_exported(bq):
    L = ctypes.CDLL(bq.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "tsqr_mi.h")).read()
    for sym in WIDE_SYMBOLS:
        assert hasattr(L, sym), sym
        assert sym + "(" in hdr, sym
        assert sym in bq.C_ABI_SYMBOLS, sym
    hpp = open(os.path.join(ROOT, "include", "tsqr", "blockqr.hpp")).read()
    assert "struct buffer_fp64_wide" in hpp and "qr_fp64_wide(" in hpp
    assert callable(bq.qr_f64_wide) and issubclass(bq.buffer_f64_wide, bq.buffer_f64)


def test_f64_wide_working_sizes(bq):
    L = bq.lib()
    for m in (1, 33, 9211, 1 << 20, 1 << 23):
        for n in (1, 7, 51, 64):                              # one panel: the sizes of tsqr_mi_qr_f64
            if n > m:
                continue
            assert L.tsqr_mi_working_q_size_f64_wide(m, n) == L.tsqr_mi_working_q_size_f64(m, n)
            assert L.tsqr_mi_working_r_size_f64_wide(m, n) == L.tsqr_mi_working_r_size_f64(m, n)
    for m in (65, 200, 1100, 9211, 1 << 16, 1 << 18, 1 << 20, 1 << 23):
        for n in (65, 100, 128, 256, 640, 1000, 1024):
            if n > m:
                continue
            nb = (n + 63) // 64
            blocks = nb * (nb + 1) // 2 * 4096
            wq = L.tsqr_mi_working_q_size_f64_wide(m, n)
            wr = L.tsqr_mi_working_r_size_f64_wide(m, n)
            # wq: six block stores (G, G', R, Z, T, copy of R) and the small words; independent of m
            assert wq >= 6 * blocks, (m, n, wq)
            assert wq <= 6 * blocks + 80 * 1024, (m, n, wq)
            assert wq == L.tsqr_mi_working_q_size_f64_wide(n, n)
            # wr: whole sets of partials (one per row slice), capped
            assert wr >= blocks and wr % blocks == 0, (m, n, wr)
            assert wr <= WR_CAP, (m, n, wr)
    assert L.tsqr_mi_working_r_size_f64_wide(1 << 23, 1024) <= WR_CAP
    assert L.tsqr_mi_working_r_size_f64_wide(1 << 40, 1024) <= WR_CAP
    assert L.tsqr_mi_working_q_size_f64_wide(0, 100) == 0 and L.tsqr_mi_working_r_size_f64_wide(100, 0) == 0


def test_f64_wide_invalid_sizes_without_gpu(bq):
    # every check comes before any HIP call: null pointers are safe
    L = bq.lib()
    z = ctypes.c_void_p(0)
    for (m, n) in [(4, 8), (0, 0), (0, 4), (4, 0), (100, 101), (1000, 1025)]:
        assert L.tsqr_mi_qr_f64_wide(0, z, max(m, 1), z, max(n, 1), z, max(m, 1), m, n, z, z, z) == bq.error_invalid_matrix_size
    assert L.tsqr_mi_qr_f64_wide(1, z, 2000, z, 1025, z, 2000, 2000, 1025, z, z, z) == bq.error_unsupported_mode
    assert "n <= 1024" in bq.last_error()
    # leading dimensions below the rows of their operand
    assert L.tsqr_mi_qr_f64_wide(0, z, 299, z, 200, z, 300, 300, 200, z, z, z) == bq.error_invalid_matrix_size
    assert L.tsqr_mi_qr_f64_wide(0, z, 300, z, 199, z, 300, 300, 200, z, z, z) == bq.error_invalid_matrix_size
    assert L.tsqr_mi_qr_f64_wide(0, z, 300, z, 200, z, 299, 300, 200, z, z, z) == bq.error_invalid_matrix_size
    assert L.tsqr_mi_last_sweeps_f64() == 0
    # the n <= 64 entry keeps its answer, and points at the wide one
    assert L.tsqr_mi_qr_f64(1, z, 100, z, 65, z, 100, 100, 65, z, z, z) == bq.error_unsupported_mode
    assert "n <= 64" in bq.last_error()


def test_qr_f64_wide_operand_checks(bq):
    import torch
    m, n = 300, 100
    bf = bq.buffer_f64_wide(False)     # (not allocated: every check below raises before the buffer is looked at)
    a64 = torch.zeros(m * n, dtype=torch.float64)
    r64 = torch.zeros(n * n, dtype=torch.float64)
    with pytest.raises(TypeError):
        bq.qr_f64_wide(a64.float(), m, r64, n, a64, m, m, n, bf)
    with pytest.raises(TypeError):
        bq.qr_f64_wide(a64, m, r64.float(), n, a64, m, m, n, bf)
    with pytest.raises(TypeError):
        bq.qr_f64_wide(a64, m, r64, n, a64.clone(), m, m, n, bf)
    with pytest.raises(TypeError):
        bq.qr_f64_wide(a64, m, r64, n, [0.0] * (m * n), m, m, n, bf)
    if torch.cuda.is_available():                              # (the GPU box: the size and overlap checks on device tensors)
        dev = "cuda"
        a = torch.zeros(m * n, dtype=torch.float64, device=dev)
        q = torch.zeros(m * n, dtype=torch.float64, device=dev)
        r = torch.zeros(n * n, dtype=torch.float64, device=dev)
        assert bq.qr_f64_wide(q, m, r, n, a, m, m, 1025, bf) == bq.error_invalid_matrix_size      # n > m
        with pytest.raises(ValueError):
            bq.qr_f64_wide(q[:-1], m, r, n, a, m, m, n, bf)
        with pytest.raises(ValueError):
            bq.qr_f64_wide(q, m, r[:-1], n, a, m, m, n, bf)
        with pytest.raises(ValueError):
            bq.qr_f64_wide(q, m - 1, r, n, a, m, m, n, bf)
        with pytest.raises(ValueError):
            bq.qr_f64_wide(a[1:], m, r, n, a, m, m - 1, n, bf)     # q overlaps a without being a
        with pytest.raises(ValueError):
            bq.qr_f64_wide(q, m, a[:n * n], n, a, m, m, n, bf)     # r overlaps a
        with pytest.raises(RuntimeError):
            bq.qr_f64_wide(q, m, r, n, a, m, m, n, bf)             # not allocated


CPP_SAMPLE = r"""
#include <tsqr/blockqr.hpp>
#include <cstdio>
int main() {
	const std::size_t m = 4000, n = 300;
	mtk::qr::buffer_fp64_wide<false> bf;
	double *a = nullptr, *q = nullptr, *r = nullptr;
	if (hipMalloc(&a, sizeof(double) * m * n) != hipSuccess) return 0;   // (no GPU: compiled and linked is what the CPU test checks)
	(void)hipMalloc(&q, sizeof(double) * m * n);
	(void)hipMalloc(&r, sizeof(double) * n * n);
	bf.allocate(m, n);
	const mtk::qr::state_t st = mtk::qr::qr_fp64_wide<false>(q, m, r, n, a, m, m, n, bf);
	std::printf("state %d, sweeps %d, %zu bytes of work space\n", st, tsqr_mi_last_sweeps_f64(), bf.get_device_memory_size());
	bf.destroy();
	(void)hipFree(a); (void)hipFree(q); (void)hipFree(r);
	return 0;
}
"""


def test_cpp_qr_fp64_wide_compiles_and_links(bq):
    with compile_and_link(CPP_SAMPLE, "sample_fp64_wide") as exe:
        assert os.path.exists(exe)

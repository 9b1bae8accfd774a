"""CPU tests of the R-only fp64 entry (tsqr_mi_r_f64): exported symbols and their signatures, work-space sizes, argument checks that
come before any HIP call, the Python operand checks of r_f64, and a C++ caller of mtk::qr::r_fp64 that compiles and links (with hipcc,
the way tests/test_f64_abi.py builds its sample: the C++ samples of this project are not host-only translation units)."""
import ctypes
import os

import pytest

from abi_util import compile_and_link, header_flat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

R_SYMBOLS = ("tsqr_mi_r_f64", "tsqr_mi_working_q_size_f64_r", "tsqr_mi_working_r_size_f64_r")


def test_r_symbols_exported_with_the_stated_signatures(bq):
    L = ctypes.CDLL(bq.LIB_PATH)
    flat = header_flat()
    for sym in R_SYMBOLS:
        assert hasattr(L, sym), sym
        assert sym in bq.C_ABI_SYMBOLS, sym
    assert "size_t tsqr_mi_working_q_size_f64_r(size_t m, size_t n);" in flat
    assert "size_t tsqr_mi_working_r_size_f64_r(size_t m, size_t n);" in flat
    assert ("int tsqr_mi_r_f64(int reorth, double* r, size_t ldr, const double* a, size_t lda, size_t m, size_t n, "
            "void* wq, void* wr, void* stream);") in flat
    assert bq.r_f64 and bq.buffer_f64_r
    import tsqr_gpu_amd
    assert tsqr_gpu_amd.r_f64 is bq.r_f64 and tsqr_gpu_amd.buffer_f64_r is bq.buffer_f64_r


def test_r_working_sizes(bq):
    L = bq.lib()
    ms = (1, 15, 16, 17, 33, 1000, 4099, 9211, 1 << 16, 1 << 20, (1 << 20) + 1, 1 << 23)
    for n in (1, 7, 16, 17, 33, 51, 64):
        wqs = set()
        for m in ms:
            wq, wr = L.tsqr_mi_working_q_size_f64_r(m, n), L.tsqr_mi_working_r_size_f64_r(m, n)
            wqs.add(wq)
            assert wq >= L.tsqr_mi_working_q_size_f64(m, n) + 4096, (m, n, wq)       # the full entry's layout and Z_acc
            assert wr >= L.tsqr_mi_working_r_size_f64(m, n), (m, n, wr)
            # the second plan: at most 2048 waves over the 16-row tiles, one partial per workgroup of four waves
            nt = (n + 15) // 16
            tiles = (m + 15) // 16
            tpw = max(1, (tiles + 2047) // 2048)
            nwaves = (tiles + tpw - 1) // tpw
            assert wr >= ((nwaves + 3) // 4) * (nt * (nt + 1) // 2) * 256, (m, n, wr)
            assert wr <= 512 * 10 * 256, (m, n, wr)
        assert len(wqs) == 1, "wq depends on m"
    for m, n in ((0, 4), (4, 0), (0, 0)):
        assert L.tsqr_mi_working_q_size_f64_r(m, n) == 0 and L.tsqr_mi_working_r_size_f64_r(m, n) == 0


def test_r_invalid_sizes_without_gpu(bq):
    # every check comes before any HIP call: null pointers are safe
    L = bq.lib()
    z = ctypes.c_void_p(0)
    for (m, n) in [(4, 8), (0, 0), (0, 4), (4, 0)]:
        assert L.tsqr_mi_r_f64(0, z, max(n, 1), z, max(m, 1), m, n, z, z, z) == bq.error_invalid_matrix_size
    assert L.tsqr_mi_r_f64(0, z, 7, z, 100, 100, 8, z, z, z) == bq.error_invalid_matrix_size      # ldr < n
    assert L.tsqr_mi_r_f64(0, z, 8, z, 99, 100, 8, z, z, z) == bq.error_invalid_matrix_size       # lda < m
    assert L.tsqr_mi_r_f64(1, z, 65, z, 100, 100, 65, z, z, z) == bq.error_unsupported_mode
    assert "tsqr_mi_r_f64" in bq.last_error() and "n <= 64" in bq.last_error()
    assert L.tsqr_mi_last_sweeps_f64() == 0


def test_r_f64_operand_checks(bq):
    import torch
    m, n = 100, 8
    bf = bq.buffer_f64_r(False)        # (not allocated: every check below raises before the buffer is looked at)
    a64 = torch.zeros(m * n, dtype=torch.float64)
    r64 = torch.zeros(n * n, dtype=torch.float64)
    with pytest.raises(TypeError):
        bq.r_f64(r64.float(), n, a64, m, m, n, bf)
    with pytest.raises(TypeError):
        bq.r_f64(r64, n, a64.float(), m, m, n, bf)
    with pytest.raises(TypeError):
        bq.r_f64(r64.numpy(), n, a64, m, m, n, bf)
    with pytest.raises(TypeError):
        bq.r_f64(r64, n, a64, m, m, n, bf)                   # CPU tensors of the right type
    if torch.cuda.is_available():                              # (the GPU box: the size and overlap checks on device tensors)
        a = torch.zeros(m * n, dtype=torch.float64, device="cuda")
        r = torch.zeros(n * n, dtype=torch.float64, device="cuda")
        with pytest.raises(ValueError):
            bq.r_f64(r[:-1], n, a, m, m, n, bf)
        with pytest.raises(ValueError):
            bq.r_f64(r, n, a[:-1], m, m, n, bf)
        with pytest.raises(ValueError):
            bq.r_f64(r, n - 1, a, m, m, n, bf)
        with pytest.raises(ValueError):
            bq.r_f64(a[:n * n], n, a, m, m, n, bf)            # r overlaps a
        with pytest.raises(RuntimeError):
            bq.r_f64(r, n, a, m, m, n, bf)                     # everything in order but the buffer


def test_r_f64_operand_checks_cpu_sizes(bq):
    # the size and overlap rules on plain numbers (the helper r_f64 runs on the tensors' addresses)
    chk = bq.check_f64_r_operands
    m, n = 100, 8
    ok = dict(r=(10 ** 6, n * n), a=(10 ** 7, m * n))
    chk(m, n, n, m, **ok)
    chk(m, n, n + 3, m + 1, r=(10 ** 6, (n - 1) * (n + 3) + n), a=(10 ** 7, (n - 1) * (m + 1) + m))
    with pytest.raises(ValueError):
        chk(m, n, n, m, r=(10 ** 6, n * n - 1), a=ok["a"])
    with pytest.raises(ValueError):
        chk(m, n, n, m, r=ok["r"], a=(10 ** 7, m * n - 1))
    with pytest.raises(ValueError):
        chk(m, n, n - 1, m, **ok)
    with pytest.raises(ValueError):
        chk(m, n, n, m - 1, **ok)
    with pytest.raises(ValueError):
        chk(m, n, n, m, r=(10 ** 7 + 8 * (m * n - 1), n * n), a=ok["a"])      # r starts on a's last element
    with pytest.raises(ValueError):
        chk(m, n, n, m, r=(10 ** 7 - 8, n * n), a=ok["a"])                     # r ends inside a
    chk(m, n, n, m, r=(10 ** 7 - 8 * n * n, n * n), a=ok["a"])                 # r ends where a begins


CPP_SAMPLE = r"""
#include <tsqr/blockqr.hpp>
#include <cstdio>
int main() {
	const std::size_t m = 1000, n = 24;
	mtk::qr::buffer_fp64_r<true> bf;
	double *a = nullptr, *r = nullptr;
	if (hipMalloc(&a, sizeof(double) * m * n) != hipSuccess) return 0;   // (no GPU: compiled and linked is what the CPU test checks)
	(void)hipMalloc(&r, sizeof(double) * n * n);
	bf.allocate(m, n);
	const double* ca = a;
	const mtk::qr::state_t st = mtk::qr::r_fp64<true>(r, n, ca, m, m, n, bf);
	std::printf("state %d, sweeps %d, %zu bytes of work space\n", st, tsqr_mi_last_sweeps_f64(), bf.get_device_memory_size());
	bf.destroy();
	(void)hipFree(a); (void)hipFree(r);
	return 0;
}
"""


def test_cpp_r_fp64_compiles_and_links(bq):
    with compile_and_link(CPP_SAMPLE, "sample_fp64_r") as exe:
        assert os.path.exists(exe)

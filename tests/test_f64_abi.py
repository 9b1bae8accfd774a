"""CPU tests of the fp64 entry (tsqr_mi_qr_f64): exported symbols, work-space sizes, argument checks that come before any HIP
call, the Python operand checks of qr_f64, and a C++ caller of mtk::qr::qr_fp64 that compiles and links."""
import ctypes
import os

import pytest

from abi_util import compile_and_link

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F64_SYMBOLS = ("tsqr_mi_qr_f64", "tsqr_mi_working_q_size_f64", "tsqr_mi_working_r_size_f64", "tsqr_mi_last_sweeps_f64")


def test_f64_symbols_exported(bq):
    L = ctypes.CDLL(bq.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "tsqr_mi.h")).read()
    for sym in F64_SYMBOLS:
        assert hasattr(L, sym), sym
        assert sym + "(" in hdr, sym
        assert sym in bq.C_ABI_SYMBOLS, sym
    assert "#define TSQR_MI_ERROR_NOT_FINITE      3" in hdr
    assert bq.error_not_finite == 3


def _gram_need(m, n):
    # partials of the Gram pass: one per workgroup of four waves, at most 2048 waves over the 64-row chunks; NT (NT + 1) / 2 tiles of 256
    nt = (n + 15) // 16
    nch = (m + 63) // 64
    cpw = max(1, (nch + 2047) // 2048)
    nwaves = (nch + cpw - 1) // cpw
    return ((nwaves + 3) // 4) * (nt * (nt + 1) // 2) * 256


def test_f64_working_sizes(bq):
    L = bq.lib()
    for m in (1, 33, 9211, 1 << 20, 1 << 23):
        for n in (1, 7, 16, 51, 64):
            wq = L.tsqr_mi_working_q_size_f64(m, n)
            wr = L.tsqr_mi_working_r_size_f64(m, n)
            # wq: Z and one R factor (64 x 64 each), the summed Gram tiles (10 x 256 + the row count), four slots of status words
            assert wq >= 2 * 4096 + 10 * 256 + 1 + 8, (m, n, wq)
            assert wr >= _gram_need(m, n), (m, n, wr)
            assert wr <= 512 * 10 * 256, (m, n, wr)              # (never more than the 512 workgroups of partials)
    assert L.tsqr_mi_working_q_size_f64(0, 4) == 0 and L.tsqr_mi_working_r_size_f64(4, 0) == 0


def test_f64_invalid_sizes_without_gpu(bq):
    # every check comes before any HIP call: null pointers are safe
    L = bq.lib()
    z = ctypes.c_void_p(0)
    for (m, n) in [(4, 8), (0, 0), (0, 4), (4, 0)]:
        assert L.tsqr_mi_qr_f64(0, z, max(m, 1), z, max(n, 1), z, max(m, 1), m, n, z, z, z) == bq.error_invalid_matrix_size
    assert L.tsqr_mi_qr_f64(1, z, 100, z, 65, z, 100, 100, 65, z, z, z) == bq.error_unsupported_mode
    assert "n <= 64" in bq.last_error()
    # leading dimensions below the rows of their operand
    assert L.tsqr_mi_qr_f64(0, z, 99, z, 8, z, 100, 100, 8, z, z, z) == bq.error_invalid_matrix_size
    assert L.tsqr_mi_qr_f64(0, z, 100, z, 7, z, 100, 100, 8, z, z, z) == bq.error_invalid_matrix_size
    assert L.tsqr_mi_qr_f64(0, z, 100, z, 8, z, 99, 100, 8, z, z, z) == bq.error_invalid_matrix_size
    assert L.tsqr_mi_last_sweeps_f64() == 0


def test_qr_f64_operand_checks(bq):
    import torch
    m, n = 100, 8
    bf = bq.buffer_f64(False)          # (not allocated: every check below raises before the buffer is looked at)
    a64 = torch.zeros(m * n, dtype=torch.float64)
    r64 = torch.zeros(n * n, dtype=torch.float64)
    # float32 operands
    with pytest.raises(TypeError):
        bq.qr_f64(a64.float(), m, r64, n, a64, m, m, n, bf)
    with pytest.raises(TypeError):
        bq.qr_f64(a64, m, r64.float(), n, a64, m, m, n, bf)
    # CPU tensors of the right type
    with pytest.raises(TypeError):
        bq.qr_f64(a64, m, r64, n, a64.clone(), m, m, n, bf)
    if torch.cuda.is_available():                              # (the GPU box: the size and overlap checks on device tensors)
        dev = "cuda"
        a = torch.zeros(m * n, dtype=torch.float64, device=dev)
        q = torch.zeros(m * n, dtype=torch.float64, device=dev)
        r = torch.zeros(n * n, dtype=torch.float64, device=dev)
        with pytest.raises(ValueError):
            bq.qr_f64(q[:-1], m, r, n, a, m, m, n, bf)
        with pytest.raises(ValueError):
            bq.qr_f64(q, m, r[:-1], n, a, m, m, n, bf)
        with pytest.raises(ValueError):
            bq.qr_f64(q, m - 1, r, n, a, m, m, n, bf)
        with pytest.raises(ValueError):
            bq.qr_f64(a[1:], m, r, n, a, m, m - 1, n, bf)     # q overlaps a without being a
        with pytest.raises(ValueError):
            bq.qr_f64(q, m, a[:n * n], n, a, m, m, n, bf)     # r overlaps a


def test_qr_f64_operand_checks_cpu_sizes(bq):
    # the size and overlap rules on plain numbers (the same helper qr_f64 runs on the tensors' addresses)
    chk = bq.check_f64_operands
    m, n = 100, 8
    ok = dict(q=(0, m * n), r=(10 ** 6, n * n), a=(10 ** 7, m * n))
    chk(m, n, m, n, m, **ok)
    with pytest.raises(ValueError):
        chk(m, n, m, n, m, q=(0, m * n - 1), r=ok["r"], a=ok["a"])
    with pytest.raises(ValueError):
        chk(m, n, m, n, m, q=ok["q"], r=(10 ** 6, n * n - 1), a=ok["a"])
    with pytest.raises(ValueError):
        chk(m, n, m - 1, n, m, **ok)
    with pytest.raises(ValueError):
        chk(m, n, m, n - 1, m, **ok)
    # q == a (same address, same ld): in place, allowed
    chk(m, n, m, n, m, q=(10 ** 7, m * n), r=ok["r"], a=(10 ** 7, m * n))
    # q overlapping a elsewhere, or with another ld
    with pytest.raises(ValueError):
        chk(m, n, m, n, m, q=(10 ** 7 + 8, m * n), r=ok["r"], a=(10 ** 7, m * n + 1))
    with pytest.raises(ValueError):
        chk(m, n, m + 1, n, m, q=(10 ** 7, (m + 1) * n), r=ok["r"], a=(10 ** 7, (m + 1) * n))
    # r overlapping q or a
    with pytest.raises(ValueError):
        chk(m, n, m, n, m, q=ok["q"], r=(8 * (m * n - 1), n * n), a=ok["a"])
    with pytest.raises(ValueError):
        chk(m, n, m, n, m, q=ok["q"], r=(10 ** 7 - 8, n * n), a=ok["a"])


CPP_SAMPLE = r"""
#include <tsqr/blockqr.hpp>
#include <cstdio>
int main() {
	const std::size_t m = 1000, n = 24;
	mtk::qr::buffer_fp64<true> bf;
	double *a = nullptr, *q = nullptr, *r = nullptr;
	if (hipMalloc(&a, sizeof(double) * m * n) != hipSuccess) return 0;   // (no GPU: compiled and linked is what the CPU test checks)
	(void)hipMalloc(&q, sizeof(double) * m * n);
	(void)hipMalloc(&r, sizeof(double) * n * n);
	bf.allocate(m, n);
	const mtk::qr::state_t st = mtk::qr::qr_fp64<true>(q, m, r, n, a, m, m, n, bf);
	std::printf("state %d, sweeps %d\n", st, tsqr_mi_last_sweeps_f64());
	bf.destroy();
	(void)hipFree(a); (void)hipFree(q); (void)hipFree(r);
	return 0;
}
"""


def test_cpp_qr_fp64_compiles_and_links(bq):
    with compile_and_link(CPP_SAMPLE, "sample_fp64") as exe:
        assert os.path.exists(exe)

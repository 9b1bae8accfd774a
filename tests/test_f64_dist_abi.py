"""CPU tests of the row-partitioned fp64 entries (tsqr_mi_qr_f64_dist, _fn, _cb): exported and declared symbols with their prototypes,
work-space sizes, the argument checks that come before any HIP call and before any collective, the operand checks of
dist.RowPartitionedQRF64's binding, and a C++ caller of mtk::qr::qr_fp64_dist that compiles and links."""
import ctypes
import os

import pytest

from abi_util import compile_and_link, header_flat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEAD = "int reorth, double* q, size_t ldq, double* r, size_t ldr, double* a, size_t lda, size_t m_local, size_t n, void* wq, void* wr, "
PROTOTYPES = {
    "tsqr_mi_working_q_size_f64_dist": "size_t tsqr_mi_working_q_size_f64_dist(size_t m_local, size_t n, int nranks);",
    "tsqr_mi_working_r_size_f64_dist": "size_t tsqr_mi_working_r_size_f64_dist(size_t m_local, size_t n, int nranks);",
    "tsqr_mi_qr_f64_dist": "int tsqr_mi_qr_f64_dist(" + HEAD + "void* nccl_comm, int nranks, void* stream);",
    "tsqr_mi_qr_f64_dist_fn": "int tsqr_mi_qr_f64_dist_fn(" + HEAD + "void* nccl_comm, void* nccl_allreduce_fn, int nranks, void* stream);",
    "tsqr_mi_qr_f64_dist_cb": "int tsqr_mi_qr_f64_dist_cb(" + HEAD + "tsqr_mi_allreduce_f64_cb allreduce, void* user, int nranks, void* stream);",
}
CALLED = []
CB = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p)(lambda *a: CALLED.append(a) or 0)


def test_f64_dist_symbols_and_prototypes(bq):
    L = ctypes.CDLL(bq.LIB_PATH)
    hdr = header_flat()
    for sym, proto in PROTOTYPES.items():
        assert hasattr(L, sym), sym
        assert proto in hdr, proto
        assert sym in bq.C_ABI_SYMBOLS, sym
    lib = bq.lib()
    sz, vp, ci = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int
    head = [ci, vp, sz, vp, sz, vp, sz, sz, sz, vp, vp]
    assert lib.tsqr_mi_qr_f64_dist.argtypes == head + [vp, ci, vp]
    assert lib.tsqr_mi_qr_f64_dist_fn.argtypes == head + [vp, vp, ci, vp]
    assert lib.tsqr_mi_qr_f64_dist_cb.argtypes == head + [vp, vp, ci, vp]
    for name in ("tsqr_mi_working_q_size_f64_dist", "tsqr_mi_working_r_size_f64_dist"):
        assert getattr(lib, name).argtypes == [sz, sz, ci] and getattr(lib, name).restype is sz
    # the header repeats the warning of the fp32 block and states the contract
    assert "leaves the others waiting" in hdr and "GLOBAL row count must be >= n" in hdr
    hpp = open(os.path.join(ROOT, "include", "tsqr", "blockqr.hpp")).read()
    assert "struct buffer_fp64_dist" in hpp and "qr_fp64_dist(" in hpp
    from tsqr_gpu_amd import dist as tdist
    assert callable(tdist.RowPartitionedQRF64)
    assert callable(bq.get_working_q_size_f64_dist) and callable(bq.get_working_r_size_f64_dist)


def test_f64_dist_working_sizes(bq):
    L = bq.lib()
    for nranks in (1, 2, 8):
        assert L.tsqr_mi_working_q_size_f64_dist(0, 100, nranks) == 0 and L.tsqr_mi_working_r_size_f64_dist(0, 100, nranks) == 0
        assert L.tsqr_mi_working_q_size_f64_dist(100, 0, nranks) == 0 and L.tsqr_mi_working_r_size_f64_dist(100, 0, nranks) == 0
        for m in (1, 33, 40, 9211, 1 << 20, 1 << 23):                      # (m < n included: a block may be shorter than it is wide)
            for n in (1, 33, 64, 65, 200, 1024):
                assert L.tsqr_mi_working_q_size_f64_dist(m, n, nranks) >= L.tsqr_mi_working_q_size_f64_wide(m, n) > 0
                assert L.tsqr_mi_working_r_size_f64_dist(m, n, nranks) >= L.tsqr_mi_working_r_size_f64_wide(m, n) > 0
                assert bq.get_working_q_size_f64_dist(m, n, nranks) == L.tsqr_mi_working_q_size_f64_dist(m, n, nranks)
                assert bq.get_working_r_size_f64_dist(m, n, nranks) == L.tsqr_mi_working_r_size_f64_dist(m, n, nranks)
                # room for the summed Gram matrix and the row count behind it: what one exchange carries
                nb = (n + 63) // 64
                nt = (min(n, 64) + 15) // 16
                nelem = nt * (nt + 1) // 2 * 256 if n <= 64 else nb * (nb + 1) // 2 * 4096
                assert L.tsqr_mi_working_q_size_f64_dist(m, n, nranks) >= nelem + 1


def _entries(L, z):
    """the three entries as callables of (reorth, ldq, ldr, lda, m_local, n), each with a null all-reduce / communicator, and the _cb
    entry once more with a callback that must never run"""
    return [
        ("dist", lambda re_, ldq, ldr, lda, m, n: L.tsqr_mi_qr_f64_dist(re_, z, ldq, z, ldr, z, lda, m, n, z, z, z, 1, z)),
        ("dist_fn", lambda re_, ldq, ldr, lda, m, n: L.tsqr_mi_qr_f64_dist_fn(re_, z, ldq, z, ldr, z, lda, m, n, z, z, z, z, 1, z)),
        ("dist_cb", lambda re_, ldq, ldr, lda, m, n: L.tsqr_mi_qr_f64_dist_cb(re_, z, ldq, z, ldr, z, lda, m, n, z, z, z, z, 1, z)),
        ("dist_cb+cb", lambda re_, ldq, ldr, lda, m, n: L.tsqr_mi_qr_f64_dist_cb(re_, z, ldq, z, ldr, z, lda, m, n, z, z, CB, z, 2, z)),
    ]


def test_f64_dist_states_without_gpu(bq):
    # every check comes before any HIP call and any collective: null pointers are safe, the callback never runs
    L = bq.lib()
    z = ctypes.c_void_p(0)
    del CALLED[:]
    for name, call in _entries(L, z):
        for (m, n) in [(0, 0), (0, 4), (4, 0), (0, 200), (300, 0)]:
            assert call(0, max(m, 1), max(n, 1), max(m, 1), m, n) == bq.error_invalid_matrix_size, (name, m, n)
            assert "m_local >= 1" in bq.last_error(), (name, bq.last_error())
        # leading dimensions below the rows of their operand (n <= 64 and beyond)
        for (m, n) in [(300, 48), (300, 200), (40, 64)]:
            assert call(0, m - 1, n, m, m, n) == bq.error_invalid_matrix_size, (name, m, n)
            assert call(1, m, n - 1, m, m, n) == bq.error_invalid_matrix_size, (name, m, n)
            assert call(0, m, n, m - 1, m, n) == bq.error_invalid_matrix_size, (name, m, n)
            assert "ldq >= m_local" in bq.last_error()
        assert call(1, 2000, 1025, 2000, 2000, 1025) == bq.error_unsupported_mode, name
        assert "n <= 1024" in bq.last_error()
        assert call(0, 10, 1025, 10, 10, 1025) == bq.error_unsupported_mode, name            # (m_local < n is no size error)
        assert L.tsqr_mi_last_sweeps_f64() == 0
    # valid sizes, nothing to exchange with: state 2 with its text, still before any HIP call
    for name, call in _entries(L, z)[:3]:
        assert call(0, 300, 200, 300, 300, 200) == bq.error_unsupported_mode, name
        assert "all-reduce" in bq.last_error()
        assert call(0, 40, 64, 40, 40, 64) == bq.error_unsupported_mode, name
    assert CALLED == []


def test_row_partitioned_qr_f64_operand_checks(bq):
    """dist.RowPartitionedQRF64 checks dtype, device and sizes before it calls C (which cannot see an allocation)"""
    import torch
    from tsqr_gpu_amd import dist as tdist
    m, n = 300, 100
    drv = tdist.RowPartitionedQRF64.__new__(tdist.RowPartitionedQRF64)      # (no GPU here: the checks need no work space)
    drv.n, drv.m_local, drv.world = n, m, 1
    a = torch.zeros(m * n, dtype=torch.float64)
    r = torch.zeros(n * n, dtype=torch.float64)
    with pytest.raises(TypeError):
        drv._check_operands(a.float(), m, r, a, m, m)
    with pytest.raises(TypeError):
        drv._check_operands(a, m, r.float(), a, m, m)
    with pytest.raises(TypeError):
        drv._check_operands(a, m, r, [0.0] * (m * n), m, m)
    with pytest.raises(TypeError):
        drv._check_operands(a, m, r, a, m, m)                               # float64, but not on the GPU
    if torch.cuda.is_available():
        drv = tdist.RowPartitionedQRF64(m, n, comm="callbacks")
        a, q, r = a.cuda(), a.cuda(), r.cuda()
        for bad in ((q[:-1], m, r, a, m), (q, m, r[:-1], a, m), (q, m, r, a[:-1], m), (q, m - 1, r, a, m), (q, m, r, a, m - 1)):
            with pytest.raises(ValueError):
                drv.qr(*bad)
        with pytest.raises(ValueError):
            drv.qr(q, m + 1, r, a, m + 1, m_local=m + 1)                    # a taller block: q and a are short for it


CPP_SAMPLE = r"""
#include <tsqr/blockqr.hpp>
#include <cstdio>
int main() {
	const std::size_t m_local = 4000, n = 300;
	mtk::qr::buffer_fp64_dist<true> bf;
	double *a = nullptr, *q = nullptr, *r = nullptr;
	if (hipMalloc(&a, sizeof(double) * m_local * n) != hipSuccess) return 0;   // (no GPU: compiled and linked is what the CPU test checks)
	(void)hipMalloc(&q, sizeof(double) * m_local * n);
	(void)hipMalloc(&r, sizeof(double) * n * n);
	bf.allocate(m_local, n, 1);
	// no communicator in this sample: the call must come back with error_unsupported_mode before it touches anything
	const mtk::qr::state_t st = mtk::qr::qr_fp64_dist<true>(q, m_local, r, n, a, m_local, m_local, n, bf, nullptr, 1);
	std::printf("state %d (%s), %zu bytes of work space\n", st, tsqr_mi_last_error(), bf.get_device_memory_size());
	bf.destroy();
	(void)hipFree(a); (void)hipFree(q); (void)hipFree(r);
	return st == mtk::qr::error_unsupported_mode ? 0 : 1;
}
"""


def test_cpp_qr_fp64_dist_compiles_and_links(bq):
    with compile_and_link(CPP_SAMPLE, "sample_fp64_dist") as exe:
        assert os.path.exists(exe)

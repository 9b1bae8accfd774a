// A C++ caller of mtk::qr::qrcp_fp64 (include/tsqr/blockqr.hpp): a P = q r of a row-major 1000 x 24 matrix with Q, then R and the
// pivots alone.  tests/test_f64_qrcp_abi.py compiles and links it; on a machine without a GPU it ends at the first allocation.
#include <tsqr/blockqr.hpp>
#include <cstdio>

int main() {
	const std::size_t m = 1000, n = 24;
	double *a = nullptr, *q = nullptr, *r = nullptr;
	int* jpvt = nullptr;
	if (hipMalloc(&a, sizeof(double) * m * n) != hipSuccess) return 0;   // (no GPU: compiled and linked is what the CPU test checks)
	(void)hipMalloc(&q, sizeof(double) * m * n);
	(void)hipMalloc(&r, sizeof(double) * n * n);
	(void)hipMalloc(&jpvt, sizeof(int) * n);
	(void)hipMemset(a, 0, sizeof(double) * m * n);
	{
		mtk::qr::buffer_fp64_qrcp<false> bf;
		bf.allocate(m, n);
		const mtk::qr::state_t st = mtk::qr::qrcp_fp64<false>(q, n, r, n, jpvt, a, n, m, n, bf, nullptr, mtk::qr::row_major, mtk::qr::row_major);
		std::printf("jobq 1: state %d (a zero matrix: %d is expected), ladder sweeps %d, %zu bytes of work space\n", st,
		            mtk::qr::error_not_finite, tsqr_mi_last_sweeps_f64(), bf.get_device_memory_size());
	}
	{
		mtk::qr::buffer_fp64_qrcp<true, false> bf;
		bf.allocate(m, n);
		const mtk::qr::state_t st = mtk::qr::qrcp_fp64<true, false>(nullptr, 0, r, n, jpvt, a, n, m, n, bf, nullptr, mtk::qr::row_major);
		std::printf("jobq 0: state %d, %zu bytes of work space\n", st, bf.get_device_memory_size());
	}
	(void)hipFree(a); (void)hipFree(q); (void)hipFree(r); (void)hipFree(jpvt);
	return 0;
}

// A C++ caller of mtk::qr::svd_fp64 (include/tsqr/blockqr.hpp): a = u diag(s) v^T of a row-major 1000 x 24 matrix with U, then the
// singular values alone.  tests/test_f64_svd_abi.py compiles and links it; on a machine without a GPU it ends at the first allocation.
#include <tsqr/blockqr.hpp>
#include <cstdio>

int main() {
	const std::size_t m = 1000, n = 24;
	double *a = nullptr, *u = nullptr, *s = nullptr, *v = nullptr;
	if (hipMalloc(&a, sizeof(double) * m * n) != hipSuccess) return 0;   // (no GPU: compiled and linked is what the CPU test checks)
	(void)hipMalloc(&u, sizeof(double) * m * n);
	(void)hipMalloc(&s, sizeof(double) * n);
	(void)hipMalloc(&v, sizeof(double) * n * n);
	(void)hipMemset(a, 0, sizeof(double) * m * n);
	{
		mtk::qr::buffer_fp64_svd<false> bf;
		bf.allocate(m, n);
		const mtk::qr::state_t st = mtk::qr::svd_fp64<false>(u, n, s, v, n, a, n, m, n, bf, nullptr, mtk::qr::row_major, mtk::qr::row_major);
		std::printf("jobu 1: state %d (a zero matrix: %d is expected), ladder sweeps %d, Jacobi sweeps %d, %zu bytes of work space\n", st,
		            mtk::qr::error_not_finite, tsqr_mi_last_sweeps_f64(), tsqr_mi_last_jacobi_sweeps_f64(), bf.get_device_memory_size());
	}
	{
		mtk::qr::buffer_fp64_svd<true, false> bf;
		bf.allocate(m, n);
		const mtk::qr::state_t st = mtk::qr::svd_fp64<true, false>(nullptr, 0, s, nullptr, 0, a, n, m, n, bf, nullptr, mtk::qr::row_major);
		std::printf("jobu 0: state %d, %zu bytes of work space\n", st, bf.get_device_memory_size());
		if (st == mtk::qr::error_no_convergence) std::printf("the Jacobi iteration reached its cap\n");
	}
	(void)hipFree(a); (void)hipFree(u); (void)hipFree(s); (void)hipFree(v);
	return 0;
}

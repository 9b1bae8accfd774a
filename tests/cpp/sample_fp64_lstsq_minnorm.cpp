// A C++ caller of mtk::qr::lstsq_minnorm_fp64 (include/tsqr/blockqr.hpp): the rank and the minimum-norm least-squares solution of a
// row-major 1000 x 16 matrix whose column 11 is a copy of column 4, three right-hand sides, next to the basic solution of
// mtk::qr::lstsq_rank_fp64 on the same operands.  Rows 4 and 11 of the minimum-norm x are equal up to rounding and its norm is no larger.
// tests/test_f64_lstsq_minnorm_abi.py compiles and links it, tests/test_gpu_f64_lstsq_minnorm.py runs it; on a machine without a GPU it
// ends at the first allocation.
#include <tsqr/blockqr.hpp>
#include <cmath>
#include <cstdio>
#include <vector>

int main() {
	const std::size_t m = 1000, n = 16, nrhs = 3;
	double *a = nullptr, *b = nullptr, *x = nullptr, *r = nullptr;
	int* jpvt = nullptr;
	if (hipMalloc(&a, sizeof(double) * m * n) != hipSuccess) return 0;   // (no GPU: compiled and linked is what the CPU test checks)
	(void)hipMalloc(&b, sizeof(double) * m * nrhs);
	(void)hipMalloc(&x, sizeof(double) * n * nrhs);
	(void)hipMalloc(&r, sizeof(double) * n * n);
	(void)hipMalloc(&jpvt, sizeof(int) * n);
	std::vector<double> ha(m * n), hb(m * nrhs), hx(n * nrhs), hx0(n * nrhs);
	unsigned long long s = 12345;
	auto next = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0 - 0.5; };
	for (std::size_t i = 0; i < m; i++) {
		for (std::size_t j = 0; j < n; j++) ha[i * n + j] = next();
		ha[i * n + 11] = ha[i * n + 4];
		for (std::size_t j = 0; j < nrhs; j++) hb[i * nrhs + j] = next();
	}
	(void)hipMemcpy(a, ha.data(), sizeof(double) * m * n, hipMemcpyHostToDevice);
	(void)hipMemcpy(b, hb.data(), sizeof(double) * m * nrhs, hipMemcpyHostToDevice);
	const double *ca = a, *cb = b;
	mtk::qr::buffer_fp64_lstsq_rank<false> bf0;
	bf0.allocate(m, n, nrhs);
	int rank0 = -1;
	const mtk::qr::state_t st0 = mtk::qr::lstsq_rank_fp64<false>(x, n, r, n, jpvt, &rank0, ca, n, cb, nrhs, m, n, nrhs, bf0, 1e-8, 1, nullptr,
	                                                            mtk::qr::row_major, mtk::qr::row_major);
	(void)hipMemcpy(hx0.data(), x, sizeof(double) * n * nrhs, hipMemcpyDeviceToHost);
	bf0.destroy();
	mtk::qr::buffer_fp64_lstsq_minnorm<false> bf;
	bf.allocate(m, n, nrhs);
	int rank = -1;
	const mtk::qr::state_t st = mtk::qr::lstsq_minnorm_fp64<false>(x, n, r, n, jpvt, &rank, ca, n, cb, nrhs, m, n, nrhs, bf, 1e-8, 1, nullptr,
	                                                              mtk::qr::row_major, mtk::qr::row_major);
	(void)hipMemcpy(hx.data(), x, sizeof(double) * n * nrhs, hipMemcpyDeviceToHost);
	double twin = 0.0, norm = 0.0, norm0 = 0.0;
	for (std::size_t j = 0; j < nrhs; j++) {
		const double d = std::fabs(hx[j * n + 4] - hx[j * n + 11]) / std::fabs(hx[j * n + 4]);
		twin = d > twin ? d : twin;
		for (std::size_t i = 0; i < n; i++) { norm += hx[j * n + i] * hx[j * n + i]; norm0 += hx0[j * n + i] * hx0[j * n + i]; }
	}
	std::printf("states %d %d, ranks %d %d of %zu, rows 4 and 11 differ by %.1e relative, norm %.6f against the basic %.6f, %s, "
	            "ladder sweeps %d, %zu bytes of work space\n", st0, st, rank0, rank, n, twin, std::sqrt(norm), std::sqrt(norm0),
	            norm <= norm0 ? "not larger" : "LARGER", tsqr_mi_last_sweeps_f64(), bf.get_device_memory_size());
	bf.destroy();
	(void)hipFree(a); (void)hipFree(b); (void)hipFree(x); (void)hipFree(r); (void)hipFree(jpvt);
	return 0;
}

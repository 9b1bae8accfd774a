// The layout arguments of mtk::qr::r_fp64 and mtk::qr::lstsq_fp64 (include/tsqr/blockqr.hpp): a row-major A and B -- a plain C array
// a[m][n] -- are read where they lie.  First the argument checks, which need no GPU; then, where there is one, the same matrices in both
// layouts: R and X must have the same bits.
#include <tsqr/blockqr.hpp>
#include <cstdio>
#include <cstring>
#include <vector>

int main() {
	const std::size_t m = 1000, n = 24, nrhs = 3;
	// a row-major operand needs lda >= n, not lda >= m; a layout other than the two is an invalid size
	if (tsqr_mi_r_f64_lay(mtk::qr::row_major, 0, nullptr, n, nullptr, n - 1, m, n, nullptr, nullptr, nullptr) != mtk::qr::error_invalid_matrix_size) return 1;
	if (tsqr_mi_r_f64_lay(2, 0, nullptr, n, nullptr, m, m, n, nullptr, nullptr, nullptr) != mtk::qr::error_invalid_matrix_size) return 2;
	if (tsqr_mi_r_f64_lay(mtk::qr::row_major, 0, nullptr, 65, nullptr, 65, m, 65, nullptr, nullptr, nullptr) != mtk::qr::error_unsupported_mode) return 3;
	std::printf("argument checks ok\n");

	double *a_rm = nullptr, *a_cm = nullptr, *b_rm = nullptr, *b_cm = nullptr, *x = nullptr, *r = nullptr;
	if (hipMalloc(&a_rm, sizeof(double) * m * n) != hipSuccess) return 0;   // (no GPU: compiled, linked and the checks ran)
	(void)hipMalloc(&a_cm, sizeof(double) * m * n);
	(void)hipMalloc(&b_rm, sizeof(double) * m * nrhs);
	(void)hipMalloc(&b_cm, sizeof(double) * m * nrhs);
	(void)hipMalloc(&x, sizeof(double) * n * nrhs * 2);
	(void)hipMalloc(&r, sizeof(double) * n * n * 2);
	std::vector<double> ha(m * n), hat(m * n), hb(m * nrhs), hbt(m * nrhs);
	unsigned long long s = 12345;
	auto rnd = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) * 0x1p-53 - 0.5; };
	for (std::size_t i = 0; i < m; i++) {
		for (std::size_t j = 0; j < n; j++) hat[j * m + i] = ha[i * n + j] = rnd();
		for (std::size_t j = 0; j < nrhs; j++) hbt[j * m + i] = hb[i * nrhs + j] = rnd();
	}
	(void)hipMemcpy(a_rm, ha.data(), sizeof(double) * m * n, hipMemcpyHostToDevice);
	(void)hipMemcpy(a_cm, hat.data(), sizeof(double) * m * n, hipMemcpyHostToDevice);
	(void)hipMemcpy(b_rm, hb.data(), sizeof(double) * m * nrhs, hipMemcpyHostToDevice);
	(void)hipMemcpy(b_cm, hbt.data(), sizeof(double) * m * nrhs, hipMemcpyHostToDevice);

	mtk::qr::buffer_fp64_lstsq<true> bf;
	bf.allocate(m, n, nrhs);
	const mtk::qr::state_t st_cm = mtk::qr::lstsq_fp64<true>(x, n, r, n, a_cm, m, b_cm, m, m, n, nrhs, bf);
	const mtk::qr::state_t st_rm = mtk::qr::lstsq_fp64<true>(x + n * nrhs, n, r + n * n, n, a_rm, n, b_rm, nrhs, m, n, nrhs, bf, 1, nullptr,
	                                                         mtk::qr::row_major, mtk::qr::row_major);
	std::vector<double> hx(2 * n * nrhs), hr(2 * n * n);
	(void)hipMemcpy(hx.data(), x, sizeof(double) * hx.size(), hipMemcpyDeviceToHost);
	(void)hipMemcpy(hr.data(), r, sizeof(double) * hr.size(), hipMemcpyDeviceToHost);
	const bool same_x = std::memcmp(hx.data(), hx.data() + n * nrhs, sizeof(double) * n * nrhs) == 0;
	const bool same_r = std::memcmp(hr.data(), hr.data() + n * n, sizeof(double) * n * n) == 0;

	mtk::qr::buffer_fp64_r<false> bfr;
	bfr.allocate(m, n);
	const mtk::qr::state_t st_r = mtk::qr::r_fp64<false>(r, n, a_rm, n, m, n, bfr, nullptr, mtk::qr::row_major);
	std::printf("lstsq_fp64 states %d (column-major) %d (row-major), X %s, R %s; r_fp64 row-major state %d, %d sweeps\n", st_cm, st_rm,
	            same_x ? "bitwise equal" : "DIFFERS", same_r ? "bitwise equal" : "DIFFERS", st_r, tsqr_mi_last_sweeps_f64());
	bf.destroy();
	bfr.destroy();
	(void)hipFree(a_rm); (void)hipFree(a_cm); (void)hipFree(b_rm); (void)hipFree(b_cm); (void)hipFree(x); (void)hipFree(r);
	return (st_cm == 0 && st_rm == 0 && st_r == 0 && same_x && same_r) ? 0 : 4;
}

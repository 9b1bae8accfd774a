// The layout arguments of mtk::qr::qr_fp64_wide (include/tsqr/blockqr.hpp): a row-major A of more than 64 columns -- a plain C array
// a[m][n] -- is factored where it lies and Q is written row-major.  First the argument checks, which need no GPU; then, where there is
// one, the same matrix in both layouts: Q (read as a matrix) and R must have the same bits.
#include <tsqr/blockqr.hpp>
#include <cstdio>
#include <cstring>
#include <vector>

int main() {
	const std::size_t m = 1000, n = 100;
	using mtk::qr::col_major;
	using mtk::qr::row_major;
	// a row-major operand needs ld >= n, not ld >= m; a layout other than the two is an invalid size; n > 1024 is unsupported; in place
	// (here: both pointers null) needs one layout
	if (tsqr_mi_qr_f64_wide_lay(row_major, row_major, 0, nullptr, n, nullptr, n, nullptr, n - 1, m, n, nullptr, nullptr, nullptr) != mtk::qr::error_invalid_matrix_size) return 1;
	if (tsqr_mi_qr_f64_wide_lay(col_major, 2, 0, nullptr, m, nullptr, n, nullptr, m, m, n, nullptr, nullptr, nullptr) != mtk::qr::error_invalid_matrix_size) return 2;
	if (tsqr_mi_qr_f64_wide_lay(row_major, row_major, 0, nullptr, 1025, nullptr, 1025, nullptr, 1025, 2000, 1025, nullptr, nullptr, nullptr) != mtk::qr::error_unsupported_mode) return 3;
	if (tsqr_mi_qr_f64_wide_lay(row_major, col_major, 0, nullptr, m, nullptr, n, nullptr, m, m, n, nullptr, nullptr, nullptr) != mtk::qr::error_invalid_matrix_size) return 4;
	std::printf("argument checks ok\n");

	double *a_rm = nullptr, *a_cm = nullptr, *q_rm = nullptr, *q_cm = nullptr, *r = nullptr;
	if (hipMalloc(&a_rm, sizeof(double) * m * n) != hipSuccess) return 0;   // (no GPU: compiled, linked and the checks ran)
	(void)hipMalloc(&a_cm, sizeof(double) * m * n);
	(void)hipMalloc(&q_rm, sizeof(double) * m * n);
	(void)hipMalloc(&q_cm, sizeof(double) * m * n);
	(void)hipMalloc(&r, sizeof(double) * n * n * 2);
	std::vector<double> ha(m * n), hat(m * n);
	unsigned long long s = 12345;
	auto rnd = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) * 0x1p-53 - 0.5; };
	for (std::size_t i = 0; i < m; i++)
		for (std::size_t j = 0; j < n; j++) hat[j * m + i] = ha[i * n + j] = rnd();
	(void)hipMemcpy(a_rm, ha.data(), sizeof(double) * m * n, hipMemcpyHostToDevice);
	(void)hipMemcpy(a_cm, hat.data(), sizeof(double) * m * n, hipMemcpyHostToDevice);

	mtk::qr::buffer_fp64_wide<true> bf;
	bf.allocate(m, n);
	const mtk::qr::state_t st_cm = mtk::qr::qr_fp64_wide<true>(q_cm, m, r, n, a_cm, m, m, n, bf);     // an existing caller: unchanged
	const mtk::qr::state_t st_rm = mtk::qr::qr_fp64_wide<true>(q_rm, n, r + n * n, n, a_rm, n, m, n, bf, nullptr, row_major, row_major);
	std::vector<double> hq_cm(m * n), hq_rm(m * n), hr(2 * n * n);
	(void)hipMemcpy(hq_cm.data(), q_cm, sizeof(double) * m * n, hipMemcpyDeviceToHost);
	(void)hipMemcpy(hq_rm.data(), q_rm, sizeof(double) * m * n, hipMemcpyDeviceToHost);
	(void)hipMemcpy(hr.data(), r, sizeof(double) * hr.size(), hipMemcpyDeviceToHost);
	bool same_q = true;
	for (std::size_t i = 0; i < m && same_q; i++)
		for (std::size_t j = 0; j < n; j++)
			if (std::memcmp(&hq_rm[i * n + j], &hq_cm[j * m + i], sizeof(double)) != 0) { same_q = false; break; }
	const bool same_r = std::memcmp(hr.data(), hr.data() + n * n, sizeof(double) * n * n) == 0;
	// in place on the row-major copy
	const mtk::qr::state_t st_in = mtk::qr::qr_fp64_wide<true>(a_rm, n, r + n * n, n, a_rm, n, m, n, bf, nullptr, row_major, row_major);
	(void)hipMemcpy(hq_cm.data(), a_rm, sizeof(double) * m * n, hipMemcpyDeviceToHost);
	const bool same_in = std::memcmp(hq_cm.data(), hq_rm.data(), sizeof(double) * m * n) == 0;
	std::printf("qr_fp64_wide states %d (column-major) %d (row-major) %d (row-major, in place), Q %s, R %s, in place %s, %d sweeps\n", st_cm,
	            st_rm, st_in, same_q ? "bitwise equal" : "DIFFERS", same_r ? "bitwise equal" : "DIFFERS",
	            same_in ? "bitwise equal" : "DIFFERS", tsqr_mi_last_sweeps_f64());
	bf.destroy();
	(void)hipFree(a_rm); (void)hipFree(a_cm); (void)hipFree(q_rm); (void)hipFree(q_cm); (void)hipFree(r);
	return (st_cm == 0 && st_rm == 0 && st_in == 0 && same_q && same_r && same_in) ? 0 : 5;
}

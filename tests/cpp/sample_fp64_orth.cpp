// mtk::qr::orth_fp64 (include/tsqr/blockqr.hpp): a block W is orthogonalised against an orthonormal basis V, the step of a block Krylov
// method.  First the argument checks, which need no GPU; then, where there is one, two steps of a block Arnoldi-like recurrence: the
// basis grows from Q0 by the block the call returns, and the figures ||V^T Q||_F, ||Q^T Q - I||_F and ||W - V S - Q R||_F / ||W||_F are
// printed and held to the bounds of include/tsqr_mi.h.
#include <tsqr/blockqr.hpp>
#include <cmath>
#include <cstdio>
#include <vector>

int main() {
	const std::size_t m = 1000, n = 24, kmax = 2 * n;
	using mtk::qr::col_major;
	double one = 0.0;
	double* const p = &one;                                // (a non-null pointer no rejected call may touch)
	const auto bad = mtk::qr::error_invalid_matrix_size;
	if (tsqr_mi_orth_f64(col_major, col_major, 2, 0, p, m, p, n, p, n, p, m, m, n, 65, p, p, nullptr) != bad) return 1;        // n > 64
	if (tsqr_mi_orth_f64(col_major, col_major, 3, 0, p, m, p, n, p, n, p, m, m, n, n, p, p, nullptr) != bad) return 2;         // passes
	if (tsqr_mi_orth_f64(col_major, col_major, 2, 0, p, m, p, n, p, n, p, m, 2 * n - 1, n, n, p, p, nullptr) != bad) return 3; // k + n > m
	if (tsqr_mi_orth_f64(col_major, 2, 2, 0, p, m, p, n, p, n, p, m, m, n, n, p, p, nullptr) != bad) return 4;                 // layout
	if (tsqr_mi_orth_f64(col_major, col_major, 2, 0, p, m, p, n - 1, p, n, p, m, m, n, n, p, p, nullptr) != bad) return 5;     // lds < k
	if (one != 0.0) return 6;
	std::printf("argument checks ok\n");

	double *basis = nullptr, *w = nullptr, *s = nullptr, *r = nullptr;
	if (hipMalloc(&basis, sizeof(double) * m * (kmax + n)) != hipSuccess) return 0;   // (no GPU: compiled, linked and the checks ran)
	(void)hipMalloc(&w, sizeof(double) * m * n);
	(void)hipMalloc(&s, sizeof(double) * kmax * n);
	(void)hipMalloc(&r, sizeof(double) * n * n);
	unsigned long long seed = 2024;
	auto rnd = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (double)(seed >> 11) * 0x1p-53 - 0.5; };
	std::vector<double> h0(m * n), hw(m * n), hq(m * n), hs(kmax * n), hr(n * n), hv(m * kmax);   // (the basis holds up to kmax + n columns)
	for (auto& x : h0) x = rnd();
	(void)hipMemcpy(basis, h0.data(), sizeof(double) * m * n, hipMemcpyHostToDevice);
	mtk::qr::buffer_fp64<true> bf0;
	bf0.allocate(m, n);
	if (mtk::qr::qr_fp64<true>(basis, m, r, n, basis, m, m, n, bf0) != 0) return 7;     // Q0: the first n columns of the basis
	bf0.destroy();

	mtk::qr::buffer_fp64_orth<false> bf;
	bf.allocate(m, kmax, n);
	bool ok = true;
	std::size_t k = n;
	for (int step = 0; step < 2; step++) {
		// W = (a little of the basis) + 1e-6 noise: nearly inside span(V), where one round of projection is not enough
		(void)hipMemcpy(hv.data(), basis, sizeof(double) * m * k, hipMemcpyDeviceToHost);
		for (std::size_t j = 0; j < n; j++)
			for (std::size_t i = 0; i < m; i++) hw[j * m + i] = hv[((j * 7 + step) % k) * m + i] + 0.5 * hv[((j + 3) % k) * m + i] + 1e-6 * rnd();
		(void)hipMemcpy(w, hw.data(), sizeof(double) * m * n, hipMemcpyHostToDevice);
		const mtk::qr::state_t st = mtk::qr::orth_fp64<false>(w, m, s, k, r, n, basis, m, m, k, n, bf);
		(void)hipMemcpy(hq.data(), w, sizeof(double) * m * n, hipMemcpyDeviceToHost);
		(void)hipMemcpy(hs.data(), s, sizeof(double) * k * n, hipMemcpyDeviceToHost);
		(void)hipMemcpy(hr.data(), r, sizeof(double) * n * n, hipMemcpyDeviceToHost);
		long double vq = 0, qq = 0, res = 0, wn = 0;
		for (std::size_t j = 0; j < n; j++) {
			for (std::size_t c = 0; c < k; c++) {
				long double d = 0;
				for (std::size_t i = 0; i < m; i++) d += (long double)hv[c * m + i] * hq[j * m + i];
				vq += d * d;
			}
			for (std::size_t c = 0; c < n; c++) {
				long double d = c == j ? -1.0L : 0.0L;
				for (std::size_t i = 0; i < m; i++) d += (long double)hq[c * m + i] * hq[j * m + i];
				qq += d * d;
			}
			for (std::size_t i = 0; i < m; i++) {
				long double d = hw[j * m + i];
				for (std::size_t c = 0; c < k; c++) d -= (long double)hv[c * m + i] * hs[j * k + c];
				for (std::size_t c = 0; c <= j; c++) d -= (long double)hq[c * m + i] * hr[j * n + c];
				res += d * d;
				wn += (long double)hw[j * m + i] * hw[j * m + i];
			}
		}
		const double f_vq = (double)sqrtl(vq), f_qq = (double)sqrtl(qq), f_res = (double)sqrtl(res / wn);
		std::printf("step %d: k = %zu, state %d, %d sweeps, ||V^T Q||_F %.2e, ||Q^T Q - I||_F %.2e, residual %.2e\n", step, k, st,
		            tsqr_mi_last_sweeps_f64(), f_vq, f_qq, f_res);
		// (||V^T Q||_F: the floor of the bound of include/tsqr_mi.h, 4 max(k, n) 2^-53; the other two are the QR entry's claims)
		ok = ok && st == 0 && f_vq <= 4.0 * (double)(k > n ? k : n) * 0x1p-53 && f_qq <= 1e-11 && f_res <= 1e-13;
		(void)hipMemcpy(basis + m * k, w, sizeof(double) * m * n, hipMemcpyDeviceToDevice);   // the basis grows by Q
		k += n;
	}
	bf.destroy();
	(void)hipFree(basis); (void)hipFree(w); (void)hipFree(s); (void)hipFree(r);
	std::printf("%s\n", ok ? "orth_fp64 ok" : "orth_fp64 OUTSIDE THE BOUNDS");
	return ok ? 0 : 8;
}

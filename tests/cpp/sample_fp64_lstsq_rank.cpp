// A C++ caller of mtk::qr::lstsq_rank_fp64 (include/tsqr/blockqr.hpp): the rank and the basic least-squares solution of a row-major
// 1000 x 16 matrix whose column 11 is a copy of column 4, three right-hand sides.  tests/test_f64_lstsq_rank_abi.py compiles and links
// it, tests/test_gpu_f64_lstsq_rank.py runs it; on a machine without a GPU it ends at the first allocation.
#include <tsqr/blockqr.hpp>
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
	std::vector<double> ha(m * n), hb(m * nrhs), hx(n * nrhs);
	unsigned long long s = 12345;
	auto next = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0 - 0.5; };
	for (std::size_t i = 0; i < m; i++) {
		for (std::size_t j = 0; j < n; j++) ha[i * n + j] = next();
		ha[i * n + 11] = ha[i * n + 4];
		for (std::size_t j = 0; j < nrhs; j++) hb[i * nrhs + j] = next();
	}
	(void)hipMemcpy(a, ha.data(), sizeof(double) * m * n, hipMemcpyHostToDevice);
	(void)hipMemcpy(b, hb.data(), sizeof(double) * m * nrhs, hipMemcpyHostToDevice);
	mtk::qr::buffer_fp64_lstsq_rank<false> bf;
	bf.allocate(m, n, nrhs);
	int rank = -1;
	const double *ca = a, *cb = b;
	const mtk::qr::state_t st = mtk::qr::lstsq_rank_fp64<false>(x, n, r, n, jpvt, &rank, ca, n, cb, nrhs, m, n, nrhs, bf, 1e-8, 1, nullptr,
	                                                           mtk::qr::row_major, mtk::qr::row_major);
	(void)hipMemcpy(hx.data(), x, sizeof(double) * n * nrhs, hipMemcpyDeviceToHost);
	int zero_rows = 0;
	for (std::size_t i = 0; i < n; i++) {
		bool zero = true;
		for (std::size_t j = 0; j < nrhs; j++) zero = zero && hx[j * n + i] == 0.0;
		zero_rows += zero ? 1 : 0;
	}
	std::printf("state %d, rank %d of %zu, zero rows of x %d, ladder sweeps %d, %zu bytes of work space\n", st, rank, n, zero_rows,
	            tsqr_mi_last_sweeps_f64(), bf.get_device_memory_size());
	bf.destroy();
	(void)hipFree(a); (void)hipFree(b); (void)hipFree(x); (void)hipFree(r); (void)hipFree(jpvt);
	return 0;
}

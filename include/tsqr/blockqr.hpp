// blockqr.hpp -- MI355X-native replacement for the reference header of the same name.
//
// Keeps the public surface of reference src/blockqr.hpp (mtk::qr::compute_mode :12-23, tsqr_colmun_size :25,
// state_t :27-29, get_working_*_size :55-57, buffer :59-140, qr :142-175) so that callers written against
// enp1s0/tsqr-gpu compile unchanged, except for ONE argument: the reference passes a cublasHandle_t, which it
// uses only to obtain the stream (src/blockqr.cu:58-59) and to run its inter-panel GEMMs.  There is no cuBLAS on
// ROCm and no compatibility shim here; the last argument is a hipStream_t (mtk::qr::handle_t).  Overloads
// without the handle use the null stream.
//
// Header-only: everything forwards to the extern "C" ABI of libtsqr_mi.so (include/tsqr_mi.h).
// Link with -ltsqr_mi.
#ifndef __BLOCKQR_HPP__
#define __BLOCKQR_HPP__
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <type_traits>
#include "../tsqr_mi.h"
#include "tsqr.hpp"                             // mtk::tsqr (the reference's blockqr.hpp includes its tsqr.hpp as well)

namespace mtk {
namespace qr {

enum compute_mode {
	fp16_notc,
	fp16_tc_nocor,
	fp32_notc,
	fp32_tc_cor,
	fp32_tc_nocor,
	mixed_tc_cor_emu,
	tf32_tc_cor,
	tf32_tc_cor_emu,
	tf32_tc_nocor,
	tf32_tc_nocor_emu,
};

constexpr std::size_t tsqr_colmun_size = 16;

using state_t = int;
const state_t success_factorization = 0;
const state_t error_invalid_matrix_size = 1;
const state_t error_unsupported_mode = 2;      // new: compute_mode without a gfx950 implementation

using handle_t = hipStream_t;                  // takes the place of cublasHandle_t (see the header comment)

// reference src/blockqr.hpp:31-43: the one-panel engine's name for a block-QR mode (same enumerator names in both enums)
template <mtk::qr::compute_mode>
constexpr mtk::tsqr::compute_mode get_tsqr_compute_mode();
#define BQR_GET_TSQR_COMPUTE_MODE(mode) template<> constexpr mtk::tsqr::compute_mode get_tsqr_compute_mode<mtk::qr::compute_mode::mode>() {return mtk::tsqr::compute_mode::mode;}
BQR_GET_TSQR_COMPUTE_MODE(fp16_notc        );
BQR_GET_TSQR_COMPUTE_MODE(fp32_notc        );
BQR_GET_TSQR_COMPUTE_MODE(fp16_tc_nocor    );
BQR_GET_TSQR_COMPUTE_MODE(fp32_tc_nocor    );
BQR_GET_TSQR_COMPUTE_MODE(tf32_tc_nocor    );
BQR_GET_TSQR_COMPUTE_MODE(fp32_tc_cor      );
BQR_GET_TSQR_COMPUTE_MODE(tf32_tc_cor      );
BQR_GET_TSQR_COMPUTE_MODE(tf32_tc_cor_emu  );
BQR_GET_TSQR_COMPUTE_MODE(tf32_tc_nocor_emu);
BQR_GET_TSQR_COMPUTE_MODE(mixed_tc_cor_emu );

// Element types, as in reference src/tsqr.hpp:25-39 for the io type: float for the fp32 modes, IEEE binary16 (the reference's
// `half`) for fp16_notc / fp16_tc_nocor.  The WORKING types are float for every mode (the reference's are half for the fp16 modes
// and for the working Q of fp32_tc_nocor): this engine factors in fp32 and converts at the boundary.  The remaining modes are
// declared so that code naming them still compiles; calling them returns error_unsupported_mode.
using half_t = mtk::tsqr::half_t;
template <mtk::qr::compute_mode mode> struct get_working_q_type { using type = float; };
template <mtk::qr::compute_mode mode> struct get_working_r_type { using type = float; };
template <mtk::qr::compute_mode mode> struct get_io_type { using type = float; };
template <> struct get_io_type<fp16_notc> { using type = half_t; };
template <> struct get_io_type<fp16_tc_nocor> { using type = half_t; };

// get working memory size (element counts), reference src/blockqr.hpp:55-57
inline std::size_t get_working_q_size(const std::size_t m, const std::size_t n) { return tsqr_mi_working_q_size(m, n); }
inline std::size_t get_working_r_size(const std::size_t m, const std::size_t n) { return tsqr_mi_working_r_size(m, n); }
inline std::size_t get_working_l_size(const std::size_t m) { return tsqr_mi_working_l_size(m); }
// the same per mode: the fp16 I/O modes need room for the widened A, Q and R on top (what buffer<mode>::allocate uses; a caller
// that allocates by hand for an fp16 mode must use these, in elements of get_working_{q,r}_type<mode>::type = float)
template <mtk::qr::compute_mode mode> inline std::size_t get_working_q_size(const std::size_t m, const std::size_t n) {
	return (mode == fp16_notc || mode == fp16_tc_nocor) ? tsqr_mi_working_q_size_f16(m, n) : tsqr_mi_working_q_size(m, n);
}
template <mtk::qr::compute_mode mode> inline std::size_t get_working_r_size(const std::size_t m, const std::size_t n) {
	return (mode == fp16_notc || mode == fp16_tc_nocor) ? tsqr_mi_working_r_size_f16(m, n) : tsqr_mi_working_r_size(m, n);
}

namespace detail {
inline void check(hipError_t e, const char* what) {
	if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
// the C entry point of an io type
template <class IO> struct entry;
template <> struct entry<float> {
	static int call(int mode, int reorth, float* q, std::size_t ldq, float* r, std::size_t ldr, float* a, std::size_t lda, std::size_t m, std::size_t n,
	                void* wq, void* wr, float* reorth_w, unsigned* d_wl, unsigned* h_wl, hipStream_t stream) {
		return tsqr_mi_qr_f32(mode, reorth, q, ldq, r, ldr, a, lda, m, n, wq, wr, reorth_w, d_wl, h_wl, stream);
	}
};
template <> struct entry<half_t> {
	static int call(int mode, int reorth, half_t* q, std::size_t ldq, half_t* r, std::size_t ldr, half_t* a, std::size_t lda, std::size_t m, std::size_t n,
	                void* wq, void* wr, half_t* reorth_w, unsigned* d_wl, unsigned* h_wl, hipStream_t stream) {
		return tsqr_mi_qr_f16(mode, reorth, q, ldq, r, ldr, a, lda, m, n, wq, wr, reorth_w, d_wl, h_wl, stream);
	}
};
// Work space of a double-precision entry: two device arrays of doubles.  The buffers of the fp64 entries derive from it and add
// only their allocate(...), which names the entry's two size functions; they stay distinct types on purpose.
struct buffer_fp64_base {
	double* dwq;
	double* dwr;
	std::size_t total_memory_size;

	buffer_fp64_base() : dwq(nullptr), dwr(nullptr), total_memory_size(0lu) {}
	~buffer_fp64_base() { destroy(); }
	buffer_fp64_base(const buffer_fp64_base&) = delete;
	buffer_fp64_base& operator=(const buffer_fp64_base&) = delete;

	void destroy() {
		if (dwq) (void)hipFree(dwq);
		dwq = nullptr;
		if (dwr) (void)hipFree(dwr);
		dwr = nullptr;
	}

	std::size_t get_device_memory_size() const { return total_memory_size; }

protected:
	void allocate_doubles(const std::size_t wq_doubles, const std::size_t wr_doubles) {
		if (dwq != nullptr || dwr != nullptr) {
			throw std::runtime_error("The buffer has been already allocated");
		}
		const auto wq_size = sizeof(double) * wq_doubles;
		const auto wr_size = sizeof(double) * wr_doubles;
		check(hipMalloc(reinterpret_cast<void**>(&dwq), wq_size), "hipMalloc(dwq)");
		check(hipMalloc(reinterpret_cast<void**>(&dwr), wr_size), "hipMalloc(dwr)");
		total_memory_size = wq_size + wr_size;
	}
};
}  // namespace detail

template <mtk::qr::compute_mode mode, bool Reorthogonalize>
struct buffer {
	typename get_working_q_type<mode>::type* dwq;
	typename get_working_r_type<mode>::type* dwr;
	typename get_io_type<mode>::type* dw_reorth_r;
	unsigned* dl;
	unsigned* hl;

	std::size_t total_memory_size;

	buffer() : dwq(nullptr), dwr(nullptr), dw_reorth_r(nullptr), dl(nullptr), hl(nullptr), total_memory_size(0lu) {}
	~buffer() { destroy(); }
	buffer(const buffer&) = delete;
	buffer& operator=(const buffer&) = delete;

	void allocate(const std::size_t m, const std::size_t n) {
		if (dwq != nullptr || dwr != nullptr || dl != nullptr || hl != nullptr) {
			throw std::runtime_error("The buffer has been already allocated");
		}
		const auto wq_size = sizeof(typename get_working_q_type<mode>::type) * get_working_q_size<mode>(m, n);
		const auto wr_size = sizeof(typename get_working_r_type<mode>::type) * get_working_r_size<mode>(m, n);
		const auto l_size = sizeof(unsigned) * get_working_l_size(m);
		detail::check(hipMalloc(reinterpret_cast<void**>(&dwq), wq_size), "hipMalloc(dwq)");
		detail::check(hipMalloc(reinterpret_cast<void**>(&dwr), wr_size), "hipMalloc(dwr)");
		detail::check(hipMalloc(reinterpret_cast<void**>(&dl), l_size), "hipMalloc(dl)");
		detail::check(hipHostMalloc(reinterpret_cast<void**>(&hl), l_size), "hipHostMalloc(hl)");
		total_memory_size = wq_size + wr_size + l_size;
		if (Reorthogonalize) {
			const auto reorth_r_size = sizeof(typename get_io_type<mode>::type) * tsqr_mi_working_reorth_size(m);
			detail::check(hipMalloc(reinterpret_cast<void**>(&dw_reorth_r), reorth_r_size), "hipMalloc(dw_reorth_r)");
			total_memory_size += reorth_r_size;
		}
	}

	void destroy() {
		if (dwq) (void)hipFree(dwq);
		dwq = nullptr;
		if (dwr) (void)hipFree(dwr);
		dwr = nullptr;
		if (dw_reorth_r) (void)hipFree(dw_reorth_r);
		dw_reorth_r = nullptr;
		if (dl) (void)hipFree(dl);
		dl = nullptr;
		if (hl) (void)hipHostFree(hl);
		hl = nullptr;
	}

	// host-resident variants of the reference (src/blockqr.hpp:97-135): pinned host memory mapped to the device
	void allocate_host(const std::size_t m, const std::size_t n) {
		if (dwq != nullptr || dwr != nullptr || dl != nullptr || hl != nullptr) {
			throw std::runtime_error("The buffer has been already allocated");
		}
		const auto wq_size = sizeof(typename get_working_q_type<mode>::type) * get_working_q_size<mode>(m, n);
		const auto wr_size = sizeof(typename get_working_r_type<mode>::type) * get_working_r_size<mode>(m, n);
		const auto l_size = sizeof(unsigned) * get_working_l_size(m);
		detail::check(hipHostMalloc(reinterpret_cast<void**>(&dwq), wq_size), "hipHostMalloc(dwq)");
		detail::check(hipHostMalloc(reinterpret_cast<void**>(&dwr), wr_size), "hipHostMalloc(dwr)");
		detail::check(hipHostMalloc(reinterpret_cast<void**>(&dl), l_size), "hipHostMalloc(dl)");
		detail::check(hipHostMalloc(reinterpret_cast<void**>(&hl), l_size), "hipHostMalloc(hl)");
		total_memory_size = wq_size + wr_size + l_size;
		if (Reorthogonalize) {
			const auto reorth_r_size = sizeof(typename get_io_type<mode>::type) * tsqr_mi_working_reorth_size(m);
			detail::check(hipHostMalloc(reinterpret_cast<void**>(&dw_reorth_r), reorth_r_size), "hipHostMalloc(dw_reorth_r)");
			total_memory_size += reorth_r_size;
		}
	}

	void destroy_host() {
		if (dwq) (void)hipHostFree(dwq);
		dwq = nullptr;
		if (dwr) (void)hipHostFree(dwr);
		dwr = nullptr;
		if (dw_reorth_r) (void)hipHostFree(dw_reorth_r);
		dw_reorth_r = nullptr;
		if (dl) (void)hipHostFree(dl);
		dl = nullptr;
		if (hl) (void)hipHostFree(hl);
		hl = nullptr;
	}

	std::size_t get_device_memory_size() const { return total_memory_size; }
};

// reference src/blockqr.hpp:142-154 / src/blockqr.cu:394-433.  Blocking; returns state_t; runtime failures throw
// std::runtime_error (the reference throws from CUTF_CHECK_ERROR).
template <mtk::qr::compute_mode mode, bool Reorthogonalize>
inline state_t qr(
		typename mtk::qr::get_io_type<mode>::type* const q_ptr, const std::size_t ldq,
		typename mtk::qr::get_io_type<mode>::type* const r_ptr, const std::size_t ldr,
		typename mtk::qr::get_io_type<mode>::type* const a_ptr, const std::size_t lda,
		const std::size_t m, const std::size_t n,
		typename mtk::qr::get_working_q_type<mode>::type* const wq_ptr,
		typename mtk::qr::get_working_r_type<mode>::type* const wr_ptr,
		typename mtk::qr::get_io_type<mode>::type* const reorth_r_ptr,
		unsigned* const d_wl_ptr,
		unsigned* const h_wl_ptr,
		handle_t const stream = nullptr) {
	const int st = detail::entry<typename mtk::qr::get_io_type<mode>::type>::call(static_cast<int>(mode), Reorthogonalize ? 1 : 0,
	                              q_ptr, ldq, r_ptr, ldr, a_ptr, lda, m, n,
	                              wq_ptr, wr_ptr, reorth_r_ptr, d_wl_ptr, h_wl_ptr, stream);
	if (st < 0) throw std::runtime_error(std::string("mtk::qr::qr: ") + tsqr_mi_last_error());
	return st;
}

// reference src/blockqr.hpp:155-175
template <mtk::qr::compute_mode mode, bool Reorthogonalize>
inline state_t qr(
		typename mtk::qr::get_io_type<mode>::type* const q_ptr, const std::size_t ldq,
		typename mtk::qr::get_io_type<mode>::type* const r_ptr, const std::size_t ldr,
		typename mtk::qr::get_io_type<mode>::type* const a_ptr, const std::size_t lda,
		const std::size_t m, const std::size_t n,
		buffer<mode, Reorthogonalize>& bf,
		handle_t const stream = nullptr) {
	return qr<mode, Reorthogonalize>(
			q_ptr, ldq,
			r_ptr, ldr,
			a_ptr, lda,
			m, n,
			bf.dwq,
			bf.dwr,
			bf.dw_reorth_r,
			bf.dl,
			bf.hl,
			stream
			);
}

// Not in the reference: its qr() synchronises the stream itself (src/blockqr.cu:78, 122, 140), so one call's host round trip sits
// between two calls of a loop.  submit enqueues a call's first attempt and returns; finish waits for it (and completes the fallback
// ladder for a matrix the conditioning check rejected).  Two calls of a thread may be in flight: a loop over many matrices keeps the
// GPU busy back to back (tsqr_mi_qr_f32_submit / _finish, include/tsqr_mi.h, for the rules).  fp32 I/O modes.
using ticket = tsqr_mi_ticket;
template <mtk::qr::compute_mode mode, bool Reorthogonalize>
inline void qr_submit(
		ticket& t,
		float* const q_ptr, const std::size_t ldq,
		float* const r_ptr, const std::size_t ldr,
		float* const a_ptr, const std::size_t lda,
		const std::size_t m, const std::size_t n,
		buffer<mode, Reorthogonalize>& bf,
		handle_t const stream = nullptr) {
	static_assert(std::is_same<typename mtk::qr::get_io_type<mode>::type, float>::value, "qr_submit takes the fp32 I/O modes");
	const int st = tsqr_mi_qr_f32_submit(static_cast<int>(mode), Reorthogonalize ? 1 : 0, q_ptr, ldq, r_ptr, ldr, a_ptr, lda, m, n,
	                                     bf.dwq, bf.dwr, bf.dw_reorth_r, bf.dl, bf.hl, stream, &t);
	if (st < 0) throw std::runtime_error(std::string("mtk::qr::qr_submit: ") + tsqr_mi_last_error());
}
inline state_t qr_finish(ticket& t) {
	const int st = tsqr_mi_qr_f32_finish(&t);
	if (st < 0) throw std::runtime_error(std::string("mtk::qr::qr_finish: ") + tsqr_mi_last_error());
	return st;
}

// Not in the reference either: `count` different matrices of one shape through one call (tsqr_mi_qr_f32_batch).  What a caller's loop
//     for (i = 0; i < count; i++) mtk::qr::qr<mode, Reorth>(q[i], ldq, r[i], ldr, a[i], lda, m, n, buffer, handle);
// computes -- bit for bit, including the fallback ladder of a matrix the conditioning check rejects -- issued as a stream: the 22 us
// in which one workgroup factors the Gram matrix of matrix i are hidden in the Gram pass of matrix i + 1 (tsqr_mi.h for the rules:
// calls i and i + 1 must not conflict -- Q(i) or R(i) overlapping Q(i + 1), R(i + 1) or A(i + 1), or Q(i + 1) or R(i + 1) overlapping
// A(i) -- or they run one after the other; in place, q[i] == a[i], is fine).  q, r, a: host arrays of device pointers.
// states (optional): the state_t of every call.  Returns the first non-zero state_t.  All implemented modes (half-typed pointers for the fp16 I/O modes).
template <mtk::qr::compute_mode mode, bool Reorthogonalize>
inline state_t qr_batch(
		const std::size_t count,
		typename mtk::qr::get_io_type<mode>::type* const* const q_ptrs, const std::size_t ldq,
		typename mtk::qr::get_io_type<mode>::type* const* const r_ptrs, const std::size_t ldr,
		typename mtk::qr::get_io_type<mode>::type* const* const a_ptrs, const std::size_t lda,
		const std::size_t m, const std::size_t n,
		buffer<mode, Reorthogonalize>& bf,
		handle_t const stream = nullptr,
		state_t* const states = nullptr) {
	int st;
	if constexpr (std::is_same<typename mtk::qr::get_io_type<mode>::type, float>::value)
		st = tsqr_mi_qr_f32_batch(static_cast<int>(count), static_cast<int>(mode), Reorthogonalize ? 1 : 0, q_ptrs, ldq, r_ptrs, ldr, a_ptrs, lda, m, n,
		                          bf.dwq, bf.dwr, bf.dw_reorth_r, bf.dl, bf.hl, stream, states);
	else                                                  // the half-typed modes (same pointer arrays, elements are halves)
		st = tsqr_mi_qr_f16_batch(static_cast<int>(count), static_cast<int>(mode), Reorthogonalize ? 1 : 0, reinterpret_cast<void* const*>(q_ptrs), ldq,
		                          reinterpret_cast<void* const*>(r_ptrs), ldr, reinterpret_cast<const void* const*>(a_ptrs), lda, m, n,
		                          bf.dwq, bf.dwr, bf.dw_reorth_r, bf.dl, bf.hl, stream, states);
	if (st < 0) throw std::runtime_error(std::string("mtk::qr::qr_batch: ") + tsqr_mi_last_error());
	return st;
}

// Not in the reference: double-precision tall-skinny QR, 1 <= n <= m, n <= 64 (tsqr_mi_qr_f64, include/tsqr_mi.h for the contract).
// Reorthogonalize = false: one CholeskyQR sweep when the device's estimate of its loss of orthogonality is <= 1e-12, CholeskyQR2
// otherwise; true: CholeskyQR2 at least.  Either falls back to shifted CholeskyQR3 on a Gram matrix the Cholesky step rejects.
// Returns success_factorization, error_invalid_matrix_size, error_unsupported_mode (n > 64) or error_not_finite.
const state_t error_not_finite = TSQR_MI_ERROR_NOT_FINITE;

template <bool Reorthogonalize>
struct buffer_fp64 : detail::buffer_fp64_base {
	void allocate(const std::size_t m, const std::size_t n) { allocate_doubles(tsqr_mi_working_q_size_f64(m, n), tsqr_mi_working_r_size_f64(m, n)); }
};

// layout_t: how a (for qr_fp64 also q, for lstsq_fp64 also b) is stored.  row_major: element (i, j) at ptr[i * ld + j], ld >= the column
// count, read (q: written) where it lies (tsqr_mi_qr_f64_lay / tsqr_mi_r_f64_lay / tsqr_mi_lstsq_f64_lay); r and x stay column-major, and
// every result has the bits of the column-major call on the same matrix.
using layout_t = int;
const layout_t col_major = TSQR_MI_COL_MAJOR;
const layout_t row_major = TSQR_MI_ROW_MAJOR;

// a_layout, q_layout: the layouts of a and of q (they need not agree; in place, q_ptr == a_ptr, needs equal layouts and ldq == lda)
template <bool Reorthogonalize>
inline state_t qr_fp64(
		double* const q_ptr, const std::size_t ldq,
		double* const r_ptr, const std::size_t ldr,
		double* const a_ptr, const std::size_t lda,
		const std::size_t m, const std::size_t n,
		buffer_fp64<Reorthogonalize>& bf,
		handle_t const stream = nullptr,
		const layout_t a_layout = col_major, const layout_t q_layout = col_major) {
	const int st = tsqr_mi_qr_f64_lay(a_layout, q_layout, Reorthogonalize ? 1 : 0, q_ptr, ldq, r_ptr, ldr, a_ptr, lda, m, n, bf.dwq, bf.dwr, stream);
	if (st < 0) throw std::runtime_error(std::string("mtk::qr::qr_fp64: ") + tsqr_mi_last_error());
	return st;
}

// Not in the reference: a = u diag(s) v^T in double precision, 1 <= n <= m, n <= 64 (tsqr_mi_svd_f64, include/tsqr_mi.h for the
// contract): the ladder of qr_fp64 into u, one-sided Jacobi on R, u <- u W.  s takes n values, descending; v (n x n, column-major, ldv;
// may be null) takes V.  ComputeU = false: u_ptr is ignored, a is read only and the work space is that of r_fp64.  a_layout, u_layout
// as for qr_fp64 (in place, u_ptr == a_ptr, needs equal layouts and ldu == lda).  Returns the states of qr_fp64 or error_no_convergence.
const state_t error_no_convergence = TSQR_MI_ERROR_NO_CONVERGENCE;

template <bool Reorthogonalize, bool ComputeU = true>
struct buffer_fp64_svd : detail::buffer_fp64_base {
	void allocate(const std::size_t m, const std::size_t n) {
		allocate_doubles(tsqr_mi_working_q_size_f64_svd(m, n, ComputeU ? 1 : 0), tsqr_mi_working_r_size_f64_svd(m, n, ComputeU ? 1 : 0));
	}
};

template <bool Reorthogonalize, bool ComputeU = true>
inline state_t svd_fp64(
		double* const u_ptr, const std::size_t ldu,
		double* const s_ptr,
		double* const v_ptr, const std::size_t ldv,
		double* const a_ptr, const std::size_t lda,
		const std::size_t m, const std::size_t n,
		buffer_fp64_svd<Reorthogonalize, ComputeU>& bf,
		handle_t const stream = nullptr,
		const layout_t a_layout = col_major, const layout_t u_layout = col_major) {
	const int st = tsqr_mi_svd_f64(a_layout, u_layout, ComputeU ? 1 : 0, Reorthogonalize ? 1 : 0, u_ptr, ldu, s_ptr, v_ptr, ldv, a_ptr, lda, m, n,
	                               bf.dwq, bf.dwr, stream);
	if (st < 0) throw std::runtime_error(std::string("mtk::qr::svd_fp64: ") + tsqr_mi_last_error());
	return st;
}

// Not in the reference: a P = q r with column pivoting in double precision, 1 <= n <= m, n <= 64 (tsqr_mi_qrcp_f64, include/tsqr_mi.h for
// the contract): the ladder of qr_fp64 into q, a Householder QR with column pivoting of R on one workgroup, q <- q H.  r (n x n,
// column-major, ldr) takes R, diag(R) >= 0 and non-increasing; jpvt takes n 0-based pivots (device memory): column j of a P is column
// jpvt[j] of a.  ComputeQ = false: q_ptr is ignored, a is read only and the work space is that of r_fp64.  a_layout, q_layout as for
// qr_fp64 (in place, q_ptr == a_ptr, needs equal layouts and ldq == lda).  Returns the states of qr_fp64.
template <bool Reorthogonalize, bool ComputeQ = true>
struct buffer_fp64_qrcp : detail::buffer_fp64_base {
	void allocate(const std::size_t m, const std::size_t n) {
		allocate_doubles(tsqr_mi_working_q_size_f64_qrcp(m, n, ComputeQ ? 1 : 0), tsqr_mi_working_r_size_f64_qrcp(m, n, ComputeQ ? 1 : 0));
	}
};

template <bool Reorthogonalize, bool ComputeQ = true>
inline state_t qrcp_fp64(
		double* const q_ptr, const std::size_t ldq,
		double* const r_ptr, const std::size_t ldr,
		int* const jpvt_ptr,
		double* const a_ptr, const std::size_t lda,
		const std::size_t m, const std::size_t n,
		buffer_fp64_qrcp<Reorthogonalize, ComputeQ>& bf,
		handle_t const stream = nullptr,
		const layout_t a_layout = col_major, const layout_t q_layout = col_major) {
	const int st = tsqr_mi_qrcp_f64(a_layout, q_layout, ComputeQ ? 1 : 0, Reorthogonalize ? 1 : 0, q_ptr, ldq, r_ptr, ldr, jpvt_ptr, a_ptr, lda, m, n,
	                                bf.dwq, bf.dwr, stream);
	if (st < 0) throw std::runtime_error(std::string("mtk::qr::qrcp_fp64: ") + tsqr_mi_last_error());
	return st;
}

// Not in the reference: the R factor of qr_fp64 alone, Q never formed (tsqr_mi_r_f64, include/tsqr_mi.h for the contract): a is read
// only, no m x n work space.  Returns the states of qr_fp64.
template <bool Reorthogonalize>
struct buffer_fp64_r : detail::buffer_fp64_base {
	void allocate(const std::size_t m, const std::size_t n) { allocate_doubles(tsqr_mi_working_q_size_f64_r(m, n), tsqr_mi_working_r_size_f64_r(m, n)); }
};

template <bool Reorthogonalize>
inline state_t r_fp64(
		double* const r_ptr, const std::size_t ldr,
		const double* const a_ptr, const std::size_t lda,
		const std::size_t m, const std::size_t n,
		buffer_fp64_r<Reorthogonalize>& bf,
		handle_t const stream = nullptr,
		const layout_t a_layout = col_major) {
	const int st = tsqr_mi_r_f64_lay(a_layout, Reorthogonalize ? 1 : 0, r_ptr, ldr, a_ptr, lda, m, n, bf.dwq, bf.dwr, stream);
	if (st < 0) throw std::runtime_error(std::string("mtk::qr::r_fp64: ") + tsqr_mi_last_error());
	return st;
}

// Not in the reference: X = argmin ||A X - B||_F and the R of r_fp64, on the R-only factorisation (tsqr_mi_lstsq_f64, include/tsqr_mi.h
// for the contract and the accuracy statement): a and b are read only, no work space of size m.  Returns the states of r_fp64;
// error_unsupported_mode also for nrhs > 16 or refine outside 0 .. 4.
template <bool Reorthogonalize>
struct buffer_fp64_lstsq : detail::buffer_fp64_base {
	void allocate(const std::size_t m, const std::size_t n, const std::size_t nrhs) { allocate_doubles(tsqr_mi_working_q_size_f64_lstsq(m, n, nrhs), tsqr_mi_working_r_size_f64_lstsq(m, n, nrhs)); }
};

template <bool Reorthogonalize>
inline state_t lstsq_fp64(
		double* const x_ptr, const std::size_t ldx,
		double* const r_ptr, const std::size_t ldr,
		const double* const a_ptr, const std::size_t lda,
		const double* const b_ptr, const std::size_t ldb,
		const std::size_t m, const std::size_t n, const std::size_t nrhs,
		buffer_fp64_lstsq<Reorthogonalize>& bf,
		const int refine = 1,
		handle_t const stream = nullptr,
		const layout_t a_layout = col_major, const layout_t b_layout = col_major) {
	const int st = tsqr_mi_lstsq_f64_lay(a_layout, b_layout, Reorthogonalize ? 1 : 0, refine, x_ptr, ldx, r_ptr, ldr, a_ptr, lda, b_ptr, ldb,
	                                     m, n, nrhs, bf.dwq, bf.dwr, stream);
	if (st < 0) throw std::runtime_error(std::string("mtk::qr::lstsq_fp64: ") + tsqr_mi_last_error());
	return st;
}

// Not in the reference: the rank of A and the basic solution of min ||A X - B||_F on its numerically independent columns, on the pivoted
// R-only factorisation (tsqr_mi_lstsq_rank_f64, include/tsqr_mi.h for the contract and the measured accuracy): a and b are read only,
// no work space of size m.  r and jpvt (n ints on the device) are those of qrcp_fp64 without Q; rank is a host int; rows jpvt[rank:] of
// x are exact zeros.  rcond: column j is retained when R_jj > rcond R_00; negative: max(m, n) 2^-52.  Returns the states of lstsq_fp64;
// error_invalid_matrix_size also for a null pointer, error_unsupported_mode also for rcond >= 1 or NaN.
template <bool Reorthogonalize>
struct buffer_fp64_lstsq_rank : detail::buffer_fp64_base {
	void allocate(const std::size_t m, const std::size_t n, const std::size_t nrhs) { allocate_doubles(tsqr_mi_working_q_size_f64_lstsq_rank(m, n, nrhs), tsqr_mi_working_r_size_f64_lstsq_rank(m, n, nrhs)); }
};

template <bool Reorthogonalize>
inline state_t lstsq_rank_fp64(
		double* const x_ptr, const std::size_t ldx,
		double* const r_ptr, const std::size_t ldr,
		int* const jpvt_ptr, int* const rank,
		const double* const a_ptr, const std::size_t lda,
		const double* const b_ptr, const std::size_t ldb,
		const std::size_t m, const std::size_t n, const std::size_t nrhs,
		buffer_fp64_lstsq_rank<Reorthogonalize>& bf,
		const double rcond = -1.0,
		const int refine = 1,
		handle_t const stream = nullptr,
		const layout_t a_layout = col_major, const layout_t b_layout = col_major) {
	const int st = tsqr_mi_lstsq_rank_f64(a_layout, b_layout, Reorthogonalize ? 1 : 0, refine, rcond, x_ptr, ldx, r_ptr, ldr, jpvt_ptr, rank,
	                                      a_ptr, lda, b_ptr, ldb, m, n, nrhs, bf.dwq, bf.dwr, stream);
	if (st < 0) throw std::runtime_error(std::string("mtk::qr::lstsq_rank_fp64: ") + tsqr_mi_last_error());
	return st;
}

// Not in the reference: lstsq_rank_fp64 with the MINIMUM-NORM solution of the problem truncated at the pivoted-QR rank, LAPACK's dgelsy
// (tsqr_mi_lstsq_minnorm_f64, include/tsqr_mi.h for the method, the definition and the measured accuracy).  The arguments, states and
// r, jpvt, rank of lstsq_rank_fp64; every row of x may be non-zero; at full rank x is bitwise lstsq_rank_fp64's.
template <bool Reorthogonalize>
struct buffer_fp64_lstsq_minnorm : detail::buffer_fp64_base {
	void allocate(const std::size_t m, const std::size_t n, const std::size_t nrhs) { allocate_doubles(tsqr_mi_working_q_size_f64_lstsq_minnorm(m, n, nrhs), tsqr_mi_working_r_size_f64_lstsq_minnorm(m, n, nrhs)); }
};

template <bool Reorthogonalize>
inline state_t lstsq_minnorm_fp64(
		double* const x_ptr, const std::size_t ldx,
		double* const r_ptr, const std::size_t ldr,
		int* const jpvt_ptr, int* const rank,
		const double* const a_ptr, const std::size_t lda,
		const double* const b_ptr, const std::size_t ldb,
		const std::size_t m, const std::size_t n, const std::size_t nrhs,
		buffer_fp64_lstsq_minnorm<Reorthogonalize>& bf,
		const double rcond = -1.0,
		const int refine = 1,
		handle_t const stream = nullptr,
		const layout_t a_layout = col_major, const layout_t b_layout = col_major) {
	const int st = tsqr_mi_lstsq_minnorm_f64(a_layout, b_layout, Reorthogonalize ? 1 : 0, refine, rcond, x_ptr, ldx, r_ptr, ldr, jpvt_ptr, rank,
	                                         a_ptr, lda, b_ptr, ldb, m, n, nrhs, bf.dwq, bf.dwr, stream);
	if (st < 0) throw std::runtime_error(std::string("mtk::qr::lstsq_minnorm_fp64: ") + tsqr_mi_last_error());
	return st;
}
// Not in the reference: a block w (m x n) orthogonalised against an orthonormal basis v (m x k, read only), the step of block Arnoldi,
// block Lanczos, LOBPCG and randomised range finders (tsqr_mi_orth_f64, include/tsqr_mi.h for the method and the contract): w is
// overwritten by q with v^T q = 0, q^T q = I and w_in = v s + q r; s (k x n, lds) and r (n x n upper triangular, ldr) are column-major.
// 1 <= n <= 64, 1 <= k <= 1024, k + n <= m.  passes: 2 (BCGS2, the default) or 1.  Returns success_factorization,
// error_invalid_matrix_size (every size, layout or passes error: this entry has no error_unsupported_mode) or error_not_finite, after
// which w, s and r are undefined.  State 0 is no test that w was independent of v: compare diag(r) with w's column norms.
template <bool Reorthogonalize>
struct buffer_fp64_orth : detail::buffer_fp64_base {
	void allocate(const std::size_t m, const std::size_t k, const std::size_t n) { allocate_doubles(tsqr_mi_working_q_size_f64_orth(m, k, n), tsqr_mi_working_r_size_f64_orth(m, k, n)); }
};

template <bool Reorthogonalize>
inline state_t orth_fp64(
		double* const w_ptr, const std::size_t ldw,
		double* const s_ptr, const std::size_t lds,
		double* const r_ptr, const std::size_t ldr,
		const double* const v_ptr, const std::size_t ldv,
		const std::size_t m, const std::size_t k, const std::size_t n,
		buffer_fp64_orth<Reorthogonalize>& bf,
		handle_t const stream = nullptr,
		const layout_t v_layout = col_major, const layout_t w_layout = col_major,
		const int passes = 2) {
	const int st = tsqr_mi_orth_f64(v_layout, w_layout, passes, Reorthogonalize ? 1 : 0, w_ptr, ldw, s_ptr, lds, r_ptr, ldr, v_ptr, ldv, m, k, n,
	                                bf.dwq, bf.dwr, stream);
	if (st < 0) throw std::runtime_error(std::string("mtk::qr::orth_fp64: ") + tsqr_mi_last_error());
	return st;
}
// Not in the reference: double-precision tall-skinny QR for 1 <= n <= 1024, n <= m (tsqr_mi_qr_f64_wide, include/tsqr_mi.h for the
// contract): qr_fp64 itself for n <= 64, whole-matrix CholeskyQR sweeps with the same ladder beyond.  Returns success_factorization,
// error_invalid_matrix_size, error_unsupported_mode (n > 1024) or error_not_finite.  a_layout, q_layout (tsqr_mi_qr_f64_wide_lay): the
// layouts of a and of q as for qr_fp64 -- they need not agree; in place, q_ptr == a_ptr, needs equal layouts and ldq == lda.
template <bool Reorthogonalize>
struct buffer_fp64_wide : detail::buffer_fp64_base {
	void allocate(const std::size_t m, const std::size_t n) { allocate_doubles(tsqr_mi_working_q_size_f64_wide(m, n), tsqr_mi_working_r_size_f64_wide(m, n)); }
};

template <bool Reorthogonalize>
inline state_t qr_fp64_wide(
		double* const q_ptr, const std::size_t ldq,
		double* const r_ptr, const std::size_t ldr,
		double* const a_ptr, const std::size_t lda,
		const std::size_t m, const std::size_t n,
		buffer_fp64_wide<Reorthogonalize>& bf,
		handle_t const stream = nullptr,
		const layout_t a_layout = col_major, const layout_t q_layout = col_major) {
	const int st = tsqr_mi_qr_f64_wide_lay(a_layout, q_layout, Reorthogonalize ? 1 : 0, q_ptr, ldq, r_ptr, ldr, a_ptr, lda, m, n, bf.dwq, bf.dwr, stream);
	if (st < 0) throw std::runtime_error(std::string("mtk::qr::qr_fp64_wide: ") + tsqr_mi_last_error());
	return st;
}
// Not in the reference: qr_fp64_wide for a matrix whose rows are spread over the ranks of an RCCL communicator, one call per rank
// (tsqr_mi_qr_f64_dist, include/tsqr_mi.h for the contract): m is THIS rank's block height (1 <= m, m < n allowed), nccl_comm the
// caller's ncclComm_t -- the caller links RCCL, ncclAllReduce is taken from the global symbol scope.  R is the same on every rank.
// Returns success_factorization, error_invalid_matrix_size, error_unsupported_mode (n > 1024, or no ncclAllReduce) or error_not_finite.
template <bool Reorthogonalize>
struct buffer_fp64_dist : detail::buffer_fp64_base {
	void allocate(const std::size_t m_local, const std::size_t n, const int nranks) { allocate_doubles(tsqr_mi_working_q_size_f64_dist(m_local, n, nranks), tsqr_mi_working_r_size_f64_dist(m_local, n, nranks)); }
};

template <bool Reorthogonalize>
inline state_t qr_fp64_dist(
		double* const q_ptr, const std::size_t ldq,
		double* const r_ptr, const std::size_t ldr,
		double* const a_ptr, const std::size_t lda,
		const std::size_t m_local, const std::size_t n,
		buffer_fp64_dist<Reorthogonalize>& bf,
		void* const nccl_comm, const int nranks,
		handle_t const stream = nullptr) {
	const int st = tsqr_mi_qr_f64_dist(Reorthogonalize ? 1 : 0, q_ptr, ldq, r_ptr, ldr, a_ptr, lda, m_local, n, bf.dwq, bf.dwr, nccl_comm, nranks, stream);
	if (st < 0) throw std::runtime_error(std::string("mtk::qr::qr_fp64_dist: ") + tsqr_mi_last_error());
	return st;
}
}  // namespace qr
}  // namespace mtk

#endif /* end of include guard */

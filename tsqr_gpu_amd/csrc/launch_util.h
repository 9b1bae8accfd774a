// launch_util.h -- the pieces of host launch code that every schedule of tsqr_mi.hip and the test library share: the dispatch on the tile
// count NT, on an operand's layout and on the MFMA engine, the launch of gram_reduce1_kernel and the spin-then-poll wait on a pinned word.  ONE definition each,
// compiled into libtsqr_mi.so (tsqr_mi.hip) and into libtsqr_selftest.so (selftest.hip).  Nothing here knows the per-call context.
// Included after tsqr_kernels.hip (f64_plan.h includes it).  The including file defines fail(): what a function returns, through HIPCHK,
// when a HIP call did not succeed.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

namespace {

inline int fail(hipError_t e, const char* what);
#define HIPCHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(e_, #expr); } while (0)

// f(std::integral_constant<int, NT>{}) for NT = 1, 2, 3 and 4 (any other value: 4) -- the 16-column tiles of a panel of up to 64 columns
template <class F> inline auto with_nt(int NT, F&& f) {
	switch (NT) {
		case 1: return f(std::integral_constant<int, 1>{});
		case 2: return f(std::integral_constant<int, 2>{});
		case 3: return f(std::integral_constant<int, 3>{});
		default: return f(std::integral_constant<int, 4>{});
	}
}

// f(std::bool_constant<ROW>{}) for the layout of an operand: 0 column-major (false), any other value row-major (true)
template <class F> inline auto with_layout(int layout, F&& f) { return layout ? f(std::true_type{}) : f(std::false_type{}); }

// f(std::integral_constant<int, E>{}) for the MFMA engine of the apply pass: 0 fp32, 1 bf16x3 (any other value: 2, single fp16 product)
template <class F> inline auto with_engine(int engine, F&& f) {
	return engine == 0 ? f(std::integral_constant<int, 0>{})
	                   : (engine == 1 ? f(std::integral_constant<int, 1>{}) : f(std::integral_constant<int, 2>{}));
}

// gram_reduce1_kernel: the `nparts` partials of `nelem` doubles each -> gsum[0 .. nelem), the row count `rows` behind them
inline void launch_reduce1(hipStream_t st, double* gsum, const double* part, int nparts, int nelem, double rows) {
	hipLaunchKernelGGL(tsqrmi::gram_reduce1_kernel, dim3((nelem + 15) / 16), dim3(256), 0, st, gsum, part, nparts, nelem, rows,
	                   nullptr, (size_t)0, nullptr, 0);
}

// Spin on seen() -- a look at a pinned word the device writes -- and poll the stream now and then, so that a failed launch cannot hang
// the caller.  0: seen; 1: the stream went idle first (the caller reads its word once more); minus the HIP error otherwise.
template <class Seen> inline int spin_until(Seen seen, hipStream_t st) {
	for (;;) {
		for (int k = 0; k < 20000; k++) {
			if (seen()) return 0;
			__builtin_ia32_pause();
		}
		const hipError_t e = hipStreamQuery(st);
		if (e == hipSuccess) return 1;
		if (e != hipErrorNotReady) HIPCHK(e);
	}
}

}  // namespace

// f64_plan.h -- the host side that the fp64 entries (tsqr_mi_qr_f64, tsqr_mi_qr_f64_wide) share with the test library: the launch plans of
// the Gram and apply passes, the work-space offsets and the launch sequence of the blocked Cholesky step.  ONE definition, compiled into
// libtsqr_mi.so (tsqr_mi.hip) and into libtsqr_selftest.so (selftest.hip), so that the per-pass tests run the product's kernels with the
// product's plan and never a copy of it.  Included after tsqr_kernels.hip, tsqr_wide.hip, tsqr_f64.hip and tsqr_f64_wide.hip.
// HIPCHK and the dispatch on the tile count: launch_util.h.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstddef>
#include "launch_util.h"

namespace {

constexpr size_t PW = 64;          // panel width

inline size_t cdiv(size_t a, size_t b) { return (a + b - 1) / b; }
inline size_t np_of(size_t n) { return 16 * cdiv(std::min(n, PW), 16); }

constexpr size_t GSUM_DOUBLES = 16 * 256 + 8;          // 16 tiles (coupling) or 10 (Gram) + the row-count word of a row-partitioned run

// ---- tsqr_mi_qr_f64 (n <= 64) --------------------------------------------------------------------------------------------------------
constexpr int F64_GRAM_WAVES = 2048;                    // fixed (not tsqr_mi_set_tuning2): the work-space size must not follow a setting
// wq (doubles): [Z: 4096][R of the sweep: 4096][summed tiles + row count][status words: 4 slots x 4 words]
constexpr size_t F64_Z = 0, F64_R2 = 4096, F64_GSUM = 8192, F64_STATUS = F64_GSUM + GSUM_DOUBLES, F64_WQ = F64_STATUS + 8;

// The partition of a streaming pass over the m rows: nunits units of `unit_rows` rows dealt to nwaves waves (at most wave_cap, and no
// wave without a unit), four waves to a workgroup.  ntri: the tiles of a Gram partial.
struct F64Plan { int NT, ntri, nunits, nwaves, nblocks; };
inline F64Plan f64_plan_of(size_t m, size_t n, size_t unit_rows, int wave_cap) {
	F64Plan g{};
	g.NT = (int)(np_of(n) / 16);
	g.ntri = g.NT * (g.NT + 1) / 2;
	g.nunits = (int)cdiv(m, unit_rows);
	const size_t upw = std::max<size_t>(1, cdiv((size_t)g.nunits, (size_t)wave_cap));
	g.nwaves = (int)cdiv((size_t)g.nunits, upw);
	g.nblocks = (g.nwaves + 3) / 4;
	return g;
}
// the Gram pass (sweep 0 of every n <= 64 entry, every sweep of tsqr_mi_qr_f64): 64-row chunks
inline F64Plan f64_plan(size_t m, size_t n) { return f64_plan_of(m, n, 64, F64_GRAM_WAVES); }

// The acceptance rule of a sweep over an m x n matrix (CholArgs64, tsqr_f64.hip, states it and its sources): the bounds on S of a FIRST
// sweep (later sweeps: max_scond = infinity, never alone) and the coefficient of the shift, s = shift_coef * trace(G).  The arithmetic is
// f64_rule_of (tsqr_f64.hip), which the Cholesky kernels of a row-partitioned call evaluate themselves on the all-reduced row count.
using F64Rule = tsqrmi::F64Rule;
inline F64Rule f64_rule(size_t m, size_t n, bool first) { return tsqrmi::f64_rule_of((double)m, (int)n, first); }

// The launchers of the three passes that read A (and B) take a layout per operand: TSQR_MI_COL_MAJOR = 0, TSQR_MI_ROW_MAJOR = 1
// (include/tsqr_mi.h); ga.lda / la.lda / la.ldb are row strides for a row-major operand.  The plans, grids and partials do not depend on
// it; only the kernel's template flag does.

// the Gram pass of the n <= 64 entry on stream st: gram_f64_kernel<NT, AROW> on the plan's grid
inline void f64_gram_launch(hipStream_t st, const F64Plan& g, const tsqrmi::GramArgs64& ga, int a_layout = 0) {
	with_nt(g.NT, [&](auto nt) {
		with_layout(a_layout, [&](auto ar) {
			hipLaunchKernelGGL((tsqrmi::gram_f64_kernel<decltype(nt)::value, decltype(ar)::value>), dim3(g.nblocks), dim3(256), 0, st, ga);
		});
	});
}

// the apply pass of the n <= 64 entry runs on a persistent grid: the workgroups of the instantiation that is launched (AROW, QROW: the
// layouts of the operand read and of the operand written, tsqr_mi_qr_f64_lay) resident at once on device dev ...
template <int NT, bool AROW = false, bool QROW = false> int f64_apply_resident(int dev) {
	int nb = 0, cus = 0;
	if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void*>(&tsqrmi::apply_f64_kernel<NT, AROW, QROW>), 256, 0) != hipSuccess || nb < 1) {
		(void)hipGetLastError(); nb = 1;
	}
	if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) { (void)hipGetLastError(); cus = 256; }
	return nb * cus;
}
// ... but no more than one wave per 32-row block
inline size_t f64_apply_wgs(size_t nblocks, size_t resident) { return std::max<size_t>(1, std::min(cdiv(nblocks, 4), resident)); }
// f(nt, arow, qrow) for the instantiation apply_f64_kernel<NT, AROW, QROW> of n columns and the two layouts
template <class F> inline auto with_apply(size_t n, int a_layout, int q_layout, F&& f) {
	return with_nt((int)(np_of(n) / 16), [&](auto nt) {
		return with_layout(a_layout, [&](auto ar) { return with_layout(q_layout, [&](auto qr) { return f(nt, ar, qr); }); });
	});
}

// the two uses of trimul_f64_kernel on stream st, both in place: r (n x n, ldr) <- r2 r with r2 packed with ld 64 (the destination is the
// right factor), and z <- z zk, both NP x NP with ld NP (the destination is the left factor; the whole block is written)
inline void f64_rmul_launch(hipStream_t st, double* r, size_t ldr, const double* r2, int n) {
	hipLaunchKernelGGL(tsqrmi::trimul_f64_kernel, dim3(1), dim3(1024), 0, st, r, ldr, r2, (size_t)64, (const double*)r, ldr, n, n);
}
inline void f64r_zmul_launch(hipStream_t st, double* z, const double* zk, int n) {
	const size_t NP = np_of((size_t)n);
	hipLaunchKernelGGL(tsqrmi::trimul_f64_kernel, dim3(1), dim3(1024), 0, st, z, NP, (const double*)z, NP, zk, NP, n, (int)NP);
}

// ---- tsqr_mi_r_f64 (n <= 64, R only) ---------------------------------------------------------------------------------------------------
// Sweep 0 is the Gram pass above; sweeps k >= 1 run gramq_f64_kernel on 16-row tiles of A.  Like F64_GRAM_WAVES the wave count is a fixed
// function of (m, n) -- no occupancy query, no setting -- so that the reduction tree, the bits of R and the size of wr are the same everywhere.
constexpr int F64R_GRAMQ_WAVES = 2048;
// wq (doubles): [the F64_WQ layout (the sweep's Z, the sweep's R, summed tiles, status words)][Z_acc: the product of the inverses so far: 4096]
constexpr size_t F64R_ZACC = F64_WQ, F64R_WQ = F64R_ZACC + 4096;

inline F64Plan f64r_plan(size_t m, size_t n) { return f64_plan_of(m, n, 16, F64R_GRAMQ_WAVES); }   // 16-row tiles
// doubles of wr: the larger of the two Gram plans' partials
inline size_t f64r_wr_doubles(size_t m, size_t n) {
	const F64Plan g0 = f64_plan(m, n), g1 = f64r_plan(m, n);
	return (size_t)std::max(g0.nblocks, g1.nblocks) * g0.ntri * 256;
}

// the Gram pass of sweeps k >= 1 of the R-only entry on stream st: gramq_f64_kernel<NT, AROW> on the plan's grid
inline void f64r_gramq_launch(hipStream_t st, const F64Plan& g, const tsqrmi::GramQArgs64& ga, int a_layout = 0) {
	with_nt(g.NT, [&](auto nt) {
		with_layout(a_layout, [&](auto ar) {
			hipLaunchKernelGGL((tsqrmi::gramq_f64_kernel<decltype(nt)::value, decltype(ar)::value>), dim3(g.nblocks), dim3(256), 0, st, ga);
		});
	});
}

// ---- tsqr_mi_lstsq_f64 (n <= 64, nrhs <= 16) -------------------------------------------------------------------------------------------
// The ladder is the R-only entry's; every pass behind it runs lsq_f64_kernel on f64r_plan's grid, tiles and waves -- a fixed function of
// (m, n), the same for every nrhs -- so the reduction tree and the bits of X are the same everywhere.  A partial is NT tiles of 256 doubles,
// never more than the ntri tiles of a Gram partial: wr is the R-only entry's.
constexpr size_t F64L_MAX_NRHS = 16;
constexpr int F64L_MAX_REFINE = 4;
// wq (doubles): [the F64R_WQ layout][X, NP x 16 (ld NP): 1024][summed D: 4 tiles of 256 + the row-count word of the reduction]
// [max |D| of the pass before, one per right-hand side: the stagnation rule of lsq_update_f64_kernel: 16]
constexpr size_t F64L_X = F64R_WQ, F64L_D = F64L_X + 1024, F64L_DPREV = F64L_D + 1024 + 8, F64L_WQ = F64L_DPREV + 16;

// one pass of the least-squares entry on stream st: lsq_f64_kernel<NT, AROW, BROW> on the R-only plan's grid
inline void f64r_lsq_launch(hipStream_t st, const F64Plan& g, const tsqrmi::LsqArgs64& la, int a_layout = 0, int b_layout = 0) {
	with_nt(g.NT, [&](auto nt) {
		with_layout(a_layout, [&](auto ar) {
			with_layout(b_layout, [&](auto br) {
				hipLaunchKernelGGL((tsqrmi::lsq_f64_kernel<decltype(nt)::value, decltype(ar)::value, decltype(br)::value>), dim3(g.nblocks),
				                   dim3(256), 0, st, la);
			});
		});
	});
}

// X <- X + Z D on stream st, one workgroup.  ZDENSE clear: Z upper triangular, the least-squares entry -- the only form the library
// instantiates; set: a dense Z (lsq_rank_f64.hip, the test library)
template <bool ZDENSE = false>
inline void f64_lsq_update_launch(hipStream_t st, double* xw, double* x, size_t ldx, const double* z, const double* d, int n, int nrhs,
                                  int first, int last, double* dprev, int guard) {
	hipLaunchKernelGGL(tsqrmi::lsq_update_f64_kernel<ZDENSE>, dim3(1), dim3(1024), 0, st, xw, x, ldx, z, d, n, (int)np_of((size_t)n), nrhs,
	                   first, last, dprev, guard);
}

// ---- tsqr_mi_lstsq_rank_f64 (n <= 64, nrhs <= 16) --------------------------------------------------------------------------------------
// The ladder is the R-only entry's and the pivoted QR of its R0 is tsqr_mi_qrcp_f64's with jobq = 0; the dense Gram pass of the
// CholeskyQR step and every least-squares pass behind it run on f64r_plan's grid (lsq_rank_f64.hip has the kernels and their launchers).
// A partial is never more than the ntri tiles of a Gram partial: wr is the R-only entry's.
// wq (doubles): [the F64L_WQ layout][Zeff, NP x NP (ld NP): 4096][the step's summed Gram tiles: 10 tiles of 256 + the row-count word of
// the reduction][status words: [0] the rank, [1] the step's verdict: 8]
constexpr size_t F64K_ZEFF = F64L_WQ, F64K_G1 = F64K_ZEFF + 4096, F64K_STATUS = F64K_G1 + 10 * 256 + 8, F64K_WQ = F64K_STATUS + 8;
// tsqr_mi_lstsq_minnorm_f64: the same layout, status word [2] the verdict of lsq_minnorm_f64_kernel, and behind it
// [Zmn, NP x NP (ld NP): 4096].  Rc is not stored: that kernel repeats the step's factorisation on the same G11.
constexpr size_t F64M_ZMN = F64K_WQ, F64M_WQ = F64M_ZMN + 4096;

// ---- tsqr_mi_svd_f64 (n <= 64) ------------------------------------------------------------------------------------------------------------
// jobu = 1 runs the ladder of tsqr_mi_qr_f64_lay on the F64_WQ layout with R in the block behind it, then svd_r_f64_kernel and
// applyd_f64_kernel.  wq (doubles): [the F64_WQ layout][R, n x n with ld 64: 4096][W, NP x NP with ld NP: 4096][status words: 8]
constexpr size_t F64S_R = F64_WQ, F64S_W = F64S_R + 4096, F64S_STATUS = F64S_W + 4096, F64S_WQ = F64S_STATUS + 8;
constexpr size_t F64S_BLOCK = F64S_WQ - F64_WQ;         // what jobu = 1 adds to the QR entry's wq; wr is the QR entry's
// jobu = 0 runs the ladder of tsqr_mi_r_f64_lay on that entry's work space, unchanged in size (F64R_WQ, f64r_wr_doubles).

// svd_r_f64_kernel on stream st: one workgroup
inline void f64_svd_r_launch(hipStream_t st, const tsqrmi::SvdArgs64& sa) {
	hipLaunchKernelGGL(tsqrmi::svd_r_f64_kernel, dim3(1), dim3(1024), 0, st, sa);
}

// the workgroups of applyd_f64_kernel<NT, AROW, QROW> resident at once on device dev (f64_apply_resident for this kernel) ...
template <int NT, bool AROW = false, bool QROW = false> int f64_applyd_resident(int dev) {
	int nb = 0, cus = 0;
	if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void*>(&tsqrmi::applyd_f64_kernel<NT, AROW, QROW>), 256, 0) != hipSuccess || nb < 1) {
		(void)hipGetLastError(); nb = 1;
	}
	if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) { (void)hipGetLastError(); cus = 256; }
	return nb * cus;
}
// ... and the kernel on a grid of wgs workgroups (f64_apply_wgs of the 32-row blocks and the resident count): u = q w, in place allowed
template <int NT, bool AROW, bool QROW>
inline void f64_applyd_launch(hipStream_t st, size_t wgs, double* u, size_t ldu, const double* q, size_t ldq, size_t m, int n, const double* w) {
	hipLaunchKernelGGL((tsqrmi::applyd_f64_kernel<NT, AROW, QROW>), dim3((unsigned)wgs), dim3(256), 0, st, u, ldu, q, ldq, m, n, w, cdiv(m, 32));
}

// ---- tsqr_mi_qrcp_f64 (n <= 64) -----------------------------------------------------------------------------------------------------------
// jobq = 1 runs the ladder of tsqr_mi_qr_f64_lay on the F64_WQ layout with R0 in the caller's r, then qrcp_r_f64_kernel in place on r
// and applyd_f64_kernel.  wq (doubles): [the F64_WQ layout][H, NP x NP with ld NP: 4096][status words: 8]
constexpr size_t F64P_H = F64_WQ, F64P_STATUS = F64P_H + 4096, F64P_WQ = F64P_STATUS + 8;
constexpr size_t F64P_BLOCK = F64P_WQ - F64_WQ;         // what jobq = 1 adds to the QR entry's wq; wr is the QR entry's
// jobq = 0 runs the ladder of tsqr_mi_r_f64_lay on that entry's work space, unchanged in size (F64R_WQ, f64r_wr_doubles); H is not formed.

// qrcp_r_f64_kernel on stream st: one workgroup
inline void f64_qrcp_r_launch(hipStream_t st, const tsqrmi::QrcpArgs64& pa) {
	hipLaunchKernelGGL(tsqrmi::qrcp_r_f64_kernel, dim3(1), dim3(1024), 0, st, pa);
}

// ---- tsqr_mi_qr_f64_wide (64 < n <= 1024) ----------------------------------------------------------------------------------------------
constexpr size_t F64W_MAX_N = 1024;
constexpr size_t F64W_WR_CAP = size_t(8) << 20;         // doubles of Gram partials at most, for every m
constexpr int F64W_TARGET_WGS = 512;                    // two workgroups per CU

struct F64WPlan {
	int nb, npairs, ngroups, nslices;
	size_t cps, nch;                                     // 16-row chunks per slice, chunks
	size_t bs;                                           // doubles of one block store (npairs blocks)
	size_t o_gs, o_w, o_rw, o_zw, o_ta, o_rc, o_zd, o_sb, o_bst, o_status, wq;
};
F64WPlan f64w_plan(size_t m, size_t n) {
	F64WPlan g{};
	g.nb = (int)cdiv(n, PW);
	g.npairs = g.nb * (g.nb + 1) / 2;
	g.ngroups = (int)cdiv((size_t)g.npairs, 4);
	g.nch = cdiv(m, 16);
	const size_t cap = F64W_WR_CAP / ((size_t)g.npairs * 4096);
	const size_t want = std::max<size_t>(1, std::min({cdiv((size_t)F64W_TARGET_WGS, (size_t)g.ngroups), cap, g.nch}));
	g.cps = cdiv(g.nch, want);
	g.nslices = (int)cdiv(g.nch, g.cps);                 // (<= want)
	g.bs = (size_t)g.npairs * 4096;
	g.o_gs = 0;
	g.o_w = g.o_gs + g.bs + 64;                          // (the reduction writes the row count behind the summed blocks)
	g.o_rw = g.o_w + g.bs;
	g.o_zw = g.o_rw + g.bs;
	g.o_ta = g.o_zw + g.bs;
	g.o_rc = g.o_ta + g.bs;
	g.o_zd = g.o_rc + g.bs;
	g.o_sb = g.o_zd + (size_t)g.nb * 4096;
	g.o_bst = g.o_sb + (size_t)g.nb * (g.nb + 1);
	g.o_status = g.o_bst + (size_t)g.nb * 2;
	g.wq = g.o_status + 8;
	return g;
}

// the blocked Cholesky step of one sweep, plain (shift_coef = 0, run_if = nullptr) or shifted
int f64w_chain(hipStream_t st, tsqrmi::WideF64 wa) {
	const int nb = wa.nb;
	for (int k = 0; k < nb; k++) {
		hipLaunchKernelGGL(tsqrmi::cholw_diag_kernel, dim3(1), dim3(1024), 0, st, wa, k);
		HIPCHK(hipGetLastError());
		hipLaunchKernelGGL(tsqrmi::cholw_row_kernel, dim3(nb), dim3(1024), 0, st, wa, k);
		HIPCHK(hipGetLastError());
		const int nt = nb - k - 1;
		if (nt > 0) {
			hipLaunchKernelGGL(tsqrmi::cholw_update_kernel, dim3(nt * (nt + 1) / 2 + (k + 1) * nt), dim3(1024), 0, st, wa, k);
			HIPCHK(hipGetLastError());
		}
	}
	hipLaunchKernelGGL(tsqrmi::cholw_verdict_kernel, dim3(1), dim3(64), 0, st, wa);
	HIPCHK(hipGetLastError());
	return 0;
}

// The two passes of the wide entry that touch A or Q, on stream st.  a_layout, q_layout as for the n <= 64 launchers above (the leading
// dimension of a row-major operand is its row stride); the grids, the partition and the partials do not depend on them.
inline void f64w_gram_launch(hipStream_t st, const F64WPlan& g, const tsqrmi::GramWideF64Args& ga, int a_layout = 0) {
	with_layout(a_layout, [&](auto ar) {
		hipLaunchKernelGGL((tsqrmi::gram_wide_f64_kernel<decltype(ar)::value>), dim3((unsigned)(g.ngroups * g.nslices)), dim3(256), 0, st, ga);
	});
}
inline void f64w_apply_launch(hipStream_t st, double* q, size_t ldq, const double* a, size_t lda, size_t m, int n, int nb, const double* zw,
                              int a_layout = 0, int q_layout = 0) {
	with_layout(a_layout, [&](auto ar) {
		with_layout(q_layout, [&](auto qr) {
			hipLaunchKernelGGL((tsqrmi::apply_wide_f64_kernel<decltype(ar)::value, decltype(qr)::value>), dim3((unsigned)cdiv(m, 128)), dim3(256),
			                   0, st, q, ldq, a, lda, m, n, nb, zw);
		});
	});
}

}  // namespace

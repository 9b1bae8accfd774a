// f32_plan.h -- the host side that the fp32 engine (tsqr_mi.hip) shares with the test library: the plan of the 64-column Gram / coupling
// passes and the grouping of the coupling launches, the split of the 128-column Gram pass over its two kernel forms with its launch
// attributes and the wiring of the two-block Cholesky step, and the sizing of the apply family's persistent grid with the instance
// tables of the one-panel path, the coupling update and the half-typed path.  ONE
// definition, compiled into libtsqr_mi.so (tsqr_mi.hip) and into libtsqr_selftest.so (selftest.hip), so that the per-pass tests
// (selftest_f32.hip) run the product's kernels with the product's launch arithmetic and never a copy of it.  Host code only: nothing here
// is compiled for the device.  Included after tsqr_kernels.hip and tsqr_wide.hip; PW, cdiv: f64_plan.h; HIPCHK: launch_util.h.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cstddef>
#include <type_traits>
#include "f64_plan.h"
#include "launch_util.h"

namespace {

// ---- Gram engine geometry (n <= 64 per panel) and the coupling partials ---------------------------------------------------------------------
constexpr int GRAM_WAVES_DEFAULT = 2048;                // waves of a Gram / coupling pass unless tsqr_mi_set_tuning2 says otherwise
constexpr int BF16_SCOND_FLOOR_DEFAULT = 4;             // floor of the bf16-split level's bound on S unless TSQR_MI_BF16_MAX_SCOND says otherwise
// waves / workgroups of the Gram kernels and the size of their per-workgroup partials (in floats); gram_waves: the waves asked for
struct GramPlan { int nch, cpw, nwaves, nblocks, ntri; size_t part_floats; };
inline GramPlan gram_plan_of(size_t m, size_t n, int gram_waves) {
	GramPlan g{};
	const size_t NT = np_of(n) / 16;
	g.nch = (int)cdiv(m, 64);
	g.cpw = (int)std::max<size_t>(1, cdiv((size_t)g.nch, (size_t)std::max(1, gram_waves)));
	g.nwaves = (int)cdiv((size_t)g.nch, (size_t)g.cpw);
	g.nblocks = (g.nwaves + 3) / 4;
	g.ntri = (int)(NT * (NT + 1) / 2);
	g.part_floats = (size_t)g.nblocks * g.ntri * 256 * 2;
	return g;
}
// Coupling partials (cross_kernel: 16 tiles x 256 doubles per workgroup).  A launch covers as many trailing panels as the work space holds
// workgroup partials for -- every panel with the full workgroup count of one panel pair, so the grouping of the sums (and with it every bit
// of S) is that of rounds 1-3: up to CROSS_SLOT_CAP slots (32 MiB), never fewer than one panel's.
constexpr size_t CROSS_SLOT_CAP = 1024;
constexpr size_t CROSS_PART_DOUBLES = 16 * 256;         // one workgroup's partial
inline size_t cross_slots_of(size_t n, int nblocks) {
	if (n <= PW) return 0;
	const size_t nb = (size_t)nblocks, ntr = cdiv(n, PW) - 1;
	return std::max(nb, std::min(ntr * nb, CROSS_SLOT_CAP));
}
// trailing panels one coupling launch covers when the work space holds `slots` workgroup partials
inline size_t cross_group(size_t slots, int nblocks) { return std::max<size_t>(1, slots / (size_t)nblocks); }

// One group of the coupling of a finished panel X (m x 64) with the trailing matrix Y (m x ntc, first column at y): S_j = X^T Y_j for the gy
// trailing panels from panel j0 on -- cross_kernel on grid (nblocks, gy), then cross_reduce_multi_kernel into gm + j0 * CROSS_GSTRIDE.  fin
// (one GPU): the reduction also writes the block row of R (rblk: rows of X, columns of Y) and the operands -S_j (sm + j * 4096); otherwise
// the sums only (row-partitioned: cross_finish_kernel follows the all-reduce).
inline void cross_group_launch(hipStream_t st, const GramPlan& g, const float* x, size_t ldx, const float* y, size_t ldy, size_t m, size_t ntc,
                               size_t j0, unsigned gy, double* part, double* gm, bool fin, float* rblk, size_t ldr, float* sm) {
	const int cols = (int)(ntc - PW * j0);               // columns from trailing panel j0 on
	tsqrmi::CrossArgs ca{};
	ca.x = x; ca.ldx = ldx; ca.y = y + PW * j0 * ldy; ca.ldy = ldy; ca.m = m; ca.ny = std::min((int)PW, cols); ca.ny_total = cols;
	ca.nchunks = g.nch; ca.cpw = g.cpw; ca.nwaves = g.nwaves; ca.part = part;
	hipLaunchKernelGGL(tsqrmi::cross_kernel, dim3(g.nblocks, gy), dim3(256), 0, st, ca);
	hipLaunchKernelGGL(tsqrmi::cross_reduce_multi_kernel, dim3(256, gy), dim3(256), 0, st, gm + j0 * (size_t)tsqrmi::CROSS_GSTRIDE, ca.part, g.nblocks,
	                   (double)m, fin ? rblk + j0 * PW * ldr : (float*)nullptr, ldr, fin ? sm + j0 * 4096 : (float*)nullptr, cols);
}
// ... and the finish of the row-partitioned form for all ntr = ceil(ntc / 64) trailing panels at once
inline void cross_finish_launch(hipStream_t st, float* rblk, size_t ldr, float* sm, const double* gm, size_t ntc) {
	hipLaunchKernelGGL(tsqrmi::cross_finish_kernel, dim3(16, (unsigned)cdiv(ntc, PW)), dim3(256), 0, st, rblk, ldr, sm, gm, 0, (int)ntc);
}

// ---- gram_wide_kernel (64 < n <= 128) ---------------------------------------------------------------------------------------------------
constexpr int WIDE_MAX_WGS = 255;                       // gram_wide_kernel: one eight-wave workgroup per CU -- on 255 of the 256 CUs: in a stream of calls the
                                                        // last CU holds the factorisation of the call before (gram_wide_chain_kernel), and the partials must
                                                        // be those of the blocking call
constexpr int WIDE_NELEM = 36 * 256;                    // doubles of one workgroup's partial, and of the summed tiles
inline size_t wide_part_floats(size_t m) { return (std::min<size_t>((m + 63) / 64, WIDE_MAX_WGS) + 1) * WIDE_NELEM * 2; }

// full 64-row blocks of a 128-column matrix go to the fast form of the Gram kernel, whatever is left (ragged last rows, or the whole
// matrix when n < 128) to the general form; both write per-workgroup partials, one after the other (the fast form's first)
struct WideGramPlan { size_t nfull, nrest; int wgs_fast, wgs_rest; };
inline WideGramPlan wide_gram_plan(size_t m, size_t n, size_t lda) {
	WideGramPlan p{};
	p.nfull = (n == 2 * PW && lda <= ((size_t)1 << 23)) ? m / 64 : 0;   // (fast form: 32-bit buffer offsets)
	p.nrest = cdiv(m, 64) - p.nfull;
	p.wgs_fast = (int)std::min<size_t>(p.nfull, WIDE_MAX_WGS);
	p.wgs_rest = (int)std::min<size_t>(p.nrest, WIDE_MAX_WGS);
	return p;
}

// the dynamic-LDS sizes of the 128-column Gram kernel in its fast, general and chained forms (once per device)
inline int wide_gram_attrs() {
	HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&tsqrmi::gram_wide_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, tsqrmi::GW_LDS_BYTES));
	HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&tsqrmi::gram_wide_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, tsqrmi::GW_LDS_BYTES));
	HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&tsqrmi::gram_wide_chain_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, tsqrmi::GWC_LDS_BYTES));
	return 0;
}
// chol_wide_kernel's arguments apart from the verdict words: summed tiles, R, the fp32 Z11 / Z22 scratch (4096 floats each), the 128 x 128
// Z, the two blocks' own verdict words (16 words each), the row count and the floor of the bound on S
constexpr size_t WIDE_CHOL_SCRATCH_FLOATS = 2 * 4096 + 2 * 16;     // Z11, Z22, st1, st2 when they sit in one buffer (the test library)
inline tsqrmi::CholWideArgs chol_wide_wiring(const double* gsum, float* r, size_t ldr, size_t m, size_t n, float* zf1, float* zf2, float* zw,
                                             unsigned* st1, unsigned* st2, float scond_floor) {
	tsqrmi::CholWideArgs wa{};
	wa.gsum = gsum; wa.r = r; wa.ldr = ldr; wa.n = (int)n; wa.zf1 = zf1; wa.zf2 = zf2; wa.zw = zw; wa.st1 = st1; wa.st2 = st2;
	wa.rows = (double)m; wa.scond_floor = scond_floor;
	return wa;
}

// ---- the apply family ---------------------------------------------------------------------------------------------------------------------
// The persistent grid of an apply instance (G: its tsqrmi::ApplyGeom): as many workgroups as are resident on the 256 CUs at once, per_cu
// per CU -- or grid.wgs of them --, split over grid.gy panels and never more than grid.max_wgs; a.nchunks = row blocks of G::ROWS,
// a.nwaves = workgroups.
struct ApplyGrid { int wgs = 0; unsigned gy = 1; int max_wgs = INT_MAX; };
template <class G> inline void apply_grid_fill(tsqrmi::ApplyArgs& a, const ApplyGrid& grid, int per_cu) {
	const size_t nblk = cdiv(a.m, (size_t)G::ROWS);
	const size_t want = grid.wgs > 0 ? (size_t)grid.wgs : (size_t)256 * per_cu;
	a.nchunks = (int)nblk;
	a.nwaves = std::min((int)std::min<size_t>(nblk, std::max<size_t>(1, want / grid.gy)), grid.max_wgs);   // (the resident workgroups split over the trailing panels)
	a.cpw = 0;
}
// What an instance needs once per device before its first launch: the dynamic-LDS attribute, and the workgroups per CU -- CAP at the
// most (QUERY: and no more than the runtime's occupancy figure) -> *per_cu
template <auto KERNEL, class G, bool GRAMQ, int CAP, bool QUERY> int apply_instance_setup(int* per_cu) {
	constexpr size_t lds = G::lds_bytes(GRAMQ);
	HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
	int nb = CAP;
	if constexpr (QUERY) {
		if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void*>(KERNEL), G::THREADS, lds) != hipSuccess || nb < 1) {
			(void)hipGetLastError(); nb = 2;
		}
	}
	*per_cu = std::min(nb, CAP);
	return 0;
}

// apply_wg_kernel / apply_wg_h_kernel instances: the block height per engine (measured, profiles/r02_experiment_log.md: the bf16x3 engine
// streams best with 64-row blocks, four workgroups per CU and two blocks in flight; the exact-fp32 and fp16 engines and the coupling
// update use 128-row blocks) and the workgroups per CU at the most (LDS / register bound; the fp32-MFMA engine is slower with three)
template <int E, bool UPD> constexpr int apply_wg_rows() { return (!UPD && E == 1) ? 64 : 128; }
template <int E, int ROWS> constexpr int apply_wg_cap() { return ROWS == 64 ? 4 : (E == 0 ? 2 : 3); }
// the coupling update as sweep launches it: Y_j <- Y_j + X (-S_j) for every trailing panel j, one grid row per panel
template <int E> struct UpdApply {
	static constexpr int ROWS = apply_wg_rows<E, true>();
	using G = tsqrmi::ApplyGeom<E, 4, true, ROWS>;
	static constexpr int CAP = apply_wg_cap<E, ROWS>();
	static constexpr bool QUERY = true;
	static constexpr auto kernel() { return &tsqrmi::apply_wg_kernel<E, 4, true, ROWS>; }
	static unsigned gy(int multi_cols) { return multi_cols > 0 ? (unsigned)cdiv((size_t)multi_cols, PW) : 1u; }
};
// fp16 I/O modes: the plain product with halves at both ends -- bf16x3 engine 1 (fp16_notc) or single-fp16-product engine 2
// (fp16_tc_nocor); 64- / 128-row blocks as in the fp32 call (measured: the bf16x3 engine at 128-row blocks 90 us against 59 at 64)
template <int E, int NT> struct HalfApply {
	static constexpr int ROWS = apply_wg_rows<E, false>();
	using G = tsqrmi::ApplyGeom<E, NT, false, ROWS>;
	static constexpr int CAP = apply_wg_cap<E, ROWS>();
	static constexpr bool QUERY = true;
	static constexpr auto kernel() { return &tsqrmi::apply_wg_h_kernel<E, NT, ROWS>; }
};

// The instances of the one-panel path (64 < n <= 128).  bf16x3 / fp16 engines: eight waves on 128-row blocks, one workgroup per CU;
// fp32-MFMA engine: four waves on 64-row blocks with the compact triangular Z (40 KiB), two workgroups per CU (fixed: the occupancy is
// not asked for)
template <int E> struct WideApply {
	using G = std::conditional_t<E == 0, tsqrmi::ApplyGeom<0, 8, false, 64, 4>, tsqrmi::ApplyGeom<E, 8, false, 128, 8>>;
	static constexpr int CAP = (E == 0) ? 2 : 1;
	static constexpr bool QUERY = false;
	static constexpr auto kernel() {
		if constexpr (E == 0) return &tsqrmi::apply_wide_f32_kernel;
		else return &tsqrmi::apply_wide_kernel<E>;
	}
};

}  // namespace

// tsqr_mi.hip -- host orchestration and the extern "C" ABI of libtsqr_mi.so (declared in include/tsqr_mi.h).
//
// Host-side counterpart of the reference's block_qr_core / block_qr_reorthogonalization_core
// (reference src/blockqr.cu:45-178, 180-390) and tsqr16_geq32 (reference src/tsqr.cu:1064-1279),
// re-designed for MI355X:
//   * panel width 64 instead of 16: for n <= 64 there is no inter-panel coupling at all;
//   * R from the Gram matrix of the panel (bf16x3-split MFMA, then fp64 MFMA, then shifted Cholesky QR) with a streaming
//     Householder TSQR (fold_kernel + fold tree over the per-wave R factors: the R-stack reduction of the reference) as the
//     engine of last resort / on request;
//   * Q = A * inverse(R) on the MFMA units (apply_wg_kernel): "indirect TSQR".  Its loss of orthogonality grows like
//     cond(A)*eps, slower than the reference's 16-wide block Gram-Schmidt without reorthogonalisation; Reorthogonalize=true runs
//     a second sweep on Q (R <- R2*R), which restores ||Q^T Q - I|| to O(eps) as the reference's BCGS2 does;
//   * the same ladder serves a row-partitioned matrix (one rank per GPU): the only exchange is an all-reduce of the n x n Gram
//     tiles (+ the row count) or, for the Householder engine, an all-gather of the local R factors;
//   * no host synchronisation inside a sweep; the call is blocking like the reference's (src/blockqr.cu:140).
//
// Re-entrancy: like the reference's entry point (src/blockqr.cu:394-433) a call keeps no state outside its arguments: everything
// a call needs lives in a Ctx on the caller's stack, settings are process-wide atomics that a call snapshots once, per-device
// launch attributes are cached in lock-free tables, diagnostics (last error / last engine / event profile) are per host thread.
// Two host threads may factor different matrices with different buffers and streams at the same time.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <string>
#include <vector>

#include "../../include/tsqr_mi.h"
#include "stream_order.h"
#include "tsqr_kernels.hip"
#include "tsqr_wide.hip"
#include "tsqr_f64.hip"
#include "tsqr_f64_wide.hip"
#include "f64_plan.h"
#include "lsq_rank_f64.hip"
#include "orth_f64.hip"
#include "f32_plan.h"
#include "launch_util.h"
#include "validate.hip"

namespace {

// ---------------------------------------------------------------------------------------------------------------------------
// process-wide settings (atomics: written by the tsqr_mi_set_* calls, snapshotted once per call) and per-thread diagnostics
// ---------------------------------------------------------------------------------------------------------------------------
int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
int clamp_load_policy(int p) { return (p == 1 || p == 2) ? p : 0; }

struct Settings {
	std::atomic<int> policy{0};          // 0 auto, 1 Householder, 2 Gram without check/fallback
	std::atomic<int> gram_level{2};      // first Gram level tried: 2 bf16-split (then fp64), 1 fp64 only
	std::atomic<int> level0_waves{2048}, tree_cpw{4}, gram_waves{GRAM_WAVES_DEFAULT};
	std::atomic<int> wide{1};            // 64 < n <= 128: one Cholesky-QR panel of up to 128 columns first (policy 5 turns it off)
	std::atomic<int> apply_wgs{0};       // workgroups of the apply pass; 0: as many as are resident at once (tsqr_mi_set_tuning2)
	std::atomic<int> loop_depth{3};      // *_loop entries: 1 blocking calls, 2 two calls in flight, 3 also the chained schedule (tsqr_mi_set_loop_depth)
	std::atomic<int> load_policy{clamp_load_policy(env_int("TSQR_MI_LOAD_POLICY", 0))};   // loads of A in gram_blk_kernel and the plain 64-row apply kernel:
	                                     // 0 auto (measured once, measure_load_policy), 1 cache-allocating, 2 streamed (tsqr_mi_set_load_policy)
	// the two environment switches that are left (read once at load): the floor of the bf16-split level's bound on the scaled
	// conditioning S, and a diagnostic print of every Cholesky verdict
	const float bf16_scond_floor = (float)env_int("TSQR_MI_BF16_MAX_SCOND", BF16_SCOND_FLOOR_DEFAULT);
	// chained schedules over DIFFERENT matrices: taken when one matrix is at most this many MiB.  The Gram pass of matrix i + 1 runs
	// between the Gram pass and the apply pass of matrix i; both fit the 256 MiB Infinity Cache only up to ~half of it each -- beyond
	// that the apply pass of matrix i finds its A evicted and streams it from HBM again (measured at 2^20 x 64, 256 MiB a matrix:
	// 0.181 ms per call chained against 0.163 in stream order, profiles/r04_experiment_log.md).  A loop over ONE matrix is not affected.
	const int chain_max_mib = env_int("TSQR_MI_CHAIN_MAX_MIB", 112);
	const int debug = env_int("TSQR_MI_DEBUG", 0);
};
Settings g_set;
std::atomic<int> g_load_policy_used{0};                // what the last call that took gram_blk_kernel used (1 / 2; 0: no such call yet)
std::atomic<unsigned> g_seq{0};                        // sequence numbers of the completion flags (any thread)

thread_local std::string t_last_error;
thread_local int t_last_engine = 0;   // 0 Householder TSQR, 1 fp64 Gram/Cholesky, 2 Gram broke down -> Householder, 3 bf16-split Gram, 4 shifted

// ---- optional per-kernel-class timing with HIP events on the caller's stream (bench.py's roofline leg); per host thread ----
enum { KC_FOLD0 = 0, KC_TREE = 1, KC_TRINV = 2, KC_APPLY = 3, KC_COUPLE = 4, KC_MISC = 5, KC_GRAM = 6, KC_CHOL = 7, KC_COUNT = 8 };
struct Prof {
	bool on = false;
	static constexpr int MAXEV = 4096;
	hipEvent_t ev[2 * MAXEV];
	int cls[MAXEV];
	int n = 0;
	bool created = false;
	double ms[KC_COUNT] = {};
	long launches[KC_COUNT] = {};
};
thread_local Prof t_prof;
struct ProfScope {                 // brackets one kernel launch (or a short launch group) with two events
	int idx = -1; hipStream_t st;
	ProfScope(int kc, hipStream_t s) : st(s) {
		if (t_prof.on && t_prof.n < Prof::MAXEV) {
			idx = t_prof.n++;
			t_prof.cls[idx] = kc;
			(void)hipEventRecord(t_prof.ev[2 * idx], st);
		}
	}
	~ProfScope() { if (idx >= 0) (void)hipEventRecord(t_prof.ev[2 * idx + 1], st); }
};
void prof_collect() {              // after the stream is idle
	for (int i = 0; i < t_prof.n; i++) {
		float t = 0.0f;
		if (hipEventElapsedTime(&t, t_prof.ev[2 * i], t_prof.ev[2 * i + 1]) == hipSuccess) {
			t_prof.ms[t_prof.cls[i]] += t;
			t_prof.launches[t_prof.cls[i]] += 1;
		}
	}
	t_prof.n = 0;
}

constexpr int MAX_DEV = 64;

// (PW, cdiv, np_of and GSUM_DOUBLES: f64_plan.h; HIPCHK: launch_util.h -- both shared with the test library)
inline int fail(hipError_t e, const char* what) {
	t_last_error = std::string(what) + ": " + hipGetErrorString(e);
	return -(int)e;
}

inline int cur_device() { int d = 0; (void)hipGetDevice(&d); return (d >= 0 && d < MAX_DEV) ? d : 0; }

// per-kernel, per-device launch attributes: hipFuncSetAttribute once per (kernel instance, device); lock-free (the call is idempotent)
struct DevOnce {
	std::atomic<unsigned long long> mask{0};
	bool need(int dev) const { return !(mask.load(std::memory_order_acquire) >> dev & 1ull); }
	void done(int dev) { mask.fetch_or(1ull << dev, std::memory_order_release); }
};

// The dynamic-LDS sizes of the two Gram kernel families, set once per device for every schedule that launches one of them -- the blocking
// call as well as the chained streams (the test library, libtsqr_selftest.so, sets them itself before each of its launches: it is a
// separate shared object without this table).  The 64-column block kernel and its chained form ...
int blk_kernel_attrs(int dev) {
	static DevOnce attr;
	if (attr.need(dev)) {
		HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&tsqrmi::gram_blk_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, tsqrmi::GB_LDS_BYTES));
		HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&tsqrmi::gram_blk_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, tsqrmi::GB_LDS_BYTES));
		HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&tsqrmi::gram_blk_chain_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, tsqrmi::GB_LDS_BYTES));
		attr.done(dev);
	}
	return 0;
}
// ... and the 128-column kernel in its fast, general and chained forms
int wide_kernel_attrs(int dev) {
	static DevOnce attr;
	if (attr.need(dev)) {
		const int rc = wide_gram_attrs();                // (f32_plan.h)
		if (rc) return rc;
		attr.done(dev);
	}
	return 0;
}

// ---- reference-compatible size rules (reference src/tsqr.cu:39-60, src/blockqr.cu:34-42) ----
size_t ref_bs_log2(size_t m) {
	const unsigned c = (unsigned)std::ceil(std::log2((float)m));
	return (size_t)(std::max(5u, c) - 5u);
}
size_t ref_bs(size_t m) { return (size_t)1 << ref_bs_log2(m); }
size_t ref_wq(size_t m, size_t n) { n = std::min<size_t>(16, n); return n * m + 2 * n * n * (ref_bs(m) - 1); }
size_t ref_wr(size_t m, size_t n) { n = std::min<size_t>(16, n); const size_t b = ref_bs(m); return n * n * b + n * n * b / 2; }

// ---- fold plan: level 0 over the matrix, then levels over the stacks of per-wave R factors ----
struct Plan {
	size_t NP;
	int nlevels;
	size_t rows[24];     // source rows of each level
	int nch[24], cpw[24], nw[24];
	size_t stack_a;      // floats needed in wr (levels 0, 2, 4, ... write here)
	size_t stack_b;      // floats needed in wq (levels 1, 3, ... write here)
};

Plan make_plan(size_t m, size_t n) {
	Plan p{};
	p.NP = np_of(n);
	const int level0_waves = g_set.level0_waves.load(), tree_cpw = g_set.tree_cpw.load();
	size_t rows = m;
	int lv = 0;
	// a wave turns cpw*64 source rows into NP rows: cpw*64 >= 2*NP keeps every level shrinking
	const size_t cpw_min = std::max<size_t>(1, cdiv(2 * p.NP, 64));
	for (;;) {
		const size_t nch = cdiv(rows, 64);
		// tree levels over 64-row triangular blocks are binary: the first block is copied into R (FoldArgs::tri_init), one fold per level
		size_t cpw = (lv == 0) ? std::max(cpw_min, cdiv(nch, (size_t)level0_waves))
		                       : (p.NP == 64 ? (size_t)2 : std::max(cpw_min, (size_t)tree_cpw));
		size_t nw = cdiv(nch, cpw);
		if (nw <= 1 || nw * p.NP >= rows) { nw = 1; cpw = nch; }
		p.rows[lv] = rows; p.nch[lv] = (int)nch; p.cpw[lv] = (int)cpw; p.nw[lv] = (int)nw;
		if (nw > 1) {
			const size_t sz = nw * p.NP * p.NP;
			if (lv % 2 == 0) p.stack_a = std::max(p.stack_a, sz); else p.stack_b = std::max(p.stack_b, sz);
		}
		lv++;
		if (nw == 1) break;
		rows = nw * p.NP;
	}
	p.nlevels = lv;
	return p;
}

// Gram engine geometry and the coupling partials (GramPlan, gram_plan_of, cross_slots_of, cross_group: f32_plan.h -- shared with the test
// library), with the process's setting of the wave count
GramPlan gram_plan(size_t m, size_t n) { return gram_plan_of(m, n, g_set.gram_waves.load()); }
size_t cross_slots(size_t m, size_t n) { return cross_slots_of(n, gram_plan(m, PW).nblocks); }
// extra work space of the one-panel path for 64 < n <= 128 (offsets in floats from WqLayout::wide; the doubles first, 16-byte aligned):
// [summed tiles 36*256 + row count (+pad)] | [Z 128 x 128 fp32][Z22 fp32 4096]
constexpr size_t WIDE_G_DOUBLES = 36 * 256 + 8;
constexpr size_t WIDE_OFF_ZW = 2 * WIDE_G_DOUBLES, WIDE_OFF_ZF2 = WIDE_OFF_ZW + 128 * 128, WIDE_FLOATS = WIDE_OFF_ZF2 + 4096;
// (WIDE_MAX_WGS, wide_part_floats and the split of the Gram pass over its two kernel forms: f32_plan.h -- shared with the test library)

// layout of wq (floats): [stack_b][Z: 4096][S: 4096][R1 copy: n*n][R2: n*n][r3, r4, r5, r6: 4096 each][summed tiles + row count][status]
// (the summed tiles + row count take GSUM_DOUBLES: f64_plan.h)
struct WqLayout { size_t z, s, r1, r2, r3, r4, r5, r6, gsum, status, wide, smulti, gmulti, total; };
WqLayout wq_layout(size_t m, size_t n) {
	const Plan p = make_plan(m, n);
	WqLayout L{};
	size_t o = p.stack_b;
	o = (o + 63) & ~(size_t)63;
	L.z = o; o += 4096;
	L.s = o; o += 4096;
	L.r1 = o; o += n * n;
	L.r2 = o; o += n * n;
	L.r3 = o; o += 4096;                                 // panel-local R1, R2 of the shifted-Cholesky two-step (<= 64 x 64 each)
	L.r4 = o; o += 4096;
	L.r5 = o; o += 4096;                                 // third sweep's factor and R2 R1 of the shifted CholeskyQR3 of a reorthogonalised call (qr_core)
	L.r6 = o; o += 4096;
	o = (o + 63) & ~(size_t)63;
	L.gsum = o; o += 2 * GSUM_DOUBLES;
	L.status = o; o += 64;
	L.wide = o;
	if (n > PW) o += WIDE_FLOATS;                        // the one-panel path for 64 < n <= 128 (sweep_wide); n > 128: 128-column blocks of the panel loop (sweep)
	// several 64-column panels (round 4, right-looking coupling): the operands -S_j of the update and the summed coupling tiles of ALL trailing
	// panels of a finished panel (one slice of 4096 floats / CROSS_GSTRIDE doubles per trailing panel)
	o = (o + 63) & ~(size_t)63;
	L.smulti = o; L.gmulti = o;
	if (n > PW) {
		const size_t ntr = cdiv(n, PW) - 1;
		o += ntr * 4096;
		L.gmulti = o; o += ntr * 2 * (size_t)tsqrmi::CROSS_GSTRIDE;
	}
	L.total = o;
	return L;
}

// ---------------------------------------------------------------------------------------------------------------------------
// exchange hooks of a row-partitioned call (one rank per GPU).  Either RCCL entry points (resolved with dlopen) on the caller's
// ncclComm_t and stream, or caller-supplied callbacks (tests: torch.distributed over gloo on one GPU).
// ---------------------------------------------------------------------------------------------------------------------------
typedef int (*nccl_allgather_t)(const void*, void*, size_t, int, void*, hipStream_t);
typedef int (*nccl_allreduce_t)(const void*, void*, size_t, int, int, void*, hipStream_t);
struct Comm {
	int nranks = 1;
	void* nccl = nullptr;                                // ncclComm_t
	nccl_allreduce_t nccl_allreduce = nullptr;
	nccl_allgather_t nccl_allgather = nullptr;
	tsqr_mi_allreduce_f64_cb cb_allreduce = nullptr;
	tsqr_mi_allgather_f32_cb cb_allgather = nullptr;
	void* cb_user = nullptr;
	float* gather_buf = nullptr;                         // nranks * n * n floats (Householder engine only)
	bool active() const { return nccl != nullptr || cb_allreduce != nullptr; }
	int allreduce_f64(double* buf, size_t count, hipStream_t st) const {
		if (nccl_allreduce) return nccl_allreduce(buf, buf, count, 8 /* ncclFloat64 */, 0 /* ncclSum */, nccl, st) == 0 ? 0 : -1;
		if (cb_allreduce) return cb_allreduce(cb_user, buf, count, st) == 0 ? 0 : -1;
		return 0;
	}
	int allgather_f32(const float* send, float* recv, size_t count, hipStream_t st) const {
		if (nccl_allgather) return nccl_allgather(send, recv, count, 7 /* ncclFloat32 */, nccl, st) == 0 ? 0 : -1;
		if (cb_allgather) return cb_allgather(cb_user, send, recv, count, st) == 0 ? 0 : -1;
		return -1;
	}
};
// ncclAllReduce / ncclAllGather of a caller that LINKS RCCL itself (C++): the symbols are then in the global scope and this lookup
// returns the very copy the caller created its communicator with.  No soname search and no dlopen: a second RCCL instance (torch
// bundles one, /opt/rocm has another) must never meet a communicator of the first.  Callers that loaded RCCL privately (Python
// ctypes: RTLD_LOCAL) pass the entry points of that very handle instead (tsqr_mi_qr_f32_dist_fn).
void* rccl_symbol(const char* name) { return dlsym(RTLD_DEFAULT, name); }

// ---------------------------------------------------------------------------------------------------------------------------
// per-call context
// ---------------------------------------------------------------------------------------------------------------------------
struct HostSig { unsigned* host = nullptr; unsigned* dev = nullptr; };
// What ONE sweep is told (Ctx: what holds for the whole call).  Built where the sweep is enqueued and handed down by reference; nothing
// below writes to it.  The stream schedules and the staged entry points, which enqueue the launches of a sweep themselves, say {slot}.
struct SweepOpts {
	int slot = 0, prev_slot = -1;                        // status slot its verdicts go to / of the sweep it depends on (-1: none; rejected there: this one skips itself)
	int gramq_ready = 0;                                 // > 0: so many partials of this sweep's bf16-level Gram matrix are in place already (the pass is skipped)
	double* gramq_part = nullptr; int gramq_cap = 0;     // non-null: the apply launch writes per-workgroup Gram partials of its output there, gramq_cap at the most
	int relax = 0;                                       // bf16-level Cholesky launches use the relaxed rule (CholArgs::relax: another sweep follows)
	int retry_shift = 0;                                 // ... and factor a rejected matrix again at once, shifted (CholArgs::retry_shift)
	bool q_read_back = false;                            // Q is read back at once by the next sweep: plain stores, ascending block order (ApplyArgs::plain_q / forward)
	int load_policy = 0;                                 // loads of A in the panel's two passes: 1 cache-allocating, 2 streamed, 0: panel_qr resolves it (resolve_load_policy)
};
struct Ctx {
	hipStream_t st = nullptr;
	int dev = 0;
	float* wq = nullptr; float* wr = nullptr;
	WqLayout L{};
	size_t cross_slots = 0;                              // workgroup partials of the coupling launches the work buffer wr holds (cross_slots())
	HostSig hsig;                                        // pinned words the device can write: status words [0..2] / [4..6], completion flag [3]
	int policy = 0, gram_level = 2;
	int min_level = 2;                                   // lowest R-factor engine level used (2 bf16 Gram, 1 fp64 Gram, 0 Householder)
	bool used_shift = false, used_householder = false;
	bool wide = true;                                    // 64 < n <= 128: try the one-panel path first
	Comm comm;
	bool fold_cor = false;                               // Householder engine: block reflectors on the error-corrected bf16x3 MFMA (fp32_tc_cor)
	bool resume_accepted = false;                        // tsqr_mi_qr_f32_finish: the first attempt ran already and was accepted with
	float resume_scond = 0.0f;                           // this scaled conditioning (only the n <= 16 second sweep is left to do)
	int start_level = -1;                                // tsqr_mi_qr_f32_finish: the ladder resumes at this level (the ones above were rejected)
	unsigned* announce_word = nullptr;                   // completion word of the call in front of this one, raised by this call's first
	unsigned announce_seq = 0;                           // Gram kernel (consumed by the launch that carries it)
	double rows_global = 0.0;                            // host's view of the global row count (the device thresholds of a row-partitioned
	                                                     // call use the all-reduced count instead)
	unsigned* status_dev(int s) const { return reinterpret_cast<unsigned*>(wq + L.status) + 16 * s; }
	double* gsum() const { return reinterpret_cast<double*>(wq + L.gsum); }
};
// the pending announcement (Ctx::announce_word) rides in the Gram launch these arguments are for ...
template <class GramArgsT> void carry_announcement(Ctx& c, GramArgsT& ga) {
	ga.announce = c.announce_word; ga.announce_seq = c.announce_seq; c.announce_word = nullptr;
}
// ... or, where no Gram launch is left to carry it, in a one-thread kernel of its own
void raise_announcement(Ctx& c) {
	if (!c.announce_word) return;
	hipLaunchKernelGGL(tsqrmi::host_flag_kernel, dim3(1), dim3(1), 0, c.st, c.announce_word, c.announce_seq);
	c.announce_word = nullptr;
}

// library-owned pinned words, one set per host thread (callers whose h_wl is not pinned or too small; staged API)
struct OwnPinned {
	unsigned* host = nullptr; unsigned* dev = nullptr;
	~OwnPinned() { if (host) (void)hipHostFree(host); }
	bool get() {
		if (host) return dev != nullptr;
		if (hipHostMalloc(reinterpret_cast<void**>(&host), 64, hipHostMallocDefault) != hipSuccess) { host = nullptr; (void)hipGetLastError(); return false; }
		if (hipHostGetDevicePointer(reinterpret_cast<void**>(&dev), host, 0) != hipSuccess) { dev = nullptr; (void)hipGetLastError(); return false; }
		return true;
	}
};
thread_local OwnPinned t_own;

// Is h_wl pinned host memory the device can write, and does it hold the eight words the engine uses?  mtk::qr::buffer allocates it
// with hipHostMalloc, but a caller that sized it with the REFERENCE's get_working_l_size (batch_size + 1 words: 2..5 for m <= 128)
// must not be written past its end -- then (and for pageable memory) the thread's own pinned words are used.
// (the answer for the last h_wl of this host thread is remembered: the query sits in front of the first launch of every call, and a
// caller's loop passes the same buffer every time.  A buffer freed and re-allocated at the same address as PAGEABLE memory between two
// calls would be mistaken for the pinned one; mtk::qr::buffer always allocates hl pinned.)
struct HostSigCache { unsigned* h_wl = nullptr; unsigned* dev = nullptr; };
thread_local HostSigCache t_hsig_cache;
void resolve_host_sig(Ctx& c, unsigned* h_wl, size_t m) {
	c.hsig = HostSig{};
	if (h_wl && ref_bs(m) + 1 >= 8) {
		if (t_hsig_cache.h_wl == h_wl) { c.hsig.host = h_wl; c.hsig.dev = t_hsig_cache.dev; return; }
		hipPointerAttribute_t at{};
		if (hipPointerGetAttributes(&at, h_wl) == hipSuccess && at.type == hipMemoryTypeHost && at.devicePointer) {
			c.hsig.host = h_wl; c.hsig.dev = reinterpret_cast<unsigned*>(at.devicePointer);
			t_hsig_cache.h_wl = h_wl; t_hsig_cache.dev = c.hsig.dev;
			return;
		}
		(void)hipGetLastError();
	}
	if (t_own.get()) { c.hsig.host = t_own.host; c.hsig.dev = t_own.dev; }
}

// spin on a completion word of the pinned words (spin_until; an idle stream means the word has been raised)
int wait_word(volatile unsigned* word, unsigned seq, hipStream_t st) {
	const int w = spin_until([&] { return *word == seq; }, st);
	return w < 0 ? w : 0;
}

// End of a call on the fast path: a one-thread kernel behind the last kernel raises word 3 of the pinned words; the host spins on
// it (about 5 us cheaper than hipStreamSynchronize, tools/launch_cost.py, and free of its sporadic OS wake-up stalls) and polls
// the stream now and then so that a failed launch cannot hang the caller.  Returns 1 when the flag path is not available.
int signal_and_wait(Ctx& c) {
	if (!c.hsig.dev || t_prof.on) return 1;
	unsigned seq = ++g_seq;
	if (seq == 0) seq = ++g_seq;
	volatile unsigned* flag = reinterpret_cast<volatile unsigned*>(c.hsig.host) + 3;
	*flag = 0;
	hipLaunchKernelGGL(tsqrmi::host_flag_kernel, dim3(1), dim3(1), 0, c.st, c.hsig.dev + 3, seq);
	if (hipGetLastError() != hipSuccess) return 1;
	return wait_word(flag, seq, c.st);
}
int wait_done(Ctx& c) {
	const int w = signal_and_wait(c);
	if (w < 0) return w;
	if (w == 1) HIPCHK(hipStreamSynchronize(c.st));
	return 0;
}

// ---- calls in flight (tsqr_mi_qr_f32_submit / _finish): at most two per host thread, one per half of the pinned words (status
// words 4 * slot .. 4 * slot + 2, completion word 4 * slot + 3).  "Latching" a ticket = waiting for its completion word and copying
// the verdict out of the pinned words, after which the slot (and the stream behind it) is free for anything else. ----
thread_local tsqr_mi_ticket* t_pending[2] = {nullptr, nullptr};
thread_local unsigned t_submits = 0;
int ticket_latch(tsqr_mi_ticket* t) {
	if (!t || t->pending != 1) return 0;
	volatile unsigned* w = reinterpret_cast<volatile unsigned*>(t->words) + 4 * t->slot;
	const int rc = wait_word(w + 3, t->seq, reinterpret_cast<hipStream_t>(t->stream));
	if (rc) { t_pending[t->slot] = nullptr; t->pending = 0; t->state = -1; return rc; }
	t->verdict = w[0];
	const unsigned b = w[2];
	memcpy(&t->scond, &b, 4);
	t->pending = 2;
	if (t_pending[t->slot] == t) t_pending[t->slot] = nullptr;
	return 0;
}
int latch_all() {
	for (int s = 0; s < 2; s++)
		if (t_pending[s]) { const int rc = ticket_latch(t_pending[s]); if (rc) return rc; }
	return 0;
}

// read the status word of slot `s` (0 accepted / 1 rejected) after draining the stream (wait = false: the stream is known to be idle)
int read_status(Ctx& c, int s, unsigned* out, float* scond = nullptr, bool wait = true) {
	if (g_set.debug) {
		unsigned w3[3];
		HIPCHK(hipStreamSynchronize(c.st));
		HIPCHK(hipMemcpy(w3, c.status_dev(s), sizeof(w3), hipMemcpyDeviceToHost));
		float ratio, sc;
		memcpy(&ratio, &w3[1], 4); memcpy(&sc, &w3[2], 4);
		fprintf(stderr, "[tsqr_mi] chol status %u  min pivot ratio %.4g  scaled cond S %.4g\n", w3[0], ratio, sc);
	}
	if (c.hsig.dev) {                                    // the Cholesky kernel wrote the words to the pinned memory itself
		if (wait) {
			const int rc = wait_done(c);
			if (rc) return rc;
		}
		volatile unsigned* h = reinterpret_cast<volatile unsigned*>(c.hsig.host) + 4 * s;
		*out = h[0];
		if (scond) { const unsigned b = h[2]; memcpy(scond, &b, 4); }
		return 0;
	}
	unsigned w3[3];
	HIPCHK(hipStreamSynchronize(c.st));
	HIPCHK(hipMemcpy(w3, c.status_dev(s), sizeof(w3), hipMemcpyDeviceToHost));
	*out = w3[0];
	if (scond) memcpy(scond, &w3[2], 4);
	return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------------------------------
template <int NT> int launch_fold(const tsqrmi::FoldArgs& a, hipStream_t st) {
	const int blocks = (a.nwaves + 3) / 4;
	if constexpr (NT == 4) {
		if (a.tri_init) {
			if (a.cor) hipLaunchKernelGGL((tsqrmi::fold_kernel<4, true, true>), dim3(blocks), dim3(256), 0, st, a);
			else hipLaunchKernelGGL((tsqrmi::fold_kernel<4, true, false>), dim3(blocks), dim3(256), 0, st, a);
			return 0;
		}
	}
	if (a.cor) hipLaunchKernelGGL((tsqrmi::fold_kernel<NT, false, true>), dim3(blocks), dim3(256), 0, st, a);
	else hipLaunchKernelGGL((tsqrmi::fold_kernel<NT, false, false>), dim3(blocks), dim3(256), 0, st, a);
	return 0;
}
int dispatch_fold(int NT, const tsqrmi::FoldArgs& a, hipStream_t st) {
	return with_nt(NT, [&](auto nt) { return launch_fold<decltype(nt)::value>(a, st); });
}

// the R-stack reduction (fold_coop_kernel): nblocks upper-triangular 64 x 64 blocks of `stack` -> R, ping-ponging between `stack` and
// `other`; eight stacked blocks per workgroup and 64-step chain: 2048 -> 256 -> 32 -> 4 -> 1 in four launches / four dependent chains
int fold_coop(Ctx& c, float* r, size_t ldr, float* stack, size_t stack_ld, int nblocks, size_t n, float* other, bool cor) {
	constexpr int W = tsqrmi::FOLD_COOP_WAVES;
	constexpr int lds = tsqrmi::FOLD_COOP_LDS_FLOATS * (int)sizeof(float);
	static DevOnce attr[2];
	if (attr[cor].need(c.dev)) {
		HIPCHK(hipFuncSetAttribute(cor ? reinterpret_cast<const void*>(&tsqrmi::fold_coop_kernel<true>) : reinterpret_cast<const void*>(&tsqrmi::fold_coop_kernel<false>),
		                           hipFuncAttributeMaxDynamicSharedMemorySize, lds));
		attr[cor].done(c.dev);
	}
	float* cur = stack; size_t cur_ld = stack_ld;
	float* nxt = other;
	for (;;) {
		tsqrmi::FoldTreeArgs a{};
		a.src = cur; a.ld = cur_ld; a.nblocks = nblocks; a.n = (int)n;
		const int wgs = (nblocks + W - 1) / W;
		if (wgs == 1) { a.dst = r; a.dst_ld = ldr; a.rows_store = (int)n; a.cols_store = (int)n; }
		else { a.dst = nxt; a.dst_ld = (size_t)wgs * 64; a.rows_store = 64; a.cols_store = 64; }
		{
			ProfScope ps(KC_TREE, c.st);
			if (cor) hipLaunchKernelGGL(tsqrmi::fold_coop_kernel<true>, dim3(wgs), dim3(64 * W), lds, c.st, a);
			else hipLaunchKernelGGL(tsqrmi::fold_coop_kernel<false>, dim3(wgs), dim3(64 * W), lds, c.st, a);
		}
		HIPCHK(hipGetLastError());
		if (wgs == 1) break;
		float* t = cur; cur = nxt; nxt = t; cur_ld = (size_t)wgs * 64;
		nblocks = wgs;
	}
	return 0;
}

// R (n x n, ldr; full block written, zeros below the diagonal) of src (m x n), n <= 64: streaming Householder TSQR + fold tree.
// stack_a / stack_b: scratch for the R stacks of even / odd levels (Plan::stack_a / stack_b floats).
int fold_r(Ctx& c, float* r, size_t ldr, const float* src, size_t ld, size_t m, size_t n, float* stack_a, float* stack_b) {
	const Plan p = make_plan(m, n);
	const int NT = (int)(p.NP / 16);
	const bool cor = c.fold_cor;
	const float* cur = src; size_t cur_ld = ld;
	for (int lv = 0; lv < p.nlevels; lv++) {
		tsqrmi::FoldArgs a{};
		a.src = cur; a.ld = cur_ld; a.m = p.rows[lv];
		a.n = (int)n;                                    // stacks are NP wide, only the first n columns carry data
		a.nchunks = p.nch[lv]; a.cpw = p.cpw[lv]; a.nwaves = p.nw[lv];
		a.tri_init = (lv > 0 && p.NP == 64) ? 1 : 0;
		a.cor = cor ? 1 : 0;
		if (p.nw[lv] == 1) {
			a.dst = r; a.dst_ld = ldr; a.rows_store = (int)n; a.cols_store = (int)n;
		} else {
			float* stack = (lv % 2 == 0) ? stack_a : stack_b;
			a.dst = stack; a.dst_ld = (size_t)p.nw[lv] * p.NP; a.rows_store = (int)p.NP; a.cols_store = (int)p.NP;
			cur = stack; cur_ld = a.dst_ld;
		}
		{
			ProfScope ps(lv == 0 ? KC_FOLD0 : KC_TREE, c.st);
			dispatch_fold(NT, a, c.st);
		}
		HIPCHK(hipGetLastError());
		if (lv == 0 && p.nw[0] > 1 && p.NP == 64) {
			// 64-column panels: the whole R-stack reduction by cooperative eight-block folds (fold_coop_kernel) instead of one launch per binary level
			return fold_coop(c, r, ldr, stack_a, (size_t)p.nw[0] * 64, p.nw[0], n, stack_b, cor);
		}
	}
	return 0;
}

template <int NT> void launch_gram(const tsqrmi::GramArgs& a, int nblocks, bool bf16, hipStream_t st) {
	if (bf16) hipLaunchKernelGGL(tsqrmi::gram_bf16_kernel<NT>, dim3(nblocks), dim3(256), 0, st, a);
	else hipLaunchKernelGGL(tsqrmi::gram_kernel<NT>, dim3(nblocks), dim3(256), 0, st, a);
}
// the operands gram_blk_kernel takes: a full 64-column block of 128 k <= 2^20 rows, columns 16-byte aligned, 32-bit buffer offsets
inline bool blk_gram_ok(const float* a, size_t lda, size_t m, size_t n) {
	return n == PW && m % 128 == 0 && m <= ((size_t)1 << 20) && lda % 4 == 0 && lda <= ((size_t)1 << 24) && (reinterpret_cast<uintptr_t>(a) & 15) == 0;
}

// The load policy of A for one panel whose Gram pass takes gram_blk_kernel (tsqr_mi_set_load_policy).  A pinned setting holds for every
// such panel; under the auto setting the streamed policy is taken only where it was measured faster (measure_load_policy: once per
// process and device, by the first eligible blocking call) and only for what it was measured on: operands of at least 128 MiB, out of
// place, no profiling.  Everything else -- and every call before the measurement -- loads as it always did.
constexpr double LOAD_POLICY_MIN_BYTES = 128.0 * 1048576.0;
std::atomic<int> g_load_policy_chosen[MAX_DEV];        // 0 not measured yet, 1 cache-allocating, 2 streamed
int resolve_load_policy(int dev, double bytes, bool as_measured) {   // as_measured: out of place, and the apply pass is the plain 64-row kernel (both passes follow the policy)
	const int pinned = g_set.load_policy.load();
	if (pinned) return pinned;
	return (bytes >= LOAD_POLICY_MIN_BYTES && as_measured && !t_prof.on && g_load_policy_chosen[dev].load() == 2) ? 2 : 1;
}

// Gram matrix of src (m x n) in MFMA-accumulator order -> c.gsum() (ntri*256 doubles + the local row count behind them), summed
// over the ranks of a row-partitioned call.  bf16 = true: bf16x3-split MFMA (memory-bound, f32 C/D layout), false: fp64 MFMA.
// io_half: src holds halves (fp16 I/O modes, bf16 level only): gram_h_kernel takes them as MFMA operands directly.
int gram_g(Ctx& c, const SweepOpts& o, const float* src, size_t ld, size_t m, size_t n, bool bf16, bool io_half = false) {
	const GramPlan g = gram_plan(m, n);
	const int NT = (int)(np_of(n) / 16);
	tsqrmi::GramArgs a{};
	a.a = src; a.lda = ld; a.m = m; a.n = (int)n; a.nchunks = g.nch; a.cpw = g.cpw; a.nwaves = g.nwaves;
	a.part = reinterpret_cast<double*>(c.wr);
	a.skip_status = o.prev_slot >= 0 ? c.status_dev(o.prev_slot) : nullptr;
	const bool ready = bf16 && o.gramq_ready > 0;        // the previous sweep's apply kernel accumulated this very Gram matrix (fp64-level requests never take it)
	if (!ready) carry_announcement(c, a);
	int nparts = g.nblocks;                              // workgroups that wrote a partial
	if (ready) nparts = o.gramq_ready;
	else if (io_half) {
		ProfScope ps(KC_GRAM, c.st);
		with_nt(NT, [&](auto nt) { hipLaunchKernelGGL(tsqrmi::gram_h_kernel<decltype(nt)::value>, dim3(g.nblocks), dim3(256), 0, c.st, a); });
	} else if (bf16 && blk_gram_ok(src, ld, m, n)) {
		// full 64-column matrices that fit the 256 MiB Infinity Cache: block-pattern loads + LDS staging (gram_blk_kernel); everything
		// else: gram_bf16_kernel.  (Measured, kernel / call period under the profiler: 2^21 rows 93.8 / 322.6 vs 95.8 / 319.4 us,
		// 2^22 rows 190.0 / 621.2 vs 192.0 / 621.0, 2^23 rows 421 / 1310 vs 381 / 1266 -- beyond the cache the chunk kernel is as good
		// or better; at 2^20 rows the call is 3-5 us faster with the block kernel, profiles/r03_experiment_log.md.)
		const int rc = blk_kernel_attrs(c.dev);
		if (rc) return rc;
		a.nchunks = (int)(m / 128);
		nparts = std::min(a.nchunks, g.nblocks);
		ProfScope ps(KC_GRAM, c.st);
		if (o.load_policy == 2) hipLaunchKernelGGL(tsqrmi::gram_blk_kernel<true>, dim3(nparts), dim3(256), tsqrmi::GB_LDS_BYTES, c.st, a);
		else hipLaunchKernelGGL(tsqrmi::gram_blk_kernel<false>, dim3(nparts), dim3(256), tsqrmi::GB_LDS_BYTES, c.st, a);
		g_load_policy_used.store(o.load_policy == 2 ? 2 : 1);
	} else {
		ProfScope ps(KC_GRAM, c.st);
		with_nt(NT, [&](auto nt) { launch_gram<decltype(nt)::value>(a, g.nblocks, bf16, c.st); });
	}
	HIPCHK(hipGetLastError());
	const int nelem = g.ntri * 256;
	{
		ProfScope ps(KC_CHOL, c.st);
		launch_reduce1(c.st, c.gsum(), a.part, nparts, nelem, (double)m);
	}
	HIPCHK(hipGetLastError());
	if (c.comm.active()) {
		// the ONLY exchange of the Gram engine: <= 2560 doubles + the row count.  Every rank then factors the same matrix with the
		// same thresholds, so all ranks take the same accept / reject decisions by construction (a NaN on one rank reaches all).
		ProfScope ps(KC_MISC, c.st);
		if (c.comm.allreduce_f64(c.gsum(), (size_t)nelem + 1, c.st)) { t_last_error = "all-reduce of the Gram tiles failed"; return -1; }
	}
	return 0;
}

// The arguments of chol16_kernel: R = chol(G) (n x n, ldr), Z = inverse(R) (NP x NP in wq[L.z]), status words -> slot o.slot (the chained
// schedules: half i & 1 of call i).  level: 2 bf16, 1 fp64, 3 shifted fp64.
tsqrmi::CholArgs chol_args(const Ctx& c, const SweepOpts& o, float* r, size_t ldr, size_t n, int level) {
	tsqrmi::CholArgs a{};
	a.r = r; a.ldr = ldr; a.z = c.wq + c.L.z;
	a.status = c.status_dev(o.slot);
	a.host_status = c.hsig.dev ? c.hsig.dev + 4 * o.slot : nullptr;
	a.gsum = c.gsum();
	a.prev_status = o.prev_slot >= 0 ? c.status_dev(o.prev_slot) : nullptr;
	const int NT = (int)(np_of(n) / 16);
	a.rows_dev = c.comm.active() ? c.gsum() + (size_t)(NT * (NT + 1) / 2) * 256 : nullptr;
	a.rows = c.rows_global;
	a.shift_coef = (level == 3) ? 11.0 * 1.1102230246251565e-16 : 0.0;
	a.n = (int)n; a.NT = NT; a.level = level; a.scond_floor = g_set.bf16_scond_floor;
	if (level == 2) { a.relax = o.relax; a.retry_shift = o.retry_shift; }
	return a;
}
int chol_from_g(Ctx& c, const SweepOpts& o, float* r, size_t ldr, size_t n, int level) {
	{
		ProfScope ps(KC_CHOL, c.st);
		hipLaunchKernelGGL(tsqrmi::chol16_kernel, dim3(1), dim3(1024), 0, c.st, chol_args(c, o, r, ldr, n, level));
	}
	HIPCHK(hipGetLastError());
	return 0;
}

// The launcher of the apply family (KERNEL: the entry; G: its tsqrmi::ApplyGeom): the dynamic-LDS attribute, once per device and instance; the
// persistent grid -- as many workgroups as are resident on the 256 CUs at once, CAP per CU at the most (QUERY: and no more than the
// runtime's occupancy figure) -- or grid.wgs of them, split over grid.gy panels and never more than grid.max_wgs; a.nchunks = row blocks
// of G::ROWS, a.nwaves = workgroups (ApplyGrid, apply_instance_setup, apply_grid_fill: f32_plan.h -- shared with the test library).
// pre(a, per_cu, lds, gy) sees the sized grid before the launch; true: the pass has run, no launch.
template <auto KERNEL, class G, bool GRAMQ, int CAP, bool QUERY, class Pre>
int launch_apply(Ctx& c, tsqrmi::ApplyArgs a, const ApplyGrid& grid, Pre&& pre) {
	constexpr size_t lds = G::lds_bytes(GRAMQ);
	static DevOnce attr;                                 // (per template instance)
	static std::atomic<int> per_cu_cache[MAX_DEV];
	if (attr.need(c.dev)) {
		int nb = CAP;
		const int rc = apply_instance_setup<KERNEL, G, GRAMQ, CAP, QUERY>(&nb);
		if (rc) return rc;
		per_cu_cache[c.dev].store(nb);
		attr.done(c.dev);
	}
	const int per_cu = per_cu_cache[c.dev].load();
	apply_grid_fill<G>(a, grid, per_cu);
	if (pre(a, per_cu, lds, grid.gy)) return 0;
	hipLaunchKernelGGL(KERNEL, dim3(a.nwaves, grid.gy), dim3(G::THREADS), lds, c.st, a);
	return 0;
}
inline bool apply_no_pre(tsqrmi::ApplyArgs&, int, size_t, unsigned) { return false; }

// Four workgroups per CU on the whole chip: uneven shares by XCD parity and by dispatch round (apply_wg_body; round 3, on every box
// looked at THEN: the pass ends at 78 us instead of 84).  Round 4: on five boxes in a row the same shares COST 5-6 % of the call
// (blocking 194.9-198.9 us against 186.1-188.1 with equal shares, chained 170.3-173.2 against 159.4-161.1; three interleaved runs,
// profiles/r04_experiment_log.md) -- the XCD asymmetry they answer is a property of the box's state, not of the chip.  So the
// choice is MEASURED once per process and device (and per side of the cache size), on the first large out-of-place pass: the two
// candidates (shares by XCD parity and round / equal) run the pass itself in turn under HIP events, four times each (Q = A Z is the
// same whoever computes a block: the last run leaves the result), ~0.7 ms once; the uneven shares are taken only when they are 1 %
// faster.  TSQR_MI_APPLY_SHARES=0 / 1 / 2 pins equal / both / by round only.
// Sets a's shares; true: this was the measurement, the pass has run.
// KEY: the instance whose choice this one shares (the streamed-load instance of a kernel takes the shares of the plain one, whichever of the
// two measured them).
template <auto KEY> std::atomic<int> (&block_shares_chosen())[MAX_DEV][2] {
	static std::atomic<int> chosen[MAX_DEV][2];      // 0 not measured yet, 1 both, 2 rounds only, 3 equal; [1]: a matrix beyond the Infinity Cache
	return chosen;
}
template <auto KERNEL, auto KEY = KERNEL> bool choose_block_shares(Ctx& c, tsqrmi::ApplyArgs& a, int per_cu, size_t lds, unsigned gy) {
	if (a.nwaves != 1024 || per_cu != 4) return false;
	static const int pinned = env_int("TSQR_MI_APPLY_SHARES", -1);
	auto& chosen = block_shares_chosen<KEY>();
	auto set_mode = [](tsqrmi::ApplyArgs& x, int mode) {
		x.share[0] = x.share[1] = x.share[2] = x.share[3] = 0; x.even_share = 0;
		if (mode == 1 || mode == 2) { x.share[0] = 18; x.share[1] = 17; x.share[2] = 15; x.share[3] = 14; x.even_share = (mode == 1) ? 69 : 64; }
	};
	const double bytes = (double)a.m * (double)a.n * sizeof(float);
	const int cls = bytes > 256.0 * 1048576.0 ? 1 : 0;
	int mode = pinned == 0 ? 3 : (pinned == 1 ? 1 : (pinned == 2 ? 2 : chosen[c.dev][cls].load()));
	const bool big = bytes >= 128.0 * 1048576.0;
	if (mode == 0 && big && reinterpret_cast<const void*>(a.q) != reinterpret_cast<const void*>(a.a) && !t_prof.on) {
		constexpr int REPS = 4;                          // interleaved: uneven, equal, uneven, equal, ...
		hipEvent_t ev[2 * REPS + 1];
		bool ok = true;
		for (auto& e : ev) ok = ok && hipEventCreate(&e) == hipSuccess;
		if (ok) {
			for (int i = 0; i < 2 * REPS; i++) {
				tsqrmi::ApplyArgs x = a;
				set_mode(x, (i & 1) ? 3 : 1);
				(void)hipEventRecord(ev[i], c.st);
				hipLaunchKernelGGL(KERNEL, dim3(a.nwaves, gy), dim3(256), lds, c.st, x);
			}
			(void)hipEventRecord(ev[2 * REPS], c.st);
			ok = hipEventSynchronize(ev[2 * REPS]) == hipSuccess;
			float t[2] = {0.f, 0.f};
			for (int i = 0; i < 2 * REPS && ok; i++) { float ms = 0.f; ok = hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess; t[i & 1] += ms; }
			// (a speculative pass that skipped itself -- rejected Gram matrix -- measures nothing: ask again next time)
			if (ok && t[0] > 0.01f * REPS && t[1] > 0.01f * REPS)
				chosen[c.dev][cls].store(t[0] < 0.99f * t[1] ? 1 : 3);   // equal shares unless the uneven ones are (1 %) faster: 3 % on the boxes they were tuned on, 5-10 % SLOWER elsewhere
		}
		for (auto& e : ev) (void)hipEventDestroy(e);
		(void)hipGetLastError();
		return true;                                     // (the pass has run)
	}
	set_mode(a, mode == 0 ? 3 : mode);
	return false;
}

// apply_wg_kernel launcher; GRAMQ: the number of workgroups (one partial each) -> *gramq_nparts
template <int E, int NT, bool UPD, int ROWS, bool GRAMQ> constexpr auto apply_wg_entry() {
	if constexpr (GRAMQ) return &tsqrmi::apply_wg_gramq_kernel<E, NT, UPD, ROWS>;
	else return &tsqrmi::apply_wg_kernel<E, NT, UPD, ROWS>;
}
template <int E, int NT, bool UPD, int ROWS, bool GRAMQ = false> int launch_apply_wg(Ctx& c, const SweepOpts& o, int* gramq_nparts, const tsqrmi::ApplyArgs& a) {
	constexpr auto kernel = apply_wg_entry<E, NT, UPD, ROWS, GRAMQ>();
	// persistent grid: as many workgroups as are resident on the 256 CUs at once (LDS / register bound: 2 or 3 per CU);
	// measured: the fp32-MFMA engine is slower with three per CU (132 vs 112 us)
	constexpr int CAP = apply_wg_cap<E, ROWS>();         // (f32_plan.h)
	ApplyGrid grid;
	grid.wgs = g_set.apply_wgs.load();
	if (UPD) grid.gy = UpdApply<E>::gy(a.multi_cols);
	if (GRAMQ) grid.max_wgs = o.gramq_cap;               // one partial per workgroup: never more than the buffer holds
	if constexpr (!UPD && !GRAMQ && ROWS == 64 && NT == 4) {
		// the streamed load policy: the same kernel with nontemporal loads of A (an instance of its own: its own attributes, the same grid and shares)
		if (o.load_policy == 2) {
			constexpr auto streamed = &tsqrmi::apply_wg_kernel<E, NT, UPD, ROWS, false, true>;
			return launch_apply<streamed, tsqrmi::ApplyGeom<E, NT, UPD, ROWS>, GRAMQ, CAP, true>(c, a, grid, [&](tsqrmi::ApplyArgs& x, int per_cu, size_t lds, unsigned gy) {
				return choose_block_shares<streamed, kernel>(c, x, per_cu, lds, gy);
			});
		}
	}
	return launch_apply<kernel, tsqrmi::ApplyGeom<E, NT, UPD, ROWS>, GRAMQ, CAP, true>(c, a, grid, [&](tsqrmi::ApplyArgs& x, int per_cu, size_t lds, unsigned gy) {
		if constexpr (GRAMQ) {
			x.gpart = o.gramq_part;
			if (gramq_nparts) *gramq_nparts = x.nwaves;
		}
		if constexpr (!UPD && !GRAMQ && ROWS == 64) return choose_block_shares<kernel>(c, x, per_cu, lds, gy);
		else return false;
	});
}
template <int E, int NT, bool UPD> int launch_apply_any(Ctx& c, const SweepOpts& o, int* gramq_nparts, const tsqrmi::ApplyArgs& a) {
	if constexpr (!UPD && E != 0) {                      // (the fp32-MFMA engine's fused variant spills and loses: 0.29 vs 0.22 ms per apply)
		if (o.gramq_part && o.gramq_cap > 0) return launch_apply_wg<E, NT, UPD, 128, true>(c, o, gramq_nparts, a);
	}
	// block height per engine (measured, profiles/r02_experiment_log.md): the bf16x3 engine streams best with 64-row blocks, four
	// workgroups per CU and two blocks in flight (88 vs 92 us at 2^20 x 64); the exact-fp32 and fp16 engines and the coupling
	// update (UPD) use 128-row blocks
	return launch_apply_wg<E, NT, UPD, apply_wg_rows<E, UPD>()>(c, o, gramq_nparts, a);
}
// fp16 I/O modes: the plain product with halves at both ends -- bf16x3 engine 1 (fp16_notc) or single-fp16-product engine 2
// (fp16_tc_nocor); 64- / 128-row blocks as in the fp32 call, two blocks in flight
template <int E, int NT> int launch_apply_h(Ctx& c, const tsqrmi::ApplyArgs& a) {
	using H = HalfApply<E, NT>;                          // (the instance table: f32_plan.h)
	return launch_apply<H::kernel(), typename H::G, false, H::CAP, H::QUERY>(c, a, ApplyGrid{}, apply_no_pre);
}
template <int E> int dispatch_apply_h(Ctx& c, int NT, const tsqrmi::ApplyArgs& a) {
	return with_nt(NT, [&](auto nt) { return launch_apply_h<E, decltype(nt)::value>(c, a); });
}
template <int E> int dispatch_apply_nt(Ctx& c, const SweepOpts& o, int* gramq_nparts, int NT, const tsqrmi::ApplyArgs& a) {
	return with_nt(NT, [&](auto nt) { return launch_apply_any<E, decltype(nt)::value, false>(c, o, gramq_nparts, a); });
}

// q = a * inverse(r); n <= 64; Z in wq[L.z] (computed here from r unless z_ready)
// io_half: a and q hold halves (fp16 I/O modes; engines 1 and 2).  gramq_nparts (may be null): see launch_apply_wg
int apply_rinv(Ctx& c, const SweepOpts& o, int* gramq_nparts, int engine, float* q, size_t ldq, const float* a, size_t lda, const float* r, size_t ldr,
               size_t m, size_t n, bool z_ready = false, const unsigned* skip_status = nullptr, bool io_half = false,
               void* r16 = nullptr, size_t ldr16 = 0) {
	const size_t NP = np_of(n);
	const int NT = (int)(NP / 16);
	float* z_buf = c.wq + c.L.z;
	if (!z_ready) {
		ProfScope ps(KC_TRINV, c.st);
		hipLaunchKernelGGL(tsqrmi::trinv_kernel, dim3(1), dim3(256), 0, c.st, z_buf, r, ldr, (int)n, (int)NP);
	}
	HIPCHK(hipGetLastError());
	tsqrmi::ApplyArgs aa{};
	aa.a = a; aa.lda = lda; aa.q = q; aa.ldq = ldq; aa.m = m; aa.n = (int)n; aa.z = z_buf; aa.skip_status = skip_status;
	aa.r32 = r; aa.r16 = r16; aa.ldr16 = ldr16;         // (io_half with r16: r is then a packed n x n factor, ld n)
	aa.plain_q = aa.forward = o.q_read_back ? 1 : 0;
	int rc;
	{
		ProfScope ps(KC_APPLY, c.st);
		rc = with_engine(engine, [&](auto e) {
			constexpr int E = decltype(e)::value;
			if (!io_half) return dispatch_apply_nt<E>(c, o, gramq_nparts, NT, aa);
			if constexpr (E == 1) return dispatch_apply_h<1>(c, NT, aa);
			else return dispatch_apply_h<2>(c, NT, aa);  // (halves: the bf16x3 engine or the single-fp16-product one)
		});
	}
	if (rc) return rc;
	HIPCHK(hipGetLastError());
	return 0;
}

int engine_of(int mode) {
	if (mode == TSQR_MI_FP32_NOTC) return 0;
	if (mode == TSQR_MI_FP32_TC_COR) return 1;
	if (mode == TSQR_MI_FP32_TC_NOCOR) return 2;         // R factor as fp32_tc_cor, Q = A * inverse(R) with fp16 operands and no correction
	return -1;
}

// r <- r2 * r1 (upper triangular n x n, fp64 accumulation; r may not alias r1 / r2)
void launch_rmul(float* r, size_t ldr, const float* r2, size_t ldr2, const float* r1, size_t ldr1, size_t n, hipStream_t st) {
	if (n <= 64) {
		hipLaunchKernelGGL(tsqrmi::rmul64_kernel, dim3(1), dim3(1024), 0, st, r, ldr, r2, ldr2, r1, ldr1, (int)n, (const float*)nullptr, (size_t)0);
		return;
	}
	const unsigned gb = (unsigned)std::min<size_t>(1024, cdiv(n * n, 256));
	hipLaunchKernelGGL(tsqrmi::rmul_kernel, dim3(gb), dim3(256), 0, st, r, ldr, r2, ldr2, r1, ldr1, (int)n);
}
// r <- r3 * r2 * r1 (n <= 64: one launch, the inner product stays in LDS as fp64; otherwise through tmp, n x n packed)
void launch_rmul3(float* r, size_t ldr, const float* r3, const float* r2, const float* r1, float* tmp, size_t n, hipStream_t st) {
	if (n <= 64) {
		hipLaunchKernelGGL(tsqrmi::rmul64_kernel, dim3(1), dim3(1024), 0, st, r, ldr, r2, n, r1, n, (int)n, r3, n);
		return;
	}
	launch_rmul(tmp, n, r2, n, r1, n, n, st);
	launch_rmul(r, ldr, r3, n, tmp, n, n, st);
}

// Householder TSQR R factor of one <= 64-column panel.  Row-partitioned: every rank folds its block, the n x n factors are
// all-gathered (the exchange the north star names: RCCL all-gather of the local R factors) and every rank folds the same
// (P n) x n stack, so R is bitwise identical everywhere.
int householder_r(Ctx& c, float* rpp, size_t ldr, const float* ap, size_t lda, size_t m, size_t cc) {
	if (!c.comm.active())
		return fold_r(c, rpp, ldr, ap, lda, m, cc, c.wr, c.wq);
	if (!c.comm.gather_buf) { t_last_error = "row-partitioned Householder engine needs the gather buffer"; return -1; }
	const int P = c.comm.nranks;
	float* rl = c.wq + c.L.r4;                           // local R, packed (ld = cc)
	int rc = fold_r(c, rl, cc, ap, lda, m, cc, c.wr, c.wq);
	if (rc) return rc;
	{
		ProfScope ps(KC_MISC, c.st);
		if (c.comm.allgather_f32(rl, c.comm.gather_buf, cc * cc, c.st)) { t_last_error = "all-gather of the local R factors failed"; return -1; }
	}
	// gather_buf is [rank][column][row]; restack into wr as a column-major (P cc) x cc matrix, fold scratch behind it (both sized
	// by tsqr_mi_working_r_size_dist)
	float* stack = c.wr;
	for (int k = 0; k < P; k++)
		hipLaunchKernelGGL(tsqrmi::copy2d_kernel, dim3(16), dim3(256), 0, c.st,
		                   stack + (size_t)k * cc, (size_t)P * cc, c.comm.gather_buf + (size_t)k * cc * cc, cc, (int)cc, (int)cc);
	HIPCHK(hipGetLastError());
	const size_t stack_floats = ((size_t)P * cc * cc + 63) & ~(size_t)63;
	return fold_r(c, rpp, ldr, stack, (size_t)P * cc, (size_t)P * cc, cc, c.wr + stack_floats, c.wq);
}

constexpr int R_SHIFT_DIRECT = 9;
// R factor and Q of one <= 64-column panel.  r_engine: first Gram level (2 / 1), 0 = Householder, R_SHIFT_DIRECT = the caller has
// just seen the fp64 Gram level reject this very panel (its Gram matrix is still in the work buffer): shifted-Cholesky step at once.
// check_now: read each verdict immediately (one wait) and escalate on rejection; otherwise enqueue speculatively.
int panel_qr(Ctx& c, const SweepOpts& o, int* gramq_nparts, int engine, int r_engine, bool check_now, float* qp, size_t ldq, float* rpp, size_t ldr, const float* ap, size_t lda,
             size_t m, size_t cc) {
	int rc;
	const bool direct_shift = (r_engine == R_SHIFT_DIRECT);
	if (direct_shift) r_engine = 0;
	for (int e = r_engine; e >= 1; e--) {                // 2: bf16-split Gram, 1: fp64 Gram; with check_now a rejected level escalates
		// (o.gramq_ready: only the bf16-level request, e == 2, takes ready partials, and this loop makes one such request at the most.  Sweeps
		// are fused for n <= 64 alone -- one panel, one call of this function -- so the sweep's value can be forwarded as it is.)
		// (the load policy is a matter of the panels gram_blk_kernel takes -- gram_g sends the same ones there; every other panel's two passes
		// are the kernels and loads they always were)
		SweepOpts po = o;
		if (!(e == 2 && blk_gram_ok(ap, lda, m, cc))) po.load_policy = 1;
		else if (po.load_policy == 0) po.load_policy = resolve_load_policy(c.dev, (double)m * (double)cc * sizeof(float), qp != ap && engine == 1);
		rc = gram_g(c, po, ap, lda, m, cc, e == 2);
		if (rc) return rc;
		rc = chol_from_g(c, o, rpp, ldr, cc, e);
		if (rc) return rc;
		bool ok = true;
		if (check_now) {
			unsigned status = 0;
			rc = read_status(c, o.slot, &status);
			if (rc) return rc;
			ok = (status == 0);
		}
		if (ok) {
			c.min_level = std::min(c.min_level, e);
			// speculative (unchecked) launch under the auto policy: the kernel itself skips the pass when the level was rejected
			const unsigned* skip = (!check_now && c.policy == 0) ? c.status_dev(o.slot) : nullptr;
			return apply_rinv(c, po, gramq_nparts, engine, qp, ldq, ap, lda, rpp, ldr, m, cc, /*z_ready=*/true, skip);
		}
	}
	if ((direct_shift || (r_engine >= 1 && check_now)) && c.policy == 0) {
		// Both Gram levels rejected the panel (cond beyond ~1e6, or rank deficient).  Shifted Cholesky QR: the fp64 Gram matrix is
		// still in the work buffer; R1 = chol(G + s I) always exists, Q1 = A inverse(R1) has cond(Q1) <~ 1e5, and one unshifted fp64
		// sweep on Q1 in place finishes the panel: A = Q (R2 R1).  About 2x faster than the Householder fold below and, after that
		// second step, at least as orthogonal as its single indirect sweep.
		float* r1 = c.wq + c.L.r3; float* r2 = c.wq + c.L.r4;
		rc = chol_from_g(c, o, r1, cc, cc, 3);
		if (rc) return rc;
		unsigned status = 0;
		rc = read_status(c, o.slot, &status);
		if (rc) return rc;
		if (status == 0) {
			rc = apply_rinv(c, o, gramq_nparts, engine, qp, ldq, ap, lda, r1, cc, m, cc, /*z_ready=*/true);
			if (rc) return rc;
			rc = gram_g(c, o, qp, ldq, m, cc, /*bf16=*/false);
			if (rc) return rc;
			rc = chol_from_g(c, o, r2, cc, cc, 1);
			if (rc) return rc;
			rc = read_status(c, o.slot, &status);
			if (rc) return rc;
			if (status == 0) {
				rc = apply_rinv(c, o, gramq_nparts, engine, qp, ldq, qp, ldq, r2, cc, m, cc, /*z_ready=*/true);
			} else {
				// Q1 is still numerically rank deficient: the input has an (almost) exactly dependent column whose rounding residue is
				// itself dependent (e.g. two constant columns).  No triangular solve can make an orthonormal column out of that; a
				// second SHIFTED step keeps everything bounded instead -- the other columns come out orthonormal, the residual stays
				// at rounding level, R shows the deficiency as a tiny diagonal entry and that one column of Q is left un-normalised.
				rc = chol_from_g(c, o, r2, cc, cc, 3);
				if (rc) return rc;
				rc = read_status(c, o.slot, &status);
				if (rc) return rc;
				if (status == 0) {
					rc = apply_rinv(c, o, gramq_nparts, engine, qp, ldq, qp, ldq, r2, cc, m, cc, /*z_ready=*/true);
				} else {                                     // non-finite data: last resort, the Householder engine on Q1
					c.used_householder = true;
					rc = householder_r(c, r2, cc, qp, ldq, m, cc);
					if (rc) return rc;
					rc = apply_rinv(c, o, gramq_nparts, engine, qp, ldq, qp, ldq, r2, cc, m, cc);
				}
			}
			if (rc) return rc;
			launch_rmul(rpp, ldr, r2, cc, r1, cc, cc, c.st);
			HIPCHK(hipGetLastError());
			c.min_level = 0;
			c.used_shift = true;
			return 0;
		}
	}
	c.min_level = 0;
	c.used_householder = true;
	rc = householder_r(c, rpp, ldr, ap, lda, m, cc);
	if (rc) return rc;
	return apply_rinv(c, o, gramq_nparts, engine, qp, ldq, ap, lda, rpp, ldr, m, cc);
}

int sweep_wide(Ctx& c, const SweepOpts& o, int engine, float* q, size_t ldq, float* r, size_t ldr, const float* a, size_t lda, size_t m, size_t n);

// one sweep of 64-wide-panel block QR:  (q, r) <- qr(a);  a is overwritten for n > 64; q may alias a.
// Panels are coupled by block MODIFIED Gram-Schmidt on the matrix cores (the role of the reference's cuBLAS GEMMs, src/blockqr.cu:92-116),
// RIGHT-LOOKING since round 4: as soon as panel p is factored, ONE launch each forms S = Qp^T [A_{p+1} ... A_last] (cross_kernel, a grid row
// per trailing panel), reduces it (writing R's block row and the operands -S_j) and updates every trailing panel (A_j <- A_j - Qp S_j).
// The same operations on the same operands as the left-looking order of rounds 1-3 (for every trailing panel the updates arrive in the
// same sequence, every S_j is summed in the same grouping: bit for bit the same factors), but one update launch per PANEL instead of one
// per panel pair, and the S launches grouped as far as the work space goes: at small row counts the launches finally have the chip's
// worth of workgroups (same-box A/B of the two builds, profiles/r04_experiment_log.md: 4096 x 1024 3.36 -> 1.07 ms, 32768 x 1024 3.87 -> 1.89 ms).
// gramq_nparts (may be null): the number of Gram partials the apply launch wrote to o.gramq_part (untouched when it wrote none)
int sweep(Ctx& c, const SweepOpts& o, int* gramq_nparts, int engine, int r_engine, bool check_now, float* q, size_t ldq, float* r, size_t ldr, float* a, size_t lda, size_t m, size_t n) {
	const size_t npanels = cdiv(n, PW);
	// 128-COLUMN BLOCKS (round 4): while the bf16-split level accepts them, two neighbouring panels are factored at once by the one-panel
	// path of 64 < n <= 128 (sweep_wide: ONE Gram pass over 128 columns, the two-block Cholesky factor, ONE apply pass -- speculative, A
	// untouched when the verdict over both blocks rejects) instead of panel + coupling + panel: a third of the passes over those columns
	// and one factorisation launch instead of two + a coupling.  Their two 64-column halves then couple with everything behind the block,
	// one after the other, as any two finished panels.  A rejected block (and everything after it in this sweep) takes the 64-column way.
	bool try_wide = c.wide && c.policy == 0 && r_engine == 2 && check_now && !c.comm.active() && n > 2 * PW;
	for (size_t pi = 0; pi < npanels;) {
		const size_t P = pi * PW, cc = std::min(PW, n - P);
		size_t blockw = cc;                              // columns factored in this step
		bool wide_blk = false;
		if (try_wide && n - P > PW) {
			const size_t w = std::min(2 * PW, n - P);
			int rcw = sweep_wide(c, o, engine, q + P * ldq, ldq, r + P * ldr + P, ldr, a + P * lda, lda, m, w);
			if (rcw) return rcw;
			unsigned stw = 1u;
			rcw = read_status(c, o.slot, &stw);
			if (rcw) return rcw;
			if (stw == 0) { wide_blk = true; blockw = w; c.min_level = std::min(c.min_level, 2); }
			else try_wide = false;
		}
		if (!wide_blk) {
			const int rc = panel_qr(c, o, gramq_nparts, engine, r_engine, check_now, q + P * ldq, ldq, r + P * ldr + P, ldr, a + P * lda, lda, m, cc);
			if (rc) return rc;
		}
		pi += cdiv(blockw, PW);
		const size_t T0 = P + blockw;                    // first trailing column (blockw is a multiple of 64 here: only the last block may be ragged)
		if (T0 >= n) break;
		for (size_t X0 = P; X0 < T0; X0 += PW) {         // the finished 64-column panels of this step, one after the other
		const size_t Pc = X0;
		const size_t ntc = n - T0, ntr = cdiv(ntc, PW);
		ProfScope ps(KC_COUPLE, c.st);
		// S_j = Qp^T A_j for every trailing panel j (bf16x3 MFMA products, fp64 sums): launches over groups of trailing panels, as many as
		// the work space holds workgroup partials for (cross_slots: every panel keeps the workgroup count -- and so the grouping of its
		// sums -- of a single panel pair; at small row counts that is all of them in one launch)
		const GramPlan g = gram_plan(m, PW);
		double* gm = reinterpret_cast<double*>(c.wq + c.L.gmulti);
		float* sm = c.wq + c.L.smulti;
		float* rblk = r + T0 * ldr + Pc;                 // R(Pc : Pc + 64, T0 : n)
		const size_t grp = cross_group(c.cross_slots, g.nblocks);
		for (size_t j0 = 0; j0 < ntr; j0 += grp) {
			const unsigned gy = (unsigned)std::min(grp, ntr - j0);
			// one GPU: the reduction writes -S_j (operand of the update) and the block row of R itself; row-partitioned: the sums only
			// (cross_group_launch: f32_plan.h -- shared with the test library)
			cross_group_launch(c.st, g, q + Pc * ldq, ldq, a + T0 * lda, lda, m, ntc, j0, gy, reinterpret_cast<double*>(c.wr), gm, !c.comm.active(), rblk, ldr, sm);
			HIPCHK(hipGetLastError());
		}
		if (c.comm.active()) {
			// ONE all-reduce for the whole block row (every rank holds the same S afterwards: the same R, the same update)
			if (c.comm.allreduce_f64(gm, ntr * (size_t)tsqrmi::CROSS_GSTRIDE, c.st)) { t_last_error = "all-reduce of the coupling tiles failed"; return -1; }
			cross_finish_launch(c.st, rblk, ldr, sm, gm, ntc);
			HIPCHK(hipGetLastError());
		}
		tsqrmi::ApplyArgs ua{};
		ua.a = q + Pc * ldq; ua.lda = ldq; ua.q = a + T0 * lda; ua.ldq = lda; ua.m = m; ua.n = (int)PW; ua.z = sm;
		ua.n_out = (int)std::min(PW, ntc); ua.multi_cols = (int)ntc;
		const int rc2 = with_engine(engine, [&](auto e) { return launch_apply_any<decltype(e)::value, 4, true>(c, o, nullptr, ua); });
		if (rc2) return rc2;
		HIPCHK(hipGetLastError());
		}
	}
	return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// 64 < n <= 128 as ONE Cholesky-QR panel (tsqr_wide.hip): Gram tiles of all n columns in one pass, the 128 x 128 Cholesky factor in
// two 64 x 64 blocks, Q = A * inverse(R) in one pass.  Everything is enqueued speculatively: the verdict over both blocks lands in
// slot o.slot (and its pinned alias), the apply pass skips itself on rejection, A is untouched (q == a is allowed: every workgroup
// has its block in LDS before it writes).  r receives the full n x n factor.
// ---------------------------------------------------------------------------------------------------------------------------
template <int E> int launch_apply_wide(Ctx& c, const tsqrmi::ApplyArgs& a) {
	using W = WideApply<E>;                              // (the instance table: f32_plan.h)
	return launch_apply<W::kernel(), typename W::G, false, W::CAP, W::QUERY>(c, a, ApplyGrid{}, apply_no_pre);
}
// the one-panel path's arguments, shared by the blocking call (sweep_wide) and the stream of 128-column calls (chained128); verdict and
// skip word: status slot o.slot
struct WideWs { double* gsum; float* zw; float* zf2; };  // summed tiles, Z (128 x 128), Z22 in the work space behind WqLayout::wide
WideWs wide_ws(const Ctx& c) {
	float* w = c.wq + c.L.wide;
	return WideWs{reinterpret_cast<double*>(w), w + WIDE_OFF_ZW, w + WIDE_OFF_ZF2};
}
// the Gram pass over the first nblk 64-row blocks of a; it carries the pending announcement
tsqrmi::GramWideArgs gram_wide_args(Ctx& c, const float* a, size_t lda, size_t m, size_t n, int nblk) {
	tsqrmi::GramWideArgs ga{};
	ga.a = a; ga.lda = lda; ga.m = m; ga.n = (int)n; ga.blk0 = 0; ga.nblk = nblk; ga.part = reinterpret_cast<double*>(c.wr);
	carry_announcement(c, ga);
	return ga;
}
// chol(G11) -> Schur complement -> chol(G22') -> Z12 + verdict: one workgroup, one launch (chol_wide_kernel)
tsqrmi::CholWideArgs chol_wide_args(const Ctx& c, const SweepOpts& o, float* r, size_t ldr, size_t m, size_t n) {
	const WideWs w = wide_ws(c);
	tsqrmi::CholWideArgs wa = chol_wide_wiring(w.gsum, r, ldr, m, n, c.wq + c.L.z, w.zf2, w.zw, c.status_dev(2), c.status_dev(3), g_set.bf16_scond_floor);
	wa.status = c.status_dev(o.slot);
	wa.host_status = c.hsig.dev ? c.hsig.dev + 4 * o.slot : nullptr;
	wa.prev_status = o.prev_slot >= 0 ? c.status_dev(o.prev_slot) : nullptr;
	return wa;
}
// Q = A * inverse(R) of the one-panel path; skips itself when the verdict in o.slot rejects
int apply_wide(Ctx& c, const SweepOpts& o, int engine, float* q, size_t ldq, const float* a, size_t lda, size_t m, size_t n) {
	tsqrmi::ApplyArgs aa{};
	aa.a = a; aa.lda = lda; aa.q = q; aa.ldq = ldq; aa.m = m; aa.n = (int)n; aa.z = wide_ws(c).zw; aa.skip_status = c.status_dev(o.slot);
	int rc;
	{
		ProfScope ps(KC_APPLY, c.st);
		rc = with_engine(engine, [&](auto e) { return launch_apply_wide<decltype(e)::value>(c, aa); });
	}
	if (rc) return rc;
	HIPCHK(hipGetLastError());
	return 0;
}
int sweep_wide(Ctx& c, const SweepOpts& o, int engine, float* q, size_t ldq, float* r, size_t ldr, const float* a, size_t lda, size_t m, size_t n) {
	// the fast form of the Gram kernel for the full 64-row blocks of a 128-column matrix, the general form for the rest (wide_gram_plan)
	const WideGramPlan wp = wide_gram_plan(m, n, lda);
	const size_t nfull = wp.nfull, nrest = wp.nrest;
	const int wgs_fast = wp.wgs_fast, wgs_rest = wp.wgs_rest;
	const int rca = wide_kernel_attrs(c.dev);
	if (rca) return rca;
	{
		ProfScope ps(KC_GRAM, c.st);
		tsqrmi::GramWideArgs ga = gram_wide_args(c, a, lda, m, n, (int)nfull);   // (the first launch carries the announcement)
		if (wgs_fast) {
			hipLaunchKernelGGL((tsqrmi::gram_wide_kernel<true>), dim3(wgs_fast), dim3(512), tsqrmi::GW_LDS_BYTES, c.st, ga);
			ga.announce = nullptr;
		}
		if (wgs_rest) {
			ga.blk0 = (int)nfull; ga.nblk = (int)nrest; ga.part += (size_t)wgs_fast * 36 * 256;
			hipLaunchKernelGGL((tsqrmi::gram_wide_kernel<false>), dim3(wgs_rest), dim3(512), tsqrmi::GW_LDS_BYTES, c.st, ga);
		}
	}
	HIPCHK(hipGetLastError());
	{
		ProfScope ps(KC_CHOL, c.st);
		launch_reduce1(c.st, wide_ws(c).gsum, reinterpret_cast<const double*>(c.wr), wgs_fast + wgs_rest, 36 * 256, (double)m);
		hipLaunchKernelGGL(tsqrmi::chol_wide_kernel, dim3(1), dim3(1024), 0, c.st, chol_wide_args(c, o, r, ldr, m, n));
	}
	HIPCHK(hipGetLastError());
	return apply_wide(c, o, engine, q, ldq, a, lda, m, n);
}

// A speculative two-sweep attempt of a reorthogonalised call (R1, R2: qr_two_sweeps) ends in an error (the return value), with the call finished
// (*next_level = LADDER_DONE: Q and R final, stream drained) or with nothing done (*next_level = L: A intact, the checked ladder goes on from level L).
constexpr int LADDER_DONE = -1;

// Round 4: CholeskyQR2 / shifted CholeskyQR3 on the bf16-split Gram matrix, decided on the device, no pass wasted.
//  sweep 1  Gram pass of A -> Cholesky under the RELAXED rule (another sweep follows: Q1 must come out well conditioned, not
//           orthonormal) -- and when even that rule rejects, the same launch factors G + s I at once (shifted Cholesky QR,
//           Fukaya et al. 2020).  s = c trace(G), c = 8 * 2^-23 / sqrt(rows): four times the Frobenius bound of the bf16-split Gram
//           matrix's own error (products good to 2^-23, errors averaging over the rows: |dG_ij| ~ 2^-22 / sqrt(rows) sqrt(g_ii g_jj),
//           measured as 8e-6 S / sqrt(rows) in Q^T Q), so the fp64 Gram pass of A (108 us) and its rejected Cholesky are not needed.
//           -> Q1 = A inverse(R1), Gram tiles of Q1 from the same launch; Q1 leaves with plain stores in ASCENDING block order, so
//           that sweep 2 (descending) starts with the half of Q1 the Infinity Cache still holds (ApplyArgs::forward).
//  The host reads sweep 1's verdict word WHILE the apply pass of sweep 1 runs, then enqueues
//  accepted plain   : sweep 2 under the strict rule -> Q, R = R2 R1 (CholeskyQR2: what rounds 1-3 did for such input);
//  accepted shifted : sweep 2 under the relaxed rule (cond(Q1) ~ 1 / sqrt(c): 1e3 .. 4e3) with Gram tiles of Q2 from its
//                     apply launch, sweep 3 under the strict rule -> Q, R = R3 R2 R1 (shifted CholeskyQR3);
//  rejected         : (non-finite input, or columns near the fp32 denormal range) the checked ladder, from the fp64 Gram level.
// Every launch behind a rejected Cholesky skips itself; A is never written.  (One panel, auto policy, pinned words.)
int two_sweeps_device_decided(Ctx& c, int engine, float* q, size_t ldq, float* r, size_t ldr, float* a, size_t lda, size_t m, size_t n, int* next_level) {
	constexpr unsigned PENDING = 0xffffffffu;
	volatile unsigned* hw = reinterpret_cast<volatile unsigned*>(c.hsig.host);
	float* r1 = c.wq + c.L.r1; float* r2 = c.wq + c.L.r2;
	float* r3 = c.wq + c.L.r5; float* r4 = c.wq + c.L.r6;    // (L.r3 / L.r4 belong to panel_qr's own shifted two-step)
	double* const gq = reinterpret_cast<double*>(c.wr); const int gq_cap = gram_plan(m, n).nblocks;   // Gram partials of a sweep's output, for the sweep behind it
	const bool q_back = (double)ldq * (double)n * sizeof(float) <= 300.0e6;      // (a Q the Infinity Cache can hold half of)
	*next_level = LADDER_DONE;
	hw[0] = PENDING;
	int nq1 = 0;                                         // partials of Q1^T Q1 (none from the fp32-MFMA engine: its apply launch is not fused)
	int rc = sweep(c, SweepOpts{/*slot=*/0, /*prev_slot=*/-1, /*gramq_ready=*/0, /*gramq_part=*/gq, /*gramq_cap=*/gq_cap, /*relax=*/1, /*retry_shift=*/1, /*q_read_back=*/q_back}, &nq1, engine, 2, /*check_now=*/false, q, ldq, r1, n, a, lda, m, n);
	if (rc) return rc;
	unsigned v0 = PENDING;                               // sweep 1's verdict (its apply pass is running meanwhile)
	const int seen = spin_until([&] { return (v0 = hw[0]) != PENDING; }, c.st);
	if (seen < 0) return seen;
	if (seen == 1 && (v0 = hw[0]) == PENDING) v0 = 1u;   // (the stream is idle and nothing reported: rejected)
	unsigned s1 = 1u, s2 = 1u;
	if (v0 == 0u) {
		rc = sweep(c, SweepOpts{/*slot=*/1, /*prev_slot=*/0, /*gramq_ready=*/nq1}, nullptr, engine, 2, /*check_now=*/false, q, ldq, r2, n, q, ldq, m, n);
		if (rc) return rc;
		launch_rmul(r, ldr, r2, n, r1, n, n, c.st);
		HIPCHK(hipGetLastError());
		rc = read_status(c, 1, &s1);
		if (rc || s1 == 0) return rc;                    // both sweeps accepted: done (min_level was set by panel_qr)
		// the first sweep stands (Q holds Q1, r1 is valid); only the second one must be redone, checked, one level down
		c.min_level = 2;
		rc = sweep(c, SweepOpts{}, nullptr, engine, 1, /*check_now=*/true, q, ldq, r2, n, q, ldq, m, n);
		if (rc) return rc;
		c.min_level = std::min(c.min_level, 2);
		launch_rmul(r, ldr, r2, n, r1, n, n, c.st);
		HIPCHK(hipGetLastError());
		return wait_done(c);
	}
	if (v0 == 2u) {
		// shifted: cond(Q1) ~ sqrt(c n / 3) cond(A).  Sweep 2 first tries the bf16-split Gram matrix of Q1 -- free, its tiles came out
		// of sweep 1's apply launch -- under the relaxed rule (large row counts: c is small enough for cond(A) up to ~1e8); when
		// that is rejected (Q still holds Q1: the apply pass skipped itself) it takes the fp64 Gram matrix of Q1 in a pass of its
		// own.  Sweeps 2 and 3 are enqueued together, speculatively; sweep 3 (strict rule) reuses slot 0, whose first verdict
		// has been read.
		bool done3 = false;
		for (int att = nq1 > 0 ? 0 : 1; att < 2; att++) {
			int nq2 = 0;                                 // partials of Q2^T Q2 (the same apply variant as in sweep 1: fused for every engine but the fp32-MFMA one)
			rc = sweep(c, SweepOpts{/*slot=*/1, /*prev_slot=*/-1, /*gramq_ready=*/att == 0 ? nq1 : 0, /*gramq_part=*/gq, /*gramq_cap=*/gq_cap, /*relax=*/1}, &nq2, engine, att == 0 ? 2 : 1, /*check_now=*/false,
			           q, ldq, r2, n, q, ldq, m, n);       // (no dependency: sweep 1 is known to be accepted)
			if (!rc) rc = sweep(c, SweepOpts{/*slot=*/0, /*prev_slot=*/1, /*gramq_ready=*/nq2}, nullptr, engine, 2, /*check_now=*/false, q, ldq, r3, n, q, ldq, m, n);
			if (rc) return rc;
			launch_rmul3(r, ldr, r3, r2, r1, r4, n, c.st);
			HIPCHK(hipGetLastError());
			rc = read_status(c, 0, &s2);
			if (!rc) rc = read_status(c, 1, &s1, nullptr, /*wait=*/false);
			if (rc) return rc;
			if (s1 == 0 && s2 == 0) { done3 = true; break; }
			if (s1 == 0) break;                          // sweep 3 alone was rejected: Q holds Q2 (checked sweep below)
		}
		if (!done3) {
			// Q1 is numerically rank deficient (e.g. exactly dependent columns), or sweep 3 found Q2 short of the strict rule.
			// Q holds Q1 (sweep 2 rejected: its apply pass skipped itself) or Q2 -- A may be gone (q may alias a), so the rest is
			// done on Q in place by checked sweeps, which escalate per panel (fp64 Gram -> shifted -> Householder)
			if (s1 != 0) {
				rc = sweep(c, SweepOpts{}, nullptr, engine, 1, /*check_now=*/true, q, ldq, r2, n, q, ldq, m, n);
				if (rc) return rc;
			}
			rc = sweep(c, SweepOpts{}, nullptr, engine, 2, /*check_now=*/true, q, ldq, r3, n, q, ldq, m, n);
			if (rc) return rc;
			launch_rmul3(r, ldr, r3, r2, r1, r4, n, c.st);
			HIPCHK(hipGetLastError());
			rc = wait_done(c);
			if (rc) return rc;
		}
		c.min_level = 0; c.used_shift = true;
		return 0;
	}
	rc = wait_done(c);                                   // rejected (non-finite input, columns near the denormal range): everything enqueued skipped itself
	if (rc) return rc;
	c.min_level = 2;
	*next_level = 1;                                     // the checked ladder, from the fp64 Gram level, on the untouched A
	return 0;
}

// Optimistic attempt: both sweeps at `level`, the R product and the completion flag are enqueued without looking at a verdict.
// Device-side chain: apply 1 skips when Cholesky 1 rejected; Cholesky 2 then reports "rejected" at once; apply 2 (in
// place) skips when Cholesky 2 rejected -- so A stays intact and Q holds Q1 or garbage, never a half-applied state.
// (One panel, auto policy; without pinned words, or with the fp64 Gram level first.)
int two_sweeps_optimistic(Ctx& c, int engine, int level, float* q, size_t ldq, float* r, size_t ldr, float* a, size_t lda, size_t m, size_t n, int* next_level) {
	float* r1 = c.wq + c.L.r1; float* r2 = c.wq + c.L.r2;
	const bool fuse = level == 2;                        // (as in qr_two_sweeps)
	*next_level = LADDER_DONE;
	int nq = 0;
	int rc = sweep(c, SweepOpts{/*slot=*/0, /*prev_slot=*/-1, /*gramq_ready=*/0, /*gramq_part=*/fuse ? reinterpret_cast<double*>(c.wr) : nullptr, /*gramq_cap=*/fuse ? gram_plan(m, n).nblocks : 0}, &nq, engine, level, /*check_now=*/false,
	               q, ldq, r1, n, a, lda, m, n);
	if (!rc) rc = sweep(c, SweepOpts{/*slot=*/1, /*prev_slot=*/0, /*gramq_ready=*/nq}, nullptr, engine, level, /*check_now=*/false, q, ldq, r2, n, q, ldq, m, n);
	if (rc) return rc;
	launch_rmul(r, ldr, r2, n, r1, n, n, c.st);
	HIPCHK(hipGetLastError());
	unsigned s0 = 1u, s1 = 1u;
	rc = read_status(c, 0, &s0);
	if (!rc) rc = read_status(c, 1, &s1, nullptr, /*wait=*/false);
	if (rc) return rc;
	if (s0 == 0 && s1 == 0) return 0;                    // both sweeps accepted: done (min_level was set by panel_qr)
	c.min_level = 2;
	if (s0 != 0) { *next_level = std::max(level - 1, 0); return 0; }   // first sweep rejected at this level: checked path from the next one
	// the first sweep stands (Q holds Q1, r1 is valid); only the second one must be redone, now checked and below
	// the level that was just rejected
	rc = sweep(c, SweepOpts{}, nullptr, engine, level - 1, /*check_now=*/true, q, ldq, r2, n, q, ldq, m, n);
	if (rc) return rc;
	c.min_level = std::min(c.min_level, level);          // (first sweep ran at `level`)
	launch_rmul(r, ldr, r2, n, r1, n, n, c.st);
	HIPCHK(hipGetLastError());
	return wait_done(c);
}

// two sweeps: A = Q1 R1, then Q1 = Q R2 in place, R = R2 * R1 (the reference's BCGS2 plays this role).  R1 and R2 live in
// the work buffer (packed, ld n); every sweep writes their upper triangles in full and rmul_kernel reads nothing else,
// so neither needs zero-filling, and the product is written straight into the caller's r (zeros below the diagonal)
int qr_two_sweeps(Ctx& c, int engine, int level, int first_level, bool check_now, float* q, size_t ldq, float* r, size_t ldr, float* a, size_t lda, size_t m, size_t n) {
	const bool one_panel_auto = n <= PW && c.policy == 0;
	if (one_panel_auto && level == first_level && !t_prof.on) {
		int next = LADDER_DONE;
		const int rc = (level == 2 && c.hsig.dev) ? two_sweeps_device_decided(c, engine, q, ldq, r, ldr, a, lda, m, n, &next)
		                                          : two_sweeps_optimistic(c, engine, level, q, ldq, r, ldr, a, lda, m, n, &next);
		if (rc || next == LADDER_DONE) return rc;
		level = next;
	}
	float* r1 = c.wq + c.L.r1; float* r2 = c.wq + c.L.r2;
	// single panel: the first sweep's (last) apply launch accumulates Q^T Q while the block is in LDS, so that the second
	// sweep's bf16-level Gram pass over Q is not needed
	const bool fuse = one_panel_auto && first_level == 2;
	int nq = 0;
	int rc = sweep(c, SweepOpts{/*slot=*/0, /*prev_slot=*/-1, /*gramq_ready=*/0, /*gramq_part=*/fuse ? reinterpret_cast<double*>(c.wr) : nullptr, /*gramq_cap=*/fuse ? gram_plan(m, n).nblocks : 0}, &nq, engine, level, check_now,
	               q, ldq, r1, n, a, lda, m, n);
	if (rc) return rc;
	// the second sweep always starts at the first level again (Q1 is well conditioned)
	rc = sweep(c, SweepOpts{/*slot=*/0, /*prev_slot=*/-1, /*gramq_ready=*/nq}, nullptr, engine, first_level, check_now, q, ldq, r2, n, q, ldq, m, n);
	if (rc) return rc;
	launch_rmul(r, ldr, r2, n, r1, n, n, c.st);
	HIPCHK(hipGetLastError());
	return wait_done(c);                                 // completion flag in the pinned words, or a plain stream sync
}

// The auto load policy (tsqr_mi_set_load_policy, resolve_load_policy), measured once per process and device by the first blocking call
// that is eligible: a full 64-column fp32_tc_cor call of at least 128 MiB, out of place, accepted at the bf16-split level, no profiling.
// What a policy changes is what one call's passes leave in the Infinity Cache for the NEXT call's Gram pass, so the unit timed is the call
// sequence -- Gram pass, reduction, Cholesky, apply pass on the caller's operands, with the block shares already chosen -- and never a
// single pass: the two arms take turns in runs of two sequences (1 1 2 2 1 1 2 2 ...) and only the second sequence of a run counts, the
// first inherits the other arm's cache state.  The streamed policy is taken when its mean is below the cache-allocating arm's by more
// than the larger of 3 % and that arm's own max - min.  Every sequence writes the same Q, R and verdict (the policy does not touch the
// arithmetic): the last one leaves the result.  ~2.3 ms once.  Leaves the stream idle.
void measure_load_policy(Ctx& c, int engine, float* q, size_t ldq, float* r, size_t ldr, float* a, size_t lda, size_t m, size_t n) {
	constexpr int RUNS = 3, NSEQ = 4 * RUNS;
	hipEvent_t ev[NSEQ + 1];
	bool ok = true;
	for (auto& e : ev) ok = ok && hipEventCreate(&e) == hipSuccess;
	int choice = 1;
	if (ok) {
		for (int i = 0; i < NSEQ && ok; i++) {
			SweepOpts o{};
			o.load_policy = ((i >> 1) & 1) ? 2 : 1;
			(void)hipEventRecord(ev[i], c.st);
			ok = sweep(c, o, nullptr, engine, 2, /*check_now=*/false, q, ldq, r, ldr, a, lda, m, n) == 0;
		}
		(void)hipEventRecord(ev[NSEQ], c.st);
		ok = (hipEventSynchronize(ev[NSEQ]) == hipSuccess) && ok;
		float sum[2] = {0.f, 0.f}, lo = 1e30f, hi = 0.f;
		for (int i = 1; i < NSEQ && ok; i += 2) {
			float ms = 0.f;
			ok = hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess;
			const int arm = (i >> 1) & 1;
			sum[arm] += ms;
			if (arm == 0) { lo = std::min(lo, ms); hi = std::max(hi, ms); }
			if (g_set.debug) fprintf(stderr, "[tsqr_mi] load policy %d: sequence %.4f ms\n", arm + 1, ms);
		}
		if (ok) {
			const float mean1 = sum[0] / RUNS, mean2 = sum[1] / RUNS;
			if (mean2 < mean1 - std::max(0.03f * mean1, hi - lo)) choice = 2;
			if (g_set.debug) fprintf(stderr, "[tsqr_mi] load policy: cache-allocating %.4f ms (spread %.4f), streamed %.4f ms -> %d\n", mean1, hi - lo, mean2, choice);
		}
	} else {
		(void)hipStreamSynchronize(c.st);
	}
	for (auto& e : ev) (void)hipEventDestroy(e);
	(void)hipGetLastError();
	g_load_policy_chosen[c.dev].store(choice);           // (a measurement that failed is not asked for again: the policy stays what it was)
}

// ---------------------------------------------------------------------------------------------------------------------------
// the whole factorisation (single GPU: comm inactive; row-partitioned: this rank's block)
// ---------------------------------------------------------------------------------------------------------------------------
int qr_core(Ctx& c, int engine, int reorth, float* q, size_t ldq, float* r, size_t ldr, float* a, size_t lda, size_t m, size_t n) {
	const WqLayout& L = c.L;
	const SweepOpts plain{};                             // every sweep enqueued here: slot 0, no dependency, nothing fused (the two-sweep schedules build their own)
	c.fold_cor = (engine == 1);
	// auto policy: every mode starts at the bf16-split Gram level (exact products, fp64 accumulation across K-steps: more accurate
	// than any plain fp32 evaluation of A^T A, accepted only for well-conditioned panels), then the fp64 Gram level, the shifted
	// Cholesky QR step and the Householder fold; the mode selects the MFMA engine of the apply pass.  Policy 4 skips the bf16 level.
	const bool use_gram = (c.policy == 2) || (c.policy == 0);
	const bool may_fall_back = use_gram && c.policy == 0;
	// single panel, single sweep: run speculatively and look at the status at the final wait (A is untouched for n <= 64);
	// otherwise (several panels or a second sweep consuming Q) verify each panel right away.
	const bool deferred = may_fall_back && n <= PW && !reorth;
	const bool check_now = may_fall_back && !deferred;
	const unsigned gb = (unsigned)std::min<size_t>(1024, cdiv(n * n, 256));
	c.min_level = 2;
	c.used_shift = c.used_householder = false;
	float scond1 = 0.0f;                                 // scaled conditioning S reported by the accepted first sweep (single panel)

	// R-factor engine levels: 2 bf16-split Gram (memory-bound), 1 fp64 Gram, 0 Householder TSQR.  Deferred mode runs a level
	// speculatively and steps down when chol16_kernel rejected it; with check_now panel_qr escalates per panel by itself.
	const int first_level = !use_gram ? 0 : c.gram_level;
	bool wide_done = false;
	if (c.wide && n > PW && n <= 2 * PW && may_fall_back && first_level == 2 && !c.comm.active() && !c.resume_accepted) {
		// one Cholesky-QR panel over all n columns; rejected (ill conditioned) -> the 64-column panel path below, A is still intact
		float* r1 = c.wq + L.r1; float* r2 = c.wq + L.r2;
		unsigned st = 1u;
		int rc = sweep_wide(c, plain, engine, q, ldq, reorth ? r1 : r, reorth ? n : ldr, a, lda, m, n);
		if (rc) return rc;
		rc = read_status(c, 0, &st);
		if (rc) return rc;
		if (st == 0 && reorth) {
			rc = sweep_wide(c, plain, engine, q, ldq, r2, n, q, ldq, m, n);
			if (rc) return rc;
			rc = read_status(c, 0, &st);
			if (rc) return rc;
			if (st != 0) {                               // (Q1 is well conditioned: not expected) second sweep on the panel path
				rc = sweep(c, plain, nullptr, engine, first_level, /*check_now=*/true, q, ldq, r2, n, q, ldq, m, n);
				if (rc) return rc;
				hipLaunchKernelGGL(tsqrmi::zero_lower_kernel, dim3(gb), dim3(256), 0, c.st, r2, n, (int)n);
			}
			launch_rmul(r, ldr, r2, n, r1, n, n, c.st);
			HIPCHK(hipGetLastError());
			rc = wait_done(c);
			if (rc) return rc;
			st = 0;
		}
		wide_done = (st == 0);
	}
	if (c.resume_accepted) scond1 = c.resume_scond;
	int level = c.start_level >= 0 ? std::min(c.start_level, first_level) : first_level;
	if (wide_done || c.resume_accepted) level = -1;      // (nothing left for the ladder)
	if (reorth && level >= 0) {
		const int rc = qr_two_sweeps(c, engine, level, first_level, check_now, q, ldq, r, ldr, a, lda, m, n);
		if (rc) return rc;
		level = -1;
	}
	for (; level >= 0; level--) {
		// level 0 reached in the speculative (deferred) mode: both Gram levels were rejected and the fp64 Gram matrix of A is
		// still in the work buffer: panel_qr takes the shifted-Cholesky path on it before the Householder fold
		const bool retry_checked = (level == 0 && deferred && first_level >= 1);
		int rc = sweep(c, plain, nullptr, engine, retry_checked ? R_SHIFT_DIRECT : level, check_now || retry_checked, q, ldq, r, ldr, a, lda, m, n);
		if (rc) return rc;
		if (n > PW) hipLaunchKernelGGL(tsqrmi::zero_lower_kernel, dim3(gb), dim3(256), 0, c.st, r, ldr, (int)n);
		HIPCHK(hipGetLastError());
		if (level > 0 && deferred) {
			unsigned status = 0;
			rc = read_status(c, 0, &status, &scond1);
			if (rc) return rc;
			if (status != 0) { c.min_level = 2; continue; }       // rejected: step down and redo
			// the accepted first large blocking call of the process on this device measures the load policy (the share measurement of its
			// apply pass has run by now); submit / batch entries never come here: they use what was chosen, or the cache-allocating loads
			if (level == 2 && engine == 1 && q != a && !t_prof.on && !c.comm.active() && g_set.load_policy.load() == 0 &&
			    g_load_policy_chosen[c.dev].load() == 0 && (double)m * (double)n * sizeof(float) >= LOAD_POLICY_MIN_BYTES && blk_gram_ok(a, lda, m, n))
				measure_load_policy(c, engine, q, ldq, r, ldr, a, lda, m, n);
		} else {
			rc = wait_done(c);                           // completion flag in the pinned words, or a plain stream sync
			if (rc) return rc;
		}
		break;
	}
	// n <= 16 without reorthogonalisation: the reference's tsqr16 builds Q from its Householder tree and stays O(eps) orthogonal at
	// any conditioning, while Q = A * inverse(R) loses orthogonality like cond * eps.  When the accepted sweep reports a scaled
	// conditioning beyond 32 (measured loss ~ 3.6e-7 * sqrt(S)), a second sweep on Q in place restores O(eps): R <- R2 * R.
	if (!reorth && deferred && n <= 16 && c.min_level >= 1 && !c.used_shift && !c.used_householder && scond1 > 32.0f) {
		float* r1 = c.wq + L.r1; float* r2 = c.wq + L.r2;
		hipLaunchKernelGGL(tsqrmi::copy2d_kernel, dim3(gb), dim3(256), 0, c.st, r1, n, r, ldr, (int)n, (int)n);
		HIPCHK(hipGetLastError());
		int rc = sweep(c, plain, nullptr, engine, first_level, /*check_now=*/true, q, ldq, r2, n, q, ldq, m, n);
		if (rc) return rc;
		launch_rmul(r, ldr, r2, n, r1, n, n, c.st);
		HIPCHK(hipGetLastError());
		rc = wait_done(c);
		if (rc) return rc;
	}
	t_last_engine = !use_gram ? 0 : (c.used_householder ? 2 : (c.used_shift ? 4 : (c.min_level == 2 ? 3 : (c.min_level == 1 ? 1 : 2))));
	if (wide_done) t_last_engine = 5;                    // all n <= 128 columns as one Cholesky-QR panel (bf16-split Gram level)
	prof_collect();
	return TSQR_MI_SUCCESS;
}

void init_ctx(Ctx& c, void* wq, void* wr, size_t m_layout, size_t n, void* stream, bool keep_in_flight = false) {
	// every entry point starts here: calls of this thread still in flight (submit without finish) have their verdicts read first --
	// what follows may reuse their pinned words and status slots
	if (!keep_in_flight) (void)latch_all();
	c.st = reinterpret_cast<hipStream_t>(stream);
	c.dev = cur_device();
	c.wq = reinterpret_cast<float*>(wq);
	c.wr = reinterpret_cast<float*>(wr);
	c.L = wq_layout(m_layout, n);
	c.cross_slots = cross_slots(m_layout, n);
	c.policy = g_set.policy.load();
	c.gram_level = g_set.gram_level.load();
	c.wide = g_set.wide.load() != 0;
}

size_t working_r_need(size_t m, size_t n) {
	size_t need = 0;
	for (size_t P = 0; P < n; P += PW) {
		need = std::max(need, make_plan(m, std::min(PW, n - P)).stack_a);
		need = std::max(need, (n <= PW ? 2 : 1) * gram_plan(m, std::min(PW, n - P)).part_floats);   // (n <= 64: two sets, stream_of_calls_chained)
		if (n > PW) need = std::max(need, cross_slots(m, n) * 16 * 256 * 2);   // (coupling partials: sweep)
	}
	if (n > PW) need = std::max(need, wide_part_floats(m));   // (sweep_wide: the whole matrix for n <= 128, 128-column blocks of the panel loop beyond)
	return need;
}

int qr_dist_common(Ctx& c, int mode, int reorth, float* q, size_t ldq, float* r, size_t ldr, float* a, size_t lda, size_t m_local, size_t n,
                   void* wq, void* wr, int nranks, void* stream) {
	// (n > 64: 64-column panels coupled by block Gram-Schmidt, every coupling coefficient block all-reduced like the Gram tiles; the
	// one-panel path for 64 < n <= 128 is a single-GPU path)
	if (m_local == 0 || n == 0 || nranks < 1) return TSQR_MI_ERROR_INVALID_SIZE;
	const int engine = engine_of(mode);
	if (engine < 0) { t_last_error = "compute_mode not implemented on gfx950"; return TSQR_MI_ERROR_UNSUPPORTED; }
	init_ctx(c, wq, wr, std::max(m_local, (size_t)nranks * std::min(n, PW)), n, stream);
	c.comm.nranks = nranks;
	c.rows_global = (double)m_local * (double)nranks;    // host-side estimate only: the device thresholds use the all-reduced count
	resolve_host_sig(c, nullptr, m_local);
	return qr_core(c, engine, reorth, q, ldq, r, ldr, a, lda, m_local, n);
}

}  // namespace

extern "C" {

int tsqr_mi_version(void) { return 410; }
const char* tsqr_mi_last_error(void) { return t_last_error.c_str(); }

size_t tsqr_mi_batch_size_log2(size_t m) { return ref_bs_log2(m); }
size_t tsqr_mi_batch_size(size_t m) { return ref_bs(m); }

size_t tsqr_mi_working_q_size(size_t m, size_t n) {
	if (m == 0 || n == 0) return 0;
	return std::max(ref_wq(m, n), wq_layout(m, n).total);
}
size_t tsqr_mi_working_r_size(size_t m, size_t n) {
	if (m == 0 || n == 0) return 0;
	return std::max(ref_wr(m, n), working_r_need(m, n));
}
size_t tsqr_mi_working_l_size(size_t m) { return m == 0 ? 0 : std::max<size_t>(ref_bs(m) + 1, 8); }   // 8 words: status words + completion flag
size_t tsqr_mi_working_reorth_size(size_t m) { return 16 * 16 * 2 + m * 16; }

// row-partitioned call: the work buffers must also hold the restacked (nranks n) x n matrix of gathered R factors and its fold
size_t tsqr_mi_working_q_size_dist(size_t m_local, size_t n, int nranks) {
	if (m_local == 0 || n == 0 || nranks < 1) return 0;
	return tsqr_mi_working_q_size(std::max(m_local, (size_t)nranks * std::min(n, PW)), n);
}
size_t tsqr_mi_working_r_size_dist(size_t m_local, size_t n, int nranks) {
	if (m_local == 0 || n == 0 || nranks < 1) return 0;
	const size_t pc = std::min(n, PW);                   // (the gathered stack is one panel's: nranks * pc rows of pc columns)
	const size_t stack = (((size_t)nranks * pc * pc + 63) & ~(size_t)63) + make_plan((size_t)nranks * pc, pc).stack_a;
	return std::max(tsqr_mi_working_r_size(std::max(m_local, (size_t)nranks * pc), n), std::max(working_r_need(m_local, n), stack));
}

void tsqr_mi_profile_enable(int on) {
	if (on && !t_prof.created) {
		for (int i = 0; i < 2 * Prof::MAXEV; i++) (void)hipEventCreate(&t_prof.ev[i]);
		t_prof.created = true;
	}
	t_prof.on = on != 0;
	t_prof.n = 0;
	for (int k = 0; k < KC_COUNT; k++) { t_prof.ms[k] = 0; t_prof.launches[k] = 0; }
}
int tsqr_mi_profile_read(double* ms, long* launches, int max_classes) {
	prof_collect();
	const int k = std::min(max_classes, (int)KC_COUNT);
	for (int i = 0; i < k; i++) { ms[i] = t_prof.ms[i]; launches[i] = t_prof.launches[i]; }
	return k;
}

void tsqr_mi_set_policy(int policy) {
	switch (policy) {
		case 0: g_set.policy = 0; g_set.gram_level = 2; g_set.wide = 1; break;    // auto
		case 5: g_set.policy = 0; g_set.gram_level = 2; g_set.wide = 0; break;    // auto, 64-column panels only (no one-panel path for n <= 128)
		case 1: g_set.policy = 1; g_set.gram_level = 2; break;    // always Householder TSQR
		case 2: g_set.policy = 2; g_set.gram_level = 1; break;    // always fp64 Gram (no fallback)
		case 3: g_set.policy = 2; g_set.gram_level = 2; break;    // always bf16-split Gram (no check, no fallback)
		case 4: g_set.policy = 0; g_set.gram_level = 1; break;    // auto without the bf16-split level
		default: break;
	}
}
int tsqr_mi_last_engine(void) { return t_last_engine; }

void tsqr_mi_set_tuning(int level0_waves, int tree_chunks_per_wave) {
	if (level0_waves > 0) g_set.level0_waves = level0_waves;
	if (tree_chunks_per_wave > 1) g_set.tree_cpw = tree_chunks_per_wave;
}
void tsqr_mi_set_load_policy(int p) { g_set.load_policy = clamp_load_policy(p); }
int tsqr_mi_get_load_policy(void) { return g_load_policy_used.load(); }
void tsqr_mi_set_tuning2(int gram_waves, int apply_waves) {
	if (gram_waves > 0) g_set.gram_waves = gram_waves;
	if (apply_waves > 0) g_set.apply_wgs = std::max(1, apply_waves / 4);   // the apply kernel is launched as a persistent grid of workgroups (4 waves each)
}

int tsqr_mi_qr_f32(int mode, int reorth, float* q, size_t ldq, float* r, size_t ldr, float* a, size_t lda,
                   size_t m, size_t n, void* wq_v, void* wr_v, float* reorth_w, unsigned* d_wl, unsigned* h_wl,
                   void* stream) {
	(void)reorth_w; (void)d_wl;
	if (n > m || m == 0 || n == 0) return TSQR_MI_ERROR_INVALID_SIZE;     // reference src/blockqr.cu:409-411
	const int engine = engine_of(mode);
	if (engine < 0) { t_last_error = "compute_mode not implemented on gfx950"; return TSQR_MI_ERROR_UNSUPPORTED; }
	Ctx c;
	init_ctx(c, wq_v, wr_v, m, n, stream);
	c.rows_global = (double)m;
	resolve_host_sig(c, h_wl, m);
	return qr_core(c, engine, reorth, q, ldq, r, ldr, a, lda, m, n);
}

// ---- submit / finish: the first attempt of a call (bf16-split Gram level, everything speculative) is enqueued and the host returns;
// finish reads the verdict and, for a rejected matrix, runs the rest of the ladder as the blocking call does (include/tsqr_mi.h) ----
// CallEnv: what a row-partitioned call adds to the arguments (its collectives); env.dist == false: the single-GPU call.
struct CallEnv { bool dist = false; Comm comm; int nranks = 1; };
static void env_ctx(Ctx& c, const CallEnv& env, void* wq_v, void* wr_v, size_t m, size_t n, unsigned* h_wl, void* stream, bool keep_in_flight) {
	if (env.dist) {                                      // (as qr_dist_common)
		c.comm = env.comm;
		init_ctx(c, wq_v, wr_v, std::max(m, (size_t)env.nranks * std::min(n, PW)), n, stream, keep_in_flight);
		c.comm.nranks = env.nranks;
		c.rows_global = (double)m * (double)env.nranks;
		resolve_host_sig(c, nullptr, m);
	} else {
		init_ctx(c, wq_v, wr_v, m, n, stream, keep_in_flight);
		c.rows_global = (double)m;
		resolve_host_sig(c, h_wl, m);
	}
}
// own_flag: a one-thread completion kernel behind the attempt (the public entry: always).  The loop entries leave it out for every call
// but the last and let the NEXT call's first kernel raise the word instead (`announce`: the ticket submitted just before this one).
static int submit_impl(const CallEnv& env, int mode, int reorth, float* q, size_t ldq, float* r, size_t ldr, float* a, size_t lda,
                       size_t m, size_t n, void* wq_v, void* wr_v, unsigned* h_wl, void* stream, tsqr_mi_ticket* t,
                       tsqr_mi_ticket* announce, bool own_flag) {
	if (!t) return TSQR_MI_ERROR_INVALID_SIZE;
	*t = tsqr_mi_ticket{};
	t->mode = mode; t->reorth = reorth; t->q = q; t->r = r; t->a = a; t->ldq = ldq; t->ldr = ldr; t->lda = lda; t->m = m; t->n = n;
	t->wq = wq_v; t->wr = wr_v; t->stream = stream; t->h_wl = h_wl;
	if ((!env.dist && n > m) || m == 0 || n == 0 || env.nranks < 1) return t->state = TSQR_MI_ERROR_INVALID_SIZE;
	const int engine = engine_of(mode);
	if (engine < 0) { t_last_error = "compute_mode not implemented on gfx950"; return t->state = TSQR_MI_ERROR_UNSUPPORTED; }
	Ctx c;
	env_ctx(c, env, wq_v, wr_v, m, n, h_wl, stream, /*keep_in_flight=*/true);
	const bool narrow = n <= PW, wide = c.wide && n > PW && n <= 2 * PW && !env.dist;
	if (!(c.policy == 0 && c.gram_level == 2 && !reorth && (narrow || wide) && c.hsig.dev && !t_prof.on && !g_set.debug)) {
		// no speculative first attempt for this call: run it here (finish returns its state)
		const int rc = latch_all();
		return t->state = rc ? rc : qr_core(c, engine, reorth, q, ldq, r, ldr, a, lda, m, n);
	}
	const int slot = (int)(t_submits++ & 1u);
	if (t_pending[slot]) { const int rc = ticket_latch(t_pending[slot]); if (rc) return t->state = rc; }
	c.fold_cor = (engine == 1);
	c.min_level = 2;
	if (announce && announce->pending == 1 && !announce->own_flag) {
		if (announce->words == c.hsig.host && announce->stream == stream) {
			c.announce_word = c.hsig.dev + 4 * announce->slot + 3;
			c.announce_seq = announce->seq;
		} else {                                         // other pinned words or another stream: a completion kernel of its own after all
			hipLaunchKernelGGL(tsqrmi::host_flag_kernel, dim3(1), dim3(1), 0, reinterpret_cast<hipStream_t>(announce->stream),
			                   announce->words_dev + 4 * announce->slot + 3, announce->seq);
			(void)hipGetLastError();
		}
	}
	const SweepOpts o{slot};                             // (the ticket's half of the status words, no dependency)
	const int rc = narrow ? sweep(c, o, nullptr, engine, 2, /*check_now=*/false, q, ldq, r, ldr, a, lda, m, n) : sweep_wide(c, o, engine, q, ldq, r, ldr, a, lda, m, n);
	if (rc) return t->state = rc;
	if (c.announce_word) {                               // (no kernel of the attempt carried the announcement: raise the word here)
		raise_announcement(c);
		(void)hipGetLastError();
	}
	unsigned seq = ++g_seq;
	if (seq == 0) seq = ++g_seq;
	reinterpret_cast<volatile unsigned*>(c.hsig.host)[4 * slot + 3] = 0;
	if (own_flag) {
		hipLaunchKernelGGL(tsqrmi::host_flag_kernel, dim3(1), dim3(1), 0, c.st, c.hsig.dev + 4 * slot + 3, seq);
		if (hipGetLastError() != hipSuccess) {           // the attempt is enqueued but cannot announce itself: drain and run the call
			HIPCHK(hipStreamSynchronize(c.st));
			return t->state = qr_core(c, engine, reorth, q, ldq, r, ldr, a, lda, m, n);
		}
	}
	t->slot = slot; t->seq = seq; t->words = c.hsig.host; t->words_dev = c.hsig.dev; t->own_flag = own_flag ? 1 : 0; t->pending = 1;
	t_pending[slot] = t;
	return TSQR_MI_SUCCESS;
}
// the tickets of the public entry this thread has not finished yet, in submission order
thread_local std::vector<tsqr_mi_ticket*> t_open;
static tsqr_order::Operands ticket_ops(const tsqr_mi_ticket* t) {
	return tsqr_order::operands(t->q, t->ldq, t->r, t->ldr, t->a, t->lda, t->m, t->n, sizeof(float));
}
static int finish_impl(const CallEnv& env, tsqr_mi_ticket* t);
int tsqr_mi_qr_f32_submit(int mode, int reorth, float* q, size_t ldq, float* r, size_t ldr, float* a, size_t lda,
                          size_t m, size_t n, void* wq_v, void* wr_v, float* reorth_w, unsigned* d_wl, unsigned* h_wl,
                          void* stream, tsqr_mi_ticket* t) {
	(void)reorth_w; (void)d_wl;
	if (!t) return TSQR_MI_ERROR_INVALID_SIZE;
	// a call that conflicts with a ticket still open (stream_order.h) must not be enqueued before that ticket is finished: finish the open
	// tickets up to the last conflicting one here (the same thread, in submission order); their own finish then returns the state
	const tsqr_order::Operands me = tsqr_order::operands(q, ldq, r, ldr, a, lda, m, n, sizeof(float));
	size_t upto = 0;
	for (size_t k = 0; k < t_open.size(); k++)
		if (tsqr_order::conflict(ticket_ops(t_open[k]), me)) upto = k + 1;
	for (size_t k = 0; k < upto; k++) {
		tsqr_mi_ticket* o = t_open.front();
		t_open.erase(t_open.begin());
		const int rc = finish_impl(CallEnv{}, o);
		if (rc < 0) { *t = tsqr_mi_ticket{}; return t->state = rc; }
	}
	const int rc = submit_impl(CallEnv{}, mode, reorth, q, ldq, r, ldr, a, lda, m, n, wq_v, wr_v, h_wl, stream, t, nullptr, /*own_flag=*/true);
	if (!rc && t->pending) t_open.push_back(t);
	return rc;
}

static int finish_impl(const CallEnv& env, tsqr_mi_ticket* t) {
	if (!t) return TSQR_MI_ERROR_INVALID_SIZE;
	if (t->pending == 0) return t->state;
	if (t->pending == 1) { const int rc = ticket_latch(t); if (rc) { t->pending = 0; return t->state = rc; } }
	t->pending = 0;
	const bool wide = t->n > PW;
	if (t->verdict == 0 && !(t->n <= 16 && t->scond > 32.0f)) {
		t_last_engine = wide ? 5 : 3;                    // accepted at the bf16-split Gram level: Q and R are in place
		return t->state = TSQR_MI_SUCCESS;
	}
	// rejected (or the n <= 16 second sweep is due): the blocking path from here on; calls submitted after this one have run their
	// attempts by the time anything below executes (stream order) and init_ctx reads their verdicts before their slots are reused
	Ctx c;
	env_ctx(c, env, t->wq, t->wr, t->m, t->n, t->h_wl, t->stream, /*keep_in_flight=*/false);
	if (t->verdict == 0) { c.resume_accepted = true; c.resume_scond = t->scond; }
	else if (wide) c.wide = false;                       // the one-panel attempt was rejected: 64-column panels (A is intact)
	else c.start_level = 1;                              // the bf16-split level was rejected: the ladder resumes at the fp64 Gram level
	return t->state = qr_core(c, engine_of(t->mode), t->reorth, t->q, t->ldq, t->r, t->ldr, t->a, t->lda, t->m, t->n);
}
int tsqr_mi_qr_f32_finish(tsqr_mi_ticket* t) {
	for (size_t k = 0; k < t_open.size(); k++)
		if (t_open[k] == t) { t_open.erase(t_open.begin() + k); break; }
	return finish_impl(CallEnv{}, t);
}

}  // extern "C"

namespace {

// ---- a stream of calls: `count` factorisations of ONE shape on one stream with one set of work buffers.  The loop entries pass the same
// (q, r, a) every time (the reference's speed protocol, src/test.cu:299-309), the batch entry one triple per call (a caller with many
// matrices, reference README.md:52-87 in a loop).  Mats hides the difference; Call carries what all calls of the stream share. ----
constexpr int NOT_MINE = -1000000;                     // "this schedule is not for this stream of calls; nothing enqueued" (not a hipError_t)
struct Mats {
	float* const* qs = nullptr; float* const* rs = nullptr; float* const* as = nullptr;   // host arrays of device pointers (batch entries) ...
	float* q0 = nullptr; float* r0 = nullptr; float* a0 = nullptr;                        // ... or one triple for every call (loop entries)
	int* states = nullptr;                               // optional: the state of every call
	bool same() const { return as == nullptr; }
	float* q(int i) const { return qs ? qs[i] : q0; }
	float* r(int i) const { return rs ? rs[i] : r0; }
	float* a(int i) const { return as ? as[i] : a0; }
	void state(int i, int st) const { if (states) states[i] = st; }
	Mats from(int i) const {
		Mats t = *this;
		if (!same()) { t.qs += i; t.rs += i; t.as += i; }
		if (states) t.states += i;
		return t;
	}
};
static Mats one_triple(float* q, float* r, float* a) {
	Mats mt;
	mt.q0 = q; mt.r0 = r; mt.a0 = a;
	return mt;
}
static int triple_per_call(Mats& mt, int count, float* const* q, float* const* r, float* const* a, int* states) {
	if (count < 0 || (count > 0 && (!q || !r || !a))) return TSQR_MI_ERROR_INVALID_SIZE;
	mt.qs = q; mt.rs = r; mt.as = a; mt.states = states;
	return 0;
}
struct Call { int mode, reorth; size_t ldq, ldr, lda, m, n; void* wq; void* wr; unsigned* h_wl; void* stream; };

// Every schedule that enqueues call i + 1 before call i is finished follows one rule (stream_order.h): calls i and i + 1 must not conflict.
static tsqr_order::Operands ops_of(const Mats& mt, int i, const Call& cl, size_t esz) {
	return tsqr_order::operands(mt.q(i), cl.ldq, mt.r(i), cl.ldr, mt.a(i), cl.lda, cl.m, cl.n, esz);
}
// calls i and i + 1 of a batch conflict (a loop over one triple: never -- see out_of_order below)
static bool pair_conflicts(const Mats& mt, int count, int i, const Call& cl, size_t esz = sizeof(float)) {
	return !mt.same() && i + 1 < count && tsqr_order::conflict(ops_of(mt, i, cl, esz), ops_of(mt, i + 1, cl, esz));
}
// The chained schedules launch the Gram pass of call i + 1 BEFORE the apply pass of call i: a batch takes them only when no pair of its calls
// conflicts.  A loop over one triple takes them only when the triple does not feed itself (Q or R overlaps A, e.g. q == a: call i + 1 of
// the blocking loop factors the Q that call i left there); it keeps two calls in flight even then, because a rejected call leaves A untouched
// and the next attempt, rejected alike, is redone (two_in_flight).
static bool out_of_order(const Mats& mt, int count, const Call& cl, size_t esz = sizeof(float)) {
	if (mt.same()) { const tsqr_order::Operands o = ops_of(mt, 0, cl, esz); return !tsqr_order::feeds(o, o); }
	for (int i = 0; i + 1 < count; i++)
		if (pair_conflicts(mt, count, i, cl, esz)) return false;
	return true;
}

// A batch of different matrices takes a chained schedule only while two matrices share the Infinity Cache (Settings::chain_max_mib)
static bool chain_fits_cache(const Mats& mt, const Call& cl, size_t esz = sizeof(float)) {
	return mt.same() || (double)cl.lda * (double)cl.n * esz <= (double)g_set.chain_max_mib * 1048576.0;
}
// the chained Gram kernels read A in 16-byte pieces
static bool a_aligned16(const Mats& mt, int count) {
	for (int i = 0; i < (mt.same() ? 1 : count); i++)
		if ((reinterpret_cast<uintptr_t>(mt.a(i)) & 15) != 0) return false;
	return true;
}

// The completion-word protocol of a stream of calls.  Call i owns half i & 1 of the pinned words: its Cholesky kernel writes the verdict
// into word 0 of the half, and word 3 is raised to the call's sequence number when its last kernel has finished -- by the Gram launch of
// call i + 1 (stream order: it starts then; a one-thread kernel less per call), or by a one-thread kernel behind the last call.  The
// announcement waits in Ctx::announce_word, where gram_g and sweep_wide find it as well as the schedules' own Gram launches.
struct Completion {
	Ctx& c;
	volatile unsigned* words;
	unsigned seq[2] = {0, 0};
	explicit Completion(Ctx& ctx) : c(ctx), words(reinterpret_cast<volatile unsigned*>(ctx.hsig.host)) {}
	// behind the last launch of call i: a fresh non-zero sequence number for its word, announced by call i + 1 or (the last call) here
	int close(int i, bool last) {
		unsigned sq = ++g_seq;
		if (sq == 0) sq = ++g_seq;
		seq[i & 1] = sq;
		words[4 * (i & 1) + 3] = 0;
		c.announce_word = c.hsig.dev + 4 * (i & 1) + 3; c.announce_seq = sq;
		if (last) raise_announcement(c);
		HIPCHK(hipGetLastError());
		return 0;
	}
	int wait(int i) const { return wait_word(words + 4 * (i & 1) + 3, seq[i & 1], c.st); }
	bool rejected(int i) const { return words[4 * (i & 1)] != 0; }       // (after wait(i), or on an idle stream)
};

// The issue-ahead loop of every schedule: step(i) enqueues the launches of call i and closes it (Completion::close); the host stays one
// call ahead of the call it waits for.  A rejected verdict ends the schedule with tail(i) -- the schedule's own policy for call i and the
// ones behind it; *done = accepted calls so far.  `engine` is what tsqr_mi_last_engine reports after a stream of accepted calls.
template <class Step, class Tail>
static int run_chained(const Completion& comp, const Mats& mt, int count, int engine, Step step, Tail tail, int* done) {
	int rc = step(0);
	if (rc) return rc;
	for (int i = 0; i < count; i++) {
		if (i + 1 < count) { rc = step(i + 1); if (rc) return rc; }
		rc = comp.wait(i);
		if (rc) return rc;
		if (comp.rejected(i)) return tail(i);
		mt.state(i, TSQR_MI_SUCCESS);
		*done = i + 1;
	}
	t_last_engine = engine;
	prof_collect();
	return TSQR_MI_SUCCESS;
}

// Calls from .. count - 1 of a stream as blocking calls, one(k) each -- except call `stands` (-1: none), which an attempt already enqueued
// has settled (state 0).  Every call's state is recorded; a negative state ends the stream, and so does the first non-zero state of a loop
// over one triple (every further call would end alike).  Returns that state, else the first non-zero state (0: none).
template <class One>
static int rest_blocking(const Mats& mt, int from, int count, int stands, One one) {
	int first = 0;
	for (int k = from; k < count; k++) {
		const int st = (k == stands) ? 0 : one(k);
		mt.state(k, st);
		if (st && !first) first = st;
		if (st < 0 || (st && mt.same())) return st;
	}
	return first;
}

// one call of the stream as a plain blocking call with its whole ladder
static int blocking_one(const CallEnv& env, const Mats& mt, int i, const Call& cl) {
	if (!env.dist)
		return tsqr_mi_qr_f32(cl.mode, cl.reorth, mt.q(i), cl.ldq, mt.r(i), cl.ldr, mt.a(i), cl.lda, cl.m, cl.n, cl.wq, cl.wr, nullptr, nullptr, cl.h_wl, cl.stream);
	Ctx cc;
	cc.comm = env.comm;
	return qr_dist_common(cc, cl.mode, cl.reorth, mt.q(i), cl.ldq, mt.r(i), cl.ldr, mt.a(i), cl.lda, cl.m, cl.n, cl.wq, cl.wr, env.nranks, cl.stream);
}

// Call i of a chained stream was rejected by the bf16-split level: its apply pass skipped itself and A(i) is intact.  Everything of call
// i + 1 is enqueued behind it.  Drain the stream; call i gets its whole ladder as a blocking call; call i + 1 STANDS when it was accepted
// (it may have been factored in place -- an accepted call is never redone) and gets its ladder otherwise.  *done = calls dealt with; the
// caller goes on from there.  A loop over one triple would see every further attempt rejected as well: the rest of its count runs as
// blocking calls.  (Row-partitioned: the verdicts come from the all-reduced matrix -- every rank walks through here alike.)
static int rejected_tail(const CallEnv& env, const Mats& mt, int count, const Call& cl, int i, const Completion& comp, int* done) {
	HIPCHK(hipStreamSynchronize(comp.c.st));
	prof_collect();
	const bool next = i + 1 < count, next_rejected = next && comp.rejected(i + 1);     // (read before a blocking call reuses the words)
	if (mt.same()) {
		*done = count;
		return rest_blocking(mt, i, count, -1, [&](int k) { return blocking_one(env, mt, k, cl); });
	}
	int s = blocking_one(env, mt, i, cl);
	if (s < 0) return s;
	mt.state(i, s);
	int first = s;
	*done = i + 1;
	if (next) {
		s = 0;
		if (next_rejected) { s = blocking_one(env, mt, i + 1, cl); if (s < 0) return s; }
		mt.state(i + 1, s);
		if (s && !first) first = s;
		*done = i + 2;
	}
	return first;
}

// ---- what the 64-column chained schedules share (chained64, chained_dist, the fp16 stream) ----
// the streams gram_blk_kernel takes: every A an operand for it (blk_gram_ok), no second sweep, leading dimensions that hold the operands
static bool blk_shape(const Mats& mt, int count, const Call& cl) {
	if (cl.reorth || cl.lda < cl.m || cl.ldq < cl.m || cl.ldr < cl.n) return false;
	for (int i = 0; i < (mt.same() ? 1 : count); i++)
		if (!blk_gram_ok(mt.a(i), cl.lda, cl.m, cl.n)) return false;
	return true;
}
// the Gram pass over `a` into `part`; it carries the pending announcement
static tsqrmi::GramArgs gram_args_64(Ctx& c, const float* a, const Call& cl, int nchunks, const GramPlan& g, double* part) {
	tsqrmi::GramArgs ga{};
	ga.a = a; ga.lda = cl.lda; ga.m = cl.m; ga.n = (int)cl.n; ga.nchunks = nchunks; ga.cpw = g.cpw; ga.nwaves = g.nwaves;
	ga.part = part;
	carry_announcement(c, ga);
	return ga;
}

// The stream for full 64-column matrices of up to 2^20 rows (the shapes gram_blk_kernel takes): the R-factor chain of call i (reduction,
// Cholesky, verdict) runs inside the launch that is the Gram pass of call i + 1 (gram_blk_chain_kernel), so a call costs its two
// streaming passes and nothing else:
//     gram(0) | [chain(0) + gram(1)]  apply(0) | [chain(1) + gram(2)]  apply(1) | ... | reduce, Cholesky (launches of their own)  apply(last)
// Two sets of Gram partials (wr); verdict words alternate between the halves of the pinned words; the completion word of call i is raised
// by the first kernel behind apply(i).  Returns NOT_MINE when the shape / settings / operand order are not the ones this schedule is for
// (nothing enqueued).  A rejected verdict ends the schedule at that call (rejected_tail); *done tells the caller how far the stream got.
static int chained64(const Mats& mt, int count, const Call& cl, int* done) {
	*done = 0;
	const size_t m = cl.m, n = cl.n;
	const int engine = engine_of(cl.mode);
	if (count < 3 || engine < 0 || !blk_shape(mt, count, cl)) return NOT_MINE;
	if (!out_of_order(mt, count, cl) || !chain_fits_cache(mt, cl)) return NOT_MINE;
	Ctx c;
	env_ctx(c, CallEnv{}, cl.wq, cl.wr, m, n, cl.h_wl, cl.stream, /*keep_in_flight=*/false);
	if (!(c.policy == 0 && c.gram_level == 2 && c.hsig.dev && !g_set.debug)) return NOT_MINE;
	c.fold_cor = (engine == 1);
	int rc = blk_kernel_attrs(c.dev);
	if (rc) return rc;
	const GramPlan g = gram_plan(m, n);
	const int nchunks = (int)(m / 128), nparts = std::min(nchunks, g.nblocks), nelem = 10 * 256, nred = nelem / 16;
	double* part[2] = {reinterpret_cast<double*>(c.wr), reinterpret_cast<double*>(c.wr) + (size_t)g.nblocks * nelem};
	unsigned* ticket = c.status_dev(0) + 8;              // (a word of the status area no kernel uses)
	HIPCHK(hipMemsetAsync(ticket, 0, sizeof(unsigned), c.st));
	Completion comp(c);
	// one step = the launches of call i behind its Gram pass: chain(i) (with the Gram pass of call i + 1 when there is one), apply(i)
	auto step = [&](int i) -> int {
		const SweepOpts o{i & 1};                            // (verdict words: half i & 1, no dependency)
		if (i + 1 < count) {
			tsqrmi::ChainArgs ch{};
			ch.chol = chol_args(c, o, mt.r(i), cl.ldr, n, 2);
			ch.part = part[i & 1]; ch.nparts = nparts; ch.ticket = ticket; ch.nred = nred;
			ProfScope ps(KC_GRAM, c.st);
			hipLaunchKernelGGL(tsqrmi::gram_blk_chain_kernel, dim3(nred + nparts), dim3(256), tsqrmi::GB_LDS_BYTES, c.st,
			                   gram_args_64(c, mt.a(i + 1), cl, nchunks, g, part[(i + 1) & 1]), ch);
		} else {
			// the last call: no Gram pass left to hide behind -- the chain as launches of its own (and the completion word of the call
			// before, which no Gram kernel is there to raise)
			raise_announcement(c);
			ProfScope ps(KC_CHOL, c.st);
			launch_reduce1(c.st, c.gsum(), part[i & 1], nparts, nelem, (double)m);
			hipLaunchKernelGGL(tsqrmi::chol16_kernel, dim3(1), dim3(1024), 0, c.st, chol_args(c, o, mt.r(i), cl.ldr, n, 2));
		}
		HIPCHK(hipGetLastError());
		const int rc2 = apply_rinv(c, o, nullptr, engine, mt.q(i), cl.ldq, mt.a(i), cl.lda, mt.r(i), cl.ldr, m, n, /*z_ready=*/true, c.status_dev(i & 1));
		return rc2 ? rc2 : comp.close(i, i + 1 == count);
	};
	{
		ProfScope ps(KC_GRAM, c.st);
		hipLaunchKernelGGL(tsqrmi::gram_blk_kernel<false>, dim3(nparts), dim3(256), tsqrmi::GB_LDS_BYTES, c.st, gram_args_64(c, mt.a(0), cl, nchunks, g, part[0]));
	}
	HIPCHK(hipGetLastError());
	return run_chained(comp, mt, count, 3, step, [&](int i) { return rejected_tail(CallEnv{}, mt, count, cl, i, comp, done); }, done);
}

// The chained schedule for a stream of 128-column calls (one GPU; every 64-row block full: m % 64 == 0, the fast Gram form): the
// two-block factorisation of call i (45 us on one workgroup) rides in the Gram launch of call i + 1 (gram_wide_chain_kernel); the
// reduction of the partials stays a launch of its own in front of it:
//     gram(0) reduce(0) | [chol(0) + gram(1)]  reduce(1)  apply(0) | [chol(1) + gram(2)]  reduce(2)  apply(1) | ... | chol(last)  apply(last)
// Returns NOT_MINE when the stream is not one for it (nothing enqueued); a rejected verdict ends the schedule at that call (rejected_tail:
// its blocking call falls back to 64-column panels and overwrites A, as the blocking call does).
static int chained128(const Mats& mt, int count, const Call& cl, int* done) {
	*done = 0;
	const size_t m = cl.m, n = cl.n, lda = cl.lda, ldq = cl.ldq, ldr = cl.ldr;
	const int engine = engine_of(cl.mode);
	if (count < 3 || engine < 0 || cl.reorth || n != 2 * PW || m < n || m % 64 != 0 || m / 64 < 2 * (size_t)WIDE_MAX_WGS || lda > ((size_t)1 << 23) ||
	    lda < m || ldq < m || ldr < n || lda % 4 != 0 || !a_aligned16(mt, count))
		return NOT_MINE;
	if (!out_of_order(mt, count, cl) || !chain_fits_cache(mt, cl)) return NOT_MINE;
	Ctx c;
	env_ctx(c, CallEnv{}, cl.wq, cl.wr, m, n, cl.h_wl, cl.stream, /*keep_in_flight=*/false);
	if (!(c.wide && c.policy == 0 && c.gram_level == 2 && c.hsig.dev && !g_set.debug)) return NOT_MINE;
	const int rca = wide_kernel_attrs(c.dev);
	if (rca) return rca;
	const int nblk = (int)(m / 64), wgs = WIDE_MAX_WGS;
	Completion comp(c);
	auto gram_args = [&](int i) { return gram_wide_args(c, mt.a(i), lda, m, n, nblk); };
	auto chol_args = [&](int i) { return chol_wide_args(c, SweepOpts{/*slot=*/i & 1}, mt.r(i), ldr, m, n); };
	auto reduce = [&]() {
		ProfScope ps(KC_CHOL, c.st);
		launch_reduce1(c.st, wide_ws(c).gsum, reinterpret_cast<const double*>(c.wr), wgs, 36 * 256, (double)m);
	};
	auto step = [&](int i) -> int {
		if (i + 1 < count) {
			{
				ProfScope ps(KC_GRAM, c.st);
				hipLaunchKernelGGL(tsqrmi::gram_wide_chain_kernel, dim3(1 + wgs), dim3(512), tsqrmi::GWC_LDS_BYTES, c.st, gram_args(i + 1), chol_args(i));
			}
			reduce();
		} else {
			raise_announcement(c);
			ProfScope ps(KC_CHOL, c.st);
			hipLaunchKernelGGL(tsqrmi::chol_wide_kernel, dim3(1), dim3(1024), 0, c.st, chol_args(i));
		}
		HIPCHK(hipGetLastError());
		const int rc = apply_wide(c, SweepOpts{/*slot=*/i & 1}, engine, mt.q(i), ldq, mt.a(i), lda, m, n);
		return rc ? rc : comp.close(i, i + 1 == count);
	};
	{
		ProfScope ps(KC_GRAM, c.st);
		hipLaunchKernelGGL((tsqrmi::gram_wide_kernel<true>), dim3(wgs), dim3(512), tsqrmi::GW_LDS_BYTES, c.st, gram_args(0));
	}
	reduce();
	HIPCHK(hipGetLastError());
	return run_chained(comp, mt, count, 5, step, [&](int i) { return rejected_tail(CallEnv{}, mt, count, cl, i, comp, done); }, done);
}

// The chained schedule of a ROW-PARTITIONED stream (every rank: a full 64-column block of 128 k <= 2^20 rows).  The all-reduce sits inside
// the R-factor chain, so only the factorisation can ride in the next call's Gram launch (gram_blk_chain_kernel, `direct`):
//     gram(0) reduce(0) allreduce(0) | [chol(0) + gram(1)]  reduce(1) allreduce(1)  apply(0) | [chol(1) + gram(2)]  reduce(2) allreduce(2)  apply(1) | ...
//     ... | chol(last) (a launch of its own)  apply(last)
// -- the Cholesky launch (17.5 us + its ramp) leaves the critical path of every call but the last.  The collectives are enqueued in a
// different order than by the plain stream (allreduce(i + 1) before apply(i)), so ALL ranks must take this schedule or none.  The vote costs
// no collective of its own: the first all-reduce of the stream -- the Gram tiles of call 0, the same launch in either schedule -- carries one
// more double, 1.0 from every rank that is eligible (a rank that is not sends zeros instead of a Gram pass: the result is then thrown away);
// a one-thread kernel behind it puts the count into the pinned words and the host decides when it sees it, with Gram pass and all-reduce of
// call 0 already done.  Returns NOT_MINE when any rank is not eligible (the stream is then idle and holds nothing of this call).
// A rejected verdict -- the same on every rank -- ends the schedule at that call (rejected_tail).
static int chained_dist(const CallEnv& env, const Mats& mt, int count, const Call& cl, int* done) {
	*done = 0;
	const size_t m = cl.m, n = cl.n;
	const int engine = engine_of(cl.mode);
	if (engine < 0 || m == 0 || n == 0 || n > PW || env.nranks < 1 || env.nranks > 255) return NOT_MINE;   // (conditions every rank shares; the plain path reports errors)
	Ctx c;
	env_ctx(c, env, cl.wq, cl.wr, m, n, nullptr, cl.stream, /*keep_in_flight=*/false);
	const bool mine = c.hsig.dev && blk_shape(mt, count, cl) && c.policy == 0 && c.gram_level == 2 && !g_set.debug && out_of_order(mt, count, cl);
	c.fold_cor = (engine == 1);
	int rc = blk_kernel_attrs(c.dev);
	if (rc) return rc;
	const GramPlan g = gram_plan(m, PW);
	const int nchunks = (int)(m / 128), nparts = std::min(nchunks, g.nblocks), nelem = 10 * 256;
	double* part = reinterpret_cast<double*>(c.wr);
	Completion comp(c);
	auto chol_of = [&](int i) { return chol_args(c, SweepOpts{/*slot=*/i & 1}, mt.r(i), cl.ldr, n, 2); };   // (rows_dev: the all-reduced row count)
	auto reduce_allreduce = [&](int extra) -> int {      // partials of the Gram pass just enqueued -> summed tiles + row count (+ `extra` doubles), over all ranks
		{
			ProfScope ps(KC_CHOL, c.st);
			launch_reduce1(c.st, c.gsum(), part, nparts, nelem, (double)m);
		}
		HIPCHK(hipGetLastError());
		if (extra) hipLaunchKernelGGL(tsqrmi::set_f64_kernel, dim3(1), dim3(1), 0, c.st, c.gsum() + nelem + 1, 1.0);
		ProfScope ps(KC_MISC, c.st);
		if (c.comm.allreduce_f64(c.gsum(), (size_t)nelem + 1 + extra, c.st)) { t_last_error = "all-reduce of the Gram tiles failed"; return -1; }
		return 0;
	};
	// ---- call 0 up to its all-reduce, with the vote in the payload ----
	if (mine) {
		{
			ProfScope ps(KC_GRAM, c.st);
			hipLaunchKernelGGL(tsqrmi::gram_blk_kernel<false>, dim3(nparts), dim3(256), tsqrmi::GB_LDS_BYTES, c.st, gram_args_64(c, mt.a(0), cl, nchunks, g, part));
		}
		HIPCHK(hipGetLastError());
		rc = reduce_allreduce(1);
	} else {
		HIPCHK(hipMemsetAsync(c.gsum(), 0, sizeof(double) * ((size_t)nelem + 2), c.st));
		if (c.comm.allreduce_f64(c.gsum(), (size_t)nelem + 2, c.st)) { t_last_error = "all-reduce of the schedule flags failed"; rc = -1; }
	}
	if (rc) return rc;
	if (c.hsig.dev) {
		unsigned vs = ++g_seq;
		if ((vs & 0xffffffu) == 0) vs = ++g_seq;
		comp.words[8] = 0;
		hipLaunchKernelGGL(tsqrmi::vote_out_kernel, dim3(1), dim3(1), 0, c.st, c.gsum() + nelem + 1, c.hsig.dev + 8, vs);
		HIPCHK(hipGetLastError());
		unsigned w = 0;                                  // (as wait_word, for a word that holds the count next to the sequence number)
		const int seen = spin_until([&] { w = comp.words[8]; return (w >> 8) == (vs & 0xffffffu); }, c.st);
		if (seen < 0) return seen;
		if (seen == 1) w = comp.words[8];
		if ((int)(w & 0xffu) != env.nranks || (w >> 8) != (vs & 0xffffffu)) { prof_collect(); return NOT_MINE; }
	} else {                                             // (no pinned words on this rank: it voted "no"; it still has to leave with an idle stream)
		HIPCHK(hipStreamSynchronize(c.st));
		return NOT_MINE;
	}
	auto step = [&](int i) -> int {
		if (i + 1 < count) {
			tsqrmi::ChainArgs ch{};
			ch.chol = chol_of(i); ch.direct = 1;
			{
				ProfScope ps(KC_GRAM, c.st);
				hipLaunchKernelGGL(tsqrmi::gram_blk_chain_kernel, dim3(1 + nparts), dim3(256), tsqrmi::GB_LDS_BYTES, c.st,
				                   gram_args_64(c, mt.a(i + 1), cl, nchunks, g, part), ch);
			}
			HIPCHK(hipGetLastError());
			const int rc2 = reduce_allreduce(0);
			if (rc2) return rc2;
		} else {
			raise_announcement(c);
			ProfScope ps(KC_CHOL, c.st);
			hipLaunchKernelGGL(tsqrmi::chol16_kernel, dim3(1), dim3(1024), 0, c.st, chol_of(i));
			HIPCHK(hipGetLastError());
		}
		const int rc2 = apply_rinv(c, SweepOpts{/*slot=*/i & 1}, nullptr, engine, mt.q(i), cl.ldq, mt.a(i), cl.lda, mt.r(i), cl.ldr, m, n, /*z_ready=*/true, c.status_dev(i & 1));
		return rc2 ? rc2 : comp.close(i, i + 1 == count);
	};
	return run_chained(comp, mt, count, 3, step, [&](int i) { return rejected_tail(env, mt, count, cl, i, comp, done); }, done);
}

// Two calls in flight: call i + 1 is submitted before call i is finished; the completion word of call i is raised by the first kernel of
// call i + 1 (stream order: it starts when call i has finished), only the last call carries a completion kernel of its own.  That is the
// blocking order only while calls i and i + 1 do not conflict (stream_order.h): a rejected call i runs its ladder AFTER attempt i + 1.  A
// conflicting pair of a batch is issued in order instead -- call i (with a completion kernel of its own) is finished before call i + 1 is
// submitted.  A loop over one triple keeps two calls in flight: a rejected call leaves A untouched, so attempt i + 1 saw that same matrix
// and was rejected too; but when the triple feeds itself (q == a) the ladder of call i has since written its Q there, so call i + 1 is then
// redone as a blocking call (row-partitioned: always after a ladder -- the ranks' operands may differ, their verdicts do not).
// Row-partitioned calls: every rank takes the same verdicts (they come from the all-reduced Gram matrix), and a batch with a conflicting
// pair on any rank never gets here (stream_of_calls), hence the same path through this loop and the same order of collectives.
static bool attempt_stands(const tsqr_mi_ticket* t) { return t->verdict == 0 && !(t->n <= 16 && t->scond > 32.0f); }   // (as finish_impl)
static int two_in_flight(const CallEnv& env, const Mats& mt, int count, const Call& cl) {
	auto submit = [&](int i, tsqr_mi_ticket* t, tsqr_mi_ticket* announce, bool own_flag) {
		return submit_impl(env, cl.mode, cl.reorth, mt.q(i), cl.ldq, mt.r(i), cl.ldr, mt.a(i), cl.lda, cl.m, cl.n, cl.wq, cl.wr, cl.h_wl, cl.stream, t, announce, own_flag);
	};
	const bool redo_after_ladder = mt.same() && (env.dist || [&] { const tsqr_order::Operands o = ops_of(mt, 0, cl, sizeof(float)); return tsqr_order::feeds(o, o); }());
	tsqr_mi_ticket tk[2];
	int first = 0;
	bool ordered = pair_conflicts(mt, count, 0, cl);     // calls i and i + 1 conflict: call i is finished before call i + 1 is submitted
	int st = submit(0, &tk[0], nullptr, /*own_flag=*/count == 1 || ordered);
	if (st) { for (int k = 0; k < count; k++) mt.state(k, st); return st; }           // (invalid size / mode: the same for every call of the stream)
	for (int i = 0; i < count; i++) {
		tsqr_mi_ticket* cur = &tk[i & 1];
		tsqr_mi_ticket* nxt = (i + 1 < count) ? &tk[(i + 1) & 1] : nullptr;
		const bool ordered_next = nxt && pair_conflicts(mt, count, i + 1, cl);
		if (nxt && !ordered) {
			st = submit(i + 1, nxt, cur, /*own_flag=*/i + 2 == count || ordered_next);
			if (st) { (void)finish_impl(env, cur); return st; }
		}
		const bool had_attempt = cur->pending != 0;
		st = finish_impl(env, cur);
		mt.state(i, st);
		if (st && !first) first = st;
		if (st < 0 || (st && mt.same())) { if (nxt && !ordered) (void)finish_impl(env, nxt); return st; }   // (a loop over one triple stops at its first non-zero state)
		if (nxt && !ordered && redo_after_ladder && had_attempt && !attempt_stands(cur)) {
			// the ladder of call i ran after attempt i + 1 (which the stream has drained): call i + 1 as the blocking call
			nxt->pending = 0;
			st = nxt->state = blocking_one(env, mt, i + 1, cl);
			if (st < 0) return st;
		}
		if (nxt && ordered) {
			st = submit(i + 1, nxt, nullptr, /*own_flag=*/i + 2 == count || ordered_next);
			if (st) return st;
		}
		ordered = ordered_next;
	}
	return first;
}

// Row-partitioned batch: the ranks must take the same schedule, so whether ANY rank has a conflicting pair of calls is agreed on with one
// all-reduce of one flag (blocking: the host needs the answer before it enqueues the next call)
static int conflict_on_any_rank(const CallEnv& env, const Mats& mt, int count, const Call& cl, bool* any) {
	bool mine = false;
	for (int i = 0; i + 1 < count && !mine; i++) mine = pair_conflicts(mt, count, i, cl);
	Ctx c;
	env_ctx(c, env, cl.wq, cl.wr, cl.m, cl.n, nullptr, cl.stream, /*keep_in_flight=*/false);
	hipLaunchKernelGGL(tsqrmi::set_f64_kernel, dim3(1), dim3(1), 0, c.st, c.gsum(), mine ? 1.0 : 0.0);
	HIPCHK(hipGetLastError());
	if (c.comm.allreduce_f64(c.gsum(), 1, c.st)) { t_last_error = "all-reduce of the operand-order flag failed"; return -1; }
	double h = 0.0;
	HIPCHK(hipMemcpyAsync(&h, c.gsum(), sizeof(double), hipMemcpyDeviceToHost, c.st));
	HIPCHK(hipStreamSynchronize(c.st));
	*any = h != 0.0;
	return 0;
}

// `count` calls as a stream.  Depth 3: the chained schedules as far as they go -- a rejected call ends one, the stream goes on behind it
// with a fresh one (after a second rejection: two in flight for the rest, every attempt of a chained schedule would be thrown away).
static int stream_of_calls(const CallEnv& env, const Mats& mt, int count, const Call& cl) {
	const int depth = g_set.loop_depth.load();
	bool in_order = count < 2 || depth < 2;
	if (!in_order && env.dist && !mt.same()) {
		const int rc = conflict_on_any_rank(env, mt, count, cl, &in_order);
		if (rc) return rc;
	}
	if (in_order) return rest_blocking(mt, 0, count, -1, [&](int i) { return blocking_one(env, mt, i, cl); });
	int first = 0, pos = 0, rejections = 0;
	while (depth >= 3 && count - pos >= 3 && rejections < 2) {
		const Mats sub = mt.from(pos);
		int done = 0, st;
		if (env.dist) st = chained_dist(env, sub, count - pos, cl, &done);
		else {
			st = chained64(sub, count - pos, cl, &done);
			if (st == NOT_MINE) st = chained128(sub, count - pos, cl, &done);
		}
		if (st == NOT_MINE) break;
		if (st < 0) return st;
		if (st && !first) first = st;
		if (pos + done < count) rejections++;
		pos += done;
	}
	if (pos < count) {
		const int st = two_in_flight(env, mt.from(pos), count - pos, cl);
		if (st < 0) return st;
		if (st && !first) first = st;
	}
	return first;
}

}  // namespace

extern "C" {

void tsqr_mi_set_loop_depth(int depth) { g_set.loop_depth = depth < 2 ? 1 : (depth == 2 ? 2 : 3); }

// `count` calls with the same arguments: the reference's speed protocol (src/test.cu:299-309 is such a C++ loop around its call).
// Returns the first non-zero state.
int tsqr_mi_qr_f32_loop(int count, int mode, int reorth, float* q, size_t ldq, float* r, size_t ldr, float* a, size_t lda,
                        size_t m, size_t n, void* wq_v, void* wr_v, float* reorth_w, unsigned* d_wl, unsigned* h_wl, void* stream) {
	(void)reorth_w; (void)d_wl;
	return stream_of_calls(CallEnv{}, one_triple(q, r, a), count, Call{mode, reorth, ldq, ldr, lda, m, n, wq_v, wr_v, h_wl, stream});
}

// `count` DIFFERENT matrices of one shape (include/tsqr_mi.h): the caller of mtk::qr::qr with many matrices -- the stream of calls above
// over one (q, r, a) triple per call.
int tsqr_mi_qr_f32_batch(int count, int mode, int reorth, float* const* q, size_t ldq, float* const* r, size_t ldr, float* const* a, size_t lda,
                         size_t m, size_t n, void* wq_v, void* wr_v, float* reorth_w, unsigned* d_wl, unsigned* h_wl, void* stream, int* states) {
	(void)reorth_w; (void)d_wl;
	Mats mt;
	if (const int rc = triple_per_call(mt, count, q, r, a, states)) return rc;
	return stream_of_calls(CallEnv{}, mt, count, Call{mode, reorth, ldq, ldr, lda, m, n, wq_v, wr_v, h_wl, stream});
}

// ---- fp16 I/O modes: reference mtk::qr::qr<fp16_notc | fp16_tc_nocor, Reorthogonalize> (src/blockqr.cu:437-449; io and working
// types half, src/tsqr.hpp:27-39).  The boundary converts, the factorisation is the fp32 pipeline: A is widened into the tail of
// wq (leading dimension = m rounded up to 128: full blocks for the fast kernels), Q and R are formed in fp32 next to it and
// rounded to fp16 on the way out.  fp16_notc runs the error-corrected bf16x3 apply engine (fp32-accurate products: the pipeline of
// fp32_tc_cor), fp16_tc_nocor the single-fp16-product engine (exact for fp16 data in A; inverse(R) rounded to fp16, no correction --
// the mode's meaning in the reference, src/tcqr32x16.cu:617-667).
// A is never modified.  Costs two conversion passes on top of the fp32 call -- unless the native path inside tsqr_mi_qr_f16 takes
// the call (one panel, one sweep, aligned columns, accepted by the bf16-split level's verdict). ----
namespace {
size_t f16_ld(size_t m) { return (m + 127) & ~(size_t)127; }
size_t f16_tail_offset(size_t m, size_t n) { return (tsqr_mi_working_q_size(m, n) + 63) & ~(size_t)63; }
int f16_engine_mode(int mode) {
	if (mode == TSQR_MI_FP16_NOTC) return TSQR_MI_FP32_TC_COR;
	if (mode == TSQR_MI_FP16_TC_NOCOR) return TSQR_MI_FP32_TC_NOCOR;
	return -1;
}
}  // namespace
size_t tsqr_mi_working_q_size_f16(size_t m, size_t n) {
	if (m == 0 || n == 0) return 0;
	return f16_tail_offset(m, n) + 2 * f16_ld(m) * n + ((n * n + 63) & ~(size_t)63);
}
size_t tsqr_mi_working_r_size_f16(size_t m, size_t n) { return tsqr_mi_working_r_size(m, n); }

int tsqr_mi_qr_f16(int mode, int reorth, void* q, size_t ldq, void* r, size_t ldr, const void* a, size_t lda,
                   size_t m, size_t n, void* wq_v, void* wr_v, void* reorth_w, unsigned* d_wl, unsigned* h_wl, void* stream) {
	(void)reorth_w;
	if (n > m || m == 0 || n == 0) return TSQR_MI_ERROR_INVALID_SIZE;
	const int emode = f16_engine_mode(mode);
	if (emode < 0) { t_last_error = "tsqr_mi_qr_f16 takes fp16_notc or fp16_tc_nocor"; return TSQR_MI_ERROR_UNSUPPORTED; }
	if (ldq < m || lda < m || ldr < n) return TSQR_MI_ERROR_INVALID_SIZE;
	hipStream_t st = reinterpret_cast<hipStream_t>(stream);
	const size_t ld32 = f16_ld(m);
	float* a32 = reinterpret_cast<float*>(wq_v) + f16_tail_offset(m, n);
	float* q32 = a32 + ld32 * n;
	float* r32 = q32 + ld32 * n;
	auto aligned16 = [](const void* p, size_t ld) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 8 == 0; };
	const unsigned grid = (unsigned)std::min<size_t>(4096, cdiv(cdiv(m, 8) * n, 256));
	// Native path (one panel, one sweep, auto policy, 16-byte aligned columns): the Gram pass takes the halves of A as MFMA operands
	// (gram_h_kernel: exact products, half the bytes), the apply pass reads halves and writes halves -- no conversion passes.  The
	// verdict is the bf16-split level's; a rejected matrix (A untouched) goes through the conversion path below and its whole ladder.
	if (n <= PW && !reorth && g_set.policy.load() == 0 && g_set.gram_level.load() == 2 && aligned16(a, lda) && aligned16(q, ldq)) {
		Ctx c;
		init_ctx(c, wq_v, wr_v, m, n, stream);
		c.rows_global = (double)m;
		resolve_host_sig(c, h_wl, m);
		const SweepOpts o{};                                 // (slot 0, no dependency)
		int rc = gram_g(c, o, reinterpret_cast<const float*>(a), lda, m, n, /*bf16=*/true, /*io_half=*/true);
		if (!rc) rc = chol_from_g(c, o, r32, n, n, 2);
		// (R to fp16: workgroup 0 of the apply pass does it -- scattered 2-byte stores inside the Cholesky kernel cost that 5 us, a
		// launch of its own 4.8 us)
		if (!rc) rc = apply_rinv(c, o, nullptr, engine_of(f16_engine_mode(mode)), reinterpret_cast<float*>(q), ldq, reinterpret_cast<const float*>(a), lda,
		                         r32, n, m, n, /*z_ready=*/true, c.status_dev(0), /*io_half=*/true, r, ldr);
		if (rc) return rc;
		unsigned status = 1u;
		float scond = 0.0f;
		rc = read_status(c, 0, &status, &scond);
		if (rc) return rc;
		if (status == 0 && !(n <= 16 && scond > 32.0f)) {    // (n <= 16 with S > 32: the fp32 path adds a second sweep, see qr_core)
			t_last_engine = 3;
			return TSQR_MI_SUCCESS;
		}
	}
	hipLaunchKernelGGL(tsqrmi::widen_f16_kernel, dim3(grid), dim3(256), 0, st, a32, ld32, reinterpret_cast<const _Float16*>(a), lda, m, (int)n,
	                   aligned16(a, lda) ? 1 : 0);
	HIPCHK(hipGetLastError());
	const int rc = tsqr_mi_qr_f32(emode, reorth, q32, ld32, r32, n, a32, ld32, m, n, wq_v, wr_v, nullptr, d_wl, h_wl, stream);   // (blocking)
	if (rc) return rc;
	hipLaunchKernelGGL(tsqrmi::narrow_f16_kernel, dim3(grid), dim3(256), 0, st, reinterpret_cast<_Float16*>(q), ldq, q32, ld32, m, (int)n,
	                   aligned16(q, ldq) ? 1 : 0);
	hipLaunchKernelGGL(tsqrmi::narrow_f16_kernel, dim3((unsigned)cdiv(cdiv(n, 8) * n, 256)), dim3(256), 0, st, reinterpret_cast<_Float16*>(r), ldr, r32, n,
	                   n, (int)n, aligned16(r, ldr) ? 1 : 0);
	HIPCHK(hipGetLastError());
	return tsqr_mi_stream_wait(stream);
}

// The fp16 calls as a stream, two in flight (the native path only: one panel, no reorth, aligned halves): Gram pass on the halves, reduction,
// Cholesky + verdict, apply pass (which also rounds R), the completion word of call i raised by the Gram kernel of call i + 1.  The
// verdict words alternate between the two halves of the pinned words.  Returns NOT_MINE when the call is not one for the native path
// (nothing enqueued); a rejected verdict drains the stream and finishes the count with blocking calls (conversion path, whole ladder).
// (mt: the half-typed operands of the calls, carried as float* -- one triple for a loop, one per call for a batch)
static int stream_of_calls_f16(const Mats& mt, int count, int mode, size_t ldq, size_t ldr, size_t lda,
                               size_t m, size_t n, void* wq_v, void* wr_v, unsigned* h_wl, void* stream) {
	auto aligned16 = [](const void* p, size_t ld) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 8 == 0; };
	const int emode = f16_engine_mode(mode);
	if (emode < 0 || n > m || m == 0 || n == 0 || n > PW || n <= 16 || ldq < m || lda < m || ldr < n) return NOT_MINE;
	for (int i = 0; i < (mt.same() ? 1 : count); i++)
		if (!aligned16(mt.a(i), lda) || !aligned16(mt.q(i), ldq)) return NOT_MINE;
	const Call cl{mode, 0, ldq, ldr, lda, m, n, wq_v, wr_v, h_wl, stream};
	for (int i = 0; i + 1 < count; i++)                  // a pair of calls that conflict (stream_order.h): the batch runs as blocking calls
		if (pair_conflicts(mt, count, i, cl, sizeof(_Float16))) return NOT_MINE;
	Ctx c;
	env_ctx(c, CallEnv{}, wq_v, wr_v, m, n, h_wl, stream, /*keep_in_flight=*/false);
	if (!(c.policy == 0 && c.gram_level == 2 && c.hsig.dev && !t_prof.on && !g_set.debug)) return NOT_MINE;
	float* r32 = reinterpret_cast<float*>(wq_v) + f16_tail_offset(m, n) + 2 * f16_ld(m) * n;
	const int engine = engine_of(emode);
	Completion comp(c);
	// behind the R factor of call i, in either schedule: its apply pass (which also rounds R to halves), then its completion word
	auto apply_and_close = [&](int i) -> int {
		const int rc = apply_rinv(c, SweepOpts{/*slot=*/i & 1}, nullptr, engine, mt.q(i), ldq, mt.a(i), lda, r32, n, m, n, /*z_ready=*/true, c.status_dev(i & 1), /*io_half=*/true, mt.r(i), ldr);
		return rc ? rc : comp.close(i, i + 1 == count);
	};
	// rejected (its apply pass skipped itself: A and Q untouched): drain; this call as a blocking call (conversion path, whole
	// ladder); the call behind it, enqueued in full, stands if it was accepted; the rest of the count as blocking calls
	auto tail = [&](int i) -> int {
		HIPCHK(hipStreamSynchronize(c.st));
		const bool next_ok = i + 1 < count && !comp.rejected(i + 1);
		return rest_blocking(mt, i, count, next_ok ? i + 1 : -1, [&](int k) {
			return tsqr_mi_qr_f16(mode, 0, mt.q(k), ldq, mt.r(k), ldr, mt.a(k), lda, m, n, wq_v, wr_v, nullptr, nullptr, h_wl, stream);
		});
	};
	int done = 0;
	// n = 64, three calls or more: the chained schedule (tsqr_mi_qr_f32_loop's, with gram_h_chain_kernel) -- the R-factor chain of call i
	// inside the Gram launch of call i + 1, two sets of partials
	// (the chained launch order needs a loop's Q and R clear of its A, and two different matrices must share the Infinity Cache)
	if (!(n == PW && count >= 3 && g_set.loop_depth.load() >= 3 && out_of_order(mt, count, cl, sizeof(_Float16)) && chain_fits_cache(mt, cl, sizeof(_Float16)))) {
		// two in flight: every launch of call i; call i - 1's completion word rides in its Gram kernel (gram_g)
		auto step = [&](int i) -> int {
			const SweepOpts o{i & 1};
			int rc = gram_g(c, o, mt.a(i), lda, m, n, /*bf16=*/true, /*io_half=*/true);
			if (!rc) rc = chol_from_g(c, o, r32, n, n, 2);
			return rc ? rc : apply_and_close(i);
		};
		return run_chained(comp, mt, count, 3, step, tail, &done);
	}
	const GramPlan g = gram_plan(m, n);
	const int nelem = 10 * 256, nred = nelem / 16;
	double* part[2] = {reinterpret_cast<double*>(c.wr), reinterpret_cast<double*>(c.wr) + (size_t)g.nblocks * nelem};
	unsigned* ticket = c.status_dev(0) + 8;
	HIPCHK(hipMemsetAsync(ticket, 0, sizeof(unsigned), c.st));
	hipLaunchKernelGGL(tsqrmi::gram_h_kernel<4>, dim3(g.nblocks), dim3(256), 0, c.st, gram_args_64(c, mt.a(0), cl, g.nch, g, part[0]));
	HIPCHK(hipGetLastError());
	auto step = [&](int i) -> int {
		const SweepOpts o{i & 1};
		if (i + 1 < count) {
			tsqrmi::ChainArgs ch{};
			ch.chol = chol_args(c, o, r32, n, n, 2);
			ch.part = part[i & 1]; ch.nparts = g.nblocks; ch.ticket = ticket; ch.nred = nred;
			hipLaunchKernelGGL(tsqrmi::gram_h_chain_kernel, dim3(nred + g.nblocks), dim3(256), 0, c.st, gram_args_64(c, mt.a(i + 1), cl, g.nch, g, part[(i + 1) & 1]), ch);
		} else {
			raise_announcement(c);
			launch_reduce1(c.st, c.gsum(), part[i & 1], g.nblocks, nelem, (double)m);
			hipLaunchKernelGGL(tsqrmi::chol16_kernel, dim3(1), dim3(1024), 0, c.st, chol_args(c, o, r32, n, n, 2));
		}
		HIPCHK(hipGetLastError());
		return apply_and_close(i);
	};
	return run_chained(comp, mt, count, 3, step, tail, &done);
}

static int calls_f16(const Mats& mt, int count, int mode, int reorth, size_t ldq, size_t ldr, size_t lda, size_t m, size_t n,
                     void* wq_v, void* wr_v, void* reorth_w, unsigned* d_wl, unsigned* h_wl, void* stream) {
	if (count >= 2 && g_set.loop_depth.load() >= 2 && !reorth) {
		const int st = stream_of_calls_f16(mt, count, mode, ldq, ldr, lda, m, n, wq_v, wr_v, h_wl, stream);
		if (st != NOT_MINE) return st;
	}
	return rest_blocking(mt, 0, count, -1, [&](int i) {
		return tsqr_mi_qr_f16(mode, reorth, mt.q(i), ldq, mt.r(i), ldr, mt.a(i), lda, m, n, wq_v, wr_v, reorth_w, d_wl, h_wl, stream);
	});
}
int tsqr_mi_qr_f16_loop(int count, int mode, int reorth, void* q, size_t ldq, void* r, size_t ldr, const void* a, size_t lda,
                        size_t m, size_t n, void* wq_v, void* wr_v, void* reorth_w, unsigned* d_wl, unsigned* h_wl, void* stream) {
	const Mats mt = one_triple(reinterpret_cast<float*>(q), reinterpret_cast<float*>(r), const_cast<float*>(reinterpret_cast<const float*>(a)));
	return calls_f16(mt, count, mode, reorth, ldq, ldr, lda, m, n, wq_v, wr_v, reorth_w, d_wl, h_wl, stream);
}
// `count` DIFFERENT half-typed matrices of one shape (tsqr_mi_qr_f32_batch's counterpart for the fp16 I/O modes): calls the native path
// takes are issued as a stream, everything else as blocking calls; the same halves either way
int tsqr_mi_qr_f16_batch(int count, int mode, int reorth, void* const* q, size_t ldq, void* const* r, size_t ldr, const void* const* a, size_t lda,
                         size_t m, size_t n, void* wq_v, void* wr_v, void* reorth_w, unsigned* d_wl, unsigned* h_wl, void* stream, int* states) {
	Mats mt;                                             // (pointer arrays of the same layout: void* / float*, const or not)
	if (const int rc = triple_per_call(mt, count, reinterpret_cast<float* const*>(q), reinterpret_cast<float* const*>(r),
	                                   reinterpret_cast<float* const*>(const_cast<void* const*>(a)), states)) return rc;
	return calls_f16(mt, count, mode, reorth, ldq, ldr, lda, m, n, wq_v, wr_v, reorth_w, d_wl, h_wl, stream);
}

// ---- row-partitioned TSQR: one call per rank, the same ladder as tsqr_mi_qr_f32 with the exchange hooks switched on ----
// (CallEnv of a row-partitioned call from the caller's transport: an ncclComm_t with its entry points, or callbacks)
static int env_of_nccl(CallEnv& env, void* nccl_comm, void* nccl_allreduce_fn, void* nccl_allgather_fn, float* gather_buf, int nranks) {
	if (!nccl_comm || !nccl_allreduce_fn || !nccl_allgather_fn) {
		t_last_error = "row-partitioned call needs an ncclComm_t and the ncclAllReduce / ncclAllGather entry points of the library that created it";
		return TSQR_MI_ERROR_UNSUPPORTED;
	}
	env.dist = true; env.nranks = nranks;
	env.comm.nccl = nccl_comm;
	env.comm.nccl_allreduce = reinterpret_cast<nccl_allreduce_t>(nccl_allreduce_fn);
	env.comm.nccl_allgather = reinterpret_cast<nccl_allgather_t>(nccl_allgather_fn);
	env.comm.gather_buf = gather_buf;
	return 0;
}
static int env_of_callbacks(CallEnv& env, tsqr_mi_allreduce_f64_cb allreduce, tsqr_mi_allgather_f32_cb allgather, void* user, float* gather_buf, int nranks) {
	if (!allreduce || !allgather) return TSQR_MI_ERROR_UNSUPPORTED;
	env.dist = true; env.nranks = nranks;
	env.comm.cb_allreduce = allreduce; env.comm.cb_allgather = allgather; env.comm.cb_user = user;
	env.comm.gather_buf = gather_buf;
	return 0;
}
int tsqr_mi_qr_f32_dist_fn(int mode, int reorth, float* q, size_t ldq, float* r, size_t ldr, float* a, size_t lda,
                           size_t m_local, size_t n, void* wq_v, void* wr_v, float* gather_buf,
                           void* nccl_comm, void* nccl_allreduce_fn, void* nccl_allgather_fn, int nranks, void* stream) {
	CallEnv env;
	if (const int rc = env_of_nccl(env, nccl_comm, nccl_allreduce_fn, nccl_allgather_fn, gather_buf, nranks)) return rc;
	return blocking_one(env, one_triple(q, r, a), 0, Call{mode, reorth, ldq, ldr, lda, m_local, n, wq_v, wr_v, nullptr, stream});
}
int tsqr_mi_qr_f32_dist(int mode, int reorth, float* q, size_t ldq, float* r, size_t ldr, float* a, size_t lda,
                        size_t m_local, size_t n, void* wq_v, void* wr_v, float* gather_buf,
                        void* nccl_comm, int nranks, void* stream) {
	void* ar = rccl_symbol("ncclAllReduce");
	void* ag = rccl_symbol("ncclAllGather");
	if (!ar || !ag) {
		t_last_error = "ncclAllReduce / ncclAllGather are not in the global symbol scope (the caller does not link RCCL): "
		               "pass the entry points of the library that created the communicator to tsqr_mi_qr_f32_dist_fn";
		return TSQR_MI_ERROR_UNSUPPORTED;
	}
	return tsqr_mi_qr_f32_dist_fn(mode, reorth, q, ldq, r, ldr, a, lda, m_local, n, wq_v, wr_v, gather_buf, nccl_comm, ar, ag, nranks, stream);
}
int tsqr_mi_qr_f32_dist_cb(int mode, int reorth, float* q, size_t ldq, float* r, size_t ldr, float* a, size_t lda,
                           size_t m_local, size_t n, void* wq_v, void* wr_v, float* gather_buf,
                           tsqr_mi_allreduce_f64_cb allreduce, tsqr_mi_allgather_f32_cb allgather, void* user, int nranks, void* stream) {
	CallEnv env;
	if (const int rc = env_of_callbacks(env, allreduce, allgather, user, gather_buf, nranks)) return rc;
	return blocking_one(env, one_triple(q, r, a), 0, Call{mode, reorth, ldq, ldr, lda, m_local, n, wq_v, wr_v, nullptr, stream});
}
int tsqr_mi_qr_f32_dist_fn_loop(int count, int mode, int reorth, float* q, size_t ldq, float* r, size_t ldr, float* a, size_t lda,
                                size_t m_local, size_t n, void* wq_v, void* wr_v, float* gather_buf,
                                void* nccl_comm, void* nccl_allreduce_fn, void* nccl_allgather_fn, int nranks, void* stream) {
	CallEnv env;
	if (const int rc = env_of_nccl(env, nccl_comm, nccl_allreduce_fn, nccl_allgather_fn, gather_buf, nranks)) return rc;
	return stream_of_calls(env, one_triple(q, r, a), count, Call{mode, reorth, ldq, ldr, lda, m_local, n, wq_v, wr_v, nullptr, stream});
}
int tsqr_mi_qr_f32_dist_cb_loop(int count, int mode, int reorth, float* q, size_t ldq, float* r, size_t ldr, float* a, size_t lda,
                                size_t m_local, size_t n, void* wq_v, void* wr_v, float* gather_buf,
                                tsqr_mi_allreduce_f64_cb allreduce, tsqr_mi_allgather_f32_cb allgather, void* user, int nranks, void* stream) {
	CallEnv env;
	if (const int rc = env_of_callbacks(env, allreduce, allgather, user, gather_buf, nranks)) return rc;
	return stream_of_calls(env, one_triple(q, r, a), count, Call{mode, reorth, ldq, ldr, lda, m_local, n, wq_v, wr_v, nullptr, stream});
}

// `count` DIFFERENT row-partitioned matrices (every rank: its row block of each; one block height for all): the stream of calls of the
// loop entries over one (q, r, a) triple per call.  Every rank passes the same count, the same loop depth and operands of the same
// eligibility (alignment) on the same calls' positions (operand overlap is agreed on by an all-reduce) -- the verdicts, and so the path through the batch, are the same on
// all ranks by construction (they come from the all-reduced matrix).
int tsqr_mi_qr_f32_dist_fn_batch(int count, int mode, int reorth, float* const* q, size_t ldq, float* const* r, size_t ldr, float* const* a, size_t lda,
                                 size_t m_local, size_t n, void* wq_v, void* wr_v, float* gather_buf,
                                 void* nccl_comm, void* nccl_allreduce_fn, void* nccl_allgather_fn, int nranks, void* stream, int* states) {
	CallEnv env;
	if (const int rc = env_of_nccl(env, nccl_comm, nccl_allreduce_fn, nccl_allgather_fn, gather_buf, nranks)) return rc;
	Mats mt;
	if (const int rc = triple_per_call(mt, count, q, r, a, states)) return rc;
	return stream_of_calls(env, mt, count, Call{mode, reorth, ldq, ldr, lda, m_local, n, wq_v, wr_v, nullptr, stream});
}
int tsqr_mi_qr_f32_dist_cb_batch(int count, int mode, int reorth, float* const* q, size_t ldq, float* const* r, size_t ldr, float* const* a, size_t lda,
                                 size_t m_local, size_t n, void* wq_v, void* wr_v, float* gather_buf,
                                 tsqr_mi_allreduce_f64_cb allreduce, tsqr_mi_allgather_f32_cb allgather, void* user, int nranks, void* stream, int* states) {
	CallEnv env;
	if (const int rc = env_of_callbacks(env, allreduce, allgather, user, gather_buf, nranks)) return rc;
	Mats mt;
	if (const int rc = triple_per_call(mt, count, q, r, a, states)) return rc;
	return stream_of_calls(env, mt, count, Call{mode, reorth, ldq, ldr, lda, m_local, n, wq_v, wr_v, nullptr, stream});
}

// ---- staged entry points (building blocks; every call builds its own context) ----
int tsqr_mi_local_r_f32(float* r, size_t ldr, const float* a, size_t lda, size_t m, size_t n,
                        void* wq, void* wr, void* stream) {
	if (m == 0 || n == 0 || n > PW) return TSQR_MI_ERROR_INVALID_SIZE;
	Ctx c;
	init_ctx(c, wq, wr, m, n, stream);
	return fold_r(c, r, ldr, a, lda, m, n, c.wr, c.wq);
}

int tsqr_mi_apply_rinv_f32(int mode, float* q, size_t ldq, const float* a, size_t lda, const float* r, size_t ldr,
                           size_t m, size_t n, void* wq, void* stream) {
	if (m == 0 || n == 0 || n > PW) return TSQR_MI_ERROR_INVALID_SIZE;
	const int engine = engine_of(mode);
	if (engine < 0) return TSQR_MI_ERROR_UNSUPPORTED;
	Ctx c;
	init_ctx(c, wq, nullptr, m, n, stream);
	return apply_rinv(c, SweepOpts{}, nullptr, engine, q, ldq, a, lda, r, ldr, m, n);
}

size_t tsqr_mi_gram_elems(size_t n) { const size_t NT = np_of(n) / 16; return NT * (NT + 1) / 2 * 256; }

int tsqr_mi_gram_f32(int level, double* gsum, const float* a, size_t lda, size_t m, size_t n, void* wq, void* wr, void* stream) {
	if (m == 0 || n == 0 || n > PW || (level != 1 && level != 2)) return TSQR_MI_ERROR_INVALID_SIZE;
	Ctx c;
	init_ctx(c, wq, wr, m, n, stream);
	const int rc = gram_g(c, SweepOpts{}, a, lda, m, n, level == 2);
	if (rc) return rc;
	if (gsum && gsum != c.gsum())
		HIPCHK(hipMemcpyAsync(gsum, c.gsum(), sizeof(double) * tsqr_mi_gram_elems(n), hipMemcpyDeviceToDevice, c.st));
	return 0;
}

int tsqr_mi_chol_f32(int level, float* r, size_t ldr, const double* gsum, size_t m, size_t n, void* wq_v, unsigned* status_out, void* stream) {
	// level 3: shifted Cholesky of an fp64 (level-1) Gram matrix, G + s I with s from the row count m
	if (m == 0 || n == 0 || n > PW || (level != 1 && level != 2 && level != 3)) return TSQR_MI_ERROR_INVALID_SIZE;
	Ctx c;
	init_ctx(c, wq_v, nullptr, m, n, stream);
	c.rows_global = (double)m;
	if (gsum && gsum != c.gsum())
		HIPCHK(hipMemcpyAsync(c.gsum(), gsum, sizeof(double) * tsqr_mi_gram_elems(n), hipMemcpyDeviceToDevice, c.st));
	int rc = chol_from_g(c, SweepOpts{}, r, ldr, n, level);
	if (rc) return rc;
	if (!status_out) return 0;                           // asynchronous: read the verdict later with tsqr_mi_chol_status
	unsigned status = 0;
	rc = read_status(c, 0, &status);                     // (no pinned words in this context: stream sync + copy)
	if (rc) return rc;
	*status_out = status;
	return 0;
}

// Blocks until everything enqueued on `stream` so far has completed: a one-thread kernel raises a word in the thread's pinned
// memory and the host spins on it (hipStreamSynchronize as the fallback).  For staged callers that end with an asynchronous call.
int tsqr_mi_stream_wait(void* stream) {
	Ctx c;
	c.st = reinterpret_cast<hipStream_t>(stream);
	if (t_own.get()) { c.hsig.host = t_own.host; c.hsig.dev = t_own.dev; }
	return wait_done(c);
}

int tsqr_mi_chol_status(const void* wq_v, size_t m, size_t n, unsigned* status_out, void* stream) {
	if (m == 0 || n == 0 || n > PW || !status_out) return TSQR_MI_ERROR_INVALID_SIZE;
	Ctx c;
	init_ctx(c, const_cast<void*>(wq_v), nullptr, m, n, stream);
	return read_status(c, 0, status_out);
}

int tsqr_mi_apply_z_f32(int mode, float* q, size_t ldq, const float* a, size_t lda, size_t m, size_t n, void* wq_v, void* stream) {
	if (m == 0 || n == 0 || n > PW) return TSQR_MI_ERROR_INVALID_SIZE;
	const int engine = engine_of(mode);
	if (engine < 0) return TSQR_MI_ERROR_UNSUPPORTED;
	Ctx c;
	init_ctx(c, wq_v, nullptr, m, n, stream);
	// under the auto policy a rejected Cholesky (status word != 0) turns a speculatively enqueued apply into a no-op
	const unsigned* skip = (c.policy == 0) ? c.status_dev(0) : nullptr;
	return apply_rinv(c, SweepOpts{}, nullptr, engine, q, ldq, a, lda, nullptr, 0, m, n, /*z_ready=*/true, skip);
}

// ---- harness support: the reference's accuracy metrics evaluated on the device in fp64 (src/validation.cu, src/test.cu:147-165) ----
// scratch: (n*n + 8) doubles of device memory; out_host[0..4] = ||Q^T Q - I||_F^2, its diagonal part, its off-diagonal part,
// ||Q R - A||_F^2, ||A||_F^2.  r / a may be null: then only the orthogonality sums are computed.  gram_out_host (n*n doubles) optional.
int tsqr_mi_validate_f32(const float* q, size_t ldq, const float* r, size_t ldr, const float* a, size_t lda,
                         size_t m, size_t n, double* scratch, double* out_host, double* gram_out_host, void* stream) {
	if (m == 0 || n == 0 || n > m) return TSQR_MI_ERROR_INVALID_SIZE;
	hipStream_t st = reinterpret_cast<hipStream_t>(stream);
	double* g = scratch;
	double* sums = scratch + n * n;
	HIPCHK(hipMemsetAsync(scratch, 0, sizeof(double) * (n * n + 8), st));
	const size_t rows_per_block = 32 * std::max<size_t>(1, cdiv(cdiv(m, 32), 2048));
	hipLaunchKernelGGL(tsqrmi::gramd_kernel, dim3((unsigned)cdiv(m, rows_per_block)), dim3(256), 0, st, g, q, ldq, m, (int)n, rows_per_block);
	hipLaunchKernelGGL(tsqrmi::orth_sums_kernel, dim3(1), dim3(256), 0, st, sums, g, (int)n);
	if (r && a) hipLaunchKernelGGL(tsqrmi::resid_kernel, dim3((unsigned)cdiv(m, 256)), dim3(256), 0, st, sums, q, ldq, r, ldr, a, lda, m, (int)n);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(out_host, sums, sizeof(double) * 5, hipMemcpyDeviceToHost, st));
	if (gram_out_host) HIPCHK(hipMemcpyAsync(gram_out_host, g, sizeof(double) * n * n, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	return 0;
}

int tsqr_mi_rmul_f32(float* r, size_t ldr, const float* r2, size_t ldr2, size_t n, void* wq, void* stream) {
	if (n == 0) return TSQR_MI_ERROR_INVALID_SIZE;
	hipStream_t st = reinterpret_cast<hipStream_t>(stream);
	float* r1 = reinterpret_cast<float*>(wq);            // n*n floats at the start of wq
	const unsigned gb = (unsigned)std::min<size_t>(1024, cdiv(n * n, 256));
	hipLaunchKernelGGL(tsqrmi::copy2d_kernel, dim3(gb), dim3(256), 0, st, r1, n, r, ldr, (int)n, (int)n);
	launch_rmul(r, ldr, r2, ldr2, r1, n, n, st);
	HIPCHK(hipGetLastError());
	return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------------
// The fp64 entry (tsqr_mi_qr_f64): CholeskyQR sweeps on fp64 data, n <= 64 (kernels: tsqr_f64.hip).  A sweep is the Gram pass,
// the reduction, the Cholesky step with its verdict and the apply pass; sweep k >= 2 factors the Q of sweep k - 1 in place and
// multiplies R on the left.  The host reads the verdicts when the stream drains -- the blocking call waits there anyway -- and
// enqueues more sweeps when they are needed: one wait for a one-sweep call, and one more each time the ladder has to go on.
// ---------------------------------------------------------------------------------------------------------------------------
namespace {

constexpr int F64_MAX_SWEEPS = 6;
// (F64_GRAM_WAVES, the wq offsets F64_Z .. F64_WQ, F64Plan and f64_plan: f64_plan.h)

thread_local int t_sweeps64 = 0;
thread_local OwnPinned t_own64;                         // the verdict words of the fp64 entry (slot k & 3 for sweep k)

// The exchange of a row-partitioned sweep (comm active; tsqr_mi_qr_f64_dist*): the summed Gram tiles and the local row count behind
// them, nelem + 1 doubles, all-reduced in place on the stream between the reduction and the Cholesky step -- no host wait.  Every rank
// then factors the same bits, and the Cholesky step takes its rule from the summed row count (rows_dev).
int f64_exchange(const Comm* comm, double* gsum, size_t nelem, hipStream_t st) {
	if (!comm || !comm->active()) return 0;
	if (comm->allreduce_f64(gsum, nelem + 1, st)) { t_last_error = "all-reduce of the fp64 Gram tiles failed"; return -1; }
	return 0;
}

// The Cholesky step on the summed tiles in wq[F64_GSUM] with the rule of an m x n sweep: R -> r (ldr), Z -> wq[F64_Z], verdict -> status
// slot `slot`
int f64_chol(hipStream_t st, double* wq, size_t m, size_t n, double* r, size_t ldr, bool first, int slot, const Comm* comm) {
	const int NT = (int)(np_of(n) / 16), nelem = NT * (NT + 1) / 2 * 256;
	tsqrmi::CholArgs64 ca{};
	ca.r = r; ca.ldr = ldr; ca.z = wq + F64_Z;
	ca.status = reinterpret_cast<unsigned*>(wq + F64_STATUS) + 4 * slot;
	ca.host_status = t_own64.dev + 4 * slot;
	ca.gsum = wq + F64_GSUM;
	const F64Rule rule = f64_rule(m, n, first);          // (f64_plan.h; CholArgs64 states the rule and its sources)
	ca.shift_coef = rule.shift_coef; ca.max_scond = rule.max_scond; ca.alone_max = rule.alone_max;
	ca.n = (int)n; ca.NT = NT;
	if (comm && comm->active()) { ca.rows_dev = wq + F64_GSUM + nelem; ca.first = first ? 1 : 0; }   // (the rule of the GLOBAL row count, on the device)
	hipLaunchKernelGGL(tsqrmi::chol_f64_kernel, dim3(1), dim3(1024), 0, st, ca);
	HIPCHK(hipGetLastError());
	return 0;
}

// Gram pass, reduction and Cholesky step of one sweep over src: R -> r (ldr), Z -> wq[F64_Z], verdict -> status slot `slot`
// (layout: TSQR_MI_ROW_MAJOR when src is row-major with row stride ld -- the R-only and least-squares entries)
int f64_factor(hipStream_t st, double* wq, double* wr, const double* src, size_t ld, size_t m, size_t n, double* r, size_t ldr,
               bool first, int slot, const Comm* comm = nullptr, int layout = TSQR_MI_COL_MAJOR) {
	const F64Plan g = f64_plan(m, n);
	if (g.nblocks <= 0) { t_last_error = "fp64 Gram pass without partials"; return TSQR_MI_ERROR_INVALID_SIZE; }
	const tsqrmi::GramArgs64 ga{src, ld, m, (int)n, g.nunits, g.nwaves, wr};
	f64_gram_launch(st, g, ga, layout);
	HIPCHK(hipGetLastError());
	const int nelem = g.ntri * 256;
	launch_reduce1(st, wq + F64_GSUM, wr, g.nblocks, nelem, (double)m);
	HIPCHK(hipGetLastError());
	if (const int rc = f64_exchange(comm, wq + F64_GSUM, (size_t)nelem, st)) return rc;
	return f64_chol(st, wq, m, n, r, ldr, first, slot, comm);
}

// Q = A Z on a persistent grid: as many workgroups as are resident at once, each wave striding over 32-row blocks.  AROW, QROW: a is
// read, q is written row-major (the leading dimension is then the row stride); the resident count is that of the instantiation launched
template <int NT, bool AROW, bool QROW>
int f64_apply(hipStream_t st, int dev, double* q, size_t ldq, const double* a, size_t lda, size_t m, size_t n, const double* z) {
	static DevOnce once;
	static std::atomic<int> resident[MAX_DEV];
	if (once.need(dev)) {
		resident[dev].store(f64_apply_resident<NT, AROW, QROW>(dev));
		once.done(dev);
	}
	const size_t nblocks = cdiv(m, 32);
	const size_t wgs = f64_apply_wgs(nblocks, (size_t)resident[dev].load());
	hipLaunchKernelGGL((tsqrmi::apply_f64_kernel<NT, AROW, QROW>), dim3((unsigned)wgs), dim3(256), 0, st, q, ldq, a, lda, m, (int)n, z, nblocks);
	HIPCHK(hipGetLastError());
	return 0;
}

// One call of the QR entries with Q (qr_f64_core builds it; the sweeps read it).  comm: null but for the row-partitioned entries.
struct F64Call {
	hipStream_t st; int dev;
	double* q; size_t ldq; double* r; size_t ldr; double* a; size_t lda; size_t m, n;
	double *wq, *wr; const Comm* comm; int a_layout, q_layout;
};

// what sweep k (0-based) reads: A in a_layout for sweep 0, the Q of the sweep before in q_layout after that
struct F64Src { const double* p; size_t ld; int layout; };
F64Src f64_src(const F64Call& c, int k) { return k == 0 ? F64Src{c.a, c.lda, c.a_layout} : F64Src{c.q, c.ldq, c.q_layout}; }

// sweep k (0-based): sweep 0 factors A into r and writes Q; sweep k >= 1 factors Q in place, R <- R_k R.  a_layout, q_layout
// (tsqr_mi_qr_f64_lay): sweep 0 reads A in a_layout -- the Gram pass and the apply pass, which writes Q in q_layout; later sweeps read
// and write Q in q_layout.  R and every launch between the two passes do not depend on a layout.
int f64_sweep(const F64Call& c, int k) {
	const bool first = k == 0;
	const F64Src src = f64_src(c, k);
	int rc = f64_factor(c.st, c.wq, c.wr, src.p, src.ld, c.m, c.n, first ? c.r : c.wq + F64_R2, first ? c.ldr : 64, first, k & 3, c.comm, src.layout);
	if (rc) return rc;
	const double* z = c.wq + F64_Z;
	rc = with_apply(c.n, src.layout, c.q_layout, [&](auto nt, auto ar, auto qr) {
		return f64_apply<decltype(nt)::value, decltype(ar)::value, decltype(qr)::value>(c.st, c.dev, c.q, c.ldq, src.p, src.ld, c.m, c.n, z);
	});
	if (rc || first) return rc;
	f64_rmul_launch(c.st, c.r, c.ldr, c.wq + F64_R2, (int)c.n);
	HIPCHK(hipGetLastError());
	return 0;
}

// The ladder (include/tsqr_mi.h): verdict 0 of sweep 0 with "one sweep suffices" ends a reorth = 0 call, any other accepted first
// sweep is followed by one more (CholeskyQR2), a shifted sweep by two more (shifted CholeskyQR3), a rejected one ends the call (state 3).
template <class Sweep>                                   // sweep(k): enqueue sweep k (0-based) on st; non-zero ends the call with that state
int f64_ladder(int reorth, hipStream_t st, Sweep sweep) {
	t_sweeps64 = 0;
	if (!t_own64.get()) { t_last_error = "could not allocate the pinned verdict words"; return -(int)hipErrorOutOfMemory; }
	volatile unsigned* words = t_own64.host;
	for (int i = 0; i < 16; i++) words[i] = 1u;          // (a sweep that never reported reads as rejected)
	int sweeps = 0, need = reorth ? 2 : 1, checked = 0, last_shift = -1;
	bool shifted = false;
	for (;;) {
		while (sweeps < need) {
			const int rc = sweep(sweeps);
			if (rc) return rc;
			sweeps++;
		}
		HIPCHK(hipStreamSynchronize(st));
		for (; checked < sweeps; checked++) {
			const volatile unsigned* w = words + 4 * (checked & 3);
			const unsigned v = w[0];
			if (v == 1u) {
				t_sweeps64 = checked + 1 + (shifted ? 100 : 0);
				t_last_error = "the Cholesky step was rejected even with the shift: Inf or NaN in A, or a column norm outside [2^-511, 2^512)";
				return TSQR_MI_ERROR_NOT_FINITE;
			}
			// Row-partitioned call: each rank reads its OWN pinned words.  The ranks factored the same all-reduced bits with deterministic
			// kernels and a rule taken from the same summed row count, so the words are equal on all ranks and every rank arrives at the
			// same `need` -- the same number of sweeps, hence of all-reduces -- without a vote.
			if (v == 2u) { shifted = true; last_shift = checked; need = std::max(need, checked + 3); }
			else if (checked == 0 && !(reorth == 0 && w[3] == 1u)) need = std::max(need, 2);
		}
		need = std::min(need, F64_MAX_SWEEPS);
		if (sweeps >= need) break;
	}
	t_sweeps64 = sweeps + (shifted ? 100 : 0);
	// A shifted sweep leaves Q orthonormal only to about s / sigma_min^2; the two plain sweeps behind it are what the bands rest on.  When
	// the cap ends the ladder before they ran -- every sweep of a matrix with an exactly zero column is shifted again: the column stays
	// zero -- Q is not inside the bands (measured 1.2e-7 on the OTHER columns of a 4097 x 64 matrix), and the call says so.
	if (shifted && sweeps < last_shift + 3) {
		t_last_error = "rank-deficient input: the ladder ended before two plain sweeps had followed the last shifted one";
		return TSQR_MI_ERROR_NOT_FINITE;
	}
	return TSQR_MI_SUCCESS;
}

// (F64W_MAX_N, F64W_WR_CAP, F64W_TARGET_WGS, F64WPlan, f64w_plan and the blocked Cholesky step f64w_chain: f64_plan.h)

// sweep k (0-based) of the wide entry: sweep 0 factors A into r and writes Q; sweep k >= 1 factors Q in place, R <- R_k R.  a_layout,
// q_layout (tsqr_mi_qr_f64_wide_lay) as in f64_sweep: sweep 0 reads A in a_layout -- the Gram pass and the apply pass, which writes Q in
// q_layout; later sweeps read and write Q in q_layout.  Everything between the two passes works on the block store and knows no layout.
// A sweep: the Gram pass and its reduction; the blocked Cholesky step -- plain, then the shifted chain enqueued behind it, each of its
// launches skipping itself when the plain verdict was 0 -- so that a one-sweep call still waits on the stream once; the apply pass; R out
// or R <- R_k R.
int f64w_sweep(const F64Call& c, int k) {
	const bool first = k == 0;
	const F64Src src = f64_src(c, k);
	const hipStream_t st = c.st;
	const size_t m = c.m, n = c.n, ldr = c.ldr;
	double *const r = c.r, *const wq = c.wq, *const wr = c.wr;
	const F64WPlan g = f64w_plan(m, n);
	if (g.nslices <= 0 || g.npairs <= 0) { t_last_error = "fp64 wide Gram pass without partials"; return TSQR_MI_ERROR_INVALID_SIZE; }
	const tsqrmi::GramWideF64Args ga{src.p, src.ld, m, (int)n, g.npairs, g.ngroups, g.cps, g.nch, wr};
	f64w_gram_launch(st, g, ga, src.layout);
	HIPCHK(hipGetLastError());
	const int nelem = (int)g.bs;
	launch_reduce1(st, wq + g.o_gs, wr, g.nslices, nelem, (double)m);
	HIPCHK(hipGetLastError());
	if (const int rc = f64_exchange(c.comm, wq + g.o_gs, g.bs, st)) return rc;
	tsqrmi::WideF64 wa{};
	wa.gs = wq + g.o_gs; wa.w = wq + g.o_w; wa.rw = wq + g.o_rw; wa.zw = wq + g.o_zw; wa.ta = wq + g.o_ta; wa.zd = wq + g.o_zd;
	wa.sb = wq + g.o_sb;
	wa.bst = reinterpret_cast<unsigned*>(wq + g.o_bst);
	const int slot = k & 3;
	wa.status = reinterpret_cast<unsigned*>(wq + g.o_status) + 4 * slot;
	wa.host_status = t_own64.dev + 4 * slot;
	const F64Rule rule = f64_rule(m, n, first);          // (f64_plan.h; CholArgs64, tsqr_f64.hip, states the rule)
	wa.max_scond = rule.max_scond; wa.alone_max = rule.alone_max;
	wa.n = (int)n; wa.nb = g.nb;
	if (c.comm && c.comm->active()) { wa.rows_dev = wq + g.o_gs + g.bs; wa.first = first ? 1 : 0; }   // (the rule of the GLOBAL row count, on the device)
	wa.run_if = nullptr; wa.shift_coef = 0.0;
	int rc = f64w_chain(st, wa);
	if (rc) return rc;
	wa.run_if = wa.status; wa.shift_coef = rule.shift_coef;
	rc = f64w_chain(st, wa);
	if (rc) return rc;
	f64w_apply_launch(st, c.q, c.ldq, src.p, src.ld, m, (int)n, g.nb, (const double*)(wq + g.o_zw), src.layout, c.q_layout);
	HIPCHK(hipGetLastError());
	if (first) {
		hipLaunchKernelGGL(tsqrmi::rcopy_wide_f64_kernel, dim3((unsigned)cdiv(n * n, 256)), dim3(256), 0, st, r, ldr, (const double*)(wq + g.o_rw), (int)n);
		HIPCHK(hipGetLastError());
		return 0;
	}
	hipLaunchKernelGGL(tsqrmi::rsave_wide_f64_kernel, dim3((unsigned)cdiv(g.bs, 256)), dim3(256), 0, st, wq + g.o_rc, (const double*)r, ldr, (int)n, g.npairs);
	HIPCHK(hipGetLastError());
	hipLaunchKernelGGL(tsqrmi::rmul_wide_f64_kernel, dim3((unsigned)g.npairs), dim3(1024), 0, st, r, ldr, (const double*)(wq + g.o_rw),
	                   (const double*)(wq + g.o_rc), (int)n);
	HIPCHK(hipGetLastError());
	return 0;
}

// The ladder on the sweeps of one call: f64_sweep for n <= 64, the whole-matrix sweeps of tsqr_mi_qr_f64_wide (f64w_sweep) beyond; the
// verdict words and their meaning are the same.  a_layout, q_layout: the layouts of A and Q (tsqr_mi_qr_f64_lay, tsqr_mi_qr_f64_wide_lay).
int qr_f64_core(int reorth, double* q, size_t ldq, double* r, size_t ldr, double* a, size_t lda, size_t m, size_t n, void* wq, void* wr,
                void* stream, const Comm* comm, int a_layout, int q_layout) {
	const F64Call c{reinterpret_cast<hipStream_t>(stream), cur_device(), q, ldq, r, ldr, a, lda, m, n,
	                reinterpret_cast<double*>(wq), reinterpret_cast<double*>(wr), comm, a_layout, q_layout};
	return f64_ladder(reorth, c.st, [&](int k) { return n > PW ? f64w_sweep(c, k) : f64_sweep(c, k); });
}

// Z_acc = Z_1 ... Z_k, the inverse of R after k sweeps, from Z_k in wq[F64_Z]: a copy for k = 1, else Z_acc <- Z_acc Z_k (trimul_f64_kernel)
int f64r_zacc(hipStream_t st, int k, double* wq, size_t n) {
	const size_t NP = np_of(n);
	if (k == 1) HIPCHK(hipMemcpyAsync(wq + F64R_ZACC, wq + F64_Z, NP * NP * sizeof(double), hipMemcpyDeviceToDevice, st));
	else f64r_zmul_launch(st, wq + F64R_ZACC, wq + F64_Z, (int)n);
	HIPCHK(hipGetLastError());
	return 0;
}

// Sweep k (0-based) of the R-only entry.  Sweep 0 is f64_factor on A: R_1 -> r, Z_1 -> wq[F64_Z].  Sweep k >= 1 never forms Q: first
// Z_acc = Z_1 ... Z_k (sweep 1: a copy of Z_1; later: Z_acc <- Z_acc Z_k, with the Z_k that sweep k - 1 left in wq[F64_Z]), then the Gram
// matrix of A Z_acc straight from A (gramq_f64_kernel), the reduction, the Cholesky step of a later sweep (R_(k+1) -> wq[F64_R2],
// Z_(k+1) -> wq[F64_Z]) and r <- R_(k+1) r.  a_layout: TSQR_MI_ROW_MAJOR picks the row-major form of the two kernels that read A; every
// other launch is the same.
int f64r_sweep(hipStream_t st, int k, double* r, size_t ldr, int a_layout, const double* a, size_t lda, size_t m, size_t n, double* wq, double* wr) {
	if (k == 0) return f64_factor(st, wq, wr, a, lda, m, n, r, ldr, true, 0, nullptr, a_layout);
	double* zacc = wq + F64R_ZACC;
	if (const int rc = f64r_zacc(st, k, wq, n)) return rc;
	const F64Plan g = f64r_plan(m, n);
	if (g.nblocks <= 0) { t_last_error = "fp64 Gram pass without partials"; return TSQR_MI_ERROR_INVALID_SIZE; }
	const tsqrmi::GramQArgs64 ga{a, lda, m, (int)n, g.nunits, g.nwaves, zacc, wr};
	f64r_gramq_launch(st, g, ga, a_layout);
	HIPCHK(hipGetLastError());
	launch_reduce1(st, wq + F64_GSUM, wr, g.nblocks, g.ntri * 256, (double)m);
	HIPCHK(hipGetLastError());
	if (const int rc = f64_chol(st, wq, m, n, wq + F64_R2, 64, false, k & 3, nullptr)) return rc;
	f64_rmul_launch(st, r, ldr, wq + F64_R2, (int)n);
	HIPCHK(hipGetLastError());
	return 0;
}

// the ladder of qr_f64_core (f64_ladder) on the sweeps of f64r_sweep
int r_f64_core(int a_layout, int reorth, double* r, size_t ldr, const double* a, size_t lda, size_t m, size_t n, double* wq, double* wr, hipStream_t st) {
	return f64_ladder(reorth, st, [&](int k) { return f64r_sweep(st, k, r, ldr, a_layout, a, lda, m, n, wq, wr); });
}

// The least-squares entry behind the R-only ladder (corrected semi-normal equations carried out in Q-space; include/tsqr_mi.h).  The
// ladder's last sweep s left Z_1 ... Z_(s-1) in wq[F64R_ZACC] (nothing for s = 1) and Z_s in wq[F64_Z]: one copy or one product
// (f64r_zacc) completes Z = inverse(R).  Then refine + 1 passes, each lsq_f64_kernel (D = (A Z)^T (B - A X), X null the first time), the reduction
// and X <- X + Z D, enqueued back to back; one wait at the end.  From the second correction on a right-hand side whose D did not halve is
// left as it is and stops (lsq_update_f64_kernel's stagnation rule; its state lies in wq[F64L_DPREV]): refine <= 1 is untouched by it.
int lstsq_f64_core(int a_layout, int b_layout, int reorth, int refine, double* x, size_t ldx, double* r, size_t ldr, const double* a, size_t lda,
                   const double* b, size_t ldb, size_t m, size_t n, size_t nrhs, double* wq, double* wr, hipStream_t st) {
	if (const int rc = r_f64_core(a_layout, reorth, r, ldr, a, lda, m, n, wq, wr, st)) return rc;
	double *zacc = wq + F64R_ZACC, *xw = wq + F64L_X, *dsum = wq + F64L_D;
	if (const int rc = f64r_zacc(st, t_sweeps64 % 100, wq, n)) return rc;
	const F64Plan g = f64r_plan(m, n);
	if (g.nblocks <= 0) { t_last_error = "fp64 least-squares pass without partials"; return TSQR_MI_ERROR_INVALID_SIZE; }
	for (int p = 0; p <= refine; p++) {
		const tsqrmi::LsqArgs64 la{a, lda, b, ldb, m, (int)n, (int)nrhs, g.nunits, g.nwaves, zacc, p == 0 ? nullptr : xw, wr};
		f64r_lsq_launch(st, g, la, a_layout, b_layout);
		HIPCHK(hipGetLastError());
		launch_reduce1(st, dsum, wr, g.nblocks, g.NT * 256, (double)m);
		HIPCHK(hipGetLastError());
		f64_lsq_update_launch(st, xw, x, ldx, zacc, dsum, (int)n, (int)nrhs, p == 0 ? 1 : 0, p == refine ? 1 : 0, wq + F64L_DPREV,
		                      p >= 2 ? 1 : 0);
		HIPCHK(hipGetLastError());
	}
	HIPCHK(hipStreamSynchronize(st));
	return TSQR_MI_SUCCESS;
}

}  // namespace

extern "C" {

size_t tsqr_mi_working_q_size_f64_lstsq(size_t m, size_t n, size_t nrhs) { return (m == 0 || n == 0 || nrhs == 0) ? 0 : F64L_WQ; }
size_t tsqr_mi_working_r_size_f64_lstsq(size_t m, size_t n, size_t nrhs) {
	return (m == 0 || n == 0 || nrhs == 0) ? 0 : f64r_wr_doubles(m, std::min(n, PW));
}

// One operand of a single-GPU fp64 entry, as the entry's prologue checks it.  Results (r, x) are column-major.
struct F64Operand { int layout; size_t rows, cols, ld; };

// What every single-GPU _lay entry decides first, in the order that is its contract: the sweep count cleared; a layout other than the two
// (state 1); an empty operand, n > m or a leading dimension below the operand's extent along it -- the rows column-major, the columns
// row-major (state 1; neither sets a text); n above the entry's cap (state 2 with cap_text).  0: go on.  No HIP call.
static int f64_prologue(std::initializer_list<F64Operand> ops, size_t m, size_t n, size_t cap, const char* cap_text) {
	t_sweeps64 = 0;
	for (const F64Operand& o : ops)
		if (o.layout != TSQR_MI_COL_MAJOR && o.layout != TSQR_MI_ROW_MAJOR) return TSQR_MI_ERROR_INVALID_SIZE;
	if (n > m) return TSQR_MI_ERROR_INVALID_SIZE;
	for (const F64Operand& o : ops)
		if (o.rows == 0 || o.cols == 0 || o.ld < (o.layout == TSQR_MI_ROW_MAJOR ? o.cols : o.rows)) return TSQR_MI_ERROR_INVALID_SIZE;
	if (n > cap) { t_last_error = cap_text; return TSQR_MI_ERROR_UNSUPPORTED; }
	return 0;
}

// The in-place rule of the entries that write a Q (state 1, behind f64_prologue): q that is a itself is one operand, so it has one
// layout and one stride.
static bool f64_in_place_broken(const void* q, int q_layout, size_t ldq, const void* a, int a_layout, size_t lda) {
	return q == a && (a_layout != q_layout || ldq != lda);
}

int tsqr_mi_lstsq_f64_lay(int a_layout, int b_layout, int reorth, int refine, double* x, size_t ldx, double* r, size_t ldr,
                          const double* a, size_t lda, const double* b, size_t ldb, size_t m, size_t n, size_t nrhs,
                          void* wq, void* wr, void* stream) {
	const F64Operand A{a_layout, m, n, lda}, B{b_layout, m, nrhs, ldb}, R{TSQR_MI_COL_MAJOR, n, n, ldr}, X{TSQR_MI_COL_MAJOR, n, nrhs, ldx};
	if (const int rc = f64_prologue({A, B, R, X}, m, n, PW, "tsqr_mi_lstsq_f64 supports n <= 64")) return rc;
	if (nrhs > F64L_MAX_NRHS) { t_last_error = "tsqr_mi_lstsq_f64 supports nrhs <= 16"; return TSQR_MI_ERROR_UNSUPPORTED; }
	if (refine < 0 || refine > F64L_MAX_REFINE) { t_last_error = "tsqr_mi_lstsq_f64 supports 0 <= refine <= 4"; return TSQR_MI_ERROR_UNSUPPORTED; }
	if (const int rc = latch_all()) return rc;           // (tickets of tsqr_mi_qr_f32_submit in flight: their verdicts first)
	return lstsq_f64_core(a_layout, b_layout, reorth, refine, x, ldx, r, ldr, a, lda, b, ldb, m, n, nrhs, reinterpret_cast<double*>(wq),
	                      reinterpret_cast<double*>(wr), reinterpret_cast<hipStream_t>(stream));
}

int tsqr_mi_lstsq_f64(int reorth, int refine, double* x, size_t ldx, double* r, size_t ldr, const double* a, size_t lda,
                      const double* b, size_t ldb, size_t m, size_t n, size_t nrhs, void* wq, void* wr, void* stream) {
	return tsqr_mi_lstsq_f64_lay(TSQR_MI_COL_MAJOR, TSQR_MI_COL_MAJOR, reorth, refine, x, ldx, r, ldr, a, lda, b, ldb, m, n, nrhs, wq, wr, stream);
}

size_t tsqr_mi_working_q_size_f64_r(size_t m, size_t n) { return (m == 0 || n == 0) ? 0 : F64R_WQ; }
size_t tsqr_mi_working_r_size_f64_r(size_t m, size_t n) { return (m == 0 || n == 0) ? 0 : f64r_wr_doubles(m, std::min(n, PW)); }

int tsqr_mi_r_f64_lay(int a_layout, int reorth, double* r, size_t ldr, const double* a, size_t lda, size_t m, size_t n,
                      void* wq, void* wr, void* stream) {
	const F64Operand A{a_layout, m, n, lda}, R{TSQR_MI_COL_MAJOR, n, n, ldr};
	if (const int rc = f64_prologue({A, R}, m, n, PW, "tsqr_mi_r_f64 supports n <= 64")) return rc;
	if (const int rc = latch_all()) return rc;           // (tickets of tsqr_mi_qr_f32_submit in flight: their verdicts first)
	return r_f64_core(a_layout, reorth, r, ldr, a, lda, m, n, reinterpret_cast<double*>(wq), reinterpret_cast<double*>(wr),
	                  reinterpret_cast<hipStream_t>(stream));
}

int tsqr_mi_r_f64(int reorth, double* r, size_t ldr, const double* a, size_t lda, size_t m, size_t n, void* wq, void* wr, void* stream) {
	return tsqr_mi_r_f64_lay(TSQR_MI_COL_MAJOR, reorth, r, ldr, a, lda, m, n, wq, wr, stream);
}

size_t tsqr_mi_working_q_size_f64(size_t m, size_t n) { return (m == 0 || n == 0) ? 0 : F64_WQ; }
size_t tsqr_mi_working_r_size_f64(size_t m, size_t n) {
	if (m == 0 || n == 0) return 0;
	const F64Plan g = f64_plan(m, std::min(n, PW));
	return (size_t)g.nblocks * g.ntri * 256;
}
int tsqr_mi_last_sweeps_f64(void) { return t_sweeps64; }

int tsqr_mi_qr_f64_lay(int a_layout, int q_layout, int reorth, double* q, size_t ldq, double* r, size_t ldr, double* a, size_t lda,
                       size_t m, size_t n, void* wq, void* wr, void* stream) {
	const F64Operand A{a_layout, m, n, lda}, Q{q_layout, m, n, ldq}, R{TSQR_MI_COL_MAJOR, n, n, ldr};
	if (const int rc = f64_prologue({A, Q, R}, m, n, PW, "tsqr_mi_qr_f64 supports n <= 64 (tsqr_mi_qr_f64_wide: n <= 1024)")) return rc;
	if (f64_in_place_broken(q, q_layout, ldq, a, a_layout, lda)) return TSQR_MI_ERROR_INVALID_SIZE;
	if (const int rc = latch_all()) return rc;           // (tickets of tsqr_mi_qr_f32_submit in flight: their verdicts first)
	return qr_f64_core(reorth, q, ldq, r, ldr, a, lda, m, n, wq, wr, stream, nullptr, a_layout, q_layout);
}

int tsqr_mi_qr_f64(int reorth, double* q, size_t ldq, double* r, size_t ldr, double* a, size_t lda, size_t m, size_t n,
                   void* wq, void* wr, void* stream) {
	return tsqr_mi_qr_f64_lay(TSQR_MI_COL_MAJOR, TSQR_MI_COL_MAJOR, reorth, q, ldq, r, ldr, a, lda, m, n, wq, wr, stream);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------------
// The entries with a job flag (tsqr_mi_svd_f64, tsqr_mi_qrcp_f64; n <= 64): the ladder, then one single-workgroup kernel on R, then --
// job = 1 -- Q times the n x n matrix that kernel left in the work space, in place.  The sizes, the prologue and the path from the
// ladder to the last wait (f64_job_core) stand here once; an entry adds its kernel launch, as a callable, and what that kernel reports.
// ---------------------------------------------------------------------------------------------------------------------------
namespace {

// job = 1: the QR entry's space with `block` doubles of wq (the entry's n x n matrices behind F64_WQ); job = 0: the R-only entry's
size_t f64_job_wq(size_t m, size_t n, int job, size_t block) { return !job ? tsqr_mi_working_q_size_f64_r(m, n) : (m == 0 || n == 0) ? 0 : block; }
size_t f64_job_wr(size_t m, size_t n, int job) { return job ? tsqr_mi_working_r_size_f64(m, n) : tsqr_mi_working_r_size_f64_r(m, n); }

// What a job entry decides first: the sweep count cleared; a flag other than 0 or 1 (state 1, before everything else); f64_prologue
// on a, on q -- job = 0: not used, it stands in the checks column-major with ld = m -- and on the entry's n x n result; for job = 1
// the in-place rule.  0: go on.  No HIP call.
int f64_job_prologue(int job, int a_layout, int q_layout, const void* q, size_t ldq, const void* a, size_t lda, size_t ld_small,
                     size_t m, size_t n, const char* cap_text) {
	t_sweeps64 = 0;
	if (job != 0 && job != 1) return TSQR_MI_ERROR_INVALID_SIZE;
	const F64Operand A{a_layout, m, n, lda}, Q{job ? q_layout : TSQR_MI_COL_MAJOR, m, n, job ? ldq : m}, S{TSQR_MI_COL_MAJOR, n, n, ld_small};
	if (const int rc = f64_prologue({A, Q, S}, m, n, PW, cap_text)) return rc;
	if (job && f64_in_place_broken(q, q_layout, ldq, a, a_layout, lda)) return TSQR_MI_ERROR_INVALID_SIZE;
	return 0;
}

// U = Q W in place on a persistent grid, as f64_apply launches Q = A Z: the resident count is that of the instantiation launched
template <int NT, bool AROW, bool QROW>
int f64_applyd(hipStream_t st, int dev, double* u, size_t ldu, const double* q, size_t ldq, size_t m, size_t n, const double* w) {
	static DevOnce once;
	static std::atomic<int> resident[MAX_DEV];
	if (once.need(dev)) {
		resident[dev].store(f64_applyd_resident<NT, AROW, QROW>(dev));
		once.done(dev);
	}
	f64_applyd_launch<NT, AROW, QROW>(st, f64_apply_wgs(cdiv(m, 32), (size_t)resident[dev].load()), u, ldu, q, ldq, m, (int)n, w);
	HIPCHK(hipGetLastError());
	return 0;
}

// The common path: the ladder of tsqr_mi_qr_f64_lay (job = 1: Q into q) or of tsqr_mi_r_f64_lay (job = 0), called as they stand with R
// into r; a state other than 0 (3 included) ends the call there.  The ladder call blocks -- it reads its verdict words -- so the stream is
// idle when launch_r(st), the entry's kernel on R, and for job = 1 q = q w in place (w: n x n, from that kernel) are enqueued back to
// back, with one more wait behind them: two waits per call at least.
template <class LaunchR>
int f64_job_core(int a_layout, int q_layout, int job, int reorth, double* q, size_t ldq, double* r, size_t ldr, double* a, size_t lda,
                 size_t m, size_t n, double* wq, double* wr, void* stream, const double* w, LaunchR launch_r) {
	const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
	const int rc = job ? tsqr_mi_qr_f64_lay(a_layout, q_layout, reorth, q, ldq, r, ldr, a, lda, m, n, wq, wr, stream)
	                   : tsqr_mi_r_f64_lay(a_layout, reorth, r, ldr, a, lda, m, n, wq, wr, stream);
	if (rc) return rc;
	launch_r(st);
	HIPCHK(hipGetLastError());
	if (job) {
		const int dev = cur_device();
		const int ra = with_apply(n, q_layout, q_layout, [&](auto nt, auto ar, auto qr) {
			return f64_applyd<decltype(nt)::value, decltype(ar)::value, decltype(qr)::value>(st, dev, q, ldq, q, ldq, m, n, w);
		});
		if (ra) return ra;
	}
	HIPCHK(hipStreamSynchronize(st));
	return TSQR_MI_SUCCESS;
}

// ---- tsqr_mi_svd_f64: R into wq[F64S_R]; svd_r_f64_kernel on R writes s, V, and W into wq[F64S_W]; U = Q W.  The sweep count and the
// convergence word of the Jacobi kernel arrive in the thread's pinned verdict words, which the ladder has finished with when it returns. ----
thread_local int t_jacobi64 = 0;
// The columns of R^T rotate (svd_r_f64_kernel's transpose = 1): W is the product of the rotations and V the normalised columns.  Drmac's
// observation: the lower triangle converges in far fewer sweeps (measured, n = 64: cond 1e6 9 sweeps against 18, cond 1e12 9 against 25:
// profiles/fp64_svd_accuracy.md).
constexpr int F64S_TRANSPOSE = 1;

// R of a jobu = 0 call.  The work space of the R-only entry, whose sizes that call keeps, has no block that outlives a sweep of its
// ladder, so R lives in 32 KiB of device memory the library owns per host thread and device, allocated at the first such call.
struct OwnSvdR {
	double* p[MAX_DEV] = {};
	~OwnSvdR() { for (double* d : p) if (d) (void)hipFree(d); }
	double* get(int dev) {
		if (!p[dev] && hipMalloc(reinterpret_cast<void**>(&p[dev]), 4096 * sizeof(double)) != hipSuccess) { p[dev] = nullptr; (void)hipGetLastError(); }
		return p[dev];
	}
};
thread_local OwnSvdR t_svd_r;

int svd_f64_core(int a_layout, int u_layout, int jobu, int reorth, double* u, size_t ldu, double* s, double* v, size_t ldv,
                 double* a, size_t lda, size_t m, size_t n, double* wq, double* wr, void* stream) {
	double* r = jobu ? wq + F64S_R : t_svd_r.get(cur_device());
	if (!r) { t_last_error = "tsqr_mi_svd_f64: could not allocate the device block that holds R"; return -(int)hipErrorOutOfMemory; }
	double* w = jobu ? wq + F64S_W : nullptr;
	const int rc = f64_job_core(a_layout, u_layout, jobu, reorth, u, ldu, r, 64, a, lda, m, n, wq, wr, stream, w, [&](hipStream_t st) {
		volatile unsigned* words = t_own64.host;         // (the ladder allocated them and has read its verdicts: the stream is idle)
		words[0] = 0u; words[1] = 1u;                    // (a kernel that never reported reads as not converged)
		tsqrmi::SvdArgs64 sa{};
		sa.r = r; sa.ldr = 64; sa.s = s; sa.v = v; sa.ldv = ldv; sa.n = (int)n; sa.transpose = F64S_TRANSPOSE; sa.w = w;
		sa.status = jobu ? reinterpret_cast<unsigned*>(wq + F64S_STATUS) : nullptr;
		sa.host_status = t_own64.dev;
		f64_svd_r_launch(st, sa);
	});
	if (rc) return rc;                                   // (state 3 included: the SVD kernel did not run)
	volatile unsigned* words = t_own64.host;
	t_jacobi64 = (int)words[0];
	if (words[1] != 0u) {
		t_last_error = "tsqr_mi_svd_f64: the Jacobi iteration reached its cap of 30 sweeps";
		return TSQR_MI_ERROR_NO_CONVERGENCE;
	}
	return TSQR_MI_SUCCESS;
}

// ---- tsqr_mi_qrcp_f64: R0 into the caller's r; qrcp_r_f64_kernel factors R0 P = H R in place on r (jpvt; H into wq[F64P_H] for
// jobq = 1, not formed otherwise); Q = Q0 H.  Nothing is allocated; the kernel has no verdict of its own. ----
int qrcp_f64_core(int a_layout, int q_layout, int jobq, int reorth, double* q, size_t ldq, double* r, size_t ldr, int* jpvt,
                  double* a, size_t lda, size_t m, size_t n, double* wq, double* wr, void* stream) {
	double* h = jobq ? wq + F64P_H : nullptr;
	return f64_job_core(a_layout, q_layout, jobq, reorth, q, ldq, r, ldr, a, lda, m, n, wq, wr, stream, h, [&](hipStream_t st) {
		tsqrmi::QrcpArgs64 pa{};
		pa.r0 = r; pa.ldr0 = ldr; pa.r = r; pa.ldr = ldr; pa.jpvt = jpvt; pa.n = (int)n; pa.h = h;
		pa.status = jobq ? reinterpret_cast<unsigned*>(wq + F64P_STATUS) : nullptr;
		f64_qrcp_r_launch(st, pa);
	});
}

}  // namespace

extern "C" {

size_t tsqr_mi_working_q_size_f64_svd(size_t m, size_t n, int jobu) { return f64_job_wq(m, n, jobu, F64S_WQ); }
size_t tsqr_mi_working_r_size_f64_svd(size_t m, size_t n, int jobu) { return f64_job_wr(m, n, jobu); }
int tsqr_mi_last_jacobi_sweeps_f64(void) { return t_jacobi64; }

int tsqr_mi_svd_f64(int a_layout, int u_layout, int jobu, int reorth, double* u, size_t ldu, double* s, double* v, size_t ldv,
                    double* a, size_t lda, size_t m, size_t n, void* wq, void* wr, void* stream) {
	t_jacobi64 = 0;
	if (const int rc = f64_job_prologue(jobu, a_layout, u_layout, u, ldu, a, lda, v ? ldv : n, m, n, "tsqr_mi_svd_f64 supports n <= 64")) return rc;
	return svd_f64_core(a_layout, u_layout, jobu, reorth, u, ldu, s, v, ldv, a, lda, m, n, reinterpret_cast<double*>(wq),
	                    reinterpret_cast<double*>(wr), stream);
}

size_t tsqr_mi_working_q_size_f64_qrcp(size_t m, size_t n, int jobq) { return f64_job_wq(m, n, jobq, F64P_WQ); }
size_t tsqr_mi_working_r_size_f64_qrcp(size_t m, size_t n, int jobq) { return f64_job_wr(m, n, jobq); }

int tsqr_mi_qrcp_f64(int a_layout, int q_layout, int jobq, int reorth, double* q, size_t ldq, double* r, size_t ldr, int* jpvt,
                     double* a, size_t lda, size_t m, size_t n, void* wq, void* wr, void* stream) {
	if (const int rc = f64_job_prologue(jobq, a_layout, q_layout, q, ldq, a, lda, ldr, m, n, "tsqr_mi_qrcp_f64 supports n <= 64")) return rc;
	return qrcp_f64_core(a_layout, q_layout, jobq, reorth, q, ldq, r, ldr, jpvt, a, lda, m, n, reinterpret_cast<double*>(wq),
	                     reinterpret_cast<double*>(wr), stream);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------------
// The rank-aware least-squares entry (tsqr_mi_lstsq_rank_f64; n <= 64, nrhs <= 16; kernels: lsq_rank_f64.hip).  The ladder and the
// pivoted QR of R0 are tsqr_mi_qrcp_f64's with jobq = 0, launch for launch: tsqr_mi_r_f64_lay as it stands with R0 into the caller's r
// -- it blocks, it reads its verdict words -- then qrcp_r_f64_kernel in place on r with h == null.  Behind it, back to back on the idle
// stream with one wait at the end: lsq_rank_f64_kernel (the rank into a status word and a pinned word, Zeff into wq[F64K_ZEFF]); the
// CholeskyQR step on the retained columns -- gramq_dense_f64_kernel on Zeff, the reduction into wq[F64K_G1], lsq_rank_step_f64_kernel
// (Zeff <- Zeff inverse(Rc), its verdict into a status word and a pinned word); refine + 1 passes, each lsq_dense_f64_kernel
// (D = (A Zeff)^T (B - A X), X null the first time), the reduction and X <- X + Zeff D (lsq_update_f64_kernel<true>) under the
// stagnation rule of lstsq_f64_core with its state in wq[F64L_DPREV].  The two pinned words are the thread's verdict words, which the
// ladder has finished with when it returns (as svd_f64_core keeps its words).
// The minimum-norm entry (tsqr_mi_lstsq_minnorm_f64) is the same sequence with three changes: lsq_zg_f64_kernel in front of the Gram
// pass (Zeff -> Zg, so that the same tiles also hold G12), lsq_minnorm_f64_kernel behind the step (Zmn into wq[F64M_ZMN], its verdict
// into status word [2] and a third pinned word), and Zmn in place of Zeff as the factor of the update.  Every other launch, and every
// launch of the basic entry, is unchanged.
// ---------------------------------------------------------------------------------------------------------------------------
namespace {

// the texts of an entry of this family: the basic one and the minimum-norm one differ in their names alone
struct LstsqRankTexts {
	const char *n_max, *nrhs_max, *refine_range, *rcond_range, *step_pivot;
};
const LstsqRankTexts LSTSQ_RANK_TEXTS{
	"tsqr_mi_lstsq_rank_f64 supports n <= 64", "tsqr_mi_lstsq_rank_f64 supports nrhs <= 16", "tsqr_mi_lstsq_rank_f64 supports 0 <= refine <= 4",
	"tsqr_mi_lstsq_rank_f64 supports rcond < 1 (negative: max(m, n) 2^-52)",
	"tsqr_mi_lstsq_rank_f64: the Cholesky step on the retained columns met a pivot that is not positive or not finite"};
const LstsqRankTexts LSTSQ_MINNORM_TEXTS{
	"tsqr_mi_lstsq_minnorm_f64 supports n <= 64", "tsqr_mi_lstsq_minnorm_f64 supports nrhs <= 16",
	"tsqr_mi_lstsq_minnorm_f64 supports 0 <= refine <= 4", "tsqr_mi_lstsq_minnorm_f64 supports rcond < 1 (negative: max(m, n) 2^-52)",
	"tsqr_mi_lstsq_minnorm_f64: the Cholesky step on the retained columns met a pivot that is not positive or not finite"};

template <bool MINNORM>
int lstsq_rank_f64_core(int a_layout, int b_layout, int reorth, int refine, double rcond, double* x, size_t ldx, double* r, size_t ldr,
                        int* jpvt, int* rank, const double* a, size_t lda, const double* b, size_t ldb, size_t m, size_t n, size_t nrhs,
                        double* wq, double* wr, void* stream) {
	const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
	if (const int rc = tsqr_mi_r_f64_lay(a_layout, reorth, r, ldr, a, lda, m, n, wq, wr, stream)) return rc;   // (state 3 included: nothing else ran)
	tsqrmi::QrcpArgs64 pa{};
	pa.r0 = r; pa.ldr0 = ldr; pa.r = r; pa.ldr = ldr; pa.jpvt = jpvt; pa.n = (int)n; pa.h = nullptr; pa.status = nullptr;
	f64_qrcp_r_launch(st, pa);
	HIPCHK(hipGetLastError());
	volatile unsigned* words = t_own64.host;             // (the ladder allocated them and has read its verdicts: the stream is idle)
	words[0] = 0u; words[1] = 1u;                        // (a step kernel that never reported reads as failed)
	if constexpr (MINNORM) words[2] = 2u;                // (and so does lsq_minnorm_f64_kernel)
	double *zeff = wq + F64K_ZEFF, *xw = wq + F64L_X, *dsum = wq + F64L_D;
	const double* zupd = MINNORM ? wq + F64M_ZMN : zeff;     // the factor of the update X <- X + zupd D
	unsigned* status = reinterpret_cast<unsigned*>(wq + F64K_STATUS);
	tsqrmi::LsqRankArgs64 ka{};
	ka.r = r; ka.ldr = ldr; ka.jpvt = jpvt; ka.rcond = rcond; ka.zeff = zeff; ka.status = status; ka.host_status = t_own64.dev; ka.n = (int)n;
	f64k_rank_launch(st, ka);
	HIPCHK(hipGetLastError());
	const F64Plan g = f64r_plan(m, n);
	if (g.nblocks <= 0) { t_last_error = "fp64 least-squares pass without partials"; return TSQR_MI_ERROR_INVALID_SIZE; }
	if constexpr (MINNORM) {
		tsqrmi::LsqZgArgs64 za{};
		za.jpvt = jpvt; za.rank = status; za.zeff = zeff; za.n = (int)n;
		f64k_zg_launch(st, za);
		HIPCHK(hipGetLastError());
	}
	const tsqrmi::GramQArgs64 ga{a, lda, m, (int)n, g.nunits, g.nwaves, zeff, wr};
	f64k_gramq_launch(st, g, ga, a_layout);
	HIPCHK(hipGetLastError());
	launch_reduce1(st, wq + F64K_G1, wr, g.nblocks, g.ntri * 256, (double)m);
	HIPCHK(hipGetLastError());
	tsqrmi::LsqRankStepArgs64 sa{};
	sa.gsum = wq + F64K_G1; sa.rank = status; sa.zeff = zeff; sa.status = status + 1; sa.host_status = t_own64.dev + 1; sa.n = (int)n;
	f64k_step_launch(st, sa);
	HIPCHK(hipGetLastError());
	if constexpr (MINNORM) {
		tsqrmi::LsqMinnormArgs64 ma{};
		ma.gsum = wq + F64K_G1; ma.rank = status; ma.jpvt = jpvt; ma.zeff = zeff; ma.zmn = wq + F64M_ZMN; ma.status = status + 2;
		ma.host_status = t_own64.dev + 2; ma.n = (int)n;
		f64k_minnorm_launch(st, ma);
		HIPCHK(hipGetLastError());
	}
	for (int p = 0; p <= refine; p++) {
		const tsqrmi::LsqArgs64 la{a, lda, b, ldb, m, (int)n, (int)nrhs, g.nunits, g.nwaves, zeff, p == 0 ? nullptr : xw, wr};
		f64k_lsq_launch(st, g, la, a_layout, b_layout);
		HIPCHK(hipGetLastError());
		launch_reduce1(st, dsum, wr, g.nblocks, g.NT * 256, (double)m);
		HIPCHK(hipGetLastError());
		f64_lsq_update_launch<true>(st, xw, x, ldx, zupd, dsum, (int)n, (int)nrhs, p == 0 ? 1 : 0, p == refine ? 1 : 0, wq + F64L_DPREV,
		                            p >= 2 ? 1 : 0);
		HIPCHK(hipGetLastError());
	}
	HIPCHK(hipStreamSynchronize(st));
	*rank = (int)words[0];
	if (words[1] != 0u) {
		t_last_error = (MINNORM ? LSTSQ_MINNORM_TEXTS : LSTSQ_RANK_TEXTS).step_pivot;
		return TSQR_MI_ERROR_NOT_FINITE;
	}
	if constexpr (MINNORM) {
		if (words[2] != 0u) {
			t_last_error = "tsqr_mi_lstsq_minnorm_f64: the Cholesky factorisation of C = I + M M^T met a pivot that is not positive or not finite";
			return TSQR_MI_ERROR_NOT_FINITE;
		}
	}
	return TSQR_MI_SUCCESS;
}

// the entry of either form: every state that does not need the device is decided here, before any HIP call; the null checks first of all
template <bool MINNORM>
int lstsq_rank_f64_entry(int a_layout, int b_layout, int reorth, int refine, double rcond, double* x, size_t ldx, double* r, size_t ldr,
                         int* jpvt, int* rank, const double* a, size_t lda, const double* b, size_t ldb, size_t m, size_t n, size_t nrhs,
                         void* wq, void* wr, void* stream) {
	const LstsqRankTexts& tx = MINNORM ? LSTSQ_MINNORM_TEXTS : LSTSQ_RANK_TEXTS;
	t_sweeps64 = 0;
	if (!x || !r || !jpvt || !rank || !a || !b || !wq || !wr) return TSQR_MI_ERROR_INVALID_SIZE;
	const F64Operand A{a_layout, m, n, lda}, B{b_layout, m, nrhs, ldb}, R{TSQR_MI_COL_MAJOR, n, n, ldr}, X{TSQR_MI_COL_MAJOR, n, nrhs, ldx};
	if (const int rc = f64_prologue({A, B, R, X}, m, n, PW, tx.n_max)) return rc;
	if (nrhs > F64L_MAX_NRHS) { t_last_error = tx.nrhs_max; return TSQR_MI_ERROR_UNSUPPORTED; }
	if (refine < 0 || refine > F64L_MAX_REFINE) { t_last_error = tx.refine_range; return TSQR_MI_ERROR_UNSUPPORTED; }
	if (!(rcond < 1.0)) { t_last_error = tx.rcond_range; return TSQR_MI_ERROR_UNSUPPORTED; }
	if (rcond < 0.0) rcond = (double)std::max(m, n) * 0x1p-52;
	return lstsq_rank_f64_core<MINNORM>(a_layout, b_layout, reorth, refine, rcond, x, ldx, r, ldr, jpvt, rank, a, lda, b, ldb, m, n, nrhs,
	                                    reinterpret_cast<double*>(wq), reinterpret_cast<double*>(wr), stream);
}

}  // namespace

extern "C" {

size_t tsqr_mi_working_q_size_f64_lstsq_rank(size_t m, size_t n, size_t nrhs) { return (m == 0 || n == 0 || nrhs == 0) ? 0 : F64K_WQ; }
size_t tsqr_mi_working_r_size_f64_lstsq_rank(size_t m, size_t n, size_t nrhs) {
	return (m == 0 || n == 0 || nrhs == 0) ? 0 : f64r_wr_doubles(m, std::min(n, PW));
}

int tsqr_mi_lstsq_rank_f64(int a_layout, int b_layout, int reorth, int refine, double rcond, double* x, size_t ldx, double* r, size_t ldr,
                           int* jpvt, int* rank, const double* a, size_t lda, const double* b, size_t ldb, size_t m, size_t n, size_t nrhs,
                           void* wq, void* wr, void* stream) {
	return lstsq_rank_f64_entry<false>(a_layout, b_layout, reorth, refine, rcond, x, ldx, r, ldr, jpvt, rank, a, lda, b, ldb, m, n, nrhs, wq, wr,
	                                   stream);
}

size_t tsqr_mi_working_q_size_f64_lstsq_minnorm(size_t m, size_t n, size_t nrhs) { return (m == 0 || n == 0 || nrhs == 0) ? 0 : F64M_WQ; }
size_t tsqr_mi_working_r_size_f64_lstsq_minnorm(size_t m, size_t n, size_t nrhs) { return tsqr_mi_working_r_size_f64_lstsq_rank(m, n, nrhs); }

int tsqr_mi_lstsq_minnorm_f64(int a_layout, int b_layout, int reorth, int refine, double rcond, double* x, size_t ldx, double* r, size_t ldr,
                              int* jpvt, int* rank, const double* a, size_t lda, const double* b, size_t ldb, size_t m, size_t n, size_t nrhs,
                              void* wq, void* wr, void* stream) {
	return lstsq_rank_f64_entry<true>(a_layout, b_layout, reorth, refine, rcond, x, ldx, r, ldr, jpvt, rank, a, lda, b, ldb, m, n, nrhs, wq, wr,
	                                  stream);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------------
// Block orthogonalisation against an existing basis (tsqr_mi_orth_f64; n <= 64, k <= 1024; kernels: orth_f64.hip): BCGS2 with the
// n <= 64 ladder as the inner QR.  Round i of `passes`: the cross-Gram pass and its reduction (Si = V^T X into wq[F64O_SW]), the
// projection update X <- X - V Si in place in w, the caller's S (round 1: S = S1; round 2: S += S2 R1, with R1 still in the caller's r),
// all enqueued back to back, then the ladder of tsqr_mi_qr_f64_lay in place on w (qr_f64_core as that entry calls it; it blocks, it
// reads its verdict words) with R into the caller's r (round 1) or into wq[F64O_RW] (round 2), and behind round 2 r <- R2 r
// (trimul_f64_kernel) with one more wait.  The sweep count is the sum over the rounds, plus 100 when either took the shifted path.
// ---------------------------------------------------------------------------------------------------------------------------
namespace {

int orth_f64_core(int v_layout, int w_layout, int passes, int reorth, double* w, size_t ldw, double* s, size_t lds, double* r, size_t ldr,
                  const double* v, size_t ldv, size_t m, size_t k, size_t n, double* wq, double* wr, void* stream) {
	const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
	const F64OPlan g = f64o_plan(m, k, n);
	if (g.nslices <= 0 || g.kblocks <= 0) { t_last_error = "fp64 cross-Gram pass without partials"; return TSQR_MI_ERROR_INVALID_SIZE; }
	double *sw = wq + F64O_SW, *rw = wq + F64O_RW;
	const int NP = 16 * g.NT;
	int sweeps = 0;
	bool shifted = false;
	for (int round = 0; round < passes; round++) {
		const tsqrmi::OrthGramArgs64 ga{v, ldv, w, ldw, m, (int)k, (int)n, g.kblocks, g.nslices, g.cps, g.nch, wr};
		f64o_gram_launch(st, g, ga, v_layout, w_layout);
		HIPCHK(hipGetLastError());
		launch_reduce1(st, sw, wr, g.nslices, g.kblocks * 64 * NP, (double)m);
		HIPCHK(hipGetLastError());
		const tsqrmi::OrthUpdateArgs64 ua{w, ldw, v, ldv, m, (int)k, (int)n, g.kblocks, sw};
		f64o_update_launch(st, g, ua, v_layout, w_layout);
		HIPCHK(hipGetLastError());
		const tsqrmi::OrthSArgs64 sa{s, lds, sw, r, ldr, (int)k, (int)n, NP, round};
		f64o_s_launch(st, sa);
		HIPCHK(hipGetLastError());
		const int rc = qr_f64_core(reorth, w, ldw, round ? rw : r, round ? 64 : ldr, w, ldw, m, n, wq, wr, stream, nullptr, w_layout, w_layout);
		sweeps += t_sweeps64 % 100;
		shifted = shifted || t_sweeps64 >= 100;
		t_sweeps64 = sweeps + (shifted ? 100 : 0);
		if (rc) return rc;                                   // (state 3 included: w, s and r are undefined)
	}
	if (passes == 2) {
		f64_rmul_launch(st, r, ldr, rw, (int)n);
		HIPCHK(hipGetLastError());
		HIPCHK(hipStreamSynchronize(st));
	}
	return TSQR_MI_SUCCESS;
}

}  // namespace

extern "C" {

size_t tsqr_mi_working_q_size_f64_orth(size_t m, size_t k, size_t n) { return (m == 0 || k == 0 || n == 0) ? 0 : f64o_wq_doubles(k); }
size_t tsqr_mi_working_r_size_f64_orth(size_t m, size_t k, size_t n) {
	return (m == 0 || k == 0 || n == 0) ? 0 : f64o_wr_doubles(m, k, std::min(n, PW));
}

// every state 1 is decided here, before any HIP call; the null checks first of all
int tsqr_mi_orth_f64(int v_layout, int w_layout, int passes, int reorth, double* w, size_t ldw, double* s, size_t lds, double* r, size_t ldr,
                     const double* v, size_t ldv, size_t m, size_t k, size_t n, void* wq, void* wr, void* stream) {
	t_sweeps64 = 0;
	if (!w || !s || !r || !v || !wq || !wr) return TSQR_MI_ERROR_INVALID_SIZE;
	if (passes != 1 && passes != 2) return TSQR_MI_ERROR_INVALID_SIZE;
	if (n == 0 || n > PW || k == 0 || k > F64O_MAX_K || m < k || m - k < n) return TSQR_MI_ERROR_INVALID_SIZE;
	const F64Operand V{v_layout, m, k, ldv}, W{w_layout, m, n, ldw}, S{TSQR_MI_COL_MAJOR, k, n, lds}, R{TSQR_MI_COL_MAJOR, n, n, ldr};
	if (const int rc = f64_prologue({V, W, S, R}, m, n, PW, "tsqr_mi_orth_f64 supports n <= 64")) return rc;
	if (const int rc = latch_all()) return rc;           // (tickets of tsqr_mi_qr_f32_submit in flight: their verdicts first)
	return orth_f64_core(v_layout, w_layout, passes, reorth, w, ldw, s, lds, r, ldr, v, ldv, m, k, n, reinterpret_cast<double*>(wq),
	                     reinterpret_cast<double*>(wr), stream);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------------
// The wide fp64 entry (tsqr_mi_qr_f64_wide): n <= 64 is tsqr_mi_qr_f64 itself; 64 < n <= 1024 runs the same ladder (qr_f64_core) with
// whole-matrix sweeps on nb = ceil(n / 64) column blocks (f64w_sweep, beside f64_sweep above; kernels and block storage:
// tsqr_f64_wide.hip).
// ---------------------------------------------------------------------------------------------------------------------------
extern "C" {

size_t tsqr_mi_working_q_size_f64_wide(size_t m, size_t n) {
	if (m == 0 || n == 0) return 0;
	if (n <= PW) return tsqr_mi_working_q_size_f64(m, n);
	return f64w_plan(m, std::min(n, F64W_MAX_N)).wq;
}
size_t tsqr_mi_working_r_size_f64_wide(size_t m, size_t n) {
	if (m == 0 || n == 0) return 0;
	if (n <= PW) return tsqr_mi_working_r_size_f64(m, n);
	const F64WPlan g = f64w_plan(m, std::min(n, F64W_MAX_N));
	return (size_t)g.nslices * g.bs;
}

int tsqr_mi_qr_f64_wide_lay(int a_layout, int q_layout, int reorth, double* q, size_t ldq, double* r, size_t ldr, double* a, size_t lda,
                            size_t m, size_t n, void* wq, void* wr, void* stream) {
	const F64Operand A{a_layout, m, n, lda}, Q{q_layout, m, n, ldq}, R{TSQR_MI_COL_MAJOR, n, n, ldr};
	if (const int rc = f64_prologue({A, Q, R}, m, n, F64W_MAX_N, "tsqr_mi_qr_f64_wide supports n <= 1024")) return rc;
	if (f64_in_place_broken(q, q_layout, ldq, a, a_layout, lda)) return TSQR_MI_ERROR_INVALID_SIZE;
	if (n <= PW) return tsqr_mi_qr_f64_lay(a_layout, q_layout, reorth, q, ldq, r, ldr, a, lda, m, n, wq, wr, stream);
	if (const int rc = latch_all()) return rc;           // (tickets of tsqr_mi_qr_f32_submit in flight: their verdicts first)
	return qr_f64_core(reorth, q, ldq, r, ldr, a, lda, m, n, wq, wr, stream, nullptr, a_layout, q_layout);
}

int tsqr_mi_qr_f64_wide(int reorth, double* q, size_t ldq, double* r, size_t ldr, double* a, size_t lda, size_t m, size_t n,
                        void* wq, void* wr, void* stream) {
	return tsqr_mi_qr_f64_wide_lay(TSQR_MI_COL_MAJOR, TSQR_MI_COL_MAJOR, reorth, q, ldq, r, ldr, a, lda, m, n, wq, wr, stream);
}

// ---- row-partitioned fp64: one call per rank, the ladder of tsqr_mi_qr_f64_wide with the exchange of f64_exchange in every sweep ----
size_t tsqr_mi_working_q_size_f64_dist(size_t m_local, size_t n, int /*nranks*/) { return tsqr_mi_working_q_size_f64_wide(m_local, n); }
size_t tsqr_mi_working_r_size_f64_dist(size_t m_local, size_t n, int /*nranks*/) { return tsqr_mi_working_r_size_f64_wide(m_local, n); }

// every state that does not need the device is decided here, before any HIP call and before any collective
static int qr_f64_dist(const Comm& comm, int reorth, double* q, size_t ldq, double* r, size_t ldr, double* a, size_t lda,
                       size_t m_local, size_t n, void* wq, void* wr, void* stream) {
	t_sweeps64 = 0;
	if (m_local == 0 || n == 0 || ldq < m_local || lda < m_local || ldr < n) {
		t_last_error = "tsqr_mi_qr_f64_dist: m_local >= 1, n >= 1, ldq >= m_local, lda >= m_local and ldr >= n are required";
		return TSQR_MI_ERROR_INVALID_SIZE;
	}
	if (n > F64W_MAX_N) { t_last_error = "tsqr_mi_qr_f64_dist supports n <= 1024"; return TSQR_MI_ERROR_UNSUPPORTED; }
	if (!comm.active()) {
		t_last_error = "tsqr_mi_qr_f64_dist needs an all-reduce: a callback, or an ncclComm_t with the ncclAllReduce entry point of the library that created it";
		return TSQR_MI_ERROR_UNSUPPORTED;
	}
	if (const int rc = latch_all()) return rc;           // (tickets of tsqr_mi_qr_f32_submit in flight: their verdicts first)
	return qr_f64_core(reorth, q, ldq, r, ldr, a, lda, m_local, n, wq, wr, stream, &comm, TSQR_MI_COL_MAJOR, TSQR_MI_COL_MAJOR);
}

int tsqr_mi_qr_f64_dist_cb(int reorth, double* q, size_t ldq, double* r, size_t ldr, double* a, size_t lda, size_t m_local, size_t n,
                           void* wq, void* wr, tsqr_mi_allreduce_f64_cb allreduce, void* user, int nranks, void* stream) {
	Comm comm;
	comm.nranks = nranks; comm.cb_allreduce = allreduce; comm.cb_user = user;
	return qr_f64_dist(comm, reorth, q, ldq, r, ldr, a, lda, m_local, n, wq, wr, stream);
}
int tsqr_mi_qr_f64_dist_fn(int reorth, double* q, size_t ldq, double* r, size_t ldr, double* a, size_t lda, size_t m_local, size_t n,
                           void* wq, void* wr, void* nccl_comm, void* nccl_allreduce_fn, int nranks, void* stream) {
	Comm comm;
	comm.nranks = nranks;
	if (nccl_comm && nccl_allreduce_fn) { comm.nccl = nccl_comm; comm.nccl_allreduce = reinterpret_cast<nccl_allreduce_t>(nccl_allreduce_fn); }
	return qr_f64_dist(comm, reorth, q, ldq, r, ldr, a, lda, m_local, n, wq, wr, stream);
}
int tsqr_mi_qr_f64_dist(int reorth, double* q, size_t ldq, double* r, size_t ldr, double* a, size_t lda, size_t m_local, size_t n,
                        void* wq, void* wr, void* nccl_comm, int nranks, void* stream) {
	// (null when the caller does not link RCCL: state 2 with its text, after the size checks)
	return tsqr_mi_qr_f64_dist_fn(reorth, q, ldq, r, ldr, a, lda, m_local, n, wq, wr, nccl_comm, rccl_symbol("ncclAllReduce"), nranks, stream);
}

}  // extern "C"

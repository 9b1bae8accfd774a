// selftest_f64.hip -- one entry per pass of the fp64 entries (tsqr_mi_qr_f64: tsqr_f64.hip; tsqr_mi_qr_f64_wide: tsqr_f64_wide.hip), for
// tests/test_gpu_f64_passes.py.  Included by selftest.hip.  Every entry launches the product's kernels with the product's plan
// (f64_plan.h: the definitions libtsqr_mi.so is built from), the way f64_factor / f64_sweep / f64w_sweep of tsqr_mi.hip do, waits, and
// returns 0, minus a HIP error, or -100 when an operand of the caller is too small for the plan.  The Gram and apply entries take an
// override of the partition (0: the product's), so that a matrix of a few hundred rows reaches every edge of it.

namespace {
inline int f64_sync() {
	HIPCHK(hipGetLastError());
	HIPCHK(hipDeviceSynchronize());
	return 0;
}
}  // namespace

// apply_f64_kernel<NT, AROW, QROW>: q = a z (z: NP x NP).  wgs > 0 overrides the grid; 0: the resident workgroups of that instantiation,
// as f64_apply takes them
namespace {
template <int NT, bool AROW, bool QROW>
int selftest_f64_apply(double* q, size_t ldq, const double* a, size_t lda, size_t m, int n, const double* z, int wgs_over) {
	const size_t nblocks = cdiv(m, 32);
	size_t wgs = (size_t)wgs_over;
	if (wgs_over <= 0) {
		int dev = 0;
		(void)hipGetDevice(&dev);
		wgs = f64_apply_wgs(nblocks, (size_t)f64_apply_resident<NT, AROW, QROW>(dev));
	}
	hipLaunchKernelGGL((tsqrmi::apply_f64_kernel<NT, AROW, QROW>), dim3((unsigned)wgs), dim3(256), 0, 0, q, ldq, a, lda, m, n, z, nblocks);
	return f64_sync();
}
}  // namespace

// the nwaves override of the Gram, gramq and lsq entries (0: the plan's); false when `part` has no room for the partials of `tiles` tiles
namespace {
inline bool f64_override(F64Plan& g, int nwaves, int tiles, size_t part_cap) {
	if (nwaves > 0) { g.nwaves = nwaves; g.nblocks = (nwaves + 3) / 4; }
	return g.nblocks > 0 && (size_t)g.nblocks * tiles * 256 <= part_cap;
}
}  // namespace

namespace {
__global__ __launch_bounds__(64) void f64_rule_probe_kernel(const double* rows, const int* n, const int* first, int count, double* out) {
	const int i = blockIdx.x * 64 + threadIdx.x;
	if (i >= count) return;
	const tsqrmi::F64Rule r = tsqrmi::f64_rule_of(rows[i], n[i], first[i] != 0);
	out[3 * i] = (double)r.max_scond; out[3 * i + 1] = (double)r.alone_max; out[3 * i + 2] = r.shift_coef;
}
}  // namespace

extern "C" {

// out[0..7]: NT, ntri, nch, nwaves, nblocks, doubles of wq, doubles of wr (the partials), F64_GRAM_WAVES.  Host only.
int tsqr_selftest_f64_plan(size_t m, size_t n, long long* out) {
	if (m == 0 || n == 0 || n > PW) return -100;
	const F64Plan g = f64_plan(m, n);
	out[0] = g.NT; out[1] = g.ntri; out[2] = g.nunits; out[3] = g.nwaves; out[4] = g.nblocks;
	out[5] = (long long)F64_WQ; out[6] = (long long)g.nblocks * g.ntri * 256; out[7] = F64_GRAM_WAVES;
	return 0;
}

// the acceptance rule of an m x n sweep as the launches take it (f64_rule): out[0] max_scond, [1] alone_max, [2] shift_coef.  Host only.
int tsqr_selftest_f64_rule(size_t m, size_t n, int first, double* out) {
	if (m == 0 || n == 0 || n > F64W_MAX_N) return -100;
	const F64Rule r = f64_rule(m, n, first != 0);
	out[0] = (double)r.max_scond; out[1] = (double)r.alone_max; out[2] = r.shift_coef;
	return 0;
}

// The same rule as the DEVICE evaluates it (f64_rule_of inside a kernel: what chol_f64_kernel, cholw_verdict_kernel and wide_shift do in a
// row-partitioned call, whose row count exists on the device only): case i takes rows[i], n[i], first[i] and leaves out[3 i .. 3 i + 2] =
// max_scond, alone_max, shift_coef.  All four arrays are device memory.
int tsqr_selftest_f64_rule_device(const double* rows, const int* n, const int* first, int count, double* out) {
	if (count <= 0) return -100;
	hipLaunchKernelGGL(f64_rule_probe_kernel, dim3((unsigned)cdiv((size_t)count, 64)), dim3(64), 0, 0, rows, n, first, count, out);
	return f64_sync();
}

// out[0..19]: nb, npairs, ngroups, nslices, cps, nch, bs, o_gs, o_w, o_rw, o_zw, o_ta, o_rc, o_zd, o_sb, o_bst, o_status, wq,
// doubles of wr (the partials), F64W_WR_CAP.  Host only.
int tsqr_selftest_f64w_plan(size_t m, size_t n, long long* out) {
	if (m == 0 || n <= PW || n > F64W_MAX_N) return -100;
	const F64WPlan g = f64w_plan(m, n);
	const long long v[20] = {g.nb, g.npairs, g.ngroups, g.nslices, (long long)g.cps, (long long)g.nch, (long long)g.bs, (long long)g.o_gs,
	                         (long long)g.o_w, (long long)g.o_rw, (long long)g.o_zw, (long long)g.o_ta, (long long)g.o_rc, (long long)g.o_zd,
	                         (long long)g.o_sb, (long long)g.o_bst, (long long)g.o_status, (long long)g.wq,
	                         (long long)((size_t)g.nslices * g.bs), (long long)F64W_WR_CAP};
	for (int i = 0; i < 20; i++) out[i] = v[i];
	return 0;
}

// ---- n <= 64 --------------------------------------------------------------------------------------------------------------------------
// The Gram, gramq and lsq entries come in two forms: _lay takes a layout per operand (0 column-major; 1 row-major, the leading dimension
// is then the row stride: lda >= n, ldb >= nrhs) and goes through the launchers the product uses (f64_plan.h); the plain entry is _lay
// at layout 0.  nwaves > 0 overrides the plan's wave count -- the same partition for every layout, so the partials in `part` (part_cap
// doubles) can be compared one by one.
// Gram pass + reduction: gsum[ntri * 256 + 1] (the row count behind the tiles).
int tsqr_selftest_f64_gram_lay(int a_layout, double* gsum, const double* a, size_t lda, size_t m, int n, double* part, size_t part_cap, int nwaves) {
	if (a_layout != 0 && a_layout != 1) return -100;
	if (m == 0 || n <= 0 || n > (int)PW || lda < (a_layout ? (size_t)n : m)) return -100;
	F64Plan g = f64_plan(m, (size_t)n);
	if (!f64_override(g, nwaves, g.ntri, part_cap)) return -100;
	const tsqrmi::GramArgs64 ga{a, lda, m, n, g.nunits, g.nwaves, part};
	f64_gram_launch(0, g, ga, a_layout);
	HIPCHK(hipGetLastError());
	launch_reduce1(0, gsum, part, g.nblocks, g.ntri * 256, (double)m);
	return f64_sync();
}
int tsqr_selftest_f64_gram(double* gsum, const double* a, size_t lda, size_t m, int n, double* part, size_t part_cap, int nwaves) {
	return tsqr_selftest_f64_gram_lay(0, gsum, a, lda, m, n, part, part_cap, nwaves);
}

// chol_f64_kernel with the thresholds and the shift of an m x n first sweep (first = 1) or of a later one (0): r (n x n, ldr),
// z (NP x NP), status[4], host_words[4] (device memory standing in for the pinned words)
int tsqr_selftest_f64_chol(double* r, size_t ldr, double* z, unsigned* status, unsigned* host_words, const double* gsum, size_t m, int n,
                           int first) {
	if (m == 0 || n <= 0 || n > (int)PW || ldr < (size_t)n) return -100;
	tsqrmi::CholArgs64 ca{};
	ca.r = r; ca.ldr = ldr; ca.z = z; ca.status = status; ca.host_status = host_words; ca.gsum = gsum;
	const F64Rule rule = f64_rule(m, (size_t)n, first != 0);
	ca.shift_coef = rule.shift_coef; ca.max_scond = rule.max_scond; ca.alone_max = rule.alone_max;
	ca.n = n; ca.NT = (int)(np_of((size_t)n) / 16);
	hipLaunchKernelGGL(tsqrmi::chol_f64_kernel, dim3(1), dim3(1024), 0, 0, ca);
	return f64_sync();
}

// The apply pass in two forms, like the Gram entries above: _lay takes the layout of the operand read and of the operand written (1:
// row-major, the leading dimension is then the row stride, >= n); the plain entry is _lay at layouts 0.  q == a (in place) needs equal
// layouts and leading dimensions.
int tsqr_selftest_f64_apply_lay(int a_layout, int q_layout, double* q, size_t ldq, const double* a, size_t lda, size_t m, int n,
                                const double* z, int wgs) {
	if ((a_layout != 0 && a_layout != 1) || (q_layout != 0 && q_layout != 1)) return -100;
	if (m == 0 || n <= 0 || n > (int)PW || lda < (a_layout ? (size_t)n : m) || ldq < (q_layout ? (size_t)n : m) || wgs > 65535) return -100;
	if (q == a && (a_layout != q_layout || ldq != lda)) return -100;
	return with_apply((size_t)n, a_layout, q_layout, [&](auto nt, auto ar, auto qr) {
		return selftest_f64_apply<decltype(nt)::value, decltype(ar)::value, decltype(qr)::value>(q, ldq, a, lda, m, n, z, wgs);
	});
}
int tsqr_selftest_f64_apply(double* q, size_t ldq, const double* a, size_t lda, size_t m, int n, const double* z, int wgs) {
	return tsqr_selftest_f64_apply_lay(0, 0, q, ldq, a, lda, m, n, z, wgs);
}

// trimul_f64_kernel as f64_sweep launches it: r <- r2 r (r2 packed with ld 64), in place
int tsqr_selftest_f64_rmul(double* r, size_t ldr, const double* r2, int n) {
	if (n <= 0 || n > (int)PW || ldr < (size_t)n) return -100;
	f64_rmul_launch(0, r, ldr, r2, n);
	return f64_sync();
}

// ---- n <= 64, R only (tsqr_mi_r_f64) ------------------------------------------------------------------------------------------------------
// out[0..7]: NT, ntri, ntiles, nwaves, nblocks, doubles of wq, doubles of wr (the larger of the two Gram plans' partials),
// F64R_GRAMQ_WAVES.  Host only.
int tsqr_selftest_f64r_plan(size_t m, size_t n, long long* out) {
	if (m == 0 || n == 0 || n > PW) return -100;
	const F64Plan g = f64r_plan(m, n);
	out[0] = g.NT; out[1] = g.ntri; out[2] = g.nunits; out[3] = g.nwaves; out[4] = g.nblocks;
	out[5] = (long long)F64R_WQ; out[6] = (long long)f64r_wr_doubles(m, n); out[7] = F64R_GRAMQ_WAVES;
	return 0;
}

// gramq_f64_kernel + reduction: gsum[ntri * 256 + 1] = the tiles of (a z)^T (a z) and the row count behind them; z: NP x NP (ld NP).
int tsqr_selftest_f64_gramq_lay(int a_layout, double* gsum, const double* a, size_t lda, size_t m, int n, const double* z, double* part,
                                size_t part_cap, int nwaves) {
	if (a_layout != 0 && a_layout != 1) return -100;
	if (m == 0 || n <= 0 || n > (int)PW || lda < (a_layout ? (size_t)n : m)) return -100;
	F64Plan g = f64r_plan(m, (size_t)n);
	if (!f64_override(g, nwaves, g.ntri, part_cap)) return -100;
	const tsqrmi::GramQArgs64 ga{a, lda, m, n, g.nunits, g.nwaves, z, part};
	f64r_gramq_launch(0, g, ga, a_layout);
	HIPCHK(hipGetLastError());
	launch_reduce1(0, gsum, part, g.nblocks, g.ntri * 256, (double)m);
	return f64_sync();
}
int tsqr_selftest_f64_gramq(double* gsum, const double* a, size_t lda, size_t m, int n, const double* z, double* part, size_t part_cap,
                            int nwaves) {
	return tsqr_selftest_f64_gramq_lay(0, gsum, a, lda, m, n, z, part, part_cap, nwaves);
}

// trimul_f64_kernel as f64r_zacc launches it: z <- z zk (both NP x NP with ld NP, NP = 16 ceil(n / 16)), in place
int tsqr_selftest_f64_zmul(double* z, const double* zk, int n) {
	if (n <= 0 || n > (int)PW) return -100;
	f64r_zmul_launch(0, z, zk, n);
	return f64_sync();
}

// ---- n <= 64, least squares (tsqr_mi_lstsq_f64) ---------------------------------------------------------------------------------------------
// lsq_f64_kernel + reduction, one pass: dsum[NT * 256 + 1] = the tiles of (a z)^T (b - a x) and the row count behind them; z: NP x NP
// (ld NP), x: NP x 16 (ld NP) or null = zero.
int tsqr_selftest_f64_lsq_lay(int a_layout, int b_layout, double* dsum, const double* a, size_t lda, const double* b, size_t ldb, size_t m,
                              int n, int nrhs, const double* z, const double* x, double* part, size_t part_cap, int nwaves) {
	if ((a_layout != 0 && a_layout != 1) || (b_layout != 0 && b_layout != 1)) return -100;
	if (m == 0 || n <= 0 || n > (int)PW || nrhs <= 0 || nrhs > (int)F64L_MAX_NRHS || lda < (a_layout ? (size_t)n : m) ||
	    ldb < (b_layout ? (size_t)nrhs : m))
		return -100;
	F64Plan g = f64r_plan(m, (size_t)n);
	if (!f64_override(g, nwaves, g.NT, part_cap)) return -100;
	const tsqrmi::LsqArgs64 la{a, lda, b, ldb, m, n, nrhs, g.nunits, g.nwaves, z, x, part};
	f64r_lsq_launch(0, g, la, a_layout, b_layout);
	HIPCHK(hipGetLastError());
	launch_reduce1(0, dsum, part, g.nblocks, g.NT * 256, (double)m);
	return f64_sync();
}
int tsqr_selftest_f64_lsq(double* dsum, const double* a, size_t lda, const double* b, size_t ldb, size_t m, int n, int nrhs,
                          const double* z, const double* x, double* part, size_t part_cap, int nwaves) {
	return tsqr_selftest_f64_lsq_lay(0, 0, dsum, a, lda, b, ldb, m, n, nrhs, z, x, part, part_cap, nwaves);
}

// lsq_update_f64_kernel: xw (NP x 16, ld NP) <- xw + z d (first: xw taken as zero), and x (n x nrhs, ldx) too when last
int tsqr_selftest_f64_lsq_update(double* xw, double* x, size_t ldx, const double* z, const double* d, int n, int nrhs, int first, int last) {
	if (n <= 0 || n > (int)PW || nrhs <= 0 || nrhs > (int)F64L_MAX_NRHS || ldx < (size_t)n) return -100;
	f64_lsq_update_launch(0, xw, x, ldx, z, d, n, nrhs, first, last, nullptr, 0);   // (no stagnation rule: every update is applied)
	return f64_sync();
}

// ---- n <= 64, the passes of the rank-aware least-squares entry (tsqr_mi_lstsq_rank_f64; lsq_rank_f64.hip) -----------------------------------
// lsq_dense_f64_kernel + reduction, one pass, with the arguments of tsqr_selftest_f64_lsq_lay: z is a dense NP x NP block (ld NP)
int tsqr_selftest_f64_lsq_dense_lay(int a_layout, int b_layout, double* dsum, const double* a, size_t lda, const double* b, size_t ldb,
                                    size_t m, int n, int nrhs, const double* z, const double* x, double* part, size_t part_cap, int nwaves) {
	if ((a_layout != 0 && a_layout != 1) || (b_layout != 0 && b_layout != 1)) return -100;
	if (m == 0 || n <= 0 || n > (int)PW || nrhs <= 0 || nrhs > (int)F64L_MAX_NRHS || lda < (a_layout ? (size_t)n : m) ||
	    ldb < (b_layout ? (size_t)nrhs : m))
		return -100;
	F64Plan g = f64r_plan(m, (size_t)n);
	if (!f64_override(g, nwaves, g.NT, part_cap)) return -100;
	const tsqrmi::LsqArgs64 la{a, lda, b, ldb, m, n, nrhs, g.nunits, g.nwaves, z, x, part};
	f64k_lsq_launch(0, g, la, a_layout, b_layout);
	HIPCHK(hipGetLastError());
	launch_reduce1(0, dsum, part, g.nblocks, g.NT * 256, (double)m);
	return f64_sync();
}

// lsq_rank_f64_kernel through the product's launcher: r (n x n upper triangular, ldr), jpvt[n] and rcond in; zeff (NP x NP, ld NP) and
// status[1] (the rank) out
int tsqr_selftest_f64_lsq_rank(const double* r, size_t ldr, const int* jpvt, double rcond, double* zeff, unsigned* status, int n) {
	if (n <= 0 || n > (int)PW || ldr < (size_t)n || !r || !jpvt || !zeff || !status) return -100;
	tsqrmi::LsqRankArgs64 ka{};
	ka.r = r; ka.ldr = ldr; ka.jpvt = jpvt; ka.rcond = rcond; ka.zeff = zeff; ka.status = status; ka.host_status = nullptr; ka.n = n;
	f64k_rank_launch(0, ka);
	return f64_sync();
}

// gramq_dense_f64_kernel + reduction with the arguments of tsqr_selftest_f64_gramq_lay: z is a dense NP x NP block (ld NP).  Every
// check, the null checks included, stands before any HIP call
int tsqr_selftest_f64_gramq_dense_lay(int a_layout, double* gsum, const double* a, size_t lda, size_t m, int n, const double* z, double* part,
                                      size_t part_cap, int nwaves) {
	if (a_layout != 0 && a_layout != 1) return -100;
	if (m == 0 || n <= 0 || n > (int)PW || lda < (a_layout ? (size_t)n : m) || !gsum || !a || !z || !part) return -100;
	F64Plan g = f64r_plan(m, (size_t)n);
	if (!f64_override(g, nwaves, g.ntri, part_cap)) return -100;
	const tsqrmi::GramQArgs64 ga{a, lda, m, n, g.nunits, g.nwaves, z, part};
	f64k_gramq_launch(0, g, ga, a_layout);
	HIPCHK(hipGetLastError());
	launch_reduce1(0, gsum, part, g.nblocks, g.ntri * 256, (double)m);
	return f64_sync();
}

// lsq_rank_step_f64_kernel through the product's launcher: gsum (the ntri summed tiles of G1) and rank[1] in; zeff (NP x NP, ld NP) in
// and out; status[1] (the verdict) out.  Every check stands before any HIP call
int tsqr_selftest_f64_lsq_rank_step(const double* gsum, const unsigned* rank, double* zeff, unsigned* status, int n) {
	if (n <= 0 || n > (int)PW || !gsum || !rank || !zeff || !status) return -100;
	tsqrmi::LsqRankStepArgs64 sa{};
	sa.gsum = gsum; sa.rank = rank; sa.zeff = zeff; sa.status = status; sa.host_status = nullptr; sa.n = n;
	f64k_step_launch(0, sa);
	return f64_sync();
}

// ---- the passes the minimum-norm entry adds (tsqr_mi_lstsq_minnorm_f64; lsq_rank_f64.hip) --------------------------------------------------
// lsq_zg_f64_kernel through the product's launcher: jpvt (n ints) and rank[1] in; zeff (NP x NP, ld NP) in and out.  Every check stands
// before any HIP call
int tsqr_selftest_f64_lsq_zg(const int* jpvt, const unsigned* rank, double* zeff, int n) {
	if (n <= 0 || n > (int)PW || !jpvt || !rank || !zeff) return -100;
	tsqrmi::LsqZgArgs64 za{};
	za.jpvt = jpvt; za.rank = rank; za.zeff = zeff; za.n = n;
	f64k_zg_launch(0, za);
	return f64_sync();
}

// lsq_minnorm_f64_kernel through the product's launcher: gsum (the ntri summed tiles of the Gram matrix on Zg), rank[1], jpvt (n ints)
// and zeff (NP x NP, ld NP) in; zmn (NP x NP, ld NP) and status[1] (the verdict) out.  Every check stands before any HIP call
int tsqr_selftest_f64_lsq_minnorm(const double* gsum, const unsigned* rank, const int* jpvt, const double* zeff, double* zmn, unsigned* status,
                                  int n) {
	if (n <= 0 || n > (int)PW || !gsum || !rank || !jpvt || !zeff || !zmn || !status) return -100;
	tsqrmi::LsqMinnormArgs64 ma{};
	ma.gsum = gsum; ma.rank = rank; ma.jpvt = jpvt; ma.zeff = zeff; ma.zmn = zmn; ma.status = status; ma.host_status = nullptr; ma.n = n;
	f64k_minnorm_launch(0, ma);
	return f64_sync();
}

// lsq_update_f64_kernel<dense> through the product's launcher with the stagnation rule: dprev (16 doubles, or null) and guard as the
// entries pass them; dense = 0 runs the triangular form on the same arguments
int tsqr_selftest_f64_lsq_update_rule(int dense, double* xw, double* x, size_t ldx, const double* z, const double* d, int n, int nrhs,
                                      int first, int last, double* dprev, int guard) {
	if (n <= 0 || n > (int)PW || nrhs <= 0 || nrhs > (int)F64L_MAX_NRHS || ldx < (size_t)n || (dense != 0 && dense != 1)) return -100;
	if (dense) f64_lsq_update_launch<true>(0, xw, x, ldx, z, d, n, nrhs, first, last, dprev, guard);
	else f64_lsq_update_launch<false>(0, xw, x, ldx, z, d, n, nrhs, first, last, dprev, guard);
	return f64_sync();
}

// ---- n <= 64, SVD (tsqr_mi_svd_f64) ---------------------------------------------------------------------------------------------------------
// svd_r_f64_kernel through the product's launcher: r (n x n upper triangular, ldr) in; s[n], w (NP x NP, ld NP), v (n x n, ldv; may be
// null) and status[2] (sweeps, 0 converged / 1 cap reached) out.  transpose: 1 the product's choice (the columns of R^T rotate), 0 those of R.
int tsqr_selftest_f64_svd_r(const double* r, size_t ldr, double* s, double* w, double* v, size_t ldv, unsigned* status, int n, int transpose) {
	if (n <= 0 || n > (int)PW || ldr < (size_t)n || (v && ldv < (size_t)n) || (transpose != 0 && transpose != 1)) return -100;
	tsqrmi::SvdArgs64 sa{};
	sa.r = r; sa.ldr = ldr; sa.s = s; sa.w = w; sa.v = v; sa.ldv = ldv; sa.status = status; sa.host_status = nullptr; sa.n = n;
	sa.transpose = transpose;
	f64_svd_r_launch(0, sa);
	return f64_sync();
}

// applyd_f64_kernel<NT, QROW, UROW>: u = q w (w: NP x NP, ld NP, zero padded) with the layout of the operand read and of the operand
// written, as tsqr_selftest_f64_apply_lay; wgs > 0 overrides the grid, 0: the resident workgroups of that instantiation, as f64_applyd
// takes them.  u == q (in place) needs equal layouts and leading dimensions.
int tsqr_selftest_f64_applyd_lay(int q_layout, int u_layout, double* u, size_t ldu, const double* q, size_t ldq, size_t m, int n,
                                 const double* w, int wgs) {
	if ((q_layout != 0 && q_layout != 1) || (u_layout != 0 && u_layout != 1)) return -100;
	if (m == 0 || n <= 0 || n > (int)PW || ldq < (q_layout ? (size_t)n : m) || ldu < (u_layout ? (size_t)n : m) || wgs > 65535) return -100;
	if (u == q && (q_layout != u_layout || ldu != ldq)) return -100;
	return with_apply((size_t)n, q_layout, u_layout, [&](auto nt, auto ar, auto qr) {
		constexpr int NT = decltype(nt)::value;
		constexpr bool AR = decltype(ar)::value, QR = decltype(qr)::value;
		size_t g = (size_t)wgs;
		if (wgs <= 0) {
			int dev = 0;
			(void)hipGetDevice(&dev);
			g = f64_apply_wgs(cdiv(m, 32), (size_t)f64_applyd_resident<NT, AR, QR>(dev));
		}
		f64_applyd_launch<NT, AR, QR>(0, g, u, ldu, q, ldq, m, n, w);
		return f64_sync();
	});
}

// ---- n <= 64, pivoted QR (tsqr_mi_qrcp_f64) -------------------------------------------------------------------------------------------------
// qrcp_r_f64_kernel through the product's launcher: r0 (n x n upper triangular, ldr0) in; r (n x n, ldr; may be r0 with ldr == ldr0),
// jpvt[n], h (NP x NP, ld NP; may be null: not formed) and status[2] (steps, exactly zero pivot columns; may be null) out.
int tsqr_selftest_f64_qrcp_r(const double* r0, size_t ldr0, double* r, size_t ldr, int* jpvt, double* h, unsigned* status, int n) {
	if (n <= 0 || n > (int)PW || ldr0 < (size_t)n || ldr < (size_t)n || !r0 || !r || !jpvt || (r == r0 && ldr != ldr0)) return -100;
	tsqrmi::QrcpArgs64 pa{};
	pa.r0 = r0; pa.ldr0 = ldr0; pa.r = r; pa.ldr = ldr; pa.jpvt = jpvt; pa.h = h; pa.status = status; pa.n = n;
	f64_qrcp_r_launch(0, pa);
	return f64_sync();
}

// ---- 64 < n <= 1024 ---------------------------------------------------------------------------------------------------------------------
// The Gram and apply entries come in two forms, like those of n <= 64 above: _lay takes a layout per operand (0 column-major; 1
// row-major, the leading dimension is then the row stride, >= n) and goes through the launchers the product uses (f64_plan.h); the plain
// entry is _lay at layout 0.
// Gram pass + reduction: gs[bs + 1] in the block store's layout.  cps > 0 overrides the chunks per slice -- the same partition for
// every layout; part holds part_cap doubles.
int tsqr_selftest_f64w_gram_lay(int a_layout, double* gs, const double* a, size_t lda, size_t m, int n, double* part, size_t part_cap,
                                size_t cps) {
	if (a_layout != 0 && a_layout != 1) return -100;
	if (m == 0 || n <= (int)PW || n > (int)F64W_MAX_N || lda < (a_layout ? (size_t)n : m)) return -100;
	F64WPlan g = f64w_plan(m, (size_t)n);
	if (cps > 0) { g.cps = cps; g.nslices = (int)cdiv(g.nch, g.cps); }
	if (g.nslices <= 0 || g.npairs <= 0 || (size_t)g.nslices * g.bs > part_cap) return -100;
	const tsqrmi::GramWideF64Args ga{a, lda, m, n, g.npairs, g.ngroups, g.cps, g.nch, part};
	f64w_gram_launch(0, g, ga, a_layout);
	HIPCHK(hipGetLastError());
	launch_reduce1(0, gs, part, g.nslices, (int)g.bs, (double)m);
	return f64_sync();
}
int tsqr_selftest_f64w_gram(double* gs, const double* a, size_t lda, size_t m, int n, double* part, size_t part_cap, size_t cps) {
	return tsqr_selftest_f64w_gram_lay(0, gs, a, lda, m, n, part, part_cap, cps);
}

// The blocked Cholesky step on the work space wq (f64w_plan(m, n).wq doubles, the summed blocks at o_gs), status slot 0, with the
// thresholds and the shift of an m x n first sweep.  mode 0: the plain chain; 1: the shifted chain alone (it looks at the verdict word
// the caller left in the status slot); 2: plain, then shifted, as f64w_sweep enqueues them.
int tsqr_selftest_f64w_chain(double* wq, size_t m, int n, int mode, unsigned* host_words) {
	if (m == 0 || n <= (int)PW || n > (int)F64W_MAX_N || mode < 0 || mode > 2) return -100;
	const F64WPlan g = f64w_plan(m, (size_t)n);
	tsqrmi::WideF64 wa{};
	wa.gs = wq + g.o_gs; wa.w = wq + g.o_w; wa.rw = wq + g.o_rw; wa.zw = wq + g.o_zw; wa.ta = wq + g.o_ta; wa.zd = wq + g.o_zd;
	wa.sb = wq + g.o_sb;
	wa.bst = reinterpret_cast<unsigned*>(wq + g.o_bst);
	wa.status = reinterpret_cast<unsigned*>(wq + g.o_status);
	wa.host_status = host_words;
	const F64Rule rule = f64_rule(m, (size_t)n, true);
	wa.max_scond = rule.max_scond; wa.alone_max = rule.alone_max;
	wa.n = n; wa.nb = g.nb;
	wa.run_if = nullptr; wa.shift_coef = 0.0;
	if (mode != 1) {
		const int rc = f64w_chain(0, wa);
		if (rc) return rc;
	}
	if (mode != 0) {
		wa.run_if = wa.status; wa.shift_coef = rule.shift_coef;
		const int rc = f64w_chain(0, wa);
		if (rc) return rc;
	}
	return f64_sync();
}

// apply_wide_f64_kernel<AROW, QROW>: q = a Z, Z in the block store zw.  q == a (in place) needs equal layouts and leading dimensions.
int tsqr_selftest_f64w_apply_lay(int a_layout, int q_layout, double* q, size_t ldq, const double* a, size_t lda, size_t m, int n,
                                 const double* zw) {
	if ((a_layout != 0 && a_layout != 1) || (q_layout != 0 && q_layout != 1)) return -100;
	if (m == 0 || n <= (int)PW || n > (int)F64W_MAX_N || lda < (a_layout ? (size_t)n : m) || ldq < (q_layout ? (size_t)n : m)) return -100;
	if (q == a && (a_layout != q_layout || ldq != lda)) return -100;
	f64w_apply_launch(0, q, ldq, a, lda, m, n, (int)cdiv((size_t)n, PW), zw, a_layout, q_layout);
	return f64_sync();
}
int tsqr_selftest_f64w_apply(double* q, size_t ldq, const double* a, size_t lda, size_t m, int n, const double* zw) {
	return tsqr_selftest_f64w_apply_lay(0, 0, q, ldq, a, lda, m, n, zw);
}

// rcopy_wide_f64_kernel: r (n x n, ldr) = R of the block store rw
int tsqr_selftest_f64w_rcopy(double* r, size_t ldr, const double* rw, int n) {
	if (n <= (int)PW || n > (int)F64W_MAX_N || ldr < (size_t)n) return -100;
	hipLaunchKernelGGL(tsqrmi::rcopy_wide_f64_kernel, dim3((unsigned)cdiv((size_t)n * n, 256)), dim3(256), 0, 0, r, ldr, rw, n);
	return f64_sync();
}

// rsave_wide_f64_kernel + rmul_wide_f64_kernel: r <- RW r through the block store rc (both bs doubles)
int tsqr_selftest_f64w_rmul(double* r, size_t ldr, const double* rw, double* rc, int n) {
	if (n <= (int)PW || n > (int)F64W_MAX_N || ldr < (size_t)n) return -100;
	const F64WPlan g = f64w_plan((size_t)n, (size_t)n);
	hipLaunchKernelGGL(tsqrmi::rsave_wide_f64_kernel, dim3((unsigned)cdiv(g.bs, 256)), dim3(256), 0, 0, rc, (const double*)r, ldr, n, g.npairs);
	HIPCHK(hipGetLastError());
	hipLaunchKernelGGL(tsqrmi::rmul_wide_f64_kernel, dim3((unsigned)g.npairs), dim3(1024), 0, 0, r, ldr, rw, (const double*)rc, n);
	return f64_sync();
}

// ---- tsqr_mi_orth_f64 (orth_f64.hip): each pass alone, on the product's plan (f64o_plan) and launchers -----------------------------------
// out[0..5]: NT, kblocks, nslices, cps, nch, doubles of the partials.  Host only.
int tsqr_selftest_f64_orth_plan(size_t m, size_t k, size_t n, long long* out) {
	if (!out || n == 0 || n > PW || k == 0 || k > F64O_MAX_K || m < k || m - k < n) return -100;
	const F64OPlan g = f64o_plan(m, k, n);
	out[0] = g.NT; out[1] = g.kblocks; out[2] = g.nslices; out[3] = (long long)g.cps; out[4] = (long long)g.nch;
	out[5] = (long long)g.nslices * g.kblocks * 64 * 16 * g.NT;
	return 0;
}

namespace {
inline bool f64o_bad(int v_layout, int x_layout, const void* v, size_t ldv, const void* x, size_t ldx, size_t m, int k, int n) {
	if ((v_layout != 0 && v_layout != 1) || (x_layout != 0 && x_layout != 1) || !v || !x) return true;
	if (n <= 0 || n > (int)PW || k <= 0 || k > (int)F64O_MAX_K || m < (size_t)k || m - (size_t)k < (size_t)n) return true;
	return ldv < (v_layout ? (size_t)k : m) || ldx < (x_layout ? (size_t)n : m);
}
}  // namespace

// orth_gram_f64_kernel + the reduction: sw[kblocks * 64 * NP + 1] = V^T X in the work layout (S[64 b + r][c] at b * 64 * NP + 64 c + r),
// the row count behind it; part: part_cap doubles for the partials
int tsqr_selftest_f64_orth_gram(int v_layout, int x_layout, double* sw, const double* v, size_t ldv, const double* x, size_t ldx, size_t m,
                                int k, int n, double* part, size_t part_cap) {
	if (!sw || !part || f64o_bad(v_layout, x_layout, v, ldv, x, ldx, m, k, n)) return -100;
	const F64OPlan g = f64o_plan(m, (size_t)k, (size_t)n);
	const size_t blk = (size_t)64 * 16 * g.NT;
	if ((size_t)g.nslices * g.kblocks * blk > part_cap) return -100;
	const tsqrmi::OrthGramArgs64 ga{v, ldv, x, ldx, m, k, n, g.kblocks, g.nslices, g.cps, g.nch, part};
	f64o_gram_launch(0, g, ga, v_layout, x_layout);
	HIPCHK(hipGetLastError());
	launch_reduce1(0, sw, part, g.nslices, (int)(g.kblocks * blk), (double)m);
	return f64_sync();
}

// orth_update_f64_kernel: x <- x - v S in place, S given in the work layout (sw: kblocks * 64 * NP doubles)
int tsqr_selftest_f64_orth_update(int v_layout, int x_layout, double* x, size_t ldx, const double* v, size_t ldv, const double* sw, size_t m,
                                  int k, int n) {
	if (!sw || f64o_bad(v_layout, x_layout, v, ldv, x, ldx, m, k, n)) return -100;
	const F64OPlan g = f64o_plan(m, (size_t)k, (size_t)n);
	const tsqrmi::OrthUpdateArgs64 ua{x, ldx, v, ldv, m, k, n, g.kblocks, sw};
	f64o_update_launch(0, g, ua, v_layout, x_layout);
	return f64_sync();
}

// orth_s_f64_kernel: s (k x n, lds) = Sw (second = 0) or s += Sw r1 (second = 1; r1 n x n upper triangular, ldr)
int tsqr_selftest_f64_orth_s(double* s, size_t lds, const double* sw, const double* r1, size_t ldr, int k, int n, int second) {
	if (!s || !sw || n <= 0 || n > (int)PW || k <= 0 || k > (int)F64O_MAX_K || lds < (size_t)k) return -100;
	if (second != 0 && second != 1) return -100;
	if (second && (!r1 || ldr < (size_t)n)) return -100;
	const tsqrmi::OrthSArgs64 sa{s, lds, sw, r1, ldr, k, n, (int)np_of((size_t)n), second};
	f64o_s_launch(0, sa);
	return f64_sync();
}

}  // extern "C"

// selftest_f32.hip -- one entry per pass of three kernel families of the fp32 engine, for tests/test_gpu_wide_passes.py: the one-panel
// path (64 < n <= 128: sweep_wide of tsqr_mi.hip, kernels of tsqr_wide.hip and the apply_wide instances of tsqr_kernels.hip), the panel
// coupling (n > 64: cross_kernel, its reductions and the update instance, as sweep launches them) and the native half-typed path
// (tsqr_mi_qr_f16: gram_h_kernel, apply_wg_h_kernel).  Included by selftest.hip.  Every
// entry launches the product's kernels with the product's launch arithmetic (f32_plan.h: the definitions libtsqr_mi.so is built from), the
// way sweep_wide does, waits, and returns 0, minus a HIP error, or -100 -- before any launch -- when a buffer of the caller is smaller than
// the plan needs or a shape is outside the kernel's domain.  A partition override is an argument of the entry (0: the product's); no entry
// reads or writes a process-wide setting.
// This library is built with -DTSQR_CHOL_STAMPS, which compiles time stamps into the Cholesky body that chol_wide_kernel shares with
// chol16_kernel (chol_body16): the arithmetic is the product's, the instruction stream around it is not.  tests/test_gpu_chol.py already
// runs chol_wide_kernel from this build (tsqr_selftest_wide_chain) and holds it bitwise against the product's own library; that stays.

namespace {
inline int f32_sync() {
	HIPCHK(hipGetLastError());
	HIPCHK(hipDeviceSynchronize());
	return 0;
}
inline bool wide_shape_ok(size_t m, int n) { return m > 0 && m <= ((size_t)1 << 30) && n > (int)PW && n <= 2 * (int)PW; }

// the apply instance of engine E on the plan's grid (wgs_over > 0: that many workgroups, as ApplyGrid::wgs)
template <int E> int selftest_w_apply(tsqrmi::ApplyArgs a, int wgs_over) {
	using W = WideApply<E>;
	int per_cu = 0;
	const int rc = apply_instance_setup<W::kernel(), typename W::G, false, W::CAP, W::QUERY>(&per_cu);
	if (rc) return rc;
	ApplyGrid grid;
	grid.wgs = wgs_over;
	apply_grid_fill<typename W::G>(a, grid, per_cu);
	if (a.nwaves < 1 || a.nwaves > 65535) return -100;
	hipLaunchKernelGGL(W::kernel(), dim3(a.nwaves, grid.gy), dim3(W::G::THREADS), W::G::lds_bytes(false), 0, a);
	return f32_sync();
}

// the plan of a 64-column Gram / coupling pass with the default wave count, or with nwaves_over waves asked for
inline GramPlan selftest_gram_plan(size_t m, size_t n, int nwaves_over) { return gram_plan_of(m, n, nwaves_over > 0 ? nwaves_over : GRAM_WAVES_DEFAULT); }

template <int E> int selftest_update(tsqrmi::ApplyArgs a, int wgs_over) {
	using U = UpdApply<E>;
	int per_cu = 0;
	const int rc = apply_instance_setup<U::kernel(), typename U::G, false, U::CAP, U::QUERY>(&per_cu);
	if (rc) return rc;
	ApplyGrid grid;
	grid.wgs = wgs_over; grid.gy = U::gy(a.multi_cols);
	apply_grid_fill<typename U::G>(a, grid, per_cu);
	if (a.nwaves < 1 || a.nwaves > 65535 || grid.gy > 65535) return -100;
	hipLaunchKernelGGL(U::kernel(), dim3(a.nwaves, grid.gy), dim3(U::G::THREADS), U::G::lds_bytes(false), 0, a);
	return f32_sync();
}
template <int E, int NT> int selftest_h_apply(tsqrmi::ApplyArgs a, int wgs_over) {
	using H = HalfApply<E, NT>;
	int per_cu = 0;
	const int rc = apply_instance_setup<H::kernel(), typename H::G, false, H::CAP, H::QUERY>(&per_cu);
	if (rc) return rc;
	ApplyGrid grid;
	grid.wgs = wgs_over;
	apply_grid_fill<typename H::G>(a, grid, per_cu);
	if (a.nwaves < 1 || a.nwaves > 65535) return -100;
	hipLaunchKernelGGL(H::kernel(), dim3(a.nwaves, grid.gy), dim3(H::G::THREADS), H::G::lds_bytes(false), 0, a);
	return f32_sync();
}
}  // namespace

extern "C" {

// out[0..9]: nfull, nrest, wgs_fast, wgs_rest (wide_gram_plan), doubles of the partials, doubles of the summed tiles + row count,
// WIDE_MAX_WGS, row blocks of the apply pass for engines 1 / 2 (128 rows) and engine 0 (64 rows), floats of the chol entry's scratch.
// Host only.
int tsqr_selftest_w_plan(size_t m, int n, size_t lda, long long* out) {
	if (!wide_shape_ok(m, n) || lda < m) return -100;
	const WideGramPlan p = wide_gram_plan(m, (size_t)n, lda);
	out[0] = (long long)p.nfull; out[1] = (long long)p.nrest; out[2] = p.wgs_fast; out[3] = p.wgs_rest;
	out[4] = (long long)(p.wgs_fast + p.wgs_rest) * WIDE_NELEM; out[5] = WIDE_NELEM + 1; out[6] = WIDE_MAX_WGS;
	out[7] = (long long)cdiv(m, (size_t)WideApply<1>::G::ROWS); out[8] = (long long)cdiv(m, (size_t)WideApply<0>::G::ROWS);
	out[9] = (long long)WIDE_CHOL_SCRATCH_FLOATS;
	return 0;
}

// gram_wide_kernel<true> on the full blocks, gram_wide_kernel<false> on the rest, then the reduction: gsum[36 * 256 + 1] (the row count
// behind the tiles).  wgs_over > 0 caps the workgroups of each launch; part holds part_cap doubles.
int tsqr_selftest_w_gram(double* gsum, const float* a, size_t lda, size_t m, int n, double* part, size_t part_cap, int wgs_over) {
	if (!wide_shape_ok(m, n) || lda < m || wgs_over < 0) return -100;
	WideGramPlan p = wide_gram_plan(m, (size_t)n, lda);
	if (wgs_over > 0) { p.wgs_fast = std::min(p.wgs_fast, wgs_over); p.wgs_rest = std::min(p.wgs_rest, wgs_over); }
	const int nparts = p.wgs_fast + p.wgs_rest;
	if (nparts < 1 || (size_t)nparts * WIDE_NELEM > part_cap) return -100;
	const int rca = wide_gram_attrs();
	if (rca) return rca;
	tsqrmi::GramWideArgs ga{};
	ga.a = a; ga.lda = lda; ga.m = m; ga.n = n; ga.blk0 = 0; ga.nblk = (int)p.nfull; ga.part = part;
	if (p.wgs_fast) hipLaunchKernelGGL((tsqrmi::gram_wide_kernel<true>), dim3(p.wgs_fast), dim3(512), tsqrmi::GW_LDS_BYTES, 0, ga);
	if (p.wgs_rest) {
		ga.blk0 = (int)p.nfull; ga.nblk = (int)p.nrest; ga.part += (size_t)p.wgs_fast * WIDE_NELEM;
		hipLaunchKernelGGL((tsqrmi::gram_wide_kernel<false>), dim3(p.wgs_rest), dim3(512), tsqrmi::GW_LDS_BYTES, 0, ga);
	}
	HIPCHK(hipGetLastError());
	launch_reduce1(0, gsum, part, nparts, WIDE_NELEM, (double)m);
	return f32_sync();
}

// chol_wide_kernel on summed tiles gsum[36 * 256], with the arguments chol_wide_args (tsqr_mi.hip) builds: rows = m, the default floor of
// the bound on S.  r (n x n, ldr), zw (128 x 128), status[3], host_words[3] (device memory standing in for the pinned words; may be
// null), prev_status (may be null); scratch: scratch_floats >= WIDE_CHOL_SCRATCH_FLOATS (Z11, Z22 in fp32 and the two blocks' verdict
// words; out[9] of the plan entry).
int tsqr_selftest_w_chol(float* r, size_t ldr, float* zw, unsigned* status, unsigned* host_words, const unsigned* prev_status,
                         const double* gsum, size_t m, int n, float* scratch, size_t scratch_floats) {
	if (!wide_shape_ok(m, n) || ldr < (size_t)n || scratch_floats < WIDE_CHOL_SCRATCH_FLOATS) return -100;
	unsigned* st12 = reinterpret_cast<unsigned*>(scratch + 8192);
	tsqrmi::CholWideArgs wa = chol_wide_wiring(gsum, r, ldr, m, (size_t)n, scratch, scratch + 4096, zw, st12, st12 + 16, (float)BF16_SCOND_FLOOR_DEFAULT);
	wa.status = status; wa.host_status = host_words; wa.prev_status = prev_status;
	hipLaunchKernelGGL(tsqrmi::chol_wide_kernel, dim3(1), dim3(1024), 0, 0, wa);
	return f32_sync();
}

// apply_wide_f32_kernel (engine 0) / apply_wide_kernel<1> / <2>: q = a Z, Z = zw (128 x 128, ld 128).  skip_status may be null.
int tsqr_selftest_w_apply(int engine, float* q, size_t ldq, const float* a, size_t lda, size_t m, int n, const float* zw,
                          const unsigned* skip_status, int wgs_over) {
	if (!wide_shape_ok(m, n) || lda < m || ldq < m || engine < 0 || engine > 2 || wgs_over < 0 || wgs_over > 65535) return -100;
	tsqrmi::ApplyArgs aa{};
	aa.a = a; aa.lda = lda; aa.q = q; aa.ldq = ldq; aa.m = m; aa.n = n; aa.z = zw; aa.skip_status = skip_status;
	return with_engine(engine, [&](auto e) { return selftest_w_apply<decltype(e)::value>(aa, wgs_over); });
}

// ---- panel coupling (n > 64) ------------------------------------------------------------------------------------------------------------
// out[0..6]: nch, cpw, nwaves, nblocks of gram_plan(m, 64) (nwaves_over > 0: with that many waves asked for), rows one workgroup sums in
// fp32 (4 waves x cpw chunks x 64 rows), CROSS_GSTRIDE, doubles of one workgroup's partial.  Host only.
int tsqr_selftest_cross_plan(size_t m, int nwaves_over, long long* out) {
	if (m == 0 || m > ((size_t)1 << 30) || nwaves_over < 0) return -100;
	const GramPlan g = selftest_gram_plan(m, PW, nwaves_over);
	out[0] = g.nch; out[1] = g.cpw; out[2] = g.nwaves; out[3] = g.nblocks; out[4] = 4LL * g.cpw * 64; out[5] = tsqrmi::CROSS_GSTRIDE;
	out[6] = (long long)CROSS_PART_DOUBLES;
	return 0;
}

// S_j = X^T Y_j for the ntr = ceil(ny_total / 64) trailing panels of Y (m x ny_total), as sweep does it: cross_kernel on grid (nblocks, gy)
// over groups of as many panels as part (part_cap doubles) holds workgroup partials for, then cross_reduce_multi_kernel.  fused = 1:
// the reduction writes the block row of R (r_blk: 64 x ny_total, ldr) and zneg (ntr x 4096 floats: -S_j) itself; fused = 0: sums only
// (gm: ntr x CROSS_GSTRIDE doubles), then cross_finish_kernel writes R and zneg.  nwaves_over > 0: the waves asked for.
int tsqr_selftest_cross(float* r_blk, size_t ldr, float* zneg, double* gm, const float* x, size_t ldx, const float* y, size_t ldy, size_t m,
                        int ny_total, double* part, size_t part_cap, int fused, int nwaves_over) {
	if (m == 0 || m > ((size_t)1 << 30) || ny_total <= 0 || ny_total > 65535 * 64 || ldx < m || ldy < m || ldr < PW || nwaves_over < 0) return -100;
	const GramPlan g = selftest_gram_plan(m, PW, nwaves_over);
	const size_t slots = part_cap / CROSS_PART_DOUBLES;
	if (g.nblocks < 1 || slots < (size_t)g.nblocks) return -100;
	const size_t ntc = (size_t)ny_total, ntr = cdiv(ntc, PW);
	const size_t grp = cross_group(slots, g.nblocks);
	for (size_t j0 = 0; j0 < ntr; j0 += grp) {
		const unsigned gy = (unsigned)std::min(grp, ntr - j0);
		cross_group_launch(0, g, x, ldx, y, ldy, m, ntc, j0, gy, part, gm, fused != 0, r_blk, ldr, zneg);
		HIPCHK(hipGetLastError());
	}
	if (!fused) cross_finish_launch(0, r_blk, ldr, zneg, gm, ntc);
	return f32_sync();
}

// the update instance as sweep launches it: Y_j <- Y_j + X zneg_j for every 64-column panel j of Y (m x ny_total, ldy); X: m x 64;
// zneg: ceil(ny_total / 64) x 4096 floats.  wgs_over > 0: the workgroups of the whole grid (split over the panels).
int tsqr_selftest_update(int engine, float* y, size_t ldy, const float* x, size_t ldx, size_t m, const float* zneg, int ny_total, int wgs_over) {
	if (m == 0 || m > ((size_t)1 << 30) || ny_total <= 0 || ny_total > 65535 * 64 || ldx < m || ldy < m || engine < 0 || engine > 2 || wgs_over < 0) return -100;
	tsqrmi::ApplyArgs ua{};
	ua.a = x; ua.lda = ldx; ua.q = y; ua.ldq = ldy; ua.m = m; ua.n = (int)PW; ua.z = zneg;
	ua.n_out = (int)std::min(PW, (size_t)ny_total); ua.multi_cols = ny_total;
	return with_engine(engine, [&](auto e) { return selftest_update<decltype(e)::value>(ua, wgs_over); });
}

// ---- native half-typed path (16 < n <= 64) ------------------------------------------------------------------------------------------------
// gram_h_kernel<NT> + the reduction: gsum[ntri * 256 + 1].  a16: halves, lda % 8 == 0, 16-byte aligned (what tsqr_mi_qr_f16 sends it).
int tsqr_selftest_h_gram(double* gsum, const void* a16, size_t lda, size_t m, int n, double* part, size_t part_cap, int nwaves_over) {
	if (m == 0 || m > ((size_t)1 << 30) || n <= 16 || n > (int)PW || lda < m || lda % 8 != 0 || (reinterpret_cast<uintptr_t>(a16) & 15) != 0 || nwaves_over < 0) return -100;
	const GramPlan g = selftest_gram_plan(m, (size_t)n, nwaves_over);
	if (g.nblocks < 1 || (size_t)g.nblocks * g.ntri * 256 > part_cap) return -100;
	tsqrmi::GramArgs a{};
	a.a = reinterpret_cast<const float*>(a16); a.lda = lda; a.m = m; a.n = n; a.nchunks = g.nch; a.cpw = g.cpw; a.nwaves = g.nwaves; a.part = part;
	with_nt((int)(np_of((size_t)n) / 16), [&](auto nt) { hipLaunchKernelGGL(tsqrmi::gram_h_kernel<decltype(nt)::value>, dim3(g.nblocks), dim3(256), 0, 0, a); });
	HIPCHK(hipGetLastError());
	launch_reduce1(0, gsum, part, g.nblocks, g.ntri * 256, (double)m);
	return f32_sync();
}

// apply_wg_h_kernel<E, NT, ROWS>, engines 1 and 2: q16 = a16 Z (halves at both ends; z: NP x NP floats, ld NP); r32 (n x n, ld n) non-null:
// workgroup 0 also writes r16 (n x n halves, ldr16).  lda, ldq % 4 == 0, bases 8-byte aligned (what tsqr_mi_qr_f16 sends it).
int tsqr_selftest_h_apply(int engine, void* q16, size_t ldq, const void* a16, size_t lda, size_t m, int n, const float* z, const float* r32,
                          void* r16, size_t ldr16, int wgs_over) {
	if (m == 0 || m > ((size_t)1 << 30) || n <= 16 || n > (int)PW || lda < m || ldq < m || lda % 4 != 0 || ldq % 4 != 0 || engine < 1 || engine > 2 ||
	    ((reinterpret_cast<uintptr_t>(a16) | reinterpret_cast<uintptr_t>(q16)) & 7) != 0 || wgs_over < 0 || (r16 && (!r32 || ldr16 < (size_t)n))) return -100;
	tsqrmi::ApplyArgs aa{};
	aa.a = reinterpret_cast<const float*>(a16); aa.lda = lda; aa.q = reinterpret_cast<float*>(q16); aa.ldq = ldq; aa.m = m; aa.n = n; aa.z = z;
	aa.r32 = r32; aa.r16 = r16; aa.ldr16 = ldr16;
	return with_nt((int)(np_of((size_t)n) / 16), [&](auto nt) {
		constexpr int NT = decltype(nt)::value;
		return engine == 1 ? selftest_h_apply<1, NT>(aa, wgs_over) : selftest_h_apply<2, NT>(aa, wgs_over);
	});
}

}  // extern "C"

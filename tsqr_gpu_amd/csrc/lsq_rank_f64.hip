// lsq_rank_f64.hip -- the device passes of the rank-aware fp64 least-squares entry (tsqr_mi_lstsq_rank_f64: n <= 64, nrhs <= 16;
// include/tsqr_mi.h has the method, DESIGN.md section 9 the figures) and their launchers.  Included by tsqr_mi.hip and selftest.hip behind
// tsqr_f64.hip and f64_plan.h:
//   lsq_rank_f64_kernel      : the rank from the diagonal of a pivoted R and Zeff = P1 inverse(R11), the inverse factor of the retained
//                              columns, on one workgroup
//   gramq_dense_f64_kernel   : gramq_f64_kernel for a dense Z staged in LDS: per-workgroup partials of (A Zeff)^T (A Zeff)
//   lsq_rank_step_f64_kernel : the CholeskyQR step on the retained columns, G1 = Rc^T Rc and Zeff <- Zeff inverse(Rc), on one workgroup
//   lsq_dense_f64_kernel     : lsq_f64_kernel for a dense Z staged in LDS
//   lsq_zg_f64_kernel        : (tsqr_mi_lstsq_minnorm_f64) unit vectors into the dropped columns of Zeff, so that the Gram pass also gives G12
//   lsq_minnorm_f64_kernel   : (tsqr_mi_lstsq_minnorm_f64) the update factor Zmn = P pinv(Q1^T A P) of the minimum-norm form, on one workgroup
// The last pass, X <- X + Z D for a dense Z, is lsq_update_f64_kernel<true> (tsqr_f64.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace tsqrmi {

// The dense-Z form of lsq_f64_kernel (the rank-aware solve): Z is a dense NP x NP matrix (ld NP, zero padded: lsq_rank_f64_kernel's
// row-permuted triangle), so every output tile of stage 1 sums all 4 NT k-blocks, in the order 0 .. 4 NT - 1.  The 4 NT^2 operands
// would take 128 VGPRs at NT = 4 next to av, nx, xop and the accumulators, so they are staged in LDS once per workgroup in operand
// order, applyd_f64_kernel's scheme: operand (jt, kb) is 64 consecutive doubles, lane l reads element l, one conflict-free 8-byte read
// per MFMA.  Everything else -- the tile loop, the loads and the prefetch, stages 2 and 3, the partials -- is lsq_f64_kernel's, line
// for line.  It is a kernel of its own and not a flag of lsq_f64_kernel because that kernel's device code must not move: with the
// dense form behind a template flag, eight of its sixteen instantiations came out of the compiler with another closing workgroup sum
// (DESIGN.md section 9).  The copy of the tile loop has to be kept in step with lsq_f64_kernel by hand.  On an upper triangular Z the k-blocks the triangular form skips add products with exact zeros, so both
// kernels give the same D whenever no product of A with a skipped zero is non-finite.
template <int NT, bool AROW, bool BROW>
__global__ __launch_bounds__(256) void lsq_dense_f64_kernel(const LsqArgs64 a) {
	constexpr int NP = 16 * NT, KB = 4 * NT;
	__shared__ double red[2 * NT * 256];
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, lq = lane >> 4;
	const int gw = blockIdx.x * 4 + wv;
	__shared__ double zl[NT * KB * 64];
	for (int e = threadIdx.x; e < NT * KB * 64; e += 256) {
		const int l = e & 63, b = e >> 6, jt = b / KB, kb = b % KB;
		zl[e] = a.z[(size_t)(16 * jt + (l & 15)) * NP + 4 * kb + (l >> 4)];
	}
	__syncthreads();                                       // (every wave of the workgroup, idle ones included)
	f64x4 acc[NT];
#pragma unroll
	for (int t = 0; t < NT; t++) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
	if (gw < a.nwaves) {
		double xop[KB], idop[4];
#pragma unroll
		for (int kb = 0; kb < KB; kb++) {
			const int row = 4 * kb + lq;
			xop[kb] = -((a.x && row < a.n && li < a.nrhs) ? a.x[(size_t)li * NP + row] : 0.0);
		}
#pragma unroll
		for (int kb = 0; kb < 4; kb++) idop[kb] = (4 * kb + lq == li) ? 1.0 : 0.0;
		// a tile beyond the last reads nothing and leaves zeros (gramq_f64_kernel's load_tile, and the same for the tile of B)
		auto load_tile = [&](double (&av)[KB], double (&bv)[4], int tile) {
			const size_t row = (size_t)tile * 16 + li;
			const bool live = tile < a.ntiles && row < a.m;
			if constexpr (AROW) load_rows_rm<KB>(av, a.a, a.lda, row, live, a.n, lq);
			else {
#pragma unroll
				for (int kb = 0; kb < KB; kb++) {
					const int col = 4 * kb + lq;
					av[kb] = (live && col < a.n) ? a.a[(size_t)col * a.lda + row] : 0.0;
				}
			}
			if constexpr (BROW) load_rows_rm<4>(bv, a.b, a.ldb, row, live, a.nrhs, lq);
			else {
#pragma unroll
				for (int kb = 0; kb < 4; kb++) {
					const int col = 4 * kb + lq;
					bv[kb] = (live && col < a.nrhs) ? a.b[(size_t)col * a.ldb + row] : 0.0;
				}
			}
		};
		double av[KB], nx[KB], bv[4], nb[4];
		load_tile(av, bv, gw);
		for (int tile = gw; tile < a.ntiles; tile += a.nwaves) {
			load_tile(nx, nb, tile + a.nwaves);
			f64x4 qt[NT];
#pragma unroll
			for (int jt = 0; jt < NT; jt++) {
				qt[jt] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
				for (int kb = 0; kb < KB; kb++)
					qt[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[kb], zl[(jt * KB + kb) * 64 + lane], qt[jt], 0, 0, 0);
			}
			f64x4 rt = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
			for (int kb = 0; kb < 4; kb++) rt = __builtin_amdgcn_mfma_f64_16x16x4f64(bv[kb], idop[kb], rt, 0, 0, 0);
#pragma unroll
			for (int kb = 0; kb < KB; kb++) rt = __builtin_amdgcn_mfma_f64_16x16x4f64(av[kb], xop[kb], rt, 0, 0, 0);
#pragma unroll
			for (int reg = 0; reg < 4; reg++)
#pragma unroll
				for (int ti = 0; ti < NT; ti++)
					acc[ti] = __builtin_amdgcn_mfma_f64_16x16x4f64(qt[ti][reg], rt[reg], acc[ti], 0, 0, 0);
#pragma unroll
			for (int kb = 0; kb < KB; kb++) av[kb] = nx[kb];
#pragma unroll
			for (int kb = 0; kb < 4; kb++) bv[kb] = nb[kb];
		}
	}
	wg_sum4_store(acc, red, a.part + (size_t)blockIdx.x * NT * 256, wv, lane);
}

// The dense-Z form of gramq_f64_kernel (the CholeskyQR step of the rank-aware solve): what lsq_dense_f64_kernel is to lsq_f64_kernel.
// Z is a dense NP x NP matrix (ld NP, zero padded), so every output tile of stage 1 sums all 4 NT k-blocks, in the order
// 0 .. 4 NT - 1, and the 4 NT^2 operands are staged in LDS once per workgroup in operand order: operand (jt, kb) is 64 consecutive
// doubles, lane l reads element l.  The tile loop, the prefetch, load_rows_rm, the Gram MFMAs and the partials (wg_sum4_store, NTRI
// tiles) are gramq_f64_kernel's, line for line; a kernel of its own for the reason given above, and kept in step by hand.  On an upper
// triangular Z it gives gramq_f64_kernel's bits whenever no product of A with a skipped zero is non-finite.
template <int NT, bool AROW>
__global__ __launch_bounds__(256) void gramq_dense_f64_kernel(const GramQArgs64 a) {
	constexpr int NP = 16 * NT, KB = 4 * NT, NTRI = (NT * (NT + 1)) / 2;
	__shared__ double red[2 * NTRI * 256];
	__shared__ double zl[NT * KB * 64];
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, lq = lane >> 4;
	const int gw = blockIdx.x * 4 + wv;
	for (int e = threadIdx.x; e < NT * KB * 64; e += 256) {
		const int l = e & 63, b = e >> 6, jt = b / KB, kb = b % KB;
		zl[e] = a.z[(size_t)(16 * jt + (l & 15)) * NP + 4 * kb + (l >> 4)];
	}
	__syncthreads();                                       // (every wave of the workgroup, idle ones included)
	f64x4 acc[NTRI];
#pragma unroll
	for (int t = 0; t < NTRI; t++) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
	if (gw < a.nwaves) {
		// a tile beyond the last reads nothing and leaves zeros (gramq_f64_kernel's load_tile)
		auto load_tile = [&](double (&av)[KB], int tile) {
			const size_t row = (size_t)tile * 16 + li;
			const bool live = tile < a.ntiles && row < a.m;
			if constexpr (AROW) load_rows_rm<KB>(av, a.a, a.lda, row, live, a.n, lq);
			else {
#pragma unroll
				for (int kb = 0; kb < KB; kb++) {
					const int col = 4 * kb + lq;
					av[kb] = (live && col < a.n) ? a.a[(size_t)col * a.lda + row] : 0.0;
				}
			}
		};
		double av[KB], nx[KB];
		load_tile(av, gw);
		for (int tile = gw; tile < a.ntiles; tile += a.nwaves) {
			load_tile(nx, tile + a.nwaves);
			f64x4 qt[NT];
#pragma unroll
			for (int jt = 0; jt < NT; jt++) {
				qt[jt] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
				for (int kb = 0; kb < KB; kb++)
					qt[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[kb], zl[(jt * KB + kb) * 64 + lane], qt[jt], 0, 0, 0);
			}
#pragma unroll
			for (int reg = 0; reg < 4; reg++) {
				int idx = 0;
#pragma unroll
				for (int ti = 0; ti < NT; ti++)
#pragma unroll
					for (int tj = ti; tj < NT; tj++) {
						acc[idx] = __builtin_amdgcn_mfma_f64_16x16x4f64(qt[ti][reg], qt[tj][reg], acc[idx], 0, 0, 0);
						idx++;
					}
			}
#pragma unroll
			for (int kb = 0; kb < KB; kb++) av[kb] = nx[kb];
		}
	}
	wg_sum4_store(acc, red, a.part + (size_t)blockIdx.x * NTRI * 256, wv, lane);
}

// ---- the rank-aware least-squares solve: rank and inverse factor of the retained columns from R and jpvt ----------------------------------
struct LsqRankArgs64 {
	const double* r; size_t ldr;         // n x n upper triangular (only i <= j is read): qrcp_r_f64_kernel's R, diag(R) >= 0 and non-increasing
	const int* jpvt;                     // its n pivots, 0-based
	double rcond;                        // column j is retained when R_jj > rcond R_00
	double* zeff;                        // NP x NP (ld NP) out, wholly written: Zeff[jpvt[i]][j] = inverse(R11)[i][j] for i <= j < k, zero elsewhere
	unsigned* status;                    // device word [0] the rank k; null: not wanted
	unsigned* host_status;               // device-visible alias of a pinned host word receiving k; null: not wanted
	int n;
};

// One workgroup, R held in LDS (column-major, ld 64).  The rank k is the number of j with R_jj > rcond R_00, counted by every wave for
// itself from the same 64 numbers (a NaN on the diagonal is not counted; R_00 == 0 gives k = 0 and Zeff = 0).  R11 = R[:k, :k] is then
// inverted by column-oriented back substitution, wave w taking columns j = w, w + 16, ... < k and lane i holding row i of the column:
// from e_j, step l = j .. 0 forms z_l = w_l / R_ll and lanes i < l take w_i <- fma(-R_il, z_l, w_i).  Entry (i, j) is so the terms
// l = j .. i + 1 in that order, one fused multiply-add each, and one division: a fixed function of R, the same bits on every run.
// cond(R11) is about 1 / rcond at most, whatever cond(A) is.  The rows go out permuted: row i of the inverse is row jpvt[i] of Zeff (a
// pivot outside 0 .. n - 1 writes nothing), through an LDS image so that the whole NP x NP block is written once, zeros included.
// A Zeff = Q1, the orthonormal factor of the retained columns A P1.  jpvt must be a permutation of 0 .. n - 1, as qrcp_r_f64_kernel
// writes it: with a repeated pivot two lanes write the same word of the LDS image and that row of Zeff is either of the two (nothing
// outside the image is touched).  No scratch; 64.3 KB of static LDS, like qrcp_r_f64_kernel's 66.4 KB above the 64 KB of older
// targets: this file is built for gfx950 alone, whose workgroups have 160 KB.
__global__ __launch_bounds__(1024) void lsq_rank_f64_kernel(const LsqRankArgs64 a) {
	__shared__ double M[64 * 64], Zl[64 * 64];
	__shared__ int piv[64];
	static_assert(sizeof(M) + sizeof(Zl) + sizeof(piv) <= 160 * 1024, "lsq_rank_f64_kernel relies on the 160 KB of LDS of gfx950");
	const int t = threadIdx.x, lane = t & 63, wv = t >> 6, n = a.n;
	const int NP = 16 * ((n + 15) / 16);
#pragma unroll
	for (int u = 0; u < 4; u++) {
		const int e = t + 1024 * u, i = e & 63, j = e >> 6;
		M[e] = (i <= j && j < n) ? a.r[(size_t)j * a.ldr + i] : 0.0;
		Zl[e] = 0.0;
	}
	if (t < 64) piv[t] = t < n ? a.jpvt[t] : -1;
	__syncthreads();
	const double dii = M[lane * 64 + lane], d00 = M[0];
	const bool keep = lane < n && dii > a.rcond * d00;
	const int k = __popcll(__ballot(keep));
	for (int j = wv; j < k; j += 16) {
		double w = lane == j ? 1.0 : 0.0, z = 0.0;
		for (int l = j; l >= 0; l--) {
			const double q = w / dii;
			const double zl = __shfl(q, l, 64);
			if (lane == l) z = zl;
			if (lane < l) w = __builtin_fma(-M[l * 64 + lane], zl, w);
		}
		const int row = piv[lane];
		if (lane <= j && row >= 0 && row < n) Zl[j * 64 + row] = z;
	}
	__syncthreads();
#pragma unroll
	for (int u = 0; u < 4; u++) {
		const int e = t + 1024 * u, i = e & 63, j = e >> 6;
		if (i < NP && j < NP) a.zeff[(size_t)j * NP + i] = Zl[e];
	}
	if (t == 0) {
		if (a.status) a.status[0] = (unsigned)k;
		if (a.host_status) { volatile unsigned* hs = a.host_status; hs[0] = (unsigned)k; }
	}
}

// ---- the CholeskyQR step on the retained columns -----------------------------------------------------------------------------------------
struct LsqRankStepArgs64 {
	const double* gsum;                  // the summed tiles of gramq_dense_f64_kernel on Zeff: G1 = (A Zeff)^T (A Zeff), NTRI tiles of 256
	const unsigned* rank;                // the device word lsq_rank_f64_kernel wrote: k (taken as min(k, n))
	double* zeff;                        // NP x NP (ld NP), in and out: Zeff <- Zeff inverse(Rc), wholly written
	unsigned* status;                    // device word [0] the verdict: 0 ok, 1 a pivot of the Cholesky factorisation not positive or not finite
	unsigned* host_status;               // device-visible alias of a pinned host word receiving the verdict; null: not wanted
	int n;
};

// One workgroup, everything in LDS (column-major, ld 64).  Only G1[:k, :k] is read, from the tiles on and above the diagonal (entry
// (i, j), i <= j, of tile pair (i >> 4, j >> 4): wg_sum4_store's layout).  G1 = I + a perturbation of a few 1e-2 at most, so the
// factorisation G1[:k, :k] = Rc^T Rc is plain right-looking Cholesky on the upper triangle: no shift, no acceptance ladder.  Step p:
// every thread reads the pivot g = M_pp; not positive or not finite (a NaN fails g > 0) ends the loop for all threads at once, verdict 1;
// else row p is divided by sqrt(g) -- one barrier -- and entry (i, j), p < i <= j < k, takes one fused multiply-add, M_ij <-
// fma(-Rc_pi, Rc_pj, M_ij) -- one barrier.  Entry (i, j) of Rc is so a fixed chain of i fused multiply-adds, a square root and a
// division.  inverse(Rc) then comes from lsq_rank_f64_kernel's back substitution (wave per column, lane per row, terms l = j .. i + 1
// in that order), and Zeff <- Zeff inverse(Rc): entry (i, j), j < k, sums l = 0 .. j in that order, one fused multiply-add each; the
// columns j >= k are written as zeros.  A zero row of Zeff (the rows jpvt[k:] and the padding) sums products of exact zeros with
// finite numbers and stays an exact zero, and so does an entry (jpvt[i], j) with j < i: the zero structure of lsq_rank_f64_kernel's Zeff
// is kept.  Every number is a fixed function of the input: the same bits on every run.  k = 0 writes Zeff = 0 and verdict 0; verdict 1
// writes Zeff = 0 too (the passes behind it then leave X = 0, and the entry reports state 3).  No scratch; 96.5 KB of static LDS:
// this file is built for gfx950 alone, whose workgroups have 160 KB.
__global__ __launch_bounds__(1024) void lsq_rank_step_f64_kernel(const LsqRankStepArgs64 a) {
	__shared__ double M[64 * 64], Zi[64 * 64], Ze[64 * 64];
	static_assert(sizeof(M) + sizeof(Zi) + sizeof(Ze) <= 160 * 1024, "lsq_rank_step_f64_kernel relies on the 160 KB of LDS of gfx950");
	const int t = threadIdx.x, lane = t & 63, wv = t >> 6, n = a.n;
	const int NT = (n + 15) / 16, NP = 16 * NT;
	const int k = min((int)a.rank[0], n);                  // (uniform: every thread reads the same word)
#pragma unroll
	for (int u = 0; u < 4; u++) {
		const int e = t + 1024 * u, i = e & 63, j = e >> 6;
		double g = 0.0;
		if (i <= j && j < k) {
			const int ti = i >> 4, tj = j >> 4, ri = i & 15;
			const int idx = ti * NT - (ti * (ti - 1)) / 2 + (tj - ti);
			g = a.gsum[(size_t)idx * 256 + (ri >> 2) * 64 + (ri & 3) * 16 + (j & 15)];
		}
		M[e] = g;
		Zi[e] = 0.0;
		Ze[e] = (i < NP && j < NP) ? a.zeff[(size_t)j * NP + i] : 0.0;
	}
	__syncthreads();
	bool bad = false;
	for (int p = 0; p < k; p++) {
		const double g = M[p * 64 + p];
		if (!(g > 0.0) || !(g < __builtin_inf())) { bad = true; break; }     // (uniform: the same LDS word for every thread)
		const double rpp = sqrt(g);
		__syncthreads();                                  // every thread has read the pivot
		if (t < 64 && t >= p && t < k) M[t * 64 + p] = t == p ? rpp : M[t * 64 + p] / rpp;
		__syncthreads();
#pragma unroll
		for (int u = 0; u < 4; u++) {
			const int e = t + 1024 * u, i = e & 63, j = e >> 6;
			if (i > p && i <= j && j < k) M[e] = __builtin_fma(-M[i * 64 + p], M[j * 64 + p], M[e]);
		}
		__syncthreads();
	}
	if (!bad) {
		const double dii = lane < k ? M[lane * 64 + lane] : 1.0;
		for (int j = wv; j < k; j += 16) {
			double w = lane == j ? 1.0 : 0.0, z = 0.0;
			for (int l = j; l >= 0; l--) {
				const double q = w / dii;
				const double zl = __shfl(q, l, 64);
				if (lane == l) z = zl;
				if (lane < l) w = __builtin_fma(-M[l * 64 + lane], zl, w);
			}
			if (lane <= j) Zi[j * 64 + lane] = z;
		}
	}
	__syncthreads();
#pragma unroll
	for (int u = 0; u < 4; u++) {
		const int e = t + 1024 * u, i = e & 63, j = e >> 6;
		if (i < NP && j < NP) {
			double s = 0.0;
			if (!bad && j < k)
				for (int l = 0; l <= j; l++) s = __builtin_fma(Ze[l * 64 + i], Zi[j * 64 + l], s);
			a.zeff[(size_t)j * NP + i] = s;
		}
	}
	if (t == 0) {
		a.status[0] = bad ? 1u : 0u;
		if (a.host_status) { volatile unsigned* hs = a.host_status; hs[0] = bad ? 1u : 0u; }
	}
}

// ---- the minimum-norm form (tsqr_mi_lstsq_minnorm_f64): Zg, and the update factor Zmn = P pinv(S) -----------------------------------------
struct LsqZgArgs64 {
	const int* jpvt;                     // the n pivots, 0-based
	const unsigned* rank;                // the device word lsq_rank_f64_kernel wrote: k (taken as min(k, n))
	double* zeff;                        // NP x NP (ld NP), in and out: column j, k <= j < n, of lsq_rank_f64_kernel's Zeff is zero; entry (jpvt[j], j) <- 1
	int n;
};

// Zeff -> Zg in place: column j = k .. n - 1 becomes the unit vector e_jpvt[j], one thread per column, one store each (a pivot outside
// 0 .. n - 1 stores nothing); nothing else is touched.  The dense Gram pass on Zg then holds G12 = (A Zeff)^T A P2 in the columns
// k .. n - 1 of the rows 0 .. k - 1 next to G11 = (A Zeff)^T (A Zeff), whose entries keep their bits: an MFMA output entry depends on its
// own two columns of A Z alone.  lsq_rank_step_f64_kernel reads the columns below k of Zeff only and writes the others as zeros.
__global__ __launch_bounds__(64) void lsq_zg_f64_kernel(const LsqZgArgs64 a) {
	const int j = threadIdx.x, n = a.n;
	const int NP = 16 * ((n + 15) / 16);
	const int k = min((int)a.rank[0], n);
	if (j < k || j >= n) return;
	const int row = a.jpvt[j];
	if (row >= 0 && row < n) a.zeff[(size_t)j * NP + row] = 1.0;
}

struct LsqMinnormArgs64 {
	const double* gsum;                  // the summed tiles of gramq_dense_f64_kernel on Zg: G11 in [:k, :k], G12 in [:k, k:n], NTRI tiles of 256
	const unsigned* rank;                // the device word lsq_rank_f64_kernel wrote: k (taken as min(k, n))
	const int* jpvt;                     // the n pivots, 0-based
	const double* zeff;                  // NP x NP (ld NP): Zeff behind lsq_rank_step_f64_kernel on the same G11, A Zeff = Q1
	double* zmn;                         // NP x NP (ld NP) out, wholly written: Zmn = P pinv(S), S = Q1^T A P = R11' [I M]; columns >= k zero
	unsigned* status;                    // device word [0] the verdict: 0 ok, 1 a pivot of G11 (the step's verdict), 2 a pivot of C not positive or not finite
	unsigned* host_status;               // device-visible alias of a pinned host word receiving the verdict; null: not wanted
	int n;
};

// One workgroup, four 64 x 64 blocks in LDS (column-major, ld 64), each used twice.  With R11' = inverse(P1^T Zeff) (k x k, upper
// triangular; never formed) the retained columns are A P1 = Q1 R11', and S = Q1^T A P = R11' [I M].
//   W0 <- [Rc | S12]: lsq_rank_step_f64_kernel's right-looking Cholesky of G11 = Rc^T Rc, operation for operation (the same bits), with
//         the columns k .. n - 1 of G12 carried along as further columns of the rows 0 .. k - 1: row p divided by Rc_pp, entry (i, j),
//         p < i < k <= j < n, one fused multiply-add.  That is the forward substitution S12 = Rc^-T G12 = Q1^T A P2.
//   W1 <- T = P1^T Zeff = inverse(R11'), read from zeff (rows jpvt[:k], upper triangle)
//   W2 <- M = T S12 (k x (n - k), kept in the columns k .. n - 1): entry (i, j) sums l = i .. k - 1 in that order
//   W3 <- C = I + M M^T, upper triangle: entry (i, j) starts from 1 or 0 and sums the columns k .. n - 1 in that order; then C = Uc^T Uc by
//         the same Cholesky.  C is SPD with cond(C) <= 1 + ||M||^2: no shift.  A bad pivot: verdict 2.
//   W0 <- Ui = inverse(Uc): lsq_rank_f64_kernel's back substitution
//   W3 <- Y = Ui^T T: entry (i, j) sums l = 0 .. i;   W1 <- V = Ui Y = inverse(C) T: entry (i, j) sums l = i .. k - 1
//   W0 <- the image of Zmn: row jpvt[i], i < k, is row i of V; row jpvt[i], k <= i < n, is row i - k of M^T V, entry (i, j) summing
//         l = 0 .. k - 1; the columns >= k, the padding and every row no pivot names stay zero.  (A pivot outside 0 .. n - 1 is skipped.)
// Every sum is a fixed chain of one fused multiply-add per term from +0 (or 1): the same bits on every run.  At k = n there is no M:
// C = I exactly, Uc = Ui = I exactly, Y = V = T exactly (products with exact ones, sums of exact zeros), and Zmn is BITWISE the Zeff that
// came in.  k = 0 writes Zmn = 0 and verdict 0; verdicts 1 and 2 write Zmn = 0.  No scratch; 128.3 KB of static LDS: this file is built
// for gfx950 alone, whose workgroups have 160 KB.
__global__ __launch_bounds__(1024) void lsq_minnorm_f64_kernel(const LsqMinnormArgs64 a) {
	__shared__ double W0[64 * 64], W1[64 * 64], W2[64 * 64], W3[64 * 64];
	__shared__ int piv[64];
	static_assert(sizeof(W0) + sizeof(W1) + sizeof(W2) + sizeof(W3) + sizeof(piv) <= 160 * 1024,
	              "lsq_minnorm_f64_kernel relies on the 160 KB of LDS of gfx950");
	const int t = threadIdx.x, lane = t & 63, wv = t >> 6, n = a.n;
	const int NT = (n + 15) / 16, NP = 16 * NT;
	const int k = min((int)a.rank[0], n);                  // (uniform: every thread reads the same word)
	if (t < 64) {
		const int row = t < n ? a.jpvt[t] : -1;
		piv[t] = (row >= 0 && row < n) ? row : -1;
	}
	__syncthreads();
#pragma unroll
	for (int u = 0; u < 4; u++) {
		const int e = t + 1024 * u, i = e & 63, j = e >> 6;
		double g = 0.0, z = 0.0;
		if (i <= j && i < k && j < n) {
			const int ti = i >> 4, tj = j >> 4, ri = i & 15;
			const int idx = ti * NT - (ti * (ti - 1)) / 2 + (tj - ti);
			g = a.gsum[(size_t)idx * 256 + (ri >> 2) * 64 + (ri & 3) * 16 + (j & 15)];
		}
		if (i <= j && j < k && piv[i] >= 0) z = a.zeff[(size_t)j * NP + piv[i]];
		W0[e] = g;
		W1[e] = z;
	}
	__syncthreads();
	// the Cholesky factorisation of the leading k x k block of W (upper triangle), the columns k .. nc - 1 of its rows carried along
	auto chol = [&](double* W, int nc) -> bool {
		for (int p = 0; p < k; p++) {
			const double g = W[p * 64 + p];
			if (!(g > 0.0) || !(g < __builtin_inf())) return true;            // (uniform: the same LDS word for every thread)
			const double rpp = sqrt(g);
			__syncthreads();                                  // every thread has read the pivot
			if (t < 64 && t >= p && t < nc) W[t * 64 + p] = t == p ? rpp : W[t * 64 + p] / rpp;
			__syncthreads();
#pragma unroll
			for (int u = 0; u < 4; u++) {
				const int e = t + 1024 * u, i = e & 63, j = e >> 6;
				if (i > p && i <= j && i < k && j < nc) W[e] = __builtin_fma(-W[i * 64 + p], W[j * 64 + p], W[e]);
			}
			__syncthreads();
		}
		return false;
	};
	unsigned verdict = chol(W0, n) ? 1u : 0u;
	if (verdict == 0u) {
		// M = T S12
#pragma unroll
		for (int u = 0; u < 4; u++) {
			const int e = t + 1024 * u, i = e & 63, j = e >> 6;
			double s = 0.0;
			if (i < k && j >= k && j < n)
				for (int l = i; l < k; l++) s = __builtin_fma(W1[l * 64 + i], W0[j * 64 + l], s);
			W2[e] = s;
		}
		__syncthreads();
		// C = I + M M^T; W0 is free: cleared for Ui
#pragma unroll
		for (int u = 0; u < 4; u++) {
			const int e = t + 1024 * u, i = e & 63, j = e >> 6;
			double s = 0.0;
			if (i <= j && j < k) {
				s = i == j ? 1.0 : 0.0;
				for (int c = k; c < n; c++) s = __builtin_fma(W2[c * 64 + i], W2[c * 64 + j], s);
			}
			W3[e] = s;
			W0[e] = 0.0;
		}
		__syncthreads();
		if (chol(W3, k)) verdict = 2u;
	}
	if (verdict == 0u) {
		// Ui = inverse(Uc)
		const double dii = lane < k ? W3[lane * 64 + lane] : 1.0;
		for (int j = wv; j < k; j += 16) {
			double w = lane == j ? 1.0 : 0.0, z = 0.0;
			for (int l = j; l >= 0; l--) {
				const double q = w / dii;
				const double zl = __shfl(q, l, 64);
				if (lane == l) z = zl;
				if (lane < l) w = __builtin_fma(-W3[l * 64 + lane], zl, w);
			}
			if (lane <= j) W0[j * 64 + lane] = z;
		}
		__syncthreads();
		// Y = Ui^T T
		double y[4];
#pragma unroll
		for (int u = 0; u < 4; u++) {
			const int e = t + 1024 * u, i = e & 63, j = e >> 6;
			double s = 0.0;
			if (i < k && j < k)
				for (int l = 0; l <= i; l++) s = __builtin_fma(W0[i * 64 + l], W1[j * 64 + l], s);
			y[u] = s;
		}
#pragma unroll
		for (int u = 0; u < 4; u++) W3[t + 1024 * u] = y[u];                  // (W3 held Uc: only its own thread reads or writes a word here)
		__syncthreads();
		// V = Ui Y
#pragma unroll
		for (int u = 0; u < 4; u++) {
			const int e = t + 1024 * u, i = e & 63, j = e >> 6;
			double s = 0.0;
			if (i < k && j < k)
				for (int l = i; l < k; l++) s = __builtin_fma(W0[l * 64 + i], W3[j * 64 + l], s);
			y[u] = s;
		}
		__syncthreads();                                      // every thread has read T (W1) and Ui (W0)
#pragma unroll
		for (int u = 0; u < 4; u++) { W1[t + 1024 * u] = y[u]; W0[t + 1024 * u] = 0.0; }
		__syncthreads();
		// the image of Zmn: rows jpvt[:k] take V, rows jpvt[k:n] take M^T V
#pragma unroll
		for (int u = 0; u < 4; u++) {
			const int e = t + 1024 * u, i = e & 63, j = e >> 6;
			if (i < n && j < k && piv[i] >= 0) {
				double s = 0.0;
				if (i < k) s = W1[e];
				else
					for (int l = 0; l < k; l++) s = __builtin_fma(W2[i * 64 + l], W1[j * 64 + l], s);
				W0[j * 64 + piv[i]] = s;
			}
		}
	} else {
		__syncthreads();                                      // (uniform branch: every thread is here) the last reads of W0 are done
#pragma unroll
		for (int u = 0; u < 4; u++) W0[t + 1024 * u] = 0.0;
	}
	__syncthreads();
#pragma unroll
	for (int u = 0; u < 4; u++) {
		const int e = t + 1024 * u, i = e & 63, j = e >> 6;
		if (i < NP && j < NP) a.zmn[(size_t)j * NP + i] = W0[e];
	}
	if (t == 0) {
		a.status[0] = verdict;
		if (a.host_status) { volatile unsigned* hs = a.host_status; hs[0] = verdict; }
	}
}

}  // namespace tsqrmi

namespace {

// lsq_zg_f64_kernel on stream st: one wave
inline void f64k_zg_launch(hipStream_t st, const tsqrmi::LsqZgArgs64& za) {
	hipLaunchKernelGGL(tsqrmi::lsq_zg_f64_kernel, dim3(1), dim3(64), 0, st, za);
}
// lsq_minnorm_f64_kernel on stream st: one workgroup
inline void f64k_minnorm_launch(hipStream_t st, const tsqrmi::LsqMinnormArgs64& ma) {
	hipLaunchKernelGGL(tsqrmi::lsq_minnorm_f64_kernel, dim3(1), dim3(1024), 0, st, ma);
}
// lsq_rank_f64_kernel on stream st: one workgroup
inline void f64k_rank_launch(hipStream_t st, const tsqrmi::LsqRankArgs64& ka) {
	hipLaunchKernelGGL(tsqrmi::lsq_rank_f64_kernel, dim3(1), dim3(1024), 0, st, ka);
}
// the dense Gram pass on stream st: gramq_dense_f64_kernel<NT, AROW> (ga.z dense) on the grid of f64r_gramq_launch
inline void f64k_gramq_launch(hipStream_t st, const F64Plan& g, const tsqrmi::GramQArgs64& ga, int a_layout = 0) {
	with_nt(g.NT, [&](auto nt) {
		with_layout(a_layout, [&](auto ar) {
			hipLaunchKernelGGL((tsqrmi::gramq_dense_f64_kernel<decltype(nt)::value, decltype(ar)::value>), dim3(g.nblocks), dim3(256), 0, st, ga);
		});
	});
}
// lsq_rank_step_f64_kernel on stream st: one workgroup
inline void f64k_step_launch(hipStream_t st, const tsqrmi::LsqRankStepArgs64& sa) {
	hipLaunchKernelGGL(tsqrmi::lsq_rank_step_f64_kernel, dim3(1), dim3(1024), 0, st, sa);
}
// one dense pass on stream st: lsq_dense_f64_kernel<NT, AROW, BROW> (la.z dense) on the grid of f64r_lsq_launch
inline void f64k_lsq_launch(hipStream_t st, const F64Plan& g, const tsqrmi::LsqArgs64& la, int a_layout = 0, int b_layout = 0) {
	with_nt(g.NT, [&](auto nt) {
		with_layout(a_layout, [&](auto ar) {
			with_layout(b_layout, [&](auto br) {
				hipLaunchKernelGGL((tsqrmi::lsq_dense_f64_kernel<decltype(nt)::value, decltype(ar)::value, decltype(br)::value>),
				                   dim3(g.nblocks), dim3(256), 0, st, la);
			});
		});
	});
}

}  // namespace

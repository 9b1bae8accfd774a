// orth_f64.hip -- the device passes of the fp64 block orthogonalisation against an existing basis (tsqr_mi_orth_f64: n <= 64, k <= 1024;
// include/tsqr_mi.h has the method, DESIGN.md section 9 the figures) and their launchers.  Included by tsqr_mi.hip and selftest.hip behind
// tsqr_f64.hip, tsqr_f64_wide.hip and f64_plan.h:
//   orth_gram_f64_kernel   : per-slice partials of S = V^T X, one wave per (64-column block of V, row slice), on v_mfma_f64_16x16x4_f64
//   (gram_reduce1_kernel   : the partials of every slice summed in a fixed tree, unchanged)
//   orth_update_f64_kernel : X <- X - V S in place on v_mfma_f64_16x16x4_f64, S staged in LDS one 64-row block at a time
//   orth_s_f64_kernel      : the caller's S from the work copy: S = S1 (round 1), S += S2 R1 (round 2), one workgroup per 64 rows of S
// The two tall kernels take the layout of V and of X as template flags (VROW, XROW).  Element (i, j) of a row-major operand lies at
// p[i * ld + j], ld >= the column count.  The house rule of tsqr_f64.hip holds: a row-major V or X puts the same value into the register
// the column-major instance holds it in (the Gram pass; the V operand of the update), and a row-major X of the update swaps the MFMA
// operands.  So S, Q and everything behind them have the same bits for all four layout pairs.
// The work copy of S ("Sw"): kblocks = ceil(k / 64) blocks of 64 x NP doubles, NP = 16 ceil(n / 16); S[64 b + r][c] at
// b * 64 * NP + 64 * c + r.  Rows >= k and columns >= n of it are sums of products with exact zeros.
#pragma once
#include <hip/hip_runtime.h>

namespace tsqrmi {

// x[i] = P[row0 + i][col], i = 0 .. 3, zero where !colok or the row is >= m (neither is read).  ROW: P is row-major.
template <bool ROW>
__device__ __forceinline__ void orth_load4(double (&x)[4], const double* __restrict__ p, size_t ld, size_t row0, int col, bool colok, bool full,
                                           size_t m) {
	if constexpr (ROW) {
		const double* src = p + row0 * ld + col;
#pragma unroll
		for (int i = 0; i < 4; i++) x[i] = (colok && (full || row0 + i < m)) ? src[(size_t)i * ld] : 0.0;
	} else {
		const double* src = p + (size_t)col * ld + row0;
		if (colok && full) {
			const f64x2u v0 = *reinterpret_cast<const f64x2u*>(src);
			const f64x2u v1 = *reinterpret_cast<const f64x2u*>(src + 2);
			x[0] = v0[0]; x[1] = v0[1]; x[2] = v1[0]; x[3] = v1[1];
		} else {
#pragma unroll
			for (int i = 0; i < 4; i++) x[i] = (colok && row0 + i < m) ? src[i] : 0.0;
		}
	}
}

// ---- the cross-Gram pass ---------------------------------------------------------------------------------------------------------------
struct OrthGramArgs64 {
	const double* v; size_t ldv;         // m x k, read only
	const double* x; size_t ldx;         // m x n
	size_t m; int k, n;
	int kblocks, nslices;                // 64-column blocks of V; row slices
	size_t cps, nch;                     // 16-row chunks per slice, chunks
	double* part;                        // [nslices][kblocks][64 * NP]: block b of slice s in Sw's layout
};

// One wave per (block b of V, row slice): 4 NT accumulators of 16 x 16 for the 64 x NP block of V^T X, gram_wide_f64_kernel's scheme
// for the block pair (V_b, X).  The chunk is 16 rows: lane (c, q) holds rows 4 q .. 4 q + 3 of column 64 b + 16 t + c of V (t < 4)
// and of column 16 t + c of X (t < NT) -- 32-byte runs of one column, or four rows of one 128-byte row segment when the operand is
// row-major -- and MFMA step rho takes row 4 q + rho of both.  The next chunk is loaded before the products of this one, on two
// register sets rotated by unrolling.  Wave gw = 4 blockIdx.x + wave takes block gw % kblocks of slice gw / kblocks: neighbouring waves
// share the rows of X.  Columns >= k of V's last block, columns >= n of X and rows >= m are exact zeros and are NEVER loaded: in
// row-major storage that address is the next row's data, padding or, on the last row, beyond the allocation (gram_wide_f64_kernel).
// Entry (i, j) of a partial sums the rows of its slice in ascending order, four to an MFMA: a fixed function of the operands.
template <int NT, bool VROW, bool XROW>
__global__ __launch_bounds__(256) void orth_gram_f64_kernel(const OrthGramArgs64 g) {
	constexpr int NP = 16 * NT;
	const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
	const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);
	const int b = gw % g.kblocks, slice = gw / g.kblocks;
	if (slice >= g.nslices) return;                      // (no barriers in this kernel)
	f64x4 acc[4 * NT];
#pragma unroll
	for (int t = 0; t < 4 * NT; t++) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
	const size_t ch0 = (size_t)slice * g.cps, ch1 = std::min(g.nch, ch0 + g.cps);
	auto load = [&](double (&x)[4 + NT][4], size_t ch) {
		const size_t row0 = ch * 16 + 4 * q;
		const bool full = ch * 16 + 16 <= g.m;
#pragma unroll
		for (int t = 0; t < 4; t++) {
			const int col = 64 * b + 16 * t + c;
			orth_load4<VROW>(x[t], g.v, g.ldv, row0, col, col < g.k, full, g.m);
		}
#pragma unroll
		for (int t = 0; t < NT; t++) {
			const int col = 16 * t + c;
			orth_load4<XROW>(x[4 + t], g.x, g.ldx, row0, col, col < g.n, full, g.m);
		}
	};
	auto prod = [&](const double (&x)[4 + NT][4]) {
#pragma unroll
		for (int rho = 0; rho < 4; rho++)
#pragma unroll
			for (int ti = 0; ti < 4; ti++)
#pragma unroll
				for (int tj = 0; tj < NT; tj++)
					acc[ti * NT + tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[ti][rho], x[4 + tj][rho], acc[ti * NT + tj], 0, 0, 0);
	};
	double x0[4 + NT][4], x1[4 + NT][4];
	if (ch0 < ch1) load(x0, ch0);
	for (size_t ch = ch0; ch < ch1; ch += 2) {              // (two register sets rotated by unrolling, never by moves)
		if (ch + 1 < ch1) load(x1, ch + 1);
		prod(x0);
		if (ch + 1 >= ch1) break;
		if (ch + 2 < ch1) load(x0, ch + 2);
		prod(x1);
	}
	double* out = g.part + ((size_t)slice * g.kblocks + b) * (64 * NP);
#pragma unroll
	for (int ti = 0; ti < 4; ti++)
#pragma unroll
		for (int tj = 0; tj < NT; tj++)
#pragma unroll
			for (int reg = 0; reg < 4; reg++) part_store(&out[(16 * tj + c) * 64 + 16 * ti + q + 4 * reg], acc[ti * NT + tj][reg]);
}

// ---- the projection update ---------------------------------------------------------------------------------------------------------------
struct OrthUpdateArgs64 {
	double* x; size_t ldx;               // m x n, in and out
	const double* v; size_t ldv;         // m x k, read only
	size_t m; int k, n, kblocks;
	const double* s;                     // Sw: the summed partials of orth_gram_f64_kernel
};

// X <- X - V S in place.  A wave owns 32 rows (two 16-row tiles), a workgroup 128; the accumulators START as the wave's tiles of X and
// take the products of -S with V, 4 of k to an MFMA, k ascending: entry (r, j) is X[r][j], then the k-blocks 0 .. 16 kblocks - 1 in
// that order, for every layout.  Register contents, the same for every layout: vc, lane (li, lq) holds V[row0 + li][64 b + 4 kb + lq]
// (apply_f64_kernel's av); the S operand, lane (li, lq) of operand (jt, kb) holds -S[64 b + 4 kb + lq][16 jt + li] (its zop, negated:
// exact).  The layout of X picks the ORDER of the MFMA operands as in apply_f64_kernel: column-major X, D[j][r] += (-S)^T[j][k] V^T[k][r],
// register reg of lane (li, lq) is X[row0 + li][16 jt + lq + 4 reg]; row-major X, the operands swapped, register reg of lane (li, lq) is
// X[row0 + lq + 4 reg][16 jt + li].  The swap exchanges the factors of each product and nothing else, so X has the same bits.
// S does not fit in LDS at k = 1024 (512 KiB), so it is STAGED IN 64-ROW BLOCKS: block b, 64 x NP, in operand order -- operand (jt, kb) is
// 64 consecutive doubles, lane l reads element l, one conflict-free 8-byte read feeds the MFMAs of both row tiles (applyd_f64_kernel's
// scheme) -- in two buffers, block b + 1 written while block b is used, one barrier per block; V of block b + 1 is loaded ahead too.
// The price: every workgroup reads all of S once, through the L2, NP / 128 of the bytes it reads of V (a half at n = 64).
// In place is safe: a wave reads all n columns of its rows before it writes any of them (the accumulators are loaded first and stored
// last), and no two waves share a row (apply_f64_kernel's argument).  Nothing at a row >= m, or at a column between n and the leading
// dimension of X or between k and that of V, is read or written.
template <int NT, bool VROW, bool XROW>
__global__ __launch_bounds__(256) void orth_update_f64_kernel(const OrthUpdateArgs64 a) {
	constexpr int NP = 16 * NT, SB = NT * 16 * 64;
	__shared__ double sl[2][SB];
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, lq = lane >> 4;
	const size_t row0 = ((size_t)blockIdx.x * 4 + wv) * 32;
	auto stage = [&](int buf, int b) {
		const double* sb = a.s + (size_t)b * (64 * NP);
		for (int e = threadIdx.x; e < SB; e += 256) {
			const int l = e & 63, o = e >> 6, jt = o >> 4, kb = o & 15;
			sl[buf][e] = -sb[64 * (16 * jt + (l & 15)) + 4 * kb + (l >> 4)];
		}
	};
	auto loadv = [&](double (&vv)[2][16], int b) {
#pragma unroll
		for (int rt = 0; rt < 2; rt++) {
			const size_t row = row0 + 16 * rt + li;
#pragma unroll
			for (int kb = 0; kb < 16; kb++) {
				const int col = 64 * b + 4 * kb + lq;
				const bool live = row < a.m && col < a.k;
				if constexpr (VROW) vv[rt][kb] = live ? a.v[row * a.ldv + col] : 0.0;
				else vv[rt][kb] = live ? a.v[(size_t)col * a.ldv + row] : 0.0;
			}
		}
	};
	f64x4 acc[2][NT];
#pragma unroll
	for (int rt = 0; rt < 2; rt++)
#pragma unroll
		for (int jt = 0; jt < NT; jt++)
#pragma unroll
			for (int reg = 0; reg < 4; reg++) {
				if constexpr (XROW) {
					const size_t row = row0 + 16 * rt + lq + 4 * reg;
					const int col = 16 * jt + li;
					acc[rt][jt][reg] = (row < a.m && col < a.n) ? a.x[row * a.ldx + col] : 0.0;
				} else {
					const size_t row = row0 + 16 * rt + li;
					const int col = 16 * jt + lq + 4 * reg;
					acc[rt][jt][reg] = (row < a.m && col < a.n) ? a.x[(size_t)col * a.ldx + row] : 0.0;
				}
			}
	double vc[2][16], vn[2][16];
	stage(0, 0);
	loadv(vc, 0);
	for (int b = 0; b < a.kblocks; b++) {
		__syncthreads();                                     // block b is staged; every wave is done with the buffer of block b - 1
		if (b + 1 < a.kblocks) { stage((b + 1) & 1, b + 1); loadv(vn, b + 1); }
		const double* sop = sl[b & 1];
#pragma unroll
		for (int jt = 0; jt < NT; jt++)
#pragma unroll
			for (int kb = 0; kb < 16; kb++) {
				const double so = sop[(jt * 16 + kb) * 64 + lane];
#pragma unroll
				for (int rt = 0; rt < 2; rt++) {
					if constexpr (XROW) acc[rt][jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(vc[rt][kb], so, acc[rt][jt], 0, 0, 0);
					else acc[rt][jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(so, vc[rt][kb], acc[rt][jt], 0, 0, 0);
				}
			}
		if (b + 1 < a.kblocks) {
#pragma unroll
			for (int rt = 0; rt < 2; rt++)
#pragma unroll
				for (int kb = 0; kb < 16; kb++) vc[rt][kb] = vn[rt][kb];
		}
	}
#pragma unroll
	for (int rt = 0; rt < 2; rt++)
#pragma unroll
		for (int jt = 0; jt < NT; jt++)
#pragma unroll
			for (int reg = 0; reg < 4; reg++) {
				if constexpr (XROW) {
					const size_t row = row0 + 16 * rt + lq + 4 * reg;
					const int col = 16 * jt + li;
					if (row < a.m && col < a.n) a.x[row * a.ldx + col] = acc[rt][jt][reg];
				} else {
					const size_t row = row0 + 16 * rt + li;
					const int col = 16 * jt + lq + 4 * reg;
					if (row < a.m && col < a.n) a.x[(size_t)col * a.ldx + row] = acc[rt][jt][reg];
				}
			}
}

// ---- the caller's S ------------------------------------------------------------------------------------------------------------------------
struct OrthSArgs64 {
	double* s; size_t lds;               // k x n, column-major: written (second == 0) or updated in place (second != 0)
	const double* sw;                    // Sw of this round
	const double* r1; size_t ldr;        // second != 0: R of round 1, n x n upper triangular (only i <= j is read)
	int k, n, NP, second;
};

// One workgroup per 64-row block of S, no tall operand.  Round 1: S = Sw.  Round 2: S += S2 R1 -- entry (i, j) starts from S1[i][j]
// and takes l = 0 .. j in that order, one fused multiply-add each: a fixed function of the input.  The block of Sw and R1 are held in
// LDS (64 KB); thread (i, w) takes row 64 b + i and the columns w, w + 16, ...  Nothing at a row >= k or a column >= n is written.
__global__ __launch_bounds__(1024) void orth_s_f64_kernel(const OrthSArgs64 a) {
	__shared__ double S2[64 * 64], R[64 * 64];
	const int t = threadIdx.x, i = t & 63, w = t >> 6, b = blockIdx.x;
#pragma unroll
	for (int u = 0; u < 4; u++) {
		const int e = t + 1024 * u, ii = e & 63, j = e >> 6;
		S2[e] = j < a.NP ? a.sw[(size_t)b * (64 * a.NP) + 64 * j + ii] : 0.0;
		R[e] = (a.second && ii <= j && j < a.n) ? a.r1[(size_t)j * a.ldr + ii] : 0.0;
	}
	__syncthreads();
	const int row = 64 * b + i;
	if (row >= a.k) return;
	for (int j = w; j < a.n; j += 16) {
		double* dst = a.s + (size_t)j * a.lds + row;
		if (!a.second) { *dst = S2[j * 64 + i]; continue; }
		double v = *dst;
		for (int l = 0; l <= j; l++) v = __builtin_fma(S2[l * 64 + i], R[j * 64 + l], v);
		*dst = v;
	}
}

}  // namespace tsqrmi

namespace {

// ---- tsqr_mi_orth_f64 (n <= 64, k <= 1024): plan, work space, launchers ---------------------------------------------------------------------
constexpr size_t F64O_MAX_K = 1024;
constexpr int F64O_GRAM_WAVES = 1024;                   // fixed, like F64_GRAM_WAVES: the work-space size and the reduction tree follow no setting
// wq (doubles): [the F64_WQ layout of the QR entry][R of round 2, n x n with ld 64: 4096][Sw: kblocks blocks of 64 x 64 at most + the
// row-count word of the reduction]
constexpr size_t F64O_RW = F64_WQ, F64O_SW = F64O_RW + 4096;
inline size_t f64o_wq_doubles(size_t k) { return F64O_SW + cdiv(std::min(k, F64O_MAX_K), 64) * 4096 + 8; }

// The slicing rule of the cross-Gram pass: at most F64O_GRAM_WAVES / kblocks slices (64 at k = 1024) of whole 16-row chunks, none empty
struct F64OPlan { int NT, kblocks, nslices; size_t cps, nch; };
inline F64OPlan f64o_plan(size_t m, size_t k, size_t n) {
	F64OPlan g{};
	g.NT = (int)(np_of(n) / 16);
	g.kblocks = (int)cdiv(k, 64);
	g.nch = cdiv(m, 16);
	const size_t want = std::max<size_t>(1, std::min((size_t)F64O_GRAM_WAVES / (size_t)g.kblocks, g.nch));
	g.cps = cdiv(g.nch, want);
	g.nslices = (int)cdiv(g.nch, g.cps);                 // (<= want)
	return g;
}
// doubles of wr: never below the partials of the QR entry's Gram pass or of the cross-Gram pass, and monotone in m, k and n
inline size_t f64o_wr_doubles(size_t m, size_t k, size_t n) {
	const size_t NT = np_of(n) / 16, kblocks = cdiv(std::min(k, F64O_MAX_K), 64);
	const size_t qr = cdiv(std::min<size_t>(cdiv(m, 64), (size_t)F64_GRAM_WAVES), 4) * (NT * (NT + 1) / 2) * 256;
	const size_t cross = std::min<size_t>(cdiv(m, 16) * kblocks, (size_t)F64O_GRAM_WAVES) * 64 * 16 * NT;
	return std::max(qr, cross);
}

// f(nt, vrow, xrow) for the instantiation <NT, VROW, XROW> of n columns and the two layouts
template <class F> inline auto with_orth(int NT, int v_layout, int x_layout, F&& f) {
	return with_nt(NT, [&](auto nt) {
		return with_layout(v_layout, [&](auto vr) { return with_layout(x_layout, [&](auto xr) { return f(nt, vr, xr); }); });
	});
}
// the cross-Gram pass on stream st: one wave per (block, slice), four to a workgroup
inline void f64o_gram_launch(hipStream_t st, const F64OPlan& g, const tsqrmi::OrthGramArgs64& ga, int v_layout, int x_layout) {
	const unsigned wgs = (unsigned)cdiv((size_t)g.kblocks * g.nslices, 4);
	with_orth(g.NT, v_layout, x_layout, [&](auto nt, auto vr, auto xr) {
		hipLaunchKernelGGL((tsqrmi::orth_gram_f64_kernel<decltype(nt)::value, decltype(vr)::value, decltype(xr)::value>), dim3(wgs), dim3(256), 0,
		                   st, ga);
	});
}
// the projection update on stream st: one workgroup per 128 rows
inline void f64o_update_launch(hipStream_t st, const F64OPlan& g, const tsqrmi::OrthUpdateArgs64& ua, int v_layout, int x_layout) {
	with_orth(g.NT, v_layout, x_layout, [&](auto nt, auto vr, auto xr) {
		hipLaunchKernelGGL((tsqrmi::orth_update_f64_kernel<decltype(nt)::value, decltype(vr)::value, decltype(xr)::value>),
		                   dim3((unsigned)cdiv(ua.m, 128)), dim3(256), 0, st, ua);
	});
}
// orth_s_f64_kernel on stream st: one workgroup per 64 rows of S
inline void f64o_s_launch(hipStream_t st, const tsqrmi::OrthSArgs64& sa) {
	hipLaunchKernelGGL(tsqrmi::orth_s_f64_kernel, dim3((unsigned)cdiv((size_t)sa.k, 64)), dim3(1024), 0, st, sa);
}

}  // namespace

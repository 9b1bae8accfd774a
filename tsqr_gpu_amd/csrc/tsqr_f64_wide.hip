// tsqr_f64_wide.hip -- the device side of the wide double-precision entry (tsqr_mi_qr_f64_wide, 64 < n <= 1024): whole-matrix CholeskyQR
// sweeps on 64-column blocks, nb = ceil(n / 64) of them, the last one zero padded.  Included by tsqr_mi.hip after tsqr_wide.hip (whose
// tile_product_f64 it reuses) and tsqr_f64.hip.
//
// Block storage (work space): every n x n quantity -- G, the Schur complements W, R, Z = inverse(R), the products T of the triangular
// inverse, the copy of R for the R product -- is kept as its upper block pairs (I <= J), pair p = J (J + 1) / 2 + I, each a 64 x 64
// column-major block: X[64 I + r][64 J + c] at 4096 p + 64 c + r.  Columns >= n are exact zeros everywhere.
//   gram_wide_f64_kernel   : partials of A^T A, one wave per block pair and row slice, on v_mfma_f64_16x16x4_f64
//   (gram_reduce1_kernel   : the partials of every slice summed in a fixed tree, unchanged)
//   cholw_diag_kernel      : step k, chol(G'_kk) -> R_kk, Z_kk with chol_body16<double> (unchanged)
//   cholw_row_kernel       : step k, R_kJ = Z_kk^T G'_kJ (J > k), Z_Ik = -T_Ik Z_kk (I < k), Z_kk into the block store, the verdict terms
//   cholw_update_kernel    : step k, G'_IJ -= R_kI^T R_kJ (k < I <= J), T_IJ += Z_Ik R_kJ (I <= k < J)
//   cholw_verdict_kernel   : the verdict over the whole matrix: every block's pivots, the smallest pivot ratio and S, both taken with the
//                            ORIGINAL diagonal of G (chol_wide_kernel's rule for any number of blocks)
//   apply_wide_f64_kernel  : Q = A Z, in place allowed
//   rcopy / rsave / rmul_wide_f64_kernel : R out (first sweep), R <- R_k R through a work-space copy (later sweeps)
// The block products run on sixteen waves, one 16 x 16 output tile each, both operands staged in LDS (tile_product_f64).
// Only the two kernels that touch A or Q know a layout (tsqr_mi_qr_f64_wide_lay): gram_wide_f64_kernel<AROW> and
// apply_wide_f64_kernel<AROW, QROW>, one body each with the layout as a template flag like the n <= 64 kernels of tsqr_f64.hip.  Element
// (i, j) of a row-major operand lies at s[i * ld + j], ld >= n.  A row-major instance puts the same value into the same register and a
// row-major Q swaps the MFMA operands, so every bit of G, R and Q is that of the column-major instance on the transposed copy.
#include <hip/hip_runtime.h>

namespace tsqrmi {

__host__ __device__ constexpr int wpair(int I, int J) { return J * (J + 1) / 2 + I; }

struct WideF64 {
	const double* gs;                    // summed Gram blocks (+ the row count behind them)
	double* w;                           // Schur complements G' (step >= 1)
	double* rw;                          // R of the sweep
	double* zw;                          // Z = inverse(R)
	double* ta;                          // T_IJ = sum_{I <= K < k} Z_IK R_KJ, I < J (the triangular inverse, accumulated step by step)
	double* zd;                          // [nb][4096]: chol_body16's Z_kk (ld NP_k)
	double* sb;                          // [nb * nb] S terms of the Z blocks, [nb * nb + k] pivot-ratio minimum of block k
	unsigned* bst;                       // [nb][4] chol_body16's status words of block k
	unsigned* status;                    // verdict words of the sweep: [0] verdict, [1] min ratio (float bits), [2] S (float bits), [3] one sweep
	unsigned* host_status;               // pinned host alias of the same four words (written by the last kernel of the chain)
	const unsigned* run_if;              // shifted chain: the plain verdict word; the kernel runs only when it is not 0
	double shift_coef;                   // 11 u (m n + n (n + 1)): s = shift_coef * trace(G), shifted chain only (0 otherwise)
	float max_scond, alone_max;
	int n, nb;
	const double* rows_dev;              // row-partitioned call: the all-reduced (global) row count behind the summed blocks.  The two bounds
	int first;                           // and the coefficient of the shift are then f64_rule_of(rows_dev[0], n, first) (tsqr_f64.hip); of
	                                     // shift_coef only "> 0: the shifted chain" is looked at.  Null: one GPU, the arguments hold
};

__device__ __forceinline__ bool wide_skip(const WideF64& a) { return a.run_if && a.run_if[0] == 0u; }

// s = shift_coef * trace(G) of the original G, one fixed order (every kernel that adds it gets the same bits); all threads receive it
__device__ double wide_shift(const WideF64& a) {
	__shared__ double sh;
	if (threadIdx.x < 64) {
		const int j = threadIdx.x;
		double tr = 0.0;
		for (int c = j; c < a.n; c += 64) tr += a.gs[(size_t)wpair(c >> 6, c >> 6) * 4096 + (c & 63) * 65];
		for (int o = 32; o > 0; o >>= 1) tr += __shfl_xor(tr, o);
		// (one expression for every caller; the coefficient of a row-partitioned call is a pure function of one word every kernel reads alike)
		if (j == 0) sh = (a.rows_dev ? f64_rule_of(a.rows_dev[0], a.n, a.first != 0).shift_coef : a.shift_coef) * tr;
	}
	__syncthreads();
	return sh;
}

// a 64 x 64 column-major block (ld 64) into LDS (ld 65); 1024 threads
__device__ __forceinline__ void wide_stage(double* __restrict__ s, const double* __restrict__ g) {
#pragma unroll
	for (int u = 0; u < 4; u++) {
		const int e = threadIdx.x + 1024 * u;
		s[(e >> 6) * 65 + (e & 63)] = g[e];
	}
}
// chol_body16's Z_kk (ld np, zero padded to np x np) into LDS (ld 65), zeros beyond np
__device__ __forceinline__ void wide_stage_zd(double* __restrict__ s, const double* __restrict__ zd, int np) {
#pragma unroll
	for (int u = 0; u < 4; u++) {
		const int e = threadIdx.x + 1024 * u, r = e & 63, c = e >> 6;
		s[c * 65 + r] = (r < np && c < np) ? zd[c * np + r] : 0.0;
	}
}

// this wave's tile of X^T Y (TRANS) or X Y, both staged with ld 65; c[reg] = C[16 ti + lq + 4 reg][16 tj + li]
template <bool TRANS>
__device__ __forceinline__ f64x4 wide_prod(const double* Xs, const double* Ys) {
	const int w = threadIdx.x >> 6, l = threadIdx.x & 63, ti = w >> 2, tj = w & 3, li = l & 15, lq = l >> 4;
	return tile_product_f64(
		[&](int k) { return TRANS ? Xs[(16 * ti + li) * 65 + k] : Xs[k * 65 + 16 * ti + li]; },
		[&](int k) { return Ys[(16 * tj + li) * 65 + k]; }, 0, 16, lq);
}

// sum over the workgroup (1024 threads) in a fixed order; every thread receives it
__device__ __forceinline__ double wide_wg_sum(double v, double* red) {
	for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
	__syncthreads();
	if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
	__syncthreads();
	double s = 0.0;
#pragma unroll
	for (int k = 0; k < 16; k++) s += red[k];
	return s;
}

// ---- Gram pass ----------------------------------------------------------------------------------------------------------------------
// One wave per (block pair, row slice): sixteen 16 x 16 accumulators for the 64 x 64 block G_IJ.  The chunk is 16 rows (gram_f64_kernel's
// is 64): lane (c, q) holds rows 4 q .. 4 q + 3 of column c of each of the eight column tiles of blocks I and J -- 32 operands, loaded as
// 32-byte runs of one column -- and MFMA step rho takes row 4 q + rho.  The next chunk is loaded before the products of this one.  The four
// waves of a workgroup take four consecutive pairs (they share block J: one read from memory, the others from the caches) of the same
// slice, and consecutive workgroups take the same slice: the rows of a slice are read from memory about once.  Partials:
// part[(slice * npairs + p) * 4096 + 64 c + r], the block store's layout, summed by gram_reduce1_kernel over the slices.
// AROW: A is row-major (g.lda: the row stride, >= n).  The same 32 registers receive the same values -- lane (c, q) holds rows
// 16 ch + 4 q .. + 3 of column 64 blk + 16 t + c -- so every partial has the bits of the column-major instance on the transposed copy.
// The loads are 8 bytes per lane, one row per instruction: the sixteen lanes of a quarter cover 128 contiguous bytes of that row.  A
// column >= n of the zero-padded last block is an exact zero and is NEVER loaded: in row-major storage that address is the next row's
// data (lda == n), padding (lda > n) or, on the last row, beyond the allocation.  Rows >= m likewise.
struct GramWideF64Args {
	const double* a; size_t lda; size_t m; int n;
	int npairs, ngroups;                 // pairs, workgroups per slice (four pairs each)
	size_t cps, nch;                     // 16-row chunks per slice, chunks
	double* part;
};

template <bool AROW>
__global__ __launch_bounds__(256) void gram_wide_f64_kernel(const GramWideF64Args g) {
	const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
	const int grp = blockIdx.x % g.ngroups, slice = blockIdx.x / g.ngroups;
	const int p = 4 * grp + (threadIdx.x >> 6);
	if (p >= g.npairs) return;                           // (no barriers in this kernel)
	int J = 0;
	while ((J + 1) * (J + 2) / 2 <= p) J++;
	const int I = p - J * (J + 1) / 2;
	f64x4 acc[16];
#pragma unroll
	for (int t = 0; t < 16; t++) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
	const size_t ch0 = (size_t)slice * g.cps, ch1 = std::min(g.nch, ch0 + g.cps);
	auto load = [&](double (&x)[8][4], size_t ch) {
		const size_t row0 = ch * 16 + 4 * q;
		const bool full = ch * 16 + 16 <= g.m;
#pragma unroll
		for (int t = 0; t < 8; t++) {
			const int col = 64 * (t < 4 ? I : J) + 16 * (t & 3) + c;
			if constexpr (AROW) {
				const double* src = g.a + row0 * g.lda + col;
#pragma unroll
				for (int i = 0; i < 4; i++) x[t][i] = (col < g.n && (full || row0 + i < g.m)) ? src[(size_t)i * g.lda] : 0.0;
				continue;
			}
			const double* src = g.a + (size_t)col * g.lda + row0;
			if (col < g.n && full) {
				const f64x2u v0 = *reinterpret_cast<const f64x2u*>(src);
				const f64x2u v1 = *reinterpret_cast<const f64x2u*>(src + 2);
				x[t][0] = v0[0]; x[t][1] = v0[1]; x[t][2] = v1[0]; x[t][3] = v1[1];
			} else {
#pragma unroll
				for (int i = 0; i < 4; i++) x[t][i] = (col < g.n && row0 + i < g.m) ? src[i] : 0.0;
			}
		}
	};
	auto prod = [&](const double (&x)[8][4]) {
#pragma unroll
		for (int rho = 0; rho < 4; rho++)
#pragma unroll
			for (int ti = 0; ti < 4; ti++)
#pragma unroll
				for (int tj = 0; tj < 4; tj++)
					acc[ti * 4 + tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[ti][rho], x[4 + tj][rho], acc[ti * 4 + tj], 0, 0, 0);
	};
	double x0[8][4], x1[8][4];
	if (ch0 < ch1) load(x0, ch0);
	for (size_t ch = ch0; ch < ch1; ch += 2) {              // (two register sets rotated by unrolling, never by moves)
		if (ch + 1 < ch1) load(x1, ch + 1);
		prod(x0);
		if (ch + 1 >= ch1) break;
		if (ch + 2 < ch1) load(x0, ch + 2);
		prod(x1);
	}
	double* out = g.part + ((size_t)slice * g.npairs + p) * 4096;
#pragma unroll
	for (int ti = 0; ti < 4; ti++)
#pragma unroll
		for (int tj = 0; tj < 4; tj++)
#pragma unroll
			for (int reg = 0; reg < 4; reg++) part_store(&out[(16 * tj + c) * 64 + 16 * ti + q + 4 * reg], acc[ti * 4 + tj][reg]);
}

// ---- the blocked Cholesky step, right-looking -------------------------------------------------------------------------------------
// Step k (k = 0 .. nb - 1): cholw_diag_kernel, cholw_row_kernel, cholw_update_kernel (none when k = nb - 1).  G' of step 0 is G itself
// (plus s I in the shifted chain), read from the summed blocks, so that the shifted chain can start again from the original G.
// The triangular inverse follows the factorisation: Z_Ik = -(sum_{I <= K < k} Z_IK R_Kk) Z_kk (from Z R = I), the sum accumulated in
// T_Ik by the update kernels of steps I .. k - 1, one term per step in step order.

// G' block (row tile entry e of chol_body16's fp64 tile order) -> value; the shift on the diagonal
struct WideDiagLoad {
	const double* blk; int NT; int nk; double shift;
	__device__ double operator()(int e) const {
		int rem = e >> 8, ti = 0;
		while (rem >= NT - ti) { rem -= NT - ti; ti++; }
		const int tj = ti + rem, t = e & 255, reg = t >> 6, l = t & 63;
		const int row = 16 * ti + (l >> 4) + 4 * reg, col = 16 * tj + (l & 15);
		double v = blk[col * 64 + row];
		if (row == col && row < nk) v += shift;
		return v;
	}
};

__global__ __launch_bounds__(1024) void cholw_diag_kernel(const WideF64 a, int k) {
	if (wide_skip(a)) return;
	const int nk = min(64, a.n - 64 * k), NT = (nk + 15) / 16;
	const double shift = (k == 0 && a.shift_coef > 0.0) ? wide_shift(a) : 0.0;
	const double* src = (k == 0 ? a.gs : a.w) + (size_t)wpair(k, k) * 4096;
	chol_body16(a.rw + (size_t)wpair(k, k) * 4096, (size_t)64, a.zd + (size_t)k * 4096, a.bst + 4 * k, (unsigned*)nullptr,
	            WideDiagLoad{src, NT, nk, shift}, nk, NT, 0, 0.0f, INFINITY);
}

// roles: blockIdx.x < nb - k - 1: R_kJ, J = k + 1 + blockIdx.x;  < nb - 1: Z_Ik, I = blockIdx.x - (nb - k - 1);  the last one: block k itself
__global__ __launch_bounds__(1024) void cholw_row_kernel(const WideF64 a, int k) {
	if (wide_skip(a)) return;
	__shared__ double Xs[64 * 65], Ys[64 * 65], red[16];
	const int t = threadIdx.x, w = t >> 6, l = t & 63, ti = w >> 2, tj = w & 3, li = l & 15, lq = l >> 4;
	const int nr = a.nb - k - 1, b = blockIdx.x;
	const int nk = min(64, a.n - 64 * k), npk = 16 * ((nk + 15) / 16);
	const double* zd = a.zd + (size_t)k * 4096;
	if (b < nr) {                                        // R_kJ = Z_kk^T G'_kJ (k < nb - 1: Z_kk is 64 x 64)
		const int J = k + 1 + b;
		wide_stage_zd(Xs, zd, npk);
		wide_stage(Ys, (k == 0 ? a.gs : a.w) + (size_t)wpair(k, J) * 4096);
		__syncthreads();
		const f64x4 c = wide_prod<true>(Xs, Ys);
		double* out = a.rw + (size_t)wpair(k, J) * 4096;
#pragma unroll
		for (int reg = 0; reg < 4; reg++) out[(16 * tj + li) * 64 + 16 * ti + lq + 4 * reg] = c[reg];
		return;
	}
	if (b < a.nb - 1) {                                  // Z_Ik = -T_Ik Z_kk, and its S term sum g_ii Z_ij^2
		const int I = b - nr;
		wide_stage(Xs, a.ta + (size_t)wpair(I, k) * 4096);
		wide_stage_zd(Ys, zd, npk);
		__syncthreads();
		const f64x4 c = wide_prod<false>(Xs, Ys);
		double* out = a.zw + (size_t)wpair(I, k) * 4096;
		const double* gd = a.gs + (size_t)wpair(I, I) * 4096;
		double s = 0.0;
#pragma unroll
		for (int reg = 0; reg < 4; reg++) {
			const int i = 16 * ti + lq + 4 * reg, j = 16 * tj + li;
			const double z = -c[reg];
			out[j * 64 + i] = z;
			s = fma(gd[i * 65] * z, z, s);
		}
		s = wide_wg_sum(s, red);
		if (t == 0) a.sb[I * a.nb + k] = s;
		return;
	}
	// block k: Z_kk into the block store (zero padded), R_kk's padding zeroed, the S term and the smallest pivot ratio r_jj^2 / g_jj.
	// A diagonal entry of the factored matrix (G, or G + s I in the shifted chain) below the normal range counts as a ratio of zero
	// (F64_MIN_DIAG, CholArgs64: the rule of the narrow entry, taken here on the ORIGINAL diagonal like the rest of the verdict).
	const double shift = (a.shift_coef > 0.0) ? wide_shift(a) : 0.0;     // (the whole workgroup has this role: the barrier inside is uniform)
	const double* gd = a.gs + (size_t)wpair(k, k) * 4096;
	double* zo = a.zw + (size_t)wpair(k, k) * 4096;
	double* ro = a.rw + (size_t)wpair(k, k) * 4096;
	double s = 0.0;
	float ratio = 1.0f;
#pragma unroll
	for (int u = 0; u < 4; u++) {
		const int e = t + 1024 * u, r = e & 63, c = e >> 6;
		const double z = (r < npk && c < npk) ? zd[c * npk + r] : 0.0;
		zo[e] = z;
		if (r >= nk || c >= nk) ro[e] = 0.0;
		if (r < nk && c < nk) {
			s = fma(gd[r * 65] * z, z, s);
			if (r == c) ratio = fminf(ratio, (gd[r * 65] + shift >= F64_MIN_DIAG) ? (float)(1.0 / (gd[r * 65] * z * z)) : 0.0f);
		}
	}
	for (int o = 32; o > 0; o >>= 1) ratio = fminf(ratio, __shfl_xor(ratio, o));
	s = wide_wg_sum(s, red);
	__shared__ float rred[16];
	if (l == 0) rred[w] = ratio;
	__syncthreads();
	if (t == 0) {
		float rm = 1.0f;
		for (int q = 0; q < 16; q++) rm = fminf(rm, rred[q]);
		a.sb[k * a.nb + k] = s;
		a.sb[a.nb * a.nb + k] = (double)rm;
	}
}

// roles: the trailing pairs (I, J), k < I <= J, in the order J, then I; then the T pairs (I, J), I <= k < J, I major
__global__ __launch_bounds__(1024) void cholw_update_kernel(const WideF64 a, int k) {
	if (wide_skip(a)) return;
	__shared__ double Xs[64 * 65], Ys[64 * 65];
	const int t = threadIdx.x, w = t >> 6, l = t & 63, ti = w >> 2, tj = w & 3, li = l & 15, lq = l >> 4;
	const int nt = a.nb - k - 1, ntrail = nt * (nt + 1) / 2;
	int b = blockIdx.x;
	if (b < ntrail) {                                    // G'_IJ = G'_IJ (+ s I on the diagonal at step 0) - R_kI^T R_kJ
		int J = k + 1;
		while (b >= J - k) { b -= J - k; J++; }
		const int I = k + 1 + b;
		const double shift = (k == 0 && a.shift_coef > 0.0 && I == J) ? wide_shift(a) : 0.0;
		wide_stage(Xs, a.rw + (size_t)wpair(k, I) * 4096);
		wide_stage(Ys, a.rw + (size_t)wpair(k, J) * 4096);
		__syncthreads();
		const f64x4 c = wide_prod<true>(Xs, Ys);
		const double* src = (k == 0 ? a.gs : a.w) + (size_t)wpair(I, J) * 4096;
		double* out = a.w + (size_t)wpair(I, J) * 4096;
#pragma unroll
		for (int reg = 0; reg < 4; reg++) {
			const int i = 16 * ti + lq + 4 * reg, j = 16 * tj + li;
			double g = src[j * 64 + i];
			if (i == j && 64 * I + i < a.n) g += shift;
			out[j * 64 + i] = g - c[reg];
		}
		return;
	}
	b -= ntrail;                                         // T_IJ (+)= Z_Ik R_kJ (the first term, I = k, is written)
	const int I = b / nt, J = k + 1 + b % nt;
	wide_stage(Xs, a.zw + (size_t)wpair(I, k) * 4096);
	wide_stage(Ys, a.rw + (size_t)wpair(k, J) * 4096);
	__syncthreads();
	const f64x4 c = wide_prod<false>(Xs, Ys);
	double* out = a.ta + (size_t)wpair(I, J) * 4096;
#pragma unroll
	for (int reg = 0; reg < 4; reg++) {
		const int i = 16 * ti + lq + 4 * reg, j = 16 * tj + li;
		out[j * 64 + i] = (I == k) ? c[reg] : out[j * 64 + i] + c[reg];
	}
}

// The verdict over all n columns (CholArgs64's rule, tsqr_f64.hip): every block's pivots positive and finite, the smallest pivot ratio
// r_jj^2 / g_jj above F64_MIN_PIVOT_RATIO (plain chain; > 0 in the shifted one), and S = ||D Z||_F^2 / n (D = diag(sqrt(g_jj)) of the ORIGINAL G, the Z blocks' terms added in pair order) against the
// CholeskyQR2 bound.  Plain chain: words [0] 0 / 1, [3] one sweep suffices.  Shifted chain (run_if set): when the plain verdict was 0 it
// changes nothing; otherwise 2 (accepted after the shift) or 1 (non-finite input), [3] = 0.  The shifted chain's launch is the last of
// the sweep's Cholesky step and always copies the four words to the pinned host words.
__global__ __launch_bounds__(64) void cholw_verdict_kernel(const WideF64 a) {
	if (threadIdx.x != 0) return;
	const bool shifted = a.run_if != nullptr;
	if (!shifted || a.run_if[0] != 0u) {
		unsigned bad = 0u;
		float rm = 1.0f;
		double ssum = 0.0;
		for (int J = 0; J < a.nb; J++) {
			bad |= a.bst[4 * J];
			rm = fminf(rm, (float)a.sb[a.nb * a.nb + J]);
			for (int I = 0; I <= J; I++) ssum += a.sb[I * a.nb + J];
		}
		const float scond = (float)(ssum / (double)a.n);
		F64Rule rule{a.shift_coef, a.max_scond, a.alone_max};
		if (a.rows_dev) rule = f64_rule_of(a.rows_dev[0], a.n, a.first != 0);
		const float max_scond = shifted ? INFINITY : rule.max_scond;
		const float min_ratio = shifted ? 0.0f : F64_MIN_PIVOT_RATIO;
		const bool ok = bad == 0u && rm > min_ratio && scond <= max_scond;     // NaN compares false -> rejected
		a.status[0] = shifted ? (ok ? 2u : 1u) : (ok ? 0u : 1u);
		a.status[1] = __builtin_bit_cast(unsigned, rm);
		a.status[2] = __builtin_bit_cast(unsigned, scond);
		a.status[3] = (!shifted && ok && scond <= rule.alone_max) ? 1u : 0u;
	}
	if (shifted) {
		volatile unsigned* hs = a.host_status;
		hs[1] = a.status[1];
		hs[2] = a.status[2];
		hs[3] = a.status[3];
		hs[0] = a.status[0];
	}
}

// ---- apply pass -----------------------------------------------------------------------------------------------------------------------
// Q = A Z.  Each wave owns 32 rows (two 16-row tiles) and produces the output blocks J = nb - 1 .. 0 in DESCENDING order, each from the
// input blocks K <= J (Z's zero blocks skipped), as Q^T tiles like apply_f64_kernel: MFMA operand A is Z^T, operand B is A^T, so sixteen
// lanes hold sixteen consecutive rows of one column of Q.  In place (q == a, ldq == lda) is safe: no two waves share a row, and output
// block J is the LAST consumer of input block J -- its stores depend on every load of its products, and the blocks J' < J that follow
// read columns < 64 (J' + 1) <= 64 J only.  (q and a are not __restrict__: the compiler keeps the next block's loads behind the stores.)
// Both register sets are the same for every layout: zop[jt], lane (li, lq) holds Z[64 K + 4 kb + lq][64 J + 16 jt + li]; av[rt], lane
// (li, lq) holds A[row0 + 16 rt + li][64 K + 4 kb + lq] (load_rows_rm's rule, tsqr_f64.hip).  AROW: A is row-major (lda: the row stride,
// >= n) -- another address for the same register.  QROW: Q is row-major (ldq: the row stride, >= n): the MFMA operands are swapped
// (apply_f64_kernel), D[r][j] = sum_k A[r][k] Z[k][j], register reg of lane (li, lq) holds Q[row0 + 16 rt + lq + 4 reg][64 J + 16 jt + li]
// and one store instruction writes four 128-byte row segments.  Either order adds to the accumulator of an entry of Q the same four
// products of the same k-block in the same order -- the swap transposes the tile and exchanges the two factors of each product, and
// IEEE multiplication is commutative -- so Q has the same bits for all four layout pairs
// (tests/test_gpu_f64_wide_rowmajor_passes.py compares them on the device).
// In place with any one layout (q == a, the same layout, ldq == lda) stays safe by the argument above, which speaks of rows and column
// blocks, not of addresses: a wave owns its 32 rows, output block J is stored after every load of the blocks K <= J, the blocks that
// follow read columns < 64 J only, and the rows of a row-major operand with ld >= n do not overlap.  Nothing at a row >= m or at a
// column in [n, ld) is read or written.
template <bool AROW, bool QROW>
__global__ __launch_bounds__(256) void apply_wide_f64_kernel(double* q, size_t ldq, const double* a, size_t lda, size_t m, int n, int nb,
                                                             const double* __restrict__ zw) {
	const int lane = threadIdx.x & 63, li = lane & 15, lq = lane >> 4;
	const size_t row0 = ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 32;
	if (row0 >= m) return;                               // (no barriers in this kernel)
	const bool full = row0 + 32 <= m;
	for (int J = nb - 1; J >= 0; J--) {
		f64x4 acc[2][4];
#pragma unroll
		for (int rt = 0; rt < 2; rt++)
#pragma unroll
			for (int jt = 0; jt < 4; jt++) acc[rt][jt] = f64x4{0.0, 0.0, 0.0, 0.0};
		for (int K = 0; K <= J; K++) {
			const double* zb = zw + (size_t)wpair(K, J) * 4096;
#pragma unroll 4
			for (int kb = 0; kb < 16; kb++) {
				const int col = 64 * K + 4 * kb + lq;
				double av[2], zop[4];
#pragma unroll
				for (int rt = 0; rt < 2; rt++) {
					const size_t row = row0 + 16 * rt + li;
					av[rt] = (col < n && (full || row < m)) ? (AROW ? a[row * lda + col] : a[(size_t)col * lda + row]) : 0.0;
				}
#pragma unroll
				for (int jt = 0; jt < 4; jt++) zop[jt] = zb[(16 * jt + li) * 64 + 4 * kb + lq];
#pragma unroll
				for (int jt = 0; jt < 4; jt++)
#pragma unroll
					for (int rt = 0; rt < 2; rt++) {
						if constexpr (QROW) acc[rt][jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[rt], zop[jt], acc[rt][jt], 0, 0, 0);
						else acc[rt][jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(zop[jt], av[rt], acc[rt][jt], 0, 0, 0);
					}
			}
		}
#pragma unroll
		for (int rt = 0; rt < 2; rt++) {
#pragma unroll
			for (int jt = 0; jt < 4; jt++)
#pragma unroll
				for (int reg = 0; reg < 4; reg++) {
					if constexpr (QROW) {
						const size_t row = row0 + 16 * rt + lq + 4 * reg;
						const int col = 64 * J + 16 * jt + li;
						if (row < m && col < n) q[row * ldq + col] = acc[rt][jt][reg];
					} else {
						const size_t row = row0 + 16 * rt + li;
						const int col = 64 * J + 16 * jt + lq + 4 * reg;
						if (row < m && col < n) q[(size_t)col * ldq + row] = acc[rt][jt][reg];
					}
				}
		}
	}
}

// ---- R out ----------------------------------------------------------------------------------------------------------------------------
// first sweep: r (n x n, ldr) = R of the block store, exact zeros below the diagonal
__global__ __launch_bounds__(256) void rcopy_wide_f64_kernel(double* r, size_t ldr, const double* __restrict__ rw, int n) {
	const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (e >= (size_t)n * n) return;
	const int i = (int)(e % n), j = (int)(e / n);
	r[(size_t)j * ldr + i] = (i <= j) ? rw[(size_t)wpair(i >> 6, j >> 6) * 4096 + (j & 63) * 64 + (i & 63)] : 0.0;
}
// later sweeps: the running R into the block store (rc) first -- the product below cannot run in place across workgroups
__global__ __launch_bounds__(256) void rsave_wide_f64_kernel(double* __restrict__ rc, const double* __restrict__ r, size_t ldr, int n, int npairs) {
	const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (e >= (size_t)npairs * 4096) return;
	const int p = (int)(e >> 12), rr = (int)(e & 63), cc = (int)((e >> 6) & 63);
	int J = 0;
	while ((J + 1) * (J + 2) / 2 <= p) J++;
	const int I = p - J * (J + 1) / 2, i = 64 * I + rr, j = 64 * J + cc;
	rc[e] = (i < n && j < n && i <= j) ? r[(size_t)j * ldr + i] : 0.0;
}
// r <- R_k R: output block (I, J), I <= J, one workgroup = sum_{K = I .. J} RW_IK RC_KJ; zeros below the diagonal of the diagonal blocks
__global__ __launch_bounds__(1024) void rmul_wide_f64_kernel(double* r, size_t ldr, const double* __restrict__ rw, const double* __restrict__ rc, int n) {
	__shared__ double Xs[64 * 65], Ys[64 * 65];
	const int t = threadIdx.x, w = t >> 6, l = t & 63, ti = w >> 2, tj = w & 3, li = l & 15, lq = l >> 4;
	const int p = blockIdx.x;
	int J = 0;
	while ((J + 1) * (J + 2) / 2 <= p) J++;
	const int I = p - J * (J + 1) / 2;
	f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
	for (int K = I; K <= J; K++) {
		__syncthreads();
		wide_stage(Xs, rw + (size_t)wpair(I, K) * 4096);
		wide_stage(Ys, rc + (size_t)wpair(K, J) * 4096);
		__syncthreads();
		const f64x4 c = wide_prod<false>(Xs, Ys);
		acc += c;
	}
#pragma unroll
	for (int reg = 0; reg < 4; reg++) {
		const int i = 64 * I + 16 * ti + lq + 4 * reg, j = 64 * J + 16 * tj + li;
		if (i < n && j < n) r[(size_t)j * ldr + i] = (i <= j) ? acc[reg] : 0.0;
	}
}

}  // namespace tsqrmi

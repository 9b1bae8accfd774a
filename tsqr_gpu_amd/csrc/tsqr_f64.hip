// tsqr_f64.hip -- the device side of the double-precision entry (tsqr_mi_qr_f64): CholeskyQR sweeps on fp64 data, n <= 64.
// Included by tsqr_mi.hip after tsqr_kernels.hip, whose Gram reduction (gram_reduce1_kernel) and Cholesky body (chol_body16<double>)
// it reuses unchanged.
//   gram_f64_kernel   : per-workgroup partials of A^T A on v_mfma_f64_16x16x4_f64 -- gram_kernel's body (gram_body) with fp64 loads
//   chol_f64_kernel   : G -> R, Z = inverse(R) in fp64, the fp64 acceptance rule (CholArgs64), a rejected matrix factored again at
//                       once with the shift of Fukaya et al.
//   apply_f64_kernel  : Q = A Z on v_mfma_f64_16x16x4_f64, Z upper triangular (its zero blocks are skipped), in place allowed
//   trimul_f64_kernel : D = L R of two upper triangular factors on v_mfma_f64_16x16x4_f64, in place: R <- R2 R
// and of the R-only entry (tsqr_mi_r_f64), whose sweeps after the first stream A and never store Q:
//   gramq_f64_kernel  : per-workgroup partials of (A Z)^T (A Z), each 16-row block of A Z formed and consumed in registers
//   trimul_f64_kernel : Z <- Z Zk, the inverse of all sweeps so far, in place
// and of the least-squares entry (tsqr_mi_lstsq_f64), whose passes behind that ladder stream A and B and store nothing of size m:
//   lsq_f64_kernel        : per-workgroup partials of (A Z)^T (B - A X), each 16-row block of A Z and of the residual held in registers
//   lsq_update_f64_kernel : X <- X + Z D on one workgroup
// and of the SVD entry (tsqr_mi_svd_f64), behind the ladder of either entry above:
//   svd_r_f64_kernel  : R = W diag(s) V^T by one-sided Jacobi on one workgroup, R held in LDS
//   applyd_f64_kernel : U = Q W on v_mfma_f64_16x16x4_f64 for a dense W staged in LDS, in place allowed
// and of the pivoted QR entry (tsqr_mi_qrcp_f64), behind the same ladders and in front of applyd_f64_kernel:
//   qrcp_r_f64_kernel : R0 P = H R by Householder QR with column pivoting on one workgroup, R0 and H^T held in LDS
// The four passes that read A (and B) take the layout of each operand as a template flag (AROW, BROW: tsqr_mi_r_f64_lay,
// tsqr_mi_lstsq_f64_lay, tsqr_mi_qr_f64_lay).  Element (i, j) of a row-major operand lies at s[i * ld + j], ld >= the column count.  A
// row-major kernel is the column-major one with another address for the same register: at every MFMA lane (li, lq) of k-block kb holds
// S[row0 + li][4 kb + lq] in both, so every partial -- and behind the unchanged reduction R, X and the sweep count -- has the bits of the
// column-major kernel on the transposed copy.  The apply pass also takes the layout of the operand it WRITES (QROW, tsqr_mi_qr_f64_lay):
// that one swaps the MFMA operands, which changes no bit either (apply_f64_kernel says why).
#include <hip/hip_runtime.h>

namespace tsqrmi {

struct GramArgs64 {
	const double* a; size_t lda; size_t m; int n;
	int nchunks; int nwaves;
	double* part;                        // [gridDim.x][NTRI][256], the order of gram_kernel's partials
};

// AROW: A is row-major (a.lda: the row stride, >= n): load_chunk_f64_rm fills the registers load_chunk_f64 fills
template <int NT, bool AROW>
__global__ __launch_bounds__(256) void gram_f64_kernel(const GramArgs64 a) {
	constexpr int NTRI = (NT * (NT + 1)) / 2;
	__shared__ double red[2 * NTRI * 256];
	gram_body<NT, double, AROW>(a, red);
}

// The three numbers of the acceptance rule (stated at CholArgs64 below) for a sweep over `rows` x n (first: the first sweep of a call).
// ONE definition for the host (f64_rule, f64_plan.h: a one-GPU call knows its rows) and for the device (a row-partitioned call: only
// the device sees the all-reduced row count).
// Both give the same bits: rows n and n (n + 1) are exact integers below 2^53 (rows n <= 2^26 by contract, n <= 1024), so their sum is
// exact whether or not the compiler contracts it into an FMA; everything after it is a product -- one rounding each, no addition to
// contract with -- and one IEEE division, correctly rounded on both sides (no fast-math), then one conversion to float.
struct F64Rule { double shift_coef; float max_scond, alone_max; };
__host__ __device__ inline F64Rule f64_rule_of(double rows, int n, bool first) {
	F64Rule r{};
	const double u = 0x1p-53, mn = rows * (double)n + (double)n * (double)(n + 1);
	r.shift_coef = 11.0 * u * mn;
	r.max_scond = first ? (float)(1.0 / (64.0 * (double)n * u * mn)) : INFINITY;
	r.alone_max = first ? (float)(1e-12 / (4.0 * (double)n * u)) : 0.0f;
	return r;
}

// The Cholesky step of the fp64 entry: chol_body16 with fp64 R and Z.  Level 4 of the ladder ("fp64 data"): the rule is stated on the
// scaled conditioning S = ||D inverse(R)||_F^2 / n (D = diag(sqrt(g_jj)); chol_body16), with u = 2^-53 and rows = m:
//   accepted for CholeskyQR2   every pivot positive and finite, and  64 n S u (m n + n (n + 1)) <= 1.  Yamamoto, Nakatsukasa, Yanagisawa
//                              and Fukaya, "Roundoff error analysis of the CholeskyQR2 algorithm", ETNA 44 (2015): CholeskyQR2 gives
//                              O(u) orthogonality when 8 kappa sqrt(m n u + n (n + 1) u) <= 1.  The Gram error of column-scaled data
//                              is relative to the column norms, so kappa^2 is taken as ||(A D^-1)^+||_2^2 <= n S;
//   accepted ALONE (one sweep) additionally when  4 n S u <= 1e-12: the estimated ||Q^T Q - I||_F of one CholeskyQR sweep, the rounding
//                              of G (a few u relative to the column norms, per entry) carried through inverse(R) twice;
//   rejected                   otherwise: the same launch factors G + s I, s = 11 (m n + n (n + 1)) u trace(G) (Fukaya, Kannan,
//                              Nakatsukasa, Yamamoto and Yanagisawa, "Shifted Cholesky QR for computing the QR factorization of
//                              ill-conditioned matrices", SISC 42 (2020)), accepted whenever every pivot is positive: two more sweeps
//                              follow (shifted CholeskyQR3).  Rejected even so: non-finite input, or a Gram matrix outside the normal range.
//   the range                  both factorisations also require every diagonal entry of the matrix they factor (G, or G + s I) to be a NORMAL
//                              fp64 number (F64_MIN_DIAG = 2^-1022; chol_body16's min_diag).  Below it the entries of G are subnormal: they
//                              carry an absolute error of 2^-1075 instead of a relative one, nothing in the rule sees that, and the call
//                              returned 0 with ||Q^T Q - I||_F beyond the header's band (2^-520 times a 4097 x 64 Gaussian matrix: 1.8e-11
//                              after one sweep).  With g_jj >= 2^-1022 a product that underflows costs at most 2^-1075 <= u g_jj, one
//                              more rounding error of the size the rule already budgets per term.  An overflowing G needs no rule of its
//                              own: Inf and NaN fail every comparison of the verdict.
//   the pivot floor            the plain factorisation of EVERY sweep also requires the smallest pivot ratio r_jj^2 / g_jj -- the squared sine of
//                              the angle between column j and the columns before it -- to exceed F64_MIN_PIVOT_RATIO = 2^-40, the bound this
//                              library already uses for "beyond fp64 Cholesky" (chol_body16, the fp64 Gram level of the fp32 ladder); it
//                              does not depend on the shape.  A pivot is a difference g_jj - sum r_kj^2 of j + 1 rounded terms, each
//                              carrying the rounding of its Gram entries: one that small next to g_jj is mostly rounding error.
//                              Why it is needed: with exactly dependent columns in A, Q of the shifted sweep is rank deficient up to
//                              rounding and the pivot of the dependent column in the next sweep is noise (ratios of 1e-16 .. 5e-15 in a
//                              numpy model of the ladder on the cases of tests/test_gpu_f64_scale.py).  Negative noise was always
//                              shifted again; positive noise was accepted, R of that sweep had a condition number near 1 / u and
//                              Q <- Q inverse(R) lost ||A - Q R||_F / ||A||_F = 6e-10.  A first sweep does not notice the floor:
//                              S >= 1 / (n ratio), so its bound on S already implies ratio >= 64 u (m n + n (n + 1)), and that
//                              exceeds 2^-40 from m n = 128 up.  Later sweeps of in-contract input
//                              meet it only at the far end: the sweep after the shift on cond(A) = 1e12 has ratios around 1e-12 .. 1e-14
//                              and may be shifted once more (profiles/fp64_scale_tests.md has the sweep counts measured at 2^20 and
//                              2^23 rows); cond(A) <= 1e10 stays where it was.
// Sweeps after the first pass alone_max = max_scond = infinity: their input is Q of a sweep before, and only a breakdown or a pivot
// under the floor sends them to the shift.
constexpr float F64_MIN_PIVOT_RATIO = 0x1p-40f;
constexpr double F64_MIN_DIAG = 0x1p-1022;              // the smallest normal fp64 number
struct CholArgs64 {
	double* r; size_t ldr;               // R out: n x n, full block written (zeros below the diagonal)
	double* z;                           // Z = inverse(R) out: NP x NP column-major (ld NP), zero padded
	unsigned* status;                    // device words [0] verdict, [1] min pivot ratio (float bits), [2] S (float bits), [3] one sweep suffices
	unsigned* host_status;               // device-visible alias of pinned host words receiving the same four values at the end of the launch
	const double* gsum;                  // summed Gram tiles, fp64 accumulator order (gram_f64_kernel + gram_reduce1_kernel)
	double shift_coef;                   // 11 u (m n + n (n + 1)): s = shift_coef * trace(G)
	float max_scond;                     // CholeskyQR2 bound on S (above)
	float alone_max;                     // one-sweep bound on S (above); 0: never alone
	int n, NT;
	const double* rows_dev;              // row-partitioned call: the all-reduced (global) row count behind the summed tiles; the three numbers
	int first;                           // above are then f64_rule_of(rows_dev[0], n, first) and the arguments are not looked at.  Null: one GPU
};
// verdict words: 0 accepted, 2 accepted after the shift, 1 rejected (non-finite input)
__global__ __launch_bounds__(1024) void chol_f64_kernel(const CholArgs64 a) {
	auto loadg = [&](int e) { return a.gsum[e]; };
	F64Rule rule{a.shift_coef, a.max_scond, a.alone_max};
	if (a.rows_dev) rule = f64_rule_of(a.rows_dev[0], a.n, a.first != 0);     // (uniform: every thread reads the same word)
	chol_body16(a.r, a.ldr, a.z, a.status, nullptr, loadg, a.n, a.NT, 0, F64_MIN_PIVOT_RATIO, rule.max_scond, 0.0, F64_MIN_DIAG);
	__shared__ unsigned again;
	__syncthreads();
	if (threadIdx.x == 0) {                              // (thread 0 wrote the verdict itself: program order)
		again = a.status[0];
		a.status[3] = (a.status[0] == 0u && __builtin_bit_cast(float, a.status[2]) <= rule.alone_max) ? 1u : 0u;
	}
	__syncthreads();
	if (again) {
		chol_body16(a.r, a.ldr, a.z, a.status, nullptr, loadg, a.n, a.NT, 0, 0.0f, INFINITY, rule.shift_coef, F64_MIN_DIAG);
		__syncthreads();
		if (threadIdx.x == 0) {
			if (a.status[0] == 0u) a.status[0] = 2u;
			a.status[3] = 0u;
		}
	}
	if (threadIdx.x == 0) {
		volatile unsigned* hs = a.host_status;
		hs[1] = a.status[1];
		hs[2] = a.status[2];
		hs[3] = a.status[3];
		hs[0] = a.status[0];
	}
}

// v[kb] = S[row][4 kb + lq] for kb < KB from a ROW-major S (ld: the row stride), the registers the column-major loops of apply_f64_kernel,
// gramq_f64_kernel and lsq_f64_kernel fill; zero where the row is not live or the column is >= n (neither is read).
// The direct address: one load instruction reads sixteen 32-byte pieces, one per row, and the four k-blocks 4 g .. 4 g + 3 together use
// every byte of the 128-byte lines they touch.  Measured against wide loads with a 4 x 4 exchange between the four lane quarters
// (v_permlane32_swap, v_permlane16_swap), which was slower: DESIGN.md section 9 has both figures.
template <int KB>
__device__ __forceinline__ void load_rows_rm(double (&v)[KB], const double* __restrict__ s, size_t ld, size_t row, bool live, int n, int lq) {
#pragma unroll
	for (int kb = 0; kb < KB; kb++) {
		const int col = 4 * kb + lq;
		v[kb] = (live && col < n) ? s[row * ld + col] : 0.0;
	}
}

// Q = A Z, Z (ld NP) upper triangular.  Each wave owns 32-row blocks (two 16-row tiles; a persistent grid strides over them).  Both
// register sets are the same for every layout: zop, lane (li, lq) holds Z[4 kb + lq][16 jt + li]; av, lane (li, lq) holds
// A[row0 + li][4 kb + lq].  AROW: A is row-major (lda: the row stride, >= n) -- load_rows_rm fills the registers the column-major loop
// fills.  QROW: Q is row-major (ldq: the row stride, >= n).  The layout of Q picks the ORDER of the MFMA operands, so that every store
// moves whole 128-byte segments:
//   column-major Q  D[j][r] = sum_k Z[k][j] A[r][k]: operand A is Z^T, operand B is A^T, and the C/D layout (col = lane & 15,
//                   row = (lane >> 4) + 4 reg) puts sixteen consecutive ROWS of one column of Q in sixteen lanes;
//   row-major Q     D[r][j] = sum_k A[r][k] Z[k][j], the operands swapped (gramq_f64_kernel's first stage): register reg of lane
//                   (li, lq) holds Q[row0 + lq + 4 reg][16 jt + li], sixteen consecutive COLUMNS of one row in sixteen lanes, and one
//                   store instruction writes four 128-byte row segments.
// Either order forms, for every entry of Q, the accumulator plus the same four products k = 0 .. 3 of the same k-block -- the swap
// transposes the tile and exchanges the factors of each product, and IEEE multiplication is commutative -- so Q has the same bits for
// all four layout pairs (tests/test_gpu_f64_apply_rowmajor_passes.py compares them on the device).
// Output tile jt needs k < 16 (jt + 1) only: 2 NT (NT + 1) k-blocks of Z instead of 4 NT^2, held in registers for the whole kernel.
// In place (q == a, the same layout, ldq == lda) is safe: a wave reads all n columns of its rows before it writes any of them (every
// stored block depends on the loads of its own rows and columns), no two waves share a row, and rows of a row-major operand with
// ld >= n do not overlap.  Nothing at a row >= m or at a column between n and the leading dimension is read or written.
template <int NT, bool AROW, bool QROW>
__global__ __launch_bounds__(256) void apply_f64_kernel(double* q, size_t ldq, const double* a, size_t lda, size_t m, int n,
                                                        const double* __restrict__ z, size_t nblocks) {
	constexpr int NP = 16 * NT, KB = 4 * NT, NZ = 2 * NT * (NT + 1);
	const int lane = threadIdx.x & 63, li = lane & 15, lq = lane >> 4;
	const size_t gw = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (size_t)gridDim.x * 4;
	double zop[NZ];
	static_for<0, NT>([&](auto jt_) {
		constexpr int jt = decltype(jt_)::value, base = 2 * jt * (jt + 1);
#pragma unroll
		for (int kb = 0; kb < 4 * (jt + 1); kb++) zop[base + kb] = z[(size_t)(16 * jt + li) * NP + 4 * kb + lq];
	});
	for (size_t blk = gw; blk < nblocks; blk += nw) {
		const size_t row0 = blk * 32;
		double av[2][KB];
#pragma unroll
		for (int rt = 0; rt < 2; rt++) {
			const size_t row = row0 + 16 * rt + li;
			if constexpr (AROW) load_rows_rm<KB>(av[rt], a, lda, row, row < m, n, lq);
			else {
#pragma unroll
				for (int kb = 0; kb < KB; kb++) {
					const int col = 4 * kb + lq;
					av[rt][kb] = (row < m && col < n) ? a[(size_t)col * lda + row] : 0.0;
				}
			}
		}
		f64x4 acc[2][NT];
		static_for<0, NT>([&](auto jt_) {
			constexpr int jt = decltype(jt_)::value, base = 2 * jt * (jt + 1);
#pragma unroll
			for (int rt = 0; rt < 2; rt++) {
				acc[rt][jt] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
				for (int kb = 0; kb < 4 * (jt + 1); kb++) {
					if constexpr (QROW) acc[rt][jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[rt][kb], zop[base + kb], acc[rt][jt], 0, 0, 0);
					else acc[rt][jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(zop[base + kb], av[rt][kb], acc[rt][jt], 0, 0, 0);
				}
			}
		});
#pragma unroll
		for (int rt = 0; rt < 2; rt++) {
#pragma unroll
			for (int jt = 0; jt < NT; jt++)
#pragma unroll
				for (int reg = 0; reg < 4; reg++) {
					if constexpr (QROW) {
						const size_t row = row0 + 16 * rt + lq + 4 * reg;
						const int col = 16 * jt + li;
						if (row < m && col < n) q[row * ldq + col] = acc[rt][jt][reg];
					} else {
						const size_t row = row0 + 16 * rt + li;
						const int col = 16 * jt + lq + 4 * reg;
						if (row < m && col < n) q[(size_t)col * ldq + row] = acc[rt][jt][reg];
					}
				}
		}
	}
}

// D = L R, the product of two n x n upper triangular factors (n <= 64; column-major with ldl, ldr), written as the leading ext x ext block
// of d (ldd; zeros below the diagonal and beyond n), in place: d may be either factor.  Its two uses:
//   R <- R2 R   d = R, the right factor (its ld); L = R2 packed with ld 64; ext = n
//   Z <- Z Zk   d = Z, the left factor; both NP x NP with ld NP, zero padded, the layout of chol_f64_kernel's Z; ext = NP, the whole block
// One workgroup of sixteen waves stages both factors in LDS, wave w forms the 16 x 16 tile (w >> 2, w & 3) over the k range in which both
// are non-zero (rmul64_kernel's scheme with fp64 I/O).  Every thread has read its entries before the barrier that precedes the first store.
__global__ __launch_bounds__(1024) void trimul_f64_kernel(double* d, size_t ldd, const double* l, size_t ldl, const double* r, size_t ldr,
                                                          int n, int ext) {
	__shared__ double A2[64 * 65], A1[64 * 65];          // A2[i * 65 + k] = L[i][k], A1[k * 65 + j] = R[k][j]; zero outside the upper triangles
	const int t = threadIdx.x;
#pragma unroll
	for (int u = 0; u < 4; u++) {
		const int e = t + 1024 * u, i = e & 63, j = e >> 6;
		const bool in = i <= j && j < n;
		A2[i * 65 + j] = in ? l[(size_t)j * ldl + i] : 0.0;
		A1[i * 65 + j] = in ? r[(size_t)j * ldr + i] : 0.0;
	}
	__syncthreads();
	const int w = t >> 6, ln = t & 63, ti = w >> 2, tj = w & 3, li = ln & 15, lq = ln >> 4;
	f64x4 c = f64x4{0.0, 0.0, 0.0, 0.0};                // c[reg] = (L R)[16 ti + lq + 4 reg][16 tj + li]
	if (ti <= tj) {
		for (int ks = 4 * ti; ks < 4 * (tj + 1); ks++)
			c = __builtin_amdgcn_mfma_f64_16x16x4f64(A2[(16 * ti + li) * 65 + 4 * ks + lq], A1[(4 * ks + lq) * 65 + 16 * tj + li], c, 0, 0, 0);
	}
#pragma unroll
	for (int reg = 0; reg < 4; reg++) {
		const int i = 16 * ti + lq + 4 * reg, j = 16 * tj + li;
		if (i < ext && j < ext) d[(size_t)j * ldd + i] = (i <= j) ? c[reg] : 0.0;
	}
}

// ---- the R-only entry (tsqr_mi_r_f64): sweeps after the first never store Q --------------------------------------------------------
struct GramQArgs64 {
	const double* a; size_t lda; size_t m; int n;
	int ntiles; int nwaves;              // 16-row tiles of A; waves that take tiles (wave w: tiles w, w + nwaves, ...)
	const double* z;                     // NP x NP (ld NP) upper triangular, zero padded: chol_f64_kernel's Z or a product of such
	double* part;                        // [gridDim.x][NTRI][256], gram_f64_kernel's partials
};

// Per-workgroup partials of (A Z)^T (A Z) without storing A Z.  A wave takes 16-row tiles of A.  apply_f64_kernel's register contents
// (zop: lane (li, lq) holds Z[4 kb + lq][16 jt + li]; av: lane (li, lq) holds A[row0 + li][4 kb + lq]) with the MFMA operands SWAPPED:
// D[r][j] = sum_k A[row0 + r][k] Z[k][16 jt + j], so the C/D layout (col = lane & 15, row = (lane >> 4) + 4 reg) leaves
// Q[row0 + lq + 4 reg][16 jt + li] in register reg of lane (li, lq) -- the operand form of the Gram MFMA (gram_body: sixteen lanes hold
// sixteen COLUMNS of one row, the lane quarter picks the row of the K-step).  Register reg of tiles ti and tj then feed
// G(ti, tj) += Q_reg(ti)^T Q_reg(tj) directly: K-step reg sums the rows row0 + 4 reg + {0, 1, 2, 3} -- both operands come from the same
// lane and register, so they name the same row.  No LDS transpose, no store; output tile jt needs k < 16 (jt + 1) only, as in the apply
// pass.  Rows >= m and columns >= n enter as zeros.  The partials leave in gram_f64_kernel's layout (wg_sum4_store).
// AROW: A is row-major (a.lda: the row stride).
template <int NT, bool AROW>
__global__ __launch_bounds__(256) void gramq_f64_kernel(const GramQArgs64 a) {
	constexpr int NP = 16 * NT, KB = 4 * NT, NZ = 2 * NT * (NT + 1), NTRI = (NT * (NT + 1)) / 2;
	__shared__ double red[2 * NTRI * 256];
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, lq = lane >> 4;
	const int gw = blockIdx.x * 4 + wv;
	f64x4 acc[NTRI];
#pragma unroll
	for (int t = 0; t < NTRI; t++) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
	if (gw < a.nwaves) {
		double zop[NZ];
		static_for<0, NT>([&](auto jt_) {
			constexpr int jt = decltype(jt_)::value, base = 2 * jt * (jt + 1);
#pragma unroll
			for (int kb = 0; kb < 4 * (jt + 1); kb++) zop[base + kb] = a.z[(size_t)(16 * jt + li) * NP + 4 * kb + lq];
		});
		// av of the tile after this one is loaded before this one's products are issued (one wave per SIMD: nothing else hides the loads);
		// a tile beyond the last reads nothing and leaves zeros
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
			static_for<0, NT>([&](auto jt_) {
				constexpr int jt = decltype(jt_)::value, base = 2 * jt * (jt + 1);
				qt[jt] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
				for (int kb = 0; kb < 4 * (jt + 1); kb++)
					qt[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[kb], zop[base + kb], qt[jt], 0, 0, 0);
			});
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

// ---- the least-squares entry (tsqr_mi_lstsq_f64): passes over A and B behind the R-only ladder ----------------------------------------
struct LsqArgs64 {
	const double* a; size_t lda;
	const double* b; size_t ldb;         // m x nrhs right-hand sides
	size_t m; int n; int nrhs;
	int ntiles; int nwaves;              // 16-row tiles of A and B; waves that take tiles (wave w: tiles w, w + nwaves, ...)
	const double* z;                     // NP x NP (ld NP) upper triangular, zero padded: the inverse of R
	const double* x;                     // n x 16 (ld NP) current solution; may be null = zero
	double* part;                        // [gridDim.x][NT][256]: tile ti of a partial holds rows 16 ti .. 16 ti + 15 of D
};

// Per-workgroup partials of D = (A Z)^T (B - A X), NP x 16, without storing A Z or the residual.  The tile loop, the loads of av, the
// prefetch and zop are gramq_f64_kernel's.  Per 16-row tile:
//   1  qt[jt] = A_tile Z, gramq_f64_kernel's first stage: register reg of lane (li, lq) holds Q~[row0 + lq + 4 reg][16 jt + li].
//   2  rt = B_tile - A_tile X in the same C/D layout: register reg of lane (li, lq) holds the residual of row row0 + lq + 4 reg and
//      right-hand side li.  B enters through four k-blocks against an identity operand built on the fly (lane (li, lq) of k-block kb holds
//      [4 kb + lq == li]): B is then loaded exactly like A -- lane (li, lq) holds B[row0 + li][4 kb + lq], whole 128-byte column segments,
//      the same bounds logic, prefetched with the next tile of A -- where the C/D layout itself would take four loads of sixteen 32-byte
//      pieces each.  The price is 4 MFMAs of 76 at NT = 4, and that 0 * B[row][j] enters every right-hand side of that row: ONE non-finite
//      entry of B makes row `row` of the residual non-finite for ALL right-hand sides, hence every column of X (include/tsqr_mi.h says
//      so).  For finite B the four k-blocks give B exactly (b * 1 + zeros).  Then 4 NT k-blocks of av against xop, lane (li, lq) of
//      k-block kb holding -X[4 kb + lq][li] (x null: -0).
//   3  acc[ti] += qt[ti][reg]^T rt[reg] for reg 0 .. 3: the Gram MFMA of gramq_f64_kernel with rt as its second operand -- both come from
//      the same lane and register, so they name the same row.  Register reg of lane (li, lq) of acc[ti] holds D[16 ti + lq + 4 reg][li].
// Rows >= m, columns >= n and right-hand sides >= nrhs enter as zeros.  A partial is NT tiles of 256 doubles (wg_sum4_store).
// AROW: A is row-major (a.lda: the row stride); BROW: B is row-major (a.ldb: the row stride).  A row-major B still enters through the
// identity k-blocks: the products, and the rule that one non-finite entry of B spoils its row, do not depend on the layout.
template <int NT, bool AROW, bool BROW>
__global__ __launch_bounds__(256) void lsq_f64_kernel(const LsqArgs64 a) {
	constexpr int NP = 16 * NT, KB = 4 * NT, NZ = 2 * NT * (NT + 1);
	__shared__ double red[2 * NT * 256];
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, lq = lane >> 4;
	const int gw = blockIdx.x * 4 + wv;
	f64x4 acc[NT];
#pragma unroll
	for (int t = 0; t < NT; t++) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
	if (gw < a.nwaves) {
		double zop[NZ], xop[KB], idop[4];
		static_for<0, NT>([&](auto jt_) {
			constexpr int jt = decltype(jt_)::value, base = 2 * jt * (jt + 1);
#pragma unroll
			for (int kb = 0; kb < 4 * (jt + 1); kb++) zop[base + kb] = a.z[(size_t)(16 * jt + li) * NP + 4 * kb + lq];
		});
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
			static_for<0, NT>([&](auto jt_) {
				constexpr int jt = decltype(jt_)::value, base = 2 * jt * (jt + 1);
				qt[jt] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
				for (int kb = 0; kb < 4 * (jt + 1); kb++)
					qt[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[kb], zop[base + kb], qt[jt], 0, 0, 0);
			});
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

// X <- X + Z D on one workgroup (n <= 64 rows by 16 right-hand sides: not on the hot path, plain fp64).  xw: the work copy, NP x 16
// (ld NP), wholly written -- zeros in rows >= n and right-hand sides >= nrhs; first: X is taken as zero and xw is not read.  d: the summed
// partials of lsq_f64_kernel, D[k][j] at ((k >> 4) * 4 + ((k & 15) >> 2)) * 64 + (k & 3) * 16 + j.  Z upper triangular: row i sums
// k = i .. n - 1, in that order, one fused multiply-add each, so the bits do not depend on how the compiler contracts.  last: the result
// also goes to the caller's x (n x nrhs, ldx).  Thread (i, j) reads and writes no entry of X but its own.
// dprev (16 doubles, or null: every update is applied): the stagnation rule of the refinement, one right-hand side at a time.  dprev[j]
// holds max_k |D[k][j]| of the pass before, or -1 once right-hand side j has stopped.  With guard set (the entry sets it from the
// second correction on) an update whose max_k |D[k][j]| is above half of the one before is NOT applied and right-hand side j stops for
// the rest of the call: past convergence a correction is the rounding noise of its own pass, and applying it only redraws the error of
// X.  D = Q~^T (B - A X) is the correction measured in Q-space: it keeps its bits under a column scaling of A and scales exactly with
// column j of B, so the verdict is the same for A diag(2^k_c), B diag(2^j_c).  A NaN in D is skipped by the maximum, +Inf compares as
// not above +Inf: non-finite data are applied as before.
// ZDENSE (the rank-aware solve, lsq_rank_f64.hip; the library instantiates the flag clear only): Z is dense, zero padded; row i sums k = 0 .. NP - 1, in
// that order, one fused multiply-add each -- D is zero in rows >= n -- under the same stagnation rule.
template <bool ZDENSE = false>
__global__ __launch_bounds__(1024) void lsq_update_f64_kernel(double* xw, double* x, size_t ldx, const double* __restrict__ z,
                                                              const double* __restrict__ d, int n, int NP, int nrhs, int first, int last,
                                                              double* dprev, int guard) {
	const int i = threadIdx.x & 63, j = threadIdx.x >> 6;
	bool apply = true;
	if (dprev) {                                          // (uniform over the workgroup: every thread reaches the barrier)
		double dm = 0.0;
		if (j < nrhs)
			for (int k = 0; k < n; k++) dm = fmax(dm, fabs(d[((k >> 4) * 4 + ((k & 15) >> 2)) * 64 + (k & 3) * 16 + j]));
		const double pv = dprev[j];
		if (guard) apply = pv >= 0.0 && !(dm > 0.5 * pv);
		__syncthreads();                                  // every thread of right-hand side j has read dprev[j]
		if (i == 0) dprev[j] = apply ? dm : -1.0;
	}
	if (i >= NP) return;
	double v = 0.0;
	if (i < n && j < nrhs) {
		double s = 0.0;
		if (apply)
			for (int k = ZDENSE ? 0 : i; k < (ZDENSE ? NP : n); k++)
				s = __builtin_fma(z[(size_t)k * NP + i], d[((k >> 4) * 4 + ((k & 15) >> 2)) * 64 + (k & 3) * 16 + j], s);
		v = apply ? (first ? 0.0 : xw[(size_t)j * NP + i]) + s : xw[(size_t)j * NP + i];
		if (last) x[(size_t)j * ldx + i] = v;
	}
	xw[(size_t)j * NP + i] = v;
}

// ---- the SVD entry (tsqr_mi_svd_f64): R = W diag(s) V^T on one workgroup, then U = Q W ----------------------------------------------------
struct SvdArgs64 {
	const double* r; size_t ldr;         // n x n upper triangular (only i <= j is read)
	double* s;                           // n singular values out: descending, non-negative
	double* w;                           // NP x NP (ld NP) out, zero padded, chol_f64_kernel's layout of Z; null: not wanted
	double* v; size_t ldv;               // n x n out; null: not wanted
	unsigned* status;                    // device words [0] sweeps, [1] 0 converged / 1 the cap was reached; null: not wanted
	unsigned* host_status;               // device-visible alias of pinned host words receiving the same two values; null: not wanted
	int n;
	int transpose;                       // 0: the columns of R rotate (W: normalised columns, V: the rotations); 1: those of R^T (roles swapped)
};
constexpr int SVD_MAX_SWEEPS = 30;      // dgesvj's cap

// The sum of x over the 64 lanes, the same bits in every lane.  The butterfly alone does not give that: when x is a product the compiler
// may fuse it into the first addition, each lane then adds its own UNROUNDED product to its partner's rounded one, and the lanes end
// one ulp apart -- enough to give the rows of a column pair different rotations (clustered singular values turn one ulp of a_pp into
// a visible change of the angle; measured: 30 sweeps without convergence on the R of a Gaussian 4096 x 64 matrix).  So lane 0's sum is
// the sum, for every lane.
__device__ __forceinline__ double wave_sum_f64(double x) {
#pragma unroll
	for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
	return __shfl(x, 0, 64);
}

// One-sided (Hestenes) Jacobi on the n x n factor R, n <= 64, held in LDS: M = R (or R^T) and J = I, 64 x 64 column-major each; lane i of a
// wave holds row i of the two columns of a pair.  M is first scaled by the power of two that brings max |r_ij| into [1, 2) -- exact, and
// s is scaled back at the end -- so that the inner products stay in range for every column norm the ladder accepts, and a factor
// 2^k R gives the bits of R in W and V.  An odd n is padded with a column that never rotates.  Round-robin order (the circle method on
// NE = n rounded up to even players): NE - 1 steps of NE / 2 disjoint pairs, pair k of a step on wave k mod 16, one barrier per step.
// Pair (p, q), p < q: a_pp, a_qq, a_pq by wave reductions; skipped when |a_pq| <= sqrt(n) 2^-53 sqrt(a_pp) sqrt(a_qq) (dgesvj's
// criterion), else zeta = (a_qq - a_pp) / (2 a_pq), t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)), c = 1 / sqrt(1 + t^2), s = c t and
// (m_p, m_q) <- (c m_p - s m_q, s m_p + c m_q), the same for J.  A sweep without a rotation ends the iteration; SVD_MAX_SWEEPS is the cap.
// The computed c^2 + s^2 is 1 only to rounding and a column takes part in several hundred rotations, all of which scale m_j and j_j
// alike: the norms d_j = ||j_j||_2 drift from 1 by some 1e-14 at n = 64, and that drift -- not the angles -- is nearly all of
// ||J^T J - I||_F (kernel_model in tests/pass_refs_f64_svd.py, cond 1e6, n = 64: 1.34e-13, of which 1.9e-14 off the diagonal).  So the end divides it out:
// sigma_j = ||m_j||_2 / d_j, J <- J diag(d)^-1, X = the columns of M normalised by their own norms (a column of norm exactly zero --
// possible by underflow only: R of the ladder has a positive diagonal -- stays zero).  sigma is sorted descending (ties: the lower
// column first) with its columns, and (W, V) = (X, J), or (J, X) when transposed.
// Everything is a fixed function of the input: two runs give the same bits.  No scratch; 67 KB of LDS.
__global__ __launch_bounds__(1024) void svd_r_f64_kernel(const SvdArgs64 a) {
	__shared__ double M[64 * 64], J[64 * 64];
	__shared__ double sig[64], mnorm[64], jnorm[64], wmax[16];
	__shared__ int rank_of[64];
	__shared__ unsigned rotated;
	const int t = threadIdx.x, lane = t & 63, wv = t >> 6, n = a.n;
	const int NE = (n + 1) & ~1, NP = 16 * ((n + 15) / 16);
	double x[4], mx = 0.0;
#pragma unroll
	for (int u = 0; u < 4; u++) {
		const int e = t + 1024 * u, i = e & 63, j = e >> 6;
		x[u] = (i <= j && j < n) ? a.r[(size_t)j * a.ldr + i] : 0.0;
		mx = fmax(mx, fabs(x[u]));
	}
#pragma unroll
	for (int o = 32; o >= 1; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
	if (lane == 0) wmax[wv] = mx;
	__syncthreads();
#pragma unroll
	for (int k = 0; k < 16; k++) mx = fmax(mx, wmax[k]);
	const int ex = (mx > 0.0 && mx < INFINITY) ? ilogb(mx) : 0;     // 2^ex <= max |r_ij| < 2^(ex + 1)
#pragma unroll
	for (int u = 0; u < 4; u++) {
		const int e = t + 1024 * u, i = e & 63, j = e >> 6;
		M[a.transpose ? i * 64 + j : j * 64 + i] = scalbn(x[u], -ex);
		J[e] = (i == j && j < n) ? 1.0 : 0.0;
	}
	if (t == 0) rotated = 0u;
	__syncthreads();
	const double tol = sqrt((double)n) * 0x1p-53;
	const int npairs = NE / 2, nsteps = NE - 1;
	unsigned sweeps = 0, failed = 1;
	while (sweeps < (unsigned)SVD_MAX_SWEEPS) {
		for (int st = 0; st < nsteps; st++) {
			for (int k = wv; k < npairs; k += 16) {
				const int c0 = k == 0 ? st : (st + k) % nsteps, c1 = k == 0 ? NE - 1 : (st - k + nsteps) % nsteps;
				const int p = c0 < c1 ? c0 : c1, q = c0 < c1 ? c1 : c0;
				if (q >= n) continue;                        // (the padding column of an odd n)
				const double mp = M[p * 64 + lane], mq = M[q * 64 + lane];
				const double app = wave_sum_f64(mp * mp), aqq = wave_sum_f64(mq * mq), apq = wave_sum_f64(mp * mq);
				if (!(fabs(apq) > tol * (sqrt(app) * sqrt(aqq)))) continue;   // (uniform over the wave: every lane holds the same sums)
				const double zeta = (aqq - app) / (2.0 * apq);
				const double tt = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
				if (tt == 0.0) continue;                     // (zeta beyond the range: the rotation is the identity)
				const double c = 1.0 / sqrt(1.0 + tt * tt), s = c * tt;
				const double jp = J[p * 64 + lane], jq = J[q * 64 + lane];
				M[p * 64 + lane] = c * mp - s * mq;
				M[q * 64 + lane] = s * mp + c * mq;
				J[p * 64 + lane] = c * jp - s * jq;
				J[q * 64 + lane] = s * jp + c * jq;
				if (lane == 0) rotated = 1u;
			}
			__syncthreads();
		}
		sweeps++;
		const unsigned any = rotated;
		__syncthreads();                                     // every thread has read the flag of this sweep
		if (t == 0) rotated = 0u;
		__syncthreads();
		if (!any) { failed = 0; break; }
	}
	for (int j = wv; j < 64; j += 16) {
		const double mj = M[j * 64 + lane], jj = J[j * 64 + lane];
		const double ss = wave_sum_f64(mj * mj), dd = wave_sum_f64(jj * jj);
		if (lane == 0) { mnorm[j] = sqrt(ss); jnorm[j] = j < n ? sqrt(dd) : 1.0; sig[j] = sqrt(ss) / (j < n ? sqrt(dd) : 1.0); }
	}
	__syncthreads();
	if (t < n) {
		int before = 0;
		for (int k = 0; k < n; k++) before += (sig[k] > sig[t] || (sig[k] == sig[t] && k < t)) ? 1 : 0;
		rank_of[t] = before;
		a.s[before] = scalbn(sig[t], ex);
	}
	__syncthreads();
#pragma unroll
	for (int u = 0; u < 4; u++) {
		const int e = t + 1024 * u, i = e & 63, j = e >> 6;
		if (a.w && i < NP && j < NP && (i >= n || j >= n)) a.w[(size_t)j * NP + i] = 0.0;
		if (i < n && j < n) {
			const int d = rank_of[j];
			const double xn = mnorm[j] > 0.0 ? M[e] / mnorm[j] : 0.0, jv = J[e] / jnorm[j];
			if (a.w) a.w[(size_t)d * NP + i] = a.transpose ? jv : xn;
			if (a.v) a.v[(size_t)d * a.ldv + i] = a.transpose ? xn : jv;
		}
	}
	if (t == 0) {
		if (a.status) { a.status[0] = sweeps; a.status[1] = failed; }
		if (a.host_status) { volatile unsigned* hs = a.host_status; hs[1] = failed; hs[0] = sweeps; }
	}
}

// U = Q W for a dense W (NP x NP, ld NP, zero padded: svd_r_f64_kernel's): apply_f64_kernel's structure -- 32-row blocks per wave on a
// persistent grid; av, lane (li, lq) holds Q[row0 + li][4 kb + lq] for every layout (AROW: q is row-major, load_rows_rm; QROW: u is); the operand
// swap for a row-major result -- with all 4 NT k-blocks in every output tile.  The 4 NT^2 operands of W (lane (li, lq) of operand
// (jt, kb) holds W[4 kb + lq][16 jt + li]) would take 128 VGPRs at NT = 4, so they are staged in LDS once per workgroup, in operand
// order: operand (jt, kb) is 64 consecutive doubles, lane l reads element l -- one conflict-free 8-byte read feeds the MFMAs of both
// 16-row tiles.  Output tile jt is stored as soon as its KB products are summed: the registers are av (2 KB doubles) and two accumulators.
// Every entry of U is the accumulator plus the four products of k-blocks 0 .. KB - 1 in that order, the factors exchanged by the swap
// (IEEE multiplication is commutative): the same bits for all four layout pairs.
// In place (u == q, the same layout and leading dimension) is safe for apply_f64_kernel's reason: a wave loads all n columns of its 32
// rows before it stores any of them, and no two waves share a row.  Nothing at a row >= m or at a column between n and the leading
// dimension is read or written.
template <int NT, bool AROW, bool QROW>
__global__ __launch_bounds__(256) void applyd_f64_kernel(double* u, size_t ldu, const double* q, size_t ldq, size_t m, int n,
                                                         const double* __restrict__ w, size_t nblocks) {
	constexpr int NP = 16 * NT, KB = 4 * NT;
	__shared__ double wl[NT * KB * 64];
	for (int e = threadIdx.x; e < NT * KB * 64; e += 256) {
		const int l = e & 63, b = e >> 6, jt = b / KB, kb = b % KB;
		wl[e] = w[(size_t)(16 * jt + (l & 15)) * NP + 4 * kb + (l >> 4)];
	}
	__syncthreads();
	const int lane = threadIdx.x & 63, li = lane & 15, lq = lane >> 4;
	const size_t gw = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (size_t)gridDim.x * 4;
	for (size_t blk = gw; blk < nblocks; blk += nw) {
		const size_t row0 = blk * 32;
		double av[2][KB];
#pragma unroll
		for (int rt = 0; rt < 2; rt++) {
			const size_t row = row0 + 16 * rt + li;
			if constexpr (AROW) load_rows_rm<KB>(av[rt], q, ldq, row, row < m, n, lq);
			else {
#pragma unroll
				for (int kb = 0; kb < KB; kb++) {
					const int col = 4 * kb + lq;
					av[rt][kb] = (row < m && col < n) ? q[(size_t)col * ldq + row] : 0.0;
				}
			}
		}
#pragma unroll
		for (int jt = 0; jt < NT; jt++) {
			f64x4 acc[2] = {f64x4{0.0, 0.0, 0.0, 0.0}, f64x4{0.0, 0.0, 0.0, 0.0}};
#pragma unroll
			for (int kb = 0; kb < KB; kb++) {
				const double wop = wl[(jt * KB + kb) * 64 + lane];
#pragma unroll
				for (int rt = 0; rt < 2; rt++) {
					if constexpr (QROW) acc[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[rt][kb], wop, acc[rt], 0, 0, 0);
					else acc[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(wop, av[rt][kb], acc[rt], 0, 0, 0);
				}
			}
#pragma unroll
			for (int rt = 0; rt < 2; rt++)
#pragma unroll
				for (int reg = 0; reg < 4; reg++) {
					if constexpr (QROW) {
						const size_t row = row0 + 16 * rt + lq + 4 * reg;
						const int col = 16 * jt + li;
						if (row < m && col < n) u[row * ldu + col] = acc[rt][reg];
					} else {
						const size_t row = row0 + 16 * rt + li;
						const int col = 16 * jt + lq + 4 * reg;
						if (row < m && col < n) u[(size_t)col * ldu + row] = acc[rt][reg];
					}
				}
		}
	}
}

// ---- the pivoted QR entry (tsqr_mi_qrcp_f64): R0 P = H R on one workgroup, then Q = Q0 H (applyd_f64_kernel) ------------------------------
struct QrcpArgs64 {
	const double* r0; size_t ldr0;       // n x n upper triangular in (only i <= j is read)
	double* r; size_t ldr;               // n x n out: R, exact zeros below the diagonal; may be r0 itself (ldr == ldr0)
	int* jpvt;                           // n pivots out, 0-based: column j of R0 P is column jpvt[j] of R0
	double* h;                           // NP x NP (ld NP) out, zero padded, chol_f64_kernel's layout of Z; null: not wanted, not formed
	unsigned* status;                    // device words [0] steps taken (n), [1] steps whose pivot column was exactly zero; null: not wanted
	int n;
};

// Householder QR with column pivoting (Businger-Golub) of the n x n factor R0, n <= 64, held in LDS: M = R0 and G = I, 64 x 64
// column-major each; lane i of a wave holds row i of a column.  M is first scaled by the power of two that brings max |r_ij| into
// [1, 2) -- exact, R is scaled back at the end -- so that no square leaves the range for any R0 the ladder accepts, and 2^k R0 gives the
// bits of H and jpvt.  Step k = 0 .. n - 1, two barriers each:
//   pivot      nrm[j] = sum_{i >= k} m_ij^2 of every column j >= k, summed AFRESH from the entries as they stand (by the wave that last
//              wrote the column; never downdated, so dlaqp2's cancellation safeguard has nothing to guard); p = the largest, the lowest
//              index on a tie, found by every wave for itself from the same 64 numbers;
//   swap       whole columns k and p, the finished rows above k included, and the two entries of jpvt.  No copy: every wave reads
//              x = column p and y = column k before the barrier, and behind it column k is written from x and position p from y;
//   reflector  of x over rows k .. n - 1 as dlarfg builds it: alpha = x_k, s = sum_{i > k} x_i^2; s == 0: H_k = I (a zero column gives
//              R_kk = 0, nothing is divided); else beta = -sign(alpha) sqrt(alpha^2 + s), tau = (beta - alpha) / beta,
//              v = (1, x_{k+1..} / (alpha - beta)) -- every wave computes the same bits, every sum goes through wave_sum_f64;
//   apply      c <- c - tau v (v^T c) to the trailing columns of M and to all n columns of G, which so accumulates H^T by the same
//              column operation; the columns are dealt round-robin to the 16 waves, those of M first;
//   sign       beta < 0: row k of M and of G is negated (exact), so diag(R) >= 0.
// At the end R = M, H = G^T (transposed through M in a rotated image: no bank conflict).  No data-dependent iteration; everything is a fixed function of the input: two runs give the same bits.
// h == null (the R-only form): G is neither updated nor written.  Nothing is written to global memory before the end; r may be r0.
// No scratch; 66.4 KB of LDS.
__global__ __launch_bounds__(1024) void qrcp_r_f64_kernel(const QrcpArgs64 a) {
	__shared__ double M[64 * 64], G[64 * 64];
	__shared__ double nrm[64], wmax[16];
	__shared__ int piv[64];
	const int t = threadIdx.x, lane = t & 63, wv = t >> 6, n = a.n;
	const int NP = 16 * ((n + 15) / 16);
	double x0[4], mx = 0.0;
#pragma unroll
	for (int u = 0; u < 4; u++) {
		const int e = t + 1024 * u, i = e & 63, j = e >> 6;
		x0[u] = (i <= j && j < n) ? a.r0[(size_t)j * a.ldr0 + i] : 0.0;
		mx = fmax(mx, fabs(x0[u]));
	}
#pragma unroll
	for (int o = 32; o >= 1; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
	if (lane == 0) wmax[wv] = mx;
	__syncthreads();
#pragma unroll
	for (int k = 0; k < 16; k++) mx = fmax(mx, wmax[k]);
	const int ex = (mx > 0.0 && mx < INFINITY) ? ilogb(mx) : 0;     // 2^ex <= max |r_ij| < 2^(ex + 1)
#pragma unroll
	for (int u = 0; u < 4; u++) {
		const int e = t + 1024 * u, i = e & 63, j = e >> 6;
		M[e] = scalbn(x0[u], -ex);
		G[e] = (i == j && j < n) ? 1.0 : 0.0;
	}
	if (t < 64) piv[t] = t;
	__syncthreads();
	for (int j = wv; j < n; j += 16) {
		const double c = M[j * 64 + lane];
		const double s = wave_sum_f64(c * c);
		if (lane == 0) nrm[j] = s;
	}
	__syncthreads();
	unsigned zero_cols = 0;
	for (int k = 0; k < n; k++) {
		double bv = (lane >= k && lane < n) ? nrm[lane] : -1.0;
		int bi = lane;
#pragma unroll
		for (int o = 32; o >= 1; o >>= 1) {
			const double ov = __shfl_xor(bv, o, 64);
			const int oi = __shfl_xor(bi, o, 64);
			if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
		}
		int p = __shfl(bi, 0, 64);
		if (p < k || p >= n) p = k;                          // (only a NaN among the norms gets here: stay inside the matrix)
		const double x = M[p * 64 + lane], y = M[k * 64 + lane];
		const int jp = piv[p], jk = piv[k];
		__syncthreads();                                     // every wave holds the pivot, x and y: M, nrm and piv may be written
		if (t == 0) { piv[k] = jp; piv[p] = jk; }
		const double xr = (lane > k && lane < n) ? x : 0.0;
		const double alpha = __shfl(x, k, 64);
		const double s2 = wave_sum_f64(xr * xr);
		double tau = 0.0, beta = alpha, v = 0.0;
		if (s2 > 0.0) {
			beta = -copysign(sqrt(alpha * alpha + s2), alpha);
			tau = (beta - alpha) / beta;
			v = xr / (alpha - beta);
		} else if (alpha == 0.0) zero_cols++;
		if (lane == k) v = 1.0;
		const bool flip = beta < 0.0;
		const int ntrail = n - k - 1, ntask = ntrail + (a.h ? n : 0);
		for (int q = wv; q < ntask; q += 16) {
			const bool ism = q < ntrail;                     // (uniform over the wave)
			const int j = ism ? k + 1 + q : q - ntrail;
			double* col = (ism ? M : G) + j * 64;
			double c = (ism && j == p) ? y : col[lane];
			if (tau != 0.0) {
				const double d = wave_sum_f64(v * c);        // (v is zero above row k and from row n on)
				if (lane >= k) c -= (tau * d) * v;
			}
			if (flip && lane == k) c = -c;
			col[lane] = c;
			if (ism) {
				const double cr = lane > k ? c : 0.0;
				const double s = wave_sum_f64(cr * cr);
				if (lane == 0) nrm[j] = s;
			}
		}
		if (wv == (ntask & 15)) M[k * 64 + lane] = lane < k ? x : (lane == k ? fabs(beta) : 0.0);
		__syncthreads();
	}
#pragma unroll
	for (int u = 0; u < 4; u++) {
		const int e = t + 1024 * u, i = e & 63, j = e >> 6;
		if (i < n && j < n) a.r[(size_t)j * a.ldr + i] = i <= j ? scalbn(M[e], ex) : 0.0;
	}
	if (a.h) {                                               // (uniform over the workgroup)
		// H = G^T through M, which is free now: G(i, j) goes to row i of a row-major image whose rows are rotated by their index, so that
		// both the write (lane = i) and the read of a column of H (lane = i, row j of the image) touch 64 different addresses mod 64
		__syncthreads();
#pragma unroll
		for (int u = 0; u < 4; u++) {
			const int e = t + 1024 * u, i = e & 63, j = e >> 6;
			M[i * 64 + ((j + i) & 63)] = G[e];
		}
		__syncthreads();
#pragma unroll
		for (int u = 0; u < 4; u++) {
			const int e = t + 1024 * u, i = e & 63, j = e >> 6;
			if (i < NP && j < NP) a.h[(size_t)j * NP + i] = (i < n && j < n) ? M[j * 64 + ((i + j) & 63)] : 0.0;
		}
	}
	if (t < n) a.jpvt[t] = piv[t];
	if (t == 0 && a.status) { a.status[0] = (unsigned)n; a.status[1] = zero_cols; }
}

}  // namespace tsqrmi

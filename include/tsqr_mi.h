/*
 * tsqr_mi.h -- C ABI of the MI355X-native tall-skinny QR engine (libtsqr_mi.so).
 *
 * This is the drop-in boundary for the reference's hot path
 *     mtk::qr::qr<compute_mode, Reorthogonalize>() / mtk::qr::buffer
 * (reference src/blockqr.hpp:59-175, src/blockqr.cu:394-433).  The C++ templates in
 * include/tsqr/blockqr.hpp forward to these entry points; INTEGRATION.md shows the
 * binding a maintainer of the reference would add.
 *
 * Conventions (same as the reference): all matrices column-major; q, r, a and every work
 * buffer are DEVICE pointers owned by the caller (h_wl is pinned host memory); the call is
 * blocking -- it returns after the stream is idle (reference src/blockqr.cu:140); nothing
 * is allocated inside; `a` may be overwritten (it is for n > 64).
 * Re-entrant like the reference's entry point (src/blockqr.cu:394-433): a call keeps no state outside its arguments, so several
 * host threads may factor different matrices at the same time, each with its own buffers and stream (settings made with the
 * tsqr_mi_set_* calls are process-wide; tsqr_mi_last_error / tsqr_mi_last_engine / the event profile are per host thread).
 * h_wl: when it is pinned host memory of at least 8 words the engine writes its status words and completion flag there; a smaller
 * or pageable h_wl (e.g. sized with the reference's batch_size + 1 rule for m <= 128) is left untouched.
 */
#ifndef TSQR_MI_H
#define TSQR_MI_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* mtk::qr::compute_mode, same names and order as reference src/blockqr.hpp:12-23 */
enum tsqr_mi_compute_mode {
	TSQR_MI_FP16_NOTC = 0,         /* supported through tsqr_mi_qr_f16: fp16 in / out, fp32-accurate arithmetic in between (the fp32_tc_cor engines) */
	TSQR_MI_FP16_TC_NOCOR = 1,     /* supported through tsqr_mi_qr_f16: fp16 in / out, the single-fp16-product apply engine (fp32_tc_nocor's) */
	TSQR_MI_FP32_NOTC = 2,         /* supported: Q = A*inverse(R) on exact fp32 MFMA (v_mfma_f32_16x16x4_f32) */
	TSQR_MI_FP32_TC_COR = 3,       /* supported: Q = A*inverse(R) on bf16 MFMA with 3-way split error correction (six products) */
	TSQR_MI_FP32_TC_NOCOR = 4,     /* supported: R as fp32_tc_cor; Q = A*inverse(R) on fp16 MFMA, one product, no correction */
	TSQR_MI_MIXED_TC_COR_EMU = 5,
	TSQR_MI_TF32_TC_COR = 6,       /* no xf32 MFMA on gfx950: unsupported */
	TSQR_MI_TF32_TC_COR_EMU = 7,
	TSQR_MI_TF32_TC_NOCOR = 8,
	TSQR_MI_TF32_TC_NOCOR_EMU = 9
};

/* mtk::qr::state_t codes, reference src/blockqr.hpp:27-29, plus one new code */
#define TSQR_MI_SUCCESS               0   /* success_factorization */
#define TSQR_MI_ERROR_INVALID_SIZE    1   /* error_invalid_matrix_size: n > m, m == 0 or n == 0 */
#define TSQR_MI_ERROR_UNSUPPORTED     2   /* new: compute_mode without a gfx950 implementation */
#define TSQR_MI_ERROR_NOT_FINITE      3   /* new, the fp64 entries only: no factorisation inside the bands could be formed; Q and R are undefined.  A holds
                                           * an Inf or NaN; or A^T A leaves the normal fp64 range -- an entry overflows (a column norm of 2^512 or more), or
                                           * a squared column norm lies below 2^-1022 (a column norm below 2^-511, a zero matrix included); or A is rank
                                           * deficient in a way the shift cannot repair (an exactly zero column among non-zero ones: every sweep is shifted
                                           * again and the ladder ends at its cap).  On every rank alike for the row-partitioned entries.  Supported range of
                                           * column norms (the range is judged on the column norms of the sweep's input, the diagonal of its Gram matrix):
                                           * [2^-511, 2^512), and ||A||_F < 2^512 for input that takes the shifted path (its trace).  Inside
                                           * it, scaling the columns by powers of two changes no bit of Q (tests/test_gpu_f64_scale.py) */
#define TSQR_MI_ERROR_NO_CONVERGENCE  4   /* new, tsqr_mi_svd_f64 only: the Jacobi iteration reached its cap of 30 sweeps; s, v and u are undefined */
/* negative return values: -(hipError_t) of the failing runtime call */

int tsqr_mi_version(void);
const char* tsqr_mi_last_error(void);

/* replaces mtk::qr::get_working_{q,r,l}_size (reference src/blockqr.hpp:55-57, src/blockqr.cu:34-42).
 * Element counts (float / float / unsigned).  Never smaller than the reference's own formulas. */
size_t tsqr_mi_working_q_size(size_t m, size_t n);
size_t tsqr_mi_working_r_size(size_t m, size_t n);
size_t tsqr_mi_working_l_size(size_t m);
/* the reorthogonalisation scratch of mtk::qr::buffer::allocate (reference src/blockqr.hpp:91): 2*256 + 16 m floats */
size_t tsqr_mi_working_reorth_size(size_t m);
/* mtk::tsqr::get_batch_size_log2 / get_batch_size (reference src/tsqr.cu:39-44) */
size_t tsqr_mi_batch_size_log2(size_t m);
size_t tsqr_mi_batch_size(size_t m);

/*
 * replaces mtk::qr::qr<mode, Reorthogonalize>(q, ldq, r, ldr, a, lda, m, n, wq, wr, reorth_r, d_wl, h_wl, handle)
 * (reference src/blockqr.hpp:142-154).  `stream` is a hipStream_t (takes the place of the stream the
 * reference pulls out of its cublasHandle_t, src/blockqr.cu:58-59).  R: the full n x n upper triangle is
 * written and the strict lower triangle is set to exact zeros.
 * Orthogonality without reorthogonalisation (reorth = 0): one panel (n <= 64, or n <= 128 when the one-panel path accepts) loses
 * ||Q^T Q - I|| like cond(A) * eps32 at most; SEVERAL panels (n > 128, or 64 < n <= 128 on ill-conditioned input) are coupled by
 * block Gram-Schmidt as in the reference (src/blockqr.cu:45-178) and an ill-conditioned input loses orthogonality between the
 * panels -- the return code is still 0, exactly like the reference's.  Measured: 20000 x 128, cond 1e4: 5e-3 (the reference's
 * algorithm: 4.6); cond 1e7: 4.5 (reference: 15.8).  Pass reorth = 1 for O(eps32) at any conditioning up to ~1e8
 * (tests/test_gpu_wide.py, tests/test_gpu_parity.py state the bounds).
 */
int tsqr_mi_qr_f32(int mode, int reorth,
                   float* q, size_t ldq, float* r, size_t ldr, float* a, size_t lda,
                   size_t m, size_t n,
                   void* wq, void* wr, float* reorth_w, unsigned* d_wl, unsigned* h_wl,
                   void* stream);
/*
 * Stream-asynchronous form of tsqr_mi_qr_f32.  The reference's mtk::qr::qr only ENQUEUES on the handle's stream and returns
 * (reference src/blockqr.cu:395-449: kernel launches and cuBLAS calls, no synchronisation), so a caller's loop keeps the GPU busy
 * back to back (its speed protocol, src/test.cu:299-309, is such a loop).  tsqr_mi_qr_f32 blocks, because its state includes the
 * verdict of the conditioning check; the pair below gives the reference's overlap back:
 *   tsqr_mi_qr_f32_submit  enqueues the call's first attempt (bf16-split Gram level: Gram pass, Cholesky + verdict, apply pass that
 *                          skips itself on rejection, completion word) and returns;
 *   tsqr_mi_qr_f32_finish  waits for that call, and when the verdict was "rejected" runs the rest of the ladder for it (blocking),
 *                          exactly as tsqr_mi_qr_f32 would have; returns the call's state.
 * Up to TWO calls of a host thread are in flight (their verdict words alternate between the two halves of h_wl); a third submit
 * first waits for the oldest one's verdict.  Calls that have no speculative first attempt (reorth, n > 128, policy != auto,
 * profiling on, h_wl not pinned) are executed inside submit, blocking; finish then just returns their state.
 * Rules: a ticket lives until it is finished, by the thread that submitted it, tickets are finished in submission order; the
 * arguments (A, Q, R, work buffers) stay valid and unmodified by the host until then.  Two calls in flight may share the work
 * buffers (everything runs in stream order).  A call that CONFLICTS with a ticket of the thread not finished yet -- Q or R of the
 * earlier call overlaps Q, R or A of the new one, or Q or R of the new call overlaps A of the earlier one (byte ranges of
 * ((n - 1) ld + rows) elements) -- is not enqueued before it: submit finishes the open tickets up to that one first (their finish then
 * returns the state), so the pair gives what two blocking calls give.
 * Any other entry point of this library called by the thread meanwhile first waits for the verdicts of its tickets in flight.
 */
typedef struct tsqr_mi_ticket {
	int state;                      /* the call's state, valid after finish (or after a submit that ran the call itself) */
	int pending;                    /* 0 done, 1 first attempt in flight, 2 verdict read (ladder not yet run) */
	int slot;                       /* which half of the pinned words the attempt reports to */
	int own_flag;                   /* 1: a completion kernel of its own follows the attempt (always, for tsqr_mi_qr_f32_submit) */
	unsigned seq;                   /* sequence number its completion word will show */
	unsigned verdict;               /* 0 accepted / 1 rejected */
	float scond;                    /* scaled conditioning S the Cholesky kernel reported */
	int mode, reorth;
	float *q, *r, *a;
	size_t ldq, ldr, lda, m, n;
	void *wq, *wr, *stream;
	unsigned *h_wl, *words, *words_dev;   /* caller's pinned words; the pinned words actually used (host / device address) */
} tsqr_mi_ticket;
int tsqr_mi_qr_f32_submit(int mode, int reorth,
                          float* q, size_t ldq, float* r, size_t ldr, float* a, size_t lda,
                          size_t m, size_t n,
                          void* wq, void* wr, float* reorth_w, unsigned* d_wl, unsigned* h_wl,
                          void* stream, tsqr_mi_ticket* ticket);
int tsqr_mi_qr_f32_finish(tsqr_mi_ticket* ticket);

/* `count` calls of tsqr_mi_qr_f32 with the same arguments -- the loop of the reference's speed protocol (reference
 * src/test.cu:299-309) on this side of the ABI, so that a host in an interpreted language times what a C++ caller's loop costs.
 * The loop knows that another call follows and keeps the stream fed (tsqr_mi_set_loop_depth selects how far it goes):
 *   depth 1  plain blocking calls, one host round trip between two of them (the latency of a call);
 *   depth 2  two calls in flight: call i + 1 is submitted before call i is finished (submit / finish above); inside the loop the
 *            completion word of call i is raised by the first kernel of call i + 1 instead of a kernel of its own;
 *   depth 3  (default) depth 2, and for full 64-column matrices of 128 k <= 2^20 rows (16-byte aligned, no reorth) the chained
 *            schedule: the R-factor chain of call i (reduction of the Gram partials, Cholesky, verdict -- one workgroup busy, the
 *            rest of the chip idle) runs INSIDE the launch that is the Gram pass of call i + 1, so a call costs its two streaming
 *            passes and nothing else.  Needs count >= 3; wr holds two sets of Gram partials for it.  Likewise for 128 columns (m a
 *            multiple of 64, at least 510 blocks): the two-block factorisation of call i rides in the Gram launch of call i + 1.
 * At every depth every call runs all of its kernels, every verdict is read, a rejected matrix gets its whole ladder, and Q and R
 * are bit for bit those of the blocking call (tests/test_gpu_async.py).  Returns the first non-zero state.
 * The chained schedules launch the Gram pass of call i + 1 before the apply pass of call i; they are taken only when that is the
 * blocking order, i.e. when Q and R do not overlap A (a loop that factors in place, q == a, runs at depth 2: call i + 1 of the
 * blocking loop factors the Q that call i left in A, and so does the stream -- after a rejected call, call i + 1 is redone as a
 * blocking call). */
int tsqr_mi_qr_f32_loop(int count, int mode, int reorth,
                        float* q, size_t ldq, float* r, size_t ldr, float* a, size_t lda,
                        size_t m, size_t n,
                        void* wq, void* wr, float* reorth_w, unsigned* d_wl, unsigned* h_wl,
                        void* stream);
void tsqr_mi_set_loop_depth(int depth);   /* 1, 2 or 3 (default); applies to every *_loop and *_batch entry of the process */

/* `count` DIFFERENT matrices of one shape: the caller of mtk::qr::qr with many matrices to factor (the reference's README.md:52-87
 * call inside the caller's loop over its matrices).  q, r, a are HOST arrays of `count` device pointers: call i factors a[i] (m x n,
 * lda) into q[i] (ldq) and r[i] (ldr); the leading dimensions, the shape, the mode and the work buffers are shared.  The calls are
 * issued as the stream tsqr_mi_qr_f32_loop issues (tsqr_mi_set_loop_depth): at depth 3 full 64-column matrices of 128 k <= 2^20 rows
 * (and 128-column matrices of 64 k >= 32640 rows) take the chained schedule -- the R-factor chain of matrix i inside the Gram launch of
 * matrix i + 1 -- as long as no two neighbouring calls conflict; everything else, and everything at depth 2, runs two calls in flight
 * in stream order; depth 1 is a loop of blocking calls.  Calls i and i + 1 CONFLICT when Q(i) or R(i) overlaps Q(i + 1), R(i + 1) or
 * A(i + 1), or Q(i + 1) or R(i + 1) overlaps A(i) (byte ranges of ((n - 1) ld + rows) elements; a call's own q[i] == a[i], in place,
 * and two A's that are only read are no conflict): a conflicting pair is issued one call after the other (call i finished before
 * call i + 1 is enqueued), so that a rejected call i runs its ladder before call i + 1 reads or writes anything of it.
 * Whatever the schedule, every matrix gets the blocking call's result bit for bit: a matrix the conditioning check rejects mid-batch
 * gets its whole ladder (the chained schedule ends at it and a fresh one starts behind it), the accepted ones around it stand.
 * states (optional, `count` ints): the state of every call.  Returns the first non-zero state (0: all factored); a negative value
 * (runtime failure) ends the batch at once.  Blocking: complete on return. */
int tsqr_mi_qr_f32_batch(int count, int mode, int reorth,
                         float* const* q, size_t ldq, float* const* r, size_t ldr, float* const* a, size_t lda,
                         size_t m, size_t n,
                         void* wq, void* wr, float* reorth_w, unsigned* d_wl, unsigned* h_wl,
                         void* stream, int* states);

/*
 * The fp16 I/O modes: replaces mtk::qr::qr<fp16_notc | fp16_tc_nocor, Reorthogonalize> (reference src/blockqr.cu:437-449; io type
 * half, src/tsqr.hpp:38-39).  q, r, a are IEEE binary16 (`half` / `_Float16`), column-major like the fp32 entry; everything else
 * as tsqr_mi_qr_f32.  Arithmetic is this engine's fp32 pipeline with fp16 at the boundary, so the result is the fp16 rounding of an
 * fp32-accurate factorisation (the reference computes these modes IN half): fp16_notc forms Q with the error-corrected bf16x3
 * products of fp32_tc_cor, fp16_tc_nocor with one fp16 product (inverse(R) rounded to fp16, no correction).  One panel (n <= 64),
 * no reorthogonalisation, 16-byte aligned columns (base pointers, lda and ldq multiples of 8) and a matrix the bf16-split level
 * accepts take the NATIVE path: the Gram pass uses the halves of A as MFMA operands (exact products), the apply pass reads and
 * writes halves -- half the bytes of the fp32 call.  Everything else is widened into the work buffer, factored by tsqr_mi_qr_f32
 * and narrowed on the way out (two conversion passes).  A is not modified.  R entries beyond the fp16 range (column norms > 65504) become infinities, as a half-typed R does in the reference.
 * Work space: wq of tsqr_mi_working_q_size_f16(m, n) FLOATS (4-byte units: the fp32 call's own space + the widened A, Q and R),
 * wr of tsqr_mi_working_r_size_f16(m, n) floats, d_wl / h_wl as for the fp32 entry.  n <= m, any n.
 */
size_t tsqr_mi_working_q_size_f16(size_t m, size_t n);
size_t tsqr_mi_working_r_size_f16(size_t m, size_t n);
int tsqr_mi_qr_f16(int mode, int reorth,
                   void* q, size_t ldq, void* r, size_t ldr, const void* a, size_t lda,
                   size_t m, size_t n,
                   void* wq, void* wr, void* reorth_w, unsigned* d_wl, unsigned* h_wl,
                   void* stream);
/* `count` calls (the reference's speed loop, src/test.cu:299-309) as tsqr_mi_qr_f32_loop: calls the native path takes (16 < n <= 64, no reorth,
 * aligned halves) are issued as a stream -- two in flight (loop depth >= 2), for n = 64 and count >= 3 also the chained schedule (depth 3) --,
 * everything else as blocking calls; the same halves either way */
int tsqr_mi_qr_f16_loop(int count, int mode, int reorth,
                        void* q, size_t ldq, void* r, size_t ldr, const void* a, size_t lda,
                        size_t m, size_t n,
                        void* wq, void* wr, void* reorth_w, unsigned* d_wl, unsigned* h_wl,
                        void* stream);

/* `count` DIFFERENT half-typed matrices of one shape: tsqr_mi_qr_f32_batch for the fp16 I/O modes (q, r, a: host arrays of device pointers to halves).
 * Calls the native path takes (16 < n <= 64, no reorth, aligned halves, accepted by the bf16-split level) are issued as a stream -- two in flight, for
 * n = 64 the chained schedule while a matrix is small enough for two to share the Infinity Cache --, everything else, and a batch in which two neighbouring
 * calls conflict (as tsqr_mi_qr_f32_batch), as blocking calls; a matrix rejected mid-stream gets its whole ladder (conversion path), the accepted ones around it stand.  The same halves as
 * `count` calls of tsqr_mi_qr_f16.  states (optional): the state of every call.  Returns the first non-zero state. */
int tsqr_mi_qr_f16_batch(int count, int mode, int reorth,
                         void* const* q, size_t ldq, void* const* r, size_t ldr, const void* const* a, size_t lda,
                         size_t m, size_t n,
                         void* wq, void* wr, void* reorth_w, unsigned* d_wl, unsigned* h_wl,
                         void* stream, int* states);

/*
 * Staged entry points used by the row-partitioned multi-GPU path: every rank
 * factors its row block, the n x n R factors are all-gathered (RCCL), every rank folds the stack,
 * and forms its rows of Q.  n <= 64.
 */
/* R (n x n, ldr) of the local block a (m x n); m may be < n (stack of R factors is fine too). */
int tsqr_mi_local_r_f32(float* r, size_t ldr, const float* a, size_t lda, size_t m, size_t n,
                        void* wq, void* wr, void* stream);
/* q (m x n) = a (m x n) * inverse(r); q may alias a. */
int tsqr_mi_apply_rinv_f32(int mode, float* q, size_t ldq, const float* a, size_t lda,
                           const float* r, size_t ldr, size_t m, size_t n,
                           void* wq, void* stream);
/* Staged Gram engine for the row-partitioned path.  level 2 = bf16-split Gram matrix, 1 = fp64 Gram matrix.
 *   tsqr_mi_gram_f32: gsum (tsqr_mi_gram_elems(n) doubles, MFMA-accumulator order) = Gram tiles of the local block;
 *                     the caller sums gsum over the ranks (all-reduce) before
 *   tsqr_mi_chol_f32: R = chol(G) into r, inverse(R) into the work buffer, *status_out = 0 accepted / 1 rejected
 *                     (blocking); m must be the same value as in the other staged calls (it fixes the work-buffer layout)
 *   tsqr_mi_apply_z_f32: q = a * inverse(R) with the inverse left in wq by tsqr_mi_chol_f32. */
size_t tsqr_mi_gram_elems(size_t n);
int tsqr_mi_gram_f32(int level, double* gsum, const float* a, size_t lda, size_t m, size_t n, void* wq, void* wr, void* stream);
int tsqr_mi_chol_f32(int level, float* r, size_t ldr, const double* gsum, size_t m, size_t n, void* wq, unsigned* status_out, void* stream);
/* level 3 = shifted Cholesky (G + s I, s = 11 (m n + n (n+1)) 2^-53 trace(G)) of an fp64 Gram matrix: always accepted for finite
 * input; the caller must follow with one more plain sweep on the resulting Q and multiply the R factors (tsqr_mi_rmul_f32).
 * status_out == NULL above: asynchronous (no stream sync); the verdict is then read with tsqr_mi_chol_status (blocking) -- lets a
 * caller enqueue tsqr_mi_apply_z_f32 speculatively behind the Cholesky and pay one synchronisation per sweep. */
int tsqr_mi_chol_status(const void* wq, size_t m, size_t n, unsigned* status_out, void* stream);
/* blocks until everything enqueued on `stream` so far has completed (spin on a pinned completion word; stream sync as fallback) */
int tsqr_mi_stream_wait(void* stream);
int tsqr_mi_apply_z_f32(int mode, float* q, size_t ldq, const float* a, size_t lda, size_t m, size_t n, void* wq, void* stream);
/* r (n x n) <- r2 * r (upper triangular product, used after a reorthogonalisation sweep) */
int tsqr_mi_rmul_f32(float* r, size_t ldr, const float* r2, size_t ldr2, size_t n, void* wq, void* stream);

/* Row-partitioned TSQR (the reference has no multi-GPU path): one call per rank, every rank passes its own
 * row block (m_local may differ between ranks, 1 <= m_local on every rank -- a rank that returns 1 for an empty block would leave
 * the others waiting in their exchange; m_local < n is fine), r is bitwise identical on all ranks on return.  n <= 64 is one panel;
 * n > 64 runs 64-column panels whose coupling coefficients are all-reduced like the Gram tiles (a is then overwritten).  It is the SAME ladder as
 * tsqr_mi_qr_f32 with two exchange hooks switched on, all enqueued on `stream` with no host wait before the end of the call:
 *   Gram levels:        all-reduce (sum) of the Gram tiles + the local row count: <= 2561 doubles.  Every rank then factors the
 *                       same matrix with thresholds from the same (global) row count, so the accept / reject decisions agree on
 *                       all ranks by construction -- a NaN anywhere reaches everyone through the sum;
 *   Householder engine: all-gather of the n x n local R factors, every rank folds the same (nranks n) x n stack.
 * Work buffers: tsqr_mi_working_{q,r}_size_dist(m_local, n, nranks) elements; gather_buf: nranks * min(n, 64)^2 floats.
 * The communicator and the collectives that run on it must come from ONE RCCL instance (a process may have two mapped: torch
 * bundles a copy, /opt/rocm holds another), so the library never searches for librccl itself:
 * tsqr_mi_qr_f32_dist_fn: the caller passes its ncclComm_t (as void*) together with the addresses of ncclAllReduce and ncclAllGather
 *   taken from the library that created it (dlsym on that handle; Python: ctypes.cast(lib.ncclAllReduce, c_void_p)).
 * tsqr_mi_qr_f32_dist: for a caller that LINKS RCCL (C++): the two entry points are looked up in the global symbol scope
 *   (dlsym(RTLD_DEFAULT, ...)) -- the copy the caller's own ncclCommInitRank came from; TSQR_MI_ERROR_UNSUPPORTED when they are not there.
 * tsqr_mi_qr_f32_dist_cb: caller-supplied collectives (blocking or stream-ordered; in place sum / gather in rank order), e.g.
 *   torch.distributed over gloo -- what the multi-process tests use.
 * *_loop: `count` calls as a stream (see tsqr_mi_qr_f32_loop); every rank must pass the same count and run at the same loop depth -- the
 *   ranks take the same verdicts, hence the same path through the loop and the same order of collectives.  Depth 3, count >= 3: when
 *   EVERY rank holds a full 64-column block of 128 k <= 2^20 rows the Cholesky launch of call i rides in the Gram launch of call i + 1
 *   and allreduce(i + 1) is enqueued before apply(i).  The ranks agree on that without a collective of its own: the first all-reduce
 *   of the loop call (the Gram tiles of call 0) carries one more double, 1.0 from every eligible rank; nranks <= 255. */
size_t tsqr_mi_working_q_size_dist(size_t m_local, size_t n, int nranks);
size_t tsqr_mi_working_r_size_dist(size_t m_local, size_t n, int nranks);
int tsqr_mi_qr_f32_dist(int mode, int reorth,
                        float* q, size_t ldq, float* r, size_t ldr, float* a, size_t lda,
                        size_t m_local, size_t n,
                        void* wq, void* wr, float* gather_buf /* nranks*n*n floats */,
                        void* nccl_comm, int nranks, void* stream);
int tsqr_mi_qr_f32_dist_fn(int mode, int reorth,
                           float* q, size_t ldq, float* r, size_t ldr, float* a, size_t lda,
                           size_t m_local, size_t n,
                           void* wq, void* wr, float* gather_buf /* nranks*n*n floats */,
                           void* nccl_comm, void* nccl_allreduce_fn, void* nccl_allgather_fn, int nranks, void* stream);
int tsqr_mi_qr_f32_dist_fn_loop(int count, int mode, int reorth,
                                float* q, size_t ldq, float* r, size_t ldr, float* a, size_t lda,
                                size_t m_local, size_t n,
                                void* wq, void* wr, float* gather_buf,
                                void* nccl_comm, void* nccl_allreduce_fn, void* nccl_allgather_fn, int nranks, void* stream);
/* *_batch: `count` DIFFERENT row-partitioned matrices of one shape (host arrays of device pointers; one block height per rank for all of them), issued as
 * the stream of calls of the *_loop entries; every rank passes the same count and operands of the same eligibility.  When two neighbouring calls conflict
 * (tsqr_mi_qr_f32_batch) on ANY rank -- the ranks agree on that with one all-reduce of one flag per batch call -- the batch runs as blocking calls on every
 * rank.  states (optional): per call. */
int tsqr_mi_qr_f32_dist_fn_batch(int count, int mode, int reorth,
                                 float* const* q, size_t ldq, float* const* r, size_t ldr, float* const* a, size_t lda,
                                 size_t m_local, size_t n,
                                 void* wq, void* wr, float* gather_buf,
                                 void* nccl_comm, void* nccl_allreduce_fn, void* nccl_allgather_fn, int nranks, void* stream, int* states);
typedef int (*tsqr_mi_allreduce_f64_cb)(void* user, double* buf /* device */, size_t count, void* stream);
typedef int (*tsqr_mi_allgather_f32_cb)(void* user, const float* send /* device */, float* recv /* device, nranks*count */, size_t count, void* stream);
int tsqr_mi_qr_f32_dist_cb(int mode, int reorth,
                           float* q, size_t ldq, float* r, size_t ldr, float* a, size_t lda,
                           size_t m_local, size_t n,
                           void* wq, void* wr, float* gather_buf,
                           tsqr_mi_allreduce_f64_cb allreduce, tsqr_mi_allgather_f32_cb allgather, void* user, int nranks, void* stream);
int tsqr_mi_qr_f32_dist_cb_loop(int count, int mode, int reorth,
                                float* q, size_t ldq, float* r, size_t ldr, float* a, size_t lda,
                                size_t m_local, size_t n,
                                void* wq, void* wr, float* gather_buf,
                                tsqr_mi_allreduce_f64_cb allreduce, tsqr_mi_allgather_f32_cb allgather, void* user, int nranks, void* stream);
int tsqr_mi_qr_f32_dist_cb_batch(int count, int mode, int reorth,
                                 float* const* q, size_t ldq, float* const* r, size_t ldr, float* const* a, size_t lda,
                                 size_t m_local, size_t n,
                                 void* wq, void* wr, float* gather_buf,
                                 tsqr_mi_allreduce_f64_cb allreduce, tsqr_mi_allgather_f32_cb allgather, void* user, int nranks, void* stream, int* states);

/*
 * Double-precision tall-skinny QR (not in the reference): q (m x n, ldq), r (n x n, ldr) and a (m x n, lda) hold doubles, column-major,
 * device memory; 1 <= n <= 64, n <= m.  Blocking: returns when its work on `stream` has finished.  A is untouched unless q == a
 * (in place, allowed with ldq == lda); Q and R must not overlap A otherwise, nor each other.  R: the full n x n block, exact zeros below
 * the diagonal, a positive diagonal.  Bitwise deterministic (fixed reduction tree).  Work space: wq of tsqr_mi_working_q_size_f64(m, n)
 * doubles, wr of tsqr_mi_working_r_size_f64(m, n) doubles.
 * Sweeps of CholeskyQR on the fp64 matrix cores; the Cholesky step judges each Gram matrix on the device (the rule and its sources:
 * CholArgs64 in tsqr_f64.hip):
 *   reorth = 0  sweep 1 alone when its estimated ||Q^T Q - I||_F is <= 1e-12 (well-conditioned input: cond(A D^-1) <= 10 with D the column norms, always), else a
 *               second sweep on Q (CholeskyQR2); a Gram matrix the rule rejects is factored shifted, and two plain sweeps follow
 *               (shifted CholeskyQR3).  For cond(A) <= 1e12, m <= 2^23: ||Q^T Q - I||_F <= 1e-11, ||A - Q R||_F / ||A||_F <= 1e-13.
 *   reorth = 1  at least two sweeps (CholeskyQR2), shifted CholeskyQR3 on rejection: ||Q^T Q - I||_F <= 1e-12, residual as above.
 * Returns 0, 1 (n > m, m == 0, n == 0, or a leading dimension below its operand's rows), 2 (n > 64; tsqr_mi_last_error says so),
 * 3 = TSQR_MI_ERROR_NOT_FINITE, or -(hipError_t).  Sizes are checked before any HIP call.
 * tsqr_mi_last_sweeps_f64: sweeps of the calling thread's last tsqr_mi_qr_f64, plus 100 when it took the shifted path.
 */
size_t tsqr_mi_working_q_size_f64(size_t m, size_t n);
size_t tsqr_mi_working_r_size_f64(size_t m, size_t n);
int tsqr_mi_qr_f64(int reorth, double* q, size_t ldq, double* r, size_t ldr, double* a, size_t lda,
                   size_t m, size_t n, void* wq, void* wr, void* stream);
int tsqr_mi_last_sweeps_f64(void);

/*
 * The R factor alone, in double precision (not in the reference): tsqr_mi_qr_f64's R without ever forming Q, for callers that need only
 * R (semi-normal equations, preconditioning, singular values, an R that is reduced further).  r (n x n, ldr) and a (m x n, lda) hold
 * doubles, column-major, device memory; 1 <= n <= 64, n <= m.  Blocking: returns when its work on `stream` has finished.  A is never
 * written; r must not overlap A.  R: the full n x n block, exact zeros below the diagonal, a positive diagonal.  Bitwise deterministic
 * (fixed launch plans, fixed reduction tree).  Work space: wq of tsqr_mi_working_q_size_f64_r(m, n) doubles (independent of m), wr of
 * tsqr_mi_working_r_size_f64_r(m, n) doubles (the larger of the two Gram plans' partials); there is no m x n buffer.
 * The ladder, the verdicts and the acceptance rule are tsqr_mi_qr_f64's (CholArgs64 in tsqr_f64.hip).  Sweep 1 is that entry's first
 * Gram pass and Cholesky step on A -- one read of A, and for a call that ends there R is bitwise tsqr_mi_qr_f64's.  Every further
 * sweep reads A once more and writes nothing of size m: it takes the Gram matrix of A Z, Z the product of the inverses of all sweeps so
 * far, forming each 16-row block of A Z in registers (gramq_f64_kernel), and multiplies R on the left.
 *   reorth = 0  one sweep when the device's estimate allows it, else two; shifted CholeskyQR3 (three sweeps) on a rejected Gram matrix
 *   reorth = 1  at least two sweeps
 * For cond(A) <= 1e12: ||(A inverse(R))^T (A inverse(R)) - I||_F is within a small factor of Householder QR's R on the same A (DESIGN.md
 * section 9 has the measured factors), ||R^T R - A^T A||_F / ||A^T A||_F <= 1e-13.
 * Returns 0, 1 (n > m, m == 0, n == 0, lda < m or ldr < n), 2 (n > 64; tsqr_mi_last_error says so), 3 = TSQR_MI_ERROR_NOT_FINITE, or
 * -(hipError_t).  Sizes are checked before any HIP call.  tsqr_mi_last_sweeps_f64 reports this entry too.
 */
size_t tsqr_mi_working_q_size_f64_r(size_t m, size_t n);
size_t tsqr_mi_working_r_size_f64_r(size_t m, size_t n);
int tsqr_mi_r_f64(int reorth, double* r, size_t ldr, const double* a, size_t lda,
                  size_t m, size_t n, void* wq, void* wr, void* stream);

/*
 * Least squares in double precision on the R-only factorisation (not in the reference): X = argmin ||A X - B||_F and R of tsqr_mi_r_f64.
 * x (n x nrhs, ldx), r (n x n, ldr), a (m x n, lda), b (m x nrhs, ldb) hold doubles, column-major, device memory; 1 <= n <= 64, n <= m,
 * 1 <= nrhs <= 16, 0 <= refine <= 4.  Blocking.  A and B are never written; x and r must not overlap A, B or each other.  Nothing of
 * size m is stored: wq of tsqr_mi_working_q_size_f64_lstsq doubles (independent of m), wr of tsqr_mi_working_r_size_f64_lstsq doubles.
 * Bitwise deterministic (the launch plan is a fixed function of (m, n); fixed reduction tree).
 * Method -- corrected semi-normal equations carried out in Q-space: the ladder of tsqr_mi_r_f64 (reorth as there; R is bitwise that
 * entry's), Z = inverse(R) as the product of the sweeps' inverses, then refine + 1 passes that each read A and B once:
 *   X_0 = Z (Q~^T B),   X <- X + Z (Q~^T (B - A X)),   Q~ = A Z formed 16 rows at a time in registers, never stored
 * (lsq_f64_kernel).  The ladder waits on the host as tsqr_mi_r_f64 does; the passes behind it are enqueued back to
 * back with one wait at the end.  Stagnation rule, from the second correction on and one right-hand side at a time: a correction
 * whose max_k |D[k][j]|, D = Q~^T (B - A X), is above half of that of the pass before is not applied, and right-hand side j keeps its X
 * for the rest of the call -- past convergence a correction is the rounding noise of its own pass and only redraws the error of X
 * (measured without the rule: refine = 3 ended 2.15 times above refine = 2 on a 300 x 17 matrix of cond 1e6).  refine = 0 and 1
 * return the bits they always returned; refine >= 2 never returns an X that an earlier pass refused to change.
 * Accuracy: each correction pass contracts the error of X by a factor of order cond(A)^2 u, so the method is NOT a substitute for
 * Householder QR beyond cond(A) of about 1e7.  Claimed for cond(A) <= 1e6 and refine >= 1: ||X - X*||_F / ||X*||_F within a small
 * factor of LAPACK's fp64 least-squares solve on the same data (DESIGN.md section 9 and profiles/fp64_lstsq_accuracy.md have the
 * measured factors: at most 0.69 over Gaussian and cond 1 .. 1e6 matrices).  For larger cond(A) the call still returns 0 while the
 * ladder accepts A; what follows is measured (4096 x 64, 16 right-hand sides, B = A X*, error of refine = 0 / 1 / 2, LAPACK's), not a bound:
 *   cond 1e7: 7.4e-5 / 1.6e-11 / 1.3e-11, 2.7e-11;  cond 1e8: 8.3e-3 / 1.3e-10 / 1.2e-10, 1.9e-10;  cond 1e10: 1e2 / 8.0e-7 / 8.7e-9, 1.6e-8
 * -- at 1e10 X_0 has no correct digit and refine = 1 is 50 times worse than LAPACK.  refine = 0 returns X_0, whose error grows like
 * cond(A)^2 u when the residual is small.
 * Non-finite B: B enters the residual through a matrix product with an identity operand, so ONE Inf or NaN in row i of B makes row i of
 * the residual non-finite for all right-hand sides, hence every column of X; the call returns 0.  Non-finite A is the ladder's state 3.
 * Magnitudes.  A: the column norms of tsqr_mi_qr_f64, [2^-511, 2^512) (||A||_F < 2^512 on the shifted path).  B: a column b of B is in
 * contract when it is zero or
 *     2^-960 max(1, ||A||_F)  <=  ||b||_2  <=  2^1000 min(1, sigma_min(A)).
 * Above, the largest intermediates are |D| <= ||q|| ||b|| and |X| <= ||b|| / sigma_min(A); below, the correction pass of a consistent
 * system carries a residual of u ||b|| and an update of u ||b|| / ||A||, which must keep a few digits above the subnormal spacing.  The
 * columns of B do not interact (finite B): column c of X depends on column c of B alone, bit for bit.  Inside these ranges the call is
 * covariant under powers of two, bit for bit: A diag(2^k_c) and B diag(2^j_c) return diag(2^-k_c) X diag(2^j_c) and R diag(2^k_c) with
 * the same state and sweeps -- uniform k on every rung of the ladder, per-column k while the ladder does not shift
 * (tests/test_gpu_f64_lstsq_scale.py; measured there too: a Gaussian column scaled by 2^-1000 or 2^1012, beyond either end, still came
 * back with the unscaled column's bits).
 * State 0 and state 3.  State 3 is the ladder's verdict and no rank test: it is returned for Inf or NaN in A, for column norms outside
 * the range above, and for an exactly zero column (the ladder ends at its cap).  A matrix with dependent but non-zero columns -- a
 * copied column, a column that is the rounded sum of two others, a tail of copies -- is ACCEPTED on the shifted path: state 0, R
 * bitwise tsqr_mi_r_f64's, and an X that is finite, deterministic and NOT a least-squares solution.  Measured (4097 x 64 and
 * 1029 x 51, profiles/fp64_lstsq_scale_tests.md): entries of X of 1e14 .. 7e18; for B in the range of A, ||B - A X||_F of 15 .. 46
 * (||B||_F 360 .. 1470; the minimum is 1e-13) with one dependent column and 2e5 -- a hundred times ||B||_F -- with a tail of copies.  A
 * caller that cannot rule out dependent columns must test R (its smallest diagonal entry against its largest) before it uses X.
 * Returns 0; 1 (m, n or nrhs == 0, n > m, lda < m, ldb < m, ldr < n or ldx < n); 2 (n > 64, nrhs > 16, refine outside 0 .. 4;
 * tsqr_mi_last_error says which); 3 = TSQR_MI_ERROR_NOT_FINITE from the ladder (see above; x is undefined); or
 * -(hipError_t).  Sizes are checked before any HIP call.  tsqr_mi_last_sweeps_f64 reports this entry's ladder too.
 */
size_t tsqr_mi_working_q_size_f64_lstsq(size_t m, size_t n, size_t nrhs);
size_t tsqr_mi_working_r_size_f64_lstsq(size_t m, size_t n, size_t nrhs);
int tsqr_mi_lstsq_f64(int reorth, int refine, double* x, size_t ldx, double* r, size_t ldr,
                      const double* a, size_t lda, const double* b, size_t ldb,
                      size_t m, size_t n, size_t nrhs, void* wq, void* wr, void* stream);

/*
 * tsqr_mi_r_f64 and tsqr_mi_lstsq_f64 on operands that are read where they lie in either layout (not in the reference).  a_layout and
 * b_layout are TSQR_MI_COL_MAJOR (element (i, j) at a[i + j * lda], lda >= m: the entries above) or TSQR_MI_ROW_MAJOR (element (i, j)
 * at a[i * lda + j], lda >= n; for B b[i * ldb + j], ldb >= nrhs -- a contiguous C or torch array of shape (m, n)).  R and X are
 * column-major as above; the work space is that of tsqr_mi_working_{q,r}_size_f64_r and ..._f64_lstsq.  No copy of A or B is made and
 * nothing between n and lda (nrhs and ldb) or behind row m is read.
 * Bit-for-bit relation: the row-major kernels put the values of A and B into the registers the column-major kernels hold them in, on the
 * same launch plans, so R, X, the state and tsqr_mi_last_sweeps_f64 are BITWISE those of tsqr_mi_r_f64 / tsqr_mi_lstsq_f64 on a
 * column-major copy of the same matrices.  With every layout TSQR_MI_COL_MAJOR the calls ARE those entries (which call these).  The
 * accuracy statements, the ladder and the non-finite rules above hold unchanged.
 * Measured on one MI355X (profiles/fp64_rowmajor_speed.json, median of 50 blocking calls, ms; row-major / column-major / a transposing
 * copy of the operands followed by the column-major call): tsqr_mi_lstsq_f64_lay, refine 1, 16 right-hand sides, 2^20 x 64
 * 0.748 / 0.700 / 2.31, 2^23 x 64 4.67 / 4.37 / 20.4; tsqr_mi_r_f64_lay 2^20 x 64 0.187 / 0.165 / 1.46 (one sweep), 0.475 / 0.466 / 1.75
 * (reorth = 1).  The one-sweep call is 13 .. 23 % slower row-major (narrower loads in the first Gram pass); later sweeps are level.
 * Returns what those entries return; 1 also for a layout other than 0 or 1, and for a row-major operand with lda < n or ldb < nrhs
 * (not lda < m).  Arguments are checked before any HIP call.
 */
#define TSQR_MI_COL_MAJOR 0
#define TSQR_MI_ROW_MAJOR 1
int tsqr_mi_r_f64_lay(int a_layout, int reorth, double* r, size_t ldr, const double* a, size_t lda,
                      size_t m, size_t n, void* wq, void* wr, void* stream);
int tsqr_mi_lstsq_f64_lay(int a_layout, int b_layout, int reorth, int refine, double* x, size_t ldx, double* r, size_t ldr,
                          const double* a, size_t lda, const double* b, size_t ldb,
                          size_t m, size_t n, size_t nrhs, void* wq, void* wr, void* stream);

/*
 * tsqr_mi_qr_f64 on operands in either layout (not in the reference): a_layout is how A is stored, q_layout how Q is written, each
 * TSQR_MI_COL_MAJOR (element (i, j) at p[i + j * ld], ld >= m) or TSQR_MI_ROW_MAJOR (element (i, j) at p[i * ld + j], ld >= n -- a
 * contiguous C or torch array of shape (m, n)); the two need not agree.  R is column-major as above.  The work space is that of
 * tsqr_mi_working_{q,r}_size_f64.  No copy of A or Q is made; nothing between n and the leading dimension of a row-major operand, or
 * behind row m, is read or written.  1 <= n <= 64, n <= m.
 * Sweep 1 reads A in a_layout (the Gram pass, then the apply pass, which writes Q in q_layout); later sweeps read and write Q in
 * q_layout, in place (gram_f64_kernel and apply_f64_kernel with their layout flags, tsqr_f64.hip).
 * Bit-for-bit relation: the row-major kernels put the values of A into the registers the column-major kernels hold them in, on the same
 * launch plans, and a row-major Q is formed by the same products summed in the same order (the MFMA operands swapped: apply_f64_kernel),
 * so Q -- read as a matrix --, R, the state and tsqr_mi_last_sweeps_f64 are BITWISE those of tsqr_mi_qr_f64 on a column-major copy of
 * the same matrix, for all four layout pairs.  With both layouts TSQR_MI_COL_MAJOR the call IS tsqr_mi_qr_f64 (which calls this one).
 * The accuracy bands, the ladder and the non-finite rules of tsqr_mi_qr_f64 hold unchanged.  In place as there: q == a is allowed with
 * a_layout == q_layout and ldq == lda; Q and R must not overlap A otherwise, nor each other.
 * Beyond n = 64: tsqr_mi_qr_f64_wide_lay below.  Column-major only: the row-partitioned entries (tsqr_mi_qr_f64_dist*) take no layout.
 * Returns what tsqr_mi_qr_f64 returns; 1 also for a layout other than 0 or 1, for a row-major operand with a leading dimension below
 * n (not below m), and for q == a with different layouts or ldq != lda; 2 for n > 64 (tsqr_mi_last_error says so).  Arguments are
 * checked before any HIP call.
 */
int tsqr_mi_qr_f64_lay(int a_layout, int q_layout, int reorth, double* q, size_t ldq, double* r, size_t ldr, double* a, size_t lda,
                       size_t m, size_t n, void* wq, void* wr, void* stream);

/*
 * Singular value decomposition of a tall-skinny matrix in double precision (not in the reference): A = U diag(s) V^T, 1 <= n <= 64,
 * n <= m.  a (m x n, lda, a_layout) and u (m x n, ldu, u_layout) as the operands of tsqr_mi_qr_f64_lay; s: n doubles, descending and
 * non-negative; v: n x n column-major with leading dimension ldv, holding V (not V^T), or NULL when V is not wanted.  Blocking.
 * Bitwise deterministic from call to call.  The signs of the columns of U and V are those the fixed rotation order produces:
 * unspecified but reproducible.
 * Method: QR, one-sided Jacobi on R, then a product.  R = W diag(s) V^T on one workgroup (svd_r_f64_kernel, tsqr_f64.hip: Hestenes
 * rotations in round-robin order on R scaled by a power of two to max |r_ij| in [1, 2), dgesvj's criterion
 * |a_pq| <= sqrt(n) 2^-53 sqrt(a_pp a_qq), at most 30 sweeps).  The rotations act on the columns of R^T, which converges in fewer
 * sweeps than R: s_j are the column norms, V the normalised columns and W the product of the rotations.  A column whose norm is
 * exactly zero gives a zero column of V (W stays orthonormal) -- possible by underflow only, because the ladder's R has a positive
 * diagonal.
 *   jobu = 1  the ladder of tsqr_mi_qr_f64_lay, called as it stands (reorth as there), writes Q into u and R into the work space;
 *             then U = Q W in place over Q on the fp64 matrix cores (applyd_f64_kernel).  u == a is allowed as there: one layout and
 *             ldu == lda; A is untouched otherwise.  Work space: that entry's plus a block that does not depend on m --
 *             wq of tsqr_mi_working_q_size_f64(m, n) + 8200 doubles, wr of tsqr_mi_working_r_size_f64(m, n) doubles.
 *             ||U^T U - I||_F stays within that entry's band (1e-11; 1e-12 with reorth = 1) up to the orthogonality of W.
 *   jobu = 0  u, ldu and u_layout are ignored and A is read only: the ladder of tsqr_mi_r_f64_lay -- no m x n buffer, that entry's
 *             work-space sizes -- and s and V from its R.  That work space has no block that outlives a sweep, so R is kept in 32 KiB of
 *             device memory the library owns per host thread and device (allocated at the first such call).
 * Returns the states of those entries in their order -- 1 for a layout other than 0 or 1 (a_layout; u_layout with jobu = 1), for n > m,
 * m == 0, n == 0, a leading dimension below its operand's extent (ldv < n when v is given), a jobu other than 0 or 1, or u == a with
 * different layouts or leading dimensions; 2 for n > 64 -- all before any HIP call; 3 = TSQR_MI_ERROR_NOT_FINITE from the ladder, before
 * the SVD kernel runs; 4 = TSQR_MI_ERROR_NO_CONVERGENCE when the sweep cap is reached (s, v and u are then undefined); or -(hipError_t).
 * State 3 is the ladder's verdict and no rank test; the numerical rank is read off s.
 * tsqr_mi_last_sweeps_f64 reports the ladder of this entry too; tsqr_mi_last_jacobi_sweeps_f64 the Jacobi sweeps of the calling
 * thread's last tsqr_mi_svd_f64, the final sweep without a rotation included (0 when the kernel did not run).
 * Not provided: n > 64, the row-partitioned and batched forms, and the m x m U.
 */
size_t tsqr_mi_working_q_size_f64_svd(size_t m, size_t n, int jobu);
size_t tsqr_mi_working_r_size_f64_svd(size_t m, size_t n, int jobu);
int tsqr_mi_svd_f64(int a_layout, int u_layout, int jobu, int reorth,
                    double* u, size_t ldu, double* s, double* v, size_t ldv,
                    double* a, size_t lda, size_t m, size_t n,
                    void* wq, void* wr, void* stream);
int tsqr_mi_last_jacobi_sweeps_f64(void);

/*
 * QR with column pivoting of a tall-skinny matrix in double precision (not in the reference): A P = Q R, 1 <= n <= 64, n <= m --
 * what LAPACK's dgeqp3 and scipy.linalg.qr(pivoting=True, mode="economic") return.  a (m x n, lda, a_layout) and q (m x n, ldq,
 * q_layout) as the operands of tsqr_mi_qr_f64_lay; r: n x n column-major with leading dimension ldr, upper triangular with exact
 * zeros below the diagonal, diag(R) >= 0 and non-increasing, and R_kk^2 >= sum_{i=k..j} R_ij^2 for every j > k up to rounding (the
 * Businger-Golub property); jpvt: n int values on the device, 0-based: column j of A P is column jpvt[j] of A.  Blocking.  Bitwise
 * deterministic from call to call.
 * Method: QR, a small pivoted QR of R, then a product.  A = Q0 R0 by the ladder, R0 into r; R0 P = H R on one workgroup in place on r
 * (qrcp_r_f64_kernel, tsqr_f64.hip: Householder reflectors built as dlarfg builds them on R0 scaled by a power of two to
 * max |r_ij| in [1, 2); at every step the squared norms of the remaining part of every remaining column are summed afresh, never
 * downdated; the pivot is the largest, on a tie the one at the lowest POSITION among the remaining columns as the swaps of the steps
 * before have left them -- step k exchanges the columns at positions k and p, so among equal columns that is not always the lowest
 * column of A: norms (1, 1, 2) give jpvt = (2, 1, 0); a column that is exactly zero gives H_k = I and R_kk = 0 without a
 * division; a negative R_kk is made positive by negating row k of R and column k of H, which is exact).  n steps, no iteration, no
 * state of its own.
 *   jobq = 1  the ladder of tsqr_mi_qr_f64_lay, called as it stands (reorth as there), writes Q0 into q; then Q = Q0 H in place on
 *             the fp64 matrix cores (applyd_f64_kernel).  q == a is allowed as there: one layout and ldq == lda; A is untouched
 *             otherwise.  Work space: that entry's plus a block that does not depend on m -- wq of
 *             tsqr_mi_working_q_size_f64(m, n) + 4104 doubles (H and status words), wr of tsqr_mi_working_r_size_f64(m, n) doubles.
 *   jobq = 0  q, ldq and q_layout are ignored and A is read only: the ladder of tsqr_mi_r_f64_lay -- no m x n buffer, exactly that
 *             entry's work-space sizes, nothing allocated -- and R and jpvt from its R0; H is not formed.
 * Band: the claims hold where those of tsqr_mi_qr_f64_lay do, cond(A) <= 1e12: ||Q^T Q - I||_F <= 1e-11 (1e-12 with reorth = 1) up to
 * the orthogonality of H (a few n 2^-53), ||A P - Q R||_F / ||A||_F <= 1e-13.  Outside it the call returns what the ladder returns,
 * and diag(R) is then evidence of the same standing as s of tsqr_mi_svd_f64: state 3 is the ladder's verdict and no rank test, and a
 * matrix with an exactly copied column is accepted by the ladder on its shifted path (as documented for tsqr_mi_lstsq_f64) -- R0 is
 * then the factor of a perturbed matrix and the trailing diagonal of R is small but carries no bound.
 * Returns the states of those entries in their order -- 1 for a layout other than 0 or 1 (a_layout; q_layout with jobq = 1), for n > m,
 * m == 0, n == 0, a leading dimension below its operand's extent, a jobq other than 0 or 1, or q == a with different layouts or
 * leading dimensions; 2 for n > 64 -- all before any HIP call; 3 = TSQR_MI_ERROR_NOT_FINITE from the ladder, before the pivoting kernel
 * runs (r, jpvt and q are then undefined; jpvt is not written); or -(hipError_t).  tsqr_mi_last_sweeps_f64 reports the ladder of this
 * entry too.  The pointers r, jpvt, a (and q with jobq = 1) and the work space are not checked: they must be valid device memory.
 * Not provided: n > 64, the row-partitioned and batched forms, the m x m Q, and a rank-aware least-squares solve on top of it.
 */
size_t tsqr_mi_working_q_size_f64_qrcp(size_t m, size_t n, int jobq);
size_t tsqr_mi_working_r_size_f64_qrcp(size_t m, size_t n, int jobq);
int tsqr_mi_qrcp_f64(int a_layout, int q_layout, int jobq, int reorth,
                     double* q, size_t ldq, double* r, size_t ldr, int* jpvt,
                     double* a, size_t lda, size_t m, size_t n,
                     void* wq, void* wr, void* stream);

/*
 * Rank-aware least squares in double precision (not in the reference): the rank of A and the BASIC solution of min ||A X - B||_F on
 * the numerically independent columns of A; 1 <= n <= 64, n <= m, 1 <= nrhs <= 16.  a (m x n, lda, a_layout) and b (m x nrhs, ldb,
 * b_layout) as the operands of tsqr_mi_lstsq_f64_lay, read only; x: n x nrhs and r: n x n, column-major (ldx, ldr >= n), jpvt: n int
 * values, all three on the device; rank: ONE int on the HOST.  Blocking.  Bitwise deterministic from call to call, and the same bits
 * for either layout of a and of b.  Nothing of size m is stored, nothing is allocated, A and B are never written.
 * Method.  (1) The ladder of tsqr_mi_r_f64_lay writes R0 into r.  (2) qrcp_r_f64_kernel factors R0 P = H R in place on r without
 * forming H: r, jpvt and tsqr_mi_last_sweeps_f64 are BITWISE those of tsqr_mi_qrcp_f64 with jobq = 0 on the same a, a_layout and
 * reorth.  (3) The rank k is the number of j with R_jj > rcond R_00 (diag(R) is non-negative and non-increasing), and
 * Zeff = P1 inverse(R11), R11 = R[:k, :k], P1 the retained columns jpvt[:k]: cond(R11) is about 1 / rcond at most whatever cond(A) is.
 * (4) One CholeskyQR step on the retained columns: G1 = (A Zeff)^T (A Zeff) in one pass over A, G1 = Rc^T Rc by plain Cholesky,
 * Zeff <- Zeff inverse(Rc).  The ladder never stores Q, so on an exactly dependent interior column its R0 is inconsistent in the
 * columns behind it and A P1 inverse(R11) is orthonormal to about 2e-2 only; after the step it is orthonormal to about
 * cond(A P1)^2 2^-53.  (5) refine + 1 passes X <- X + Zeff (A Zeff)^T (B - A X), each one pass over A and B, with the stagnation rule of
 * tsqr_mi_lstsq_f64 (0 <= refine <= 4).  Rows jpvt[rank:] of x are exact zeros, the other rows are the least-squares solution on the
 * columns jpvt[:rank] -- the basic solution, NOT the minimum-norm one (tsqr_mi_lstsq_minnorm_f64 below).
 * Fixed point.  The iteration stops moving when Zeff^T A^T (B - A X) = 0.  Zeff^T = (R11 Rc)^-T P1^T has full row rank for any
 * non-singular R11 Rc, so that is (A P1)^T (B - A X) = 0, the normal equations of the retained columns: errors in R11 and Rc change
 * how fast the passes contract, about ||I - (A Zeff)^T (A Zeff)||, never where they stop.
 * rcond: column j is retained when R_jj > rcond R_00.  rcond < 0 stands for max(m, n) 2^-52.  The pivots of a matrix with dependent
 * columns are small but carry no bound (tsqr_mi_qrcp_f64): a column is dropped reliably when its pivot is well below rcond R_00 and
 * kept reliably when well above; on the threshold either may happen.
 * Accuracy: bounded by what was measured (MI355X, refine = 1, Gaussian and consistent B; profiles/fp64_lstsq_rank_accuracy.md has every
 * figure next to LAPACK's dgelsd on the retained columns).  The retained columns have cond(A P1) <~ 1 / rcond and each pass contracts
 * by about cond(A P1)^2 2^-53 after the step.  On the seven cases of tests/pass_refs_f64_lsq_rank.py -- a copied interior column at
 * 4096 x 16, rank 32 of 51, rank 1 of 33, rank 40 of 64 with singular values down to 1e-4, full rank 300 x 17, three copied tail
 * columns of 7, one column -- the error ||X[jpvt[:k]] - X*||_F / ||X*||_F against an extended-precision solve stays within
 * max(2 x LAPACK's, 4 n 2^-53).  Measured / LAPACK's, Gaussian B then consistent B:
 *   copied column 4096 x 16   2.5e-16 / 1.8e-15    1.6e-17 / 1.2e-15      rank 32 of 51, 1029 rows   8.8e-16 / 3.0e-15    9.2e-17 / 2.9e-15
 *   rank 1 of 33, 777 rows    2.3e-16 / 1.6e-15    5.3e-17 / 2.0e-16      rank 40 of 64, 4097 rows   1.2e-12 / 1.0e-12    2.3e-14 / 3.8e-14
 *   full rank 300 x 17        2.9e-16 / 1.7e-15    3.1e-17 / 1.7e-15      3 copied tail columns of 7 1.6e-16 / 7.0e-15    2.9e-17 / 7.9e-15
 *   one column, 65 rows       1.3e-16 / 2.7e-16    1.0e-17 / 2.8e-16
 * The hardest of them has cond(A P1) = 1e4 (rank 40 of 64).  Nothing is claimed beyond these cases: in particular not for
 * cond(A P1) above about 1e6, where the contraction cond(A P1)^2 2^-53 of a pass is no longer small.
 * Work space: wq of tsqr_mi_working_q_size_f64_lstsq_rank doubles -- tsqr_mi_lstsq_f64's plus Zeff, the step's Gram sum and status
 * words, independent of m -- and wr of tsqr_mi_working_r_size_f64_lstsq_rank doubles, the R-only entry's.
 * Returns 0; 1 when ANY of x, r, jpvt, rank, a, b, wq, wr is null (decided first of all), then for the layout, size and leading
 * dimension rules of tsqr_mi_lstsq_f64_lay (no text); 2 with a text for n > 64, nrhs > 16, refine outside 0 .. 4, rcond >= 1 or NaN,
 * in that order -- all of 1 and 2 before any HIP call; 3 = TSQR_MI_ERROR_NOT_FINITE from the ladder, unchanged (Inf or NaN in A, a
 * column norm outside [2^-511, 2^512), and still an exactly ZERO column among non-zero ones: the ladder rejects it before any rank
 * decision; x, jpvt and *rank are then not written), or 3 with its own text when the Cholesky step on the retained columns meets a
 * pivot that is not positive or not finite (x is then zero and *rank is written); or -(hipError_t).  Non-null pointers are not
 * checked further: they must be valid memory of the sizes above.
 * Not provided: n > 64, the row-partitioned and batched forms, residual norms as an output.
 */
size_t tsqr_mi_working_q_size_f64_lstsq_rank(size_t m, size_t n, size_t nrhs);
size_t tsqr_mi_working_r_size_f64_lstsq_rank(size_t m, size_t n, size_t nrhs);
int tsqr_mi_lstsq_rank_f64(int a_layout, int b_layout, int reorth, int refine, double rcond,
                           double* x, size_t ldx, double* r, size_t ldr, int* jpvt, int* rank,
                           const double* a, size_t lda, const double* b, size_t ldb,
                           size_t m, size_t n, size_t nrhs, void* wq, void* wr, void* stream);

/*
 * Minimum-norm rank-aware least squares in double precision (not in the reference): the arguments, operand rules, limits and states of
 * tsqr_mi_lstsq_rank_f64, and its r, jpvt, *rank and tsqr_mi_last_sweeps_f64 BITWISE on the same operands; x is the MINIMUM-NORM solution
 * of the problem truncated at the rank k of the pivoted QR: among all X that minimise ||Q1 Q1^T A X - B||_F, Q1 an orthonormal basis of
 * the retained columns A P1, the one of least ||X||_F.  That is LAPACK's dgelsy (and scipy.linalg.lstsq with lapack_driver="gelsy") at
 * the same rank.  dgelsd, numpy.linalg.lstsq and torch.linalg.lstsq truncate by SINGULAR VALUES instead: they agree with this entry
 * when A has exact rank k, and differ by about (what the truncation discards) x cond(A P1) otherwise.  Every row of x may be non-zero.
 * At full rank (k = n) x is BITWISE tsqr_mi_lstsq_rank_f64's.  Blocking, bitwise deterministic from call to call, the same bits for
 * either layout of a and of b; nothing of size m is stored, A and B are never written, and A is read exactly as often as by the basic
 * entry.
 * Method, with P = [P1 P2] the pivoting and k the rank.  (1) - (3) as tsqr_mi_lstsq_rank_f64.  (4) The dense Gram pass of the CholeskyQR
 * step runs on Zg: Zeff with column j = k .. n - 1 set to the unit vector e_jpvt[j].  The same tiles then hold G11 = (A Zeff)^T (A Zeff),
 * bit for bit as before, and G12 = (A Zeff)^T A P2, taken from A itself and not from r: the ladder's R0 is inconsistent behind an exactly
 * copied column, which is why the step exists.  The step runs unchanged: G11 = Rc^T Rc, Zeff <- Zeff inverse(Rc), A Zeff = Q1.
 * (5) One workgroup (lsq_minnorm_f64_kernel) repeats that factorisation with G12 carried along, S12 = Rc^-T G12 = Q1^T A P2, and forms
 * M = inverse(R11') S12 with inverse(R11') = P1^T Zeff upper triangular, so that S = Q1^T A P = R11' [I M]; C = I + M M^T and its plain
 * Cholesky factor (C is SPD, cond(C) <= 1 + ||M||^2); and Zmn = P pinv(S): rows jpvt[:k] are inverse(C) inverse(R11'), rows jpvt[k:] are
 * M^T inverse(C) inverse(R11'), columns >= k are zero.  (6) refine + 1 passes X <- X + Zmn (A Zeff)^T (B - A X): the passes of the basic
 * entry with Zmn in place of Zeff as the factor of the update, under the same stagnation rule.
 * Fixed point.  D = Q1^T (B - A X) = Q1^T B - S P^T X holds for the true S, because the part of A outside range(Q1) is orthogonal to
 * Q1.  Every update lies in range(Zmn) = range(P [I; M^T]), so the iteration stops at S P^T X = Q1^T B with X in range(P [I; M^T]) =
 * range((S P^T)^T): the minimum-norm solution of the truncated problem.  Errors in inverse(C) and inverse(R11') change how fast the
 * passes contract, not where they stop; errors in M change where they stop, at about cond(A P1) 2^-53.
 * Accuracy: bounded by what was measured (MI355X, refine = 1; profiles/fp64_lstsq_minnorm_accuracy.md has every figure).  On the seven
 * cases of tests/pass_refs_f64_lsq_rank.py the error ||X - X*||_F / ||X*||_F against an extended-precision minimum-norm solution of the
 * truncated problem stays within max(2 x LAPACK's, 4 n 2^-53), LAPACK's being numpy.linalg.lstsq on the same projected problem
 * (Q1^T A, Q1^T B).  Measured / LAPACK's, Gaussian B then consistent B:
 *   copied column 4096 x 16   2.5e-16 / 4.2e-15    5.3e-17 / 3.2e-15      rank 32 of 51, 1029 rows   8.1e-16 / 2.3e-15    3.7e-16 / 2.2e-15
 *   rank 1 of 33, 777 rows    7.0e-16 / 7.9e-16    1.5e-16 / 5.5e-16      rank 40 of 64, 4097 rows   9.3e-13 / 8.4e-13    1.8e-14 / 7.1e-14
 *   full rank 300 x 17        3.0e-16 / 1.1e-15    2.9e-17 / 1.3e-15      3 copied tail columns of 7 2.7e-16 / 7.5e-16    3.9e-17 / 7.7e-16
 *   one column, 65 rows       1.4e-16 / 2.5e-16    0       / 2.0e-16
 * On the copied column rows 4 and 11 of x agree to 9.6e-16 relative and ||X||_F is 0.148.  Cost over tsqr_mi_lstsq_rank_f64 (medians of
 * 50 blocking calls, arms interleaved): 0.21 ms at n = 64 and 0.02 ms at n = 16, independent of m.
 * Nothing is claimed beyond these seven cases, where cond(A P1) <= 1e4.  refine = 0 is not held to that bound (a model of the method
 * has 4.0e-10 on rank 40 of 64 with a consistent B).
 * Work space: wq of tsqr_mi_working_q_size_f64_lstsq_minnorm doubles -- the basic entry's plus Zmn, independent of m -- and wr of
 * tsqr_mi_working_r_size_f64_lstsq_minnorm doubles, the basic entry's.
 * Returns the states of tsqr_mi_lstsq_rank_f64 in its order, every text naming this entry, all of 1 and 2 before any HIP call; 3 from
 * the ladder or from the Cholesky step as there, and 3 with its own text when the Cholesky factorisation of C meets a pivot that is not
 * positive or not finite (x is then zero and *rank is written); or -(hipError_t).
 * Not provided: truncation by singular values (dgelsd's definition), n > 64, the row-partitioned and batched forms, residual norms as an
 * output.
 */
size_t tsqr_mi_working_q_size_f64_lstsq_minnorm(size_t m, size_t n, size_t nrhs);
size_t tsqr_mi_working_r_size_f64_lstsq_minnorm(size_t m, size_t n, size_t nrhs);
int tsqr_mi_lstsq_minnorm_f64(int a_layout, int b_layout, int reorth, int refine, double rcond,
                              double* x, size_t ldx, double* r, size_t ldr, int* jpvt, int* rank,
                              const double* a, size_t lda, const double* b, size_t ldb,
                              size_t m, size_t n, size_t nrhs, void* wq, void* wr, void* stream);

/*
 * Block orthogonalisation against an existing basis in double precision (not in the reference): the step of block Arnoldi, block
 * Lanczos, LOBPCG, randomised range finders and s-step Krylov methods.  V (m x k, read only) holds an orthonormal basis -- the caller
 * promises that, the call does not test it -- and W (m x n) a new block.  On return W holds Q with V^T Q = 0, Q^T Q = I and
 * W_in = V S + Q R; S is k x n and R n x n upper triangular with diag(R) >= 0 like tsqr_mi_qr_f64's, both column-major.
 * 1 <= n <= 64, 1 <= k <= 1024, k + n <= m.  v_layout, w_layout: TSQR_MI_COL_MAJOR or TSQR_MI_ROW_MAJOR for V and for W, as in
 * tsqr_mi_qr_f64_lay (ldv >= m or >= k, ldw >= m or >= n); lds >= k, ldr >= n.  W must not overlap V, S or R, nor S R.
 * Method: BCGS2 (block classical Gram-Schmidt with reorthogonalisation) with the n <= 64 ladder as the inner QR.  A round is
 * (1) Si = V^T X, the cross-Gram pass (orth_gram_f64_kernel: one wave per 64-column block of V and row slice on
 * v_mfma_f64_16x16x4_f64, the slices summed in a fixed tree); (2) X <- X - V Si in place in W (orth_update_f64_kernel, Si staged in
 * LDS in 64-row blocks); (3) X = Qi Ri by the ladder of tsqr_mi_qr_f64_lay in place, with its device passes, acceptance rule and
 * `reorth`.  passes = 1 runs one round: S = S1, R = R1.  passes = 2 runs two: S = S1 + S2 R1, R = R2 R1.  One round is NOT enough when
 * the projected block is ill conditioned or W lies close to span(V): with W = V C + 1e-6 G, cond(G) = 1e8 (1003 x 130 basis, 17 columns)
 * a model of one round leaves ||V^T Q||_F = 4.7e-9 where two leave 1.3e-15.  Use passes = 1 only where that loss is known not to matter.
 * Nothing of size m x k or m x n is allocated or stored besides W itself; the call allocates nothing.  Blocking, bitwise
 * deterministic from call to call, and Q, S, R, the state and the sweep count are BITWISE the same for all four layout pairs (a
 * row-major instance puts the same value into the register the column-major one holds it in, or swaps the MFMA operands).  Nothing at a
 * row >= m, or between the column count and the leading dimension of an operand, is read or written.
 * Accuracy (passes = 2, reorth = 0, the cases of tests/pass_refs_f64_orth.py): ||Q^T Q - I||_F <= 1e-11 and
 * ||W - V S - Q R||_F / ||W||_F <= 1e-13, the QR entry's claims restated, and ||V^T Q||_F <= max(2 x a NumPy model's on the same data,
 * 4 max(k, n) 2^-53); profiles/fp64_orth_accuracy.md has the table.
 * Work space: wq of tsqr_mi_working_q_size_f64_orth(m, k, n) doubles (the QR entry's plus R of round 2 and the work copy of S: it grows
 * with k, not with m) and wr of tsqr_mi_working_r_size_f64_orth(m, k, n) doubles (partials of the Gram passes, at most 4 Mi doubles).
 * Both are monotone in m, k and n.
 * Returns 0; 1 = TSQR_MI_ERROR_INVALID_SIZE for a null pointer, passes outside {1, 2}, a size outside the ranges above (n > 64 and
 * k > 1024 included: this entry has no state 2), a layout other than the two, or a leading dimension below its operand's extent -- all
 * before any HIP call, and no operand is touched; 3 = TSQR_MI_ERROR_NOT_FINITE, the ladder's state 3 on the projected block (this
 * includes Inf or NaN in V or W, which reach it through S); or -(hipError_t).  After state 3, W, S and R are UNDEFINED.
 * tsqr_mi_last_sweeps_f64 reports the SUM of the ladder's sweeps over the rounds, plus 100 when either took the shifted path.
 * State 0 is no test that W was independent of V: a W inside span(V) gives an orthonormal Q of rounding noise and a tiny R.  Compare
 * diag(R) with the column norms of W before using Q as a new direction.
 * Not provided: breakdown detection, k > 1024, n > 64, the row-partitioned and batched forms.
 */
size_t tsqr_mi_working_q_size_f64_orth(size_t m, size_t k, size_t n);
size_t tsqr_mi_working_r_size_f64_orth(size_t m, size_t k, size_t n);
int tsqr_mi_orth_f64(int v_layout, int w_layout, int passes, int reorth,
                     double* w, size_t ldw, double* s, size_t lds, double* r, size_t ldr,
                     const double* v, size_t ldv, size_t m, size_t k, size_t n,
                     void* wq, void* wr, void* stream);

/*
 * Wide double-precision tall-skinny QR (not in the reference): tsqr_mi_qr_f64's arguments, operand rules and states for 1 <= n <= 1024,
 * n <= m.  n <= 64 IS tsqr_mi_qr_f64 (bitwise the same results, its work-space sizes).  64 < n <= 1024: the same ladder of CholeskyQR
 * sweeps and the same acceptance rule (CholArgs64 in tsqr_f64.hip), each sweep over all n columns at once: the Gram matrix on 64-column
 * blocks, a blocked Cholesky factorisation judged over the whole matrix on the device (the shifted refactorisation also on the device),
 * Q = A inverse(R) (tsqr_f64_wide.hip).  Blocking; A is untouched unless q == a (in place, ldq == lda).
 * R: the full n x n block, exact zeros below the diagonal, a positive diagonal.  Bitwise deterministic (fixed reduction trees).
 * For cond(A) <= 1e12 and m n <= 2^26:
 *   ||Q^T Q - I||_F <= 1e-11 max(1, n / 64)  (reorth = 0),  <= 1e-12 max(1, n / 64)  (reorth = 1);  ||A - Q R||_F / ||A||_F <= 1e-13.
 * Work space: wq of tsqr_mi_working_q_size_f64_wide(m, n) doubles (six n x n block stores and a little more, independent of m), wr of
 * tsqr_mi_working_r_size_f64_wide(m, n) doubles (Gram partials, at most 8 Mi doubles for every m).
 * Returns 0, 1 (n > m, m == 0, n == 0, or a leading dimension below its operand's rows), 2 (n > 1024; tsqr_mi_last_error says so),
 * 3 = TSQR_MI_ERROR_NOT_FINITE, or -(hipError_t).  Sizes are checked before any HIP call.  tsqr_mi_last_sweeps_f64 reports this entry too.
 */
size_t tsqr_mi_working_q_size_f64_wide(size_t m, size_t n);
size_t tsqr_mi_working_r_size_f64_wide(size_t m, size_t n);
int tsqr_mi_qr_f64_wide(int reorth, double* q, size_t ldq, double* r, size_t ldr, double* a, size_t lda,
                        size_t m, size_t n, void* wq, void* wr, void* stream);

/*
 * tsqr_mi_qr_f64_wide on operands in either layout (not in the reference): a_layout is how A is stored, q_layout how Q is written, each
 * TSQR_MI_COL_MAJOR (element (i, j) at p[i + j * ld], ld >= m) or TSQR_MI_ROW_MAJOR (element (i, j) at p[i * ld + j], ld >= n -- a
 * contiguous C or torch array of shape (m, n)); the two need not agree.  R is column-major.  1 <= n <= 1024, n <= m; the work space is
 * that of tsqr_mi_working_{q,r}_size_f64_wide for every layout.  No copy of A or Q is made; nothing between n and the leading dimension
 * of a row-major operand, or behind row m, is read or written.  n <= 64 IS tsqr_mi_qr_f64_lay.
 * Method, 64 < n: the sweeps of tsqr_mi_qr_f64_wide.  Only two kernels touch A or Q -- the Gram pass and the apply pass
 * (gram_wide_f64_kernel, apply_wide_f64_kernel, tsqr_f64_wide.hip) -- and each takes the layout as a template flag; everything between
 * them works on 64 x 64 blocks of the work space.  Sweep 1 reads A in a_layout and writes Q in q_layout; later sweeps read and write Q
 * in q_layout, in place.
 * Bit-for-bit relation: the row-major kernels put the values of A into the registers the column-major kernels hold them in, on the same
 * launch plans (a column beyond n in the last block is an exact zero and is never loaded), and a row-major Q is formed by the same
 * products summed in the same order with the MFMA operands swapped, so Q -- read as a matrix --, R, the state and
 * tsqr_mi_last_sweeps_f64 are BITWISE those of tsqr_mi_qr_f64_wide on a column-major copy of the same matrix, for all four layout
 * pairs.  With both layouts TSQR_MI_COL_MAJOR the call IS tsqr_mi_qr_f64_wide (which calls this one).  Its accuracy bands, ladder and
 * non-finite rules hold unchanged.
 * In place: q == a is allowed with a_layout == q_layout and ldq == lda; Q and R must not overlap A otherwise, nor each other.
 * The row-partitioned entries (tsqr_mi_qr_f64_dist*) below stay column-major.
 * Returns what tsqr_mi_qr_f64_wide returns.  Checked in this order, before any HIP call: 1 for a layout other than 0 or 1; 1 for n > m,
 * m == 0, n == 0, ldr < n or a leading dimension below m (column-major) or n (row-major); 2 for n > 1024 (tsqr_mi_last_error says so);
 * 1 for q == a with different layouts or ldq != lda.
 */
int tsqr_mi_qr_f64_wide_lay(int a_layout, int q_layout, int reorth, double* q, size_t ldq, double* r, size_t ldr, double* a, size_t lda,
                            size_t m, size_t n, void* wq, void* wr, void* stream);

/*
 * Row-partitioned double-precision QR (not in the reference): tsqr_mi_qr_f64_wide for a matrix whose rows are spread over the ranks, one
 * call per rank, 1 <= n <= 1024 (n <= 64 runs the sweeps of tsqr_mi_qr_f64, wider matrices those of tsqr_mi_qr_f64_wide).  Every rank
 * passes its own row block: m_local may differ between ranks, 1 <= m_local on every rank, and m_local < n is fine.  The GLOBAL row count
 * must be >= n: that is the caller's contract and is not checked.  A rank that returns early -- 1 for an empty block, say -- leaves the
 * others waiting in their exchange, so every rank must pass arguments that get past the checks below, or none.
 * Each sweep of the ladder has ONE exchange, enqueued on `stream` between the Gram reduction and the Cholesky step, with no host wait
 * that the one-GPU call does not have: the all-reduce (sum, in place) of the Gram matrix and the local row count behind it --
 * ntri * 256 + 1 <= 2561 doubles for n <= 64, npairs * 4096 + 1 doubles (nb = ceil(n / 64), npairs = nb (nb + 1) / 2; 4.4 MB at n = 1024)
 * beyond.  Every rank then factors the same bits, and the Cholesky step evaluates the acceptance rule (CholArgs64, tsqr_f64.hip) on the
 * device from the summed, global row count: the verdicts, hence the number of sweeps and of exchanges, agree on all ranks by
 * construction, and a NaN anywhere reaches every rank through the sum.  r is bitwise identical on all ranks on return.
 * For cond(A) <= 1e12 and m_global n <= 2^26, on the stacked matrix:
 *   ||Q^T Q - I||_F <= 1e-11 max(1, n / 64)  (reorth = 0),  <= 1e-12 max(1, n / 64)  (reorth = 1);  ||A - Q R||_F / ||A||_F <= 1e-13.
 * Work space: tsqr_mi_working_{q,r}_size_f64_dist(m_local, n, nranks) doubles (never below the sizes of tsqr_mi_qr_f64_wide).
 * Transport, as for tsqr_mi_qr_f32_dist (the communicator and ncclAllReduce must come from ONE RCCL instance):
 * tsqr_mi_qr_f64_dist_fn: the caller's ncclComm_t and the address of ncclAllReduce of the library that created it;
 * tsqr_mi_qr_f64_dist:    a caller that links RCCL: ncclAllReduce from the global symbol scope, as tsqr_mi_qr_f32_dist;
 * tsqr_mi_qr_f64_dist_cb: a caller-supplied all-reduce (blocking or stream-ordered, in place sum), e.g. torch.distributed.
 * Returns the states of tsqr_mi_qr_f64_wide: 0, 1 (m_local == 0, n == 0, or a leading dimension below its operand's rows -- but not
 * n > m_local), 2 (n > 1024, or no all-reduce to call), 3 = TSQR_MI_ERROR_NOT_FINITE (on every rank alike), or -(hipError_t); 1 and 2
 * come with a tsqr_mi_last_error text and are decided before any HIP call and before any collective.  tsqr_mi_last_sweeps_f64 reports
 * these entries too.
 */
size_t tsqr_mi_working_q_size_f64_dist(size_t m_local, size_t n, int nranks);
size_t tsqr_mi_working_r_size_f64_dist(size_t m_local, size_t n, int nranks);
int tsqr_mi_qr_f64_dist(int reorth, double* q, size_t ldq, double* r, size_t ldr, double* a, size_t lda,
                        size_t m_local, size_t n, void* wq, void* wr,
                        void* nccl_comm, int nranks, void* stream);
int tsqr_mi_qr_f64_dist_fn(int reorth, double* q, size_t ldq, double* r, size_t ldr, double* a, size_t lda,
                           size_t m_local, size_t n, void* wq, void* wr,
                           void* nccl_comm, void* nccl_allreduce_fn, int nranks, void* stream);
int tsqr_mi_qr_f64_dist_cb(int reorth, double* q, size_t ldq, double* r, size_t ldr, double* a, size_t lda,
                           size_t m_local, size_t n, void* wq, void* wr,
                           tsqr_mi_allreduce_f64_cb allreduce, void* user, int nranks, void* stream);

/* Harness support (reference src/validation.cu:43-127, src/test.cu:147-165): accuracy metrics evaluated on the device in fp64.
 * scratch: n*n + 8 doubles of device memory.  out_host[0..4] = ||Q^T Q - I||_F^2, its diagonal part, its off-diagonal part,
 * ||Q R - A||_F^2, ||A||_F^2 (the last two only when r and a are given).  gram_out_host: optional n*n doubles receiving Q^T Q. */
int tsqr_mi_validate_f32(const float* q, size_t ldq, const float* r, size_t ldr, const float* a, size_t lda,
                         size_t m, size_t n, double* scratch, double* out_host, double* gram_out_host, void* stream);

/* Optional timing of the engine's kernels with HIP events recorded on the caller's stream.  Classes:
 * 0 first fold level (streams A), 1 fold-tree levels, 2 triangular inverse, 3 apply (Q = A*inverse(R)),
 * 4 inter-panel coupling (n > 64), 5 other, 6 Gram matrix, 7 Gram reduction + Cholesky + inverse.  read() returns accumulated milliseconds and launch counts
 * since enable(1); call it after the blocking qr call(s). */
void tsqr_mi_profile_enable(int on);
int tsqr_mi_profile_read(double* ms, long* launches, int max_classes);

/* R-factor engine policy (Q is always formed by apply: Q = A * inverse(R) on the MFMA units).
 *   0 auto (default), every mode: Gram engine, R = chol(A^T A).  First the bf16x3-split MFMA Gram matrix (exact products, fp64
 *                     accumulation across K-steps, memory-bound), accepted when every Cholesky pivot keeps >= 2^-5 of its diagonal
 *                     entry and the scaled conditioning S = ||D inverse(R)||_F^2 / n stays below min(128, max(4, 0.12 sqrt(rows)));
 *                     else the fp64-MFMA Gram matrix, accepted down to a pivot ratio of 2^-40 (cond(A) up to ~1e6); else the
 *                     shifted Cholesky QR step on that fp64 Gram matrix + one plain fp64 sweep in place; Householder TSQR last.
 *                     The compute mode selects the MFMA engine of the apply pass (exact fp32 / bf16x3 split / single fp16 product).
 *   1 always Householder TSQR.   2 always fp64 Gram (no fallback).   3 always bf16-split Gram (no check; tests only).
 *   4 auto without the bf16-split level.
 *   5 auto, but 64 < n <= 128 goes straight to the 64-column panel path (policy 0 first tries all n columns as ONE Cholesky-QR
 *     panel at the bf16-split level: one pass for the 128 x 128 Gram matrix, one for Q; same acceptance rule; A stays intact when it
 *     is accepted, and when it is rejected the panel path runs on the untouched input).
 * tsqr_mi_last_engine(): 0 Householder, 1 fp64 Gram, 2 Gram rejected -> Householder, 3 bf16-split Gram,
 * 4 Gram rejected -> shifted Cholesky QR (shifted fp64 Cholesky + one plain fp64 sweep in place),
 * 5 bf16-split Gram over all n <= 128 columns at once (one panel). */
void tsqr_mi_set_policy(int policy);
int tsqr_mi_last_engine(void);

/* tuning knobs (0 = keep default): waves targeted by the first fold level, chunks folded per wave on tree levels */
void tsqr_mi_set_tuning(int level0_waves, int tree_chunks_per_wave);
/* waves of the Gram kernel / of the apply kernel (apply: persistent grid of apply_waves/4 workgroups; default = all that are resident
 * at once).  Work-buffer sizes follow the Gram setting: set it before allocating. */
void tsqr_mi_set_tuning2(int gram_waves, int apply_waves);
/* Load policy of A in the two streaming passes of a full 64-column call (m a multiple of 128, at most 2^20 rows, 16-byte aligned
 * columns: the Gram block kernel and the 64-row apply kernel).  0 auto, 1 cache-allocating loads, 2 streamed: nontemporal loads in both
 * passes, for devices whose nontemporal Q stores allocate in the memory-side cache and displace A between calls.  Auto measures the two
 * once per process and device on the first blocking fp32_tc_cor call of at least 128 MiB that is out of place (a few call times, on
 * the caller's operands), takes the streamed loads only when they are clearly faster, and uses the cache-allocating loads everywhere
 * else; calls in flight (submit, and the loop and batch entries beyond loop depth 1) never measure.  The policy changes no bit of Q, R or the verdicts.  Process-wide; the
 * environment variable TSQR_MI_LOAD_POLICY sets the initial value. */
void tsqr_mi_set_load_policy(int p);
/* the policy the last such call used (1 or 2); 0 before the first one */
int tsqr_mi_get_load_policy(void);

#ifdef __cplusplus
}
#endif
#endif /* TSQR_MI_H */

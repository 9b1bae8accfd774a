"""Python mirror of the reference's host interface for the tall-skinny QR path.

Same names and argument meaning as reference src/blockqr.hpp:
  compute_mode (:12-23), tsqr_colmun_size (:25), state_t codes (:27-29),
  get_working_{q,r,l}_size (:55-57), buffer (:59-140), qr (:142-175).

Everything here is plumbing over the C ABI of csrc/libtsqr_mi.so (include/tsqr_mi.h): the
arithmetic lives in hand-written HIP kernels.  There is NO CPU fallback: importing works without
the library (so sizes/enums can be inspected), but any call that needs it raises RuntimeError.
torch is used only to own device memory and streams.
"""
import ctypes
import enum
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# TSQR_MI_LIB: another build of the library (same-box A/B of two builds, tools/r04_ab.sh); default: the in-tree one
LIB_PATH = os.environ.get("TSQR_MI_LIB") or os.path.join(_HERE, "csrc", "libtsqr_mi.so")


class compute_mode(enum.IntEnum):
    """mtk::qr::compute_mode, reference src/blockqr.hpp:12-23 (same order)."""
    fp16_notc = 0
    fp16_tc_nocor = 1
    fp32_notc = 2
    fp32_tc_cor = 3
    fp32_tc_nocor = 4
    mixed_tc_cor_emu = 5
    tf32_tc_cor = 6
    tf32_tc_cor_emu = 7
    tf32_tc_nocor = 8
    tf32_tc_nocor_emu = 9


tsqr_colmun_size = 16                 # reference src/blockqr.hpp:25 (name kept, typo included)
success_factorization = 0             # reference src/blockqr.hpp:28
error_invalid_matrix_size = 1         # reference src/blockqr.hpp:29
error_unsupported_mode = 2            # new: modes without a gfx950 implementation
error_not_finite = 3                  # new, qr_f64 only: A holds an Inf or NaN
error_no_convergence = 4              # new, svd_f64 only: the Jacobi iteration reached its cap of 30 sweeps

COL_MAJOR, ROW_MAJOR = 0, 1              # TSQR_MI_COL_MAJOR, TSQR_MI_ROW_MAJOR: the layout arguments of the *_lay entries


class Ticket(ctypes.Structure):
    """tsqr_mi_ticket (include/tsqr_mi.h): one call in flight between submit() and finish()."""
    _fields_ = [("state", ctypes.c_int), ("pending", ctypes.c_int), ("slot", ctypes.c_int), ("own_flag", ctypes.c_int), ("seq", ctypes.c_uint),
                ("verdict", ctypes.c_uint), ("scond", ctypes.c_float), ("mode", ctypes.c_int), ("reorth", ctypes.c_int),
                ("q", ctypes.c_void_p), ("r", ctypes.c_void_p), ("a", ctypes.c_void_p),
                ("ldq", ctypes.c_size_t), ("ldr", ctypes.c_size_t), ("lda", ctypes.c_size_t), ("m", ctypes.c_size_t), ("n", ctypes.c_size_t),
                ("wq", ctypes.c_void_p), ("wr", ctypes.c_void_p), ("stream", ctypes.c_void_p),
                ("h_wl", ctypes.c_void_p), ("words", ctypes.c_void_p), ("words_dev", ctypes.c_void_p)]

    def __del__(self):
        # The library holds the address of a ticket in flight, so one must not go away unfinished -- but finish belongs to the thread
        # that submitted it (include/tsqr_mi.h), and a finaliser runs wherever the collector happens to be, possibly at interpreter
        # shutdown: finish here only on the submitting thread of a live interpreter; otherwise say what went wrong.
        if self.pending == 0:                          # (1: in flight; 2: verdict read -- the library still lists it until finish)
            return
        import sys
        import threading
        if _lib is not None and not sys.is_finalizing() and getattr(self, "_tid", None) == threading.get_ident():
            _lib.tsqr_mi_qr_f32_finish(ctypes.byref(self))
        else:
            import warnings
            warnings.warn("tsqr_gpu_amd: a Ticket in flight was dropped on another thread (or at shutdown) without finish(); "
                          "call blockqr.finish(ticket) on the submitting thread", ResourceWarning, stacklevel=2)


FP16_MODES = (compute_mode.fp16_notc, compute_mode.fp16_tc_nocor)     # io type half in the reference (src/tsqr.hpp:38-39)

def _c_signatures():
    """{symbol: (restype, argtypes)} of the C ABI (include/tsqr_mi.h), in the header's order of introduction."""
    sz, vp, ci = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int
    pu, pd, pt = ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(Ticket)
    qr32 = [ci, ci, vp, sz, vp, sz, vp, sz, sz, sz, vp, vp, vp, vp, vp, vp]
    # (mode, reorth, q, ldq, r, ldr, a, lda, m_local, n, wq, wr, gather, <transport: 3 x void*>, nranks, stream)
    dist32 = [ci, ci, vp, sz, vp, sz, vp, sz, sz, sz, vp, vp, vp, vp, vp, vp, ci, vp]
    batch32 = [ci, ci, ci, vp, sz, vp, sz, vp, sz, sz, sz, vp, vp, vp, vp, vp, vp, vp]
    dist_batch32 = [ci] + dist32 + [vp]                # (count, ..., states)
    qr64 = [ci, vp, sz, vp, sz, vp, sz, sz, sz, vp, vp, vp]
    r64 = [ci, vp, sz, vp, sz, sz, sz, vp, vp, vp]
    lstsq64 = [ci, ci, vp, sz, vp, sz, vp, sz, vp, sz, sz, sz, sz, vp, vp, vp]
    dist64 = qr64[:-1]                                 # (reorth, q, ldq, r, ldr, a, lda, m_local, n, wq, wr, <transport>, nranks, stream)
    return {
        "tsqr_mi_version": (ci, []), "tsqr_mi_last_error": (ctypes.c_char_p, []),
        "tsqr_mi_working_q_size": (sz, [sz, sz]), "tsqr_mi_working_r_size": (sz, [sz, sz]), "tsqr_mi_working_l_size": (sz, [sz]),
        "tsqr_mi_working_reorth_size": (sz, [sz]), "tsqr_mi_batch_size_log2": (sz, [sz]), "tsqr_mi_batch_size": (sz, [sz]),
        "tsqr_mi_qr_f32": (ci, qr32), "tsqr_mi_local_r_f32": (ci, [vp, sz, vp, sz, sz, sz, vp, vp, vp]),
        "tsqr_mi_apply_rinv_f32": (ci, [ci, vp, sz, vp, sz, vp, sz, sz, sz, vp, vp]), "tsqr_mi_rmul_f32": (ci, [vp, sz, vp, sz, sz, vp, vp]),
        "tsqr_mi_qr_f32_dist": (ci, [ci, ci, vp, sz, vp, sz, vp, sz, sz, sz, vp, vp, vp, vp, ci, vp]),
        "tsqr_mi_set_tuning": (None, [ci, ci]), "tsqr_mi_profile_enable": (None, [ci]),
        "tsqr_mi_profile_read": (ci, [pd, ctypes.POINTER(ctypes.c_long), ci]),
        "tsqr_mi_set_policy": (None, [ci]), "tsqr_mi_last_engine": (ci, []), "tsqr_mi_set_tuning2": (None, [ci, ci]),
        "tsqr_mi_gram_elems": (sz, [sz]), "tsqr_mi_gram_f32": (ci, [ci, vp, vp, sz, sz, sz, vp, vp, vp]),
        "tsqr_mi_chol_f32": (ci, [ci, vp, sz, vp, sz, sz, vp, pu, vp]), "tsqr_mi_chol_status": (ci, [vp, sz, sz, pu, vp]),
        "tsqr_mi_stream_wait": (ci, [vp]), "tsqr_mi_apply_z_f32": (ci, [ci, vp, sz, vp, sz, sz, sz, vp, vp]),
        "tsqr_mi_validate_f32": (ci, [vp, sz, vp, sz, vp, sz, sz, sz, vp, pd, pd, vp]),
        "tsqr_mi_working_q_size_dist": (sz, [sz, sz, ci]), "tsqr_mi_working_r_size_dist": (sz, [sz, sz, ci]),
        "tsqr_mi_qr_f32_dist_cb": (ci, dist32),
        "tsqr_mi_qr_f32_loop": (ci, [ci] + qr32), "tsqr_mi_qr_f32_dist_fn": (ci, dist32),
        "tsqr_mi_qr_f32_dist_fn_loop": (ci, [ci] + dist32), "tsqr_mi_qr_f32_dist_cb_loop": (ci, [ci] + dist32),
        "tsqr_mi_qr_f16": (ci, qr32), "tsqr_mi_qr_f16_loop": (ci, [ci] + qr32),
        "tsqr_mi_working_q_size_f16": (sz, [sz, sz]), "tsqr_mi_working_r_size_f16": (sz, [sz, sz]),
        "tsqr_mi_qr_f32_submit": (ci, qr32 + [pt]), "tsqr_mi_qr_f32_finish": (ci, [pt]), "tsqr_mi_set_loop_depth": (None, [ci]),
        "tsqr_mi_qr_f32_batch": (ci, batch32), "tsqr_mi_qr_f16_batch": (ci, batch32),
        "tsqr_mi_qr_f32_dist_fn_batch": (ci, dist_batch32), "tsqr_mi_qr_f32_dist_cb_batch": (ci, dist_batch32),
        "tsqr_mi_qr_f64": (ci, qr64), "tsqr_mi_working_q_size_f64": (sz, [sz, sz]), "tsqr_mi_working_r_size_f64": (sz, [sz, sz]),
        "tsqr_mi_last_sweeps_f64": (ci, []),
        "tsqr_mi_qr_f64_wide": (ci, qr64), "tsqr_mi_working_q_size_f64_wide": (sz, [sz, sz]), "tsqr_mi_working_r_size_f64_wide": (sz, [sz, sz]),
        "tsqr_mi_working_q_size_f64_dist": (sz, [sz, sz, ci]), "tsqr_mi_working_r_size_f64_dist": (sz, [sz, sz, ci]),
        "tsqr_mi_qr_f64_dist": (ci, dist64 + [vp, ci, vp]), "tsqr_mi_qr_f64_dist_fn": (ci, dist64 + [vp, vp, ci, vp]),
        "tsqr_mi_qr_f64_dist_cb": (ci, dist64 + [vp, vp, ci, vp]),
        "tsqr_mi_r_f64": (ci, r64), "tsqr_mi_working_q_size_f64_r": (sz, [sz, sz]), "tsqr_mi_working_r_size_f64_r": (sz, [sz, sz]),
        "tsqr_mi_lstsq_f64": (ci, lstsq64),
        "tsqr_mi_working_q_size_f64_lstsq": (sz, [sz, sz, sz]), "tsqr_mi_working_r_size_f64_lstsq": (sz, [sz, sz, sz]),
        "tsqr_mi_r_f64_lay": (ci, [ci] + r64), "tsqr_mi_lstsq_f64_lay": (ci, [ci, ci] + lstsq64),
        "tsqr_mi_qr_f64_lay": (ci, [ci, ci] + qr64), "tsqr_mi_qr_f64_wide_lay": (ci, [ci, ci] + qr64),
        "tsqr_mi_working_q_size_f64_svd": (sz, [sz, sz, ci]), "tsqr_mi_working_r_size_f64_svd": (sz, [sz, sz, ci]),
        # (a_layout, u_layout, jobu, reorth, u, ldu, s, v, ldv, a, lda, m, n, wq, wr, stream)
        "tsqr_mi_svd_f64": (ci, [ci, ci, ci, ci, vp, sz, vp, vp, sz, vp, sz, sz, sz, vp, vp, vp]),
        "tsqr_mi_last_jacobi_sweeps_f64": (ci, []),
        "tsqr_mi_working_q_size_f64_qrcp": (sz, [sz, sz, ci]), "tsqr_mi_working_r_size_f64_qrcp": (sz, [sz, sz, ci]),
        # (a_layout, q_layout, jobq, reorth, q, ldq, r, ldr, jpvt, a, lda, m, n, wq, wr, stream)
        "tsqr_mi_qrcp_f64": (ci, [ci, ci, ci, ci, vp, sz, vp, sz, vp, vp, sz, sz, sz, vp, vp, vp]),
        "tsqr_mi_working_q_size_f64_lstsq_rank": (sz, [sz, sz, sz]), "tsqr_mi_working_r_size_f64_lstsq_rank": (sz, [sz, sz, sz]),
        # (a_layout, b_layout, reorth, refine, rcond, x, ldx, r, ldr, jpvt, rank, a, lda, b, ldb, m, n, nrhs, wq, wr, stream)
        "tsqr_mi_lstsq_rank_f64": (ci, [ci, ci, ci, ci, ctypes.c_double, vp, sz, vp, sz, vp, ctypes.POINTER(ci), vp, sz, vp, sz, sz, sz, sz,
                                        vp, vp, vp]),
        "tsqr_mi_working_q_size_f64_lstsq_minnorm": (sz, [sz, sz, sz]), "tsqr_mi_working_r_size_f64_lstsq_minnorm": (sz, [sz, sz, sz]),
        # (the arguments of tsqr_mi_lstsq_rank_f64)
        "tsqr_mi_lstsq_minnorm_f64": (ci, [ci, ci, ci, ci, ctypes.c_double, vp, sz, vp, sz, vp, ctypes.POINTER(ci), vp, sz, vp, sz, sz, sz, sz,
                                           vp, vp, vp]),
        "tsqr_mi_set_load_policy": (None, [ci]), "tsqr_mi_get_load_policy": (ci, []),
        "tsqr_mi_working_q_size_f64_orth": (sz, [sz, sz, sz]), "tsqr_mi_working_r_size_f64_orth": (sz, [sz, sz, sz]),
        # (v_layout, w_layout, passes, reorth, w, ldw, s, lds, r, ldr, v, ldv, m, k, n, wq, wr, stream)
        "tsqr_mi_orth_f64": (ci, [ci, ci, ci, ci, vp, sz, vp, sz, vp, sz, vp, sz, sz, sz, sz, vp, vp, vp]),
    }


C_SIGNATURES = _c_signatures()
C_ABI_SYMBOLS = list(C_SIGNATURES)
# TSQR_MI_LIB may name an older build for an A/B of the entries both have: these, the newest, may be missing from it
OPTIONAL_SYMBOLS = {
    "tsqr_mi_working_q_size_f64_dist", "tsqr_mi_working_r_size_f64_dist", "tsqr_mi_qr_f64_dist", "tsqr_mi_qr_f64_dist_fn", "tsqr_mi_qr_f64_dist_cb",
    "tsqr_mi_r_f64", "tsqr_mi_working_q_size_f64_r", "tsqr_mi_working_r_size_f64_r",
    "tsqr_mi_lstsq_f64", "tsqr_mi_working_q_size_f64_lstsq", "tsqr_mi_working_r_size_f64_lstsq",
    "tsqr_mi_r_f64_lay", "tsqr_mi_lstsq_f64_lay", "tsqr_mi_qr_f64_lay", "tsqr_mi_qr_f64_wide_lay",
    "tsqr_mi_working_q_size_f64_svd", "tsqr_mi_working_r_size_f64_svd", "tsqr_mi_svd_f64", "tsqr_mi_last_jacobi_sweeps_f64",
    "tsqr_mi_working_q_size_f64_qrcp", "tsqr_mi_working_r_size_f64_qrcp", "tsqr_mi_qrcp_f64",
    "tsqr_mi_working_q_size_f64_lstsq_rank", "tsqr_mi_working_r_size_f64_lstsq_rank", "tsqr_mi_lstsq_rank_f64",
    "tsqr_mi_working_q_size_f64_lstsq_minnorm", "tsqr_mi_working_r_size_f64_lstsq_minnorm", "tsqr_mi_lstsq_minnorm_f64",
    "tsqr_mi_set_load_policy", "tsqr_mi_get_load_policy",
    "tsqr_mi_working_q_size_f64_orth", "tsqr_mi_working_r_size_f64_orth", "tsqr_mi_orth_f64"}

_lib = None


def lib():
    """Load libtsqr_mi.so; raise loudly if it was not built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "tsqr_gpu_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C tsqr_gpu_amd/csrc`. There is no CPU fallback." % LIB_PATH)
    # torch first: its bundled HIP runtime must be the one libtsqr_mi.so binds to (loading the library before torch
    # pulls the system libamdhip64 and the process ends up with two runtimes -- "no ROCm-capable device")
    import torch  # noqa: F401
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in C_SIGNATURES.items():
        if name in OPTIONAL_SYMBOLS and not hasattr(L, name):
            continue
        fn = getattr(L, name)                          # (AttributeError: a symbol every build must have is missing)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def last_error():
    return lib().tsqr_mi_last_error().decode()


# ---- mtk::qr::get_working_*_size (reference src/blockqr.hpp:55-57) ----------------------------------
def get_working_q_size(m, n):
    return lib().tsqr_mi_working_q_size(m, n)


def get_working_r_size(m, n):
    return lib().tsqr_mi_working_r_size(m, n)


def get_working_l_size(m):
    return lib().tsqr_mi_working_l_size(m)


def get_batch_size_log2(m):
    """mtk::tsqr::get_batch_size_log2, reference src/tsqr.cu:39-41."""
    return lib().tsqr_mi_batch_size_log2(m)


def get_batch_size(m):
    return lib().tsqr_mi_batch_size(m)


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _call_args(q, ldq, r, ldr, a, lda, m, n, bf, stream, mode, reorthogonalize, fp32_only=None):
    """What qr, submit, bind and bind_loop share: mode and reorth (the buffer's unless given), the stream (the current one unless given)
    and the sixteen arguments of tsqr_mi_qr_f32, marshalled once.  fp32_only: the TypeError text for an fp16 I/O mode."""
    import torch
    mode = bf.mode if mode is None else compute_mode(mode)
    reorth = bf.reorthogonalize if reorthogonalize is None else bool(reorthogonalize)
    if fp32_only and mode in FP16_MODES:
        raise TypeError(fp32_only)
    if stream is None:
        stream = torch.cuda.current_stream()
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    args = (ci(int(mode)), ci(int(reorth)), vp(_ptr(q)), sz(ldq), vp(_ptr(r)), sz(ldr), vp(_ptr(a)), sz(lda), sz(m), sz(n),
            vp(_ptr(bf.dwq)), vp(_ptr(bf.dwr)), vp(_ptr(bf.dw_reorth_r)), vp(_ptr(bf.dl)), vp(_ptr(bf.hl)), vp(stream.cuda_stream))
    return mode, stream, args


class buffer:
    """mtk::qr::buffer<mode, Reorthogonalize>, reference src/blockqr.hpp:59-140.

    Fields dwq, dwr, dw_reorth_r, dl (device) and hl (pinned host) as in the reference;
    allocate() twice raises RuntimeError like the reference's std::runtime_error (:77-79).
    """

    def __init__(self, mode=compute_mode.fp32_tc_cor, reorthogonalize=False, device="cuda"):
        self.mode = compute_mode(mode)
        self.reorthogonalize = bool(reorthogonalize)
        self.device = device
        self.dwq = self.dwr = self.dw_reorth_r = self.dl = self.hl = None
        self.total_memory_size = 0

    def allocate(self, m, n):
        import torch
        if self.dwq is not None or self.dwr is not None or self.dl is not None or self.hl is not None:
            raise RuntimeError("The buffer has been already allocated")
        wq, wr, wl = get_working_q_size(m, n), get_working_r_size(m, n), get_working_l_size(m)
        if self.mode in FP16_MODES:                          # room for the widened A, Q and R of the fp16 entry (in 4-byte units)
            wq, wr = lib().tsqr_mi_working_q_size_f16(m, n), lib().tsqr_mi_working_r_size_f16(m, n)
        self.dwq = torch.empty(max(wq, 1), dtype=torch.float32, device=self.device)
        self.dwr = torch.empty(max(wr, 1), dtype=torch.float32, device=self.device)
        self.dl = torch.empty(max(wl, 1), dtype=torch.int32, device=self.device)
        self.hl = torch.empty(max(wl, 1), dtype=torch.int32).pin_memory()
        self.total_memory_size = 4 * (wq + wr + wl)
        if self.reorthogonalize:
            ro = lib().tsqr_mi_working_reorth_size(m)
            self.dw_reorth_r = torch.empty(max(ro, 1), dtype=torch.float32, device=self.device)
            self.total_memory_size += 4 * ro

    def destroy(self):
        self.dwq = self.dwr = self.dw_reorth_r = self.dl = self.hl = None

    def get_device_memory_size(self):
        return self.total_memory_size


def qr(q, ldq, r, ldr, a, lda, m, n, bf, stream=None, mode=None, reorthogonalize=None):
    """mtk::qr::qr<mode, Reorthogonalize>(q, ldq, r, ldr, a, lda, m, n, buffer, handle).

    q, r, a: float32 torch tensors on the GPU holding column-major data (any shape; only data_ptr is
    used) -- float16 tensors for the two fp16 I/O modes (io type half in the reference, src/tsqr.hpp:38-39; the buffer must have
    been allocated for such a mode).  `stream` (torch.cuda.Stream or None = current) takes the place of the cublasHandle_t, whose
    only role in the reference is to carry the stream (src/blockqr.cu:58-59).  Blocking, returns state_t.
    Runtime failures raise RuntimeError (the reference throws std::runtime_error from CUTF_CHECK_ERROR).
    """
    import torch
    mode, stream, args = _call_args(q, ldq, r, ldr, a, lda, m, n, bf, stream, mode, reorthogonalize)
    if mode in FP16_MODES:
        for t in (q, r, a):
            if t is not None and t.dtype != torch.float16:
                raise TypeError("%s takes float16 tensors (io type half, reference src/tsqr.hpp:38-39)" % mode.name)
        if bf.mode not in FP16_MODES:
            raise RuntimeError("the buffer was allocated for %s: an fp16 mode needs the larger work space of its own allocate()" % bf.mode.name)
        fn, name = lib().tsqr_mi_qr_f16, "tsqr_mi_qr_f16"
    else:
        fn, name = lib().tsqr_mi_qr_f32, "tsqr_mi_qr_f32"
    st = fn(*args)
    if st < 0:
        raise RuntimeError("%s failed: %s" % (name, last_error()))
    return st


def submit(q, ldq, r, ldr, a, lda, m, n, bf, stream=None, mode=None, reorthogonalize=None):
    """Stream-asynchronous qr() (tsqr_mi_qr_f32_submit): enqueues the call's first attempt and returns a ticket; finish(ticket) waits,
    completes the ladder for a rejected matrix and returns state_t.  Up to two calls of a thread are in flight; tickets are finished in
    submission order by the submitting thread.  fp32 I/O modes."""
    import threading
    mode, stream, args = _call_args(q, ldq, r, ldr, a, lda, m, n, bf, stream, mode, reorthogonalize, fp32_only="submit() takes the fp32 I/O modes")
    t = Ticket()
    t._keep = (q, r, a, bf, stream)
    t._tid = threading.get_ident()
    st = lib().tsqr_mi_qr_f32_submit(*args, ctypes.byref(t))
    if st < 0:
        raise RuntimeError("tsqr_mi_qr_f32_submit failed: %s" % last_error())
    return t


def finish(ticket):
    st = lib().tsqr_mi_qr_f32_finish(ctypes.byref(ticket))
    if st < 0:
        raise RuntimeError("tsqr_mi_qr_f32_finish failed: %s" % last_error())
    return st


def set_loop_depth(depth):
    """The loop entries (bind_loop): 1 = plain blocking calls, 2 = two calls in flight, 3 (default) = also the chained schedule for full
    64-column matrices of up to 2^20 rows (the R-factor chain of call i inside the Gram launch of call i + 1)."""
    lib().tsqr_mi_set_loop_depth(int(depth))


def bind(q, ldq, r, ldr, a, lda, m, n, bf, stream=None, mode=None, reorthogonalize=None):
    """qr() with every argument marshalled once: returns a zero-argument callable that issues exactly one C-ABI call
    (tsqr_mi_qr_f32) per invocation -- what a C++ caller's loop looks like, without per-call Python/ctypes conversions.
    The tensors, the buffer and the stream must stay alive and unchanged while the callable is in use."""
    mode, stream, args = _call_args(q, ldq, r, ldr, a, lda, m, n, bf, stream, mode, reorthogonalize)
    fn = lib().tsqr_mi_qr_f32
    keep = (q, r, a, bf, stream)

    def call():
        st = fn(*args)
        if st < 0:
            raise RuntimeError("tsqr_mi_qr_f32 failed: %s" % last_error())
        return st
    call._keep = keep
    return call


def bind_loop(q, ldq, r, ldr, a, lda, m, n, bf, stream=None, mode=None, reorthogonalize=None):
    """Like bind(), but the callable takes a count k and issues k calls from ONE C loop (tsqr_mi_qr_f32_loop): the reference's speed
    protocol (src/test.cu:299-309) without interpreter time between the calls.  The fp32 loop keeps two calls in flight (submit /
    finish) unless set_loop_depth(1)."""
    mode, stream, args = _call_args(q, ldq, r, ldr, a, lda, m, n, bf, stream, mode, reorthogonalize)
    fn = lib().tsqr_mi_qr_f16_loop if mode in FP16_MODES else lib().tsqr_mi_qr_f32_loop      # (float16 tensors for the fp16 I/O modes)
    keep = (q, r, a, bf, stream)

    def call(k=1):
        st = fn(ctypes.c_int(int(k)), *args)
        if st < 0:
            raise RuntimeError("tsqr_mi_qr_f32 failed: %s" % last_error())
        return st
    call._keep = keep
    return call


def check_batch_operands(qs, ldq, rs, ldr, as_, lda, m, n, half=False):
    """Every tensor of a batch before anything touches the GPU (the C side reads raw pointers): float32 (float16 for the fp16 I/O modes),
    on the GPU, a leading dimension of at least its rows, and room for the whole column-major operand, (n - 1) ld + rows elements.
    Raises TypeError or ValueError."""
    import torch
    want = torch.float16 if half else torch.float32
    if not (len(qs) == len(rs) == len(as_)):
        raise ValueError("qr_batch: q, r and a must name the same number of matrices")
    ops = (("q", qs, ldq, m), ("r", rs, ldr, n), ("a", as_, lda, m))
    for name, ts, ld, rows in ops:
        for i, t in enumerate(ts):
            if t.dtype != want:
                raise TypeError("qr_batch: %s[%d] is %s, this mode takes %s" % (name, i, t.dtype, want))
    for name, ts, ld, rows in ops:
        if ld < rows:
            raise ValueError("qr_batch: ld%s = %d is smaller than the %d rows of %s" % (name, ld, rows, name))
        need = (n - 1) * ld + rows if n > 0 else 0
        for i, t in enumerate(ts):
            if t.numel() < need:
                raise ValueError("qr_batch: %s[%d] holds %d elements, an operand of %d x %d with ld %d needs %d" % (name, i, t.numel(), rows, n, ld, need))
    for name, ts, ld, rows in ops:
        for i, t in enumerate(ts):
            if not t.is_cuda:
                raise TypeError("qr_batch: %s[%d] is not a GPU tensor" % (name, i))


def bind_batch(qs, ldq, rs, ldr, as_, lda, m, n, bf, stream=None, mode=None, reorthogonalize=None):
    """mtk::qr::qr_batch (tsqr_mi_qr_f32_batch / tsqr_mi_qr_f16_batch): qs, rs, as_ are equally long sequences of float32 tensors
    (float16 for the two fp16 I/O modes), one (q, r, a) triple per matrix, all of the shape m x n with the shared leading dimensions.  Returns a callable: call() factors every matrix (blocking) and
    returns (first non-zero state, [state of every call]).  The tensors, the buffer and the stream must stay alive while it is in use."""
    import torch
    mode = bf.mode if mode is None else compute_mode(mode)
    reorth = bf.reorthogonalize if reorthogonalize is None else bool(reorthogonalize)
    if mode in FP16_MODES and bf.mode not in FP16_MODES:
        raise RuntimeError("the buffer was allocated for %s: an fp16 mode needs the larger work space of its own allocate()" % bf.mode.name)
    check_batch_operands(qs, ldq, rs, ldr, as_, lda, m, n, half=mode in FP16_MODES)   # (float16 for the fp16 modes: io type half, reference src/tsqr.hpp:38-39)
    if stream is None:
        stream = torch.cuda.current_stream()
    count = len(as_)
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    arr = lambda ts: (vp * max(count, 1))(*[t.data_ptr() for t in ts])
    pq, pr, pa = arr(qs), arr(rs), arr(as_)
    states = (ci * max(count, 1))()
    fn = lib().tsqr_mi_qr_f16_batch if mode in FP16_MODES else lib().tsqr_mi_qr_f32_batch
    args = (ci(count), ci(int(mode)), ci(int(reorth)), pq, sz(ldq), pr, sz(ldr), pa, sz(lda), sz(m), sz(n),
            vp(_ptr(bf.dwq)), vp(_ptr(bf.dwr)), vp(_ptr(bf.dw_reorth_r)), vp(_ptr(bf.dl)), vp(_ptr(bf.hl)), vp(stream.cuda_stream), states)

    def call():
        st = fn(*args)
        if st < 0:
            raise RuntimeError("tsqr_mi_qr_batch failed: %s" % last_error())
        return st, list(states[:count])
    call._keep = (list(qs), list(rs), list(as_), bf, stream, pq, pr, pa, states)
    return call


def qr_batch(qs, ldq, rs, ldr, as_, lda, m, n, bf, stream=None, mode=None, reorthogonalize=None):
    """One-shot form of bind_batch(): returns (first non-zero state, [states])."""
    return bind_batch(qs, ldq, rs, ldr, as_, lda, m, n, bf, stream, mode, reorthogonalize)()


class _F64Entry:
    """One fp64 entry: its Python name, the widest n, the C symbol (the layout form is symbol + "_lay") and the two functions, named
    by their suffix, that size its work space."""

    def __init__(self, name, nmax, symbol, size_suffix):
        self.name, self.nmax, self.symbol = name, nmax, symbol
        self.wq_fn, self.wr_fn = "tsqr_mi_working_q_size" + size_suffix, "tsqr_mi_working_r_size" + size_suffix

    def sizes(self, *dims):
        """doubles of (wq, wr) for a call of these dimensions"""
        L = _lib or lib()
        return getattr(L, self.wq_fn)(*dims), getattr(L, self.wr_fn)(*dims)

    def check_buffer(self, bf, *dims, hint=""):
        """bf allocated, and for at least these dimensions; hint: what else may have made it too small, appended to that message"""
        if bf.dwq is None:
            raise RuntimeError("%s: the buffer is not allocated" % self.name)
        L = _lib or lib()                              # (sizes() spelled out: this runs in every blocking call)
        if bf.dwq.numel() < getattr(L, self.wq_fn)(*dims) or bf.dwr.numel() < getattr(L, self.wr_fn)(*dims):
            raise ValueError("%s: the buffer was allocated for a smaller matrix%s" % (self.name, hint))

    def work_space(self, device, *dims):
        """(wq, wr) allocated for one call"""
        import torch
        return tuple(torch.empty(size, dtype=torch.float64, device=device) for size in self.sizes(*dims))


_F64 = _F64Entry("qr_f64", 64, "tsqr_mi_qr_f64", "_f64")
_F64_WIDE = _F64Entry("qr_f64_wide", 1024, "tsqr_mi_qr_f64_wide", "_f64_wide")
_F64_R = _F64Entry("r_f64", 64, "tsqr_mi_r_f64", "_f64_r")
_F64_LSTSQ = _F64Entry("lstsq_f64", 64, "tsqr_mi_lstsq_f64", "_f64_lstsq")
_F64_SVD = _F64Entry("svd_f64", 64, "tsqr_mi_svd_f64", "_f64_svd")       # (its size functions take jobu behind m and n)
_F64_QRCP = _F64Entry("qrcp_f64", 64, "tsqr_mi_qrcp_f64", "_f64_qrcp")   # (jobq behind m and n)
_F64_LSTSQ_RANK = _F64Entry("lstsq_rank_f64", 64, "tsqr_mi_lstsq_rank_f64", "_f64_lstsq_rank")   # (nrhs behind m and n; no _lay form)
_F64_ORTH = _F64Entry("orth_f64", 64, "tsqr_mi_orth_f64", "_f64_orth")   # (its size functions take m, k, n; no _lay form; k <= 1024)
_F64_LSTSQ_MINNORM = _F64Entry("lstsq_rank_f64", 64, "tsqr_mi_lstsq_minnorm_f64", "_f64_lstsq_minnorm")   # (lstsq_rank_f64 with minimum_norm=True)


def _null_state(fn, *scalars):
    """The state (and last_error text) of a shape the C entry fn does not run, fetched with every pointer null: scalars are its other
    arguments in order; its checks come before any HIP call."""
    rest = iter(scalars)
    args = [None if t is ctypes.c_void_p else next(rest) for t in fn.argtypes]
    assert next(rest, None) is None, "more scalars than %s takes" % fn.__name__
    return fn(*args)


def _check_f64_tensors(who, operands):
    """Every (name, operand) a float64 tensor, then every operand on the GPU (all dtype checks come first).  Raises TypeError."""
    import torch
    tensor, f64 = torch.Tensor, torch.float64
    for opname, t in operands:
        if not isinstance(t, tensor) or t.dtype != f64:
            raise TypeError("%s: %s must be a float64 tensor, got %s" % (who, opname, getattr(t, "dtype", type(t).__name__)))
    for opname, t in operands:
        if not t.is_cuda:
            raise TypeError("%s: %s is not a GPU tensor" % (who, opname))


def _f64_call(label, fn, stream, *args):
    """fn(*args, stream) on the current stream unless one is given; a negative state (a HIP failure) raises RuntimeError"""
    if stream is None:
        import torch
        stream = torch.cuda.current_stream()
    st = fn(*args, stream.cuda_stream)
    if st < 0:
        raise RuntimeError("%s failed: %s" % (label, last_error()))
    return st


class buffer_f64:
    """Work space of qr_f64 (tsqr_mi_working_{q,r}_size_f64 doubles on the GPU).  reorthogonalize: the reorth argument qr_f64 passes
    unless told otherwise (False: one CholeskyQR sweep when the device's estimate allows it, True: CholeskyQR2 at least)."""
    _entry = _F64

    def __init__(self, reorthogonalize=False, device="cuda"):
        self.reorthogonalize = bool(reorthogonalize)
        self.device = device
        self.dwq = self.dwr = None

    def _job(self):
        """what the entry's size functions take behind m and n: the job flag of a buffer that is sized by one"""
        return ()

    def allocate(self, m, n):
        import torch
        if self.dwq is not None or self.dwr is not None:
            raise RuntimeError("The buffer has been already allocated")
        self.dwq, self.dwr = (torch.empty(max(size, 1), dtype=torch.float64, device=self.device)
                              for size in self._entry.sizes(m, n, *self._job()))

    def free(self):
        self.dwq = self.dwr = None

    def get_device_memory_size(self):
        return 0 if self.dwq is None else 8 * (self.dwq.numel() + self.dwr.numel())


def _f64_spans(who, ops):
    """ld >= rows and room for (cols - 1) ld + rows doubles for every (name, (address, elements), ld, rows, cols, row_major) of ops; a
    row-major operand is checked as its transposed view, cols "columns" of rows contiguous elements.  Returns the byte span
    (first, past the last) of each operand, in the order of ops.  Raises ValueError."""
    span = []
    for name, (addr, numel), ld, rows, cols, row_major in ops:
        if row_major:
            rows, cols = cols, rows
        if ld < rows:
            raise ValueError("%s: ld%s = %d is smaller than the %d rows of %s" % (who, name, ld, rows, name))
        need = (cols - 1) * ld + rows
        if numel < need:
            raise ValueError("%s: %s holds %d elements, an operand of %d x %d with ld %d needs %d" % (who, name, numel, rows, cols, ld, need))
        span.append((addr, addr + 8 * need))
    return span


def check_f64_operands(m, n, ldq, ldr, lda, q, r, a, row_major=False):
    """The size and overlap rules of qr_f64 on (address, elements) pairs: ld >= rows, room for (n - 1) ld + rows doubles, q either
    the very operand a (same address and ld: in place) or apart from it, r apart from both.  row_major: q and a are row-major --
    ld >= n and room for (m - 1) ld + n doubles each (check_f64_r_operands' rule); r stays column-major.  Raises ValueError."""
    ops = (("q", q, ldq, m, n, row_major), ("a", a, lda, m, n, row_major))
    if row_major:                                       # (r is checked first row-major, between q and a column-major)
        sr, sq, sa = _f64_spans("qr_f64", (("r", r, ldr, n, n, False),) + ops)
    else:
        sq, sr, sa = _f64_spans("qr_f64", (ops[0], ("r", r, ldr, n, n, False), ops[1]))
    if not (q[0] == a[0] and ldq == lda) and sq[0] < sa[1] and sa[0] < sq[1]:
        raise ValueError("qr_f64: q overlaps a without being a (in place needs q == a and ldq == lda)")
    for other, so in (("q", sq), ("a", sa)):
        if sr[0] < so[1] and so[0] < sr[1]:
            raise ValueError("qr_f64: r overlaps %s" % other)


def _f64_run(entry, label, fn, head, tensors, lds, m, n, bf, stream, reorthogonalize, check, pointers, jpvt=None, job=(), hint=""):
    """What a blocking entry on a buffer does, in the order that is its contract (qr_f64, qr_f64_wide, svd_f64, qrcp_f64): the reorth
    default; every (name, tensor) of tensors a float64 GPU tensor (then jpvt an int32 one); the size state; the cap state, asked of fn
    with every pointer null; check(), the entry's size and overlap rules; the buffer; the call.  head: fn's arguments in front of
    reorth; lds: its leading dimensions in order; pointers(): its arguments between reorth and m, read only once the operands are
    known to be tensors; job and hint: _F64Entry.check_buffer's."""
    reorth = bf.reorthogonalize if reorthogonalize is None else bool(reorthogonalize)
    _check_f64_tensors(entry.name, tensors)
    if jpvt is not None:
        _check_jpvt(entry.name, jpvt)
    if n > m or m == 0 or n == 0:
        return error_invalid_matrix_size
    if n > entry.nmax:
        return _null_state(fn, *head, int(reorth), *lds, m, n)
    check()
    entry.check_buffer(bf, m, n, *job, hint=hint)
    return _f64_call(label, fn, stream, *head, int(reorth), *pointers(), m, n, bf.dwq.data_ptr(), bf.dwr.data_ptr())


def _qr_f64(entry, q, ldq, r, ldr, a, lda, m, n, bf, stream, reorthogonalize, row_major=False):
    """The body of qr_f64 (entry _F64) and qr_f64_wide (_F64_WIDE).  row_major: the entry's _lay form (tsqr_mi_qr_f64_lay,
    tsqr_mi_qr_f64_wide_lay) with q and a row-major."""
    symbol = entry.symbol + "_lay" if row_major else entry.symbol
    head = (ROW_MAJOR, ROW_MAJOR) if row_major else ()       # (the layout form's two leading arguments)
    return _f64_run(entry, symbol, getattr(lib(), symbol), head, (("q", q), ("r", r), ("a", a)), (ldq, ldr, lda), m, n, bf, stream,
                    reorthogonalize,
                    lambda: check_f64_operands(m, n, ldq, ldr, lda, (q.data_ptr(), q.numel()), (r.data_ptr(), r.numel()),
                                               (a.data_ptr(), a.numel()), row_major=bool(row_major)),
                    lambda: (q.data_ptr(), ldq, r.data_ptr(), ldr, a.data_ptr(), lda))


def qr_f64(q, ldq, r, ldr, a, lda, m, n, bf, stream=None, reorthogonalize=None, row_major=False):
    """Double-precision tall-skinny QR (tsqr_mi_qr_f64), 1 <= n <= 64, n <= m: q, r, a are float64 GPU tensors holding column-major
    data (only data_ptr and numel are used); q may be a itself (in place, ldq == lda).  row_major=True (tsqr_mi_qr_f64_lay): q and a
    hold ROW-major data, element (i, j) at i * ld + j with ld >= n -- a contiguous (m, n) tensor with ld = n -- read and written where
    they lie; r stays column-major, and q, r, the state and the sweep count have the bits of the column-major call on the same matrix.
    Blocking; returns the state: 0,
    error_invalid_matrix_size, error_unsupported_mode (n > 64) or error_not_finite.  Operands are checked before anything is launched:
    TypeError for a wrong dtype or a CPU tensor, ValueError for a short tensor, a leading dimension below the rows (row-major: below
    the columns), or overlapping operands.  last_sweeps_f64() tells how many sweeps the call took.  qr_f64_tensor is the same
    factorisation on a two-dimensional tensor with any strides."""
    return _qr_f64(_F64, q, ldq, r, ldr, a, lda, m, n, bf, stream, reorthogonalize, row_major)


class buffer_f64_wide(buffer_f64):
    """Work space of qr_f64_wide (tsqr_mi_working_{q,r}_size_f64_wide doubles on the GPU); reorthogonalize as in buffer_f64."""
    _entry = _F64_WIDE


def qr_f64_wide(q, ldq, r, ldr, a, lda, m, n, bf, stream=None, reorthogonalize=None, row_major=False):
    """Double-precision tall-skinny QR for 1 <= n <= 1024, n <= m (tsqr_mi_qr_f64_wide; qr_f64 itself for n <= 64): the arguments,
    operand rules and states of qr_f64, error_unsupported_mode for n > 1024.  row_major=True (tsqr_mi_qr_f64_wide_lay): q and a hold
    ROW-major data, element (i, j) at i * ld + j with ld >= n, read and written where they lie; r stays column-major, and q, r, the
    state and the sweep count have the bits of the column-major call on the same matrix; in place needs q == a and ldq == lda.
    bf is a buffer_f64_wide (the same for both layouts).  Operands are checked before anything is launched (TypeError / ValueError,
    check_f64_operands).  last_sweeps_f64() tells how many sweeps the call took.  qr_f64_wide_tensor is the same factorisation on a
    two-dimensional tensor with any strides."""
    return _qr_f64(_F64_WIDE, q, ldq, r, ldr, a, lda, m, n, bf, stream, reorthogonalize, row_major)


class buffer_f64_r(buffer_f64):
    """Work space of r_f64 (tsqr_mi_working_{q,r}_size_f64_r doubles on the GPU: no m x n part); reorthogonalize as in buffer_f64."""
    _entry = _F64_R


def check_f64_r_operands(m, n, ldr, lda, r, a, row_major=False):
    """check_f64_operands' rules for the two operands of r_f64: ld >= rows, room for (n - 1) ld + rows doubles, r apart from a.
    row_major: a is row-major -- lda >= n and room for (m - 1) lda + n doubles, the span r has to stay clear of."""
    sr, sa = _f64_spans("r_f64", (("r", r, ldr, n, n, False), ("a", a, lda, m, n, row_major)))
    if sr[0] < sa[1] and sa[0] < sr[1]:
        raise ValueError("r_f64: r overlaps a")


def r_f64(r, ldr, a, lda, m, n, bf, stream=None, reorthogonalize=None, row_major=False):
    """The R factor of qr_f64 alone, Q never formed (tsqr_mi_r_f64), 1 <= n <= 64, n <= m: r and a are float64 GPU tensors holding
    column-major data (only data_ptr and numel are used); a is read only.  row_major=True (tsqr_mi_r_f64_lay): a holds ROW-major data,
    element (i, j) at i * lda + j with lda >= n -- a contiguous (m, n) tensor with lda = n -- read where it lies; r stays column-major and
    has the bits of the column-major call on the same matrix.  bf is a buffer_f64_r.  Blocking; returns the state: 0,
    error_invalid_matrix_size, error_unsupported_mode (n > 64) or error_not_finite.  Operands are checked before anything is launched:
    TypeError for a wrong dtype or a CPU tensor, ValueError for a short tensor, a leading dimension below the rows, or r overlapping a.
    last_sweeps_f64() tells how many sweeps the call took."""
    entry = _F64_R
    reorth = bf.reorthogonalize if reorthogonalize is None else bool(reorthogonalize)
    _check_f64_tensors(entry.name, (("r", r), ("a", a)))
    if n > m or m == 0 or n == 0:
        return error_invalid_matrix_size
    fn = lib().tsqr_mi_r_f64_lay
    layout = ROW_MAJOR if row_major else COL_MAJOR
    if n > entry.nmax:
        return _null_state(fn, layout, int(reorth), ldr, lda, m, n)
    check_f64_r_operands(m, n, ldr, lda, (r.data_ptr(), r.numel()), (a.data_ptr(), a.numel()), row_major=bool(row_major))
    entry.check_buffer(bf, m, n)
    return _f64_call(entry.symbol, fn, stream, layout, int(reorth), r.data_ptr(), ldr, a.data_ptr(), lda, m, n,
                     bf.dwq.data_ptr(), bf.dwr.data_ptr())


class _F64StateError(RuntimeError):
    """A tensor-level fp64 entry ended with a non-zero state (.state); each entry raises its own subclass."""

    def __init__(self, state, text):
        RuntimeError.__init__(self, text)
        self.state = state


class LstsqError(_F64StateError):
    """lstsq_f64 ended with a non-zero state (.state: error_invalid_matrix_size, error_unsupported_mode or error_not_finite)"""


def _columns_contiguous(t):
    rows, cols = t.shape
    return t.stride(0) == 1 and (cols == 1 or t.stride(1) >= max(rows, 1))


def _colmajor_f64(t):
    """(tensor whose storage holds t column-major, its leading dimension): t itself when its columns are already contiguous (stride 1
    down a column, at least the row count between columns), a column-major copy otherwise -- the operand of the call is never written"""
    rows, cols = t.shape
    if _columns_contiguous(t):
        return t, (t.stride(1) if cols > 1 else max(rows, 1))
    return t.t().contiguous().t(), max(rows, 1)


def _operand_f64(t):
    """(tensor, leading dimension, layout) under which lstsq_f64 hands the two-dimensional t to tsqr_mi_lstsq_f64_lay.  Used where it
    lies: columns contiguous (_colmajor_f64's rule: COL_MAJOR), rows contiguous (stride(1) == 1 and stride(0) >= cols: ROW_MAJOR), or a
    single column (any stride(0) >= 1: ROW_MAJOR with that stride).  Any other operand: _colmajor_f64's copy."""
    cols = t.shape[1]
    if not _columns_contiguous(t) and (t.stride(1) == 1 or cols == 1) and t.stride(0) >= max(cols, 1):
        return t, t.stride(0), ROW_MAJOR
    return _colmajor_f64(t) + (COL_MAJOR,)


def lstsq_f64(a, b, reorth=False, refine=1, stream=None):
    """X = argmin ||a X - b||_F in double precision (tsqr_mi_lstsq_f64: include/tsqr_mi.h has the method and the accuracy statement;
    claimed for cond(a) <= 1e6, not a substitute for Householder QR beyond cond(a) of about 1e7).  a: m x n float64 GPU tensor,
    1 <= n <= 64, n <= m; b: m x nrhs (or m) float64 GPU tensor, nrhs <= 16; any strides; neither is written.  An operand is read where
    it lies, without a copy, when its columns are contiguous (stride(0) == 1, stride(1) >= m), when its rows are contiguous
    (stride(1) == 1, stride(0) >= its column count: every contiguous torch tensor), or when it has a single column; any other operand
    (a[:, ::2], an expanded or overlapping view) is copied once into column-major storage.  The result has the same bits whichever way
    the operand is stored.  reorth: the R-only ladder's argument (r_f64); refine: correction
    passes, 0 .. 4 (from the second on, a right-hand side whose correction did not halve keeps its x and stops).  Blocking.  Returns (x, r): x n x nrhs (n when b is one-dimensional), r the n x n upper-triangular factor, bitwise
    r_f64's on the same a.  Raises TypeError for a wrong dtype or a CPU tensor, ValueError for shapes that do not fit together, LstsqError
    (.state) when the C entry returns a state other than 0: sizes it does not support, or error_not_finite from the ladder (Inf or NaN
    in a, a column norm outside [2^-511, 2^512), or an exactly zero column).  That state is no rank test: dependent but non-zero columns
    (a copied column, a sum of two others) are accepted on the shifted path, and the x that comes back is finite and NOT a
    least-squares solution (entries of 1e14 and more; include/tsqr_mi.h has the measured residuals and the range of b's magnitudes) --
    test r before using x when the columns may be dependent.  last_sweeps_f64() tells how many sweeps the ladder took."""
    import torch
    entry = _F64_LSTSQ
    _check_f64_tensors(entry.name, (("a", a), ("b", b)))
    if a.dim() != 2 or b.dim() not in (1, 2) or b.shape[0] != a.shape[0]:
        raise ValueError("lstsq_f64: a must be m x n and b m x nrhs (or m), got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    vector = b.dim() == 1
    b2 = b.unsqueeze(1) if vector else b
    m, n = a.shape
    nrhs = b2.shape[1]
    if m == 0 or n == 0 or nrhs == 0 or n > m or n > entry.nmax or nrhs > 16 or not 0 <= int(refine) <= 4:
        st = _null_state(lib().tsqr_mi_lstsq_f64, int(bool(reorth)), int(refine), max(n, 1), max(n, 1), max(m, 1), max(m, 1), m, n, nrhs)
        raise LstsqError(st, "lstsq_f64: state %d for a %d x %d, nrhs %d, refine %d%s"
                         % (st, m, n, nrhs, int(refine), (": " + last_error()) if st == error_unsupported_mode else ""))
    ac, lda, a_layout = _operand_f64(a)
    bc, ldb, b_layout = _operand_f64(b2)
    x = torch.empty((nrhs, n), dtype=torch.float64, device=a.device)
    r = torch.empty((n, n), dtype=torch.float64, device=a.device)
    wq, wr = entry.work_space(a.device, m, n, nrhs)
    with torch.cuda.device(a.device):
        st = _f64_call(entry.symbol, lib().tsqr_mi_lstsq_f64_lay, stream, a_layout, b_layout, int(bool(reorth)), int(refine), x.data_ptr(), n,
                       r.data_ptr(), n, ac.data_ptr(), lda, bc.data_ptr(), ldb, m, n, nrhs, wq.data_ptr(), wr.data_ptr())
    if st:
        raise LstsqError(st, "lstsq_f64: state %d: %s" % (st, last_error()))
    x = x.t()
    return (x[:, 0] if vector else x), r.t()


class LstsqRankError(_F64StateError):
    """lstsq_rank_f64 ended with a non-zero state (.state: error_invalid_matrix_size, error_unsupported_mode or error_not_finite)"""


def lstsq_rank_f64(a, b, rcond=None, reorth=False, refine=1, stream=None, *, minimum_norm=False):
    """The rank of a and the basic solution of min ||a X - b||_F on its numerically independent columns, in double precision
    (tsqr_mi_lstsq_rank_f64: include/tsqr_mi.h has the method and the measured accuracy).  a: m x n float64 GPU tensor, 1 <= n <= 64,
    n <= m; b: m x nrhs (or m) float64 GPU tensor, nrhs <= 16; any strides, read where they lie or copied once under the rule of
    lstsq_f64; neither is written, and the result has the same bits whichever way an operand is stored.  rcond: column j of the pivoted
    R is retained when R_jj > rcond R_00; None: max(m, n) 2^-52; must be below 1.  reorth: the R-only ladder's argument; refine:
    correction passes, 0 .. 4.  Blocking.  Returns (x, r, p, rank): x n x nrhs (n when b is one-dimensional) with exact zeros in the rows
    p[rank:] and the least-squares solution on the columns p[:rank] in the others -- the basic solution, not the minimum-norm one;
    r (n x n upper triangular) and p (n int32 pivots, 0-based, a[:, p] = Q r) bitwise qrcp_f64's with compute_q=False on the same a;
    rank a Python int.  Raises TypeError for a wrong dtype or a CPU tensor, ValueError for shapes that do not fit together,
    LstsqRankError (.state) when the entry does not run the shape or returns a state other than 0: error_not_finite from the ladder (Inf
    or NaN in a, a column norm outside [2^-511, 2^512), or an exactly zero column among non-zero ones) or from the Cholesky step on the
    retained columns.
    minimum_norm=True (keyword only; tsqr_mi_lstsq_minnorm_f64): x is the minimum-norm solution of the problem truncated at that rank,
    what LAPACK's dgelsy and scipy.linalg.lstsq(lapack_driver="gelsy") return at the same rank (numpy.linalg.lstsq and torch.linalg.lstsq
    truncate by singular values instead and agree when a has exact rank).  Every row of x may then be non-zero; r, p and rank are bitwise
    those of the default, and at full rank so is x.  The same arguments, checks and errors; error_not_finite also from the Cholesky
    factorisation of C = I + M M^T."""
    import math
    import torch
    entry = _F64_LSTSQ_MINNORM if minimum_norm else _F64_LSTSQ_RANK
    _check_f64_tensors(entry.name, (("a", a), ("b", b)))
    if a.dim() != 2 or b.dim() not in (1, 2) or b.shape[0] != a.shape[0]:
        raise ValueError("lstsq_rank_f64: a must be m x n and b m x nrhs (or m), got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    vector = b.dim() == 1
    b2 = b.unsqueeze(1) if vector else b
    m, n = a.shape
    nrhs = b2.shape[1]
    rc = -1.0 if rcond is None else float(rcond)
    # (the C entry rejects a null pointer before it looks at a size, so a shape it does not run is decided here, by its rules and in its
    # order, without a call)
    if m == 0 or n == 0 or nrhs == 0 or n > m:
        raise LstsqRankError(error_invalid_matrix_size, "lstsq_rank_f64: state %d for a %d x %d, nrhs %d" % (error_invalid_matrix_size, m, n, nrhs))
    for bad, text in ((n > entry.nmax, "n <= 64"), (nrhs > 16, "nrhs <= 16"), (not 0 <= int(refine) <= 4, "0 <= refine <= 4"),
                      (math.isnan(rc) or rc >= 1.0, "rcond < 1")):
        if bad:
            raise LstsqRankError(error_unsupported_mode, "lstsq_rank_f64: state %d for a %d x %d, nrhs %d, refine %d, rcond %r: "
                                 "%s supports %s" % (error_unsupported_mode, m, n, nrhs, int(refine), rcond, entry.symbol, text))
    ac, lda, a_layout = _operand_f64(a)
    bc, ldb, b_layout = _operand_f64(b2)
    x = torch.empty((nrhs, n), dtype=torch.float64, device=a.device)
    r = torch.empty((n, n), dtype=torch.float64, device=a.device)
    p = torch.empty((n,), dtype=torch.int32, device=a.device)
    rank = ctypes.c_int(-1)
    wq, wr = entry.work_space(a.device, m, n, nrhs)
    with torch.cuda.device(a.device):
        st = _f64_call(entry.symbol, getattr(lib(), entry.symbol), stream, a_layout, b_layout, int(bool(reorth)), int(refine), rc,
                       x.data_ptr(), n, r.data_ptr(), n, p.data_ptr(), ctypes.byref(rank), ac.data_ptr(), lda, bc.data_ptr(), ldb, m, n, nrhs,
                       wq.data_ptr(), wr.data_ptr())
    if st:
        raise LstsqRankError(st, "lstsq_rank_f64: state %d: %s" % (st, last_error()))
    x = x.t()
    return (x[:, 0] if vector else x), r.t(), p, int(rank.value)


class QrError(_F64StateError):
    """qr_f64_tensor or qr_f64_wide_tensor ended with a non-zero state (.state: error_invalid_matrix_size, error_unsupported_mode or error_not_finite)"""


def _f64_tensor_operand(entry, symbol, error, a, reorth, job=()):
    """How a tensor form (entry.name + "_tensor") starts: a a float64 GPU tensor (TypeError) with two dimensions (ValueError); a shape
    the C entry `symbol` does not run raises error with the state that entry gives it, asked with every pointer null (job: its job
    flag, behind the two layouts).  Returns (fn, m, n) and _operand_f64(a): the operand of the call, its leading dimension, its layout."""
    name = entry.name + "_tensor"
    _check_f64_tensors(name, (("a", a),))
    if a.dim() != 2:
        raise ValueError("%s: a must be m x n, got %s" % (name, tuple(a.shape)))
    m, n = a.shape
    fn = getattr(lib(), symbol)
    if m == 0 or n == 0 or n > m or n > entry.nmax:
        st = _null_state(fn, COL_MAJOR, COL_MAJOR, *job, int(bool(reorth)), max(m, 1), max(n, 1), max(m, 1), m, n)
        raise error(st, "%s: state %d for a %d x %d%s" % (name, st, m, n, (": " + last_error()) if st == error_unsupported_mode else ""))
    return (fn, m, n) + _operand_f64(a)


def _f64_q_for(a, ac, lda, layout, overwrite_a):
    """(q, ldq) for the m x n factor a tensor form returns beside a, of which it hands ac (ld lda, layout) to the call: a itself when
    overwrite_a holds and a is used where it lies (in place: the same layout and leading dimension), a fresh tensor otherwise,
    row-major for a row-major operand and with column-major strides for a column-major one."""
    import torch
    m, n = a.shape
    if overwrite_a and ac.data_ptr() == a.data_ptr():
        return a, lda
    if layout == ROW_MAJOR:
        return torch.empty((m, n), dtype=torch.float64, device=a.device), n
    return torch.empty((n, m), dtype=torch.float64, device=a.device).t(), m


def _f64_tensor_call(entry, label, error, a, fn, stream, *args):
    """_f64_call on a's device; a state other than 0 raises error"""
    import torch
    with torch.cuda.device(a.device):
        st = _f64_call(label, fn, stream, *args)
    if st:
        raise error(st, "%s_tensor: state %d: %s" % (entry.name, st, last_error()))


def _qr_f64_tensor(entry, a, reorth, overwrite_a, stream):
    """The body of qr_f64_tensor (entry _F64) and qr_f64_wide_tensor (_F64_WIDE) on the entry's _lay form."""
    import torch
    symbol = entry.symbol + "_lay"
    fn, m, n, ac, lda, layout = _f64_tensor_operand(entry, symbol, QrError, a, reorth)
    q, ldq = _f64_q_for(a, ac, lda, layout, overwrite_a)
    r = torch.empty((n, n), dtype=torch.float64, device=a.device)
    wq, wr = entry.work_space(a.device, m, n)
    _f64_tensor_call(entry, symbol, QrError, a, fn, stream, layout, layout, int(bool(reorth)), q.data_ptr(), ldq, r.data_ptr(), n,
                     ac.data_ptr(), lda, m, n, wq.data_ptr(), wr.data_ptr())
    return q, r.t()


def qr_f64_tensor(a, reorth=False, overwrite_a=False, stream=None):
    """(q, r) of the double-precision tall-skinny QR (tsqr_mi_qr_f64_lay: include/tsqr_mi.h has the method and the accuracy bands) of a
    two-dimensional float64 GPU tensor a, m x n with 1 <= n <= 64, n <= m, any strides.  a is read where it lies, without a copy, when
    its columns are contiguous, when its rows are contiguous (every contiguous torch tensor) or when it has a single column
    (_operand_f64's rule, as for lstsq_f64); any other a (a[:, ::2], an expanded view) is copied once into column-major storage.
    q has a's shape, row-major for a row-major a and with column-major strides for a column-major one; r is the n x n upper-triangular
    factor.  For the same matrix q and r have the same bits whichever way a is stored.  overwrite_a=True: when a is used where it lies,
    q IS a (the factorisation runs in place); otherwise a is never written.  reorth: CholeskyQR2 at least (qr_f64).  The work space is
    allocated per call.  Blocking.  Raises TypeError for a wrong dtype or a CPU tensor, ValueError for a tensor that is not
    two-dimensional, QrError (.state) when the C entry returns a state other than 0: sizes it does not support (n > m, an empty a:
    error_invalid_matrix_size; n > 64: error_unsupported_mode) or error_not_finite from the ladder (Inf or NaN in a, or a
    rank-deficient a).  last_sweeps_f64() tells how many sweeps the call took."""
    return _qr_f64_tensor(_F64, a, reorth, overwrite_a, stream)


def qr_f64_wide_tensor(a, reorth=False, overwrite_a=False, stream=None):
    """qr_f64_tensor for 1 <= n <= 1024 (tsqr_mi_qr_f64_wide_lay: include/tsqr_mi.h has the method and the accuracy bands): the same
    contract -- a is used where it lies when its columns or its rows are contiguous (_operand_f64's rule) and copied once into
    column-major storage otherwise, q has a's shape and layout, the same bits of q and r whichever way a is stored, overwrite_a, a work
    space per call, TypeError / ValueError / QrError (.state; error_unsupported_mode for n > 1024).  For n <= 64 the result has the bits
    of qr_f64_tensor.  last_sweeps_f64() tells how many sweeps the call took."""
    return _qr_f64_tensor(_F64_WIDE, a, reorth, overwrite_a, stream)


def _f64_apart(who, span, pair, in_place, rule):
    """span: {name: (first byte, past the last)} in the order the operands are examined.  Every two of them apart, except the two of
    `pair` when in_place holds (they are one operand); where those two overlap otherwise, the message ends with rule.  Raises
    ValueError."""
    names = list(span)
    for i, x in enumerate(names):
        for y in names[i + 1:]:
            if {x, y} == pair and in_place:
                continue
            if span[x][0] < span[y][1] and span[y][0] < span[x][1]:
                raise ValueError("%s: %s overlaps %s%s" % (who, x, y, rule if {x, y} == pair else ""))


class SvdError(_F64StateError):
    """svd_f64_tensor ended with a non-zero state (.state: error_invalid_matrix_size, error_unsupported_mode, error_not_finite or
    error_no_convergence)"""


class buffer_f64_svd(buffer_f64):
    """Work space of svd_f64 (tsqr_mi_working_{q,r}_size_f64_svd doubles on the GPU).  compute_u: the jobu the space is sized for --
    True: the QR entry's space and the SVD block; False: the R-only entry's (no m x n part; it does not serve a call with compute_u).
    reorthogonalize as in buffer_f64."""
    _entry = _F64_SVD

    def __init__(self, reorthogonalize=False, device="cuda", compute_u=True):
        buffer_f64.__init__(self, reorthogonalize, device)
        self.compute_u = bool(compute_u)

    def _job(self):
        return (int(self.compute_u),)


def check_f64_svd_operands(m, n, ldu, ldv, lda, u, s, v, a, row_major=False):
    """The size and overlap rules of svd_f64 on (address, elements) pairs (u and v may be None: not used): check_f64_operands' rules for
    u and a (row_major: both row-major), v n x n column-major with ldv >= n, s of n elements; u either the very operand a (same address
    and ld: in place) or apart from it; s and v apart from u, from a and from each other.  Raises ValueError."""
    ops = [("a", a, lda, m, n, row_major), ("s", s, n, n, 1, False)]
    if u is not None:
        ops.append(("u", u, ldu, m, n, row_major))
    if v is not None:
        ops.append(("v", v, ldv, n, n, False))
    span = dict(zip((o[0] for o in ops), _f64_spans("svd_f64", ops)))
    _f64_apart("svd_f64", span, {"a", "u"}, u is not None and u[0] == a[0] and ldu == lda,
               " without being a (in place needs u == a and ldu == lda)")


def svd_f64(u, ldu, s, v, ldv, a, lda, m, n, bf, stream=None, reorthogonalize=None, row_major=False, compute_u=True):
    """Double-precision tall-skinny SVD (tsqr_mi_svd_f64), a = u diag(s) v^T, 1 <= n <= 64, n <= m: u, s, v, a are float64 GPU tensors
    (only data_ptr and numel are used); a and u hold column-major data, or ROW-major data with row_major=True (element (i, j) at
    i * ld + j, ld >= n) as in qr_f64; s takes n values, descending; v (n x n, column-major, ldv; None: not wanted) takes V, not its
    transpose.  compute_u=False (jobu = 0): u is not used (None is fine), a is read only, and bf must have been made with
    compute_u=False or True -- the larger space serves both.  u may be a itself (in place, ldu == lda).  bf is a buffer_f64_svd.
    Blocking; returns the state: 0, error_invalid_matrix_size, error_unsupported_mode (n > 64), error_not_finite (the ladder's verdict)
    or error_no_convergence.  Operands are checked before anything is launched: TypeError for a wrong dtype or a CPU tensor,
    ValueError for a short tensor, a short leading dimension or overlapping operands.  last_sweeps_f64() tells how many sweeps the
    ladder took, last_jacobi_sweeps_f64() how many the Jacobi iteration took.  The signs of the columns of u and v are reproducible
    but not specified."""
    entry = _F64_SVD
    jobu = 1 if compute_u else 0
    layout = ROW_MAJOR if row_major else COL_MAJOR
    pair = lambda t: (t.data_ptr(), t.numel())
    return _f64_run(entry, entry.symbol, lib().tsqr_mi_svd_f64, (layout, layout, jobu),
                    [("s", s), ("a", a)] + ([("u", u)] if jobu else []) + ([("v", v)] if v is not None else []), (ldu, ldv, lda),
                    m, n, bf, stream, reorthogonalize,
                    lambda: check_f64_svd_operands(m, n, ldu, ldv, lda, pair(u) if jobu else None, pair(s),
                                                   None if v is None else pair(v), pair(a), row_major=bool(row_major)),
                    lambda: (u.data_ptr() if jobu else None, ldu, s.data_ptr(), None if v is None else v.data_ptr(), ldv,
                             a.data_ptr(), lda),
                    job=(jobu,), hint=" (or without compute_u)")


def svd_f64_tensor(a, reorth=False, compute_uv=True, overwrite_a=False, stream=None):
    """(U, S, Vh) of the double-precision tall-skinny SVD (tsqr_mi_svd_f64: include/tsqr_mi.h has the method) of a two-dimensional
    float64 GPU tensor a, m x n with 1 <= n <= 64, n <= m, any strides: the shapes of torch.linalg.svd(a, full_matrices=False) -- U m x n,
    S of n values, descending, Vh n x n = V transposed.  compute_uv=False returns S alone (jobu = 0: Q is never formed and a is only
    read).  a is read where it lies when its columns or its rows are contiguous (_operand_f64's rule, as for qr_f64_tensor) and copied
    once into column-major storage otherwise; U has a's layout, and U, S and Vh have the same bits whichever way a is stored.
    overwrite_a=True: when a is used where it lies, U IS a.  reorth: the ladder's argument (qr_f64).  The work space is allocated per
    call.  Blocking.  The signs of the columns of U and rows of Vh are reproducible but not specified.  Raises TypeError for a wrong
    dtype or a CPU tensor, ValueError for a tensor that is not two-dimensional, SvdError (.state) when the C entry returns a state other
    than 0: sizes it does not support, error_not_finite from the ladder (Inf or NaN in a, a zero column), or error_no_convergence."""
    import torch
    entry = _F64_SVD
    jobu = 1 if compute_uv else 0
    fn, m, n, ac, lda, layout = _f64_tensor_operand(entry, entry.symbol, SvdError, a, reorth, (jobu,))
    u, ldu = _f64_q_for(a, ac, lda, layout, overwrite_a) if jobu else (None, lda)
    s = torch.empty(n, dtype=torch.float64, device=a.device)
    v = torch.empty((n, n), dtype=torch.float64, device=a.device) if jobu else None      # (column-major V: read as a tensor, it is Vh)
    wq, wr = entry.work_space(a.device, m, n, jobu)
    _f64_tensor_call(entry, entry.symbol, SvdError, a, fn, stream, layout, layout, jobu, int(bool(reorth)),
                     u.data_ptr() if jobu else None, ldu, s.data_ptr(), v.data_ptr() if jobu else None, n, ac.data_ptr(), lda, m, n,
                     wq.data_ptr(), wr.data_ptr())
    return (u, s, v) if jobu else s


class QrcpError(_F64StateError):
    """qrcp_f64_tensor ended with a non-zero state (.state: error_invalid_matrix_size, error_unsupported_mode or error_not_finite)"""


class buffer_f64_qrcp(buffer_f64):
    """Work space of qrcp_f64 (tsqr_mi_working_{q,r}_size_f64_qrcp doubles on the GPU).  compute_q: the jobq the space is sized for --
    True: the QR entry's space and the block for H; False: the R-only entry's (no m x n part; it does not serve a call with compute_q).
    reorthogonalize as in buffer_f64."""
    _entry = _F64_QRCP

    def __init__(self, reorthogonalize=False, device="cuda", compute_q=True):
        buffer_f64.__init__(self, reorthogonalize, device)
        self.compute_q = bool(compute_q)

    def _job(self):
        return (int(self.compute_q),)


def check_f64_qrcp_operands(m, n, ldq, ldr, lda, q, r, jpvt, a, row_major=False):
    """The size and overlap rules of qrcp_f64 on (address, elements) pairs (q may be None: not used): check_f64_operands' rules for q
    and a (row_major: both row-major), r n x n column-major with ldr >= n, jpvt of n 4-byte elements; q either the very operand a
    (same address and ld: in place) or apart from it; r and jpvt apart from q, from a and from each other.  Raises ValueError."""
    ops = [("a", a, lda, m, n, row_major), ("r", r, ldr, n, n, False)]
    if q is not None:
        ops.append(("q", q, ldq, m, n, row_major))
    span = dict(zip((o[0] for o in ops), _f64_spans("qrcp_f64", ops)))
    if jpvt[1] < n:
        raise ValueError("qrcp_f64: jpvt holds %d elements, %d pivots need %d" % (jpvt[1], n, n))
    span["jpvt"] = (jpvt[0], jpvt[0] + 4 * n)
    _f64_apart("qrcp_f64", span, {"a", "q"}, q is not None and q[0] == a[0] and ldq == lda,
               " without being a (in place needs q == a and ldq == lda)")


def _check_jpvt(who, jpvt):
    import torch
    if not isinstance(jpvt, torch.Tensor) or jpvt.dtype != torch.int32:
        raise TypeError("%s: jpvt must be an int32 tensor, got %s" % (who, getattr(jpvt, "dtype", type(jpvt).__name__)))
    if not jpvt.is_cuda:
        raise TypeError("%s: jpvt is not a GPU tensor" % who)


def qrcp_f64(q, ldq, r, ldr, jpvt, a, lda, m, n, bf, stream=None, reorthogonalize=None, row_major=False, compute_q=True):
    """Double-precision tall-skinny QR with column pivoting (tsqr_mi_qrcp_f64), a P = q r, 1 <= n <= 64, n <= m: q, r, a are float64 GPU
    tensors and jpvt an int32 GPU tensor (only data_ptr and numel are used); a and q hold column-major data, or ROW-major data with
    row_major=True (element (i, j) at i * ld + j, ld >= n) as in qr_f64; r (n x n, column-major, ldr) takes R -- upper triangular,
    diag(R) >= 0 and non-increasing; jpvt takes n 0-based pivots: column j of a P is column jpvt[j] of a.  compute_q=False (jobq = 0):
    q is not used (None is fine), a is read only, and bf must have been made with compute_q=False or True -- the larger space serves
    both.  q may be a itself (in place, ldq == lda).  bf is a buffer_f64_qrcp.  Blocking; returns the state: 0,
    error_invalid_matrix_size, error_unsupported_mode (n > 64) or error_not_finite (the ladder's verdict; no rank test -- the rank is
    read off diag(R)).  Operands are checked before anything is launched: TypeError for a wrong dtype or a CPU tensor, ValueError for a
    short tensor, a short leading dimension or overlapping operands.  last_sweeps_f64() tells how many sweeps the ladder took."""
    entry = _F64_QRCP
    jobq = 1 if compute_q else 0
    layout = ROW_MAJOR if row_major else COL_MAJOR
    pair = lambda t: (t.data_ptr(), t.numel())
    return _f64_run(entry, entry.symbol, lib().tsqr_mi_qrcp_f64, (layout, layout, jobq),
                    [("r", r), ("a", a)] + ([("q", q)] if jobq else []), (ldq, ldr, lda), m, n, bf, stream, reorthogonalize,
                    lambda: check_f64_qrcp_operands(m, n, ldq, ldr, lda, pair(q) if jobq else None, pair(r), pair(jpvt), pair(a),
                                                    row_major=bool(row_major)),
                    lambda: (q.data_ptr() if jobq else None, ldq, r.data_ptr(), ldr, jpvt.data_ptr(), a.data_ptr(), lda),
                    jpvt=jpvt, job=(jobq,), hint=" (or without compute_q)")


def qrcp_f64_tensor(a, reorth=False, compute_q=True, overwrite_a=False, stream=None):
    """(q, r, p) of the double-precision tall-skinny QR with column pivoting (tsqr_mi_qrcp_f64: include/tsqr_mi.h has the method and the
    band) of a two-dimensional float64 GPU tensor a, m x n with 1 <= n <= 64, n <= m, any strides: the shapes of
    scipy.linalg.qr(a, mode="economic", pivoting=True) -- q m x n, r n x n upper triangular with diag(r) >= 0 and non-increasing, p an
    int64 tensor of n pivots with a[:, p] = q @ r.  compute_q=False returns (r, p) (jobq = 0: Q is never formed and a is only read).
    a is read where it lies when its columns or its rows are contiguous (_operand_f64's rule, as for qr_f64_tensor) and copied once
    into column-major storage otherwise; q has a's layout, and q, r and p have the same bits whichever way a is stored.
    overwrite_a=True: when a is used where it lies, q IS a.  reorth: the ladder's argument (qr_f64).  The work space is allocated per
    call.  Blocking.  Raises TypeError for a wrong dtype or a CPU tensor, ValueError for a tensor that is not two-dimensional, QrcpError
    (.state) when the C entry returns a state other than 0: sizes it does not support, or error_not_finite from the ladder (Inf or NaN
    in a, a zero column).  That state is no rank test: the numerical rank is read off diag(r)."""
    import torch
    entry = _F64_QRCP
    jobq = 1 if compute_q else 0
    fn, m, n, ac, lda, layout = _f64_tensor_operand(entry, entry.symbol, QrcpError, a, reorth, (jobq,))
    q, ldq = _f64_q_for(a, ac, lda, layout, overwrite_a) if jobq else (None, lda)
    r = torch.empty((n, n), dtype=torch.float64, device=a.device)
    jpvt = torch.empty(n, dtype=torch.int32, device=a.device)
    wq, wr = entry.work_space(a.device, m, n, jobq)
    _f64_tensor_call(entry, entry.symbol, QrcpError, a, fn, stream, layout, layout, jobq, int(bool(reorth)),
                     q.data_ptr() if jobq else None, ldq, r.data_ptr(), n, jpvt.data_ptr(), ac.data_ptr(), lda, m, n,
                     wq.data_ptr(), wr.data_ptr())
    p = jpvt.to(torch.int64)
    return (q, r.t(), p) if jobq else (r.t(), p)


class OrthError(_F64StateError):
    """orth_f64_tensor ended with a non-zero state (.state: error_invalid_matrix_size or error_not_finite)"""


class buffer_f64_orth(buffer_f64):
    """Work space of orth_f64 (tsqr_mi_working_{q,r}_size_f64_orth doubles on the GPU); allocate(m, k, n).  reorthogonalize: the reorth
    argument of the inner ladder, as in buffer_f64."""
    _entry = _F64_ORTH

    def allocate(self, m, k, n):
        import torch
        if self.dwq is not None or self.dwr is not None:
            raise RuntimeError("The buffer has been already allocated")
        self.dwq, self.dwr = (torch.empty(max(size, 1), dtype=torch.float64, device=self.device) for size in self._entry.sizes(m, k, n))


def check_f64_orth_operands(m, k, n, ldw, lds, ldr, ldv, w, s, r, v, v_row_major=False, w_row_major=False):
    """The size and overlap rules of orth_f64 on (address, elements) pairs: every leading dimension at least its operand's extent along
    it (the rows; the columns of a row-major v or w), room for the whole operand, w apart from v, s and r, and s apart from r (v is
    read only: it may share memory with s or r only at the caller's risk, and that is rejected too).  Raises ValueError."""
    ops = (("w", w, ldw, m, n, w_row_major), ("v", v, ldv, m, k, v_row_major), ("s", s, lds, k, n, False), ("r", r, ldr, n, n, False))
    span = dict(zip((o[0] for o in ops), _f64_spans("orth_f64", ops)))
    _f64_apart("orth_f64", span, set(), False, "")


def _orth_size_ok(m, k, n, passes):
    return passes in (1, 2) and 1 <= n <= 64 and 1 <= k <= 1024 and k + n <= m


def orth_f64(w, ldw, s, lds, r, ldr, v, ldv, m, k, n, bf, passes=2, stream=None, reorthogonalize=None, v_row_major=False,
             w_row_major=False):
    """Block orthogonalisation against an existing basis (tsqr_mi_orth_f64: include/tsqr_mi.h has the method and the contract):
    v (m x k, orthonormal columns, read only) and w (m x n) are float64 GPU tensors holding column-major data, or ROW-major data with
    v_row_major / w_row_major (element (i, j) at i * ld + j); only data_ptr and numel are used.  1 <= n <= 64, 1 <= k <= 1024,
    k + n <= m, passes 1 or 2.  w is overwritten by q with v^T q = 0, q^T q = I and w_in = v s + q r; s (k x n, lds) and r (n x n upper
    triangular, ldr) are column-major.  bf is a buffer_f64_orth.  Blocking; returns the state: 0, error_invalid_matrix_size (a size or
    passes outside the ranges: this entry has no error_unsupported_mode) or error_not_finite (w, s and r are then undefined).  Operands are
    checked before anything is launched: TypeError for a wrong dtype or a CPU tensor, ValueError for a short tensor, a short leading
    dimension or overlapping operands.  last_sweeps_f64() tells the sum of the ladder's sweeps over the rounds.  State 0 is no test that w
    was independent of v: compare diag(r) with w's column norms."""
    entry = _F64_ORTH
    reorth = bf.reorthogonalize if reorthogonalize is None else bool(reorthogonalize)
    _check_f64_tensors(entry.name, (("w", w), ("s", s), ("r", r), ("v", v)))
    if not _orth_size_ok(m, k, n, passes):
        return error_invalid_matrix_size
    pair = lambda t: (t.data_ptr(), t.numel())
    check_f64_orth_operands(m, k, n, ldw, lds, ldr, ldv, pair(w), pair(s), pair(r), pair(v), bool(v_row_major), bool(w_row_major))
    entry.check_buffer(bf, m, k, n)
    return _f64_call(entry.symbol, lib().tsqr_mi_orth_f64, stream, ROW_MAJOR if v_row_major else COL_MAJOR,
                     ROW_MAJOR if w_row_major else COL_MAJOR, int(passes), int(reorth), w.data_ptr(), ldw, s.data_ptr(), lds, r.data_ptr(), ldr,
                     v.data_ptr(), ldv, m, k, n, bf.dwq.data_ptr(), bf.dwr.data_ptr())


def orth_f64_tensor(v, w, passes=2, reorth=False, overwrite_w=False, stream=None):
    """(q, s, r) of the block orthogonalisation of w against the orthonormal basis v (tsqr_mi_orth_f64: include/tsqr_mi.h has the method):
    v m x k and w m x n two-dimensional float64 GPU tensors, 1 <= n <= 64, 1 <= k <= 1024, k + n <= m, any strides; v^T q = 0,
    q^T q = I, w = v s + q r with s k x n and r n x n upper triangular, diag(r) >= 0.  Each operand is used where it lies when its columns
    or its rows are contiguous (_operand_f64's rule, as for qr_f64_tensor), each with its own layout, and copied once into column-major
    storage otherwise; q has w's shape and layout, and q, s and r have the same bits whichever way v and w are stored.
    overwrite_w=True: when w is used where it lies, q IS w; otherwise w is never written (the call then works on a copy of w: the only
    m x n allocation).  passes: 2 (BCGS2) or 1 (one round; not enough when w lies close to span(v)).  reorth: the inner ladder's argument.
    The work space is allocated per call.  Blocking.  Raises TypeError for a wrong dtype or a CPU tensor, ValueError for tensors that are
    not two-dimensional or whose row counts differ, OrthError (.state) for a state other than 0: error_invalid_matrix_size for sizes or
    passes outside the ranges, error_not_finite from the ladder on the projected block (Inf or NaN in v or w included).  State 0 is no
    test that w was independent of v: compare diag(r) with w's column norms."""
    import torch
    entry = _F64_ORTH
    _check_f64_tensors("orth_f64_tensor", (("v", v), ("w", w)))
    if v.dim() != 2 or w.dim() != 2 or v.shape[0] != w.shape[0]:
        raise ValueError("orth_f64_tensor: v must be m x k and w m x n, got %s and %s" % (tuple(v.shape), tuple(w.shape)))
    (m, k), n = v.shape, w.shape[1]
    if not _orth_size_ok(m, k, n, passes):
        raise OrthError(error_invalid_matrix_size, "orth_f64_tensor: state %d for v %d x %d, w %d x %d, passes %r"
                        % (error_invalid_matrix_size, m, k, m, n, passes))
    vc, ldv, v_layout = _operand_f64(v)
    wc, ldw, w_layout = _operand_f64(w)
    if wc.data_ptr() == w.data_ptr() and not overwrite_w:  # (used where it lies but not to be written: q starts as a copy in w's layout)
        if w_layout == ROW_MAJOR:
            wc, ldw = w.clone(memory_format=torch.contiguous_format), n
        else:
            wc, ldw = w.t().clone(memory_format=torch.contiguous_format).t(), m
    s = torch.empty((n, k), dtype=torch.float64, device=w.device)
    r = torch.empty((n, n), dtype=torch.float64, device=w.device)
    wq, wr = entry.work_space(w.device, m, k, n)
    with torch.cuda.device(w.device):
        st = _f64_call(entry.symbol, lib().tsqr_mi_orth_f64, stream, v_layout, w_layout, int(passes), int(bool(reorth)), wc.data_ptr(), ldw,
                       s.data_ptr(), k, r.data_ptr(), n, vc.data_ptr(), ldv, m, k, n, wq.data_ptr(), wr.data_ptr())
    if st:
        raise OrthError(st, "orth_f64_tensor: state %d: %s" % (st, last_error()))
    return wc, s.t(), r.t()


def get_working_q_size_f64_dist(m_local, n, nranks):
    """Doubles of wq for tsqr_mi_qr_f64_dist* (dist.RowPartitionedQRF64 allocates them itself)."""
    return lib().tsqr_mi_working_q_size_f64_dist(m_local, n, nranks)


def get_working_r_size_f64_dist(m_local, n, nranks):
    """Doubles of wr for tsqr_mi_qr_f64_dist*."""
    return lib().tsqr_mi_working_r_size_f64_dist(m_local, n, nranks)


def last_sweeps_f64():
    """Sweeps of this thread's last qr_f64 / qr_f64_wide / r_f64 / lstsq_f64 / row-partitioned fp64 call, plus 100 when it took the shifted path."""
    return lib().tsqr_mi_last_sweeps_f64()


def last_jacobi_sweeps_f64():
    """Jacobi sweeps of this thread's last svd_f64 / svd_f64_tensor call, the final sweep without a rotation included."""
    return lib().tsqr_mi_last_jacobi_sweeps_f64()


def set_tuning(level0_waves=0, tree_chunks_per_wave=0):
    lib().tsqr_mi_set_tuning(level0_waves, tree_chunks_per_wave)


KERNEL_CLASSES = ["fold_level0", "fold_tree", "trinv", "apply", "coupling", "other", "gram", "chol"]


def profile_enable(on=True):
    lib().tsqr_mi_profile_enable(int(bool(on)))


def profile_read():
    """{class: (milliseconds, launches)} accumulated since profile_enable(True)."""
    ms = (ctypes.c_double * 8)()
    cnt = (ctypes.c_long * 8)()
    k = lib().tsqr_mi_profile_read(ms, cnt, 8)
    return {KERNEL_CLASSES[i]: (ms[i], cnt[i]) for i in range(k)}


POLICY_AUTO, POLICY_HOUSEHOLDER, POLICY_GRAM_F64, POLICY_GRAM_BF16, POLICY_AUTO_NO_BF16 = 0, 1, 2, 3, 4
ENGINE_NAMES = {0: "householder_tsqr", 1: "gram_f64_cholesky", 2: "gram_rejected_then_householder", 3: "gram_bf16x3_cholesky",
                4: "gram_rejected_then_shifted_cholesky_qr2", 5: "gram_bf16x3_cholesky_one_panel_128"}


def set_policy(policy):
    """R-factor engine policy (include/tsqr_mi.h)."""
    lib().tsqr_mi_set_policy(int(policy))


def last_engine():
    return lib().tsqr_mi_last_engine()

"""Speed of the fp64 entries (tsqr_mi_qr_f64, n <= 64, and tsqr_mi_qr_f64_wide, the wide_* cases): median time of blocking calls per
case, the sweep count, effective TB/s (24 m n bytes per sweep: the Gram pass reads A, the apply pass reads A and writes Q), for the wide
cases the fp64 rate of one sweep's executed products (2 m n^2, Gram pass and apply pass together), and torch.linalg.qr(float64) on the
same GPU for 2^20 x 64 and for every wide shape.  Prints one JSON line.  Usage: python tools/f64_speed.py [--calls 50] [--warmup 5]
--dist1: instead, the cost of the row-partitioned entry's hook on ONE rank -- tsqr_mi_qr_f64_dist_fn over a one-rank raw RCCL communicator
against the plain entry on the same operands, calls interleaved in this process, at 2^20 x 64 and 2^18 x 256.  (One rank: the all-reduce
moves nothing between GPUs; this says nothing about several ranks.)
--r-only: instead, the R-only entry (tsqr_mi_r_f64) next to tsqr_mi_qr_f64 on the same operands in this process, at 2^20, 2^16 and
2^23 rows x 64: Gaussian with reorth = 0 and 1, and cond 1e12.  Per case the median of --calls blocking calls of each entry, the sweep
counts, the ratio r_only / full and whether the one-sweep R is bitwise the full call's.  Writes nothing itself: redirect the JSON line
(profiles/fp64_r_speed.json).
--lstsq: instead, the least-squares entry (tsqr_mi_lstsq_f64, reorth = 0) with refine 0 and 1, tsqr_mi_r_f64 alone and
torch.linalg.lstsq(float64) on the same Gaussian operands in this process, at 2^16, 2^20 and 2^23 rows x 64 with 1 and 16 right-hand
sides: the median of --calls blocking calls each (torch at 2^23 rows: of five).  Redirect the JSON line (profiles/fp64_lstsq_speed.json).
--row-major: instead, the layout entries (tsqr_mi_r_f64_lay with reorth 0 and 1, tsqr_mi_lstsq_f64_lay with refine 1 and 16 right-hand
sides) at 2^16, 2^20 and 2^23 rows x 64 and 2^20 x 16, Gaussian, three arms interleaved call by call in this process: (i) the layout
entry on row-major operands, (ii) the column-major entry on operands transposed beforehand, (iii) the transposing copy of each operand
(t().contiguous().t(), allocation included: what lstsq_f64 did to a contiguous tensor before the layout entries) followed by the
column-major entry.  Arm (ii) runs three times per round: the max / min of its three medians is the spread a ratio has to be read
against.  Per arm the median of --calls blocking calls; the ratios i / ii and i / iii; whether R and X of (i) are bitwise those of (ii).
Redirect the JSON line (profiles/fp64_rowmajor_speed.json).
--qr-row-major: instead, the full QR's layout entry (tsqr_mi_qr_f64_lay, reorth 0 and 1) at the shapes and under the protocol of
--row-major: (i) the layout entry on row-major A and Q, (ii) tsqr_mi_qr_f64 on operands transposed beforehand, (iii) the transposing
copy of A (t().contiguous().t()), tsqr_mi_qr_f64 and a transposing copy of Q back into row-major storage, waited for.  Asserts that Q
and R of (i) are bitwise those of (ii) in every case.  Redirect the JSON line (profiles/fp64_qr_rowmajor_speed.json)."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cond_matrix(torch, m, n, cond, seed):
    # A = U diag(s) V^T built in fp64 (torch's QR on the GPU only shapes the test matrix; the measured call is the engine's)
    g = torch.Generator(device="cuda").manual_seed(seed)
    u, _ = torch.linalg.qr(torch.randn(m, n, dtype=torch.float64, device="cuda", generator=g))
    v, _ = torch.linalg.qr(torch.randn(n, n, dtype=torch.float64, device="cuda", generator=g))
    s = torch.logspace(0.0, -float(torch.log10(torch.tensor(cond))), n, dtype=torch.float64, device="cuda")
    return (u * s) @ v.T


def time_case(torch, bq, a_rm, reorth, calls, warmup, wide=False):
    m, n = a_rm.shape
    a = a_rm.T.contiguous()                                 # (n, m): column-major m x n
    q = torch.empty_like(a)
    r = torch.empty(n, n, dtype=torch.float64, device="cuda")
    bf = bq.buffer_f64_wide(reorth) if wide else bq.buffer_f64(reorth)
    bf.allocate(m, n)
    entry = bq.qr_f64_wide if wide else bq.qr_f64
    for _ in range(warmup):
        assert entry(q, m, r, n, a, m, m, n, bf) == 0, bq.last_error()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        st = entry(q, m, r, n, a, m, m, n, bf)
        ts.append(time.perf_counter() - t0)
        assert st == 0
    ts.sort()
    med = ts[len(ts) // 2]
    sweeps = bq.last_sweeps_f64()
    nsw = sweeps % 100
    eye = torch.eye(n, dtype=torch.float64, device="cuda")
    qm = q.T
    orth = torch.linalg.norm(qm.T @ qm - eye).item()
    out = {"m": m, "n": n, "reorth": reorth, "median_ms": med * 1e3, "min_ms": ts[0] * 1e3, "sweeps": sweeps,
           "eff_TBps": 24.0 * m * n * nsw / med / 1e12, "orth_fro": orth}
    if wide:
        out["products_TFps"] = 2.0 * m * n * n * nsw / med / 1e12
    return out


def time_torch_qr(torch, a_rm, reps=3):
    torch.linalg.qr(a_rm)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        torch.linalg.qr(a_rm)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2] * 1e3


def r_only(torch, bq, calls, warmup):
    n = 64
    out = {"tool": "f64_speed --r-only", "calls": calls, "warmup": warmup, "cases": []}

    def timed(call):
        for _ in range(warmup):
            assert call() == 0, bq.last_error()
        ts = []
        for _ in range(calls):
            t0 = time.perf_counter()
            st = call()                                     # (blocking: returns when the stream has drained)
            ts.append(time.perf_counter() - t0)
            assert st == 0
        ts.sort()
        return ts[len(ts) // 2] * 1e3, ts[0] * 1e3, bq.last_sweeps_f64()

    for lg in (20, 16, 23):
        m = 1 << lg
        gauss = lambda: torch.randn(m, n, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(lg))
        for name, make, reorth in (("gauss_2p%d_r0" % lg, gauss, 0), ("gauss_2p%d_r1" % lg, gauss, 1),
                                   ("cond1e12_2p%d_r0" % lg, lambda: cond_matrix(torch, m, n, 1e12, lg), 0)):
            a = make().T.contiguous()                       # (n, m): column-major m x n
            q = torch.empty_like(a)
            r_full = torch.empty(n, n, dtype=torch.float64, device="cuda")
            r_only_ = torch.empty(n, n, dtype=torch.float64, device="cuda")
            bf, bfr = bq.buffer_f64(reorth), bq.buffer_f64_r(reorth)
            bf.allocate(m, n)
            bfr.allocate(m, n)
            full = timed(lambda: bq.qr_f64(q, m, r_full, n, a, m, m, n, bf))
            ronly = timed(lambda: bq.r_f64(r_only_, n, a, m, m, n, bfr))
            dr = (torch.linalg.norm(r_only_ - r_full) / torch.linalg.norm(r_full)).item()
            out["cases"].append({"case": name, "m": m, "n": n, "reorth": reorth,
                                 "full_median_ms": full[0], "full_min_ms": full[1], "full_sweeps": full[2],
                                 "r_only_median_ms": ronly[0], "r_only_min_ms": ronly[1], "r_only_sweeps": ronly[2],
                                 "ratio_r_only_over_full": ronly[0] / full[0], "r_bitwise_equal": bool(torch.equal(r_only_, r_full)),
                                 "r_rel_diff": dr, "work_bytes_full": bf.get_device_memory_size() + 8 * q.numel(),
                                 "work_bytes_r_only": bfr.get_device_memory_size()})
            del a, q, bf, bfr
            torch.cuda.empty_cache()
    print(json.dumps(out))


def lstsq(torch, bq, calls, warmup):
    import ctypes
    L = bq.lib()
    vp = ctypes.c_void_p
    n = 64
    out = {"tool": "f64_speed --lstsq", "calls": calls, "warmup": warmup, "cases": []}

    def timed(call):
        for _ in range(warmup):
            assert call() == 0, bq.last_error()
        ts = []
        for _ in range(calls):
            t0 = time.perf_counter()
            st = call()                                     # (blocking: returns when the stream has drained)
            ts.append(time.perf_counter() - t0)
            assert st == 0
        ts.sort()
        return ts[len(ts) // 2] * 1e3, ts[0] * 1e3

    for lg in (16, 20, 23):
        m = 1 << lg
        g = torch.Generator(device="cuda").manual_seed(lg)
        a = torch.randn(n, m, dtype=torch.float64, device="cuda", generator=g)      # (n, m): column-major m x n
        r = torch.empty(n, n, dtype=torch.float64, device="cuda")
        bfr = bq.buffer_f64_r(False)
        bfr.allocate(m, n)
        ronly = timed(lambda: bq.r_f64(r, n, a, m, m, n, bfr))
        r_sweeps = bq.last_sweeps_f64()
        for nrhs in (1, 16):
            b = torch.randn(nrhs, m, dtype=torch.float64, device="cuda", generator=g)
            x = torch.empty(nrhs, n, dtype=torch.float64, device="cuda")
            wq = torch.empty(L.tsqr_mi_working_q_size_f64_lstsq(m, n, nrhs), dtype=torch.float64, device="cuda")
            wr = torch.empty(L.tsqr_mi_working_r_size_f64_lstsq(m, n, nrhs), dtype=torch.float64, device="cuda")
            st = torch.cuda.current_stream().cuda_stream
            case = {"m": m, "n": n, "nrhs": nrhs, "r_only_median_ms": ronly[0], "r_only_min_ms": ronly[1], "r_only_sweeps": r_sweeps,
                    "work_bytes": 8 * (wq.numel() + wr.numel())}
            for refine in (0, 1):
                t = timed(lambda: L.tsqr_mi_lstsq_f64(0, refine, vp(x.data_ptr()), n, vp(r.data_ptr()), n, vp(a.data_ptr()), m,
                                                      vp(b.data_ptr()), m, m, n, nrhs, vp(wq.data_ptr()), vp(wr.data_ptr()), vp(st)))
                case["lstsq_refine%d_median_ms" % refine], case["lstsq_refine%d_min_ms" % refine] = t
                case["lstsq_sweeps"] = bq.last_sweeps_f64()
            case["ms_per_pass"] = case["lstsq_refine1_median_ms"] - case["lstsq_refine0_median_ms"]
            am, bm = a.T, b.T                               # torch's driver on the same operands (it copies what it overwrites)

            def torch_call():
                torch.linalg.lstsq(am, bm)
                torch.cuda.synchronize()
                return 0
            tt = timed(torch_call) if lg < 23 else (None, None)
            if lg == 23:                                    # (five calls: the library's solve takes long at this size)
                torch_call()
                ts = []
                for _ in range(5):
                    t0 = time.perf_counter()
                    torch_call()
                    ts.append(time.perf_counter() - t0)
                ts.sort()
                tt = (ts[2] * 1e3, ts[0] * 1e3)
            case["torch_lstsq_median_ms"], case["torch_lstsq_min_ms"] = tt
            xt = torch.linalg.lstsq(am, bm).solution
            # ||A^T (B - A X)||_F / (||A||_F ||B||_F) in fp64 on the GPU, for the entry's X (refine = 1) and for torch's
            nres = lambda xs: (torch.linalg.norm(am.T @ (bm - am @ xs)) / (torch.linalg.norm(am) * torch.linalg.norm(bm))).item()
            case["normal_residual_lstsq"], case["normal_residual_torch"] = nres(x.T), nres(xt)
            case["rel_diff_to_torch"] = (torch.linalg.norm(x.T - xt) / torch.linalg.norm(xt)).item()
            case["norm_x_lstsq"], case["norm_x_torch"] = torch.linalg.norm(x).item(), torch.linalg.norm(xt).item()
            for k, v in case.items():                       # (torch's solution at 2^23 rows came back non-finite: null in the JSON line)
                if isinstance(v, float) and not math.isfinite(v):
                    case[k] = None
            out["cases"].append(case)
            del b, x, wq, wr, xt
        del a, r, bfr
        torch.cuda.empty_cache()
    print(json.dumps(out))


def row_major(torch, bq, calls, warmup):
    import ctypes
    L = bq.lib()
    vp = ctypes.c_void_p
    out = {"tool": "f64_speed --row-major", "calls": calls, "warmup": warmup, "cases": []}
    for lg, n in ((16, 64), (20, 64), (23, 64), (20, 16)):
        m, nrhs = 1 << lg, 16
        g = torch.Generator(device="cuda").manual_seed(lg + n)
        a_rm = torch.randn(m, n, dtype=torch.float64, device="cuda", generator=g)        # row-major m x n
        b_rm = torch.randn(m, nrhs, dtype=torch.float64, device="cuda", generator=g)
        a_cm, b_cm = a_rm.t().contiguous(), b_rm.t().contiguous()                          # (n, m): column-major m x n
        x = [torch.empty(nrhs, n, dtype=torch.float64, device="cuda") for _ in range(2)]
        r = [torch.empty(n, n, dtype=torch.float64, device="cuda") for _ in range(2)]
        wq = torch.empty(L.tsqr_mi_working_q_size_f64_lstsq(m, n, nrhs), dtype=torch.float64, device="cuda")
        wr = torch.empty(L.tsqr_mi_working_r_size_f64_lstsq(m, n, nrhs), dtype=torch.float64, device="cuda")
        st = vp(torch.cuda.current_stream().cuda_stream)
        work = (vp(wq.data_ptr()), vp(wr.data_ptr()), st)

        def r_call(lay, a, lda, reorth, k):
            return L.tsqr_mi_r_f64_lay(lay, reorth, vp(r[k].data_ptr()), n, vp(a.data_ptr()), lda, m, n, *work)

        def l_call(lay, a, lda, b, ldb, k):
            return L.tsqr_mi_lstsq_f64_lay(lay, lay, 0, 1, vp(x[k].data_ptr()), n, vp(r[k].data_ptr()), n, vp(a.data_ptr()), lda,
                                           vp(b.data_ptr()), ldb, m, n, nrhs, *work)

        def copy_then(call, with_b):
            a_c = a_rm.t().contiguous()                     # (the copy is enqueued on the stream of the call behind it)
            b_c = b_rm.t().contiguous() if with_b else None
            return call(a_c, b_c)

        kinds = [("r_f64_reorth0", lambda lay, a, lda, b, ldb, k: r_call(lay, a, lda, 0, k), False),
                 ("r_f64_reorth1", lambda lay, a, lda, b, ldb, k: r_call(lay, a, lda, 1, k), False),
                 ("lstsq_f64_refine1_nrhs16", l_call, True)]
        for kind, call, with_b in kinds:
            ii = lambda: call(0, a_cm, m, b_cm, m, 1)
            arms = [("i_row_major", lambda: call(1, a_rm, n, b_rm, nrhs, 0)), ("ii_col_major", ii),
                    ("iii_copy_then_col_major", lambda: copy_then(lambda ac, bc: call(0, ac, m, bc if with_b else b_cm, m, 1), with_b)),
                    ("ii_col_major_again", ii), ("ii_col_major_third", ii)]
            ts = {name: [] for name, _ in arms}
            for i in range(warmup + calls):
                for name, fn in arms:
                    t0 = time.perf_counter()
                    rc = fn()                               # (blocking: returns when the stream has drained)
                    dt = time.perf_counter() - t0
                    assert rc == 0, bq.last_error()
                    if i >= warmup:
                        ts[name].append(dt)
            med = {k: sorted(v)[len(v) // 2] * 1e3 for k, v in ts.items()}
            ii_meds = [med["ii_col_major"], med["ii_col_major_again"], med["ii_col_major_third"]]
            arms[0][1]()
            arms[1][1]()
            case = {"m": m, "n": n, "call": kind, "sweeps": bq.last_sweeps_f64(),
                    "i_row_major_median_ms": med["i_row_major"], "ii_col_major_median_ms": sorted(ii_meds)[1],
                    "iii_copy_then_col_major_median_ms": med["iii_copy_then_col_major"],
                    "ii_medians_ms": ii_meds, "ii_spread_max_over_min": max(ii_meds) / min(ii_meds),
                    "ratio_i_over_ii": med["i_row_major"] / sorted(ii_meds)[1],
                    "ratio_i_over_iii": med["i_row_major"] / med["iii_copy_then_col_major"],
                    "i_not_slower_than_iii": bool(med["i_row_major"] <= med["iii_copy_then_col_major"]),
                    "r_bitwise_equal": bool(torch.equal(r[0], r[1])),
                    "x_bitwise_equal": bool(torch.equal(x[0], x[1])) if with_b else None}
            out["cases"].append(case)
        del a_rm, b_rm, a_cm, b_cm, x, r, wq, wr
        torch.cuda.empty_cache()
    print(json.dumps(out))


def qr_row_major(torch, bq, calls, warmup):
    import ctypes
    L = bq.lib()
    vp = ctypes.c_void_p
    out = {"tool": "f64_speed --qr-row-major", "calls": calls, "warmup": warmup, "cases": []}
    for lg, n in ((16, 64), (20, 64), (23, 64), (20, 16)):
        m = 1 << lg
        g = torch.Generator(device="cuda").manual_seed(lg + n)
        a_rm = torch.randn(m, n, dtype=torch.float64, device="cuda", generator=g)        # row-major m x n
        a_cm = a_rm.t().contiguous()                                                       # (n, m): column-major m x n
        q_rm, q_cm = torch.empty_like(a_rm), torch.empty_like(a_cm)
        r = [torch.empty(n, n, dtype=torch.float64, device="cuda") for _ in range(2)]
        wq = torch.empty(L.tsqr_mi_working_q_size_f64(m, n), dtype=torch.float64, device="cuda")
        wr = torch.empty(L.tsqr_mi_working_r_size_f64(m, n), dtype=torch.float64, device="cuda")
        work = (vp(wq.data_ptr()), vp(wr.data_ptr()), vp(torch.cuda.current_stream().cuda_stream))

        def call(lay, q, a, ld, reorth, k):
            return L.tsqr_mi_qr_f64_lay(lay, lay, reorth, vp(q.data_ptr()), ld, vp(r[k].data_ptr()), n, vp(a.data_ptr()), ld, m, n, *work)

        def copy_in_out(reorth):
            a_c = a_rm.t().contiguous()                     # (the copy is enqueued on the stream of the call behind it)
            rc = call(0, q_cm, a_c, m, reorth, 1)
            q_out = q_cm.t().contiguous()                   # Q back in the caller's layout
            torch.cuda.synchronize()
            del q_out
            return rc

        for reorth in (0, 1):
            ii = lambda: call(0, q_cm, a_cm, m, reorth, 1)
            arms = [("i_row_major", lambda: call(1, q_rm, a_rm, n, reorth, 0)), ("ii_col_major", ii),
                    ("iii_copy_in_col_major_copy_out", lambda: copy_in_out(reorth)),
                    ("ii_col_major_again", ii), ("ii_col_major_third", ii)]
            ts = {name: [] for name, _ in arms}
            for i in range(warmup + calls):
                for name, fn in arms:
                    t0 = time.perf_counter()
                    rc = fn()                               # (blocking: returns when the stream has drained)
                    dt = time.perf_counter() - t0
                    assert rc == 0, bq.last_error()
                    if i >= warmup:
                        ts[name].append(dt)
            med = {k: sorted(v)[len(v) // 2] * 1e3 for k, v in ts.items()}
            ii_meds = [med["ii_col_major"], med["ii_col_major_again"], med["ii_col_major_third"]]
            arms[1][1]()
            sweeps_ii = bq.last_sweeps_f64()
            arms[0][1]()
            sweeps_i = bq.last_sweeps_f64()
            q_equal, r_equal = bool(torch.equal(q_rm, q_cm.t())), bool(torch.equal(r[0], r[1]))
            assert q_equal and r_equal and sweeps_i == sweeps_ii, (m, n, reorth, q_equal, r_equal, sweeps_i, sweeps_ii)
            out["cases"].append({"m": m, "n": n, "call": "qr_f64_reorth%d" % reorth, "sweeps": sweeps_i,
                                 "i_row_major_median_ms": med["i_row_major"], "ii_col_major_median_ms": sorted(ii_meds)[1],
                                 "iii_copy_in_col_major_copy_out_median_ms": med["iii_copy_in_col_major_copy_out"],
                                 "ii_medians_ms": ii_meds, "ii_spread_max_over_min": max(ii_meds) / min(ii_meds),
                                 "ratio_i_over_ii": med["i_row_major"] / sorted(ii_meds)[1],
                                 "ratio_i_over_iii": med["i_row_major"] / med["iii_copy_in_col_major_copy_out"],
                                 "i_faster_than_iii": bool(med["i_row_major"] < med["iii_copy_in_col_major_copy_out"]),
                                 "q_bitwise_equal": q_equal, "r_bitwise_equal": r_equal})
        del a_rm, a_cm, q_rm, q_cm, r, wq, wr
        torch.cuda.empty_cache()
    print(json.dumps(out))


def dist1(torch, bq, calls, warmup):
    import ctypes
    rccl = ctypes.CDLL("librccl.so")

    class UniqueId(ctypes.Structure):
        _fields_ = [("internal", ctypes.c_byte * 128)]

    uid = UniqueId()
    assert rccl.ncclGetUniqueId(ctypes.byref(uid)) == 0
    comm = ctypes.c_void_p()
    rccl.ncclCommInitRank.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, UniqueId, ctypes.c_int]
    assert rccl.ncclCommInitRank(ctypes.byref(comm), 1, uid, 0) == 0
    allreduce = ctypes.cast(rccl.ncclAllReduce, ctypes.c_void_p)
    L = bq.lib()
    out = {"tool": "f64_speed --dist1", "calls": calls, "cases": []}
    try:
        for m, n in ((1 << 20, 64), (1 << 18, 256)):
            a = torch.randn(n, m, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
            q = torch.empty_like(a)
            r = torch.empty(n, n, dtype=torch.float64, device="cuda")
            wq = torch.empty(L.tsqr_mi_working_q_size_f64_dist(m, n, 1), dtype=torch.float64, device="cuda")
            wr = torch.empty(L.tsqr_mi_working_r_size_f64_dist(m, n, 1), dtype=torch.float64, device="cuda")
            st = torch.cuda.current_stream().cuda_stream
            head = (0, q.data_ptr(), m, r.data_ptr(), n, a.data_ptr(), m, m, n, wq.data_ptr(), wr.data_ptr())
            plain = lambda: L.tsqr_mi_qr_f64_wide(*head, st)
            hooked = lambda: L.tsqr_mi_qr_f64_dist_fn(*head, comm, allreduce, 1, st)
            ts = {"plain": [], "dist1": []}
            for i in range(warmup + calls):
                for name, fn in (("plain", plain), ("dist1", hooked)):
                    t0 = time.perf_counter()
                    rc = fn()
                    dt = time.perf_counter() - t0
                    assert rc == 0, bq.last_error()
                    if i >= warmup:
                        ts[name].append(dt)
            med = {k: sorted(v)[len(v) // 2] * 1e3 for k, v in ts.items()}
            lo = {k: min(v) * 1e3 for k, v in ts.items()}
            out["cases"].append({"m": m, "n": n, "sweeps": L.tsqr_mi_last_sweeps_f64(), "plain_median_ms": med["plain"],
                                 "dist1_median_ms": med["dist1"], "plain_min_ms": lo["plain"], "dist1_min_ms": lo["dist1"]})
            del a, q, r, wq, wr
            torch.cuda.empty_cache()
    finally:
        rccl.ncclCommDestroy.argtypes = [ctypes.c_void_p]
        rccl.ncclCommDestroy(comm)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cases", default="", help="comma-separated case names (default: all)")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch.linalg.qr baseline")
    ap.add_argument("--r-only", action="store_true", help="time tsqr_mi_r_f64 next to tsqr_mi_qr_f64 on the same operands")
    ap.add_argument("--lstsq", action="store_true", help="time tsqr_mi_lstsq_f64 next to tsqr_mi_r_f64 and torch.linalg.lstsq")
    ap.add_argument("--row-major", action="store_true", help="time the layout entries on row-major operands next to the column-major entries")
    ap.add_argument("--qr-row-major", action="store_true", help="time tsqr_mi_qr_f64_lay on row-major A and Q next to tsqr_mi_qr_f64")
    ap.add_argument("--dist1", action="store_true", help="time the one-rank row-partitioned call over raw RCCL next to the plain entry")
    args = ap.parse_args()
    import torch
    from tsqr_gpu_amd import blockqr as bq
    if args.dist1:
        return dist1(torch, bq, args.calls, args.warmup)
    if args.r_only:
        return r_only(torch, bq, args.calls, args.warmup)
    if args.lstsq:
        return lstsq(torch, bq, args.calls, args.warmup)
    if args.row_major:
        return row_major(torch, bq, args.calls, args.warmup)
    if args.qr_row_major:
        return qr_row_major(torch, bq, args.calls, args.warmup)
    n = 64
    out = {"tool": "f64_speed", "cases": []}
    gauss = lambda m, seed: torch.randn(m, n, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))
    cases = [("gauss_2p20_r0", lambda: gauss(1 << 20, 1), 0), ("gauss_2p20_r1", lambda: gauss(1 << 20, 1), 1),
             ("cond1e12_2p20_r0", lambda: cond_matrix(torch, 1 << 20, n, 1e12, 2), 0),
             ("gauss_2p16_r0", lambda: gauss(1 << 16, 3), 0), ("gauss_2p23_r0", lambda: gauss(1 << 23, 4), 0)]
    wgauss = lambda m, n, seed: torch.randn(m, n, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))
    wide_shapes = [("2p18x128", 1 << 18, 128), ("2p18x256", 1 << 18, 256), ("2p16x1024", 1 << 16, 1024)]
    wide = []
    for tag, m, wn in wide_shapes:
        wide += [("wide_gauss_%s_r0" % tag, (lambda m=m, wn=wn: wgauss(m, wn, 5)), 0),
                 ("wide_gauss_%s_r1" % tag, (lambda m=m, wn=wn: wgauss(m, wn, 5)), 1),
                 ("wide_cond1e12_%s_r0" % tag, (lambda m=m, wn=wn: cond_matrix(torch, m, wn, 1e12, 6)), 0)]
    only = [c for c in args.cases.split(",") if c]
    for name, make, reorth in cases + wide:
        if only and name not in only:
            continue
        res = time_case(torch, bq, make(), reorth, args.calls, args.warmup, wide=name.startswith("wide_"))
        res["case"] = name
        out["cases"].append(res)
        torch.cuda.empty_cache()
    if args.no_torch:
        print(json.dumps(out))
        return
    if not only or any(not c.startswith("wide_") for c in only):
        out["torch_linalg_qr_f64_2p20x64_ms"] = time_torch_qr(torch, gauss(1 << 20, 1))
    for tag, m, wn in wide_shapes:
        if only and not any(tag in c for c in only):
            continue
        out["torch_linalg_qr_f64_%s_ms" % tag] = time_torch_qr(torch, wgauss(m, wn, 5))
        torch.cuda.empty_cache()
    for c in out["cases"]:
        tq = out.get("torch_linalg_qr_f64_2p%dx%d_ms" % (c["m"].bit_length() - 1, c["n"]))
        if tq is not None and c["case"].startswith("wide_"):
            c["speedup_vs_torch"] = tq / c["median_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()

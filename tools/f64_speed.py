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
and R of (i) are bitwise those of (ii) in every case.  Redirect the JSON line (profiles/fp64_qr_rowmajor_speed.json).
--wide-row-major: instead, the wide entry's layout form (tsqr_mi_qr_f64_wide_lay, reorth 0 and 1) at 2^18 x 128, 2^18 x 256 and
2^16 x 1024, Gaussian, three arms interleaved call by call in this process on the same operands: (a) the layout entry on row-major A and
Q, (b) tsqr_mi_qr_f64_wide on operands transposed beforehand, (c) what a contiguous tensor cost before: the transposing copy of A,
tsqr_mi_qr_f64_wide and a transposing copy of Q back, waited for.  Per arm the median of --calls (default here: 20) blocking calls; the
ratios a / b and a / c; asserts that Q and R of (a) are bitwise those of (b).  With --parent-lib PATH (another build of libtsqr_mi.so,
the parent commit's) arm (b) alone is also run in fresh processes, alternating PATH (through TSQR_MI_LIB) and the in-tree library, two
runs each: the parent's two medians give the spread the in-tree median is read against, and the checksums of Q and R of the
column-major call are compared.  Writes the JSON to --out (default profiles/fp64_wide_rowmajor_speed.json) and prints it.
--svd: instead, the SVD entry (tsqr_mi_svd_f64, reorth = 0, column-major Gaussian operands) at 2^16, 2^20 and 2^23 rows x 64 and
2^20 x 16 (--cases 2p20x64,... picks some): jobu = 1 interleaved call by call with tsqr_mi_qr_f64_lay, jobu = 0 with tsqr_mi_r_f64_lay,
on the same operands in this process; per arm the median of --calls blocking calls, the ladder and Jacobi sweep counts, the difference
svd - qr (what the Jacobi kernel and the dense apply add), and torch.linalg.svd(float64, full_matrices=False) and
torch.linalg.svdvals on the same matrix (median of three; --no-torch skips them).  Writes the JSON to --svd-out (default
profiles/fp64_svd_speed.json) and prints it.  --svd-arms svd_jobu1 runs that arm alone and writes no file: the run to put under a
kernel trace for the per-kernel split (profiles/fp64_svd_kernel_stats_2p20x64.csv).
--qrcp: instead, the pivoted QR entry (tsqr_mi_qrcp_f64, reorth = 0, column-major Gaussian operands) at the shapes of --svd (--cases
picks some): six arms interleaved call by call on the same operands in this process -- jobq = 1, tsqr_mi_qr_f64_lay, jobq = 0,
tsqr_mi_r_f64_lay, tsqr_mi_svd_f64 with jobu = 0 and with jobu = 1; per arm the median of --calls blocking calls, the ladder sweeps, what
the pivoting kernel and the dense apply add to the entry under them, and the ratio jobq = 0 / svd jobu = 0: the two answers to "what is
the numerical rank".  Writes the JSON to --qrcp-out (default profiles/fp64_qrcp_speed.json) and prints it.  --qrcp-arms qrcp_jobq1
runs that arm alone and writes no file: the run to put under a kernel trace (profiles/fp64_qrcp_kernel_stats_2p20x64.csv).

--lstsq-rank: instead, the rank-aware least-squares entry (tsqr_mi_lstsq_rank_f64, refine 0 and 1, 3 right-hand sides, the default
rcond, reorth = 0, column-major Gaussian operands) at the shapes of --svd, next to tsqr_mi_lstsq_f64_lay at refine 1, tsqr_mi_qrcp_f64
with jobq = 0 and tsqr_mi_r_f64_lay: one process, the five arms interleaved call by call, the median of --calls blocking calls.  Writes
the JSON to --lstsq-rank-out (default profiles/fp64_lstsq_rank_speed.json) and prints it.  --lstsq-rank-arms lstsq_rank_refine1 runs
that arm alone and writes no file: the run to put under a kernel trace (profiles/fp64_lstsq_rank_kernel_stats_2p20x64.csv).
--lstsq-minnorm: instead, the minimum-norm entry (tsqr_mi_lstsq_minnorm_f64, refine 1, 3 right-hand sides, the default rcond) next to
tsqr_mi_lstsq_rank_f64 on the same operands, in one process with the arms interleaved, on the same four shapes; writes the JSON to
--lstsq-minnorm-out (default profiles/fp64_lstsq_minnorm_speed.json) and prints it.
--orth: instead, the block orthogonalisation entry (tsqr_mi_orth_f64) next to the composed form and to qr_f64_wide_tensor on [V W]
(orth() below has the arms and shapes); writes the JSON to --orth-out (default profiles/fp64_orth_speed.json) and prints it;
--orth-arms runs the named arms alone, for a kernel trace."""
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


WIDE_RM_SHAPES = ((18, 128), (18, 256), (16, 1024))


def bits_checksum(torch, t):
    """two 64-bit words over the bit patterns of t's elements in storage order: their wrap-around sum, and the same with element k
    weighted by 2 k + 1 (so that a permutation shows)"""
    v = t.contiguous().view(-1).view(torch.int64)
    w = torch.arange(v.numel(), dtype=torch.int64, device=v.device) * 2 + 1
    return [int(v.sum().item()), int((v * w).sum().item())]


def wide_col_only(torch, bq, calls, warmup):
    """arm (b) of --wide-row-major alone, through an entry every build has: the child processes of --parent-lib"""
    import ctypes
    L = bq.lib()
    vp = ctypes.c_void_p
    out = {"lib": bq.LIB_PATH, "cases": []}
    for lg, n in WIDE_RM_SHAPES:
        m = 1 << lg
        g = torch.Generator(device="cuda").manual_seed(lg + n)
        a_cm = torch.randn(m, n, dtype=torch.float64, device="cuda", generator=g).t().contiguous()     # (n, m): column-major m x n
        q_cm = torch.empty_like(a_cm)
        r = torch.empty(n, n, dtype=torch.float64, device="cuda")
        wq = torch.empty(L.tsqr_mi_working_q_size_f64_wide(m, n), dtype=torch.float64, device="cuda")
        wr = torch.empty(L.tsqr_mi_working_r_size_f64_wide(m, n), dtype=torch.float64, device="cuda")
        st = vp(torch.cuda.current_stream().cuda_stream)
        for reorth in (0, 1):
            ts = []
            for i in range(warmup + calls):
                t0 = time.perf_counter()
                rc = L.tsqr_mi_qr_f64_wide(reorth, vp(q_cm.data_ptr()), m, vp(r.data_ptr()), n, vp(a_cm.data_ptr()), m, m, n,
                                           vp(wq.data_ptr()), vp(wr.data_ptr()), st)
                dt = time.perf_counter() - t0
                assert rc == 0, bq.last_error()
                if i >= warmup:
                    ts.append(dt)
            out["cases"].append({"m": m, "n": n, "reorth": reorth, "median_ms": sorted(ts)[len(ts) // 2] * 1e3, "min_ms": min(ts) * 1e3,
                                 "sweeps": bq.last_sweeps_f64(), "q_checksum": bits_checksum(torch, q_cm), "r_checksum": bits_checksum(torch, r)})
        del a_cm, q_cm, r, wq, wr
        torch.cuda.empty_cache()
    print(json.dumps(out))


def wide_parent_ab(parent_lib, calls, warmup):
    """arm (b) in four fresh processes, parent / in-tree / parent / in-tree, before this process touches the GPU"""
    import subprocess
    runs = []
    for lib in (parent_lib, None, parent_lib, None):
        env = dict(os.environ)
        env.pop("TSQR_MI_LIB", None)
        if lib:
            env["TSQR_MI_LIB"] = os.path.abspath(lib)
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--wide-col-only", "--calls", str(calls), "--warmup", str(warmup)],
                             env=env, capture_output=True, text=True, check=True)
        runs.append(json.loads(res.stdout.strip().splitlines()[-1]))
    p1, n1, p2, n2 = runs
    cases = []
    for cp1, cn1, cp2, cn2 in zip(p1["cases"], n1["cases"], p2["cases"], n2["cases"]):
        pm, nm = [cp1["median_ms"], cp2["median_ms"]], [cn1["median_ms"], cn2["median_ms"]]
        spread = max(pm) / min(pm)
        cases.append({"m": cp1["m"], "n": cp1["n"], "reorth": cp1["reorth"], "parent_medians_ms": pm, "in_tree_medians_ms": nm,
                      "parent_spread_max_over_min": spread, "ratio_in_tree_over_parent": (sum(nm) / 2) / (sum(pm) / 2),
                      "worst_in_tree_over_best_parent": max(nm) / min(pm),
                      "in_tree_within_parent_spread": bool(max(nm) <= max(pm)),
                      "sweeps_parent": cp1["sweeps"], "sweeps_in_tree": cn1["sweeps"],
                      "q_checksum": cn1["q_checksum"], "r_checksum": cn1["r_checksum"],
                      "checksums_equal_to_parent": bool(all(c["q_checksum"] == cp1["q_checksum"] and c["r_checksum"] == cp1["r_checksum"]
                                                            and c["sweeps"] == cp1["sweeps"] for c in (cn1, cp2, cn2)))})
    return {"protocol": "tsqr_mi_qr_f64_wide alone, one fresh process per run in the order parent, in-tree, parent, in-tree; the median "
                        "of %d blocking calls after %d warm-up calls" % (calls, warmup), "cases": cases}


def wide_row_major(torch, bq, calls, warmup, parent):
    import ctypes
    L = bq.lib()
    vp = ctypes.c_void_p
    out = {"tool": "f64_speed --wide-row-major", "calls": calls, "warmup": warmup, "cases": []}
    for lg, n in WIDE_RM_SHAPES:
        m = 1 << lg
        g = torch.Generator(device="cuda").manual_seed(lg + n)
        a_rm = torch.randn(m, n, dtype=torch.float64, device="cuda", generator=g)        # row-major m x n
        a_cm = a_rm.t().contiguous()                                                       # (n, m): column-major m x n
        q_rm, q_cm = torch.empty_like(a_rm), torch.empty_like(a_cm)
        r = [torch.empty(n, n, dtype=torch.float64, device="cuda") for _ in range(2)]
        wq = torch.empty(L.tsqr_mi_working_q_size_f64_wide(m, n), dtype=torch.float64, device="cuda")
        wr = torch.empty(L.tsqr_mi_working_r_size_f64_wide(m, n), dtype=torch.float64, device="cuda")
        work = (vp(wq.data_ptr()), vp(wr.data_ptr()), vp(torch.cuda.current_stream().cuda_stream))

        def row(reorth):
            return L.tsqr_mi_qr_f64_wide_lay(1, 1, reorth, vp(q_rm.data_ptr()), n, vp(r[0].data_ptr()), n, vp(a_rm.data_ptr()), n, m, n, *work)

        def col(reorth, a=None):
            a = a_cm if a is None else a
            return L.tsqr_mi_qr_f64_wide(reorth, vp(q_cm.data_ptr()), m, vp(r[1].data_ptr()), n, vp(a.data_ptr()), m, m, n, *work)

        def copy_in_out(reorth):
            a_c = a_rm.t().contiguous()                     # (the copy is enqueued on the stream of the call behind it)
            rc = col(reorth, a_c)
            q_out = q_cm.t().contiguous()                   # Q back in the caller's layout
            torch.cuda.synchronize()
            del q_out
            return rc

        for reorth in (0, 1):
            arms = [("a_row_major", lambda: row(reorth)), ("b_col_major", lambda: col(reorth)),
                    ("c_copy_in_col_major_copy_out", lambda: copy_in_out(reorth))]
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
            arms[1][1]()
            sweeps_b = bq.last_sweeps_f64()
            arms[0][1]()
            sweeps_a = bq.last_sweeps_f64()
            q_equal, r_equal = bool(torch.equal(q_rm, q_cm.t())), bool(torch.equal(r[0], r[1]))
            assert q_equal and r_equal and sweeps_a == sweeps_b, (m, n, reorth, q_equal, r_equal, sweeps_a, sweeps_b)
            out["cases"].append({"m": m, "n": n, "call": "qr_f64_wide_reorth%d" % reorth, "sweeps": sweeps_a,
                                 "a_row_major_median_ms": med["a_row_major"], "b_col_major_median_ms": med["b_col_major"],
                                 "c_copy_in_col_major_copy_out_median_ms": med["c_copy_in_col_major_copy_out"],
                                 "min_ms": {k: min(v) * 1e3 for k, v in ts.items()},
                                 "ratio_a_over_b": med["a_row_major"] / med["b_col_major"],
                                 "ratio_a_over_c": med["a_row_major"] / med["c_copy_in_col_major_copy_out"],
                                 "a_faster_than_c": bool(med["a_row_major"] < med["c_copy_in_col_major_copy_out"]),
                                 "q_bitwise_equal": q_equal, "r_bitwise_equal": r_equal})
        del a_rm, a_cm, q_rm, q_cm, r, wq, wr
        torch.cuda.empty_cache()
    if parent is not None:
        out["column_major_call_against_parent"] = parent
    return out


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


SVD_SHAPES = ((16, 64), (20, 64), (23, 64), (20, 16))
# work spaces of the arms of --svd and --qrcp: key -> (suffix of the entry's two size functions, their arguments behind m and n)
JOB_WORK = {"svd1": ("_svd", (1,)), "svd0": ("_svd", (0,)), "qrcp1": ("_qrcp", (1,)), "qrcp0": ("_qrcp", (0,)), "qr": ("", ()), "r": ("_r", ())}


def job_work_spaces(torch, L, keys, m, n):
    """{key: (wq, wr, (wq, wr, the current stream) as the three last arguments of a call)} for the keys of JOB_WORK"""
    import ctypes
    vp = ctypes.c_void_p
    stream = vp(torch.cuda.current_stream().cuda_stream)
    work = {}
    for key in keys:
        suffix, extra = JOB_WORK[key]
        wq = torch.empty(getattr(L, "tsqr_mi_working_q_size_f64" + suffix)(m, n, *extra), dtype=torch.float64, device="cuda")
        wr = torch.empty(getattr(L, "tsqr_mi_working_r_size_f64" + suffix)(m, n, *extra), dtype=torch.float64, device="cuda")
        work[key] = (wq, wr, (vp(wq.data_ptr()), vp(wr.data_ptr()), stream))
    return work


def time_arms(bq, arms, calls, warmup, only_arms, read_sweeps):
    """The (name, blocking call) arms interleaved, warmup + calls rounds; only_arms: these alone.  Returns (the arms run, {name: median
    ms}, {name: read_sweeps() after one more call}) -- the last None under only_arms: a run under a kernel trace, which wants the
    medians of the chosen arms and nothing else."""
    if only_arms:
        arms = [arm for arm in arms if arm[0] in only_arms]
    ts = {name: [] for name, _ in arms}
    for i in range(warmup + calls):
        for name, fn in arms:
            t0 = time.perf_counter()
            rc = fn()                                       # (blocking: returns when the stream has drained)
            dt = time.perf_counter() - t0
            assert rc == 0, (name, rc, bq.last_error())
            if i >= warmup:
                ts[name].append(dt)
    med = {k: sorted(x)[len(x) // 2] * 1e3 for k, x in ts.items()}
    if only_arms:
        return arms, med, None
    sweeps = {}
    for name, fn in arms:
        fn()
        sweeps[name] = read_sweeps()
    return arms, med, sweeps


def svd(torch, bq, calls, warmup, only, no_torch, only_arms=()):
    import ctypes
    L = bq.lib()
    vp = ctypes.c_void_p
    out = {"tool": "f64_speed --svd", "calls": calls, "warmup": warmup, "reorth": 0, "layout": "column-major", "cases": []}
    for lg, n in SVD_SHAPES:
        if only and "2p%dx%d" % (lg, n) not in only:
            continue
        m = 1 << lg
        g = torch.Generator(device="cuda").manual_seed(lg + n)
        a_rm = torch.randn(m, n, dtype=torch.float64, device="cuda", generator=g)
        a = a_rm.t().contiguous()                           # (n, m): column-major m x n
        u, q = torch.empty_like(a), torch.empty_like(a)
        s = [torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(2)]
        v = [torch.empty(n, n, dtype=torch.float64, device="cuda") for _ in range(2)]
        r = torch.empty(n, n, dtype=torch.float64, device="cuda")
        work = job_work_spaces(torch, L, ("svd1", "svd0", "qr", "r"), m, n)
        arms = [("svd_jobu1", lambda: L.tsqr_mi_svd_f64(0, 0, 1, 0, vp(u.data_ptr()), m, vp(s[1].data_ptr()), vp(v[1].data_ptr()), n,
                                                        vp(a.data_ptr()), m, m, n, *work["svd1"][2])),
                ("qr_f64_lay", lambda: L.tsqr_mi_qr_f64_lay(0, 0, 0, vp(q.data_ptr()), m, vp(r.data_ptr()), n, vp(a.data_ptr()), m, m, n,
                                                            *work["qr"][2])),
                ("svd_jobu0", lambda: L.tsqr_mi_svd_f64(0, 0, 0, 0, None, m, vp(s[0].data_ptr()), vp(v[0].data_ptr()), n,
                                                        vp(a.data_ptr()), m, m, n, *work["svd0"][2])),
                ("r_f64_lay", lambda: L.tsqr_mi_r_f64_lay(0, 0, vp(r.data_ptr()), n, vp(a.data_ptr()), m, m, n, *work["r"][2]))]
        arms, med, sweeps = time_arms(bq, arms, calls, warmup, only_arms,
                                      lambda: (L.tsqr_mi_last_sweeps_f64(), L.tsqr_mi_last_jacobi_sweeps_f64()))
        if only_arms:
            out["cases"].append({"m": m, "n": n, "median_ms": med})
            continue
        um = u.t()
        orth = torch.linalg.norm(um.T @ um - torch.eye(n, dtype=torch.float64, device="cuda")).item()
        res = (torch.linalg.norm(a_rm - (um * s[1]) @ v[1]) / torch.linalg.norm(a_rm)).item()    # (v[1] read as a tensor is V^T)
        case = {"m": m, "n": n, "svd_jobu1_median_ms": med["svd_jobu1"], "qr_f64_lay_median_ms": med["qr_f64_lay"],
                "svd_jobu0_median_ms": med["svd_jobu0"], "r_f64_lay_median_ms": med["r_f64_lay"],
                "jobu1_minus_qr_ms": med["svd_jobu1"] - med["qr_f64_lay"], "jobu0_minus_r_ms": med["svd_jobu0"] - med["r_f64_lay"],
                "ladder_sweeps": sweeps["svd_jobu1"][0], "jacobi_sweeps": sweeps["svd_jobu1"][1],
                "ladder_sweeps_jobu0": sweeps["svd_jobu0"][0], "jacobi_sweeps_jobu0": sweeps["svd_jobu0"][1],
                "s_bitwise_equal_jobu0_jobu1": bool(torch.equal(s[0], s[1])), "orth_fro": orth, "residual": res}
        if not no_torch:
            def torch_median(fn, reps=3):
                fn()
                torch.cuda.synchronize()
                tt = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    tt.append(time.perf_counter() - t0)
                return sorted(tt)[len(tt) // 2] * 1e3
            case["torch_linalg_svd_ms"] = torch_median(lambda: torch.linalg.svd(a_rm, full_matrices=False))
            case["torch_linalg_svdvals_ms"] = torch_median(lambda: torch.linalg.svdvals(a_rm))
            case["speedup_jobu1_vs_torch_svd"] = case["torch_linalg_svd_ms"] / med["svd_jobu1"]
            case["speedup_jobu0_vs_torch_svdvals"] = case["torch_linalg_svdvals_ms"] / med["svd_jobu0"]
        out["cases"].append(case)
        del a_rm, a, u, q, s, v, r, work
        torch.cuda.empty_cache()
    return out


def qrcp(torch, bq, calls, warmup, only, only_arms=()):
    import ctypes
    L = bq.lib()
    vp = ctypes.c_void_p
    out = {"tool": "f64_speed --qrcp", "calls": calls, "warmup": warmup, "reorth": 0, "layout": "column-major", "cases": []}
    for lg, n in SVD_SHAPES:
        if only and "2p%dx%d" % (lg, n) not in only:
            continue
        m = 1 << lg
        g = torch.Generator(device="cuda").manual_seed(lg + n)
        a_rm = torch.randn(m, n, dtype=torch.float64, device="cuda", generator=g)
        a = a_rm.t().contiguous()                           # (n, m): column-major m x n
        q = [torch.empty_like(a) for _ in range(3)]         # Q of jobq = 1, of the QR entry, U of the SVD
        r = [torch.empty(n, n, dtype=torch.float64, device="cuda") for _ in range(4)]
        jp = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2)]
        s = torch.empty(n, dtype=torch.float64, device="cuda")
        v = torch.empty(n, n, dtype=torch.float64, device="cuda")
        work = job_work_spaces(torch, L, ("qrcp1", "qrcp0", "svd1", "svd0", "qr", "r"), m, n)
        ap_ = vp(a.data_ptr())
        arms = [("qrcp_jobq1", lambda: L.tsqr_mi_qrcp_f64(0, 0, 1, 0, vp(q[0].data_ptr()), m, vp(r[0].data_ptr()), n, vp(jp[0].data_ptr()),
                                                          ap_, m, m, n, *work["qrcp1"][2])),
                ("qr_f64_lay", lambda: L.tsqr_mi_qr_f64_lay(0, 0, 0, vp(q[1].data_ptr()), m, vp(r[1].data_ptr()), n, ap_, m, m, n, *work["qr"][2])),
                ("qrcp_jobq0", lambda: L.tsqr_mi_qrcp_f64(0, 0, 0, 0, None, m, vp(r[2].data_ptr()), n, vp(jp[1].data_ptr()),
                                                          ap_, m, m, n, *work["qrcp0"][2])),
                ("r_f64_lay", lambda: L.tsqr_mi_r_f64_lay(0, 0, vp(r[3].data_ptr()), n, ap_, m, m, n, *work["r"][2])),
                ("svd_jobu0", lambda: L.tsqr_mi_svd_f64(0, 0, 0, 0, None, m, vp(s.data_ptr()), vp(v.data_ptr()), n, ap_, m, m, n, *work["svd0"][2])),
                ("svd_jobu1", lambda: L.tsqr_mi_svd_f64(0, 0, 1, 0, vp(q[2].data_ptr()), m, vp(s.data_ptr()), vp(v.data_ptr()), n,
                                                        ap_, m, m, n, *work["svd1"][2]))]
        arms, med, sweeps = time_arms(bq, arms, calls, warmup, only_arms, L.tsqr_mi_last_sweeps_f64)
        if only_arms:
            out["cases"].append({"m": m, "n": n, "median_ms": med})
            continue
        qm, p = q[0].t(), jp[0].long()
        orth = torch.linalg.norm(qm.T @ qm - torch.eye(n, dtype=torch.float64, device="cuda")).item()
        res = (torch.linalg.norm(a_rm[:, p] - qm @ r[0].t()) / torch.linalg.norm(a_rm)).item()
        d = torch.diagonal(r[0])
        case = {"m": m, "n": n}
        case.update({name + "_median_ms": med[name] for name, _ in arms})
        case.update({"jobq1_minus_qr_ms": med["qrcp_jobq1"] - med["qr_f64_lay"], "jobq0_minus_r_ms": med["qrcp_jobq0"] - med["r_f64_lay"],
                     "jobq0_over_svd_jobu0": med["qrcp_jobq0"] / med["svd_jobu0"], "jobq1_over_svd_jobu1": med["qrcp_jobq1"] / med["svd_jobu1"],
                     "ladder_sweeps": sweeps["qrcp_jobq1"], "ladder_sweeps_jobq0": sweeps["qrcp_jobq0"],
                     "r_and_jpvt_bitwise_equal_jobq0_jobq1": bool(torch.equal(r[0], r[2]) and torch.equal(jp[0], jp[1])),
                     "diag_nonincreasing": bool((d[1:] <= d[:-1]).all().item() and (d >= 0).all().item()),
                     "orth_fro": orth, "residual": res,
                     "checksum_q_qr_f64_lay": float(q[1].sum().item()), "checksum_r_qr_f64_lay": float(r[1].sum().item()),
                     "checksum_r_r_f64_lay": float(r[3].sum().item()), "checksum_s_svd": float(s.sum().item())})
        out["cases"].append(case)
        del a_rm, a, q, r, jp, s, v, work
        torch.cuda.empty_cache()
    return out


def lstsq_rank(torch, bq, calls, warmup, only, only_arms=()):
    """--lstsq-rank: tsqr_mi_lstsq_rank_f64 (refine 0 and 1, the default rcond, 3 right-hand sides) next to tsqr_mi_lstsq_f64_lay at
    refine 1, tsqr_mi_qrcp_f64 at jobq 0 and tsqr_mi_r_f64_lay, column-major Gaussian operands, reorth 0.  No time is set in advance: the
    expected structure of a call is the jobq 0 call plus one dense Gram pass and refine + 1 dense passes, and the JSON reports the
    measured sum next to those parts."""
    import ctypes
    L = bq.lib()
    vp = ctypes.c_void_p
    nrhs = 3
    out = {"tool": "f64_speed --lstsq-rank", "calls": calls, "warmup": warmup, "reorth": 0, "layout": "column-major", "nrhs": nrhs,
           "rcond": "default (max(m, n) 2^-52)", "cases": []}
    for lg, n in SVD_SHAPES:
        if only and "2p%dx%d" % (lg, n) not in only:
            continue
        m = 1 << lg
        g = torch.Generator(device="cuda").manual_seed(lg + n)
        a = torch.randn(m, n, dtype=torch.float64, device="cuda", generator=g).t().contiguous()      # (n, m): column-major m x n
        b = torch.randn(m, nrhs, dtype=torch.float64, device="cuda", generator=g).t().contiguous()
        x = [torch.empty(nrhs, n, dtype=torch.float64, device="cuda") for _ in range(3)]
        r = [torch.empty(n, n, dtype=torch.float64, device="cuda") for _ in range(5)]
        jp = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3)]
        rank = [ctypes.c_int(-1) for _ in range(2)]
        work = job_work_spaces(torch, L, ("qrcp0", "r"), m, n)
        stream = work["r"][2][2]
        sized = {}
        for key, suffix in (("rank", "_lstsq_rank"), ("lstsq", "_lstsq")):
            wq = torch.empty(getattr(L, "tsqr_mi_working_q_size_f64" + suffix)(m, n, nrhs), dtype=torch.float64, device="cuda")
            wr = torch.empty(getattr(L, "tsqr_mi_working_r_size_f64" + suffix)(m, n, nrhs), dtype=torch.float64, device="cuda")
            sized[key] = (wq, wr, (vp(wq.data_ptr()), vp(wr.data_ptr()), stream))
        ap_, bp_ = vp(a.data_ptr()), vp(b.data_ptr())
        rank_arm = lambda i, refine: (lambda: L.tsqr_mi_lstsq_rank_f64(0, 0, 0, refine, -1.0, vp(x[i].data_ptr()), n, vp(r[i].data_ptr()), n,
                                                                     vp(jp[i].data_ptr()), ctypes.byref(rank[i]), ap_, m, bp_, m, m, n, nrhs,
                                                                     *sized["rank"][2]))
        arms = [("lstsq_rank_refine0", rank_arm(0, 0)), ("lstsq_rank_refine1", rank_arm(1, 1)),
                ("lstsq_f64_lay_refine1", lambda: L.tsqr_mi_lstsq_f64_lay(0, 0, 0, 1, vp(x[2].data_ptr()), n, vp(r[2].data_ptr()), n, ap_, m, bp_, m,
                                                                         m, n, nrhs, *sized["lstsq"][2])),
                ("qrcp_jobq0", lambda: L.tsqr_mi_qrcp_f64(0, 0, 0, 0, None, m, vp(r[3].data_ptr()), n, vp(jp[2].data_ptr()), ap_, m, m, n,
                                                          *work["qrcp0"][2])),
                ("r_f64_lay", lambda: L.tsqr_mi_r_f64_lay(0, 0, vp(r[4].data_ptr()), n, ap_, m, m, n, *work["r"][2]))]
        arms, med, sweeps = time_arms(bq, arms, calls, warmup, only_arms, L.tsqr_mi_last_sweeps_f64)
        if only_arms:
            out["cases"].append({"m": m, "n": n, "median_ms": med})
            continue
        case = {"m": m, "n": n}
        case.update({name + "_median_ms": med[name] for name, _ in arms})
        # the parts a call is expected to consist of: the jobq 0 call, the dense Gram pass with the step (refine 0 minus jobq 0 minus one
        # dense pass, itself the difference of the two refine counts)
        dense_pass = med["lstsq_rank_refine1"] - med["lstsq_rank_refine0"]
        case.update({"one_dense_pass_ms": dense_pass, "refine0_minus_jobq0_ms": med["lstsq_rank_refine0"] - med["qrcp_jobq0"],
                     "gram_and_step_ms": med["lstsq_rank_refine0"] - med["qrcp_jobq0"] - dense_pass,
                     "refine1_over_lstsq_f64_refine1": med["lstsq_rank_refine1"] / med["lstsq_f64_lay_refine1"],
                     "rank": rank[1].value, "ladder_sweeps": sweeps["lstsq_rank_refine1"],
                     "r_and_jpvt_bitwise_equal_jobq0": bool(torch.equal(r[1], r[3]) and torch.equal(jp[1], jp[2])),
                     "x_max_abs_diff_to_lstsq_f64": float((x[1] - x[2]).abs().max().item())})
        out["cases"].append(case)
        del a, b, x, r, jp, work, sized
        torch.cuda.empty_cache()
    return out


def lstsq_minnorm(torch, bq, calls, warmup, only):
    """--lstsq-minnorm: tsqr_mi_lstsq_minnorm_f64 next to tsqr_mi_lstsq_rank_f64, both at refine 1 with the default rcond and 3
    right-hand sides, column-major Gaussian operands, reorth 0, and on the same A with its last column a copy of its first (rank n - 1:
    M is not empty).  No time is set in advance: the expected difference is the two single-workgroup kernels the entry adds."""
    import ctypes
    L = bq.lib()
    vp = ctypes.c_void_p
    nrhs = 3
    out = {"tool": "f64_speed --lstsq-minnorm", "calls": calls, "warmup": warmup, "reorth": 0, "layout": "column-major", "nrhs": nrhs,
           "refine": 1, "rcond": "default (max(m, n) 2^-52)", "cases": []}
    for lg, n in SVD_SHAPES:
        if only and "2p%dx%d" % (lg, n) not in only:
            continue
        m = 1 << lg
        g = torch.Generator(device="cuda").manual_seed(lg + n)
        a = torch.randn(m, n, dtype=torch.float64, device="cuda", generator=g).t().contiguous()      # (n, m): column-major m x n
        b = torch.randn(m, nrhs, dtype=torch.float64, device="cuda", generator=g).t().contiguous()
        ac = a.clone()
        ac[n - 1] = ac[0]                                      # the copied column
        x = [torch.empty(nrhs, n, dtype=torch.float64, device="cuda") for _ in range(4)]
        r = [torch.empty(n, n, dtype=torch.float64, device="cuda") for _ in range(4)]
        jp = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(4)]
        rank = [ctypes.c_int(-1) for _ in range(4)]
        stream = job_work_spaces(torch, L, ("r",), m, n)["r"][2][2]
        sized = {}
        for key in ("rank", "minnorm"):
            wq = torch.empty(getattr(L, "tsqr_mi_working_q_size_f64_lstsq_" + key)(m, n, nrhs), dtype=torch.float64, device="cuda")
            wr = torch.empty(getattr(L, "tsqr_mi_working_r_size_f64_lstsq_" + key)(m, n, nrhs), dtype=torch.float64, device="cuda")
            sized[key] = (wq, wr, (vp(wq.data_ptr()), vp(wr.data_ptr()), stream))
        bp_ = vp(b.data_ptr())
        arm = lambda i, key, mat, rcond=-1.0: (lambda: getattr(L, "tsqr_mi_lstsq_%s_f64" % key)(
            0, 0, 0, 1, rcond, vp(x[i].data_ptr()), n, vp(r[i].data_ptr()), n, vp(jp[i].data_ptr()), ctypes.byref(rank[i]), vp(mat.data_ptr()),
            m, bp_, m, m, n, nrhs, *sized[key][2]))
        arms = [("basic", arm(0, "rank", a)), ("minnorm", arm(1, "minnorm", a))]
        copied = [("basic_copied", arm(2, "rank", ac, 1e-8)), ("minnorm_copied", arm(3, "minnorm", ac, 1e-8))]      # (rcond 1e-8 there)
        copied_states = [fn() for _, fn in copied]              # (a state other than 0 is reported, and the pair is not timed)
        arms, med, sweeps = time_arms(bq, arms + (copied if not any(copied_states) else []), calls, warmup, (), L.tsqr_mi_last_sweeps_f64)
        case = {"m": m, "n": n, "copied_states": copied_states}
        case.update({name + "_median_ms": med[name] for name, _ in arms})
        if not any(copied_states):
            case["minnorm_minus_basic_copied_ms"] = med["minnorm_copied"] - med["basic_copied"]
        case.update({"minnorm_minus_basic_ms": med["minnorm"] - med["basic"],
                     "ranks": [v.value for v in rank], "ladder_sweeps": sweeps["minnorm"],
                     "full_rank_x_bitwise_equal": bool(torch.equal(x[0], x[1])),
                     "r_and_jpvt_bitwise_equal": bool(torch.equal(r[0], r[1]) and torch.equal(jp[0], jp[1]) and torch.equal(r[2], r[3])
                                                      and torch.equal(jp[2], jp[3])),
                     "copied_norm_x_basic": float(x[2].norm().item()), "copied_norm_x_minnorm": float(x[3].norm().item())})
        out["cases"].append(case)
        del a, ac, b, x, r, jp, sized
        torch.cuda.empty_cache()
    return out


ORTH_SHAPES = ((20, 64, 64), (20, 256, 64), (20, 1024, 64), (16, 256, 16))


def orth(torch, bq, calls, warmup, only, only_arms=()):
    """--orth: tsqr_mi_orth_f64 (arm a) next to the composition available without it (arm b: w -= v @ (v.T @ w), then qr_f64_tensor in
    place; with passes = 2 both steps twice and the small products S = S1 + S2 R1, R = R2 R1 in torch) and to qr_f64_wide_tensor on
    [V W] (arm c, where k + n <= 1024), at 2^20 x (k = 64, 256, 1024) x 64 and 2^16 x 256 x 16, both layouts, passes 1 and 2, reorth 0.
    V: the Q of a Gaussian matrix (qr_f64_wide_tensor, reorth); W Gaussian.  One process, the arms interleaved call by call, medians of
    --calls blocking calls.  Arms a and b work in place, so each of their calls first copies W into its work tensor; that copy alone is
    the arm copy_w.  No time is set in advance."""
    out = {"tool": "f64_speed --orth", "calls": calls, "warmup": warmup, "reorth": 0, "cases": []}
    for lg, k, n in ORTH_SHAPES:
        tag = "2p%dx%dx%d" % (lg, k, n)
        if only and tag not in only:
            continue
        m = 1 << lg
        g = torch.Generator(device="cuda").manual_seed(lg + k + n)
        v_rm = bq.qr_f64_wide_tensor(torch.randn(m, k, dtype=torch.float64, device="cuda", generator=g), reorth=True, overwrite_a=True)[0]
        w_rm = torch.randn(m, n, dtype=torch.float64, device="cuda", generator=g)
        case = {"m": m, "k": k, "n": n}
        for layout in ("row", "col"):
            row = layout == "row"
            as_layout = (lambda t: t) if row else (lambda t: t.t().contiguous().t())
            v, w0 = as_layout(v_rm), as_layout(w_rm)
            wk = torch.empty_strided(w0.shape, w0.stride(), dtype=torch.float64, device="cuda")
            vw = as_layout(torch.cat([v_rm, w_rm], dim=1)) if k + n <= 1024 else None
            s = torch.empty(n, k, dtype=torch.float64, device="cuda")
            r = torch.empty(n, n, dtype=torch.float64, device="cuda")
            bf = bq.buffer_f64_orth()
            bf.allocate(m, k, n)
            ldv, ldw = (k, n) if row else (m, m)

            def arm_a(passes):
                def call():
                    wk.copy_(w0)
                    return bq.orth_f64(wk, ldw, s, k, r, n, v, ldv, m, k, n, bf, passes=passes, v_row_major=row, w_row_major=row)
                return call

            def arm_b(passes):
                def call():
                    wk.copy_(w0)
                    s_acc = r_acc = None
                    x = wk
                    for _ in range(passes):
                        si = v.t() @ x
                        x -= v @ si
                        x, ri = bq.qr_f64_tensor(x, overwrite_a=True)
                        s_acc, r_acc = (si, ri) if s_acc is None else (s_acc + si @ r_acc, ri @ r_acc)
                    torch.cuda.synchronize()
                    return 0
                return call

            def arm_c():
                bq.qr_f64_wide_tensor(vw)
                return 0

            def copy_w():
                wk.copy_(w0)
                torch.cuda.synchronize()
                return 0

            arms = [("copy_w_" + layout, copy_w)]
            for passes in (1, 2):
                arms += [("a_orth_p%d_%s" % (passes, layout), arm_a(passes)), ("b_composed_p%d_%s" % (passes, layout), arm_b(passes))]
            if vw is not None:
                arms.append(("c_qr_wide_%s" % layout, arm_c))
            arms, med, sweeps = time_arms(bq, arms, calls, warmup, only_arms, bq.last_sweeps_f64)
            case.update({name + "_median_ms": med[name] for name, _ in arms})
            if sweeps is not None:
                case.update({name + "_sweeps": sweeps[name] for name, _ in arms if name.startswith("a_")})
                for passes in (1, 2):
                    a, b = med["a_orth_p%d_%s" % (passes, layout)], med["b_composed_p%d_%s" % (passes, layout)]
                    case["a_over_b_p%d_%s" % (passes, layout)] = a / b
                    if vw is not None:
                        case["a_over_c_p%d_%s" % (passes, layout)] = a / med["c_qr_wide_%s" % layout]
            del v, w0, wk, vw, bf
            torch.cuda.empty_cache()
        out["cases"].append(case)
        del v_rm, w_rm
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=None, help="blocking calls per case or arm (default 50; --wide-row-major: 20)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cases", default="", help="comma-separated case names (default: all)")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch.linalg.qr baseline")
    ap.add_argument("--r-only", action="store_true", help="time tsqr_mi_r_f64 next to tsqr_mi_qr_f64 on the same operands")
    ap.add_argument("--lstsq", action="store_true", help="time tsqr_mi_lstsq_f64 next to tsqr_mi_r_f64 and torch.linalg.lstsq")
    ap.add_argument("--row-major", action="store_true", help="time the layout entries on row-major operands next to the column-major entries")
    ap.add_argument("--qr-row-major", action="store_true", help="time tsqr_mi_qr_f64_lay on row-major A and Q next to tsqr_mi_qr_f64")
    ap.add_argument("--dist1", action="store_true", help="time the one-rank row-partitioned call over raw RCCL next to the plain entry")
    ap.add_argument("--wide-row-major", action="store_true", help="time tsqr_mi_qr_f64_wide_lay on row-major A and Q next to tsqr_mi_qr_f64_wide")
    ap.add_argument("--wide-col-only", action="store_true", help="arm (b) of --wide-row-major alone (the child processes of --parent-lib)")
    ap.add_argument("--parent-lib", default="", help="--wide-row-major: another build of libtsqr_mi.so to run arm (b) against")
    ap.add_argument("--svd", action="store_true", help="time tsqr_mi_svd_f64 (jobu 1 and 0) next to tsqr_mi_qr_f64_lay, tsqr_mi_r_f64_lay and torch.linalg.svd")
    ap.add_argument("--svd-arms", default="", help="--svd: run only these arms (svd_jobu1, qr_f64_lay, svd_jobu0, r_f64_lay) and write no file: for a kernel trace")
    ap.add_argument("--svd-out", default=os.path.join(ROOT, "profiles", "fp64_svd_speed.json"), help="--svd: the JSON file ('' writes none)")
    ap.add_argument("--qrcp", action="store_true", help="time tsqr_mi_qrcp_f64 (jobq 1 and 0) next to tsqr_mi_qr_f64_lay, tsqr_mi_r_f64_lay and tsqr_mi_svd_f64")
    ap.add_argument("--qrcp-arms", default="", help="--qrcp: run only these arms (qrcp_jobq1, qr_f64_lay, qrcp_jobq0, r_f64_lay, svd_jobu0, svd_jobu1) and write no file")
    ap.add_argument("--qrcp-out", default=os.path.join(ROOT, "profiles", "fp64_qrcp_speed.json"), help="--qrcp: the JSON file ('' writes none)")
    ap.add_argument("--lstsq-rank", action="store_true", help="time tsqr_mi_lstsq_rank_f64 (refine 0 and 1) next to tsqr_mi_lstsq_f64_lay, tsqr_mi_qrcp_f64 (jobq 0) and tsqr_mi_r_f64_lay")
    ap.add_argument("--lstsq-rank-arms", default="", help="--lstsq-rank: run only these arms (lstsq_rank_refine0, lstsq_rank_refine1, lstsq_f64_lay_refine1, qrcp_jobq0, r_f64_lay) and write no file")
    ap.add_argument("--lstsq-rank-out", default=os.path.join(ROOT, "profiles", "fp64_lstsq_rank_speed.json"), help="--lstsq-rank: the JSON file ('' writes none)")
    ap.add_argument("--lstsq-minnorm", action="store_true", help="time tsqr_mi_lstsq_minnorm_f64 next to tsqr_mi_lstsq_rank_f64 (refine 1), arms interleaved")
    ap.add_argument("--lstsq-minnorm-out", default=os.path.join(ROOT, "profiles", "fp64_lstsq_minnorm_speed.json"), help="--lstsq-minnorm: the JSON file ('' writes none)")
    ap.add_argument("--orth", action="store_true", help="time tsqr_mi_orth_f64 next to the composed form (torch.matmul + qr_f64_tensor) and qr_f64_wide_tensor on [V W]")
    ap.add_argument("--orth-arms", default="", help="--orth: run only these arms (e.g. a_orth_p2_col) and write no file: for a kernel trace")
    ap.add_argument("--orth-out", default=os.path.join(ROOT, "profiles", "fp64_orth_speed.json"), help="--orth: the JSON file ('' writes none)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp64_wide_rowmajor_speed.json"), help="--wide-row-major: the JSON file")
    args = ap.parse_args()
    wide_rm = args.wide_row_major or args.wide_col_only
    if args.calls is None:
        args.calls = 20 if wide_rm else 50
    parent = wide_parent_ab(args.parent_lib, args.calls, args.warmup) if args.wide_row_major and args.parent_lib else None
    import torch
    from tsqr_gpu_amd import blockqr as bq
    if args.wide_col_only:
        return wide_col_only(torch, bq, args.calls, args.warmup)
    if args.wide_row_major:
        out = wide_row_major(torch, bq, args.calls, args.warmup, parent)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
        print(json.dumps(out))
        return
    if args.svd:
        only_arms = [c for c in args.svd_arms.split(",") if c]
        out = svd(torch, bq, args.calls, args.warmup, [c for c in args.cases.split(",") if c], args.no_torch, only_arms)
        if args.svd_out and not only_arms:
            with open(args.svd_out, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")
        print(json.dumps(out))
        return
    if args.qrcp:
        only_arms = [c for c in args.qrcp_arms.split(",") if c]
        out = qrcp(torch, bq, args.calls, args.warmup, [c for c in args.cases.split(",") if c], only_arms)
        if args.qrcp_out and not only_arms:
            with open(args.qrcp_out, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")
        print(json.dumps(out))
        return
    if args.lstsq_rank:
        only_arms = [c for c in args.lstsq_rank_arms.split(",") if c]
        out = lstsq_rank(torch, bq, args.calls, args.warmup, [c for c in args.cases.split(",") if c], only_arms)
        if args.lstsq_rank_out and not only_arms:
            with open(args.lstsq_rank_out, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")
        print(json.dumps(out))
        return
    if args.orth:
        only_arms = [c for c in args.orth_arms.split(",") if c]
        out = orth(torch, bq, args.calls, args.warmup, [c for c in args.cases.split(",") if c], only_arms)
        if args.orth_out and not only_arms:
            with open(args.orth_out, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")
        print(json.dumps(out))
        return
    if args.lstsq_minnorm:
        out = lstsq_minnorm(torch, bq, args.calls, args.warmup, [c for c in args.cases.split(",") if c])
        if args.lstsq_minnorm_out:
            with open(args.lstsq_minnorm_out, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")
        print(json.dumps(out))
        return
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

"""Speed of the fp64 entry (tsqr_mi_qr_f64): median time of blocking calls per case, the sweep count, effective TB/s (24 m n bytes
per sweep: the Gram pass reads A, the apply pass reads A and writes Q), and torch.linalg.qr(float64) on the same GPU for 2^20 x 64.
Prints one JSON line.  Usage: python tools/f64_speed.py [--calls 50] [--warmup 5]"""
import argparse
import json
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


def time_case(torch, bq, a_rm, reorth, calls, warmup):
    m, n = a_rm.shape
    a = a_rm.T.contiguous()                                 # (n, m): column-major m x n
    q = torch.empty_like(a)
    r = torch.empty(n, n, dtype=torch.float64, device="cuda")
    bf = bq.buffer_f64(reorth)
    bf.allocate(m, n)
    for _ in range(warmup):
        assert bq.qr_f64(q, m, r, n, a, m, m, n, bf) == 0, bq.last_error()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        st = bq.qr_f64(q, m, r, n, a, m, m, n, bf)
        ts.append(time.perf_counter() - t0)
        assert st == 0
    ts.sort()
    med = ts[len(ts) // 2]
    sweeps = bq.last_sweeps_f64()
    nsw = sweeps % 100
    eye = torch.eye(n, dtype=torch.float64, device="cuda")
    qm = q.T
    orth = torch.linalg.norm(qm.T @ qm - eye).item()
    return {"m": m, "n": n, "reorth": reorth, "median_ms": med * 1e3, "min_ms": ts[0] * 1e3, "sweeps": sweeps,
            "eff_TBps": 24.0 * m * n * nsw / med / 1e12, "orth_fro": orth}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cases", default="", help="comma-separated case names (default: all)")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch.linalg.qr baseline")
    args = ap.parse_args()
    import torch
    from tsqr_gpu_amd import blockqr as bq
    n = 64
    out = {"tool": "f64_speed", "cases": []}
    gauss = lambda m, seed: torch.randn(m, n, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))
    cases = [("gauss_2p20_r0", lambda: gauss(1 << 20, 1), 0), ("gauss_2p20_r1", lambda: gauss(1 << 20, 1), 1),
             ("cond1e12_2p20_r0", lambda: cond_matrix(torch, 1 << 20, n, 1e12, 2), 0),
             ("gauss_2p16_r0", lambda: gauss(1 << 16, 3), 0), ("gauss_2p23_r0", lambda: gauss(1 << 23, 4), 0)]
    only = [c for c in args.cases.split(",") if c]
    for name, make, reorth in cases:
        if only and name not in only:
            continue
        res = time_case(torch, bq, make(), reorth, args.calls, args.warmup)
        res["case"] = name
        out["cases"].append(res)
        torch.cuda.empty_cache()
    if args.no_torch:
        print(json.dumps(out))
        return
    a = gauss(1 << 20, 1)
    torch.linalg.qr(a)
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        torch.linalg.qr(a)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    out["torch_linalg_qr_f64_2p20x64_ms"] = sorted(ts)[1] * 1e3
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""SHA-256 (first 16 hex digits) of the results of the fp64 entries that take a tensor -- qr_f64_tensor, qr_f64_wide_tensor, lstsq_f64
(3 right-hand sides), svd_f64_tensor with and without U, qrcp_f64_tensor with and without Q, lstsq_rank_f64 and the same with minimum_norm=True
(x, r, jpvt and the rank, a line each; on the same 3 right-hand sides, the default rcond), orth_f64_tensor with passes 1 and 2 (the
matrix as w against the Q of a Gaussian m x 2 n matrix as v) -- at 9211 x 51, 2^20 x 64, 100 x 7 and
65536 x 128, torch.randn with seed m + n generated on the device, handed over row-major ("row") and with column-major strides
("col"), reorth 0 and 1; at 9211 x 51 also the three entries that can run in place, with overwrite_a=True on a clone.  The entries are
bitwise deterministic, so two builds of libtsqr_mi.so that are meant to compute the same thing must print the same table:

  python tools/f64_checksums.py --parent-lib PATH    PATH: another build of libtsqr_mi.so (the parent commit's)

runs the table once with PATH (through TSQR_MI_LIB) and once with the in-tree library, in two fresh processes, prints every line with
== or != and exits 2 when a line differs.  Without --parent-lib it prints the in-tree table alone.  profiles/fp64_qrcp_parent_checksums.md
was printed by this tool."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ((9211, 51), (1 << 20, 64), (100, 7), (65536, 128))


def table():
    import torch
    from tsqr_gpu_amd import blockqr as bq
    sha = lambda t: hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()[:16]
    out = {}
    for m, n in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(m + n)
        a = torch.randn(m, n, dtype=torch.float64, device="cuda", generator=g)
        b = torch.randn(m, 3, dtype=torch.float64, device="cuda", generator=g)
        for reorth in (False, True):
            for name, x in (("row", a), ("col", a.t().contiguous().t())):
                key = "%dx%d r%d %s " % (m, n, reorth, name)
                q, r = bq.qr_f64_wide_tensor(x, reorth=reorth)
                out[key + "qr_wide"] = (sha(q), sha(r), bq.last_sweeps_f64())
                if n <= 64:
                    q, r = bq.qr_f64_tensor(x, reorth=reorth)
                    out[key + "qr"] = (sha(q), sha(r), bq.last_sweeps_f64())
                    xs, r = bq.lstsq_f64(x, b, reorth=reorth)
                    out[key + "lstsq"] = (sha(xs), sha(r), bq.last_sweeps_f64())
                    u, s, vh = bq.svd_f64_tensor(x, reorth=reorth)
                    out[key + "svd1"] = (sha(u), sha(s), sha(vh), bq.last_jacobi_sweeps_f64())
                    out[key + "svd0"] = (sha(bq.svd_f64_tensor(x, reorth=reorth, compute_uv=False)),)
                    q, r, p = bq.qrcp_f64_tensor(x, reorth=reorth)
                    out[key + "qrcp1"] = (sha(q), sha(r), sha(p), bq.last_sweeps_f64())
                    r, p = bq.qrcp_f64_tensor(x, reorth=reorth, compute_q=False)
                    out[key + "qrcp0"] = (sha(r), sha(p))
                    if hasattr(bq.lib(), "tsqr_mi_lstsq_rank_f64"):     # (absent from a --parent-lib older than the entry)
                        xs, r, p, rank = bq.lstsq_rank_f64(x, b, reorth=reorth)
                        out[key + "lstsq_rank x"] = (sha(xs), bq.last_sweeps_f64())
                        out[key + "lstsq_rank r"] = (sha(r),)
                        out[key + "lstsq_rank jpvt"] = (sha(p),)
                        out[key + "lstsq_rank rank"] = (rank,)
                    if hasattr(bq.lib(), "tsqr_mi_lstsq_minnorm_f64"):  # (absent from a --parent-lib older than the entry)
                        xs, r, p, rank = bq.lstsq_rank_f64(x, b, reorth=reorth, minimum_norm=True)
                        out[key + "lstsq_minnorm x"] = (sha(xs), bq.last_sweeps_f64())
                        out[key + "lstsq_minnorm r"] = (sha(r),)
                        out[key + "lstsq_minnorm jpvt"] = (sha(p),)
                        out[key + "lstsq_minnorm rank"] = (rank,)
                    if hasattr(bq.lib(), "tsqr_mi_orth_f64") and m >= 4 * n:   # (absent from a --parent-lib older than the entry)
                        # w = the matrix of the line; v: the Q of another Gaussian matrix of 2 n columns in the same layout
                        gv = torch.Generator(device="cuda").manual_seed(m + 3 * n)
                        vq = bq.qr_f64_wide_tensor(torch.randn(m, 2 * n, dtype=torch.float64, device="cuda", generator=gv), reorth=True)[0]
                        vq = vq if name == "row" else vq.t().contiguous().t()
                        for passes in (1, 2):
                            q, s_, r = bq.orth_f64_tensor(vq, x, passes=passes, reorth=reorth)
                            out[key + "orth p%d" % passes] = (sha(q), sha(s_), sha(r), bq.last_sweeps_f64())
                    if (m, n) == SHAPES[0]:                 # in place, on a clone (it keeps x's strides); the flag: q IS the clone
                        c = x.clone()
                        q, r = bq.qr_f64_tensor(c, reorth=reorth, overwrite_a=True)
                        out[key + "qr overwrite_a"] = (sha(q), sha(r), q is c, bq.last_sweeps_f64())
                        c = x.clone()
                        u, s, vh = bq.svd_f64_tensor(c, reorth=reorth, overwrite_a=True)
                        out[key + "svd1 overwrite_a"] = (sha(u), sha(s), sha(vh), u is c, bq.last_jacobi_sweeps_f64())
                        c = x.clone()
                        q, r, p = bq.qrcp_f64_tensor(c, reorth=reorth, overwrite_a=True)
                        out[key + "qrcp1 overwrite_a"] = (sha(q), sha(r), sha(p), q is c, bq.last_sweeps_f64())
    return out


def table_in_child(lib):
    """the table of a fresh process that loads lib ('' the in-tree library), as lists"""
    env = dict(os.environ)
    env.pop("TSQR_MI_LIB", None)
    if lib:
        env["TSQR_MI_LIB"] = os.path.abspath(lib)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("the run with %s failed (%d): %s" % (lib or "the in-tree library", res.returncode, res.stderr[-2000:]))
    return json.loads([line for line in res.stdout.splitlines() if line.startswith("CHECKSUMS ")][0][10:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="", help="another build of libtsqr_mi.so to compare the in-tree one against")
    ap.add_argument("--child", action="store_true", help="print the table of this process's library as one JSON line (used by the tool itself)")
    args = ap.parse_args()
    if args.child:
        print("CHECKSUMS " + json.dumps(table(), sort_keys=True))
        return 0
    tree = table_in_child("")
    parent = table_in_child(args.parent_lib) if args.parent_lib else None
    for key in sorted(tree):
        mark = "" if parent is None else (" new" if key not in parent else " ==" if parent[key] == tree[key] else " != %s" % (parent[key],))
        print(key, tree[key], mark.strip())
    if parent is None:
        return 0
    # a line the parent library cannot print (an entry it does not have) is marked new and does not count; every line it prints must
    # be there and equal
    equal = all(key in tree and tree[key] == parent[key] for key in parent)
    print("entries:", len(tree), "of the parent:", len(parent), "all of the parent's equal:", equal)
    return 0 if equal else 2


if __name__ == "__main__":
    sys.exit(main())

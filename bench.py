#!/usr/bin/env python3
"""bench.py -- headline benchmark of the tall-skinny QR hot path (BASELINE.json: TSQR GFLOP/s and ||Q^T Q - I||_F,
M = 2^20 x N = 64 per GPU, fp32_tc_cor).

  python bench.py --gpus 1 --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

A bare `python bench.py --gpus N` (N > 1, no launcher in front: WORLD_SIZE unset) starts its own N ranks: before anything touches
the GPU it runs the torch.distributed.run command above as a child process, forwards its output and exits with its status.

A "step" is one factorisation (mtk::qr::qr; C ABI tsqr_mi_qr_f32, or the row-partitioned driver for N > 1) of a synthetic matrix
already resident in HBM.  `value` / `ms_per_step` are the REFERENCE'S PROTOCOL: K BLOCKING calls one after the other on the same
(q, r, a) -- src/test.cu:289-309 -- issued by one C loop (tsqr_mi_qr_f32_loop at loop depth 1: no interpreter time between calls),
W untimed calls in front, taken in steady state.  A plain run does only that: set-up, SETTLE_STEPS untimed blocking calls that carry
the GPU past its start-up clock / power transient, the W + K window, and the JSON line.
--dump-outputs DIR: after the timed window, what its last call handed the caller -- R whole and a fixed sample of Q's rows -- as
DIR/r.npy and DIR/q.npy (float32, row-major; see dump_outputs).  The input is a fixed function of the arguments.
--full adds, in this order before the `value` window: one checked blocking call (accuracy in fp64), then, each with its own roofline
object (apply-pass duration from HIP events over a leg of the same schedule):
  first_window     the same blocking window taken at process start (inside the GPU's clock / power transient after idle)
  stream_same_a    the K calls as a stream on the same A (tsqr_mi_qr_f32_loop, depth 3: chained schedule where it applies)
  stream_rotating  K calls over R >= 3 rotating (A, Q, R) triples through the batch entry (tsqr_mi_qr_f32_batch): no call finds its A
                   in the 256 MiB Infinity Cache left there by an earlier call -- the cache-cold number
  blocking_rotating  the same rotation as blocking calls
and K blocking calls under HIP events (`roofline`); after it, the accuracy of what the `value` window left in Q and R, the device
probe and the CPU baseline.
Weak scaling (default): every rank owns 2^20 rows (N = 8 is BASELINE's C4, 2^23 x 64).  --scaling strong: the GLOBAL matrix is fixed
(2^23 x 64 unless --m says otherwise) and split over the ranks.
--workload selects the BASELINE.json configuration: c2 (default, the headline: 2^20 x 64 fp32_tc_cor U(-1,1)), c3 (2^20 x 128,
--mode fp32_tc_cor | fp32_notc), c5 (latms cond 1e8, 2^20 x 64, Reorthogonalize = true); c4 is `--gpus 8` of c2's per-GPU shape.
Prints ONE JSON line on rank 0; with --full it also holds the accuracy figures and the `roofline` and `cpu_baseline` objects.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def usable_cpus():
    """Host threads the CPU baseline may use: affinity mask, cgroup CPU quota, and at most 16 (the CPU share of a one-GPU
    box on this pool -- os.cpu_count() reports the whole 256-thread host there, and oversubscribing slows OpenMP down)."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except Exception:
        pass
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return max(1, min(n, 16))


CPU_THREADS = usable_cpus()
for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):   # before numpy / the oracle's libgomp load
    os.environ.setdefault(_v, str(CPU_THREADS))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

PEAK_F32_MATRIX_TFLOPS = 157.3     # MI355X fp32 MFMA/vector peak (MI355X_MICROARCH.md, chip-level parameters)
PEAK_HBM_TBS = 8.0                 # HBM3E spec
# calls 10-30 of a process run 5-8 % slow (GPU clock / power settling, profiles/r02_experiment_log.md; about 20 ms of streaming
# removes it): a plain run issues these untimed blocking calls before its W + K window so that `value` stays a steady-state figure
SETTLE_STEPS = 128
DUMP_Q_BYTES = 32 << 20            # --dump-outputs: Q is sampled by rows down to this size (float32)


def f_qr(m, n):
    """Algorithmic flops of geqrf + explicit thin Q: 4MN^2 - 4/3 N^3 (SURVEY.md 8d / BASELINE.md section 2)."""
    return 4.0 * m * n * n - 4.0 / 3.0 * n ** 3


def f_r(m, n):
    return 2.0 * m * n * n - 2.0 / 3.0 * n ** 3


def synth_block(m_local, n, m_global, row0, seed, device):
    """U(-1,1) entries keyed by (seed, global row, column) with a splitmix64-style integer hash, so that 1/2/4/8-GPU
    runs see the identical global matrix.  Returned as an (n, m_local) tensor = column-major m_local x n."""
    rows = torch.arange(row0, row0 + m_local, device=device, dtype=torch.int64)
    out = torch.empty(n, m_local, device=device, dtype=torch.float32)
    for j in range(n):
        x = rows + (j * m_global + seed * 1000003 + 0x632BE5AB)     # int64 arithmetic wraps; only the bit mixing matters
        x = (x ^ (x >> 30)) * 0x1CE4E5B9
        x = (x ^ (x >> 27)) * 0x133111EB
        x = x ^ (x >> 31)
        u = (x & ((1 << 24) - 1)).to(torch.float32) * (1.0 / (1 << 24))
        out[j] = u * 2.0 - 1.0
    return out


def device_probe():
    """What this box is and what it sustains right now, for reading `value` across boxes (round 4: the same library ran the blocking headline
    call at 0.163 ms on one box and at 0.196-0.198 ms on five others).  Device properties, plus two library-independent probes taken AFTER all
    timed windows: a torch bf16 GEMM (8192^3, hipBLASLt) and a torch device-to-device copy of 1 GiB -- plumbing used as a yardstick, not
    part of the path."""
    import torch
    p = torch.cuda.get_device_properties(0)
    dev = {"name": p.name, "arch": getattr(p, "gcnArchName", ""), "compute_units": p.multi_processor_count,
           "total_memory_gib": round(p.total_memory / 2.0 ** 30, 1)}
    for k in ("clock_rate", "memory_clock_rate", "L2_cache_size"):
        if hasattr(p, k):
            dev[k] = getattr(p, k)
    try:
        x = torch.randn(8192, 8192, device="cuda", dtype=torch.bfloat16)
        y = torch.randn(8192, 8192, device="cuda", dtype=torch.bfloat16)
        src = torch.empty(1 << 28, device="cuda", dtype=torch.float32)
        dst = torch.empty_like(src)
        for _ in range(3):
            torch.matmul(x, y); dst.copy_(src)
        torch.cuda.synchronize()
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        for _ in range(10):
            torch.matmul(x, y)
        e1.record()
        for _ in range(10):
            dst.copy_(src)
        e2.record()
        torch.cuda.synchronize()
        dev["probe_bf16_gemm_8192_tflops"] = round(10 * 2 * 8192.0 ** 3 / (e0.elapsed_time(e1) * 1e-3) / 1e12, 1)
        dev["probe_copy_1gib_gbs"] = round(10 * 2 * 2.0 ** 30 / (e1.elapsed_time(e2) * 1e-3) / 1e9, 1)
    except Exception as e:                                           # (a probe must never cost the line)
        dev["probe_error"] = str(e)[:200]
    return dev


def cpu_baseline(n, mode_name, sample_rows):
    """The reported CPU baseline (north star): host LAPACK sgeqrf + sorgqr (explicit thin Q, F_QR flops -- like for like) on the box's
    host cores, on a bounded sample of the same workload (sample_rows x n, U(-1,1)); sgeqrf alone (F_R) and the CPU oracle
    (restatement of the reference algorithm, oracle/ref_tsqr.c, OpenMP over leaves) are nested extras."""
    from oracle import ref_oracle as ro
    a = ro.uniform_matrix(sample_rows, n, seed=0)
    cores = int(os.environ.get("OMP_NUM_THREADS", CPU_THREADS))
    out = None
    try:
        from scipy.linalg import lapack
        af = np.asfortranarray(a)
        lapack.sgeqrf(np.asfortranarray(a[:4096]))
        t = time.time(); qr_, tau, _, info = lapack.sgeqrf(af); t_geqrf = time.time() - t
        t = time.time(); qq, _, info = lapack.sorgqr(qr_[:, :n], tau); t_orgqr = time.time() - t
        out = {"value": f_qr(sample_rows, n) / (t_geqrf + t_orgqr) / 1e9, "unit": "GFLOP/s", "cores": cores, "kind": "lapack",
               "sample": "scipy.linalg.lapack (OpenBLAS) sgeqrf + sorgqr on %d x %d U(-1,1), %.2f s on %d threads; F_QR = 4MN^2 - 4/3 N^3" % (
                   sample_rows, n, t_geqrf + t_orgqr, cores),
               "sgeqrf_only_gflops": f_r(sample_rows, n) / t_geqrf / 1e9, "orth_fro": ro.orthogonality_fro(qq)}
    except Exception as e:  # no LAPACK on the box: the oracle port becomes the baseline
        out = None
        lapack_error = str(e)
    md = ro.FP32_NOTC if mode_name == "fp32_notc" else ro.FP32_TC_COR   # the oracle models the two north-star modes
    ro.qr(a[:4096], md, False)
    t = time.time()
    st, q, r = ro.qr(a, md, False)
    dt = time.time() - t
    port = {"value": f_qr(sample_rows, n) / dt / 1e9, "unit": "GFLOP/s", "cores": cores, "kind": "port",
            "sample": "oracle/ref_tsqr.c (%s, reference algorithm, OpenMP) on %d x %d U(-1,1), %.2f s" % (mode_name, sample_rows, n, dt),
            "orth_fro": ro.orthogonality_fro(q), "residual": ro.residual(a, q, r)}
    if out is None:
        port["lapack_error"] = lapack_error
        return port
    out["oracle_port"] = port
    return out


def pmc_traffic(kernel_class, m, n, mode):
    """HBM bytes per launch of the dominant kernel.  NOT measured in this run: replayed from the newest committed rocprofv3 PMC
    summary (profiles/rNN_pmc_hbm_traffic.json: FETCH_SIZE x2 for gfx950, WRITE_SIZE exact, separate --pmc passes), valid only
    for the workload those passes were taken on (2^20 x 64, fp32_tc_cor).  Returns (bytes or None, source label)."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_hbm_traffic.json")))
    if not files or m != 1 << 20 or n != 64 or mode != "fp32_tc_cor":
        return None, None
    try:
        data = json.load(open(files[-1]))
        for k in data["kernels"].values():
            if k.get("class") == kernel_class:
                return k["hbm_bytes"], "static: %s (rocprofv3 --pmc passes of an earlier run, not this one)" % os.path.relpath(files[-1], ROOT)
    except Exception:
        pass
    return None, None


def dump_outputs(dirname, q_t, r_t, m, n):
    """What the last timed call handed its caller, for comparing two builds output for output: DIR/r.npy = R (n x n) whole and
    DIR/q.npy = Q (m x n) -- all rows when they fit in DUMP_Q_BYTES, otherwise the rows numpy.random.default_rng(0).choice(m, k,
    replace=False) picks, ascending, k = DUMP_Q_BYTES / (4 n).  Both float32, row-major.  q_t / r_t are the engine's column-major
    (n, ld) / (n, n) tensors; with several ranks, rank 0's row block."""
    os.makedirs(dirname, exist_ok=True)
    k = DUMP_Q_BYTES // (4 * n)
    if k < m:
        idx = np.sort(np.random.default_rng(0).choice(m, k, replace=False))
        q_t = q_t[:, torch.from_numpy(idx).to(q_t.device)]
    np.save(os.path.join(dirname, "q.npy"), np.ascontiguousarray(q_t.float().cpu().numpy().T))
    np.save(os.path.join(dirname, "r.npy"), np.ascontiguousarray(r_t.float().cpu().numpy().T))


WORKLOADS = {
    # BASELINE.json configs[1], [2], [4] ([3] = `--gpus 8` of c2's per-GPU shape; [0] is the CPU-runnable LAPACK case, tests/test_gpu_configs.py)
    "c2": dict(m=1 << 20, n=64, mode="fp32_tc_cor", reorth=0, input="uniform", cpu_rows=1 << 20),
    "c3": dict(m=1 << 20, n=128, mode="fp32_tc_cor", reorth=0, input="uniform", cpu_rows=1 << 19),
    "c5": dict(m=1 << 20, n=64, mode="fp32_tc_cor", reorth=1, input="latms_cond1e8", cpu_rows=1 << 20),
    # not a BASELINE configuration: c2's shape through the half-typed modes (io type half, reference src/tsqr.hpp:38-39)
    "c2h": dict(m=1 << 20, n=64, mode="fp16_tc_nocor", reorth=0, input="uniform", cpu_rows=1 << 20),
}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=32)       # reference protocol: 1 warm-up + C = 16 calls (src/test.cu:289-309)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--workload", default="c2", choices=sorted(WORKLOADS), help="BASELINE.json configuration (see the module docstring)")
    ap.add_argument("--m", type=int, default=None, help="rows per GPU (default: the workload's)")
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--mode", default=None, choices=["fp32_tc_cor", "fp32_notc", "fp32_tc_nocor", "fp16_notc", "fp16_tc_nocor"])
    ap.add_argument("--reorth", type=int, default=None)
    ap.add_argument("--full", action="store_true",
                    help="everything beside `value`: the checked call and the accuracy figures, the extra windows and their roofline legs, the "
                         "device probe and the CPU baseline (the options below that shape those are --full options)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write R and a fixed row sample of Q from the last timed call as DIR/r.npy, DIR/q.npy (float32)")
    ap.add_argument("--cpu-sample-rows", type=int, default=None)   # c2: the whole headline matrix, ~15 s of CPU work on 16 host threads
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-first-window", action="store_true", help="skip the extra timing window at process start (profiling runs)")
    ap.add_argument("--gram-waves", type=int, default=0)
    ap.add_argument("--apply-waves", type=int, default=0)
    ap.add_argument("--policy", type=int, default=0)
    ap.add_argument("--force-dist", action="store_true", help="use the row-partitioned driver even on one GPU")
    ap.add_argument("--dist-comm", default="auto", choices=["auto", "rccl", "callbacks"],
                    help="transport of the row-partitioned driver's two exchanges: raw RCCL communicator (C calls ncclAllReduce itself, "
                         "no Python between kernels) or torch.distributed callbacks; auto = rccl when every rank can create it")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="process-group backend; gloo only to rehearse the multi-rank logic with several ranks on ONE GPU (or none)")
    ap.add_argument("--rehearse", action="store_true",
                    help="NO GPU: the per-rank executor is the numpy test double of tests/dist_double.py.  Exercises the launcher, the "
                         "collectives and the JSON plumbing on CPU; the numbers say nothing about the product and are labelled so")
    ap.add_argument("--ld-pad", type=int, default=0, help="leading dimension = m + pad (experiments on DRAM channel mapping)")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="weak: --m rows PER GPU (default 2^20; N = 8 is BASELINE's C4).  strong: --m is the GLOBAL row count (default 2^23, "
                         "SURVEY.md 8e) and every rank owns m / N rows")
    ap.add_argument("--rotate", type=int, default=4, help="(A, Q, R) triples of the rotating-buffer windows (>= 3; 0 switches those windows off)")
    ap.add_argument("--only-value", action="store_true", help="skip the extra windows (profiling runs): checked step, roofline leg, `value` window")
    args = ap.parse_args(argv)
    w = WORKLOADS[args.workload]
    if args.scaling == "strong":
        m_glob = args.m if args.m is not None else 1 << 23
        assert m_glob % args.gpus == 0, "--scaling strong: the global row count must divide by --gpus"
        args.m = m_glob // args.gpus
    for k in ("m", "n", "mode", "reorth"):
        if getattr(args, k) is None:
            setattr(args, k, w[k])
    if args.cpu_sample_rows is None:
        args.cpu_sample_rows = min(w["cpu_rows"], args.m)
    args.input = w["input"]
    return args


def spawn_own_ranks(argv, gpus):
    """`python bench.py --gpus N` without a launcher: run N ranks of this file under torch.distributed.run as ONE child process
    (this process has not touched the GPU and never will), forward its output, return its exit status."""
    import socket
    import subprocess
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    # the ranks' own arguments travel in the environment: the launcher's argument parser chokes on options of the script that
    # happen to abbreviate one of its own (--m is "ambiguous" to it even behind the script name)
    env = dict(os.environ, TSQR_BENCH_ARGV=json.dumps(list(argv)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)]
    return subprocess.call(cmd, env=env)


def make_input(args, m, n, m_glob, rank, dev, seed=0):
    """seed 0: the workload's matrix; seeds 1, 2, ...: further matrices of the same kind (the rotating-buffer windows)"""
    if args.input == "uniform" or args.rehearse:
        return synth_block(m, n, m_glob, rank * m, seed, dev)
    # C5: latms-style A = U diag(s) V^T with the reference's singular-value draw (src/test_cond.cu:31-50), cond 1e8, fixed seed
    from tsqr_gpu_amd import harness
    return harness.get_rand_matrix_with_cond_number(m, n, 1e8, seed=5 + seed, device=dev)


def roofline_of(prof, steps, m, n, io_half, world):
    """roofline object of the dominant kernel class of a profiled leg (HIP events on the engine's stream)"""
    if not prof or not any(v[1] for v in prof.values()):
        return None
    dom = max(prof, key=lambda k: prof[k][0])
    dom_ms, dom_launches = prof[dom]
    per_launch_s = dom_ms * 1e-3 / max(dom_launches, 1)
    esz = 2.0 if io_half else 4.0                            # bytes per element of A and Q
    if dom == "apply":                                       # Q = A * inverse(R): read A, write Q
        bound, alg_bytes, alg_flops = "hbm", 2 * esz * m * n, 2.0 * m * n * n
    elif dom == "gram":                                      # G = A^T A: read A once
        bound, alg_bytes, alg_flops = "hbm", esz * m * n, 2.0 * m * n * n
    else:                                                    # Householder fold: R factor of the local block
        bound, alg_bytes, alg_flops = "mfma", 4.0 * m * n, f_r(m, n)
    if bound == "hbm":
        ach, peak, unit = alg_bytes / per_launch_s / 1e9, PEAK_HBM_TBS * 1e3, "GB/s"
    else:
        ach, peak, unit = alg_flops / per_launch_s / 1e12, PEAK_F32_MATRIX_TFLOPS, "TFLOP/s"
    return {"kernel": dom, "bound": bound, "achieved": ach, "peak": peak, "unit": unit, "frac": ach / peak,
            "avg_launch_us": per_launch_s * 1e6, "launches": dom_launches,
            "algorithmic_flops_per_launch": alg_flops, "algorithmic_bytes_per_launch": alg_bytes,
            "kernel_ms_per_step": {k: v[0] / steps for k, v in prof.items() if v[1]}}


def main():
    argv = sys.argv[1:]
    if not argv and os.environ.get("TSQR_BENCH_ARGV"):       # a rank started by spawn_own_ranks
        argv = json.loads(os.environ["TSQR_BENCH_ARGV"])
    args = parse_args(argv)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:    # bare multi-GPU invocation: become the launcher, before any GPU call
        sys.exit(spawn_own_ranks(argv, args.gpus))

    from tsqr_gpu_amd import blockqr as bq
    if not args.rehearse:
        bq.lib()                                            # fail loudly if the HIP library is missing
        bq.lib().tsqr_mi_set_tuning2(args.gram_waves, args.apply_waves)
        bq.set_policy(args.policy)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == args.gpus, "WORLD_SIZE (%d) != --gpus (%d)" % (world, args.gpus)
    gpu = not args.rehearse
    if gpu:
        assert torch.cuda.is_available(), "bench.py needs a GPU (--rehearse runs the launcher/collective plumbing on a CPU double)"
        if args.backend == "gloo":                           # rehearsal: ranks may share a device
            local_rank = local_rank % torch.cuda.device_count()
        torch.cuda.set_device(local_rank)
    else:
        assert args.backend == "gloo", "--rehearse runs on CPU: use --backend gloo"
    if world > 1 or (args.force_dist and "RANK" in os.environ):
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group("gloo")
    dev = torch.device("cuda", local_rank) if gpu else torch.device("cpu")
    if world > 1:                                           # communicator set-up (lazy in RCCL) must never land in the timed region
        warm = torch.zeros(2560, dtype=torch.float64, device=dev)
        dist.all_reduce(warm)
        if gpu:
            torch.cuda.synchronize()
    m, n = args.m, args.n
    m_glob = m * world
    assert world == 1 or n <= 64, "the row-partitioned path factors one 64-wide panel (c3 is a one-GPU workload)"
    assert world == 1 or args.input == "uniform", "c5 is a one-GPU workload"
    mode = bq.compute_mode[args.mode]

    ld = m + args.ld_pad
    io_half = (not args.rehearse) and mode in bq.FP16_MODES   # the half-typed modes: fp16 in, fp16 out (one-GPU workloads)
    assert not io_half or (world == 1 and not args.force_dist), "the fp16 I/O modes are single-GPU entry points"
    io_dt = torch.float16 if io_half else torch.float32
    single = world == 1 and not args.force_dist and not args.rehearse

    def new_triple(seed):
        a = make_input(args, m, n, m_glob, rank, dev, seed).to(io_dt)
        if args.ld_pad:
            a_pad = torch.zeros(n, ld, dtype=io_dt, device=dev)
            a_pad[:, :m] = a
            a = a_pad[:, :m]
        return a, torch.empty(n, ld, dtype=io_dt, device=dev)[:, :m], torch.zeros(n, n, dtype=io_dt, device=dev)

    d_a, d_q, d_r = new_triple(0)
    a_keep = d_a.clone() if n > 64 and args.full else None   # n > 64: the engine may overwrite A (it does not on the one-panel path)
    eng = None
    if args.rehearse:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from dist_double import NumpyRowBackend
        from tsqr_gpu_amd import dist as tdist
        eng = tdist.RowPartitionedQR(mode, m, n, backend=NumpyRowBackend(n, tdist.TorchCollectives()))

        def run_steps(k):
            for _ in range(k):
                assert eng.qr(d_q, ld, d_r, d_a, ld, reorthogonalize=bool(args.reorth)) == 0
    elif single:
        bf = bq.buffer(mode, bool(args.reorth), device=dev)
        bf.allocate(m, n)
        loop = bq.bind_loop(d_q, ld, d_r, n, d_a, ld, m, n, bf)  # K calls issued by ONE C loop (tsqr_mi_qr_f32_loop): what a C++ caller's
        # loop costs (the reference's speed protocol is such a loop, src/test.cu:299-309), no interpreter time between calls.  The loop
        # depth (bq.set_loop_depth) selects the protocol: 1 = blocking calls, 3 = a stream of calls (chained schedule where it applies).

        def run_steps(k):
            st = loop(k)
            assert st == 0, st
    else:
        from tsqr_gpu_amd import dist as tdist
        eng = tdist.RowPartitionedQR(mode, m, n, comm=args.dist_comm)    # K steps = one C loop; RCCL called from C on this stream
        dloop = eng.bind_loop(d_q, ld, d_r, d_a, ld, reorthogonalize=bool(args.reorth))

        def run_steps(k):
            st = dloop(k)
            assert st == 0, st                              # (complete on return, like the single-GPU loop)

    # rotating buffers (one GPU, fp32 I/O): R triples more than an Infinity Cache apart, K calls = one call of the batch entry over the
    # cyclic sequence of triples -- every call runs on an A the cache has not seen since R - 1 other matrices went through it
    rot = None
    if args.full and single and not io_half and args.rotate >= 3 and not args.only_value:
        triples = [(d_a, d_q, d_r)] + [new_triple(s) for s in range(1, args.rotate)]
        binds = {}

        def run_rot(k):
            if k not in binds:
                seq = [triples[i % len(triples)] for i in range(k)]
                binds[k] = bq.bind_batch([t[1] for t in seq], ld, [t[2] for t in seq], n, [t[0] for t in seq], ld, m, n, bf)
            st, _ = binds[k]()
            assert st == 0, st
        rot = run_rot

    def barrier():
        if world > 1:
            dist.barrier()
        if gpu:
            torch.cuda.synchronize()

    def set_depth(d):
        if gpu:
            bq.set_loop_depth(d)                            # (every rank alike: the loop depth is a per-process setting)

    def timed_window(steps_fn, depth):
        """The contract's measurement: W untimed warm-up steps, then exactly K steps between barrier + synchronize, MAX over ranks."""
        set_depth(depth)
        try:
            steps_fn(args.warmup)
            barrier()
            t0 = time.perf_counter()
            steps_fn(args.steps)
            barrier()
            dt = time.perf_counter() - t0
        finally:
            set_depth(3)
        if world > 1:
            tt = torch.tensor([dt], device=dev, dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            dt = float(tt.item())
        return dt / args.steps * 1e3

    def profiled_leg(steps_fn, depth):
        """K steps of the same schedule under HIP events on the engine's stream: per-kernel-class durations (the roofline leg)"""
        if not gpu:
            return None
        set_depth(depth)
        bq.profile_enable(True)
        try:
            steps_fn(args.steps)
            barrier()
            return bq.profile_read()
        finally:
            bq.profile_enable(False)
            set_depth(3)

    def accuracy(q_t, r_t, a_t):
        """||Q^T Q - I||_F and ||A - QR||_F / ||A||_F in fp64 (global Q: all-reduce of Q_p^T Q_p)"""
        q64 = q_t.double()
        gram = q64 @ q64.T
        r64 = r_t.double().T.contiguous()
        a64 = a_t.double()
        res_num = ((r64.T @ q64) - a64).pow(2).sum().reshape(1)
        res_den = a64.pow(2).sum().reshape(1)
        if world > 1:
            dist.all_reduce(gram); dist.all_reduce(res_num); dist.all_reduce(res_den)
        return (float((gram - torch.eye(n, device=dev, dtype=torch.float64)).norm().item()), float(torch.sqrt(res_num / res_den).item()))

    flops = f_qr(m_glob, n)

    def window_obj(ms, prof, note):
        o = {"ms_per_step": ms, "value": flops / (ms * 1e-3) / 1e9, "unit": "GFLOP/s", "note": note}
        rf = roofline_of(prof, args.steps, m, n, io_half, world)
        if rf is not None:
            o["roofline"] = rf
        return o

    if args.full:
        # 1. one blocking step, checked: accuracy of the factorisation evaluated in fp64, A untouched
        set_depth(1)
        run_steps(1)
        set_depth(3)
        barrier()
        orth_first, res_first = accuracy(d_q, d_r, a_keep if a_keep is not None else d_a)
        a_untouched = True if a_keep is None else bool(torch.equal(a_keep, d_a))
        if not a_untouched:                                  # panel path for n > 64 (ill-conditioned input): every step needs a fresh A
            raise SystemExit("bench.py: the engine overwrote A on this workload; timing repeated calls on it would not measure the workload")
    elif gpu:
        # a plain run: carry the GPU past its start-up transient, where --full runs the windows below
        set_depth(1)
        run_steps(SETTLE_STEPS)
        set_depth(3)
        barrier()

    extras = {}
    if args.full and not args.only_value and not args.rehearse:
        # 2. the blocking window at process start: the first ~30 calls of a process run 5-8 % slower than all later ones (GPU clock /
        #    power settling after idle: profiles/r02_experiment_log.md) -- the position round 2's `value` was taken at
        if not args.no_first_window:
            ms = timed_window(run_steps, 1)
            extras["first_window"] = window_obj(ms, None, "the blocking-call window (as `value`) taken at process start, inside the GPU's clock / power transient after idle")
        # 3. the K calls as a stream on the same A (loop entry, depth 3), and its own profiled leg
        ms = timed_window(run_steps, 3)
        extras["stream_same_a"] = window_obj(ms, profiled_leg(run_steps, 3),
                                             "K calls of one C loop (tsqr_mi_qr_f32_loop / _dist_*_loop) issued as a stream: call i + 1 submitted before call i is finished; "
                                             "full 64-column blocks of <= 2^20 rows: the R-factor chain of call i inside the Gram launch of call i + 1 (chained schedule).  "
                                             "Same A every call (the reference's speed protocol): a 256 MiB A is largely Infinity-Cache resident between passes AND calls")
        if rot is not None:
            # 4. rotating triples: the batch entry (chained where the library takes it), then the same rotation as blocking calls
            ms = timed_window(rot, 3)
            extras["stream_rotating"] = window_obj(ms, profiled_leg(rot, 3),
                                                   "K calls over %d rotating (A, Q, R) triples (%.0f MiB each) through tsqr_mi_qr_f32_batch, loop depth 3: no call finds its A in the "
                                                   "256 MiB Infinity Cache from an earlier CALL (cache-cold across calls)" % (args.rotate, (2.0 * m * ld + n * n) * 4 / 2 ** 20))
            ms = timed_window(rot, 2)
            extras["two_in_flight_rotating"] = window_obj(ms, None, "the same rotation, two calls in flight in stream order (tsqr_mi_qr_f32_batch at loop depth 2)")
            ms = timed_window(rot, 1)
            extras["blocking_rotating"] = window_obj(ms, profiled_leg(rot, 1), "the same rotation as blocking calls (tsqr_mi_qr_f32_batch at loop depth 1)")
            o2, r2 = accuracy(triples[-1][1], triples[-1][2], triples[-1][0])
            extras["stream_rotating"]["orth_fro_last_triple"] = o2
            extras["stream_rotating"]["residual_last_triple"] = r2

    # 5. the roofline leg of `value`: K blocking calls under HIP events
    prof = profiled_leg(run_steps, 1) if args.full else None
    # 6. the contract's window: W + K BLOCKING calls (the reference's protocol, src/test.cu:289-309)
    ms_per_step = timed_window(run_steps, 1)
    gflops = flops / (ms_per_step * 1e-3) / 1e9
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, d_q, d_r, m, n)
    if args.full:
        # accuracy of what the timed schedule left in Q and R (the last call of the window)
        orth_fro, residual = accuracy(d_q, d_r, a_keep if a_keep is not None else d_a)

    if rank == 0:
        engine_name = "numpy-double (rehearsal)" if args.rehearse else bq.ENGINE_NAMES.get(eng.last_engine if eng is not None else bq.last_engine(), "?")
        roofline = roofline_of(prof, args.steps, m, n, io_half, world)
        if roofline is not None:
            traffic, traffic_source = pmc_traffic(roofline["kernel"], m, n, args.mode) if args.workload == "c2" and args.scaling == "weak" else (None, None)
            roofline.update({"traffic": traffic, "traffic_source": traffic_source,
                             "note": "blocking calls on the SAME A (the reference's own protocol, src/test.cu:299-309): a 256 MiB A stays largely resident in the 256 MiB "
                                     "Infinity Cache between the two passes and between steps, so this HBM fraction is fabric-side (FETCH_SIZE counts those hits as "
                                     "memory-side requests); stream_rotating / blocking_rotating carry the cache-cold rooflines",
                             "r_factor_engine": engine_name,
                             "whole_path": {"tflops": gflops / 1e3 / world, "peak_tflops_f32_matrix": PEAK_F32_MATRIX_TFLOPS,
                                            "frac_f32_matrix_peak": gflops / 1e3 / world / PEAK_F32_MATRIX_TFLOPS,
                                            "algorithmic_gbs": 4.0 * (2 * m * n + n * n) / (ms_per_step * 1e-3) / 1e9,
                                            "frac_hbm_peak": 4.0 * (2 * m * n + n * n) / (ms_per_step * 1e-3) / 1e12 / PEAK_HBM_TBS}})
        inp = "U(-1,1)" if args.input == "uniform" else "latms cond 1e8 (src/test_cond.cu:31-50 spectrum, seed 5)"
        exchange = None
        if eng is not None:                                  # what the ranks exchange per call
            exchange = ("r_allgather: all-gather of the n x n local R factors (%d B per rank), Householder engine" % (4 * min(n, 64) ** 2) if args.policy == 1 else
                        "gram_allreduce: all-reduce of the Gram tiles + row count (%d doubles = %d B), Gram engines; the Householder engine's "
                        "r_allgather only as the ladder's last resort" % (10 * 256 + 1, 8 * (10 * 256 + 1)))
        out = {"metric": "tsqr_gflops", "value": gflops, "unit": "GFLOP/s", "n_gpus": world, "steps": args.steps,
               "warmup": args.warmup, "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": args.scaling,
               "vs_baseline": None, "dtype": ("f16 in / out, f32 accumulation" if io_half else "f32"),
               "data": "synthetic",
               "config": {"workload": "%s: M=%s x N=%d per GPU, %s, reorth=%d, %s; global %d x %d (%s scaling); F_QR=4MN^2-4/3N^3; R-factor engine: %s" % (
                   args.workload, ("2^%d" % int(np.log2(m))) if m & (m - 1) == 0 else str(m), n, args.mode, args.reorth, inp, m_glob, n, args.scaling, engine_name),
                   "engine": engine_name, "m_per_gpu": m, "n": n, "mode": args.mode, "reorthogonalize": bool(args.reorth),
                   "parallelism": "row-partitioned x%d" % world,
                   "dist_transport": (eng.transport if eng is not None else None), "dist_exchange": exchange},
               "call_protocol": "value / ms_per_step: K BLOCKING calls on the same (q, r, a), one after the other (reference src/test.cu:289-309), issued by one C loop "
                                "(loop depth 1), W untimed calls in front; taken in steady state (window_order) -- with --full, first_window is the same window at process start",
               "full": args.full}
        if args.full:
            out.update({"orth_fro": orth_fro, "orth_ref_metric": orth_fro / np.sqrt(n), "residual": residual,
                        "orth_fro_checked_step": orth_first, "residual_checked_step": res_first,
                        "window_order": "1 checked blocking step; first_window (W + K blocking); stream_same_a (W + K, then K under HIP events); stream_rotating, "
                                        "two_in_flight_rotating, blocking_rotating (W + K each; K under events for the first and the last); K blocking calls under HIP "
                                        "events (`roofline`); then the W + K blocking window `value` is taken from; orth_fro / residual are evaluated on the Q and R "
                                        "that window left",
                        "roofline": roofline})
            out.update(extras)
        else:
            out["window_order"] = ("%d untimed blocking calls (past the start-up transient); then the W + K blocking window `value` is taken from" % SETTLE_STEPS
                                   if gpu else "the W + K window `value` is taken from")
        if args.rehearse:
            out["rehearsal"] = True
            out["data"] = "synthetic (CPU rehearsal with the numpy test double: NOT a measurement of the product)"
        if args.full and not args.rehearse:
            out["device"] = device_probe()
        if args.full and world == 1 and not args.no_cpu_baseline and not args.rehearse and not io_half:
            out["cpu_baseline"] = cpu_baseline(n, args.mode, args.cpu_sample_rows)
        print(json.dumps(out))
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

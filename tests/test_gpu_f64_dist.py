"""The row-partitioned fp64 entries (tsqr_mi_qr_f64_dist_cb / _fn, dist.RowPartitionedQRF64) on ONE GPU: one rank in process against
tsqr_mi_qr_f64_wide bit for bit; two and four processes over gloo (the scaffolding of tests/test_gpu_dist.py, ONE spawn per world size:
start-up dominates) for the properties of the header on the stacked matrix, equal verdicts on every rank, the rule's use of the GLOBAL
row count, the shifted path and a NaN on one rank only; and one rank over a raw RCCL communicator.  (RCCL refuses two ranks on one
device: the multi-rank all-reduce of the raw transport never runs here.)"""
import ctypes
import os

import numpy as np
import pytest

from tests.test_gpu_dist import _run as _spawn_ranks

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53


# ---- matrices: every rank (and the parent) builds the same global matrix from the case's description ------------------------------------
def _matrix(case):
    from tests import pass_refs_f64 as p64
    m, n, seed = sum(case["heights"]), case["n"], case["seed"]
    rng = np.random.default_rng(seed)
    if case["kind"] == "ladder":
        return p64.ladder_matrix(m, n, case["s_target"], seed)[0]
    if case["kind"] == "cond":
        u, _ = np.linalg.qr(rng.standard_normal((m, n)))
        v, _ = np.linalg.qr(rng.standard_normal((n, n)))
        return (u * np.logspace(0.0, -np.log10(case["cond"]), n)) @ v.T
    a = rng.standard_normal((m, n))
    if case["kind"] == "nan":
        a[case["heights"][0] + 5, n // 2] = np.nan           # (in rank 1's block)
    return a


def _case(heights, n, reorth=0, kind="gauss", seed=0, single=False, **more):
    return dict(heights=tuple(heights), n=n, reorth=reorth, kind=kind, seed=seed or 1000 + n + len(heights), single=single, **more)


def _bands(n, reorth):
    return (1e-12 if reorth else 1e-11) * max(1.0, n / 64.0), 1e-13


# ---- one rank, in process ------------------------------------------------------------------------------------------------------------------
def _nelem(n):
    nt, nb = (min(n, 64) + 15) // 16, (n + 63) // 64
    return nt * (nt + 1) // 2 * 256 if n <= 64 else nb * (nb + 1) // 2 * 4096


@pytest.fixture(scope="module")
def one_rank_refs(bq):
    """tsqr_mi_qr_f64_wide on every shape of the one-rank tests, computed once: (a, {reorth: (q, r, sweeps)}), all on the GPU"""
    import torch
    refs = {}
    for m, n in [(777, 1), (4097, 33), (5000, 64), (3000, 65), (2048, 200), (1 << 16, 64), (8192, 130)]:
        g = torch.Generator(device="cuda").manual_seed(m + n)
        a = torch.randn(n, m, dtype=torch.float64, device="cuda", generator=g)      # column-major m x n
        per = {}
        for reorth in (0, 1):
            q = torch.empty_like(a); r = torch.zeros(n, n, dtype=torch.float64, device="cuda")
            bf = bq.buffer_f64_wide(reorth)
            bf.allocate(m, n)
            assert bq.qr_f64_wide(q, m, r, n, a, m, m, n, bf) == 0, bq.last_error()
            torch.cuda.synchronize()
            per[reorth] = (q, r, bq.last_sweeps_f64())
        refs[(m, n)] = (a, per)
    return refs


def _same_bits(x, y):
    import torch
    return torch.equal(x.view(torch.int64), y.view(torch.int64))


@pytest.mark.parametrize("m,n", [(777, 1), (4097, 33), (5000, 64), (3000, 65), (2048, 200)])
def test_one_rank_callback_is_the_plain_entry_bit_for_bit(bq, one_rank_refs, m, n):
    """a callback that leaves the buffer alone (the sum over one rank) and notes its count: Q, R and the sweep count of
    tsqr_mi_qr_f64_wide, one exchange of nelem + 1 doubles per sweep; both reorth values, out of place and in place (q == a)"""
    import torch
    a, per = one_rank_refs[(m, n)]
    L = bq.lib()
    counts = []
    cb = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p)(
        lambda user, buf, count, stream: counts.append(count) or 0)
    wq = torch.empty(L.tsqr_mi_working_q_size_f64_dist(m, n, 1), dtype=torch.float64, device="cuda")
    wr = torch.empty(L.tsqr_mi_working_r_size_f64_dist(m, n, 1), dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for reorth in (0, 1):
        q_ref, r_ref, sweeps_ref = per[reorth]
        for in_place in ((False, True) if reorth == 0 else (False,)):
            src = a.clone()
            q = src if in_place else torch.full_like(a, float("nan"))
            r = torch.full((n, n), float("nan"), dtype=torch.float64, device="cuda")
            del counts[:]
            rc = L.tsqr_mi_qr_f64_dist_cb(reorth, q.data_ptr(), m, r.data_ptr(), n, src.data_ptr(), m, m, n, wq.data_ptr(), wr.data_ptr(),
                                          cb, None, 1, st)
            torch.cuda.synchronize()
            assert rc == 0, (rc, bq.last_error())
            sweeps = L.tsqr_mi_last_sweeps_f64()
            assert sweeps == sweeps_ref, (sweeps, sweeps_ref)
            assert counts == [_nelem(n) + 1] * (sweeps % 100), (counts, sweeps)
            assert _same_bits(q, q_ref) and _same_bits(r, r_ref), (m, n, reorth, in_place)
            assert in_place or _same_bits(src, a)


@pytest.mark.parametrize("m,n", [(1 << 16, 64), (8192, 130)])
def test_one_rank_raw_rccl_is_the_plain_entry_bit_for_bit(bq, one_rank_refs, m, n):
    """tsqr_mi_qr_f64_dist_fn on a one-rank RCCL communicator created through ctypes (as tests/test_gpu_configs.py does): the
    ncclAllReduce handed to the C side comes from the same library handle as the communicator"""
    import torch
    try:
        rccl = ctypes.CDLL("librccl.so")
    except OSError:
        pytest.skip("librccl.so not loadable by name")

    class UniqueId(ctypes.Structure):
        _fields_ = [("internal", ctypes.c_byte * 128)]

    uid = UniqueId()
    assert rccl.ncclGetUniqueId(ctypes.byref(uid)) == 0
    comm = ctypes.c_void_p()
    rccl.ncclCommInitRank.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, UniqueId, ctypes.c_int]
    assert rccl.ncclCommInitRank(ctypes.byref(comm), 1, uid, 0) == 0
    try:
        a, per = one_rank_refs[(m, n)]
        L = bq.lib()
        wq = torch.empty(L.tsqr_mi_working_q_size_f64_dist(m, n, 1), dtype=torch.float64, device="cuda")
        wr = torch.empty(L.tsqr_mi_working_r_size_f64_dist(m, n, 1), dtype=torch.float64, device="cuda")
        for reorth in (0, 1):
            q_ref, r_ref, sweeps_ref = per[reorth]
            q = torch.full_like(a, float("nan"))
            r = torch.full((n, n), float("nan"), dtype=torch.float64, device="cuda")
            rc = L.tsqr_mi_qr_f64_dist_fn(reorth, q.data_ptr(), m, r.data_ptr(), n, a.data_ptr(), m, m, n, wq.data_ptr(), wr.data_ptr(),
                                          comm, ctypes.cast(rccl.ncclAllReduce, ctypes.c_void_p), 1, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert rc == 0, (rc, bq.last_error())
            assert L.tsqr_mi_last_sweeps_f64() == sweeps_ref
            assert _same_bits(q, q_ref) and _same_bits(r, r_ref), (m, n, reorth)
    finally:
        rccl.ncclCommDestroy.argtypes = [ctypes.c_void_p]
        rccl.ncclCommDestroy(comm)


# ---- several ranks: every case of a world size inside one spawn ---------------------------------------------------------------------------
def _run_case(rank, world, case):
    """one row-partitioned call per rank; rank 0 returns the properties of the stacked factorisation, computed on the host in fp64"""
    import torch
    import torch.distributed as dist
    from tsqr_gpu_amd import blockqr as bq, dist as tdist
    heights, n, reorth = case["heights"], case["n"], case["reorth"]
    a_glob = _matrix(case)
    row0, m_local = sum(heights[:rank]), heights[rank]
    d_a = torch.from_numpy(np.ascontiguousarray(a_glob[row0:row0 + m_local].T)).cuda()
    keep = d_a.clone()
    d_q = torch.full_like(d_a, float("nan"))
    d_r = torch.full((n, n), float("nan"), dtype=torch.float64, device="cuda")
    drv = tdist.RowPartitionedQRF64(m_local, n, comm="callbacks")
    st = drv.qr(d_q, m_local, d_r, d_a, m_local, reorthogonalize=bool(reorth))
    torch.cuda.synchronize()
    info = torch.tensor([st, drv.last_sweeps, int(_same_bits(keep, d_a))], dtype=torch.int64)
    infos = [torch.zeros(3, dtype=torch.int64) for _ in range(world)]
    dist.all_gather(infos, info)
    r_bits = d_r.cpu().view(torch.int64)
    rs = [torch.zeros(n, n, dtype=torch.int64) for _ in range(world)]
    dist.all_gather(rs, r_bits)
    mmax = max(heights)
    qpad = torch.zeros(n, mmax, dtype=torch.float64); qpad[:, :m_local] = d_q.cpu()
    qs = [torch.zeros(n, mmax, dtype=torch.float64) for _ in range(world)]
    dist.all_gather(qs, qpad)
    if rank != 0:
        return None
    res = {"transport": drv.transport, "states": [int(t[0]) for t in infos], "sweeps": [int(t[1]) for t in infos],
           "a_untouched": all(int(t[2]) == 1 for t in infos), "r_same": all(torch.equal(rs[0], t) for t in rs)}
    if any(res["states"]):
        return res
    q = np.concatenate([t.numpy().T[:heights[k]] for k, t in enumerate(qs)], axis=0)
    r = d_r.cpu().numpy().T
    res["tril_zero"] = bool(np.all(np.tril(r, -1) == 0.0))
    res["diag_positive"] = bool(np.all(np.diag(r) > 0.0))
    res["orth"] = float(np.linalg.norm(q.T @ q - np.eye(n)))
    res["residual"] = float(np.linalg.norm(a_glob - q @ r) / np.linalg.norm(a_glob))
    if case["single"]:                                       # the one-GPU entry on the stacked matrix, in this process
        m = sum(heights)
        s_a = torch.from_numpy(np.ascontiguousarray(a_glob.T)).cuda()
        s_q = torch.empty_like(s_a); s_r = torch.zeros(n, n, dtype=torch.float64, device="cuda")
        bf = bq.buffer_f64_wide(bool(reorth))
        bf.allocate(m, n)
        assert bq.qr_f64_wide(s_q, m, s_r, n, s_a, m, m, n, bf) == 0, bq.last_error()
        torch.cuda.synchronize()
        r1 = s_r.cpu().numpy().T
        res["r_vs_single"] = float(np.linalg.norm(r - r1) / np.linalg.norm(r1))
        res["cond"] = float(np.linalg.cond(a_glob))
        res["single_sweeps"] = bq.last_sweeps_f64()
    return res


def _worker64(rank, world, port, heights, n, cases, reorth, policy, cond, loop, out):
    """(the argument list of tests/test_gpu_dist.py's workers; `cases` travels in the place of its mode)"""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    results = [_run_case(rank, world, case) for case in cases]
    if rank == 0:
        out.put({"cases": results})
    dist.destroy_process_group()


def _spawn(world, cases):
    """one group of `world` processes for all `cases`: guarded workers, polling parent, no rank left on the card (test_gpu_dist._run)"""
    assert world <= 4 and all(len(c["heights"]) == world for c in cases)
    return _spawn_ranks((0,) * world, 0, mode=cases, worker=_worker64)["cases"]


def _check_case(case, res, r_ratio=None):
    n, reorth = case["n"], case["reorth"]
    orth_max, res_max = _bands(n, reorth)
    print("heights %s n %d reorth %d %s: sweeps %s  ||QtQ-I||_F %.2e  residual %.2e%s" % (
        case["heights"], n, reorth, case["kind"], res["sweeps"], res.get("orth", -1), res.get("residual", -1),
        "  |R - R_single| / |R_single| %.2e (cond %.2e, single sweeps %d)" % (res["r_vs_single"], res["cond"], res["single_sweeps"])
        if "r_vs_single" in res else ""))
    assert res["transport"] == "torch.distributed callbacks"
    assert res["states"] == [0] * len(case["heights"]), res["states"]
    assert res["r_same"], "R differs between ranks"
    assert len(set(res["sweeps"])) == 1, res["sweeps"]
    assert res["a_untouched"]
    assert res["tril_zero"] and res["diag_positive"]
    assert res["orth"] <= orth_max, ("orthogonality", res["orth"], orth_max)
    assert res["residual"] <= res_max, ("residual", res["residual"])
    if case["single"]:
        # two factorisations inside the header's residual and orthogonality bands can differ by this much, to first order
        bound = 2e-11 * max(1.0, n / 64.0) + 3e-13 * res["cond"]
        assert res["r_vs_single"] <= bound, ("R against the one-GPU entry", res["r_vs_single"], bound)
        if r_ratio is not None:
            r_ratio.append(res["r_vs_single"])


def test_two_ranks(bq):
    """unequal blocks, a block shorter than n, n beyond 64 (the wide sweeps) and reorth = 1; cond 1e8 and 1e12 (shifted path, the
    same on both ranks); a NaN in rank 1's block (state 3 on both ranks, through the sum)"""
    cases = [_case((3000, 1777), 64, single=True), _case((40, 5000), 64, single=True), _case((2000, 1500), 130, single=True),
             _case((1500, 1100), 200, reorth=1, single=True),
             _case((9000, 7384), 64, kind="cond", cond=1e8), _case((9000, 7384), 64, kind="cond", cond=1e12),
             _case((3000, 1777), 64, kind="nan"), _case((2000, 1500), 130, kind="nan")]
    results = _spawn(2, cases)
    ratios = []
    for case, res in zip(cases[:4], results[:4]):
        _check_case(case, res, ratios)
    print("largest |R_dist - R_single| / |R_single| over two ranks: %.2e" % max(ratios))
    for case, res in zip(cases[4:6], results[4:6]):
        _check_case(case, res)
        assert res["sweeps"][0] >= 103, res["sweeps"]
    for case, res in zip(cases[6:], results[6:]):
        print("NaN on rank 1, n %d: states %s sweeps %s" % (case["n"], res["states"], res["sweeps"]))
        assert res["states"] == [3, 3] and len(set(res["sweeps"])) == 1, res


def _ladder_cases():
    from tests import pass_refs_f64 as p64
    mx_global = p64.rule(4096, 64)[0]
    return mx_global, [_case((1024,) * 4, 64, kind="ladder", s_target=2.0 * mx_global, seed=64),
                       _case((1024,) * 4, 64, kind="ladder", s_target=mx_global / 4.0, seed=64)]


def test_four_ranks_and_the_global_row_count(bq):
    """heights from one row to 3000; then four blocks of 1024 rows with S_ref prescribed between the CholeskyQR2 bound of the global
    row count and that of a block's: a rule fed with the LOCAL row count accepts (2 sweeps), the rule of the header rejects and takes
    the shifted path (103) on every rank.  Control: S_ref below both bounds gives 2."""
    from tests import pass_refs_f64 as p64
    mx_global, ladder = _ladder_cases()
    mx_local = p64.rule(1024, 64)[0]
    a = _matrix(ladder[0])
    s_ref = p64.scond_ref(p64.matmul_ld(a.T, a))[0]           # (longdouble, on the CPU, before anything runs on the GPU)
    print("S_ref %.6g between 1.5 max_scond(4096, 64) = %.6g and max_scond(1024, 64) / 1.5 = %.6g" % (s_ref, 1.5 * mx_global, mx_local / 1.5))
    assert 1.5 * mx_global <= s_ref <= mx_local / 1.5
    cases = [_case((3000, 1, 777, 1234), 48, single=True)] + ladder
    results = _spawn(4, cases)
    for case, res in zip(cases, results):
        _check_case(case, res)
    assert results[1]["sweeps"] == [103] * 4, results[1]["sweeps"]
    assert results[2]["sweeps"] == [2] * 4, results[2]["sweeps"]

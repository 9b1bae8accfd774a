"""The minimum-norm rank-aware fp64 least-squares entry end to end, through blockqr.lstsq_rank_f64(..., minimum_norm=True) and through
the C entry (a C++ caller of mtk::qr::lstsq_minnorm_fp64): the seven cases of tests/pass_refs_f64_lsq_rank.py with both kinds of
right-hand side at refine = 1, held to pass_refs_f64_lsq_minnorm.check -- the expected rank and
rel_err(X, X*) <= max(2 x LAPACK's, 4 n 2^-53) against the extended-precision minimum-norm solution of the truncated problem, LAPACK's
being numpy.linalg.lstsq on the same projected problem; r, p, rank and the sweep count bitwise the basic call's; X bitwise the basic
call's at full rank; equal rows for copied columns; ||X|| no larger and the residual no worse than the basic call's; the same bits for
the four layout pairs and from call to call; the states.

Measured on the device (MI355X, refine = 1), err / LAPACK's / bound per case: profiles/fp64_lstsq_minnorm_accuracy.md has the table."""
import os
import subprocess

import numpy as np
import pytest

from tests import pass_refs_f64_lsq_minnorm as pm
from tests import pass_refs_f64_lsq_rank as pk
from tests.test_gpu_f64_lstsq_rank import bits, dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [c[0] for c in pk.CASES]


@pytest.fixture(scope="module")
def gpu(bq):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return bq, torch


_solved = {}


def solve_case(gpu, name, kind, refine=1, minimum_norm=True):
    """(x, r, p, rank, sweeps) of a case with the layouts, reorth and rcond it names; computed once per key"""
    bq, torch = gpu
    key = (name, kind, refine, minimum_norm)
    if key not in _solved:
        _, m, n, _, rcond, _, a_row, b_row, reorth = next(c for c in pk.CASES if c[0] == name)
        a, b = dev(torch, pk.case_matrix(name), a_row), dev(torch, pk.case_rhs(name, kind), b_row)
        x, r, p, rank = bq.lstsq_rank_f64(a, b, rcond=rcond, reorth=bool(reorth), refine=refine, minimum_norm=minimum_norm)
        _solved[key] = (x, r, p, rank, bq.last_sweeps_f64())
    return _solved[key]


@pytest.mark.parametrize("kind", pk.RHS_KINDS)
@pytest.mark.parametrize("case", pk.CASES, ids=IDS)
def test_case_is_inside_the_bound(gpu, case, kind):
    bq, torch = gpu
    name, m, n, nrhs = case[:4]
    x, r, p, rank, _ = solve_case(gpu, name, kind)
    assert tuple(x.shape) == (n, nrhs) and tuple(r.shape) == (n, n) and p.dtype == torch.int32 and isinstance(rank, int)
    xh, ph = x.cpu().numpy(), p.cpu().numpy()
    f = pm.figures(name, kind, xh, ph, rank) if sorted(ph.tolist()) == list(range(n)) else None
    print("lstsq_minnorm %-16s %-10s rank %2d figures %s" % (name, kind, rank, f))
    pm.check(name, kind, xh, ph, rank)


@pytest.mark.parametrize("kind", pk.RHS_KINDS)
@pytest.mark.parametrize("case", pk.CASES, ids=IDS)
def test_against_the_basic_call(gpu, case, kind):
    """r, p, rank and the sweep count bitwise the basic call's; ||X|| <= ||X_basic|| per column; ||B - A X|| within rounding of the
    basic call's (both solve the same truncated problem: the residuals differ by the two solves' errors, each below the bound of
    check() times ||A|| ||X||); at full rank X bitwise the basic call's"""
    name, m, n = case[:3]
    x, r, p, rank, sweeps = solve_case(gpu, name, kind)
    x0, r0, p0, rank0, sweeps0 = solve_case(gpu, name, kind, minimum_norm=False)
    assert rank == rank0 and sweeps == sweeps0 and np.array_equal(bits(r), bits(r0)) and np.array_equal(p.cpu().numpy(), p0.cpu().numpy())
    xh, x0h = x.cpu().numpy(), x0.cpu().numpy()
    assert np.all(np.linalg.norm(xh, axis=0) <= np.linalg.norm(x0h, axis=0) * (1 + 4 * pk.U))
    a64, b = np.asarray(pk.case_matrix(name)), np.asarray(pk.case_rhs(name, kind), pk.LD).reshape(m, -1)
    a = a64.astype(pk.LD)
    fro = lambda e: np.sqrt(np.sum(e * e))
    res, res0 = fro(b - a @ xh.reshape(n, -1)), fro(b - a @ x0h.reshape(n, -1))
    f = pm.figures(name, kind, xh, p.cpu().numpy(), rank)
    slack = 2.0 * f["bound"] * np.linalg.norm(a64, 2) * (np.linalg.norm(xh) + np.linalg.norm(x0h))
    # what the truncation leaves out of A moves the residual too: ||A - Q1 Q1^T A|| ||X||, zero to rounding at exact rank
    q1, _ = np.linalg.qr(a64[:, p.cpu().numpy()[:rank]])
    left_out = np.linalg.norm(a64 - q1 @ (q1.T @ a64), 2)
    slack += left_out * (np.linalg.norm(xh) + np.linalg.norm(x0h))
    print("lstsq_minnorm %-16s %-10s ||X|| %.6g basic %.6g  residual %.17g basic %.17g slack %.2e" % (
        name, kind, np.linalg.norm(xh), np.linalg.norm(x0h), float(res), float(res0), float(slack)))
    assert abs(float(res - res0)) <= slack
    if name in ("full_300x17", "one_65x1"):
        assert rank == n and np.array_equal(bits(x), bits(x0))


def test_copied_columns_have_equal_rows(gpu):
    """copied_4096x16: rows 4 and 11 of X agree to 16 x 2^-53 relative; tail3_100x7: rows 3 .. 6 likewise"""
    for name, rows in (("copied_4096x16", (4, 11)), ("tail3_100x7", (3, 4, 5, 6))):
        for kind in pk.RHS_KINDS:
            xh = solve_case(gpu, name, kind)[0].cpu().numpy()
            for i in rows[1:]:
                d = np.abs(xh[i] - xh[rows[0]]) / np.abs(xh[rows[0]])
                print("lstsq_minnorm %-16s %-10s rows %d and %d differ by %.2e relative" % (name, kind, rows[0], i, d.max()))
                assert np.all(d <= 16 * pk.U), (name, kind, i, d.max())


def test_norm_of_the_copied_case(gpu):
    assert abs(float(np.linalg.norm(solve_case(gpu, "copied_4096x16", "gaussian")[0].cpu().numpy())) - 0.148) < 1e-3


@pytest.mark.parametrize("name", ["rank32_1029x51", "tail3_100x7"])
def test_row_major_and_column_major_operands_give_the_same_bits(gpu, name):
    bq, torch = gpu
    _, m, n, _, rcond, _, _, _, reorth = next(c for c in pk.CASES if c[0] == name)
    ah, bh = pk.case_matrix(name), pk.case_rhs(name, "gaussian")
    out = []
    for a_row, b_row in ((0, 0), (1, 1), (1, 0), (0, 1)):
        x, r, p, rank = bq.lstsq_rank_f64(dev(torch, ah, a_row), dev(torch, bh, b_row), rcond=rcond, reorth=bool(reorth), minimum_norm=True)
        out.append((bits(x), bits(r), p.cpu().numpy(), rank))
    for other in out[1:]:
        assert all(np.array_equal(u, v) for u, v in zip(out[0][:3], other[:3])) and out[0][3] == other[3]


@pytest.mark.parametrize("name", ["copied_4096x16", "rank40_4097x64"])
def test_two_calls_give_equal_bits(gpu, name):
    bq, torch = gpu
    _, m, n, _, rcond, _, a_row, b_row, reorth = next(c for c in pk.CASES if c[0] == name)
    a, b = dev(torch, pk.case_matrix(name), a_row), dev(torch, pk.case_rhs(name, "gaussian"), b_row)
    x1, r1, p1, k1 = bq.lstsq_rank_f64(a, b, rcond=rcond, reorth=bool(reorth), minimum_norm=True)
    x0, r0, p0, k0, _ = solve_case(gpu, name, "gaussian")
    assert np.array_equal(bits(x0), bits(x1)) and np.array_equal(bits(r0), bits(r1)) and torch.equal(p0, p1) and k0 == k1


def test_one_dimensional_b(gpu):
    bq, torch = gpu
    name = "copied_4096x16"
    a, b = dev(torch, pk.case_matrix(name), 0), dev(torch, pk.case_rhs(name, "gaussian"), 0)
    x, r, p, rank = bq.lstsq_rank_f64(a, b[:, 2], rcond=1e-8, minimum_norm=True)
    x2, _, _, rank2 = bq.lstsq_rank_f64(a, b[:, 2:3], rcond=1e-8, minimum_norm=True)
    assert tuple(x.shape) == (16,) and rank == rank2 == 15 and np.array_equal(bits(x), bits(x2[:, 0]))


@pytest.mark.parametrize("refine", [0, 2])
def test_other_refine_counts_run_and_return_finite_x(gpu, refine):
    for name in ("copied_4096x16", "rank1_777x33"):
        k_expected = next(c[5] for c in pk.CASES if c[0] == name)
        x, _, p, rank, _ = solve_case(gpu, name, "gaussian", refine)
        xh = x.cpu().numpy()
        print("lstsq_minnorm %-16s refine %d: %s" % (name, refine, pm.figures(name, "gaussian", xh, p.cpu().numpy(), rank)))
        assert rank == k_expected and np.isfinite(xh).all()


def test_nan_in_a_is_state_3(gpu):
    bq, torch = gpu
    a = np.array(pk.case_matrix("full_300x17"))
    a[123, 5] = np.nan
    with pytest.raises(bq.LstsqRankError) as e:
        bq.lstsq_rank_f64(dev(torch, a, 0), dev(torch, pk.case_rhs("full_300x17", "gaussian"), 0), minimum_norm=True)
    assert e.value.state == 3


def test_cpp_sample(gpu):
    """tests/cpp/sample_fp64_lstsq_minnorm.cpp, compiled and linked the way tests/test_f64_lstsq_minnorm_abi.py does it: a copied column
    among 16 gives rank 15 from both entries, equal rows 4 and 11 and a norm no larger than the basic solution's"""
    from abi_util import compile_and_link
    with compile_and_link(os.path.join(ROOT, "tests", "cpp", "sample_fp64_lstsq_minnorm.cpp"), "sample_fp64_lstsq_minnorm") as exe:
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0 and "states 0 0, ranks 15 15 of 16," in out.stdout and "not larger" in out.stdout, out.stdout + out.stderr
    twin = float(out.stdout.split("differ by ")[1].split(" ")[0])
    assert twin <= 16 * pk.U

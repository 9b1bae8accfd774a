"""The rank-aware fp64 least-squares entry end to end, through blockqr.lstsq_rank_f64 and through the C entry (a C++ caller of
mtk::qr::lstsq_rank_fp64): the seven cases of tests/pass_refs_f64_lsq_rank.py with both kinds of right-hand side, held to
pass_refs_f64_lsq_rank.check as it stands -- the expected rank, exact zeros in the dropped rows, the error on the retained columns within
max(2 x LAPACK's, 4 n 2^-53) of an extended-precision solve -- r, p and the sweep count bitwise those of the pivoted QR without Q, the
same bits for either layout of the operands and from call to call, and the states.

Measured on the device (MI355X, refine = 1), err / LAPACK's / bound per case: profiles/fp64_lstsq_rank_accuracy.md has the table."""
import os
import subprocess

import numpy as np
import pytest

from tests import pass_refs_f64_lsq_rank as pk

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gpu(bq):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return bq, torch


def dev(torch, h, row_major):
    """h on the device, rows contiguous (row_major) or columns contiguous"""
    t = torch.from_numpy(np.ascontiguousarray(h)).cuda()
    return t if row_major else t.t().contiguous().t()


def bits(t):
    return t.contiguous().cpu().numpy().view(np.int64)


_solved = {}


def solve_case(gpu, name, kind, refine=1):
    """(x, r, p, rank, sweeps) of a case with the layouts, reorth and rcond it names; computed once per (case, kind, refine)"""
    bq, torch = gpu
    key = (name, kind, refine)
    if key not in _solved:
        _, m, n, _, rcond, _, a_row, b_row, reorth = next(c for c in pk.CASES if c[0] == name)
        a, b = dev(torch, pk.case_matrix(name), a_row), dev(torch, pk.case_rhs(name, kind), b_row)
        x, r, p, rank = bq.lstsq_rank_f64(a, b, rcond=rcond, reorth=bool(reorth), refine=refine)
        _solved[key] = (x, r, p, rank, bq.last_sweeps_f64())
    return _solved[key]


@pytest.mark.parametrize("kind", pk.RHS_KINDS)
@pytest.mark.parametrize("case", pk.CASES, ids=[c[0] for c in pk.CASES])
def test_case_is_inside_the_bound(gpu, case, kind):
    """pass_refs_f64_lsq_rank.check as it stands: rank, permutation, exact zero rows, err <= max(2 x LAPACK's, 4 n 2^-53)"""
    bq, torch = gpu
    name, m, n, nrhs = case[:4]
    x, r, p, rank, _ = solve_case(gpu, name, kind)
    assert tuple(x.shape) == (n, nrhs) and tuple(r.shape) == (n, n) and p.dtype == torch.int32 and isinstance(rank, int)
    xh, ph = x.cpu().numpy(), p.cpu().numpy()
    f = pk.figures(name, kind, xh, ph, rank) if sorted(ph.tolist()) == list(range(n)) else None
    print("lstsq_rank %-16s %-10s rank %2d figures %s" % (name, kind, rank, f))
    pk.check(name, kind, xh, ph, rank)


@pytest.mark.parametrize("case", pk.CASES, ids=[c[0] for c in pk.CASES])
def test_r_jpvt_and_sweeps_are_the_pivoted_qr_s(gpu, case):
    """r, jpvt and tsqr_mi_last_sweeps_f64 are bitwise those of the pivoted QR without Q on the same a, layout and reorth"""
    bq, torch = gpu
    name, a_row, reorth = case[0], case[6], case[8]
    _, r, p, _, sweeps = solve_case(gpu, name, "gaussian")
    a = dev(torch, pk.case_matrix(name), a_row)
    r2, p2 = bq.qrcp_f64_tensor(a, reorth=bool(reorth), compute_q=False)
    assert bq.last_sweeps_f64() == sweeps
    assert np.array_equal(bits(r), bits(r2)) and np.array_equal(p.cpu().numpy(), p2.cpu().numpy().astype(np.int32))
    rh = r.cpu().numpy()
    assert not np.tril(rh, -1).any()


@pytest.mark.parametrize("name", ["rank32_1029x51", "tail3_100x7"])
def test_row_major_and_column_major_operands_give_the_same_bits(gpu, name):
    bq, torch = gpu
    _, m, n, _, rcond, _, _, _, reorth = next(c for c in pk.CASES if c[0] == name)
    ah, bh = pk.case_matrix(name), pk.case_rhs(name, "gaussian")
    out = []
    for a_row, b_row in ((0, 0), (1, 1), (1, 0), (0, 1)):
        x, r, p, rank = bq.lstsq_rank_f64(dev(torch, ah, a_row), dev(torch, bh, b_row), rcond=rcond, reorth=bool(reorth))
        out.append((bits(x), bits(r), p.cpu().numpy(), rank))
    for other in out[1:]:
        assert all(np.array_equal(u, v) for u, v in zip(out[0][:3], other[:3])) and out[0][3] == other[3]


@pytest.mark.parametrize("name", ["copied_4096x16", "rank40_4097x64"])
def test_two_calls_give_equal_bits(gpu, name):
    bq, torch = gpu
    _, m, n, _, rcond, _, a_row, b_row, reorth = next(c for c in pk.CASES if c[0] == name)
    a, b = dev(torch, pk.case_matrix(name), a_row), dev(torch, pk.case_rhs(name, "gaussian"), b_row)
    x1, r1, p1, k1 = bq.lstsq_rank_f64(a, b, rcond=rcond, reorth=bool(reorth))
    x0, r0, p0, k0, _ = solve_case(gpu, name, "gaussian")
    assert np.array_equal(bits(x0), bits(x1)) and np.array_equal(bits(r0), bits(r1)) and torch.equal(p0, p1) and k0 == k1


def test_one_dimensional_b(gpu):
    bq, torch = gpu
    name = "copied_4096x16"
    a, b = dev(torch, pk.case_matrix(name), 0), dev(torch, pk.case_rhs(name, "gaussian"), 0)
    x, r, p, rank = bq.lstsq_rank_f64(a, b[:, 2], rcond=1e-8)
    x2, _, _, rank2 = bq.lstsq_rank_f64(a, b[:, 2:3], rcond=1e-8)
    assert tuple(x.shape) == (16,) and rank == rank2 == 15 and np.array_equal(bits(x), bits(x2[:, 0]))


@pytest.mark.parametrize("refine", [0, 2])
def test_other_refine_counts_run_and_leave_zero_rows(gpu, refine):
    for name in ("copied_4096x16", "rank1_777x33"):
        k_expected = next(c[5] for c in pk.CASES if c[0] == name)
        x, _, p, rank, _ = solve_case(gpu, name, "gaussian", refine)
        xh, ph = x.cpu().numpy(), p.cpu().numpy()
        f = pk.figures(name, "gaussian", xh, ph, rank)
        print("lstsq_rank %-16s refine %d: %s" % (name, refine, f))
        assert rank == k_expected and f["zero_rows"] and np.isfinite(xh).all()


def test_full_rank_case_has_rank_17(gpu):
    assert solve_case(gpu, "full_300x17", "gaussian")[3] == 17
    assert solve_case(gpu, "full_300x17", "consistent")[3] == 17


def test_nan_in_a_is_state_3(gpu):
    bq, torch = gpu
    a = np.array(pk.case_matrix("full_300x17"))
    a[123, 5] = np.nan
    with pytest.raises(bq.LstsqRankError) as e:
        bq.lstsq_rank_f64(dev(torch, a, 0), dev(torch, pk.case_rhs("full_300x17", "gaussian"), 0))
    assert e.value.state == 3


def test_cpp_sample_reports_rank_15(gpu):
    """tests/cpp/sample_fp64_lstsq_rank.cpp, compiled and linked the way tests/test_f64_lstsq_rank_abi.py does it: a copied column
    among 16 gives rank 15 and one zero row of x"""
    from abi_util import compile_and_link
    with compile_and_link(os.path.join(ROOT, "tests", "cpp", "sample_fp64_lstsq_rank.cpp"), "sample_fp64_lstsq_rank") as exe:
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0 and "state 0, rank 15 of 16, zero rows of x 1," in out.stdout, out.stdout + out.stderr

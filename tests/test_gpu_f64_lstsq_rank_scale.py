"""The two rank-aware fp64 least-squares entries (tsqr_mi_lstsq_rank_f64, tsqr_mi_lstsq_minnorm_f64) through their C entries, between
the seven hand-picked cases of tests/pass_refs_f64_lsq_rank.py: with padded leading dimensions and guard bands, with the rank rule ON
its threshold, with the rank on every edge of the 16-column tiles, and under power-of-two scaling of A and B.  Every case runs BOTH
entries and prints its figures before it asserts.  Generators, exponents, expected values and measures:
tests/pass_refs_f64_lsq_rank_scale.py; tests/test_pass_refs_f64_lsq_rank_scale.py proves every precondition on the CPU and shows that
each assertion catches a defect.  What the device printed: profiles/fp64_lstsq_rank_scale_tests.md.

Expected values come from numpy, longdouble or closed forms, never from the library -- with one exception made on purpose: part 2 reads
the device's own r, because the thing under test there is the rule applied to r (one IEEE multiply and one compare, repeated in numpy:
an exact expectation that rests on no assumption about how r was computed), not r.
The only bounds are "bit for bit", 4 n 2^-53 (pass_refs_f64_lsq.floor_of) and the header's max(2 x LAPACK's, 4 n 2^-53)."""
import ctypes

import numpy as np
import pytest

from tests import pass_refs_f64_lsq as pl
from tests import pass_refs_f64_lsq_minnorm as pm
from tests import pass_refs_f64_lsq_rank as pk
from tests import pass_refs_f64_lsq_rank_scale as pr
from tests import pass_refs_f64_scale as ps
from tests.test_gpu_f64_qrcp import COL, ISENT, NAN, PAIRS, ROW, dev

pytestmark = pytest.mark.gpu
vp = ctypes.c_void_p
ENTRIES = ((False, "tsqr_mi_lstsq_rank_f64"), (True, "tsqr_mi_lstsq_minnorm_f64"))


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


# ---- 0: a caller of the C entries with guard bands -------------------------------------------------------------------------------------------
def rank_call(bq, a, b, a_layout, b_layout, reorth, refine, rcond, minimum_norm, pad=(3, 5, 2, 1)):
    """tsqr_mi_lstsq_rank_f64 (minimum_norm: tsqr_mi_lstsq_minnorm_f64) on device copies of a (m x n) and b (m x nrhs) in the layouts
    named, with lda, ldb, ldx, ldr above the minimum by pad and NaN in the padding; x and r pre-filled with NaN, jpvt between two -777
    sentinels, rank the middle one of three host ints pre-set to -777, the work space sized by the entry's own functions.  rcond None:
    -1.0, the default.  After the call, WHATEVER its state: a and b keep their bits, the padding of x and r is still NaN, the sentinels
    of jpvt and the two outer host ints are intact.  -> (state, sweeps, x (n x nrhs, host), r (n x n, host), jpvt (host), rank, the
    text of tsqr_mi_last_error)."""
    torch = _torch()
    L = bq.lib()
    m, n = a.shape
    nrhs = b.shape[1]
    name = "lstsq_minnorm" if minimum_norm else "lstsq_rank"
    apool, ad, lda = dev(torch, a, a_layout, pad[0])
    bpool, bd, ldb = dev(torch, b, b_layout, pad[1])
    before = apool.clone(), bpool.clone()
    ldx, ldr = n + pad[2], n + pad[3]
    x = torch.full((nrhs, ldx), NAN, dtype=torch.float64, device="cuda")
    r = torch.full((n, ldr), NAN, dtype=torch.float64, device="cuda")
    jp = torch.full((n + 2,), ISENT, dtype=torch.int32, device="cuda")
    rank = (ctypes.c_int * 3)(ISENT, ISENT, ISENT)
    wq = torch.empty(getattr(L, "tsqr_mi_working_q_size_f64_" + name)(m, n, nrhs), dtype=torch.float64, device="cuda")
    wr = torch.empty(getattr(L, "tsqr_mi_working_r_size_f64_" + name)(m, n, nrhs), dtype=torch.float64, device="cuda")
    state = getattr(L, "tsqr_mi_%s_f64" % name)(
        a_layout, b_layout, int(reorth), int(refine), -1.0 if rcond is None else float(rcond), vp(x.data_ptr()), ldx, vp(r.data_ptr()), ldr,
        vp(jp.data_ptr() + 4), ctypes.cast(ctypes.byref(rank, ctypes.sizeof(ctypes.c_int)), ctypes.POINTER(ctypes.c_int)),
        vp(ad.data_ptr()), lda, vp(bd.data_ptr()), ldb, m, n, nrhs, vp(wq.data_ptr()), vp(wr.data_ptr()),
        vp(torch.cuda.current_stream().cuda_stream))
    sweeps = L.tsqr_mi_last_sweeps_f64()
    text = bq.last_error()
    torch.cuda.synchronize()
    i64 = torch.int64
    assert torch.equal(apool.view(i64), before[0].view(i64)), "A was written"
    assert torch.equal(bpool.view(i64), before[1].view(i64)), "B was written"
    assert bool(torch.isnan(x[:, n:]).all()), "the padding of x was written"
    assert bool(torch.isnan(r[:, n:]).all()), "the padding of r was written"
    assert int(jp[0]) == ISENT and int(jp[-1]) == ISENT, "jpvt was written outside its n values"
    assert rank[0] == ISENT and rank[2] == ISENT, "a host int next to *rank was written"
    return (state, sweeps, x[:, :n].t().cpu().numpy().copy(), r[:, :n].t().cpu().numpy().copy(), jp[1:-1].cpu().numpy().copy(),
            int(rank[1]), text)


def _same_result(u, v, with_x=True):
    """(state, sweeps, x, r, jpvt, rank) of two calls agree in every bit; with_x False: all but x"""
    return (u[0] == v[0] and u[1] == v[1] and (not with_x or pl.same_bits(u[2], v[2])) and pl.same_bits(u[3], v[3])
            and np.array_equal(u[4], v[4]) and u[5] == v[5])


def _operands(name):
    _, m, n, nrhs, rcond, k_expected, a_row, b_row, reorth = pr.case_of(name)
    return pk.case_matrix(name), pk.case_rhs(name, "gaussian"), rcond, k_expected, a_row, b_row, reorth


# ---- 1: the C entry against the tensor call --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pr.ENTRY_CASES)
def test_c_entry_is_the_tensor_call_in_every_layout(bq, name):
    """x, r, jpvt, rank and the sweep count of rank_call -- padded leading dimensions, guard bands -- are bitwise those of
    blockqr.lstsq_rank_f64 on the same data (minimal leading dimensions), and equal across the four layout pairs, for both entries"""
    torch = _torch()
    a, b, rcond, k_expected, _, _, reorth = _operands(name)
    at, bt = torch.from_numpy(np.array(a)).cuda(), torch.from_numpy(np.array(b)).cuda()
    for minimum_norm, symbol in ENTRIES:
        xt, rt, pt, kt = bq.lstsq_rank_f64(at, bt, rcond=rcond, reorth=bool(reorth), minimum_norm=minimum_norm)
        want = (0, bq.last_sweeps_f64(), xt.cpu().numpy(), rt.cpu().numpy(), pt.cpu().numpy(), kt)
        print("%s %s: tensor call rank %d sweeps %d" % (symbol, name, kt, want[1]))
        assert kt == k_expected
        for a_lay, b_lay in PAIRS:
            got = rank_call(bq, a, b, a_lay, b_lay, reorth, 1, rcond, minimum_norm)
            assert got[0] == 0, (symbol, name, a_lay, b_lay, got[0], got[6])
            assert _same_result(got, want), (symbol, name, "the C entry differs from the tensor call", a_lay, b_lay, got[5], got[1])
    # other paddings, the minimal ones included, change nothing
    base = rank_call(bq, a, b, COL, ROW, reorth, 1, rcond, False)
    for pad in ((0, 0, 0, 0), (1, 2, 7, 5)):
        assert _same_result(rank_call(bq, a, b, COL, ROW, reorth, 1, rcond, False, pad=pad), base), (name, pad)


# ---- 2: the rank rule at its threshold, read off the device's own R -------------------------------------------------------------------------
@pytest.mark.parametrize("name", pr.THRESHOLD_CASES)
def test_rank_rule_at_its_threshold(bq, name):
    """One call with the case's rcond gives the device's r; pass_refs_f64_lsq_rank_scale.threshold_rconds builds from diag(r) the values
    0, -1 (the default), the case's own and, around the ratio q = r_jj / r_00 of five to seven pivots (k_expected - 1, k_expected and
    n - 1 among them), nextafter(q, 0), q, nextafter(q, 1).  For EVERY value and both entries: the state is 0 or 3, and 3 only with the
    entry's own text; rank == rank_of(r, rcond) exactly, in state 3 too (the header: *rank is written); r, jpvt and the sweep count are
    bitwise the first call's (rcond reaches neither the ladder nor the pivoting kernel); state 0: x finite and, in the basic entry,
    exact zeros in the rows jpvt[rank:]; state 3: x all exact zeros; at rank == n the minimum-norm x is bitwise the basic x.  Accuracy
    (pass_refs_f64_lsq_rank.figures / pass_refs_f64_lsq_minnorm.figures, bound max(2 x LAPACK's, 4 n 2^-53)) is asserted for the values
    whose retained set is the case's k_expected columns -- the header's claim and nothing more -- and printed for the others.
    At least one value must land exactly on fl(rcond r_00) == r_jj: there > and >= part."""
    a, b, rcond, k_expected, a_row, b_row, reorth = _operands(name)
    m, n = a.shape
    first = {mn: rank_call(bq, a, b, a_row, b_row, reorth, 1, rcond, mn) for mn, _ in ENTRIES}
    assert first[False][0] == 0 and first[True][0] == 0, (name, first[False][6], first[True][6])
    assert _same_result(first[False], first[True], with_x=False), "r, jpvt, rank or the sweeps differ between the entries"
    r, jpvt, sweeps = first[False][3], first[False][4], first[False][1]
    assert sorted(jpvt.tolist()) == list(range(n)) and first[False][5] == k_expected
    d = np.diag(r)
    values = pr.threshold_rconds(d, m, n, k_expected, rcond)
    print("threshold %s: sweeps %d, diag(r)/r_00 at %s: %s" % (name, sweeps, pr.threshold_indices(n, k_expected),
                                                              ["%.3e" % (d[j] / d[0]) for j in pr.threshold_indices(n, k_expected)]))
    landed, met_3 = [], []
    for label, v in values:
        rc = pr.default_rcond(m, n) if v < 0 else v
        want = pk.rank_of(r, rc)
        if pr.lands_on(d, rc):
            landed.append(label)
        xs = {}
        for mn, symbol in ENTRIES:
            state, sw, x, r1, p1, rank, text = rank_call(bq, a, b, a_row, b_row, reorth, 1, v, mn)
            xs[mn] = x if state == 0 else None
            fig = None
            if state == 0 and np.isfinite(x).all():
                fig = (pm if mn else pk).figures(name, "gaussian", x, p1, rank)
            print("threshold %s %-26s rcond %-8s %.17g: state %d rank %2d (numpy on r: %2d, lands on %s) %s%s"
                  % (name, symbol, label, v, state, rank, want, pr.lands_on(d, rc), fig, "  text: " + text if state else ""))
            assert state in (0, 3), (name, symbol, label, state, text)
            assert rank == want, (name, symbol, label, "rank", rank, want)
            assert sw == sweeps and pl.same_bits(r1, r) and np.array_equal(p1, jpvt), (name, symbol, label, "rcond changed r, jpvt or the sweeps")
            if state == 3:
                met_3.append((symbol, label))
                assert text.startswith(symbol + ":") and "Cholesky" in text, (name, symbol, label, text)
                assert not x.any() and not np.isnan(x).any(), (name, symbol, label, "state 3 with a non-zero x")
                continue
            assert np.isfinite(x).all(), (name, symbol, label, "state 0 with an x that is not finite")
            if not mn:
                assert not x[jpvt[rank:]].any(), (name, symbol, label, "a dropped row of x is not zero")
            if rank == k_expected:
                assert fig.get("zero_rows", True) and fig["err"] <= fig["bound"], (name, symbol, label, fig)
        if want == n and xs[False] is not None and xs[True] is not None:
            assert pl.same_bits(xs[True], xs[False]), (name, label, "full rank: the minimum-norm x is not the basic x")
    print("threshold %s: %d values, %d land exactly (%s); state 3 met at %s" % (name, len(values), len(landed), landed, met_3 or "no value"))
    assert landed, (name, "no value of the list lands exactly on a pivot")


# ---- 3: the rank at every tile edge, on a matrix whose answer is known in closed form --------------------------------------------------------
def _block_case(bq, tag, n, nrhs, e, a, b, rcond, reorth, layouts):
    res = {mn: rank_call(bq, a, b, layouts[0], layouts[1], reorth, 1, rcond, mn) for mn, _ in ENTRIES}
    for mn, symbol in ENTRIES:
        st, sw, x, r, p, rank, text = res[mn]
        print("%s %-26s state %d sweeps %d rank %2d (expected %2d)%s" % (tag, symbol, st, sw, rank, pr.expected_rank(e, rcond, a.shape[0]),
                                                                        "  text: " + text if st else ""))
    st, sw, x, r, p, rank, _ = res[False]
    f = pr.check_block(e, a, b, rcond, st, sw, reorth, x, r, p, rank, x_minnorm=res[True][2])
    print("%s err %.3e floor %.3e" % (tag, f["err"], f["floor"]))
    assert _same_result(res[True], res[False], with_x=False), (tag, "the minimum-norm entry's state, r, jpvt, rank or sweeps")
    return f


@pytest.mark.parametrize("n,nrhs", pr.TILE_SHAPES)
def test_rank_at_every_tile_edge_in_closed_form(bq, n, nrhs):
    """pass_refs_f64_lsq_rank_scale.block_orthogonal: columns with disjoint supports, one +-1 pattern times 2^-e_j, e shuffled with
    ties, m = 16 n + 3; rcond = 2^-t puts the rank on 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63 and n, and every t but the last has a
    pivot exactly ON the threshold, which the strict inequality drops.  A^T A is exactly diagonal, so without assuming an exact square
    root anywhere: state 0; 1 sweep, 2 with reorth; jpvt = expected_jpvt(e) -- the lowest POSITION on a tie with the kernel's
    exchanges, which is NOT the stable argsort of e once an exchange has displaced a tied column (include/tsqr_mi.h says so now; the
    CPU file shows the difference on these very e); diag(R)[i] / diag(R)[0] == 2^-(e_jpvt[i] - min e) exactly; R exactly diagonal; the
    rank; exact zero rows in the dropped positions; rel_err(x[retained], closed form in longdouble) <= 4 n 2^-53; the minimum-norm x
    bitwise the basic x (Q1^T A P2 is an exact zero matrix, M = 0, C = I)."""
    e = pr.graded_e(n)
    a, b = pr.block_orthogonal(n, e, nrhs=nrhs)
    for i, (k, t, lands) in enumerate(pr.tile_grid(n)):
        tag = "tiles n %d nrhs %d t %2d k %2d (a pivot on the threshold: %s)" % (n, nrhs, t, k, lands)
        _block_case(bq, tag, n, nrhs, e, a, b, 2.0 ** -t, i % 2, PAIRS[(i + n) % 4])


def test_default_rcond_in_closed_form(bq):
    """the same matrix with m = 4097 rows and a span of 40: max(m, n) 2^-52 = 2^-40 (1 + 2^-12) drops the one pivot at 2^-40 of R_00,
    rank 63; max(m, n) 2^-53, or max(m, n) taken as n, would keep it"""
    n, nrhs, extra = pr.DEFAULT_SHAPE
    e = pr.graded_e(n, span=40)
    a, b = pr.block_orthogonal(n, e, extra_rows=extra, nrhs=nrhs)
    assert a.shape[0] == 4097 and pr.expected_rank(e, -1.0, 4097) == 63
    for reorth, layouts in ((0, (ROW, COL)), (1, (COL, ROW))):
        _block_case(bq, "default rcond 4097 x 64 reorth %d" % reorth, n, nrhs, e, a, b, -1.0, reorth, layouts)


# ---- 4: power-of-two scaling of A and B ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pk.CASES, ids=[c[0] for c in pk.CASES])
def test_uniform_scaling_of_a_and_columns_of_b_is_bitwise_covariant(bq, case):
    """A -> 2^k A for k in {-400, -1, 1, 401}, B -> B diag(2^j_c) with j_c in [-400, 400], both ends used, refine 0, 1 and 2, both
    entries, the case's own layouts, reorth and rcond (the default included): the state, the sweep count, the rank and jpvt of the
    unscaled call, R' = 2^k R and X' = 2^-k X diag(2^j_c), bit for bit -- the exact zero rows of the basic entry and every row of the
    minimum-norm one.  By the code: the rank rule is a ratio, Zeff scales exactly with R, A Zeff keeps its bits, M = T S12 is invariant.
    UNIFORM k only: a per-column scaling of A changes the column norms, hence legitimately the pivots, and is not covariant; the
    copied-column and tail cases sit on the ladder's shifted path, which follows a uniform scaling.  The unscaled refine = 1 result is
    held to check() of its entry; covariance carries that to the scaled calls."""
    name, m, n, nrhs, rcond, k_expected, a_row, b_row, reorth = case
    a, b = pk.case_matrix(name), pk.case_rhs(name, "gaussian")
    scaled = [(k, j, ps.scale_uniform(a, k), ps.scale_columns(b, j)) for k, j in pr.scale_pairs(name)]
    for refine in pr.SCALE_REFINES:
        for mn, symbol in ENTRIES:
            tag = "scaling %s %s refine %d" % (name, symbol, refine)
            st0, sw0, x0, r0, p0, k0, text = rank_call(bq, a, b, a_row, b_row, reorth, refine, rcond, mn)
            print("%s: state %d sweeps %d rank %d" % (tag, st0, sw0, k0))
            assert st0 == 0 and k0 == k_expected, (tag, st0, k0, text)
            if refine == 1:
                print("%s: %s" % (tag, (pm if mn else pk).check(name, "gaussian", x0, p0, k0)))
            for i, (k, j, ak, bj) in enumerate(scaled):
                lay = (a_row, b_row) if i % 2 == 0 else (1 - a_row, 1 - b_row)
                st, sw, x, r, p, kk, text = rank_call(bq, ak, bj, lay[0], lay[1], reorth, refine, rcond, mn)
                print("%s k %4d j %4d .. %4d: state %d sweeps %d rank %d" % (tag, k, j.min(), j.max(), st, sw, kk))
                assert (st, sw, kk) == (st0, sw0, k0) and np.array_equal(p, p0), (tag, k, st, sw, kk, text)
                assert pl.same_bits(r, np.ldexp(r0, k)), (tag, k, "R is not 2^k R")
                assert pl.same_bits(x, pl.scale_x(x0, k, j)), (tag, k, "X is not 2^-k X diag(2^j_c)")

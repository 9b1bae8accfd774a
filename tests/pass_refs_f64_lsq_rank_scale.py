"""Pure-numpy generators, exponents, expected values and measures for the tests of the two rank-aware fp64 least-squares entries
(tsqr_mi_lstsq_rank_f64, tsqr_mi_lstsq_minnorm_f64) at the threshold of the rank rule, at every edge of the 16-column tiles and under
power-of-two scaling (tests/test_gpu_f64_lstsq_rank_scale.py).  Built on tests/pass_refs_f64_lsq_rank.py (cases, rank_of, figures, the
model of the call), tests/pass_refs_f64_lsq.py (lstsq_ld, rel_err, floor_of, same_bits, scale_x, log2_span) and
tests/pass_refs_f64_scale.py (scale_uniform, UNIFORM_K); nothing of them is copied.  No GPU, no library, no torch:
tests/test_pass_refs_f64_lsq_rank_scale.py proves every precondition on the CPU and shows that each assertion catches a defect.

Three parts.
  threshold  the rcond values that sit on, just below and just above a pivot ratio R_jj / R_00 of a GIVEN R (the device's own, on
             purpose: the thing under test is the rule applied to R, not R), and a model of the front end's rule with its two defects;
  tiles      block_orthogonal: a matrix whose pivoted QR, rank and solution are known in closed form for every rcond = 2^-t, so that the
             rank can be put on every edge of the 16-column tiles;
  scaling    a numpy model of either entry with every intermediate, for the proof that A -> 2^k A, B -> B diag(2^j_c) keeps them inside
             [2^-1000, 2^1000] and that the model is bitwise covariant, with the two defects that break it."""
import functools

import numpy as np

from tests import pass_refs_f64 as p64
from tests import pass_refs_f64_lsq as pl
from tests import pass_refs_f64_lsq_minnorm as pm
from tests import pass_refs_f64_lsq_rank as pk
from tests import pass_refs_f64_lsq_rank_step as pst
from tests import pass_refs_f64_qrcp as pq
from tests import pass_refs_f64_scale as ps

U = pk.U
LD = pk.LD


def case_of(name):
    return next(c for c in pk.CASES if c[0] == name)


# ---- part 1: the C entry against the tensor call ---------------------------------------------------------------------------------------------
ENTRY_CASES = ("tail3_100x7", "full_300x17", "rank1_777x33", "copied_4096x16")

# ---- part 2: the rank rule at its threshold --------------------------------------------------------------------------------------------------
THRESHOLD_CASES = ("copied_4096x16", "rank32_1029x51", "rank40_4097x64", "tail3_100x7")


def default_rcond(m, n, defect=None):
    """what rcond < 0 stands for: max(m, n) 2^-52.  defect 'default_half': 2^-53"""
    return max(m, n) * (2.0 ** -53 if defect == "default_half" else 2.0 ** -52)


def entry_rank(r, rcond, m, n, defect=None):
    """the rank the entry reports for the R it computed: the front end's rule for a negative rcond, then lsq_rank_f64_kernel's count of
    the j with R_jj > fl(rcond R_00) -- one IEEE multiply and one compare.  defects: 'ge' counts R_jj >= rcond R_00; 'default_half'."""
    rc = default_rcond(m, n, defect) if rcond < 0 else rcond
    if defect == "ge":
        d = np.diag(np.asarray(r, np.float64))
        return int(np.sum(d >= rc * d[0]))
    return pk.rank_of(r, rc)


def threshold_indices(n, k_expected):
    """the pivots whose ratio the list brackets: 1, k_expected - 1, k_expected, n - 1 and two in between, inside 1 .. n - 1"""
    want = {1, k_expected - 1, k_expected, n - 1, n // 2, (k_expected + n) // 2, max(1, k_expected // 2)}
    return sorted(j for j in want if 1 <= j <= n - 1)


def lands_on(d, rc):
    """the indices j >= 1 with fl(rc d_0) == d_j > 0: the values at which > and >= part"""
    d = np.asarray(d, np.float64)
    return [int(j) for j in np.flatnonzero(d[1:] == rc * d[0]) + 1 if d[j] > 0]


def threshold_rconds(d, m, n, k_expected, rcond):
    """[(label, rcond)] for diag(R) = d: 0.0, -1.0 (the default), the case's own value, and for every j of threshold_indices with
    d_j > 0 the three doubles nextafter(q, 0), q, nextafter(q, 1) around q = fl(d_j / d_0) -- plus, where none of the three gives
    fl(rcond d_0) == d_j, the doubles within four ulps of q that do (fl(fl(d_j / d_0) d_0) need not return d_j).  Values at or above 1
    are left out: the entry rejects them."""
    d = np.asarray(d, np.float64)
    out = [("zero", 0.0), ("default", -1.0), ("case", -1.0 if rcond is None else float(rcond))]
    for j in threshold_indices(n, k_expected):
        if not d[j] > 0.0:
            continue
        q = d[j] / d[0]
        window = [q]
        for _ in range(4):
            window = [np.nextafter(window[0], 0.0)] + window + [np.nextafter(window[-1], 1.0)]
        for off, v in zip(range(-4, 5), window):
            near = abs(off) <= 1
            if (near or v * d[0] == d[j]) and 0.0 < v < 1.0:
                out.append(("j%d%+d" % (j, off), float(v)))
    return out


# ---- part 3: a matrix whose answer is known in closed form -----------------------------------------------------------------------------------
TILE_SHAPES = ((17, 1), (33, 5), (48, 16), (64, 16))       # (n, nrhs); m = 16 n + 3
TILE_RANKS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63)   # and n itself
E_OFFSET = 3                                                # min e: the expected values subtract it
DEFAULT_SHAPE = (64, 5, 3073)                               # (n, nrhs, extra_rows): m = 4097, so that max(m, n) 2^-52 = 2^-40 (1 + 2^-12)


def graded_e(n, span=None):
    """n integers e_j >= E_OFFSET in shuffled order.  Sorted, e rises by one at every odd position and at every multiple of 16 and
    stays where it is elsewhere: pairs of equal values (ties), and a strict rise at every k of TILE_RANKS, so that rcond = 2^-t can put
    the rank on each of them.  The span max e - min e is n // 2 + (n - 1) // 16 <= 35.  span: further rises at the even positions
    2, 4, .. until the span is that value (the case of the default rcond needs 40)."""
    rise = np.array([i % 2 == 1 or i % 16 == 0 for i in range(n)])
    rise[0] = False
    if span is not None:
        for i in range(2, n, 2):
            if rise.sum() >= span:
                break
            rise[i] = True
        assert rise.sum() == span, (n, span)
    v = np.cumsum(rise) + E_OFFSET
    assert v.max() - v.min() <= 40 and (n < 3 or len(set(v.tolist())) < n), "the span, or no tie"
    rng = np.random.default_rng(5000 + n)
    return v[rng.permutation(n)].astype(np.int64)


@functools.lru_cache(maxsize=None)
def _pattern(s):
    return np.where(np.random.default_rng(91).integers(0, 2, size=s) == 1, 1.0, -1.0)


def block_orthogonal(n, e, s=16, extra_rows=3, nrhs=1):
    """(A, B), read-only.  A has m = s n + extra_rows rows; column j is non-zero in rows s j .. s j + s - 1 only, where it holds one
    fixed +-1 pattern (the same for every column) times 2^-e_j; the extra rows are zero.  B: integers in [-3, 3].  A^T A is exactly
    diagonal, s 4^-e_j, and every product and partial sum of a Gram pass over A is exact."""
    e = np.asarray(e, np.int64)
    assert e.shape == (n,) and e.min() >= 0 and e.max() - e.min() <= 40
    m = s * n + extra_rows
    a = np.zeros((m, n))
    for j in range(n):
        a[s * j:s * j + s, j] = np.ldexp(_pattern(s), -int(e[j]))
    b = np.random.default_rng(7 * n + nrhs).integers(-3, 4, size=(m, nrhs)).astype(np.float64)
    return pl._frozen(a), pl._frozen(b)


def expected_jpvt(e):
    """the pivots of qrcp_r_f64_kernel on columns of norms 2^-e_j that are orthogonal: step k takes the largest remaining norm, the lowest
    POSITION on a tie, and EXCHANGES the columns at positions k and p.  With ties this is not the stable argsort of e: the exchange
    moves the column that stood at k behind columns it used to precede (e = (1, 1, 0) gives (2, 1, 0), the argsort (2, 0, 1)).  A pure
    function of the integers e."""
    e = [int(v) for v in e]
    pos = list(range(len(e)))
    for k in range(len(e)):
        rest = [e[pos[i]] for i in range(k, len(e))]
        p = k + rest.index(min(rest))
        pos[k], pos[p] = pos[p], pos[k]
    return np.array(pos, np.int64)


def expected_rank(e, rcond, m=None):
    """#{j : 2^-(e_j - min e) > rcond}, rcond < 0 standing for max(m, n) 2^-52: exact, because diag(R) / R_00 is exactly 2^-(e_j - min e)
    and fl(rcond R_00) is rcond R_00 for a power of two (for the default it lies a factor 1 + 2^-12 above a power of two at
    DEFAULT_SHAPE, far from every ratio on the scale of a rounding)"""
    e = np.asarray(e, np.int64)
    rc = default_rcond(m, len(e)) if rcond < 0 else rcond
    return int(np.sum(np.ldexp(1.0, -(e - e.min()).astype(np.int32)) > rc))


def rcond_for_rank(e, k):
    """(t, lands): rcond = 2^-t gives rank k -- t = the (k + 1)-th smallest e_j - min e, a pivot exactly ON the threshold that the strict
    inequality drops (lands True), or one more than the largest for k = n"""
    v = np.sort(np.asarray(e, np.int64) - int(np.min(e)))
    if k == len(v):
        return int(v[-1]) + 1, False
    assert v[k - 1] < v[k], ("no rcond gives this rank", k)
    return int(v[k]), True


def tile_grid(n):
    """[(k, t, lands)] of a shape: every k of TILE_RANKS below n, and n"""
    e = graded_e(n)
    return [(k,) + rcond_for_rank(e, k) for k in TILE_RANKS if k < n] + [(n,) + rcond_for_rank(e, n)]


def closed_form_x(a, b, e, k, jpvt):
    """X in longdouble: row j = (a_j . b) / (a_j . a_j) for the retained columns jpvt[:k], zero for the others"""
    p64.require_longdouble()
    al, bl = np.asarray(a, LD), np.asarray(b, LD)
    x = np.zeros((a.shape[1], b.shape[1]), LD)
    for j in np.asarray(jpvt)[:k]:
        x[j] = (al[:, j] @ bl) / (al[:, j] @ al[:, j])
    return x


def check_block(e, a, b, rcond, state, sweeps, reorth, x, r, jpvt, rank, x_minnorm=None):
    """every assertion of part 3 on one result; returns {err, floor, rank}.  x_minnorm: the minimum-norm entry's X of the same call,
    which must be x bit for bit (Q1^T A P2 is an exact zero matrix: M = 0, C = I)."""
    e = np.asarray(e, np.int64)
    n = len(e)
    x, r, jpvt = np.asarray(x, np.float64), np.asarray(r, np.float64), np.asarray(jpvt)
    assert state == 0, ("state", state)
    assert sweeps == (2 if reorth else 1), ("sweeps", sweeps)
    want_p = expected_jpvt(e)
    assert np.array_equal(jpvt, want_p), ("jpvt", jpvt.tolist(), want_p.tolist())
    d = np.diag(r)
    assert d[0] > 0 and np.array_equal(d, np.ldexp(d[0], -(e[want_p] - e.min()).astype(np.int32))), ("the ratios of diag(R)", d / d[0])
    assert not (r - np.diag(d)).any(), "R is not exactly diagonal"
    k = expected_rank(e, rcond, a.shape[0])
    assert rank == k, ("rank", rank, k)
    assert not x[want_p[k:]].any(), "a dropped row of X is not zero"
    ref = closed_form_x(a, b, e, k, want_p)
    err, floor = pl.rel_err(x[want_p[:k]], ref[want_p[:k]]), pl.floor_of(n)
    assert err <= floor, ("the retained rows of X", err, floor)
    if x_minnorm is not None:
        assert pl.same_bits(x_minnorm, x), "the minimum-norm X is not the basic X"
    return {"err": err, "floor": floor, "rank": k}


def block_r0(a, reorth=0):
    """the ladder's R0 on a block-orthogonal A as tests/pass_refs_f64.model_chol computes it from the exact diagonal Gram matrix: one
    sweep, two with reorth (the second on Q = A Z, whose Gram matrix is diagonal again)"""
    r0, z = p64.model_chol(a.T @ a)
    if reorth:
        q = a @ z
        r2, _ = p64.model_chol(np.diag(np.diag(q.T @ q)))
        r0 = r2 @ r0
    return r0


# ---- part 4: power-of-two scaling ------------------------------------------------------------------------------------------------------------
SCALE_K = ps.UNIFORM_K
SCALE_REFINES = (0, 1, 2)
B_SPAN = 400
RANGE_LOG2 = pl.RANGE_LOG2


def b_exponents(name, flip=False):
    """j_c of B -> B diag(2^j_c) for a case: integers in [-B_SPAN, B_SPAN] with both ends (one column: -B_SPAN); flip: the negated set,
    so that a case with one right-hand side meets both ends too"""
    nrhs = case_of(name)[3]
    j = ps.graded_exponents(np.random.default_rng(sum(ord(c) for c in name) + 31), nrhs, B_SPAN)
    return -j if flip else j


def scale_pairs(name):
    """[(k, j_c)] of a case: every k of SCALE_K, the exponents of B alternating with their negation"""
    return [(k, b_exponents(name, flip=i % 2 == 1)) for i, k in enumerate(SCALE_K)]


def model_trace(a, b, rcond, refine, minimum_norm, defect=None):
    """fp64 model of either entry with its intermediates: pass_refs_f64_lsq_rank_step.model_lstsq_rank_step (basic) or
    pass_refs_f64_lsq_minnorm.model_lstsq_minnorm (minimum norm), operation for operation, on Householder's R0.  Returns
    (X, R, p, rank, {name: array}): R0, the threshold rcond R_00, Zeff before the step, G1, Rc, Zeff behind it, and for the minimum-norm
    form G12, S12, M, C, Zmn; the residual, D and X of every pass.  defects: 'zg_scaled' -- the unit entries of Zg are R_00, a number that
    scales with A, in place of 1; 'float_d' -- D is narrowed to float before it is used."""
    m, n = a.shape
    tr = {}
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        r0 = pl.householder_r(a)
        r, _, p = pq.householder_qrcp(r0, dtype=np.float64)
        p = np.asarray(p)
        rc = default_rcond(m, n) if rcond is None or rcond < 0 else rcond
        k = pk.rank_of(r, rc)
        z0 = pk.zeff_of(r, p, k)
        tr.update(R0=r0, R=r, threshold=np.array([[rc * r[0, 0]]]), Zeff0=z0)
        zg = z0
        if minimum_norm:
            zg = pm.zg_of(z0, p, k)
            if defect == "zg_scaled":
                zg[p[k:], np.arange(k, n)] = r[0, 0]
        q = a @ zg
        g = q.T @ q
        z, verdict = pst.step_of(z0, g, k)
        assert verdict == 0, "the Cholesky step of the model met a bad pivot"
        tr.update(G1=g[:k, :k], Rc=pst.chol_upper(g[:k, :k]), Zeff=z)
        zupd = z
        if minimum_norm:
            zupd, verdict = pm.zmn_of(g, z, p, k)
            assert verdict == 0, "the Cholesky factorisation of C in the model met a bad pivot"
            _, s12 = pm.s12_of(g, k)
            mm = np.triu(z[p[:k], :k]) @ s12
            tr.update(G12=g[:k, k:], S12=s12, M=mm, C=np.eye(k) + mm @ mm.T, Zmn=zupd)
        q = a @ z
        x, state = None, None
        for t in range(refine + 1):
            res = b if x is None else b - a @ x
            d = q.T @ res
            if defect == "float_d":
                d = d.astype(np.float32).astype(np.float64)
            x, state = pl.stagnation_step(x, zupd @ d, d, state, t)
            tr["residual%d" % t], tr["D%d" % t], tr["X%d" % t] = res, d, x
    return x, r, p, k, tr


# how every intermediate scales under A -> 2^k A, B -> B diag(2^j_c): (power of 2^k on every entry, whether the columns carry 2^j_c)
SCALING_OF = {"R0": (1, 0), "R": (1, 0), "threshold": (1, 0), "Zeff0": (-1, 0), "G1": (0, 0), "Rc": (0, 0), "Zeff": (-1, 0),
              "G12": (1, 0), "S12": (1, 0), "M": (0, 0), "C": (0, 0), "Zmn": (-1, 0), "residual": (0, 1), "D": (0, 1), "X": (-1, 1)}


def scaled_spans(tr, k, j):
    """{name: (lowest, highest) log2 of the non-zero magnitudes} of every intermediate of the call on 2^k A and B diag(2^j), from the
    trace of the unscaled model (pass_refs_f64_lsq.log2_span: in longdouble, nothing can leave its range)"""
    out = {}
    for name, v in tr.items():
        pk_, pj = SCALING_OF[name if name in SCALING_OF else name.rstrip("0123456789")]      # (residual0, D1, X2: one per pass)
        if np.size(v) == 0:                                  # (G12, S12 at full rank)
            continue
        v = np.asarray(v, np.float64).reshape(v.shape[0], -1)
        out[name] = pl.log2_span(v, row_exp=pk_ * k, col_exp=j if pj else 0)
    return out


def covariant(base, scaled, k, j):
    """the asserted property on (X, R, p, rank) of the unscaled and of the scaled call: the same rank and pivots, R' = 2^k R and
    X' = 2^-k X diag(2^j_c), bit for bit"""
    x0, r0, p0, k0 = base[:4]
    x1, r1, p1, k1 = scaled[:4]
    return (k0 == k1 and np.array_equal(np.asarray(p0), np.asarray(p1)) and pl.same_bits(r1, np.ldexp(r0, k))
            and pl.same_bits(x1, pl.scale_x(x0, k, j)))

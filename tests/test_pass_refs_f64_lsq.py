"""CPU checks of tests/pass_refs_f64_lsq.py: the exact reference of the least-squares pass agrees with a model of the pass, every seeded
defect of the model is caught by the comparison the GPU tests make, and the numpy model of the whole call passes the accuracy check of
tests/test_gpu_f64_lstsq.py on that test's own inputs -- the algorithm itself can meet what the entry is asked to meet.  Every accuracy
case prints its figures (profiles/fp64_lstsq_accuracy.md records them)."""
import functools

import numpy as np
import pytest

from tests import pass_refs_f64_lsq as pl


@pytest.mark.parametrize("m,n,nrhs", [(1, 1, 1), (17, 17, 5), (100, 33, 16), (4099, 64, 16)])
def test_model_matches_exact_reference(m, n, nrhs):
    a, z, x, b = pl.exact_case(np.random.default_rng(m + n + nrhs), m, n, nrhs)
    want = pl.pack_d(pl.d_exact(a, z, x, b), n)
    assert np.array_equal(pl.model_pass(a, z, x, b), want)
    d = pl.unpack_d(want, n)
    assert np.array_equal(d[:n, :nrhs], pl.d_exact(a, z, x, b)) and not d[n:].any() and not d[:, nrhs:].any()
    assert np.array_equal(pl.model_pass(a, z, np.zeros_like(x), b), pl.pack_d(pl.d_exact(a, z, None, b), n))


@pytest.mark.parametrize("defect", ["x_sign", "drop_tail_row", "swap_ti"])
@pytest.mark.parametrize("m,n,nrhs", [(33, 17, 1), (100, 64, 16)])
def test_exact_check_bites(m, n, nrhs, defect):
    a, z, x, b = pl.exact_case(np.random.default_rng(7 * m + n), m, n, nrhs)
    want = pl.pack_d(pl.d_exact(a, z, x, b), n)
    assert not np.array_equal(pl.model_pass(a, z, x, b, defect), want)


def test_layouts():
    x = np.arange(1.0, 7.0).reshape(3, 2)
    v = pl.pad_x(x, 3)
    assert v.shape == (256,) and v[0] == 1.0 and v[16 + 2] == 6.0 and v[2 * 16] == 0.0
    assert np.array_equal(pl.unpad_x(v, 3)[:3, :2], x)
    d = np.arange(1.0, 1.0 + 17 * 2).reshape(17, 2)
    w = pl.pack_d(d, 17)
    # D[5][1]: tile 0, row 5 = lq 1 + 4 * reg 1, lane 16 * 1 + 1;  D[16][0]: tile 1, register 0, lane 0
    assert w.shape == (512,) and w[(0 * 4 + 1) * 64 + 17] == d[5, 1] and w[256] == d[16, 0]
    assert np.array_equal(pl.unpack_d(w, 17)[:17, :2], d)


def test_explicit_inverse_and_reference_solve():
    rng = np.random.default_rng(2)
    a, b = rng.standard_normal((300, 9)), rng.standard_normal((300, 4))
    r = pl.householder_r(a)
    assert np.all(np.diag(r) > 0) and np.abs(pl.explicit_inverse(r) @ r - np.eye(9)).max() < 1e-13
    x = pl.lstsq_ld(a, b)
    assert pl.normal_residual(a, b, x) < 1e-17                   # (longdouble: far below fp64 rounding)
    assert pl.rel_err(np.linalg.lstsq(a, b, rcond=None)[0], x) < 1e-14


@functools.lru_cache(maxsize=None)
def model_figures(case):
    """(error of refine 0, 1, 2, error of numpy's lstsq), all against the longdouble Householder solve"""
    _, m, n, nrhs, cond, kind = case
    a, b = pl.accuracy_input(m, n, nrhs, cond, kind)
    ref = pl.lstsq_ld(a, b)
    errs = [pl.rel_err(pl.model_lstsq(a, b, k)[0], ref) for k in (0, 1, 2)]
    return errs, pl.rel_err(np.linalg.lstsq(a, b, rcond=None)[0], ref)


# the factor of the GPU test's assertion (tests/test_gpu_f64_lstsq.py says how it was fixed); the model's largest ratio is 0.62
# (profiles/fp64_lstsq_accuracy.md)
MODEL_FACTOR = 2.0


@pytest.mark.parametrize("case", pl.accuracy_cases(), ids=lambda c: c[0])
def test_model_meets_the_accuracy_check(case):
    (e0, e1, e2), lapack = model_figures(case)
    n = case[2]
    print("model %-32s refine 0 %.3e  1 %.3e  2 %.3e  lapack %.3e  ratio(refine 1) %.3g  floor %.3e"
          % (case[0], e0, e1, e2, lapack, e1 / lapack if lapack > 0 else float(e1 > 0), pl.floor_of(n)))
    assert e1 <= max(MODEL_FACTOR * lapack, pl.floor_of(n))
    assert e2 <= 2.0 * max(e1, pl.floor_of(n))


def test_accuracy_check_bites():
    """a correction formed from B + A X doubles the error instead of removing it: far outside the band"""
    case = [c for c in pl.accuracy_cases() if c[0].startswith("cond1e+04") and c[5] == "gaussian"][0]
    _, m, n, nrhs, cond, kind = case
    a, b = pl.accuracy_input(m, n, nrhs, cond, kind)
    ref = pl.lstsq_ld(a, b)
    lapack = pl.rel_err(np.linalg.lstsq(a, b, rcond=None)[0], ref)
    bad = pl.rel_err(pl.model_lstsq(a, b, 1, defect="x_sign")[0], ref)
    assert bad > 64.0 * max(lapack, pl.floor_of(n))

"""The NumPy model of the fp64 block orthogonalisation (tests/pass_refs_f64_orth.py) against the bounds the GPU tests use: with two rounds
the reference alone meets them on every case, and with one round it misses the ||V^T Q||_F bound on the near-span cases -- so the bound
tells one round from two."""
import numpy as np
import pytest

from tests import pass_refs_f64_orth as po


@pytest.mark.parametrize("case", list(po.CASES))
def test_model_with_two_rounds_is_inside_the_bounds(case):
    vq, qtq, res = po.model_figures(case, 2)
    print("%s: ||V^T Q|| %.2e (floor %.2e)  ||Q^T Q - I|| %.2e  residual %.2e" % (case, vq, po.vq_floor(case), qtq, res))
    assert vq <= po.vq_floor(case)
    assert qtq <= po.QTQ_BOUND
    assert res <= po.RESID_BOUND
    assert po.vq_bound(case) == max(2.0 * vq, po.vq_floor(case))


@pytest.mark.parametrize("case", po.NEAR_SPAN)
def test_model_with_one_round_misses_the_bound_near_the_span(case):
    vq = po.model_figures(case, 1)[0]
    print("%s: one round leaves ||V^T Q|| = %.2e, bound %.2e" % (case, vq, po.vq_bound(case)))
    assert vq > po.vq_bound(case)


def test_model_factors_and_signs():
    v, w = po.make("1003x130x17")
    q, s, r = po.model(v, w, 2)
    assert s.shape == (130, 17) and r.shape == (17, 17)
    assert np.all(np.diag(r) >= 0.0) and np.all(np.tril(r, -1) == 0.0)
    q1, s1, r1 = po.model(v, w, 1)
    assert np.all(np.diag(r1) >= 0.0)
    assert np.allclose(s, s1, rtol=0, atol=1e-12 * np.abs(s1).max())


def test_cases_are_what_they_claim():
    for case, (m, k, n, eps, cond, _) in po.CASES.items():
        v, w = po.make(case)
        assert v.shape == (m, k) and w.shape == (m, n) and k + n <= m and 1 <= n <= 64 and 1 <= k <= 1024
        assert np.linalg.norm(v.T @ v - np.eye(k)) < 1e-12
        assert not v.flags.writeable and not w.flags.writeable
    g = po.with_cond(np.random.default_rng(0), 200, 17, 1e8)
    sv = np.linalg.svd(g, compute_uv=False)
    assert abs(sv[0] / sv[-1] / 1e8 - 1.0) < 1e-6
    assert po.TABLE == list(po.CASES)[:7] and "4096x1024x64-caps" in po.NEAR_SPAN

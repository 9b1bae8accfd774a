"""CPU checks of tests/pass_refs_f64_r.py: the exact references of the R-only entry's pass tests agree with a model of the pass, and every
seeded defect of the model is caught by the comparison the GPU tests make -- the yardstick can fail."""
import numpy as np
import pytest

from tests import pass_refs as pr
from tests import pass_refs_f64 as p64
from tests import pass_refs_f64_r as p64r


@pytest.mark.parametrize("m,n", [(1, 1), (17, 17), (100, 33), (4099, 64)])
def test_model_matches_exact_reference(m, n):
    a, z = p64r.exact_pair(np.random.default_rng(m + n), m, n)
    want = pr.pack_tiles(p64r.gramq_exact(a, z), n, False)
    assert np.array_equal(p64r.model_gramq(a, z), want)
    g = pr.unpack_tiles(want, n, False)
    assert np.array_equal(g[:n, :n], p64r.gramq_exact(a, z)) and p64.padding_is_zero(g, n)


@pytest.mark.parametrize("defect", ["drop_tile", "transposed_tile", "stale_z"])
@pytest.mark.parametrize("m,n", [(33, 17), (100, 64)])
def test_exact_check_bites(m, n, defect):
    a, z = p64r.exact_pair(np.random.default_rng(7 * m + n), m, n)
    want = pr.pack_tiles(p64r.gramq_exact(a, z), n, False)
    assert not np.array_equal(p64r.model_gramq(a, z, defect), want)


def test_dense_bound_holds_for_the_model_and_bites():
    """the fp64 model stays inside gramq_bound against longdouble; a dropped row tile and a Q rounded to fp32 do not"""
    rng = np.random.default_rng(3)
    m, n = 1000, 7
    a, z = rng.standard_normal((m, n)), p64r.mixed_triangular(rng, n)
    ref = np.asarray(p64r.gramq_ld(a, z), np.float64)
    ref_ld = p64r.gramq_ld(a, z)
    bound = p64r.gramq_bound(a, z)
    good = pr.unpack_tiles(p64r.model_gramq(a, z), n, False)[:n, :n]
    assert np.all(np.abs(np.asarray(good.astype(p64.LD) - ref_ld, np.float64)) <= bound)
    bad = pr.unpack_tiles(p64r.model_gramq(a, z, "drop_tile"), n, False)[:n, :n]
    assert np.any(np.abs(bad - ref) > bound)
    q32 = (a @ z).astype(np.float32).astype(np.float64)
    assert np.any(np.abs(q32.T @ q32 - ref) > bound)


def test_pad_z_layout():
    z = np.triu(np.arange(1.0, 10.0).reshape(3, 3))
    v = p64r.pad_z(z, 3)
    assert v.shape == (256,) and v[0 * 16 + 0] == 1.0 and v[2 * 16 + 1] == 6.0 and v[1 * 16 + 2] == 0.0
    assert np.array_equal(p64r.unpad_z(v, 3)[:3, :3], z)


def test_measures_of_r():
    """orth_of_r and gram_residual_of_r on Householder's R are at the level of fp64 rounding; a perturbed R is far off"""
    a = p64r.cond_matrix(300, 9, 1e4, 1)
    r = np.linalg.qr(a, mode="r")
    r *= np.sign(np.diag(r))[:, None]
    ata = p64r.gram_ld(a)
    assert p64r.orth_of_r(a, r) < 1e-11 and p64r.gram_residual_of_r(ata, r) < 1e-14
    r2 = r.copy()
    r2[0, 5] *= 1.0 + 1e-6
    assert p64r.orth_of_r(a, r2) > 1e-9 and p64r.gram_residual_of_r(ata, r2) > 1e-10

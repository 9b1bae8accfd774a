"""The fp64 entry (tsqr_mi_qr_f64) on the GPU: the bands of include/tsqr_mi.h, the sweep counts of the ladder, padded leading
dimensions with NaN guard bands, in place against out of place, determinism, and non-finite input.  References are numpy's
LAPACK (fp64) on the host; conditioned matrices are built on the host in fp64."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53


def _torch():
    import torch
    return torch


def _padded(a_host, ld, dev="cuda"):
    """column-major m x n copy of a_host inside an (n, ld) float64 tensor whose padding rows are NaN"""
    torch = _torch()
    m, n = a_host.shape
    t = torch.full((n, ld), float("nan"), dtype=torch.float64, device=dev)
    t[:, :m] = torch.from_numpy(np.ascontiguousarray(a_host.T)).to(dev)
    return t


def _run(bq, a_host, reorth, pad=(3, 5, 2), a_dev=None):
    """factor a_host (m x n) with lda = m + pad[0], ldq = m + pad[1], ldr = n + pad[2]; returns state, Q, R (host), the raw tensors"""
    torch = _torch()
    m, n = a_host.shape
    lda, ldq, ldr = m + pad[0], m + pad[1], n + pad[2]
    a = _padded(a_host, lda) if a_dev is None else a_dev
    q = torch.full((n, ldq), float("nan"), dtype=torch.float64, device="cuda")
    r = torch.full((n, ldr), float("nan"), dtype=torch.float64, device="cuda")
    bf = bq.buffer_f64(reorth)
    bf.allocate(m, n)
    st = bq.qr_f64(q, ldq, r, ldr, a, lda, m, n, bf)
    torch.cuda.synchronize()
    return st, q, r, a


def _check(bq, a_host, q, r, reorth, cond):
    """bands of include/tsqr_mi.h, R's shape, guard bands, agreement with LAPACK's R"""
    torch = _torch()
    m, n = a_host.shape
    ldq, ldr = q.shape[1], r.shape[1]
    assert torch.isnan(q[:, m:]).all(), "Q's padding rows were written"
    assert torch.isnan(r[:, n:]).all(), "R's padding rows were written"
    Q = q[:, :m].T                                        # device, m x n
    R = r[:, :n].T.cpu().numpy()
    assert np.all(np.tril(R, -1) == 0.0), "R has non-zeros below the diagonal"
    assert np.all(np.diag(R) > 0.0), "R's diagonal is not positive"
    I = torch.eye(n, dtype=torch.float64, device="cuda")
    orth = torch.linalg.norm(Q.T @ Q - I).item()
    A = torch.from_numpy(a_host).cuda()
    res = (torch.linalg.norm(A - Q @ torch.from_numpy(R).cuda()) / torch.linalg.norm(A)).item()
    assert orth <= (1e-12 if reorth else 1e-11), ("orthogonality", orth)
    assert res <= 1e-13, ("residual", res)
    r_lp = np.linalg.qr(a_host, mode="r")
    r_lp = np.sign(np.diag(r_lp))[:, None] * r_lp
    dr = np.linalg.norm(R - r_lp) / np.linalg.norm(R)
    assert dr <= 50 * n * U53 * cond, ("R against LAPACK", dr, cond)
    return orth, res


def _cond_matrix(m, n, cond, seed):
    rng = np.random.default_rng(seed)
    u, _ = np.linalg.qr(rng.standard_normal((m, n)))
    v, _ = np.linalg.qr(rng.standard_normal((n, n)))
    s = np.logspace(0.0, -np.log10(cond), n)
    return (u * s) @ v.T


@pytest.mark.parametrize("m,n", [(64, 1), (100, 7), (4096, 16), (9211, 51), (65536, 64), (1 << 20, 64)])
@pytest.mark.parametrize("reorth", [0, 1])
def test_f64_shapes(bq, m, n, reorth):
    a_host = np.random.default_rng(m + n).standard_normal((m, n))
    st, q, r, _ = _run(bq, a_host, reorth)
    assert st == 0, (st, bq.last_error())
    cond = np.linalg.cond(a_host) if m * n <= 1 << 22 else 1.1
    _check(bq, a_host, q, r, reorth, cond)
    sweeps = bq.last_sweeps_f64()
    if reorth:
        assert sweeps == 2, sweeps
    else:
        assert sweeps == 1, sweeps                         # Gaussian tall-skinny: cond(A) < 10, one sweep


@pytest.mark.parametrize("m", [4096, 65536])
@pytest.mark.parametrize("cond", [1.0, 1e3, 1e8, 1e12])
@pytest.mark.parametrize("reorth", [0, 1])
def test_f64_conditioning(bq, m, cond, reorth):
    n = 64
    a_host = _cond_matrix(m, n, cond, seed=int(np.log10(cond)) + m)
    st, q, r, _ = _run(bq, a_host, reorth)
    assert st == 0, (st, bq.last_error())
    orth, res = _check(bq, a_host, q, r, reorth, cond)
    sweeps = bq.last_sweeps_f64()
    print("m %d cond %.0e reorth %d: sweeps %d  ||QtQ-I||_F %.2e  residual %.2e" % (m, cond, reorth, sweeps, orth, res))
    if cond == 1.0 and not reorth:
        assert sweeps == 1
    if reorth:
        assert sweeps % 100 >= 2
    if cond == 1e12:
        assert sweeps >= 100, sweeps


def test_f64_in_place_and_determinism(bq):
    torch = _torch()
    m, n = 9211, 51
    a_host = _cond_matrix(m, n, 1e6, seed=5)
    for reorth in (0, 1):
        st, q1, r1, a = _run(bq, a_host, reorth)
        assert st == 0
        a_before = _padded(a_host, a.shape[1])
        assert torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(a_before, nan=7.0)), "A was modified out of place"
        st, q2, r2, _ = _run(bq, a_host, reorth)
        assert st == 0
        assert torch.equal(q1[:, :m], q2[:, :m]) and torch.equal(r1[:, :n], r2[:, :n]), "two calls differ"
        # in place: q == a, ldq == lda
        lda = m + 3
        a_in = _padded(a_host, lda)
        r3 = torch.full((n, n + 2), float("nan"), dtype=torch.float64, device="cuda")
        bf = bq.buffer_f64(reorth)
        bf.allocate(m, n)
        st = bq.qr_f64(a_in, lda, r3, n + 2, a_in, lda, m, n, bf)
        torch.cuda.synchronize()
        assert st == 0
        assert torch.equal(a_in[:, :m], q1[:, :m]), "in place differs from out of place"
        assert torch.isnan(a_in[:, m:]).all()
        assert torch.equal(r3[:, :n], r1[:, :n])


def test_f64_non_finite(bq):
    m, n = 4096, 16
    a_host = np.random.default_rng(3).standard_normal((m, n))
    bad = a_host.copy()
    bad[1000, 5] = np.nan
    st, _, _, _ = _run(bq, bad, 0)
    assert st == bq.error_not_finite == 3
    bad[1000, 5] = np.inf
    st, _, _, _ = _run(bq, bad, 1)
    assert st == 3
    st, q, r, _ = _run(bq, a_host, 0)
    assert st == 0
    _check(bq, a_host, q, r, 0, np.linalg.cond(a_host))


# ---- the ladder: S_ref prescribed on both sides of both thresholds of the acceptance rule -------------------------------------------------
@pytest.mark.parametrize("n", [16, 64])
def test_f64_ladder_sweep_counts(bq, n):
    """A with S_ref = mean(1 / sigma_i(A D^-1)^2) at alone_max / 2, 2 alone_max, max_scond / 4 and 4 max_scond (thresholds from
    CholArgs64's formulas and the shape, pass_refs_f64.rule; the margins 2 and 4 are conditions: at the CholeskyQR2 bound S moves by
    about 1/64 with the rounding of G; tests/test_pass_refs_f64.py checks on the CPU that every matrix lands on its side): the sweep
    count exactly -- 1, 2, 2, 103 (reorth = 1: 2, 2, 2, 103) -- and the bands of the header.  Where the first sweep ends the call the
    measured ||QtQ-I||_F is printed next to the rule's estimate 4 n S u."""
    from tests import pass_refs_f64 as p64
    m = 4096
    for name, target, s0, s1 in p64.ladder_targets(m, n):
        a_host, s_ref = p64.ladder_matrix(m, n, target, n)
        cond = np.linalg.cond(a_host)
        for reorth, want in ((0, s0), (1, s1)):
            st, q, r, _ = _run(bq, a_host, reorth)
            assert st == 0, (st, bq.last_error())
            sweeps = bq.last_sweeps_f64()
            orth, res = _check(bq, a_host, q, r, reorth, cond)
            print("ladder %d x %d  S_ref = %s = %.4g  reorth %d: sweeps %d  ||QtQ-I||_F %.2e  residual %.2e%s" % (
                m, n, name, s_ref, reorth, sweeps, orth, res,
                "  one-sweep estimate 4nSu %.2e" % (4 * n * s_ref * U53) if sweeps == 1 else ""))
            assert sweeps == want, (name, reorth, sweeps, want)


def test_f64_limit_2p23_x_64_in_place(bq):
    """the documented limit m = 2^23 at n = 64, in place, Gaussian data generated on the device: the bands of the header"""
    torch = _torch()
    m, n = 1 << 23, 64
    g = torch.Generator(device="cuda").manual_seed(23)
    a0 = torch.randn(n, m, dtype=torch.float64, device="cuda", generator=g)      # column-major m x n, lda = m
    a = a0.clone()
    r = torch.full((n, n + 2), float("nan"), dtype=torch.float64, device="cuda")
    for reorth in (0, 1):
        a.copy_(a0)
        bf = bq.buffer_f64(reorth)
        bf.allocate(m, n)
        st = bq.qr_f64(a, m, r, n + 2, a, m, m, n, bf)
        torch.cuda.synchronize()
        assert st == 0, (st, bq.last_error())
        rt = r[:, :n]                                                             # R^T
        orth = torch.linalg.norm(a @ a.T - torch.eye(n, dtype=torch.float64, device="cuda")).item()
        res = (torch.linalg.norm(a0 - rt @ a) / torch.linalg.norm(a0)).item()
        print("2^23 x 64 in place reorth %d: sweeps %d  ||QtQ-I||_F %.2e  residual %.2e" % (reorth, bq.last_sweeps_f64(), orth, res))
        assert torch.isnan(r[:, n:]).all() and torch.all(torch.triu(rt, 1) == 0) and torch.all(torch.diagonal(rt) > 0)   # (rt is R^T)
        assert orth <= (1e-12 if reorth else 1e-11) and res <= 1e-13

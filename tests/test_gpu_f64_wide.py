"""The wide fp64 entry (tsqr_mi_qr_f64_wide, 64 < n <= 1024) on the GPU: the bands of include/tsqr_mi.h, the sweep counts of the ladder,
ragged last column blocks, padded leading dimensions with NaN guard bands, the one-panel path against qr_f64 bit for bit, in place
against out of place, determinism, and non-finite input.  References: numpy's LAPACK R (fp64) on the host; conditioned matrices are
built on the GPU with torch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53


def _torch():
    import torch
    return torch


def _padded(a_dev, ld):
    """column-major m x n copy of the (m, n) device tensor a_dev inside an (n, ld) float64 tensor whose padding rows are NaN"""
    torch = _torch()
    m, n = a_dev.shape
    t = torch.full((n, ld), float("nan"), dtype=torch.float64, device="cuda")
    t[:, :m] = a_dev.T
    return t


def _run(bq, a_dev, reorth, pad=(3, 5, 2), entry=None, bf=None):
    """factor a_dev (m x n, device) with lda = m + pad[0], ldq = m + pad[1], ldr = n + pad[2]; returns state, q, r, a (raw tensors)"""
    torch = _torch()
    m, n = a_dev.shape
    lda, ldq, ldr = m + pad[0], m + pad[1], n + pad[2]
    a = _padded(a_dev, lda)
    q = torch.full((n, ldq), float("nan"), dtype=torch.float64, device="cuda")
    r = torch.full((n, ldr), float("nan"), dtype=torch.float64, device="cuda")
    if bf is None:
        bf = bq.buffer_f64_wide(reorth)
        bf.allocate(m, n)
    st = (entry or bq.qr_f64_wide)(q, ldq, r, ldr, a, lda, m, n, bf, reorthogonalize=reorth)
    torch.cuda.synchronize()
    return st, q, r, a


def _gauss(m, n, seed):
    torch = _torch()
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(m, n, dtype=torch.float64, device="cuda", generator=g)


def _cond_matrix(m, n, cond, seed):
    # A = U diag(s) V^T in fp64 on the GPU (torch's QR only shapes the test matrix)
    torch = _torch()
    g = torch.Generator(device="cuda").manual_seed(seed)
    u, _ = torch.linalg.qr(torch.randn(m, n, dtype=torch.float64, device="cuda", generator=g))
    v, _ = torch.linalg.qr(torch.randn(n, n, dtype=torch.float64, device="cuda", generator=g))
    s = torch.logspace(0.0, -float(np.log10(cond)), n, dtype=torch.float64, device="cuda")
    return (u * s) @ v.T


def _check(a_dev, q, r, reorth, cond=None):
    """bands of include/tsqr_mi.h, R's shape, guard bands, agreement with LAPACK's R within 50 n u cond; returns (orth, res, cond)"""
    torch = _torch()
    m, n = a_dev.shape
    assert torch.isnan(q[:, m:]).all(), "Q's padding rows were written"
    assert torch.isnan(r[:, n:]).all(), "R's padding rows were written"
    Q = q[:, :m].T
    Rd = r[:, :n].T
    R = Rd.cpu().numpy()
    assert np.all(np.tril(R, -1) == 0.0), "R has non-zeros below the diagonal"
    assert np.all(np.diag(R) > 0.0), "R's diagonal is not positive"
    I = torch.eye(n, dtype=torch.float64, device="cuda")
    orth = torch.linalg.norm(Q.T @ Q - I).item()
    res = (torch.linalg.norm(a_dev - Q @ Rd) / torch.linalg.norm(a_dev)).item()
    scale = max(1.0, n / 64.0)
    assert orth <= (1e-12 if reorth else 1e-11) * scale, ("orthogonality", orth)
    assert res <= 1e-13, ("residual", res)
    r_lp = np.linalg.qr(a_dev.cpu().numpy(), mode="r")
    r_lp = np.sign(np.diag(r_lp))[:, None] * r_lp
    if cond is None:
        cond = np.linalg.cond(r_lp)
    dr = np.linalg.norm(R - r_lp) / np.linalg.norm(R)
    assert dr <= 50 * n * U53 * cond, ("R against LAPACK", dr, cond)
    return orth, res, cond


SHAPES = [(200, 65), (4096, 100), (65536, 128), (16384, 256), (8192, 640), (4096, 1024), (1100, 1024)]


@pytest.mark.parametrize("m,n", SHAPES)
def test_f64_wide_shapes(bq, m, n):
    a_dev = _gauss(m, n, m + n)
    cond = None
    for reorth in (0, 1):
        st, q, r, _ = _run(bq, a_dev, reorth)
        assert st == 0, (st, bq.last_error())
        sweeps = bq.last_sweeps_f64()
        orth, res, cond = _check(a_dev, q, r, reorth, cond)
        print("%d x %d reorth %d: sweeps %d  ||QtQ-I||_F %.2e  residual %.2e  cond %.1f" % (m, n, reorth, sweeps, orth, res, cond))
        if m >= 16 * n:                                   # Gaussian tall-skinny: cond(A) < 10, one sweep / CholeskyQR2
            assert sweeps == (2 if reorth else 1), sweeps
        else:
            assert sweeps == 2 or (sweeps == 1 and not reorth), sweeps


@pytest.mark.parametrize("n", [128, 256])
def test_f64_wide_conditioning(bq, n):
    m = 16384
    for cond in (1.0, 1e3, 1e8, 1e12):
        a_dev = _cond_matrix(m, n, cond, seed=int(np.log10(cond)) + n)
        for reorth in (0, 1):
            st, q, r, _ = _run(bq, a_dev, reorth)
            assert st == 0, (st, bq.last_error())
            sweeps = bq.last_sweeps_f64()
            orth, res, _ = _check(a_dev, q, r, reorth, max(cond, 1.0) * 1.01)
            print("m %d n %d cond %.0e reorth %d: sweeps %d  ||QtQ-I||_F %.2e  residual %.2e" % (m, n, cond, reorth, sweeps, orth, res))
            if cond == 1.0:
                assert sweeps == (2 if reorth else 1), sweeps
            if reorth:
                assert sweeps % 100 >= 2
            if cond == 1e12:
                assert sweeps >= 100, sweeps


@pytest.mark.parametrize("n", [1, 51, 64])
def test_f64_wide_one_panel_is_qr_f64(bq, n):
    torch = _torch()
    m = 9211
    a_dev = _cond_matrix(m, n, 1e5, seed=n) if n > 1 else _gauss(m, n, 1)
    for reorth in (0, 1):
        bf = bq.buffer_f64(reorth)
        bf.allocate(m, n)
        st1, q1, r1, _ = _run(bq, a_dev, reorth, entry=bq.qr_f64, bf=bf)
        s1 = bq.last_sweeps_f64()
        st2, q2, r2, _ = _run(bq, a_dev, reorth)
        s2 = bq.last_sweeps_f64()
        assert st1 == st2 == 0 and s1 == s2
        assert torch.equal(q1[:, :m], q2[:, :m]) and torch.equal(r1[:, :n], r2[:, :n]), "the one-panel path differs from qr_f64"


@pytest.mark.parametrize("m,n", [(4096, 256), (3000, 1000)])
def test_f64_wide_in_place_and_determinism(bq, m, n):
    torch = _torch()
    a_dev = _cond_matrix(m, n, 1e6, seed=n)
    for reorth in (0, 1):
        st, q1, r1, a = _run(bq, a_dev, reorth)
        assert st == 0, (st, bq.last_error())
        assert torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(_padded(a_dev, a.shape[1]), nan=7.0)), "A was modified"
        st, q2, r2, _ = _run(bq, a_dev, reorth)
        assert st == 0
        assert torch.equal(q1[:, :m], q2[:, :m]) and torch.equal(r1[:, :n], r2[:, :n]), "two calls differ"
        lda = m + 3                                      # in place: q == a, ldq == lda
        a_in = _padded(a_dev, lda)
        r3 = torch.full((n, n + 2), float("nan"), dtype=torch.float64, device="cuda")
        bf = bq.buffer_f64_wide(reorth)
        bf.allocate(m, n)
        st = bq.qr_f64_wide(a_in, lda, r3, n + 2, a_in, lda, m, n, bf)
        torch.cuda.synchronize()
        assert st == 0
        assert torch.equal(a_in[:, :m], q1[:, :m]), "in place differs from out of place"
        assert torch.isnan(a_in[:, m:]).all()
        assert torch.equal(r3[:, :n], r1[:, :n])


def test_f64_wide_non_finite(bq):
    m, n = 4096, 200                                     # blocks of 64, 64, 64, 8 columns
    a_dev = _gauss(m, n, 3)
    bf = bq.buffer_f64_wide(False)
    bf.allocate(m, n)
    for val, col in ((float("nan"), 195), (float("inf"), 199), (float("nan"), 192)):
        bad = a_dev.clone()
        bad[1000, col] = val
        st, _, _, _ = _run(bq, bad, 0, bf=bf)
        assert st == bq.error_not_finite == 3, (val, col, st)
    bad = a_dev.clone()
    bad[7, 150] = float("inf")
    st, _, _, _ = _run(bq, bad, 1, bf=bf)
    assert st == 3
    st, q, r, _ = _run(bq, a_dev, 0, bf=bf)              # the same buffer, good data
    assert st == 0, (st, bq.last_error())
    assert bq.last_sweeps_f64() == 1
    _check(a_dev, q, r, 0)


# ---- the ladder: S_ref prescribed on both sides of both thresholds of the acceptance rule -------------------------------------------------
@pytest.mark.parametrize("n", [128, 200])
def test_f64_wide_ladder_sweep_counts(bq, n):
    """as tests/test_gpu_f64.py::test_f64_ladder_sweep_counts, through tsqr_mi_qr_f64_wide: S is summed over block pairs here, and a
    sum without its off-diagonal terms would take one sweep where CholeskyQR2 is needed.  Sweep counts exactly: 1, 2, 2, 103
    (reorth = 1: 2, 2, 2, 103), and the bands of the header."""
    from tests import pass_refs_f64 as p64
    torch = _torch()
    m = 4096
    for name, target, s0, s1 in p64.ladder_targets(m, n):
        a_host, s_ref = p64.ladder_matrix(m, n, target, n)
        a_dev = torch.from_numpy(a_host).cuda()
        cond = np.linalg.cond(a_host)
        for reorth, want in ((0, s0), (1, s1)):
            st, q, r, _ = _run(bq, a_dev, reorth)
            assert st == 0, (st, bq.last_error())
            sweeps = bq.last_sweeps_f64()
            orth, res, _ = _check(a_dev, q, r, reorth, cond)
            print("ladder %d x %d  S_ref = %s = %.4g  reorth %d: sweeps %d  ||QtQ-I||_F %.2e  residual %.2e%s" % (
                m, n, name, s_ref, reorth, sweeps, orth, res,
                "  one-sweep estimate 4nSu %.2e" % (4 * n * s_ref * U53) if sweeps == 1 else ""))
            assert sweeps == want, (name, reorth, sweeps, want)


def test_f64_wide_limit_2p16_x_1024(bq):
    """the documented limit m n = 2^26 at n = 1024, Gaussian data generated on the device: the bands of the header"""
    torch = _torch()
    m, n = 1 << 16, 1024
    a_dev = _gauss(m, n, 26)
    I = torch.eye(n, dtype=torch.float64, device="cuda")
    for reorth in (0, 1):
        st, q, r, _ = _run(bq, a_dev, reorth)
        assert st == 0, (st, bq.last_error())
        assert torch.isnan(q[:, m:]).all() and torch.isnan(r[:, n:]).all()
        Q, Rd = q[:, :m].T, r[:, :n].T
        orth = torch.linalg.norm(Q.T @ Q - I).item()
        res = (torch.linalg.norm(a_dev - Q @ Rd) / torch.linalg.norm(a_dev)).item()
        print("2^16 x 1024 reorth %d: sweeps %d  ||QtQ-I||_F %.2e  residual %.2e" % (reorth, bq.last_sweeps_f64(), orth, res))
        assert torch.all(torch.tril(Rd, -1) == 0) and torch.all(torch.diagonal(Rd) > 0)
        assert orth <= (1e-12 if reorth else 1e-11) * n / 64 and res <= 1e-13

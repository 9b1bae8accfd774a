"""NumPy model, figures and cases of the fp64 block orthogonalisation (tsqr_mi_orth_f64): BCGS2 with numpy.linalg.qr as the inner
factorisation, its signs fixed so that diag(R) >= 0.  The figures are evaluated in longdouble.  Shared by the CPU test of the model
(tests/test_pass_refs_f64_orth.py) and the GPU tests; every case and every model result is computed once and must not be modified."""
import functools

import numpy as np

U = 2.0 ** -53
QTQ_BOUND, RESID_BOUND = 1e-11, 1e-13        # the QR entry's own claims (include/tsqr_mi.h), restated for this entry

# id: (m, k, n, eps, cond(G) or None, seed).  W = V C + eps G: V from numpy.linalg.qr of a Gaussian, C Gaussian, G Gaussian or with the
# stated condition number.
CASES = {
    "1003x130x17": (1003, 130, 17, 1.0, None, 1),             # three V blocks, the last padded; two column tiles; m no multiple of 16
    "1003x130x17-near": (1003, 130, 17, 1e-6, None, 2),       # near span
    "1003x130x17-near-cond1e8": (1003, 130, 17, 1e-6, 1e8, 3),   # near span; the one-factorisation form fails here
    "80x64x16-complete": (80, 64, 16, 1e-6, None, 4),         # k + n = m: Q completes the space
    "333x1x1": (333, 1, 1, 1e-6, None, 5),                    # k = 1, n = 1
    "2061x65x64-cond1e8": (2061, 65, 64, 1.0, 1e8, 6),        # one column past a block edge, full width, more than one sweep
    "4096x1024x64-caps": (4096, 1024, 64, 1e-6, None, 7),     # both caps
    "1003x63x16": (1003, 63, 16, 1.0, None, 8),               # the block edge of k and the tile edge of n, eps = 1
    "1003x63x64": (1003, 63, 64, 1.0, None, 9),
    "1003x64x16": (1003, 64, 16, 1.0, None, 10),
    "1003x64x64": (1003, 64, 64, 1.0, None, 11),
    "33000x70x20-slices": (33000, 70, 20, 1.0, None, 12),     # 2063 chunks on 2 blocks: five chunks to a slice, the last slice short
}
TABLE = list(CASES)[:7]                                       # the table of the issue
NEAR_SPAN = [c for c in CASES if CASES[c][3] < 1.0]
EPS_ONE = [c for c in CASES if CASES[c][3] == 1.0]


def with_cond(rng, m, n, cond):
    """an m x n matrix with singular values log-spaced from 1 down to 1 / cond"""
    u = np.linalg.qr(rng.standard_normal((m, n)))[0]
    v = np.linalg.qr(rng.standard_normal((n, n)))[0]
    s = np.logspace(0.0, -np.log10(cond), n) if n > 1 else np.ones(1)
    return (u * s) @ v.T


@functools.lru_cache(maxsize=None)
def make(case):
    """-> (V, W), read only"""
    m, k, n, eps, cond, seed = CASES[case]
    rng = np.random.default_rng(seed)
    v = np.ascontiguousarray(np.linalg.qr(rng.standard_normal((m, k)))[0])
    c = rng.standard_normal((k, n))
    g = rng.standard_normal((m, n)) if cond is None else with_cond(rng, m, n, cond)
    w = v @ c + eps * g
    v.setflags(write=False)
    w.setflags(write=False)
    return v, w


def qr_pos(x):
    """numpy.linalg.qr with diag(R) >= 0"""
    q, r = np.linalg.qr(x)
    sg = np.where(np.diag(r) < 0.0, -1.0, 1.0)
    return q * sg, sg[:, None] * r


def model(v, w, passes=2):
    """BCGS2 -> (Q, S, R): the round Si = V^T X, X <- X - V Si, X = Qi Ri, `passes` times; S = S1 + S2 R1, R = R2 R1"""
    x = np.array(w)
    s = r = None
    for rnd in range(passes):
        si = v.T @ x
        x, ri = qr_pos(x - v @ si)
        s, r = (si, ri) if rnd == 0 else (s + si @ r, ri @ r)
    return x, s, r


def figures(v, w, q, s, r):
    """(||V^T Q||_F, ||Q^T Q - I||_F, ||W - V S - Q R||_F / ||W||_F) in longdouble"""
    ld = np.longdouble
    vl, wl, ql, sl, rl = (np.asarray(a, dtype=ld) for a in (v, w, q, s, r))
    n = q.shape[1]
    fro = lambda a: float(np.sqrt(np.sum(a * a)))
    return fro(vl.T @ ql), fro(ql.T @ ql - np.eye(n, dtype=ld)), fro(wl - vl @ sl - ql @ rl) / fro(wl)


@functools.lru_cache(maxsize=None)
def model_figures(case, passes=2):
    v, w = make(case)
    return figures(v, w, *model(v, w, passes))


def vq_floor(case):
    _, k, n = CASES[case][:3]
    return 4.0 * max(k, n) * U


def vq_bound(case):
    """max(2 x the model's ||V^T Q||_F on the same data, 4 max(k, n) 2^-53): the convention of the least-squares tests"""
    return max(2.0 * model_figures(case, 2)[0], vq_floor(case))

"""CPU tests of the test-library entries of the rank-aware least-squares passes (tsqr_selftest_f64_lsq_dense_lay,
tsqr_selftest_f64_lsq_rank, tsqr_selftest_f64_lsq_update_rule; selftest_f64.hip): they are exported, and every call below is rejected
with -100 by the argument checks, which come before any HIP call -- all pointers are null and nothing is launched."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
c_sz, c_p, c_i, c_d = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int, ctypes.c_double
REJECTED = -100


@pytest.fixture(scope="module")
def T(bq):
    bq.lib()                                               # (torch's HIP runtime first, as every user of the libraries loads it)
    L = ctypes.CDLL(os.path.join(ROOT, "tsqr_gpu_amd", "csrc", "libtsqr_selftest.so"))
    sig = {
        "tsqr_selftest_f64_lsq_dense_lay": [c_i, c_i, c_p, c_p, c_sz, c_p, c_sz, c_sz, c_i, c_i, c_p, c_p, c_p, c_sz, c_i],
        "tsqr_selftest_f64_lsq_rank": [c_p, c_sz, c_p, c_d, c_p, c_p, c_i],
        "tsqr_selftest_f64_lsq_update_rule": [c_i, c_p, c_p, c_sz, c_p, c_p, c_i, c_i, c_i, c_i, c_p, c_i],
    }
    for name, args in sig.items():
        assert hasattr(L, name), name
        getattr(L, name).restype = c_i
        getattr(L, name).argtypes = args
    return L


def test_dense_pass_hook_rejects_before_any_launch(T):
    def call(a_lay=0, b_lay=0, lda=100, ldb=100, m=100, n=8, nrhs=3):
        return T.tsqr_selftest_f64_lsq_dense_lay(a_lay, b_lay, None, None, lda, None, ldb, m, n, nrhs, None, None, None, 0, 0)
    for bad in (dict(a_lay=2), dict(b_lay=-1), dict(m=0), dict(n=0), dict(n=65), dict(nrhs=0), dict(nrhs=17), dict(lda=99), dict(ldb=99),
                dict(a_lay=1, lda=7), dict(b_lay=1, ldb=2)):
        assert call(**bad) == REJECTED, bad


def test_rank_hook_rejects_before_any_launch(T):
    some = ctypes.c_void_p(64)
    for n, ldr, r, jp, z, st in ((0, 8, some, some, some, some), (65, 65, some, some, some, some), (8, 7, some, some, some, some),
                                 (8, 8, None, some, some, some), (8, 8, some, None, some, some), (8, 8, some, some, None, some),
                                 (8, 8, some, some, some, None)):
        assert T.tsqr_selftest_f64_lsq_rank(r, ldr, jp, 1e-8, z, st, n) == REJECTED, (n, ldr)


def test_update_hook_rejects_before_any_launch(T):
    def call(dense=1, ldx=8, n=8, nrhs=3):
        return T.tsqr_selftest_f64_lsq_update_rule(dense, None, None, ldx, None, None, n, nrhs, 1, 1, None, 0)
    for bad in (dict(dense=2), dict(dense=-1), dict(n=0), dict(n=65, ldx=65), dict(nrhs=0), dict(nrhs=17), dict(ldx=7)):
        assert call(**bad) == REJECTED, bad

"""The acceptance rule of the fp64 entries evaluated ON THE DEVICE (f64_rule_of inside a kernel, tsqr_f64.hip: what the Cholesky step of
a row-partitioned call does with the all-reduced row count) against the host's f64_rule, the one every one-GPU launch takes: the three
numbers must be the same bits, or two ranks -- or the same matrix on one GPU and on two -- could take different rungs of the ladder."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_device_rule_equals_host_rule_bit_for_bit(bq):
    import torch
    from tests import pass_refs_f64 as p64
    L = ctypes.CDLL(os.path.join(ROOT, "tsqr_gpu_amd", "csrc", "libtsqr_selftest.so"))
    c_p, c_sz, c_i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    L.tsqr_selftest_f64_rule.argtypes = [c_sz, c_sz, c_i, c_p]
    L.tsqr_selftest_f64_rule_device.argtypes = [c_p, c_p, c_p, c_i, c_p]
    cases = []
    for n in (1, 33, 64, 65, 1024):
        for rows in (1, 4096, 1 << 23, (1 << 26) // n, 777, 1234567, (1 << 26) // n - 1):
            for first in (1, 0):
                cases.append((rows, n, first))
    want = np.empty((len(cases), 3))
    out = (ctypes.c_double * 3)()
    for i, (rows, n, first) in enumerate(cases):
        assert L.tsqr_selftest_f64_rule(rows, n, first, ctypes.cast(out, c_p)) == 0
        want[i] = out[:]
    rows_d = torch.tensor([float(c[0]) for c in cases], dtype=torch.float64, device="cuda")
    n_d = torch.tensor([c[1] for c in cases], dtype=torch.int32, device="cuda")
    first_d = torch.tensor([c[2] for c in cases], dtype=torch.int32, device="cuda")
    got_d = torch.full((len(cases), 3), float("nan"), dtype=torch.float64, device="cuda")
    assert L.tsqr_selftest_f64_rule_device(rows_d.data_ptr(), n_d.data_ptr(), first_d.data_ptr(), len(cases), got_d.data_ptr()) == 0
    got = got_d.cpu().numpy()
    for i, c in enumerate(cases):
        assert got[i].view(np.uint64).tolist() == want[i].view(np.uint64).tolist(), (c, got[i], want[i])
    # and both are the rule the tests state in numpy (first sweep) / infinity, never alone, the same shift (later sweeps)
    for i, (rows, n, first) in enumerate(cases):
        mx, al, sh = p64.rule(rows, n)
        assert got[i][2] == sh
        assert (got[i][0], got[i][1]) == ((mx, al) if first else (np.inf, 0.0))

"""The block loop of the apply kernels (apply_wg_body) run MORE THAN ONCE per workgroup on small matrices.

With the default persistent grid a workgroup gets a second block only above ~65 536 rows, so no small test runs the loop, the two-deep
prefetch hand-over (v <- v2) or the tail of a workgroup's progression more than once.  tsqr_mi_set_tuning2(0, 4) gives the apply pass ONE
workgroup (every block in one progression), tsqr_mi_set_tuning2(0, 8) two (odd and even progressions).  The setting cannot be put back to
"as many as are resident", so all cases run in one fresh child process (this file as a script) and the small grid never reaches the rest
of the suite.

Cases: tsqr_mi_apply_rinv_f32 on the exact small-integer data of test_gpu_passes.test_apply_exact_inverse_small_integers -- Q must be
exact -- for m in {323, 449} (six and eight 64-row blocks with a row tail; three and four 128-row blocks), n in {64, 33, 7}, the three
engines, out of place and in place; then one reorthogonalised tsqr_mi_qr_f32 call (fp32_tc_cor, 1000 x 64) with one workgroup -- the
fused-Gram variant over several blocks -- held to the bounds of test_gpu_parity.test_parity_with_oracle_reorth."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SPLITS = {64: 23, 33: 16, 7: 3}                 # the split of exact_inverse_pair: away from a tile boundary, on one, inside the only tile


@pytest.mark.gpu
def test_apply_block_loop_with_one_and_two_workgroups(bq):
    out = subprocess.run([sys.executable, "-s", os.path.abspath(__file__)], capture_output=True, text=True, timeout=240, cwd=ROOT)
    print(out.stdout[-4000:])
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "apply grid: 73 cases passed" in out.stdout


def _child():
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from oracle import ref_oracle as oracle
    from tests import pass_refs as pr
    from tests import test_gpu_parity as par
    from tests import test_gpu_passes as tp
    from tsqr_gpu_amd import blockqr as bq

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    L = bq.lib()
    env = (bq, L, torch)
    cases = 0
    for apply_waves in (4, 8):                  # four waves a workgroup: one workgroup, then two
        L.tsqr_mi_set_tuning2(0, apply_waves)
        for m in (323, 449):
            for n in (64, 33, 7):
                for engine in (0, 1, 2):
                    for inplace in (False, True):
                        rng = np.random.default_rng(m * 7 + n + engine)
                        r, z = pr.exact_inverse_pair(rng, n, SPLITS[n], bmax=63, scale_exp=0)
                        r, z = r * np.float32(8.0), z / 8.0
                        a = pr.exact_ints(rng, m, n, kmax=63, exps=(0, 0))
                        q = tp._apply_case(env, bq.compute_mode[tp.ENGINES[engine]], a, r, inplace)
                        ref = a.astype(np.float64) @ z
                        assert np.array_equal(q, ref), (apply_waves, m, n, engine, inplace, np.argwhere(q != ref)[:5])
                        cases += 1
    # the fused-Gram variant (first sweep of a reorthogonalised call, 128-row blocks): eight blocks in one workgroup
    L.tsqr_mi_set_tuning2(0, 4)
    md = bq.compute_mode.fp32_tc_cor
    a = oracle.uniform_matrix(1000, 64, seed=12)
    st, q, r = par.run_gpu(bq, torch, a, md, True, ldq_pad=3)
    assert st == bq.success_factorization
    assert np.abs(np.tril(r, -1)).max() == 0.0
    res, orth = oracle.residual(a, q, r), oracle.orthogonality_fro(q)
    print("reorth 1000 x 64, one workgroup: residual %.3g (< %.3g), orthogonality %.3g (< %.3g)" % (res, par.RES_TOL, orth, par.ORTH_TOL))
    assert res < par.RES_TOL
    assert orth < par.ORTH_TOL
    st_o, q_o, r_o = oracle.qr(a, int(md), True)
    assert st_o == 0
    qn, rn = oracle.sign_normalise(q, r)
    qon, ron = oracle.sign_normalise(q_o, np.triu(r_o))
    scale = max(1.0, np.linalg.cond(a.astype(np.float64)) / 10)
    assert np.abs(rn - ron).max() / np.abs(ron).max() < par.PAR_TOL * scale
    assert np.abs(qn - qon).max() < par.PAR_TOL * scale
    q2, r2 = np.linalg.qr(a.astype(np.float64))
    _, r2n = oracle.sign_normalise(q2, r2)
    assert np.abs(rn - r2n).max() / np.abs(r2n).max() < 5e-6 * scale
    cases += 1
    print("apply grid: %d cases passed" % cases)


if __name__ == "__main__":
    _child()

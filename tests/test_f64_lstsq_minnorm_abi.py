"""CPU tests of the minimum-norm rank-aware fp64 least-squares entry (tsqr_mi_lstsq_minnorm_f64): exported symbols and their signatures,
work-space sizes, the table of states, the keyword of lstsq_rank_f64, the two test-library hooks of its kernels, and a C++ caller of
mtk::qr::lstsq_minnorm_fp64 that compiles and links.

EVERY call in this file is rejected before a HIP call.  The table of states is that of tests/test_f64_lstsq_rank_abi.py, case for case
and in its order -- the entry has tsqr_mi_lstsq_rank_f64's checks -- with every text naming THIS entry."""
import ctypes
import os

import pytest

from abi_util import compile_and_link, header_flat
from tests import test_f64_lstsq_rank_abi as base

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("tsqr_mi_lstsq_minnorm_f64", "tsqr_mi_working_q_size_f64_lstsq_minnorm", "tsqr_mi_working_r_size_f64_lstsq_minnorm")
BAD, UNSUPPORTED, COL, ROW, SOME, POINTERS = base.BAD, base.UNSUPPORTED, base.COL, base.ROW, base.SOME, base.POINTERS


def test_symbols_exported_with_the_stated_signatures(bq):
    L = ctypes.CDLL(bq.LIB_PATH)
    flat = header_flat()
    for sym in SYMBOLS:
        assert hasattr(L, sym), sym
        assert sym in bq.C_ABI_SYMBOLS, sym
    assert "size_t tsqr_mi_working_q_size_f64_lstsq_minnorm(size_t m, size_t n, size_t nrhs);" in flat
    assert "size_t tsqr_mi_working_r_size_f64_lstsq_minnorm(size_t m, size_t n, size_t nrhs);" in flat
    assert ("int tsqr_mi_lstsq_minnorm_f64(int a_layout, int b_layout, int reorth, int refine, double rcond, double* x, size_t ldx, "
            "double* r, size_t ldr, int* jpvt, int* rank, const double* a, size_t lda, const double* b, size_t ldb, "
            "size_t m, size_t n, size_t nrhs, void* wq, void* wr, void* stream);") in flat
    assert bq.C_SIGNATURES["tsqr_mi_lstsq_minnorm_f64"] == bq.C_SIGNATURES["tsqr_mi_lstsq_rank_f64"]
    # the "Not provided" lists no longer name the minimum-norm solution
    assert "Not provided: the minimum-norm solution" not in flat
    import inspect
    par = inspect.signature(bq.lstsq_rank_f64).parameters["minimum_norm"]
    assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is False
    sel = ctypes.CDLL(os.path.join(ROOT, "tsqr_gpu_amd", "csrc", "libtsqr_selftest.so"))
    assert hasattr(sel, "tsqr_selftest_f64_lsq_zg") and hasattr(sel, "tsqr_selftest_f64_lsq_minnorm")


def test_working_sizes(bq):
    L = bq.lib()
    wqs = set()
    for n in (1, 7, 16, 17, 33, 51, 64):
        for m in (1, 15, 16, 17, 33, 1000, 4099, 9211, 1 << 16, 1 << 20, (1 << 20) + 1, 1 << 23):
            for nrhs in (1, 5, 16):
                wq, wr = L.tsqr_mi_working_q_size_f64_lstsq_minnorm(m, n, nrhs), L.tsqr_mi_working_r_size_f64_lstsq_minnorm(m, n, nrhs)
                wqs.add(wq)
                # the basic entry's layout and Zmn (64 x 64) behind it; wr is the basic entry's
                assert wq == L.tsqr_mi_working_q_size_f64_lstsq_rank(m, n, nrhs) + 4096, (m, n, nrhs, wq)
                assert wr == L.tsqr_mi_working_r_size_f64_lstsq_rank(m, n, nrhs), (m, n, nrhs, wr)
    assert len(wqs) == 1, "wq depends on m, n or nrhs"
    for m, n, nrhs in ((0, 4, 1), (4, 0, 1), (4, 4, 0), (0, 0, 0)):
        assert L.tsqr_mi_working_q_size_f64_lstsq_minnorm(m, n, nrhs) == 0 and L.tsqr_mi_working_r_size_f64_lstsq_minnorm(m, n, nrhs) == 0


def call(L, m=100, n=8, nrhs=3, lay=None, ld=None, refine=1, reorth=0, rcond=1e-8, null=()):
    """test_f64_lstsq_rank_abi.call on tsqr_mi_lstsq_minnorm_f64"""
    lay = dict(lay or {})
    lds = {}
    for op, rows, cols in (("a", m, n), ("b", m, nrhs), ("r", n, n), ("x", n, nrhs)):
        lds[op] = max(cols if lay.get(op, COL) == ROW else rows, 1)
    lds.update(ld or {})
    host_rank = ctypes.c_int(-7)
    ptr = {name: (None if name in null else SOME) for name in POINTERS}
    ptr["rank"] = None if "rank" in null else ctypes.byref(host_rank)
    st = L.tsqr_mi_lstsq_minnorm_f64(lay.get("a", COL), lay.get("b", COL), reorth, refine, rcond, ptr["x"], lds["x"], ptr["r"], lds["r"],
                                     ptr["jpvt"], ptr["rank"], ptr["a"], lds["a"], ptr["b"], lds["b"], m, n, nrhs, ptr["wq"], ptr["wr"], None)
    assert host_rank.value == -7, "a rejected call wrote the rank"
    return st


def own(text):
    return None if text is None else text.replace("tsqr_mi_lstsq_rank_f64", "tsqr_mi_lstsq_minnorm_f64")


CASES = [pytest.param(kw, state, own(text), id=cid) for cid, kw, state, text in base.state_cases()]


@pytest.mark.parametrize("kw,state,text", CASES)
def test_state_sweeps_and_text(bq, kw, state, text):
    """the state, the sweep count cleared, a text naming this entry for every state 2 and the text left alone by a state 1"""
    from tests.test_f64_entry_states import Z
    L = bq.lib()
    assert L.tsqr_mi_r_f64(0, Z, 65, Z, 100, 100, 65, Z, Z, Z) == UNSUPPORTED      # a sentinel text from another entry's state 2
    sentinel = bq.last_error()
    assert "tsqr_mi_r_f64 supports n <= 64" in sentinel
    assert call(L, **kw) == state
    assert L.tsqr_mi_last_sweeps_f64() == 0
    if text is None:
        assert state == BAD and bq.last_error() == sentinel
    else:
        assert "tsqr_mi_lstsq_minnorm_f64" in text and text in bq.last_error() and text not in sentinel


def test_table_is_the_basic_entry_s():
    assert len(CASES) == len(base.CASES) and [c.id for c in CASES] == [c.id for c in base.CASES]
    texts = [c.values[2] for c in CASES if c.values[2] is not None]
    assert len(texts) == 29 and all("tsqr_mi_lstsq_minnorm_f64" in t for t in texts)      # (every state 2 of the table)


def test_keyword_operand_checks(bq):
    import torch
    a = torch.zeros(100, 8, dtype=torch.float64)
    b = torch.zeros(100, 3, dtype=torch.float64)
    for bad in ((a.float(), b), (a, b.float()), (a, b)):                      # (the last: CPU tensors of the right type)
        with pytest.raises(TypeError):
            bq.lstsq_rank_f64(*bad, minimum_norm=True)
    with pytest.raises(TypeError):
        bq.lstsq_rank_f64(a, b, None, False, 1, None, True)                   # keyword only
    if torch.cuda.is_available():                              # (the GPU box: shapes and states on device tensors; nothing is launched)
        a, b = a.cuda(), b.cuda()
        wide = torch.zeros(100, 65, dtype=torch.float64, device="cuda")
        many = torch.zeros(100, 17, dtype=torch.float64, device="cuda")
        for args, kw, state in (((a[:4], b[:4]), {}, BAD), ((wide, b), {}, UNSUPPORTED), ((a, many), {}, UNSUPPORTED),
                                ((a, b), dict(refine=5), UNSUPPORTED), ((a, b), dict(rcond=1.0), UNSUPPORTED)):
            with pytest.raises(bq.LstsqRankError) as e:
                bq.lstsq_rank_f64(*args, minimum_norm=True, **kw)
            assert e.value.state == state
            if state == UNSUPPORTED:
                assert "tsqr_mi_lstsq_minnorm_f64" in str(e.value)


# ---- the two test-library hooks: every call is rejected by the argument checks, which come before any HIP call -----------------------------
REJECTED = -100
c_p, c_i = ctypes.c_void_p, ctypes.c_int


@pytest.fixture(scope="module")
def T(bq):
    bq.lib()                                               # (torch's HIP runtime first, as every user of the libraries loads it)
    L = ctypes.CDLL(os.path.join(ROOT, "tsqr_gpu_amd", "csrc", "libtsqr_selftest.so"))
    sig = {"tsqr_selftest_f64_lsq_zg": [c_p, c_p, c_p, c_i], "tsqr_selftest_f64_lsq_minnorm": [c_p, c_p, c_p, c_p, c_p, c_p, c_i]}
    for name, args in sig.items():
        assert hasattr(L, name), name
        getattr(L, name).restype = c_i
        getattr(L, name).argtypes = args
    return L


def test_zg_hook_rejects_before_any_launch(T):
    for n, p, k, z in ((0, SOME, SOME, SOME), (65, SOME, SOME, SOME), (-1, SOME, SOME, SOME), (8, None, SOME, SOME), (8, SOME, None, SOME),
                       (8, SOME, SOME, None), (8, None, None, None)):
        assert T.tsqr_selftest_f64_lsq_zg(p, k, z, n) == REJECTED, n


def test_minnorm_hook_rejects_before_any_launch(T):
    full = [SOME] * 6
    for n in (0, 65, -1):
        assert T.tsqr_selftest_f64_lsq_minnorm(*full, n) == REJECTED, n
    for i in range(6):
        args = list(full)
        args[i] = None
        assert T.tsqr_selftest_f64_lsq_minnorm(*args, 8) == REJECTED, i
    assert T.tsqr_selftest_f64_lsq_minnorm(*([None] * 6), 8) == REJECTED


def test_cpp_lstsq_minnorm_fp64_compiles_and_links(bq):
    with compile_and_link(os.path.join(ROOT, "tests", "cpp", "sample_fp64_lstsq_minnorm.cpp"), "sample_fp64_lstsq_minnorm") as exe:
        assert os.path.exists(exe)

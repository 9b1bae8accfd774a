"""CPU tests of the rank-aware fp64 least-squares entry (tsqr_mi_lstsq_rank_f64): exported symbols and their signatures, work-space
sizes, the table of states, the Python operand checks of lstsq_rank_f64, the two test-library hooks of its CholeskyQR step, and a C++
caller of mtk::qr::lstsq_rank_fp64 that compiles and links.

EVERY call in this file is rejected before a HIP call.  The entry's order (tsqr_mi.hip): the sweep count cleared; any null among x, r,
jpvt, rank, a, b, wq, wr (state 1); f64_prologue -- layouts, n > m, empty operands and short leading dimensions (state 1), n > 64 (state
2); nrhs > 16, refine outside 0 .. 4, rcond >= 1 or NaN (state 2); only then the first HIP call.  Because the null check comes first, the
cases that are to reach a later check pass non-null pointers: addresses that are never followed (SOME), and a real host int for rank.
No case passes such pointers together with arguments that pass every check: each case breaks exactly the check it names, and the cases
with a null pointer end at the first statement whatever else they carry."""
import ctypes
import os

import pytest

from abi_util import compile_and_link, header_flat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("tsqr_mi_lstsq_rank_f64", "tsqr_mi_working_q_size_f64_lstsq_rank", "tsqr_mi_working_r_size_f64_lstsq_rank")
BAD, UNSUPPORTED = 1, 2
COL, ROW = 0, 1
SOME = ctypes.c_void_p(64)
POINTERS = ("x", "r", "jpvt", "rank", "a", "b", "wq", "wr")
NAN = float("nan")


def test_symbols_exported_with_the_stated_signatures(bq):
    L = ctypes.CDLL(bq.LIB_PATH)
    flat = header_flat()
    for sym in SYMBOLS:
        assert hasattr(L, sym), sym
        assert sym in bq.C_ABI_SYMBOLS, sym
    assert "size_t tsqr_mi_working_q_size_f64_lstsq_rank(size_t m, size_t n, size_t nrhs);" in flat
    assert "size_t tsqr_mi_working_r_size_f64_lstsq_rank(size_t m, size_t n, size_t nrhs);" in flat
    assert ("int tsqr_mi_lstsq_rank_f64(int a_layout, int b_layout, int reorth, int refine, double rcond, double* x, size_t ldx, "
            "double* r, size_t ldr, int* jpvt, int* rank, const double* a, size_t lda, const double* b, size_t ldb, "
            "size_t m, size_t n, size_t nrhs, void* wq, void* wr, void* stream);") in flat
    restype, argtypes = bq.C_SIGNATURES["tsqr_mi_lstsq_rank_f64"]
    assert restype is ctypes.c_int and len(argtypes) == 21 and argtypes[4] is ctypes.c_double
    import tsqr_gpu_amd
    assert tsqr_gpu_amd.lstsq_rank_f64 is bq.lstsq_rank_f64 and issubclass(bq.LstsqRankError, RuntimeError)
    sel = ctypes.CDLL(os.path.join(ROOT, "tsqr_gpu_amd", "csrc", "libtsqr_selftest.so"))
    assert hasattr(sel, "tsqr_selftest_f64_gramq_dense_lay") and hasattr(sel, "tsqr_selftest_f64_lsq_rank_step")


def test_working_sizes(bq):
    L = bq.lib()
    ms = (1, 15, 16, 17, 33, 1000, 4099, 9211, 1 << 16, 1 << 20, (1 << 20) + 1, 1 << 23)
    wqs = set()
    for n in (1, 7, 16, 17, 33, 51, 64):
        for m in ms:
            for nrhs in (1, 5, 16):
                wq, wr = L.tsqr_mi_working_q_size_f64_lstsq_rank(m, n, nrhs), L.tsqr_mi_working_r_size_f64_lstsq_rank(m, n, nrhs)
                wqs.add(wq)
                # the least-squares entry's layout, Zeff (64 x 64), the step's Gram sum (10 tiles of 256 and the reduction's row count)
                # and two status words
                assert wq >= L.tsqr_mi_working_q_size_f64_lstsq(m, n, nrhs) + 4096 + 2560 + 1 + 1, (m, n, nrhs, wq)
                assert wr >= L.tsqr_mi_working_r_size_f64_lstsq(m, n, nrhs), (m, n, nrhs, wr)
                # the dense Gram pass leaves ntri tiles per workgroup of four waves on the R-only entry's second plan
                nt = (n + 15) // 16
                tiles = (m + 15) // 16
                tpw = max(1, (tiles + 2047) // 2048)
                nwaves = (tiles + tpw - 1) // tpw
                assert wr >= ((nwaves + 3) // 4) * (nt * (nt + 1) // 2) * 256, (m, n, nrhs, wr)
    assert len(wqs) == 1, "wq depends on m, n or nrhs"
    for m, n, nrhs in ((0, 4, 1), (4, 0, 1), (4, 4, 0), (0, 0, 0)):
        assert L.tsqr_mi_working_q_size_f64_lstsq_rank(m, n, nrhs) == 0 and L.tsqr_mi_working_r_size_f64_lstsq_rank(m, n, nrhs) == 0


def call(L, m=100, n=8, nrhs=3, lay=None, ld=None, refine=1, reorth=0, rcond=1e-8, null=()):
    """lay: {operand: layout} (column-major unless named); ld: {operand: leading dimension} (the smallest valid one unless named);
    null: the pointers passed as null (the others: SOME, and a host int for rank)"""
    lay = dict(lay or {})
    lds = {}
    for op, rows, cols in (("a", m, n), ("b", m, nrhs), ("r", n, n), ("x", n, nrhs)):
        lds[op] = max(cols if lay.get(op, COL) == ROW else rows, 1)
    lds.update(ld or {})
    host_rank = ctypes.c_int(-7)
    ptr = {name: (None if name in null else SOME) for name in POINTERS}
    ptr["rank"] = None if "rank" in null else ctypes.byref(host_rank)
    st = L.tsqr_mi_lstsq_rank_f64(lay.get("a", COL), lay.get("b", COL), reorth, refine, rcond, ptr["x"], lds["x"], ptr["r"], lds["r"],
                                  ptr["jpvt"], ptr["rank"], ptr["a"], lds["a"], ptr["b"], lds["b"], m, n, nrhs, ptr["wq"], ptr["wr"], None)
    assert host_rank.value == -7, "a rejected call wrote the rank"
    return st


N64 = "tsqr_mi_lstsq_rank_f64 supports n <= 64"
NRHS = "tsqr_mi_lstsq_rank_f64 supports nrhs <= 16"
REFINE = "tsqr_mi_lstsq_rank_f64 supports 0 <= refine <= 4"
RCOND = "tsqr_mi_lstsq_rank_f64 supports rcond < 1"


def state_cases():
    """(id, keyword arguments of call, state, substring of last_error or None -- None: a state 1 that must leave the text alone)"""
    m, n = 100, 8
    out = []
    for op in ("a", "b"):
        for bad in (2, -1):
            out.append(("layout_%s_%d" % (op, bad), dict(lay={op: bad}), BAD, None))
        out.append(("layout_%s_beyond_cap" % op, dict(m=74, n=65, lay={op: 2}), BAD, None))
    for pair in ((COL, COL), (ROW, ROW), (ROW, COL), (COL, ROW)):
        lay = dict(zip(("a", "b"), pair))
        tag = "".join("cr"[v] for v in pair)
        out.append(("n_above_m_" + tag, dict(m=4, n=8, lay=lay), BAD, None))
        out.append(("m_zero_" + tag, dict(m=0, n=4, lay=lay), BAD, None))
        out.append(("n_zero_" + tag, dict(m=4, n=0, lay=lay), BAD, None))
        out.append(("nrhs_zero_" + tag, dict(nrhs=0, lay=lay), BAD, None))
        extent = {"a": (m, n), "b": (m, 3), "r": (n, n), "x": (n, 3)}
        for op in "xrab":
            least = extent[op][1] if lay.get(op, COL) == ROW else extent[op][0]
            out.append(("ld%s_short_%s" % (op, tag), dict(lay=lay, ld={op: least - 1}), BAD, None))
        out.append(("cap_" + tag, dict(m=74, n=65, lay=lay, reorth=1), UNSUPPORTED, N64))
        out.append(("cap_with_short_lda_" + tag, dict(m=74, n=65, lay=lay, ld={"a": (65 if lay["a"] == ROW else 74) - 1}), BAD, None))
        out.append(("nrhs_17_" + tag, dict(lay=lay, nrhs=17), UNSUPPORTED, NRHS))
        out.append(("refine_5_" + tag, dict(lay=lay, refine=5), UNSUPPORTED, REFINE))
        out.append(("refine_negative_" + tag, dict(lay=lay, refine=-1), UNSUPPORTED, REFINE))
        out.append(("rcond_one_" + tag, dict(lay=lay, rcond=1.0), UNSUPPORTED, RCOND))
        out.append(("rcond_nan_" + tag, dict(lay=lay, rcond=NAN), UNSUPPORTED, RCOND))
    out.append(("rcond_two", dict(rcond=2.0), UNSUPPORTED, RCOND))
    out.append(("rcond_inf", dict(rcond=float("inf")), UNSUPPORTED, RCOND))
    # the order of the state 2 checks: the cap, nrhs, refine, rcond
    out.append(("cap_before_nrhs", dict(m=100, n=65, nrhs=17), UNSUPPORTED, N64))
    out.append(("nrhs_before_refine", dict(nrhs=17, refine=5), UNSUPPORTED, NRHS))
    out.append(("refine_before_rcond", dict(refine=5, rcond=1.0), UNSUPPORTED, REFINE))
    out.append(("size_before_rcond", dict(ld={"a": 99}, rcond=NAN), BAD, None))
    # each null pointer in turn, on arguments that would otherwise go on: state 1 at the first statement; and in front of every other check
    for name in POINTERS:
        out.append(("null_" + name, dict(null=(name,)), BAD, None))
        out.append(("null_%s_before_cap" % name, dict(m=74, n=65, null=(name,)), BAD, None))
        out.append(("null_%s_before_rcond" % name, dict(rcond=NAN, null=(name,)), BAD, None))
    out.append(("all_null", dict(null=POINTERS), BAD, None))
    out.append(("all_null_beyond_cap", dict(m=74, n=65, null=POINTERS), BAD, None))
    return out


CASES = [pytest.param(kw, state, text, id=cid) for cid, kw, state, text in state_cases()]


@pytest.mark.parametrize("kw,state,text", CASES)
def test_state_sweeps_and_text(bq, kw, state, text):
    """the rules tests/test_f64_entry_states.py holds the other entries to: the state, the sweep count cleared, a text of its own for every
    state 2 and the text left alone by a state 1"""
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
        assert text in bq.last_error() and text not in sentinel


def test_table_covers_what_the_entry_decides():
    ids = [c.id for c in CASES]
    assert len(set(ids)) == len(ids)
    for kind in ("n_above_m", "m_zero", "n_zero", "nrhs_zero", "lda_short", "ldb_short", "ldr_short", "ldx_short", "layout_a_2", "layout_b_-1",
                 "cap_", "nrhs_17", "refine_5", "refine_negative", "rcond_one", "rcond_nan", "all_null") + tuple("null_" + p for p in POINTERS):
        assert any(kind in i for i in ids), kind
    for tag in ("cc", "rr", "rc", "cr"):
        for op in "xrab":
            assert "ld%s_short_%s" % (op, tag) in ids


def test_lstsq_rank_f64_operand_checks(bq):
    import torch
    a = torch.zeros(100, 8, dtype=torch.float64)
    b = torch.zeros(100, 3, dtype=torch.float64)
    for bad in ((a.float(), b), (a, b.float()), (a.numpy(), b), (a, b)):       # (the last: CPU tensors of the right type)
        with pytest.raises(TypeError):
            bq.lstsq_rank_f64(*bad)
    if torch.cuda.is_available():                              # (the GPU box: shapes and states on device tensors; nothing is launched)
        a, b = a.cuda(), b.cuda()
        with pytest.raises(ValueError):
            bq.lstsq_rank_f64(a, b[:99])
        with pytest.raises(ValueError):
            bq.lstsq_rank_f64(a.reshape(-1), b)
        wide = torch.zeros(100, 65, dtype=torch.float64, device="cuda")
        many = torch.zeros(100, 17, dtype=torch.float64, device="cuda")
        for args, kw, state in (((a[:4], b[:4]), {}, BAD), ((wide, b), {}, UNSUPPORTED), ((a, many), {}, UNSUPPORTED),
                                ((a, b), dict(refine=5), UNSUPPORTED), ((a, b), dict(refine=-1), UNSUPPORTED),
                                ((a, b), dict(rcond=1.0), UNSUPPORTED), ((a, b), dict(rcond=NAN), UNSUPPORTED)):
            with pytest.raises(bq.LstsqRankError) as e:
                bq.lstsq_rank_f64(*args, **kw)
            assert e.value.state == state


# ---- the two test-library hooks of the CholeskyQR step: every call is rejected by the argument checks, which come before any HIP call ----
REJECTED = -100
c_sz, c_p, c_i = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int


@pytest.fixture(scope="module")
def T(bq):
    bq.lib()                                               # (torch's HIP runtime first, as every user of the libraries loads it)
    L = ctypes.CDLL(os.path.join(ROOT, "tsqr_gpu_amd", "csrc", "libtsqr_selftest.so"))
    sig = {
        "tsqr_selftest_f64_gramq_dense_lay": [c_i, c_p, c_p, c_sz, c_sz, c_i, c_p, c_p, c_sz, c_i],
        "tsqr_selftest_f64_lsq_rank_step": [c_p, c_p, c_p, c_p, c_i],
    }
    for name, args in sig.items():
        assert hasattr(L, name), name
        getattr(L, name).restype = c_i
        getattr(L, name).argtypes = args
    return L


def test_dense_gram_hook_rejects_before_any_launch(T):
    def hook(a_lay=0, lda=100, m=100, n=8, cap=1 << 20, nwaves=0, null=()):
        g, a, z, part = (None if name in null else SOME for name in ("gsum", "a", "z", "part"))
        return T.tsqr_selftest_f64_gramq_dense_lay(a_lay, g, a, lda, m, n, z, part, cap, nwaves)
    for bad in (dict(a_lay=2), dict(a_lay=-1), dict(m=0), dict(n=0), dict(n=65), dict(lda=99), dict(a_lay=1, lda=7), dict(cap=0),
                dict(cap=255), dict(nwaves=5, cap=511), dict(null=("gsum",)), dict(null=("a",)), dict(null=("z",)), dict(null=("part",)),
                dict(null=("gsum", "a", "z", "part"))):
        assert hook(**bad) == REJECTED, bad


def test_step_hook_rejects_before_any_launch(T):
    for n, g, k, z, st in ((0, SOME, SOME, SOME, SOME), (65, SOME, SOME, SOME, SOME), (-1, SOME, SOME, SOME, SOME), (8, None, SOME, SOME, SOME),
                           (8, SOME, None, SOME, SOME), (8, SOME, SOME, None, SOME), (8, SOME, SOME, SOME, None), (8, None, None, None, None)):
        assert T.tsqr_selftest_f64_lsq_rank_step(g, k, z, st, n) == REJECTED, n


def test_cpp_lstsq_rank_fp64_compiles_and_links(bq):
    with compile_and_link(os.path.join(ROOT, "tests", "cpp", "sample_fp64_lstsq_rank.cpp"), "sample_fp64_lstsq_rank") as exe:
        assert os.path.exists(exe)

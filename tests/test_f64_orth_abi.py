"""CPU tests of the fp64 block orthogonalisation entry (tsqr_mi_orth_f64): exported symbols and their signatures, work-space sizes, the
table of state-1 argument sets, the operand checks of the Python layer, the test-library hooks and a C++ caller of mtk::qr::orth_fp64
that compiles and links.  EVERY call in this file is rejected before a HIP call."""
import ctypes
import os

import pytest

from abi_util import compile_and_link, header_flat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("tsqr_mi_orth_f64", "tsqr_mi_working_q_size_f64_orth", "tsqr_mi_working_r_size_f64_orth")
BAD, COL, ROW = 1, 0, 1
HOOKS = ("tsqr_selftest_f64_orth_plan", "tsqr_selftest_f64_orth_gram", "tsqr_selftest_f64_orth_update", "tsqr_selftest_f64_orth_s")


def test_symbols_exported_with_the_stated_signatures(bq):
    L = ctypes.CDLL(bq.LIB_PATH)
    flat = header_flat()
    for sym in SYMBOLS:
        assert hasattr(L, sym), sym
        assert sym in bq.C_ABI_SYMBOLS, sym
    assert "size_t tsqr_mi_working_q_size_f64_orth(size_t m, size_t k, size_t n);" in flat
    assert "size_t tsqr_mi_working_r_size_f64_orth(size_t m, size_t k, size_t n);" in flat
    assert ("int tsqr_mi_orth_f64(int v_layout, int w_layout, int passes, int reorth, double* w, size_t ldw, double* s, size_t lds, "
            "double* r, size_t ldr, const double* v, size_t ldv, size_t m, size_t k, size_t n, void* wq, void* wr, void* stream);") in flat
    sz, vp, ci = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int
    assert bq.C_SIGNATURES["tsqr_mi_orth_f64"] == (ci, [ci, ci, ci, ci, vp, sz, vp, sz, vp, sz, vp, sz, sz, sz, sz, vp, vp, vp])
    assert bq.C_SIGNATURES["tsqr_mi_working_q_size_f64_orth"] == (sz, [sz, sz, sz])
    assert "After state 3, W, S and R are UNDEFINED" in flat and "Compare diag(R) with the column norms of W" in flat
    assert issubclass(bq.OrthError, bq._F64StateError)
    import inspect
    par = inspect.signature(bq.orth_f64_tensor).parameters
    assert list(par) == ["v", "w", "passes", "reorth", "overwrite_w", "stream"]
    assert par["passes"].default == 2 and par["reorth"].default is False and par["overwrite_w"].default is False
    sel = ctypes.CDLL(os.path.join(ROOT, "tsqr_gpu_amd", "csrc", "libtsqr_selftest.so"))
    for h in HOOKS:
        assert hasattr(sel, h), h
    assert not any(hasattr(L, h) for h in HOOKS), "the hooks belong to the test library only"


MS = (2, 15, 16, 17, 33, 130, 1000, 4099, 9211, 1 << 16, (1 << 16) + 1, 1 << 20, (1 << 20) + 1, 1 << 23)
KS = (1, 63, 64, 65, 130, 512, 1023, 1024)
NS = (1, 7, 16, 17, 33, 51, 64)


def test_working_sizes_are_monotone_and_cover_the_qr_entry(bq):
    L = bq.lib()
    size = {(m, k, n): (L.tsqr_mi_working_q_size_f64_orth(m, k, n), L.tsqr_mi_working_r_size_f64_orth(m, k, n))
            for m in MS for k in KS for n in NS}
    for (m, k, n), (wq, wr) in size.items():
        # what the n <= 64 QR entry needs inside, R of round 2 and the work copy of S
        assert wq >= L.tsqr_mi_working_q_size_f64(m, n) + 4096 + ((k + 63) // 64) * 64 * 16 * ((n + 15) // 16), (m, k, n)
        assert wr >= L.tsqr_mi_working_r_size_f64(m, n), (m, k, n)
        assert wr <= 4 << 20, (m, k, n)
    for axis, values in ((0, MS), (1, KS), (2, NS)):
        for key, (wq, wr) in size.items():
            i = values.index(key[axis])
            if i + 1 < len(values):
                nxt = list(key)
                nxt[axis] = values[i + 1]
                wq2, wr2 = size[tuple(nxt)]
                assert wq2 >= wq and wr2 >= wr, (key, tuple(nxt))
    assert len({wq for (m, k, n), (wq, _) in size.items() if k == 130}) == 1, "wq depends on m or n"
    for m, k, n in ((0, 4, 1), (4, 0, 1), (4, 4, 0), (0, 0, 0)):
        assert L.tsqr_mi_working_q_size_f64_orth(m, k, n) == 0 and L.tsqr_mi_working_r_size_f64_orth(m, k, n) == 0


def test_plan_partials_fit_the_working_size(bq):
    bq.lib()
    T = ctypes.CDLL(os.path.join(ROOT, "tsqr_gpu_amd", "csrc", "libtsqr_selftest.so"))
    T.tsqr_selftest_f64_orth_plan.restype = ctypes.c_int
    T.tsqr_selftest_f64_orth_plan.argtypes = [ctypes.c_size_t] * 3 + [ctypes.POINTER(ctypes.c_longlong)]
    L = bq.lib()
    out = (ctypes.c_longlong * 6)()
    for m in MS + (2061, 33000):
        for k in KS:
            for n in NS:
                if k + n > m:
                    assert T.tsqr_selftest_f64_orth_plan(m, k, n, out) == -100
                    continue
                assert T.tsqr_selftest_f64_orth_plan(m, k, n, out) == 0
                nt, kblocks, nslices, cps, nch, part = list(out)
                assert nt == (n + 15) // 16 and kblocks == (k + 63) // 64 and nch == (m + 15) // 16
                assert nslices >= 1 and (nslices - 1) * cps < nch <= nslices * cps, (m, k, n)      # every chunk once, no empty slice
                assert nslices * kblocks <= 1024
                assert part == nslices * kblocks * 64 * 16 * nt <= L.tsqr_mi_working_r_size_f64_orth(m, k, n), (m, k, n)
    assert T.tsqr_selftest_f64_orth_plan(33000, 70, 20, out) == 0 and out[2] >= 2      # the slices case of tests/pass_refs_f64_orth.py


def call(L, guard, m=1003, k=130, n=17, passes=2, lay=(COL, COL), ld=None, null=()):
    """tsqr_mi_orth_f64 with every operand the same guarded host word: a call that gets past the checks would fault, a rejected one
    must leave the word alone"""
    v_lay, w_lay = lay
    lds = {"w": n if w_lay == ROW else m, "s": k, "r": n, "v": k if v_lay == ROW else m}
    lds.update(ld or {})
    ptr = {name: (None if name in null else ctypes.addressof(guard)) for name in ("w", "s", "r", "v", "wq", "wr")}
    st = L.tsqr_mi_orth_f64(v_lay, w_lay, passes, 0, ptr["w"], max(lds["w"], 0), ptr["s"], max(lds["s"], 0), ptr["r"], max(lds["r"], 0),
                            ptr["v"], max(lds["v"], 0), m, k, n, ptr["wq"], ptr["wr"], None)
    assert guard.value == -7.5, "a rejected call wrote an operand"
    return st


STATE_ONE = [
    ("n-zero", dict(n=0)), ("n-65", dict(n=65)), ("n-1025", dict(n=1025, m=4096)), ("k-zero", dict(k=0)), ("k-1025", dict(k=1025, m=4096)),
    ("m-zero", dict(m=0)), ("k-plus-n-above-m", dict(m=146)), ("m-below-k", dict(m=100)), ("passes-0", dict(passes=0)),
    ("passes-3", dict(passes=3)), ("passes-negative", dict(passes=-1)), ("v-layout-2", dict(lay=(2, COL))), ("w-layout-2", dict(lay=(COL, 2))),
    ("v-layout-negative", dict(lay=(-1, COL))), ("ldw-below-m", dict(ld={"w": 1002})), ("ldv-below-m", dict(ld={"v": 1002})),
    ("lds-below-k", dict(ld={"s": 129})), ("ldr-below-n", dict(ld={"r": 16})), ("row-major-ldw-below-n", dict(lay=(COL, ROW), ld={"w": 16})),
    ("row-major-ldv-below-k", dict(lay=(ROW, COL), ld={"v": 129})), ("row-major-ldv-17", dict(lay=(ROW, ROW), ld={"v": 17})),
    ("null-w", dict(null=("w",))), ("null-s", dict(null=("s",))), ("null-r", dict(null=("r",))), ("null-v", dict(null=("v",))),
    ("null-wq", dict(null=("wq",))), ("null-wr", dict(null=("wr",))), ("all-null", dict(null=("w", "s", "r", "v", "wq", "wr"))),
]


@pytest.mark.parametrize("kw", [pytest.param(kw, id=cid) for cid, kw in STATE_ONE])
def test_state_one_before_any_launch(bq, kw):
    """state 1, the sweep count cleared, no text set, and no operand touched"""
    from tests.test_f64_entry_states import Z
    L = bq.lib()
    assert L.tsqr_mi_r_f64(0, Z, 65, Z, 100, 100, 65, Z, Z, Z) == 2        # a sentinel text from another entry's state 2
    sentinel = bq.last_error()
    guard = ctypes.c_double(-7.5)
    assert call(L, guard, **kw) == BAD
    assert L.tsqr_mi_last_sweeps_f64() == 0
    assert bq.last_error() == sentinel


def test_row_major_leading_dimensions_are_accepted_by_the_size_rules(bq):
    """the smallest legal leading dimensions pass every size rule in all four layout pairs: such a call stops only at a null operand"""
    L = bq.lib()
    guard = ctypes.c_double(-7.5)
    for lay in ((COL, COL), (COL, ROW), (ROW, COL), (ROW, ROW)):
        assert call(L, guard, lay=lay, null=("wr",)) == BAD
        assert call(L, guard, m=147, lay=lay, null=("wr",)) == BAD


def test_python_operand_checks(bq):
    m, k, n = 100, 20, 5
    a = 1 << 20
    ok = dict(w=(a, m * n), s=(a + 8 * m * n, k * n), r=(a + 8 * (m * n + k * n), n * n), v=(a + 8 * (m * n + k * n + n * n), m * k))
    chk = lambda ldw=m, lds=k, ldr=n, ldv=m, vrm=False, wrm=False, **over: bq.check_f64_orth_operands(
        m, k, n, ldw, lds, ldr, ldv, *(over.get(x, ok[x]) for x in ("w", "s", "r", "v")), v_row_major=vrm, w_row_major=wrm)
    chk()
    chk(ldw=n, ldv=k, vrm=True, wrm=True)
    for kw in (dict(ldw=m - 1), dict(lds=k - 1), dict(ldr=n - 1), dict(ldv=m - 1), dict(ldw=n - 1, wrm=True), dict(ldv=k - 1, vrm=True),
               dict(w=(a, m * n - 1)), dict(v=(ok["v"][0], m * k - 1)), dict(s=(ok["s"][0], k * n - 1)), dict(r=(ok["r"][0], n * n - 1)),
               dict(ldw=m + 1), dict(ldv=m + 1)):
        with pytest.raises(ValueError):
            chk(**kw)
    for x, y in (("w", "v"), ("w", "s"), ("w", "r"), ("s", "r")):
        with pytest.raises(ValueError, match="overlaps"):
            chk(**{y: (ok[x][0] + 8, ok[y][1])})
    import torch
    v, w = torch.zeros(m, k, dtype=torch.float64), torch.zeros(m, n, dtype=torch.float64)
    for bad in ((v.float(), w), (v, w.float()), (v, w)):                      # (the last: CPU tensors of the right type)
        with pytest.raises(TypeError):
            bq.orth_f64_tensor(*bad)
    if torch.cuda.is_available():                              # (the GPU box: shapes and states on device tensors; nothing is launched)
        v, w = v.cuda(), w.cuda()
        with pytest.raises(ValueError):
            bq.orth_f64_tensor(v, w[:50])
        for args, kw in (((v, torch.zeros(m, 65, dtype=torch.float64, device="cuda")), {}), ((v, w), dict(passes=3)),
                         ((v[:24], w[:24]), {})):
            with pytest.raises(bq.OrthError) as e:
                bq.orth_f64_tensor(*args, **kw)
            assert e.value.state == BAD


REJECTED = -100
c_p, c_i, c_z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t


def test_hooks_reject_before_any_launch(bq):
    bq.lib()                                               # (torch's HIP runtime first, as every user of the libraries loads it)
    T = ctypes.CDLL(os.path.join(ROOT, "tsqr_gpu_amd", "csrc", "libtsqr_selftest.so"))
    sig = {"tsqr_selftest_f64_orth_gram": [c_i, c_i, c_p, c_p, c_z, c_p, c_z, c_z, c_i, c_i, c_p, c_z],
           "tsqr_selftest_f64_orth_update": [c_i, c_i, c_p, c_z, c_p, c_z, c_p, c_z, c_i, c_i],
           "tsqr_selftest_f64_orth_s": [c_p, c_z, c_p, c_p, c_z, c_i, c_i, c_i]}
    for name, args in sig.items():
        getattr(T, name).restype, getattr(T, name).argtypes = c_i, args
    some = ctypes.addressof(ctypes.c_double(0.0))
    m, k, n = 1003, 130, 17
    for vl, xl, ldv, ldx, mm, kk, nn in ((2, 0, m, m, m, k, n), (0, 2, m, m, m, k, n), (0, 0, m - 1, m, m, k, n), (0, 0, m, m - 1, m, k, n),
                                         (1, 1, k - 1, n, m, k, n), (1, 1, k, n - 1, m, k, n), (0, 0, m, m, m, k, 65), (0, 0, m, m, m, 1025, n),
                                         (0, 0, 146, 146, 146, k, n), (0, 0, m, m, m, 0, n), (0, 0, m, m, m, k, 0)):
        assert T.tsqr_selftest_f64_orth_gram(vl, xl, some, some, ldv, some, ldx, mm, kk, nn, some, 1 << 30) == REJECTED
        assert T.tsqr_selftest_f64_orth_update(vl, xl, some, ldx, some, ldv, some, mm, kk, nn) == REJECTED
    assert T.tsqr_selftest_f64_orth_gram(0, 0, some, some, m, some, m, m, k, n, some, 16) == REJECTED          # no room for the partials
    assert T.tsqr_selftest_f64_orth_gram(0, 0, None, some, m, some, m, m, k, n, some, 1 << 30) == REJECTED
    assert T.tsqr_selftest_f64_orth_update(0, 0, None, m, some, m, some, m, k, n) == REJECTED
    for args in ((None, k, some, some, n, k, n, 1), (some, k - 1, some, some, n, k, n, 0), (some, k, some, None, n, k, n, 1),
                 (some, k, some, some, n - 1, k, n, 1), (some, k, some, some, n, k, 65, 0), (some, k, some, some, n, 1025, n, 0),
                 (some, k, some, some, n, k, n, 2), (some, k, None, some, n, k, n, 0)):
        assert T.tsqr_selftest_f64_orth_s(*args) == REJECTED, args


def test_cpp_orth_fp64_compiles_links_and_checks_its_arguments(bq):
    import subprocess
    with compile_and_link(os.path.join(ROOT, "tests", "cpp", "sample_fp64_orth.cpp"), "sample_fp64_orth") as exe:
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "argument checks ok" in out.stdout

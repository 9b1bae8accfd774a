"""CPU test of what every fp64 entry decides before it touches the device: the returned state, the sweep count and the
tsqr_mi_last_error text, one table over the eight single-GPU entries and the two row-partitioned ones that take their transport as
pointers.  Every call passes null pointers (so q == a in the QR entries, and the row-partitioned entries have no all-reduce), and every
case ends at a check: nothing here reaches a HIP call.

The order of the checks is contract (include/tsqr_mi.h): layouts, sizes and leading dimensions (state 1, no text), the column cap
(state 2 with the entry's text), for least squares nrhs and then refine (state 2), the in-place rule of the QR entries (state 1).  The
row-partitioned entries differ: their size check sets a text, m_local < n is allowed, there is no in-place rule, and a call that passes
the size checks without an all-reduce ends in state 2.

The sweep count is asserted to be 0 after every call, but a process without a GPU never sets it to anything else: the assertion
cannot tell whether an entry still clears it."""
import ctypes

import pytest

COL, ROW = 0, 1
BAD, UNSUPPORTED = 1, 2
Z = ctypes.c_void_p(0)
NEEDS_ALLREDUCE = "tsqr_mi_qr_f64_dist needs an all-reduce"
DIST_SIZES = "tsqr_mi_qr_f64_dist: m_local >= 1, n >= 1, ldq >= m_local, lda >= m_local and ldr >= n are required"


class Entry:
    """symbol; kind: which argument list; nlay: leading layout arguments; cap and the text of n > cap"""

    def __init__(self, symbol, kind, nlay, cap, cap_text):
        self.symbol, self.kind, self.nlay, self.cap, self.cap_text = symbol, kind, nlay, cap, cap_text
        self.dist = kind.startswith("dist")
        # the operands that have a layout argument in the _lay form, in the order of those arguments, and each one's column count
        self.laid = {"qr": ("a", "q"), "r": ("a",), "lstsq": ("a", "b")}.get(kind, ("a", "q"))

    def call(self, L, m, n, lay=None, ld=None, nrhs=3, refine=1, reorth=0):
        """lay: {operand: layout} (column-major unless named); ld: {operand: leading dimension} (the smallest valid one unless named)"""
        lay = dict(lay or {})
        lds = {}
        for op, rows, cols in (("a", m, n), ("q", m, n), ("b", m, nrhs), ("r", n, n), ("x", n, nrhs)):
            lds[op] = max(cols if lay.get(op, COL) == ROW else rows, 1)
        lds.update(ld or {})
        head = [lay.get(op, COL) for op in self.laid[:self.nlay]]
        assert self.nlay or not lay, "a layout for an entry without layout arguments"
        fn = getattr(L, self.symbol)
        if self.kind == "qr":
            return fn(*head, reorth, Z, lds["q"], Z, lds["r"], Z, lds["a"], m, n, Z, Z, Z)
        if self.kind == "r":
            return fn(*head, reorth, Z, lds["r"], Z, lds["a"], m, n, Z, Z, Z)
        if self.kind == "lstsq":
            return fn(*head, reorth, refine, Z, lds["x"], Z, lds["r"], Z, lds["a"], Z, lds["b"], m, n, nrhs, Z, Z, Z)
        return fn(reorth, Z, lds["q"], Z, lds["r"], Z, lds["a"], m, n, Z, Z, Z, Z, 2, Z)      # (dist_cb / dist_fn: transport null, 2 ranks)


QR64 = "tsqr_mi_qr_f64 supports n <= 64"
WIDE = "tsqr_mi_qr_f64_wide supports n <= 1024"
ENTRIES = [
    Entry("tsqr_mi_qr_f64", "qr", 0, 64, QR64), Entry("tsqr_mi_qr_f64_lay", "qr", 2, 64, QR64),
    Entry("tsqr_mi_qr_f64_wide", "qr", 0, 1024, WIDE), Entry("tsqr_mi_qr_f64_wide_lay", "qr", 2, 1024, WIDE),
    Entry("tsqr_mi_r_f64", "r", 0, 64, "tsqr_mi_r_f64 supports n <= 64"), Entry("tsqr_mi_r_f64_lay", "r", 1, 64, "tsqr_mi_r_f64 supports n <= 64"),
    Entry("tsqr_mi_lstsq_f64", "lstsq", 0, 64, "tsqr_mi_lstsq_f64 supports n <= 64"),
    Entry("tsqr_mi_lstsq_f64_lay", "lstsq", 2, 64, "tsqr_mi_lstsq_f64 supports n <= 64"),
    Entry("tsqr_mi_qr_f64_dist_cb", "dist_cb", 0, 1024, "tsqr_mi_qr_f64_dist supports n <= 1024"),
    Entry("tsqr_mi_qr_f64_dist_fn", "dist_fn", 0, 1024, "tsqr_mi_qr_f64_dist supports n <= 1024"),
]


def cases_of(e):
    """(id, keyword arguments of Entry.call, state, substring of last_error or None) -- None: a state 1 that must leave the text alone"""
    m, n = (300, 100) if e.cap > 64 else (100, 8)
    sizes = DIST_SIZES if e.dist else None                  # (the row-partitioned size check is the one state 1 with a text)
    # a call that passes every check it meets up to the in-place rule: single-GPU QR entries end there only when the rule is broken, so
    # their cases below always break an earlier check or that one; the others need no such care
    out = []
    layouts = [{}]
    if e.nlay:
        ops = e.laid[:e.nlay]
        layouts = [dict(zip(ops, pair)) for pair in ([(COL,) * len(ops), (ROW,) * len(ops)] + ([(ROW, COL), (COL, ROW)] if len(ops) == 2 else []))]
        for op in ops:                                      # 1. a layout that is neither: before the sizes and before the cap
            for bad in (2, -1):
                out.append(("layout_%s_%d" % (op, bad), dict(m=m, n=n, lay={op: bad}), BAD, None))
            out.append(("layout_%s_beyond_cap" % op, dict(m=e.cap + 10, n=e.cap + 1, lay={op: 2}), BAD, None))
    for lay in layouts:
        tag = "".join("cr"[v] for v in lay.values()) or "c"
        # 2. n > m, and 3. m = 0 (the row-partitioned entries allow a block lower than it is wide)
        if e.dist:
            out.append(("n_above_m_" + tag, dict(m=4, n=8), UNSUPPORTED, NEEDS_ALLREDUCE))
        else:
            out.append(("n_above_m_" + tag, dict(m=4, n=8, lay=lay), BAD, None))
        out.append(("m_zero_" + tag, dict(m=0, n=4, lay=lay), BAD, sizes))
        out.append(("n_zero_" + tag, dict(m=4, n=0, lay=lay), BAD, sizes))
        # 4. each leading dimension one below its minimum
        operands = {"qr": "qra", "r": "ra", "lstsq": "xrab"}.get(e.kind, "qra")
        extent = {"a": (m, n), "q": (m, n), "b": (m, 3), "r": (n, n), "x": (n, 3)}
        for op in operands:
            least = extent[op][1] if lay.get(op, COL) == ROW else extent[op][0]
            out.append(("ld%s_short_%s" % (op, tag), dict(m=m, n=n, lay=lay, ld={op: least - 1}), BAD, sizes))
        # 5. n one above the cap: behind the sizes, in front of everything else
        out.append(("cap_" + tag, dict(m=e.cap + 10, n=e.cap + 1, lay=lay, reorth=1), UNSUPPORTED, e.cap_text))
        out.append(("cap_with_short_lda_" + tag, dict(m=e.cap + 10, n=e.cap + 1, lay=lay,
                                                      ld={"a": (e.cap + 1 if lay.get("a", COL) == ROW else e.cap + 10) - 1}), BAD, sizes))
        if e.kind == "lstsq":                               # nrhs, then refine, both behind the cap
            out.append(("nrhs_17_" + tag, dict(m=m, n=n, lay=lay, nrhs=17), UNSUPPORTED, "tsqr_mi_lstsq_f64 supports nrhs <= 16"))
            out.append(("refine_5_" + tag, dict(m=m, n=n, lay=lay, refine=5), UNSUPPORTED, "tsqr_mi_lstsq_f64 supports 0 <= refine <= 4"))
            out.append(("refine_negative_" + tag, dict(m=m, n=n, lay=lay, refine=-1), UNSUPPORTED, "tsqr_mi_lstsq_f64 supports 0 <= refine <= 4"))
            out.append(("nrhs_17_and_refine_5_" + tag, dict(m=m, n=n, lay=lay, nrhs=17, refine=5), UNSUPPORTED, "nrhs <= 16"))
            out.append(("cap_before_nrhs_" + tag, dict(m=100, n=65, lay=lay, nrhs=17), UNSUPPORTED, e.cap_text))
            out.append(("nrhs_zero_" + tag, dict(m=m, n=n, lay=lay, nrhs=0), BAD, None))
        # 6. q == a (both null) with unequal strides, the last check; the cap comes before it
        if e.kind == "qr":
            stride = {"q": (n if lay.get("q", COL) == ROW else m) + 1}
            if lay.get("q", COL) == lay.get("a", COL):
                out.append(("in_place_strides_" + tag, dict(m=m, n=n, lay=lay, ld=stride), BAD, None))
                if e.cap > 64:                              # (the wide entry decides it itself before it forwards n <= 64)
                    out.append(("in_place_strides_one_panel_" + tag, dict(m=100, n=8, lay=lay, ld={"q": (8 if lay.get("q", COL) == ROW else 100) + 1}), BAD, None))
            else:                                           # unequal layouts (equal strides where the two minima allow it)
                big = max(m, n)
                out.append(("in_place_layouts_" + tag, dict(m=m, n=n, lay=lay, ld={"q": big, "a": big}), BAD, None))
            out.append(("cap_before_in_place_" + tag, dict(m=e.cap + 10, n=e.cap + 1, lay=lay, ld={"q": e.cap + 11, "a": e.cap + 12}),
                        UNSUPPORTED, e.cap_text))
        if e.dist:                                          # no in-place rule: the call goes on to the transport check
            out.append(("in_place_strides_" + tag, dict(m=m, n=n, ld={"q": m + 1}), UNSUPPORTED, NEEDS_ALLREDUCE))
            out.append(("cap_before_transport_" + tag, dict(m=4, n=1025), UNSUPPORTED, e.cap_text))
    return out


CASES = [pytest.param(e, kw, state, text, id="%s-%s" % (e.symbol, cid)) for e in ENTRIES for cid, kw, state, text in cases_of(e)]


@pytest.mark.parametrize("entry,kw,state,text", CASES)
def test_entry_state_sweeps_and_text(bq, entry, kw, state, text):
    L = bq.lib()
    # a sentinel text from another entry's state 2, set just before the call
    if entry.kind == "r":
        assert L.tsqr_mi_qr_f64(0, Z, 100, Z, 65, Z, 100, 100, 65, Z, Z, Z) == UNSUPPORTED
    else:
        assert L.tsqr_mi_r_f64(0, Z, 65, Z, 100, 100, 65, Z, Z, Z) == UNSUPPORTED
    sentinel = bq.last_error()
    assert "supports n <= 64" in sentinel and entry.cap_text not in sentinel
    assert entry.call(L, **kw) == state
    assert L.tsqr_mi_last_sweeps_f64() == 0
    if text is None:
        assert state == BAD and bq.last_error() == sentinel        # (an invalid size of a single-GPU entry sets no text)
    else:
        assert text in bq.last_error() and text not in sentinel


def test_table_covers_every_entry_and_kind_of_case():
    ids = [c.id for c in CASES]
    assert len(set(ids)) == len(ids)
    for e in ENTRIES:
        mine = [i for i in ids if i.startswith(e.symbol + "-")]
        for kind in ("n_above_m", "m_zero", "lda_short", "ldr_short", "cap_"):
            assert any(kind in i for i in mine), (e.symbol, kind)
        assert any("layout_" in i for i in mine) == bool(e.nlay)
        if e.kind == "qr":
            assert any("in_place_strides" in i for i in mine) and any("in_place_layouts" in i for i in mine) == (e.nlay == 2)
        if e.kind == "lstsq":
            assert any("nrhs_17" in i for i in mine) and any("refine_5" in i for i in mine)

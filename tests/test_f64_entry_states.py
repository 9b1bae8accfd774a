"""CPU test of what every fp64 entry decides before it touches the device: the returned state, the sweep count and the
tsqr_mi_last_error text, one table over the ten single-GPU entries and the two row-partitioned ones that take their transport as
pointers.  Every call passes null pointers (so q == a in the QR entries, and the row-partitioned entries have no all-reduce; the one
exception is the SVD's v, whose ldv counts only when v is not null: an address that is never followed), and every case ends at a
check: nothing here reaches a HIP call.

The order of the checks is contract (include/tsqr_mi.h): layouts, sizes and leading dimensions (state 1, no text), the column cap
(state 2 with the entry's text), for least squares nrhs and then refine (state 2), the in-place rule of the QR entries (state 1).  The
row-partitioned entries differ: their size check sets a text, m_local < n is allowed, there is no in-place rule, and a call that passes
the size checks without an all-reduce ends in state 2.  The entries with a job flag (SVD, pivoted QR) reject a flag other than 0 or 1
first of all (state 1, no text); with the flag 0 the layout and the leading dimension of Q / U are not looked at and there is no
in-place rule, so a job = 0 case that is to show what is ignored ends at the cap, the last check there is.

The sweep count is asserted to be 0 after every call, but a process without a GPU never sets it to anything else: the assertion
cannot tell whether an entry still clears it."""
import ctypes

import pytest

COL, ROW = 0, 1
BAD, UNSUPPORTED = 1, 2
Z = ctypes.c_void_p(0)
SOME = ctypes.c_void_p(64)                                  # (the SVD's v where ldv is to count: never followed)
NEEDS_ALLREDUCE = "tsqr_mi_qr_f64_dist needs an all-reduce"
DIST_SIZES = "tsqr_mi_qr_f64_dist: m_local >= 1, n >= 1, ldq >= m_local, lda >= m_local and ldr >= n are required"


class Entry:
    """symbol; kind: which argument list; nlay: leading layout arguments; cap and the text of n > cap; small: the n x n result that
    has a leading dimension (r; the SVD's v)"""

    def __init__(self, symbol, kind, nlay, cap, cap_text, small="r"):
        self.symbol, self.kind, self.nlay, self.cap, self.cap_text, self.small = symbol, kind, nlay, cap, cap_text, small
        self.dist = kind.startswith("dist")
        # the operands that have a layout argument in the _lay form, in the order of those arguments, and each one's column count
        self.laid = {"qr": ("a", "q"), "r": ("a",), "lstsq": ("a", "b")}.get(kind, ("a", "q"))

    def call(self, L, m, n, lay=None, ld=None, nrhs=3, refine=1, reorth=0, job=1, v_null=False):
        """lay: {operand: layout} (column-major unless named); ld: {operand: leading dimension} (the smallest valid one unless named);
        job, v_null: the job flag of the "job" kind, and the SVD's v null, so that ldv does not count"""
        lay = dict(lay or {})
        lds = {}
        for op, rows, cols in (("a", m, n), ("q", m, n), ("b", m, nrhs), ("r", n, n), ("v", n, n), ("x", n, nrhs)):
            lds[op] = max(cols if lay.get(op, COL) == ROW else rows, 1)
        lds.update(ld or {})
        head = [lay.get(op, COL) for op in self.laid[:self.nlay]]
        assert self.nlay or not lay, "a layout for an entry without layout arguments"
        fn = getattr(L, self.symbol)
        if self.kind == "qr":
            return fn(*head, reorth, Z, lds["q"], Z, lds["r"], Z, lds["a"], m, n, Z, Z, Z)
        if self.kind == "r":
            return fn(*head, reorth, Z, lds["r"], Z, lds["a"], m, n, Z, Z, Z)
        if self.kind == "job" and self.small == "v":        # (a, u layouts, jobu, reorth, u, ldu, s, v, ldv, a, lda, ...)
            return fn(*head, job, reorth, Z, lds["q"], Z, Z if v_null else SOME, lds["v"], Z, lds["a"], m, n, Z, Z, Z)
        if self.kind == "job":                              # (a, q layouts, jobq, reorth, q, ldq, r, ldr, jpvt, a, lda, ...)
            return fn(*head, job, reorth, Z, lds["q"], Z, lds["r"], Z, Z, lds["a"], m, n, Z, Z, Z)
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
    Entry("tsqr_mi_svd_f64", "job", 2, 64, "tsqr_mi_svd_f64 supports n <= 64", small="v"),
    Entry("tsqr_mi_qrcp_f64", "job", 2, 64, "tsqr_mi_qrcp_f64 supports n <= 64"),
    Entry("tsqr_mi_qr_f64_dist_cb", "dist_cb", 0, 1024, "tsqr_mi_qr_f64_dist supports n <= 1024"),
    Entry("tsqr_mi_qr_f64_dist_fn", "dist_fn", 0, 1024, "tsqr_mi_qr_f64_dist supports n <= 1024"),
]


def cases_of(e):
    """(id, keyword arguments of Entry.call, state, substring of last_error or None) -- None: a state 1 that must leave the text alone"""
    if e.kind == "job":
        return job_cases_of(e)
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


def job_cases_of(e):
    """cases_of for an entry with a job flag.  job = 1: the families of the "qr" kind, with the entry's small operand in r's place.
    job = 0: q (u) is not used, so only a's layout and the leading dimensions of a and of the small operand can end a call in state 1."""
    m, n, sm = 100, 8, e.small
    big_m, big_n = e.cap + 10, e.cap + 1
    least = lambda op, lay, mm, nn: nn if op in "aq" and lay.get(op, COL) == ROW else (mm if op in "aq" else nn)
    out = []
    for bad in (2, -1):                                     # 0. the job flag: before everything else, the cap included
        out.append(("job_flag_%d" % bad, dict(m=m, n=n, job=bad), BAD, None))
        out.append(("job_flag_%d_beyond_cap" % bad, dict(m=big_m, n=big_n, job=bad), BAD, None))
        out.append(("job_flag_%d_bad_layout" % bad, dict(m=m, n=n, job=bad, lay={"a": 2}), BAD, None))
    for job in (1, 0):
        j = "job%d_" % job
        for op in ("a", "q") if job else ("a",):            # 1. a layout that is neither: before the sizes and before the cap
            for bad in (2, -1):
                out.append((j + "layout_%s_%d" % (op, bad), dict(m=m, n=n, job=job, lay={op: bad}), BAD, None))
            out.append((j + "layout_%s_beyond_cap" % op, dict(m=big_m, n=big_n, job=job, lay={op: 2}), BAD, None))
        pairs = [(COL, COL), (ROW, ROW), (ROW, COL), (COL, ROW)] if job else [(COL, COL), (ROW, COL)]
        for lay in (dict(zip(("a", "q"), pair)) for pair in pairs):
            tag = "".join("cr"[v] for v in lay.values())
            out.append((j + "n_above_m_" + tag, dict(m=4, n=8, job=job, lay=lay), BAD, None))         # 2., 3.
            out.append((j + "m_zero_" + tag, dict(m=0, n=4, job=job, lay=lay), BAD, None))
            out.append((j + "n_zero_" + tag, dict(m=4, n=0, job=job, lay=lay), BAD, None))
            for op in ("q", sm, "a") if job else (sm, "a"):  # 4. each leading dimension that counts one below its minimum
                out.append((j + "ld%s_short_%s" % (op, tag), dict(m=m, n=n, job=job, lay=lay, ld={op: least(op, lay, m, n) - 1}), BAD, None))
            # 5. n one above the cap: behind the sizes, in front of the in-place rule
            out.append((j + "cap_" + tag, dict(m=big_m, n=big_n, job=job, lay=lay, reorth=1), UNSUPPORTED, e.cap_text))
            out.append((j + "cap_with_short_lda_" + tag, dict(m=big_m, n=big_n, job=job, lay=lay, ld={"a": least("a", lay, big_m, big_n) - 1}),
                        BAD, None))
            if job:                                         # 6. q == a (both null) with unequal strides or layouts, the last check
                if lay["q"] == lay["a"]:
                    out.append((j + "in_place_strides_" + tag, dict(m=m, n=n, job=1, lay=lay, ld={"q": least("q", lay, m, n) + 1}), BAD, None))
                else:
                    out.append((j + "in_place_layouts_" + tag, dict(m=m, n=n, job=1, lay=lay, ld={"q": m, "a": m}), BAD, None))
                out.append((j + "cap_before_in_place_" + tag, dict(m=big_m, n=big_n, job=1, lay=lay, ld={"q": big_m + 1, "a": big_m + 2}),
                            UNSUPPORTED, e.cap_text))
            else:                                           # q's layout and ldq are not looked at: the call goes on to the cap
                out.append((j + "layout_q_ignored_" + tag, dict(m=big_m, n=big_n, job=0, lay=dict(lay, q=2)), UNSUPPORTED, e.cap_text))
                out.append((j + "ldq_short_ignored_" + tag, dict(m=big_m, n=big_n, job=0, lay=lay, ld={"q": 0}), UNSUPPORTED, e.cap_text))
        if sm == "v":                                       # ldv counts only when v is not null
            out.append((j + "ldv_short_beyond_cap", dict(m=big_m, n=big_n, job=job, ld={"v": big_n - 1}), BAD, None))
            out.append((j + "ldv_short_v_null_goes_on_to_cap", dict(m=big_m, n=big_n, job=job, ld={"v": big_n - 1}, v_null=True),
                        UNSUPPORTED, e.cap_text))
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
    if entry.small == "v":
        assert L.tsqr_mi_last_jacobi_sweeps_f64() == 0
    if text is None:
        assert state == BAD and bq.last_error() == sentinel        # (an invalid size of a single-GPU entry sets no text)
    else:
        assert text in bq.last_error() and text not in sentinel


def test_table_covers_every_entry_and_kind_of_case():
    ids = [c.id for c in CASES]
    assert len(set(ids)) == len(ids)
    for e in ENTRIES:
        mine = [i for i in ids if i.startswith(e.symbol + "-")]
        for kind in ("n_above_m", "m_zero", "lda_short", "ld%s_short" % e.small, "cap_"):
            assert any(kind in i for i in mine), (e.symbol, kind)
        assert any("layout_" in i for i in mine) == bool(e.nlay)
        if e.kind == "qr":
            assert any("in_place_strides" in i for i in mine) and any("in_place_layouts" in i for i in mine) == (e.nlay == 2)
        if e.kind == "lstsq":
            assert any("nrhs_17" in i for i in mine) and any("refine_5" in i for i in mine)
        if e.kind == "job":
            for job in ("job1_", "job0_"):
                for kind in ("layout_a", "n_above_m", "m_zero", "n_zero", "lda_short", "ld%s_short" % e.small, "cap_"):
                    assert any(job + kind in i for i in mine), (e.symbol, job, kind)
            for kind in ("job_flag_2", "job_flag_-1", "job_flag_2_beyond_cap", "job_flag_-1_beyond_cap", "job1_layout_q", "job1_ldq_short",
                         "job1_in_place_strides", "job1_in_place_layouts", "job1_cap_before_in_place", "job0_layout_q_ignored",
                         "job0_ldq_short_ignored"):
                assert any(kind in i for i in mine), (e.symbol, kind)
            assert not any("job0_in_place" in i for i in mine)
            assert any("v_null" in i for i in mine) == (e.small == "v")

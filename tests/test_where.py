"""Value predicates on the host (no GPU): Where.keeps and tests/where_model.py pinned by hand-written
vectors, the constructor's argument checks, the struct against the header, and every MTBLX_E_INVAL of
the C calls, which are all refused before any device call."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import where_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = (1 << 64) - 1


def u64(*xs):
    return b"".join((x & M).to_bytes(8, "little") for x in xs)


# ---------------------------------------------------------------- 1. Where.keeps by hand
def test_u64le_one_field():
    from mtblx import Where
    w = Where(1, [(0, 10, 20)])
    assert [w.keeps(u64(x)) for x in (9, 10, 15, 20, 21, 0, M)] == [False, True, True, True, False, False, False]
    assert w.keeps(b"") is None and w.keeps(u64(15)[:7]) is None and w.keeps(u64(15) + b"\0") is None
    assert w.keeps(u64(15, 15)) is None
    o = Where(1, [(0, 10, 20, "outside")])
    assert [o.keeps(u64(x)) for x in (9, 10, 20, 21)] == [True, False, False, True]
    assert o.keeps(b"1234567") is None
    assert Where(1, [(0, 10, 20, "inside")]) == w


def test_u64le_three_fields():
    from mtblx import Where
    # (count, time_first, time_last): count >= 5 and time_last >= 1000
    w = Where(3, [(0, 5, None), (2, 1000, None)])
    assert w.keeps(u64(5, 0, 1000)) is True
    assert w.keeps(u64(4, 0, 1000)) is False
    assert w.keeps(u64(5, 0, 999)) is False
    assert w.keeps(u64(M, M, M)) is True
    assert w.keeps(u64(5, 0)) is None and w.keeps(u64(5, 0, 1000, 1)) is None
    a = Where(3, [(0, 5, None), (2, 1000, None)], mode="any")
    assert a.keeps(u64(4, 0, 1000)) is True and a.keeps(u64(5, 0, 999)) is True
    assert a.keeps(u64(4, 7, 999)) is False
    assert a.keeps(b"x" * 23) is None
    # field 1 is not constrained: its value never matters
    assert w.keeps(u64(5, M, 1000)) is True and a.keeps(u64(4, M, 999)) is False


def test_bounds_at_the_ends_and_points():
    from mtblx import Where
    assert Where(1, [(0, None, None)]).keeps(u64(0)) is True and Where(1, [(0, None, None)]).keeps(u64(M)) is True
    assert Where(1, [(0, 0, 0)]).keeps(u64(0)) is True and Where(1, [(0, 0, 0)]).keeps(u64(1)) is False
    assert Where(1, [(0, M, M)]).keeps(u64(M)) is True and Where(1, [(0, M, M)]).keeps(u64(M - 1)) is False
    p = Where(1, [(0, 1 << 63, 1 << 63)])                   # lo == hi, above the signed range: unsigned compares
    assert [p.keeps(u64(x)) for x in ((1 << 63) - 1, 1 << 63, (1 << 63) + 1)] == [False, True, False]
    assert Where(1, [(0, 1 << 63, None)]).keeps(u64(5)) is False
    assert Where(1, [(0, None, (1 << 63) - 1)]).keeps(u64(1 << 63)) is False


def test_lo_above_hi_is_an_empty_range():
    from mtblx import Where
    e = Where(1, [(0, 20, 10)])
    assert [e.keeps(u64(x)) for x in (0, 10, 15, 20, M)] == [False] * 5
    o = Where(1, [(0, 20, 10, "outside")])
    assert [o.keeps(u64(x)) for x in (0, 10, 15, 20, M)] == [True] * 5
    assert e.keeps(b"") is None and o.keeps(b"") is None    # a bad value stays bad


def test_no_clause():
    from mtblx import Where
    assert Where(2).keeps(u64(1, 2)) is True                # all of nothing
    assert Where(2, mode="any").keeps(u64(1, 2)) is False   # some of nothing
    assert Where(2).keeps(u64(1)) is None and Where(2, mode="any").keeps(u64(1)) is None


def test_varint_vectors():
    from mtblx import Where
    w1 = Where(1, [(0, 5, None)], encoding="varint")
    assert w1.keeps(b"\x05") is True and w1.keeps(b"\x04") is False
    ten = b"\xff" * 9 + b"\x01"                             # a 10-byte field: 2^64 - 1
    assert Where(1, [(0, M, M)], encoding="varint").keeps(ten) is True
    over = b"\xff" * 9 + b"\x7f"                            # the tenth byte holds bits above 2^64: dropped
    assert Where(1, [(0, M, M)], encoding="varint").keeps(over) is True
    hi = b"\x80" * 9 + b"\x02"                              # only a bit above 2^64: reads as 0
    assert Where(1, [(0, 0, 0)], encoding="varint").keeps(hi) is True
    assert Where(1, [(0, 0, 0)], encoding="varint").keeps(b"\x80\x00") is True     # non-canonical zero
    assert Where(1, [(0, 1, 1)], encoding="varint").keeps(b"\x81\x80\x00") is True   # non-canonical one
    assert w1.keeps(b"\x85") is None                        # unterminated at the value's end
    assert w1.keeps(b"\xff" * 10) is None                   # unterminated within 10 bytes
    assert w1.keeps(b"\xff" * 10 + b"\x01") is None         # an 11-byte field
    assert w1.keeps(b"\x05\x00") is None                    # a byte left over
    assert w1.keeps(b"") is None                            # the empty value
    w3 = Where(3, [(0, 2, 3), (2, 300, None)], encoding="varint")
    assert w3.keeps(b"\x02\x00\xac\x02") is True            # (2, 0, 300)
    assert w3.keeps(b"\x02\x00\xab\x02") is False           # (2, 0, 299)
    assert w3.keeps(b"\x04\x00\xac\x02") is False
    assert w3.keeps(b"\x02\x00") is None and w3.keeps(b"\x02\x00\xac") is None
    assert w3.keeps(b"\x02\x00\xac\x02\x00") is None
    assert w3.keeps(u64(2, 0, 300)) is None                 # 24 bytes are not three varints here


def test_keeps_agrees_with_reduce_decode():
    from mtblx import Reduce, Where
    red = Reduce("sum", "min", "max", encoding="varint")
    w = Where.like(red, [(1, 7, 7)])
    assert w.nfields == 3 and w.varint and w.same_layout(red) and not w.same_layout(Reduce("sum", "min", "max"))
    for row in ([0, 7, 0], [1 << 63, 7, M], [0, 8, 0]):
        v = red.encode(row)
        assert w.keeps(v) is (row[1] == 7)
    assert Where.like(Reduce("sum")) == Where(1)
    with pytest.raises(ValueError):
        Where.like("sum_u64")


def test_model_by_hand():
    from mtblx import Where
    w = Where(1, [(0, 10, None)])
    recs = [(b"a", u64(10)), (b"bb", u64(9)), (b"", u64(11)), (b"ccc", b""), (b"d", u64(12) + b"x"), (b"eeee", u64(M))]
    assert wm.verdicts(recs, w) == [True, False, True, None, None, True]
    m = wm.filter_records(recs, w)
    assert m["records"] == [recs[0], recs[2], recs[5]] and m["src_idx"] == [0, 2, 5]
    assert m["totals"] == [3, 5, 24, 2, 1] and m["seg_end"] == [] and m["seg_bad"] == []
    m = wm.filter_records(recs, w, [0, 0, 1, 4, 4, 6])
    assert m["seg_end"] == [0, 1, 2, 2, 3] and m["seg_bad"] == [0, 0, 1, 0, 1]
    assert wm.segments(m, 0) == [] and wm.segments(m, 2) == [recs[2]] and wm.segments(m, 4) == [recs[5]]
    assert wm.filter_records([], w, [0])["totals"] == [0, 0, 0, 0, 0]
    assert wm.filter_records([], w, [0, 0])["seg_end"] == [0]


# ---------------------------------------------------------------- 2. the constructor
def test_where_value_errors():
    from mtblx import Where
    for bad in (0, 9, -1, True, "3", 2.0, None):
        with pytest.raises(ValueError):
            Where(bad)
    with pytest.raises(ValueError):
        Where(1, encoding="u32le")
    with pytest.raises(ValueError):
        Where(1, mode="none")
    for cl in ([(1, 0, 0)], [(-1, 0, 0)], [(True, 0, 0)], [("0", 0, 0)],      # the field
               [(0, 0)], [(0, 0, 0, "outside", 1)], [5],                     # the clause's shape
               [(0, 0, 0, "without")],                                       # the fourth item
               [(0, -1, 0)], [(0, 0, 1 << 64)], [(0, 1.5, 2)], [(0, 0, "9")], [(0, True, 5)],   # the bounds
               [(0, 1, 2), (0, 3, 4)]):                                      # a second clause on one field
        with pytest.raises(ValueError):
            Where(1, cl)
    with pytest.raises(ValueError):
        Where(3, [(0, 1, 2), (1, 1, 2), (0, 1, 2, "outside")])
    w = Where(3, [(2, None, 9, "outside"), (0, 4, None)])
    assert (w.mask, w.outside, w.lo[:3], w.hi[:3]) == (0b101, 0b100, (4, 0, 0), (M, M, 9))


def test_eq_hash_repr():
    from mtblx import Where
    a = Where(3, [(0, 1, 2), (2, 5, None, "outside")], "varint", "any")
    b = Where(3, [(2, 5, None, "outside"), (0, 1, 2)], "varint", "any")
    assert a == b and hash(a) == hash(b) and len({a, b}) == 1
    for other in (Where(3, [(0, 1, 2), (2, 5, None)], "varint", "any"), Where(3, [(0, 1, 2), (2, 5, None, "outside")]),
                  Where(3, [(0, 1, 2), (2, 5, None, "outside")], "varint"), Where(4, [(0, 1, 2)], "varint", "any"), 3):
        assert a != other
    assert repr(a) == f"Where(3, [(0, 1, 2), (2, 5, {M}, 'outside')], encoding='varint', mode='any')"
    assert repr(Where(1)) == "Where(1, [])"
    assert eval(repr(a), {"Where": Where}) == a


def test_python_entry_points_check_before_the_device():
    import mtblx
    with pytest.raises(ValueError):
        mtblx.filter_records(None, "count >= 5")
    with pytest.raises(ValueError):
        mtblx.filter_records(None, None)
    with pytest.raises(ValueError):
        mtblx.where.filter_file(b"", "x")
    assert mtblx.where.as_where(None) is None


# ---------------------------------------------------------------- 3. the struct against the header
def test_cstruct():
    from mtblx import Where, _lib
    w = Where(3, [(2, None, 9, "outside"), (0, 4, None)], "varint", "any").cstruct()
    assert isinstance(w, _lib.WhereSpec)
    assert (w.nfields, w.flags, w.mask, w.outside) == (3, _lib.WHERE_ANY | _lib.WHERE_VARINT, 0b101, 0b100)
    assert list(w.lo) == [4, 0, 0, 0, 0, 0, 0, 0] and list(w.hi) == [M, M, 9] + [M] * 5
    assert Where(1).cstruct().flags == 0 and _lib.WHERE_VARINT == _lib.REDUCE_VARINT


@pytest.mark.skipif(shutil.which("cc") is None and shutil.which("gcc") is None, reason="no C compiler")
def test_struct_sizes_against_the_header(tmp_path):
    from mtblx import _lib
    lines = ['#include <stddef.h>', '#include "mtblx.h"']
    for cname, cls in (("mtblx_where", _lib.WhereSpec), ("mtblx_filtered", _lib.Filtered)):
        lines.append(f'_Static_assert(sizeof({cname}) == {C.sizeof(cls)}, "sizeof {cname}");')
        for name, _ in cls._fields_:
            lines.append(f'_Static_assert(offsetof({cname}, {name}) == {getattr(cls, name).offset}, "{cname}.{name}");')
    lines.append("_Static_assert(MTBLX_WHERE_VARINT == MTBLX_REDUCE_VARINT, \"the varint bit\");")
    lines.append(f"_Static_assert(MTBLX_WHERE_ANY == {_lib.WHERE_ANY} && MTBLX_WHERE_OVERFLOW == {_lib.WHERE_OVERFLOW} && "
                 f"MTBLX_WHERE_NOT_PLANNED == {_lib.WHERE_NOT_PLANNED} && MTBLX_WHERE_BADSEG == {_lib.WHERE_BADSEG}, "
                 "\"the flags\");")
    src = tmp_path / "sizes.c"
    src.write_text("\n".join(lines) + "\n")
    cc = shutil.which("cc") or shutil.which("gcc")
    r = subprocess.run([cc, "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert C.sizeof(_lib.WhereSpec) == 144 and C.sizeof(_lib.Filtered) == 72


# ---------------------------------------------------------------- 4. MTBLX_E_INVAL, before any device call
A = 0x7000_0000_0000            # made-up addresses, 256-byte aligned: never dereferenced
INVAL = -1


def _args(L, n=10, nseg=2):
    from mtblx import Where, _lib
    rec = _lib.Records(A, A + 0x1000, A + 0x2000, A + 0x3000, n)
    w = Where(3, [(0, 1, 2), (2, 5, 9, "outside")]).cstruct()
    out = _lib.Filtered(keys=A + 0x4000, keys_cap=64, vals=A + 0x5000, vals_cap=64, key_end=A + 0x6000,
                        val_end=A + 0x7000, src_idx=A + 0x8000, rec_cap=8, flags=A + 0x9000)
    return dict(rec=rec, w=w, seg=A + 0xa000, nseg=nseg, totals=(C.c_uint64 * 6)(), seg_end=A + 0xb000,
                seg_bad=A + 0xc000, ws=A + 0x10000, wsb=L.mtblx_where_workspace_bytes(n, nseg), out=out)


def _plan(L, a):
    return L.mtblx_where_plan(C.byref(a["rec"]) if a["rec"] is not None else None,
                              C.byref(a["w"]) if a["w"] is not None else None, C.c_void_p(a["seg"]), a["nseg"],
                              a["totals"], C.c_void_p(a["seg_end"]), C.c_void_p(a["seg_bad"]), C.c_void_p(a["ws"]),
                              a["wsb"], None)


def _emit(L, a):
    return L.mtblx_where_emit(C.byref(a["rec"]) if a["rec"] is not None else None,
                              C.byref(a["out"]) if a["out"] is not None else None, C.c_void_p(a["ws"]), a["wsb"], None)


SPEC = ["null-where", "nfields-0", "nfields-9", "flag-2", "flag-high", "mask-above", "outside-above", "outside-not-in-mask"]


@pytest.mark.parametrize("what", SPEC)
def test_where_plan_refuses_the_predicate(mtblx_lib, what):
    a = _args(mtblx_lib)
    w = a["w"]
    if what == "null-where":
        a["w"] = None
    elif what == "nfields-0":
        w.nfields, w.mask, w.outside = 0, 0, 0
    elif what == "nfields-9":
        w.nfields = 9
    elif what == "flag-2":
        w.flags = 2
    elif what == "flag-high":
        w.flags = 0x100 | 0x10
    elif what == "mask-above":
        w.mask = 0b1101
    elif what == "outside-above":
        w.mask, w.outside = 0b1111, 0b1000
    elif what == "outside-not-in-mask":
        w.outside = 0b110
    assert _plan(mtblx_lib, a) == INVAL


def test_where_plan_accepts_every_legal_mask_bit(mtblx_lib):
    """the spec check alone: nfields 8 with all eight bits is legal (refused later for another reason)"""
    a = _args(mtblx_lib)
    a["w"].nfields, a["w"].mask, a["w"].outside = 8, 0xFF, 0xFF
    a["ws"] = None
    assert _plan(mtblx_lib, a) == INVAL
    a = _args(mtblx_lib)
    a["w"].nfields, a["w"].mask, a["w"].outside = 7, 0xFF, 0
    assert _plan(mtblx_lib, a) == INVAL


SHARED = ["null-records", "null-workspace", "workspace-misaligned", "workspace-small", "too-many-records", "null-key_end",
          "null-val_end", "key_end-misaligned", "val_end-misaligned"]


@pytest.mark.parametrize("what", SHARED)
def test_where_plan_and_emit_refuse(mtblx_lib, what):
    from mtblx import _lib
    a = _args(mtblx_lib)
    if what == "null-records":
        a["rec"] = None
    elif what == "null-workspace":
        a["ws"] = None
    elif what == "workspace-misaligned":
        a["ws"] += 128
    elif what == "workspace-small":
        a["wsb"] -= 1
    elif what == "too-many-records":
        a["rec"].n = _lib.MERGE_MAX_RECORDS
        a["wsb"] = 1 << 62
    elif what.startswith("null-"):
        setattr(a["rec"], what[5:], None)
    else:
        f = what.split("-")[0]
        setattr(a["rec"], f, getattr(a["rec"], f) + 4)
    assert _plan(mtblx_lib, a) == INVAL
    assert _emit(mtblx_lib, a) == INVAL


@pytest.mark.parametrize("what", ["null-totals", "too-many-segments", "null-seg_off", "null-seg_end", "seg_off-misaligned",
                                  "seg_end-misaligned", "seg_bad-misaligned"])
def test_where_plan_refuses_its_own(mtblx_lib, what):
    from mtblx import _lib
    a = _args(mtblx_lib)
    if what == "null-totals":
        a["totals"] = None
    elif what == "too-many-segments":
        a["nseg"] = _lib.REDUCE_MAX_SEGMENTS + 1
    elif what == "null-seg_off":
        a["seg"] = None
    elif what == "null-seg_end":
        a["seg_end"] = None
    else:
        f = {"seg_off": "seg"}.get(what.split("-")[0], what.split("-")[0])
        a[f] += 4
    assert _plan(mtblx_lib, a) == INVAL


@pytest.mark.parametrize("what", ["null-out", "null-flags", "flags-misaligned", "null-keys", "null-vals", "null-key_end",
                                  "null-val_end", "key_end-misaligned", "val_end-misaligned", "src_idx-misaligned"])
def test_where_emit_refuses_its_outputs(mtblx_lib, what):
    a = _args(mtblx_lib)
    o = a["out"]
    if what == "null-out":
        a["out"] = None
    elif what == "flags-misaligned":
        o.flags += 2
    elif what.startswith("null-"):
        setattr(o, what[5:], None)
    else:
        f = what.split("-")[0]
        setattr(o, f, getattr(o, f) + 4)
    assert _emit(mtblx_lib, a) == INVAL


def test_where_workspace_and_tile(mtblx_lib):
    T = mtblx_lib.mtblx_where_tile()
    assert T == 1024 == mtblx_lib.mtblx_rollup_tile() == mtblx_lib.mtblx_reduce_seg_tile()
    w = [mtblx_lib.mtblx_where_workspace_bytes(n, 1) for n in (0, 1, T, T + 1, 100 * T)]
    assert 0 < w[0] <= w[1] < w[2] <= w[3] < w[4] and all(x % 256 == 0 for x in w)
    assert mtblx_lib.mtblx_where_workspace_bytes(1000, 0) == mtblx_lib.mtblx_where_workspace_bytes(1000, 1 << 20)


def test_scan_reduce_where_argument_checks_need_no_device(mtblx_lib):
    """everything mtblx_scan_reduce refuses, a bad predicate, a layout that is not the spec's, a NULL or
    misaligned nmatch: MTBLX_E_INVAL before any device call (no address given here is ever
    dereferenced); nq == 0: MTBLX_OK with zero totals"""
    import numpy as np
    from mtblx import Reduce, Where, _lib
    L = mtblx_lib
    need = L.mtblx_scan_workspace_bytes(1)
    host = np.zeros(need + 512, np.uint8)
    wp = (host.ctypes.data + 255) & ~255
    p = C.c_void_p(host.ctypes.data)
    odd = C.c_void_p(host.ctypes.data + 4)
    ty = np.ascontiguousarray([2], np.int32)
    red = Reduce("sum", "min", "max")

    def call(spec=red.cstruct(), where=Where.like(red, [(0, 1, 2)]).cstruct(), fields=p, nbad=p, nmatch=p, wsp=wp,
             wsb=need, nq=1, totals=True, version=1):
        tot = (C.c_uint64 * 4)(7, 7, 7, 7)
        rc = L.mtblx_scan_reduce_where(p, 1000, version, 0, 0, 100, None, None, None, None, 0, None,
                                       C.c_void_p(ty.ctypes.data), p, p, p, p, None, 64, nq, p, tot if totals else None,
                                       C.c_void_p(wsp) if wsp else None, wsb, C.byref(spec) if spec is not None else None,
                                       fields, nbad, C.byref(where) if where is not None else None, nmatch, None)
        return rc, list(tot)

    bad_op = red.cstruct()
    bad_op.op[1] = 3
    for kw in (dict(spec=None), dict(spec=bad_op), dict(fields=None), dict(nbad=None), dict(nmatch=None), dict(totals=False),
               dict(fields=odd), dict(nbad=odd), dict(nmatch=odd), dict(wsp=None), dict(wsp=wp + 8), dict(wsb=need - 1),
               dict(version=2), dict(where=None)):
        assert call(**kw)[0] == INVAL, kw
    for w in (Where(2, [(0, 1, 2)]), Where(4), Where(3, encoding="varint")):          # not the spec's layout
        assert call(where=w.cstruct())[0] == INVAL, w
    assert call(spec=Reduce("sum", "min", "max", encoding="varint").cstruct())[0] == INVAL
    for field, value in (("flags", 2), ("mask", 0b1001), ("outside", 0b010), ("nfields", 0)):
        w = Where.like(red, [(0, 1, 2)]).cstruct()
        setattr(w, field, value)
        assert call(where=w)[0] == INVAL, field
    rc, tot = call(nq=0)
    assert rc == _lib.MTBLX_OK and tot == [0, 0, 0, 0]
    v = Reduce("sum", encoding="varint")
    rc, tot = call(nq=0, spec=v.cstruct(), where=Where.like(v, mode="any").cstruct())
    assert rc == _lib.MTBLX_OK and tot == [0, 0, 0, 0]
    assert (host == 0).all()

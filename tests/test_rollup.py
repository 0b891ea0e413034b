"""Rollups without a GPU: the host definition (tests/rollup_model.py) on hand-derived cases, the
monotonicity the feature rests on, GroupBy's argument checks, and every MTBLX_E_INVAL of the C calls
(the checks run before any device call, so made-up addresses are enough)."""
import ctypes as C
import itertools

import pytest

import rollup_model as rm

M = (1 << 64) - 1


def _u64(*xs):
    return b"".join(x.to_bytes(8, "little") for x in xs)


# ---------------------------------------------------------------- 1. the model, by hand
def test_gkey_length_by_hand():
    g = ("length", 3)
    assert rm.gkey(b"", g) == b"" and rm.gkey(b"ab", g) == b"ab" and rm.gkey(b"abc", g) == b"abc"
    assert rm.gkey(b"abcd", g) == b"abc" and rm.gkey(b"abc\x00", g) == b"abc"
    assert rm.gkey(b"xyz", ("length", 1)) == b"x" and rm.gkey(b"xyz", ("length", 257)) == b"xyz"


def test_gkey_delimiter_by_hand():
    dot = ("delimiter", 0x2e, 1)
    assert rm.gkey(b"com.example.www", dot) == b"com."
    assert rm.gkey(b"com", dot) == b"com" and rm.gkey(b"", dot) == b""
    assert rm.gkey(b".x", dot) == b"." and rm.gkey(b"x.", dot) == b"x."
    dot3 = ("delimiter", 0x2e, 3)
    assert rm.gkey(b"a.b.c.d.e", dot3) == b"a.b.c."
    assert rm.gkey(b"a.b.c", dot3) == b"a.b.c"            # fewer than count: the whole key
    assert rm.gkey(b"...x", dot3) == b"..." and rm.gkey(b"a..b.", dot3) == b"a..b."
    assert rm.gkey(b"a\x00b\x00", ("delimiter", 0, 2)) == b"a\x00b\x00"
    assert rm.gkey(b"\xff\xffz", ("delimiter", 0xff, 2)) == b"\xff\xff"


def test_rollup_by_hand():
    from mtblx import Reduce
    red = Reduce("sum", "min", "max")
    recs = [(b"a.1", _u64(1, 10, 10)), (b"a.2", _u64(2, 5, 50)), (b"a.3", b"short"), (b"b", _u64(7, 7, 7)),
            (b"c.1", b""), (b"c.1x", _u64(M, 0, M)), (b"c.2", _u64(2, 1, 1))]
    m = rm.rollup(recs, ("delimiter", 0x2e, 1), red)
    assert m["keys"] == [b"a.", b"b", b"c."]
    assert m["grp_rec"] == [0, 3, 4, 7] and m["seg_grp"] == [0, 3]
    assert m["nrec"] == [3, 1, 3] and m["nbad"] == [1, 0, 1]
    assert m["fields"] == [(3, 5, 50), (7, 7, 7), (1, 0, M)]                      # M + 2 wraps to 1
    assert m["values"] == [_u64(3, 5, 50), _u64(7, 7, 7), _u64(1, 0, M)]
    # segments: a boundary inside the run of "a." gives two groups with equal keys; empty segments
    m = rm.rollup(recs, ("delimiter", 0x2e, 1), red, [0, 0, 2, 2, 7, 7])
    assert m["keys"] == [b"a.", b"a.", b"b", b"c."] and m["grp_rec"] == [0, 2, 3, 4, 7]
    assert m["seg_grp"] == [0, 0, 1, 1, 4, 4]
    assert m["nbad"] == [0, 1, 0, 1] and m["fields"][1] == (0, M, 0)              # a group of one bad value
    assert m["values"][1] == _u64(0, M, 0)                                        # the identities encoded
    assert rm.groups_of(m, 1) == [(b"a.", (3, 5, 50), 2, 0)] and rm.groups_of(m, 2) == []
    # runs, not sets: an unsorted input keeps equal group keys that are not adjacent apart
    m = rm.rollup([(b"ab", b""), (b"b", b""), (b"ac", b"")], ("length", 1), Reduce("sum"))
    assert m["keys"] == [b"a", b"b", b"a"]
    # varint: the value is the canonical encoding, also of a non-canonical single input
    rv = Reduce("sum", encoding="varint")
    m = rm.rollup([(b"k1", b"\x80\x00"), (b"k2", b"\x7f"), (b"k3", b"\x01")], ("length", 1), rv)
    assert m["values"] == [b"\x80\x01"] and m["fields"] == [(128,)]
    m = rm.rollup([(b"k1", b"\x80\x00")], ("length", 1), rv)
    assert m["values"] == [b"\x00"]                                               # nothing passes through
    assert rm.rollup([], ("length", 1), rv) == dict(keys=[], values=[], fields=[], nrec=[], nbad=[], grp_rec=[0],
                                                    seg_grp=[0, 0])


def test_groupby_gkey_is_the_model():
    from mtblx import GroupBy
    keys = [b"", b".", b"a", b"a.b", b"a.b.c", b"..", b"ab.cd.ef.gh", b"abcdefghij"]
    for g in (GroupBy.length(1), GroupBy.length(4), GroupBy.delimiter(0x2e), GroupBy.delimiter(b".", 2),
              GroupBy.delimiter(0x2e, 3)):
        for k in keys:
            assert g.gkey(k) == rm.gkey(k, g), (g, k)


# ---------------------------------------------------------------- 2. monotone: groups are runs
def _all_keys():
    out = []
    for n in range(7):
        out.extend(bytes(t) for t in itertools.product((0x00, 0x2e, 0xff), repeat=n))
    return sorted(out)


@pytest.mark.parametrize("rule", [("length", 1), ("length", 2), ("length", 5), ("length", 9),
                                  ("delimiter", 0x2e, 1), ("delimiter", 0x2e, 2), ("delimiter", 0x00, 1),
                                  ("delimiter", 0xff, 3), ("delimiter", 0x41, 1)])
def test_sorted_unique_keys_give_sorted_group_keys(rule):
    """an alphabet of three bytes, every key of 0 to 6 bytes (1093 of them, sorted): the group keys come
    out sorted, and the runs are as many as the distinct group keys -- the whole set and 40 random
    subsets"""
    import random
    keys = _all_keys()
    assert len(keys) == 1093 and len(set(keys)) == 1093
    rng = random.Random(7)
    for trial in range(41):
        ks = keys if trial == 0 else sorted(rng.sample(keys, rng.randrange(1, 300)))
        gk = [rm.gkey(k, rule) for k in ks]
        assert gk == sorted(gk)
        runs = sum(1 for i in range(len(gk)) if i == 0 or gk[i] != gk[i - 1])
        assert runs == len(set(gk))
        hd = rm.heads([(k, b"") for k in ks], rule)
        assert sum(hd) == runs


# ---------------------------------------------------------------- 3. GroupBy's arguments
def test_groupby_value_errors():
    from mtblx import GroupBy
    for bad in (0, -1, 1.5, None, "3", True, 1 << 64):
        with pytest.raises(ValueError):
            GroupBy.length(bad)
    for bad in (-1, 256, 1.0, None, b"", b"ab", "x", True):
        with pytest.raises(ValueError):
            GroupBy.delimiter(bad)
    for bad in (0, -1, 2.0, None, True, 1 << 32):
        with pytest.raises(ValueError):
            GroupBy.delimiter(0x2e, bad)
    assert GroupBy.length(1) == GroupBy.length(1) and GroupBy.length(1) != GroupBy.length(2)
    assert GroupBy.delimiter(b".") == GroupBy.delimiter(0x2e, 1)
    g = GroupBy.delimiter(0xff, 3).cstruct()
    assert (g.kind, g.delim, g.count) == (1, 255, 3)
    g = GroupBy.length(257).cstruct()
    assert (g.kind, g.length) == (0, 257)


def test_python_entry_points_check_before_the_device():
    from mtblx import GroupBy, Reduce, reduce_encode, rollup_records
    with pytest.raises(ValueError, match="GroupBy"):
        rollup_records(None, ("length", 1), Reduce("sum"))
    with pytest.raises(ValueError, match="Reduce"):
        rollup_records(None, GroupBy.length(1), "concat")
    with pytest.raises(ValueError, match="Reduce"):
        reduce_encode(None, "first")


# ---------------------------------------------------------------- 4. MTBLX_E_INVAL, before any device call
A = 0x7000_0000_0000            # made-up addresses, 256-byte aligned: never dereferenced
INVAL = -1


def _args(mtblx_lib, n=10, nseg=2):
    from mtblx import _lib
    rec = _lib.Records(A, A + 0x1000, A + 0x2000, A + 0x3000, n)
    grp = _lib.Group(_lib.GROUP_LENGTH, 4, 0, 0)
    wsb = mtblx_lib.mtblx_rollup_workspace_bytes(n, nseg)
    out = _lib.Rolled(keys=A + 0x4000, keys_cap=64, key_end=A + 0x5000, key_end_cap=80, grp_rec=A + 0x6000,
                      grp_rec_cap=88, seg_grp=A + 0x7000, seg_grp_cap=8 * (nseg + 1), flags=A + 0x8000)
    return dict(rec=rec, grp=grp, seg=A + 0x9000, nseg=nseg, totals=A + 0xa000, ws=A + 0x10000, wsb=wsb, out=out)


def _plan(L, a):
    return L.mtblx_rollup_plan(C.byref(a["rec"]) if a["rec"] is not None else None,
                               C.byref(a["grp"]) if a["grp"] is not None else None, C.c_void_p(a["seg"]), a["nseg"],
                               C.c_void_p(a["totals"]), C.c_void_p(a["ws"]), a["wsb"], None)


def _emit(L, a):
    return L.mtblx_rollup_emit(C.byref(a["rec"]) if a["rec"] is not None else None,
                               C.byref(a["grp"]) if a["grp"] is not None else None, C.c_void_p(a["seg"]), a["nseg"],
                               C.byref(a["out"]) if a["out"] is not None else None, C.c_void_p(a["ws"]), a["wsb"], None)


def _shared_bad(a, what):
    """break one argument that the plan and the emit check alike"""
    from mtblx import _lib
    g = a["grp"]
    if what == "null-group":
        a["grp"] = None
    elif what == "null-records":
        a["rec"] = None
    elif what == "kind":
        g.kind = 2
    elif what == "length-0":
        g.length = 0
    elif what == "count-0":
        g.kind, g.delim, g.count = _lib.GROUP_DELIM, 0x2e, 0
    elif what == "delim-256":
        g.kind, g.delim, g.count = _lib.GROUP_DELIM, 256, 1
    elif what == "null-workspace":
        a["ws"] = None
    elif what == "workspace-misaligned":
        a["ws"] += 128
    elif what == "workspace-small":
        a["wsb"] -= 1
    elif what == "too-many-records":
        a["rec"].n = _lib.MERGE_MAX_RECORDS
        a["wsb"] = 1 << 62
    elif what == "too-many-segments":
        a["nseg"] = _lib.REDUCE_MAX_SEGMENTS + 1
        a["out"].seg_grp_cap = 1 << 40
    elif what == "null-key_end":
        a["rec"].key_end = None
    elif what == "key_end-misaligned":
        a["rec"].key_end += 4
    elif what == "null-seg_off":
        a["seg"] = None
    elif what == "seg_off-misaligned":
        a["seg"] += 4
    else:
        raise AssertionError(what)


SHARED = ["null-group", "null-records", "kind", "length-0", "count-0", "delim-256", "null-workspace",
          "workspace-misaligned", "workspace-small", "too-many-records", "too-many-segments", "null-key_end",
          "key_end-misaligned", "null-seg_off", "seg_off-misaligned"]


@pytest.mark.parametrize("what", SHARED)
def test_rollup_plan_and_emit_refuse(mtblx_lib, what):
    a = _args(mtblx_lib)
    _shared_bad(a, what)
    assert _plan(mtblx_lib, a) == INVAL
    assert _emit(mtblx_lib, a) == INVAL


def test_rollup_plan_refuses_its_totals(mtblx_lib):
    for t in (None, A + 0xa004):
        a = _args(mtblx_lib)
        a["totals"] = t
        assert _plan(mtblx_lib, a) == INVAL


@pytest.mark.parametrize("what", ["null-out", "null-flags", "flags-misaligned", "null-keys", "null-key_end", "null-grp_rec",
                                  "null-seg_grp", "key_end-misaligned", "grp_rec-misaligned", "seg_grp-misaligned"])
def test_rollup_emit_refuses_its_outputs(mtblx_lib, what):
    a = _args(mtblx_lib)
    o = a["out"]
    if what == "null-out":
        a["out"] = None
    elif what == "null-flags":
        o.flags = None
    elif what == "flags-misaligned":
        o.flags += 2
    elif what == "null-keys":
        o.keys = None
    elif what.startswith("null-"):
        setattr(o, what[5:], None)
    else:
        f = what.split("-")[0]
        setattr(o, f, getattr(o, f) + 4)
    assert _emit(mtblx_lib, a) == INVAL


def test_rollup_workspace_and_tile(mtblx_lib):
    T = mtblx_lib.mtblx_rollup_tile()
    assert T >= 256 and T % 256 == 0
    w = [mtblx_lib.mtblx_rollup_workspace_bytes(n, 1) for n in (0, 1, T, T + 1, 100 * T)]
    assert 0 < w[0] <= w[1] <= w[2] < w[3] < w[4] and all(x % 256 == 0 for x in w)
    assert mtblx_lib.mtblx_rollup_workspace_bytes(1000, 1) == mtblx_lib.mtblx_rollup_workspace_bytes(1000, 1 << 20)
    e = [mtblx_lib.mtblx_reduce_encode_workspace_bytes(n) for n in (0, 1, T + 1, 1000 * T)]
    assert 0 < e[0] <= e[1] <= e[2] < e[3]


def _encode(L, spec, n=5, fields=A, vals=A + 0x1000, val_end=A + 0x2000, cap=None, ws=A + 0x3000, wsb=None):
    nf = spec.nfields if spec is not None else 1
    varint = spec is not None and spec.op[0] & 0x10
    cap = (10 if varint else 8) * nf * n if cap is None else cap
    wsb = L.mtblx_reduce_encode_workspace_bytes(n) if wsb is None else wsb
    return L.mtblx_reduce_encode(C.c_void_p(fields), n, C.byref(spec) if spec is not None else None, C.c_void_p(vals),
                                 C.c_void_p(val_end), cap, C.c_void_p(ws), wsb, None)


def test_reduce_encode_refuses(mtblx_lib):
    from mtblx import Reduce, _lib
    L = mtblx_lib
    for red in (Reduce("sum", "min", "max"), Reduce("sum", "min", "max", encoding="varint")):
        spec = red.cstruct()
        width = 30 if red.varint else 24
        assert _encode(L, spec, fields=None) == INVAL
        assert _encode(L, spec, fields=A + 4) == INVAL
        assert _encode(L, spec, vals=None) == INVAL
        assert _encode(L, spec, val_end=None) == INVAL
        assert _encode(L, spec, val_end=A + 0x2004) == INVAL
        assert _encode(L, spec, ws=None) == INVAL
        assert _encode(L, spec, ws=A + 0x3001) == INVAL
        assert _encode(L, spec, wsb=0) == INVAL
        assert _encode(L, spec, cap=5 * width - 1) == INVAL
        assert _encode(L, spec, n=_lib.MERGE_MAX_RECORDS, cap=1 << 62, wsb=1 << 40) == INVAL
        assert _encode(L, spec, n=0, fields=None, vals=None, val_end=None, ws=None, wsb=0, cap=0) == 0   # nothing to do
    assert _encode(L, None) == INVAL
    bad = Reduce("sum").cstruct()
    bad.nfields = 9
    assert _encode(L, bad) == INVAL
    bad = Reduce("sum", "min").cstruct()
    bad.op[1] |= 0x10                     # one field varint, one not
    assert _encode(L, bad) == INVAL
    bad = Reduce("sum").cstruct()
    bad.op[0] = 3
    assert _encode(L, bad) == INVAL

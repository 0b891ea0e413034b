"""Set operations on the Merger, the part that needs no GPU: the model (tests/select_model.py)
against hand-written answers, mtblx.Select's own checks, and the argument checks of
mtblx_merge_plan_select / mtblx_merge_seg_plan_select through the loaded library."""
import ctypes as C

import numpy as np
import pytest

import select_model as sm


def _sel():
    import mtblx
    return mtblx.Select


# three small sources: "a" in 0; "b" in 0, 1; "c" in 0, 1, 2; "d" in 1; "e" in 1, 2; "f" in 2
SRC = [
    [(b"a", b"a0"), (b"b", b"b0"), (b"c", b"c0")],
    [(b"b", b"b1"), (b"c", b"c1"), (b"d", b"d1"), (b"e", b"e1")],
    [(b"c", b"c2"), (b"e", b"e2"), (b"f", b"f2")],
]


def _keys(sel):
    return [k for k, _ in sm.select_groups(SRC, sel)]


def test_model_hand_answers():
    S = _sel()
    assert sm.masked_groups(SRC) == [
        (b"a", 0b001, [b"a0"]), (b"b", 0b011, [b"b0", b"b1"]), (b"c", 0b111, [b"c0", b"c1", b"c2"]),
        (b"d", 0b010, [b"d1"]), (b"e", 0b110, [b"e1", b"e2"]), (b"f", 0b100, [b"f2"])]
    assert _keys(None) == _keys(S.union()) == [b"a", b"b", b"c", b"d", b"e", b"f"]
    assert _keys(S.intersection(3)) == [b"c"]
    assert _keys(S.intersection(2)) == [b"b", b"c"]
    assert _keys(S.difference(0, [1, 2])) == [b"a"]
    assert _keys(S.difference(1, [0])) == [b"d", b"e"]
    assert _keys(S.exactly_one()) == [b"a", b"d", b"f"]
    assert _keys(S.at_least(2)) == [b"b", b"c", b"e"]
    assert _keys(S(require=[0, 1], max_count=2)) == [b"b"]
    # the values of a kept group are all of its values, in source order; a semi-join keeps A's
    assert sm.select_groups(SRC, S.at_least(3)) == [(b"c", [b"c0", b"c1", b"c2"])]
    assert sm.select_merge(SRC, S(require=[0, 1]), lambda k, vs: vs[0]) == [(b"b", b"b0"), (b"c", b"c0")]
    assert sm.left_out(SRC, S.exactly_one()) == (3, 7)
    assert sm.left_out(SRC, S.union()) == (0, 0)


def test_model_empty_keys():
    """the quirk runs before the selection; asserted against hand answers, not the heap's order"""
    S = _sel()
    # an empty key in one source among other keys vanishes before the selection sees anything
    src = [[(b"", b"e0"), (b"k", b"k0")], [(b"k", b"k1"), (b"m", b"m1")]]
    assert sm.masked_groups(src) == [(b"k", 0b11, [b"k0", b"k1"]), (b"m", 0b10, [b"m1"])]
    assert sm.select_groups(src, S.difference(0, [1])) == []
    assert sm.select_groups(src, S.exactly_one()) == [(b"m", [b"m1"])]
    # only empty keys: one item whose mask is the highest-numbered source's
    only = [[(b"", b"x0")], [(b"", b"x1")], [(b"", b"x2")]]
    assert sm.masked_groups(only) == [(b"", 0b100, [b"x2"])]
    assert sm.select_groups(only, S.difference(2, [0, 1])) == [(b"", [b"x2"])]
    assert sm.select_groups(only, S.intersection(3)) == []
    assert sm.select_groups(only, S(require=[0])) == []
    assert sm.select_groups(only, S.exactly_one()) == [(b"", [b"x2"])]


def test_select_python_checks():
    S = _sel()
    from mtblx import _lib, setops
    u = S.union()
    assert (u.require, u.exclude, u.min_count, u.max_count) == (0, 0, 1, 64)
    assert S(min_count=0).min_count == 1                       # 0 reads as 1
    assert S.intersection(64).require == (1 << 64) - 1
    d = S.difference(0, [1, 5])
    assert (d.require, d.exclude) == (1, 0b100010)
    c = d.cstruct()
    assert isinstance(c, _lib.SelectSpec) and C.sizeof(c) == 24
    assert (c.require, c.exclude, c.min_count, c.max_count) == (1, 0b100010, 1, 64)
    assert d.keeps(0b1) and d.keeps(0b1101) and not d.keeps(0b11) and not d.keeps(0b100)
    assert S.at_least(2).keeps(0b101) and not S.at_least(2).keeps(0b100)
    assert S.exactly_one() == S(max_count=1) and S.exactly_one() != S.union()
    for bad in (dict(require=[64]), dict(exclude=[-1]), dict(require=[1], exclude=[1]), dict(max_count=0),
                dict(max_count=65), dict(min_count=3, max_count=2), dict(min_count=-1), dict(require=["0"])):
        with pytest.raises(ValueError):
            S(**bad)
    with pytest.raises(ValueError):
        S.intersection(65)
    with pytest.raises(ValueError):
        S.intersection(0)
    # a source that is not there, more than 64 sources: refused before any device work
    assert setops.as_select(None, 3) is None
    assert setops.as_select(d, 6) is d
    with pytest.raises(ValueError):
        setops.as_select(d, 5)
    with pytest.raises(ValueError):
        setops.as_select(u, 65)
    with pytest.raises(ValueError):
        setops.as_select("union", 2)


def test_symbols_bound(mtblx_lib):
    import mtblx
    for n in ("mtblx_merge_plan_select", "mtblx_merge_seg_plan_select"):
        assert n in mtblx.EXPORTS
        assert getattr(mtblx_lib, n).argtypes is not None
    assert mtblx_lib.mtblx_abi_version() == 3
    assert {"Select", "setops"} <= set(mtblx.__all__)
    assert callable(mtblx.setops.diff_files)


# (nsrc, require, exclude, min_count, max_count): every refusal of include/mtblx.h "Set operations"
REFUSED = [
    (3, 0b1000, 0, 1, 64),        # a require bit at nsrc
    (3, 0, 1 << 63, 1, 64),       # an exclude bit above nsrc
    (0, 1, 0, 1, 64),             # no sources, a bit named
    (3, 0b011, 0b010, 1, 64),     # a source both required and excluded
    (3, 0, 0, 1, 0),              # max_count == 0
    (3, 0, 0, 1, 65),             # max_count > 64
    (3, 0, 0, 3, 2),              # min_count > max_count
    (3, 0, 0, 0, 0),              # max(min_count, 1) > max_count
]
ACCEPTED_SHAPE = [(3, 0b101, 0b010, 0, 1), (64, (1 << 64) - 1, 0, 64, 64)]


def _plan_args(_lib, L, nsrc):
    host = np.zeros(4096 + 256, np.uint8)           # an aligned, non-NULL address; never dereferenced
    wp = (host.ctypes.data + 255) & ~255
    arr = (_lib.Records * max(nsrc, 1))()           # empty sources
    return host, wp, arr


@pytest.mark.parametrize("case", REFUSED)
def test_plan_select_refusals_need_no_device(mtblx_lib, case):
    from mtblx import _lib
    L = mtblx_lib
    nsrc, req, exc, mn, mx = case
    host, wp, arr = _plan_args(_lib, L, nsrc)
    tot = (C.c_uint64 * 8)()
    sel = _lib.SelectSpec(req, exc, mn, mx)
    need = L.mtblx_merge_workspace_bytes(0, nsrc)
    assert 0 < need <= 4096
    assert L.mtblx_merge_plan_select(arr, nsrc, C.byref(sel), tot, C.c_void_p(wp), need, None) == _lib.MTBLX_E_INVAL
    nseg = 2
    need = L.mtblx_merge_seg_workspace_bytes(0, nsrc, nseg)
    assert 0 < need <= 4096
    off = np.zeros(nseg + 1, np.uint64)
    offs = (C.c_void_p * max(nsrc, 1))(*([off.ctypes.data] * max(nsrc, 1)))
    seg_end = np.zeros(nseg, np.uint64)
    assert L.mtblx_merge_seg_plan_select(arr, offs, nsrc, nseg, C.byref(sel), tot, C.c_void_p(seg_end.ctypes.data),
                                         C.c_void_p(wp), need, None) == _lib.MTBLX_E_INVAL


def test_plan_select_refuses_what_the_plain_plans_refuse(mtblx_lib):
    from mtblx import _lib
    L = mtblx_lib
    host, wp, arr = _plan_args(_lib, L, 1)
    arr[0] = _lib.Records(0, 0, 0, 0, 1000)
    tot = (C.c_uint64 * 8)()
    sel = _lib.SelectSpec(0, 0, 1, 64)
    need = L.mtblx_merge_workspace_bytes(1000, 1)
    INVAL = _lib.MTBLX_E_INVAL
    for s in (C.byref(sel), None):   # sel == NULL is the plain plan, its checks included
        assert L.mtblx_merge_plan_select(arr, 1, s, tot, None, need, None) == INVAL              # NULL workspace
        assert L.mtblx_merge_plan_select(arr, 1, s, tot, C.c_void_p(wp + 8), need, None) == INVAL   # misaligned
        assert L.mtblx_merge_plan_select(arr, 1, s, tot, C.c_void_p(wp), 4096, None) == INVAL    # too small
        assert L.mtblx_merge_plan_select(arr, 1, s, None, C.c_void_p(wp), need, None) == INVAL   # NULL totals
        many = (_lib.Records * 65)()
        assert L.mtblx_merge_plan_select(many, 65, s, tot, C.c_void_p(wp), 1 << 40, None) == INVAL
        off = np.zeros(2, np.uint64)
        offs = (C.c_void_p * 1)(off.ctypes.data)
        seg_end = np.zeros(1, np.uint64)
        sneed = L.mtblx_merge_seg_workspace_bytes(1000, 1, 1)
        se = C.c_void_p(seg_end.ctypes.data)
        assert L.mtblx_merge_seg_plan_select(arr, offs, 1, 1, s, tot, se, None, sneed, None) == INVAL
        assert L.mtblx_merge_seg_plan_select(arr, offs, 1, 1, s, tot, se, C.c_void_p(wp), 4096, None) == INVAL
        assert L.mtblx_merge_seg_plan_select(arr, offs, 1, 1, s, tot, None, C.c_void_p(wp), sneed, None) == INVAL
        assert L.mtblx_merge_seg_plan_select(arr, None, 1, 1, s, tot, se, C.c_void_p(wp), sneed, None) == INVAL
        assert L.mtblx_merge_seg_plan_select(arr, offs, 1, (1 << 24) + 1, s, tot, se, C.c_void_p(wp), 1 << 40,
                                             None) == INVAL


def test_accepted_rules_pass_the_rule_check():
    """the rules the C check must NOT refuse, through the same predicate Select applies"""
    S = _sel()
    for nsrc, req, exc, mn, mx in ACCEPTED_SHAPE:
        bits = lambda m: [i for i in range(64) if m >> i & 1]   # noqa: E731
        s = S(bits(req), bits(exc), mn, mx)
        assert s.check(nsrc) is s
    for nsrc, req, exc, mn, mx in REFUSED:
        bits = lambda m: [i for i in range(64) if m >> i & 1]   # noqa: E731
        with pytest.raises(ValueError):
            S(bits(req), bits(exc), mn, mx).check(nsrc)

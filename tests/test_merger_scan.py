"""Merger.scan_batch without a GPU: the new symbols, every argument check of the segmented merge
(MTBLX_E_INVAL before any device call), the Python argument checks, and the per-query model the GPU
tests compare with (tests/merger_scan_util.py) on vectors worked out by hand."""
import ctypes as C

import numpy as np
import pytest

import merger_model as mm
import merger_scan_util as U

SYMBOLS = ("mtblx_merge_seg_workspace_bytes", "mtblx_merge_seg_plan", "mtblx_merge_seg_emit",
           "mtblx_merge_seg_emit_reduce")


def test_symbols_bound(mtblx_lib):
    import mtblx
    from mtblx import _lib
    for n in SYMBOLS + ("mtblx_merge_seg_plan_timed",):
        assert n in mtblx.EXPORTS
        assert getattr(mtblx_lib, n).argtypes is not None
    assert mtblx_lib.mtblx_abi_version() == 3
    assert _lib.MERGE_MAX_SEGMENTS >= 1 << 24 and _lib.MERGE_BADSEG == 4
    assert {"MergedScanBatch", "merge_segments"} <= set(mtblx.__all__)
    assert mtblx.MergedScanBatch is not None and callable(mtblx.merge_segments)


def test_workspace_bytes_monotone(mtblx_lib):
    f = mtblx_lib.mtblx_merge_seg_workspace_bytes
    assert f(0, 0, 0) > 0
    assert f(1000, 8, 10) >= mtblx_lib.mtblx_merge_workspace_bytes(1000, 8) + 12 * 10
    for a, b in (((1000, 8, 10), (100_000, 8, 10)), ((1000, 8, 10), (1000, 64, 10)),
                 ((1000, 8, 10), (1000, 8, 100_000)), ((0, 0, 0), (0, 0, 1 << 24))):
        assert f(*a) <= f(*b)
    assert f(1000, 8, 10) < f(100_000, 8, 10) and f(1000, 8, 10) < f(1000, 8, 100_000)
    assert f((1 << 32) - 16, 1, 1) == 0 and f(10, 1, (1 << 24) + 1) == 0   # beyond the limits: no size


class _Args:
    """one source of 1000 records cut into 4 segments; addresses that are never dereferenced"""

    def __init__(self, L, _lib, nsrc=1, nseg=4, n=1000):
        self.host = np.zeros(4096 + 256, np.uint8)
        self.wp = (self.host.ctypes.data + 255) & ~255
        self.src = (_lib.Records * max(nsrc, 1))()
        self.off = (C.c_void_p * max(nsrc, 1))()
        for i in range(nsrc):
            self.src[i] = _lib.Records(0, self.wp, 0, self.wp, n)
            self.off[i] = self.wp
        self.nsrc, self.nseg = nsrc, nseg
        self.need = L.mtblx_merge_seg_workspace_bytes(n * nsrc, nsrc, nseg)
        self.tot = (C.c_uint64 * 6)()
        self.flags = np.zeros(1, np.uint32)
        self.out = _lib.Merged(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, self.flags.ctypes.data)
        self.spec = _lib.ReduceSpec()
        self.spec.nfields = 1


def _calls(L, a, src="src", off="off", nsrc=None, nseg=None, ws="wp", wsb=None, tot="tot", seg_end="wp", out="out",
           mode=1):
    """the three entry points with one argument replaced -> their return codes"""
    g = lambda name: None if name is None else getattr(a, name)   # noqa: E731
    nsrc = a.nsrc if nsrc is None else nsrc
    nseg = a.nseg if nseg is None else nseg
    wsb = a.need if wsb is None else wsb
    wsp = ws if isinstance(ws, int) else g(ws)
    wsv = None if wsp is None else C.c_void_p(wsp)
    se = None if seg_end is None else C.c_void_p(g(seg_end))
    o = None if out is None else C.byref(g(out))
    rc = [L.mtblx_merge_seg_plan(g(src), g(off), nsrc, nseg, g(tot), se, wsv, wsb, None)]
    if tot is not None and seg_end is not None:   # these two are the plan's alone
        rc.append(L.mtblx_merge_seg_emit(g(src), g(off), nsrc, nseg, mode, o, wsv, wsb, None))
        rc.append(L.mtblx_merge_seg_emit_reduce(g(src), g(off), nsrc, nseg, C.byref(a.spec), o, wsv, wsb, None))
    return rc


def test_argument_checks_need_no_device(mtblx_lib):
    """every MTBLX_E_INVAL of the contract returns before any device call (no GPU here, and none
    of the addresses handed in is device memory)"""
    from mtblx import _lib
    L, E = mtblx_lib, _lib.MTBLX_E_INVAL
    a = _Args(L, _lib)
    assert a.need > 4096
    bad = lambda **kw: all(rc == E for rc in _calls(L, a, **kw))   # noqa: E731
    assert bad(ws=None)                                   # NULL workspace
    assert bad(ws=a.wp + 8)                               # misaligned workspace
    assert bad(wsb=a.need - 1) and bad(wsb=4096)          # short ws_bytes
    assert bad(nseg=(1 << 24) + 1, wsb=1 << 40)           # too many segments
    assert bad(src=None) and bad(off=None)                # NULL required pointers
    assert bad(tot=None) and bad(seg_end=None)
    assert _calls(L, a, out=None)[1:] == [E, E]
    assert L.mtblx_merge_seg_emit(a.src, a.off, 1, 4, 7, C.byref(a.out), C.c_void_p(a.wp), a.need, None) == E   # mode
    noflags = _lib.Merged(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    assert L.mtblx_merge_seg_emit(a.src, a.off, 1, 4, 1, C.byref(noflags), C.c_void_p(a.wp), a.need, None) == E
    a.spec.nfields = 9
    assert _calls(L, a)[2] == E                           # a bad reduce spec
    a.spec.nfields = 1
    a.off[0] = None
    assert bad()                                          # a NULL seg_off entry
    many = _Args(L, _lib, nsrc=65, n=1)
    assert all(rc == E for rc in _calls(L, many, nsrc=65, wsb=1 << 40))   # more than 64 sources
    big = _Args(L, _lib, nsrc=2, n=(1 << 31))             # 2^32 records in all
    assert all(rc == E for rc in _calls(L, big, wsb=1 << 62))
    one = _Args(L, _lib, nsrc=1, n=(1 << 32) - 16)
    assert all(rc == E for rc in _calls(L, one, wsb=1 << 62))
    noend = _Args(L, _lib)
    noend.src[0] = _lib.Records(0, 0, 0, 0, 1000)         # records without END arrays
    assert all(rc == E for rc in _calls(L, noend))


def test_python_argument_checks():
    """bad query tuples and limits are refused before any source is touched (the sources here are
    not readers at all)"""
    from mtblx import merger
    m = merger.Merger([object()], "concat")
    for q in [("scan", b"k")], [("range", b"a")], [("get", b"a", b"b")], [b"k"], [()]:
        with pytest.raises(ValueError, match="bad query"):
            m.scan_batch(q)
    with pytest.raises(ValueError, match="one per query"):
        m.scan_batch([("get", b"a"), ("get", b"b")], max_records=[1])
    with pytest.raises(ValueError, match="negative"):
        m.scan_batch([("get", b"a")], max_records=-1)
    with pytest.raises(ValueError, match="negative"):
        m.scan_batch_groups([("get", b"a"), ("from", b"")], max_records=[None, -3])
    qs, lim = merger.check_queries([("prefix", bytearray(b"ab")), ["range", b"a", b"b"]], 5)
    assert qs == [("prefix", b"ab"), ("range", b"a", b"b")] and lim == [5, 5]


def test_model_vectors_by_hand():
    """the per-query model on lists as the sources' iterators would yield them"""
    # two sources answering ("prefix", b"a"): a shared key, source order inside the group
    lists = [[(b"a1", b"s0"), (b"a3", b"s0")], [(b"a1", b"s1"), (b"a2", b"s1")]]
    want = [(b"a1", [b"s0", b"s1"]), (b"a2", [b"s1"]), (b"a3", [b"s0"])]
    assert U.promised_groups(lists) == want and mm.canon(U.model_groups(lists)) == mm.canon(want)
    assert U.merged(want, U.PICK["concat"]) == [(b"a1", b"s0s1"), (b"a2", b"s1"), (b"a3", b"s0")]
    assert U.merged(want, U.PICK["last"])[0] == (b"a1", b"s1") and U.cut(want, 1) == want[:1] and U.cut(want, 0) == []
    assert U.cut(want, None) == want and U.cut(want, 9) == want
    # no source matches: nothing
    assert U.promised_groups([[], [], []]) == [] == U.model_groups([[], [], []])
    # the quirk per query, on the lists each query of QUIRK_QUERIES yields over QUIRK_SOURCES
    s = U.QUIRK_SOURCES
    only_empty = [[r for r in recs if r[0] == b""] for recs in s]          # ("range", "", "") and ("get", "")
    assert U.promised_groups(only_empty) == [(b"", [b"c"])]               # the highest-numbered source's value
    got = U.model_groups(only_empty)
    assert len(got) == 1 and got[0][0] == b"" and len(got[0][1]) == 1      # which value: the heap's choice
    everything = [(b"k1", [b"x", b"y"]), (b"k2", [b"z"])]                  # ("prefix", "") and ("from", "")
    assert U.promised_groups(s) == everything and mm.canon(U.model_groups(s)) == mm.canon(everything)
    assert [U.cut(everything, m) for m in (0, 1, 2)] == [[], everything[:1], everything]
    # the m + 1 edge: with limit m = 1 every source is asked for 2 records; the merged cut is still
    # the first item of the unlimited result (source 2's k2 is not needed for it)
    two_each = [recs[:2] for recs in s]
    assert U.cut(U.promised_groups(two_each), 1) == everything[:1]
    # with limit 0 every source hands over its one empty-key record: one item is built and none reported
    assert U.cut(U.promised_groups([recs[:1] for recs in s]), 0) == []
    assert U.sum_u64([(5).to_bytes(8, "little"), ((1 << 64) - 1).to_bytes(8, "little")]) == (4).to_bytes(8, "little")

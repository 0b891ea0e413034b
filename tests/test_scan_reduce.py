"""Aggregating scans (mtblx_scan_reduce, mtblx_reduce_segments, Reader.reduce_batch,
Merger.reduce_batch), the parts that need no GPU: Reduce.fold pinned against vectors worked out by
hand, the argument checks of both C calls, and the Python argument errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = (1 << 64) - 1


def u(*xs):
    return b"".join(int(x).to_bytes(8, "little") for x in xs)


# ---------------------------------------------------------------- Reduce.fold by hand
def test_fold_wrapping_sum():
    from mtblx import Reduce
    assert Reduce("sum").fold([u(M), u(2)]) == ((1,), 2, 0)
    assert Reduce("sum").fold([u(M), u(1)]) == ((0,), 2, 0)
    assert Reduce("sum").fold([u(1 << 63), u(1 << 63), u(5)]) == ((5,), 3, 0)


def test_fold_min_max_across_the_sign_bit():
    from mtblx import Reduce
    vals = [u((1 << 63) - 1), u(1 << 63), u(3), u(M)]          # unsigned: 3 < 2^63 - 1 < 2^63 < 2^64 - 1
    assert Reduce("min").fold(vals) == ((3,), 4, 0)
    assert Reduce("max").fold(vals) == ((M,), 4, 0)
    assert Reduce("min", "max").fold([u(1 << 63, 1), u(7, 1 << 63)]) == ((7, 1 << 63), 2, 0)


def test_fold_eight_fields():
    from mtblx import Reduce
    r = Reduce("sum", "min", "max", "sum", "min", "max", "sum", "sum")
    a = u(1, 2, 3, 4, 5, 6, 7, M)
    b = u(10, 1, 30, 40, 50, 5, 70, 1)
    c = u(100, 3, 2, 400, 4, 60, 700, 1)
    assert r.fold([a, b, c]) == ((111, 1, 30, 444, 4, 60, 777, 1), 3, 0)
    assert r.width == 64


def test_fold_empty_gives_the_identities():
    from mtblx import Reduce
    assert Reduce("sum", "min", "max").fold([]) == ((0, M, 0), 0, 0)
    assert Reduce("sum", "min", "max").identities() == (0, M, 0)
    assert Reduce("min").fold([b"short"]) == ((M,), 1, 1)      # nothing good: still the identity


def test_fold_counts_other_lengths_as_bad():
    from mtblx import Reduce
    r = Reduce("sum", "min", "max")                               # W = 24
    good = [u(1, 9, 9), u(2, 4, 11)]
    bad = [b"", b"x" * 23, b"x" * 25, u(77)]                      # 0, W - 1, W + 1, 8
    assert r.fold(good + bad) == ((3, 4, 11), 6, 4)
    assert r.fold(bad[:1] + good[:1] + bad[1:] + good[1:]) == ((3, 4, 11), 6, 4)   # wherever they stand
    assert r.fold(bad) == ((0, M, 0), 4, 4)
    assert Reduce("sum").fold([u(77), u(1, 2)]) == ((77,), 2, 1)  # 8 bytes are good when W = 8


# ---------------------------------------------------------------- the ABI surface
def test_symbols_exported_and_declared(mtblx_lib):
    from mtblx import _lib
    hdr = open(os.path.join(ROOT, "include", "mtblx.h")).read()
    for s in ("mtblx_scan_reduce", "mtblx_reduce_segments", "mtblx_reduce_seg_tile"):
        assert s in _lib.EXPORTS
        assert getattr(mtblx_lib, s) is not None
        assert re.search(r"\b%s\(" % s, hdr), s
    assert "#define MTBLX_REDUCE_BADSEG %du" % _lib.REDUCE_BADSEG in hdr
    assert "#define MTBLX_REDUCE_SEG_TILE %d" % _lib.REDUCE_SEG_TILE in hdr
    assert "#define MTBLX_REDUCE_MAX_SEGMENTS 0x%Xu" % _lib.REDUCE_MAX_SEGMENTS in hdr
    assert mtblx_lib.mtblx_reduce_seg_tile() == _lib.REDUCE_SEG_TILE
    assert mtblx_lib.mtblx_abi_version() == 3


def _spec(_lib, nfields=1, ops=(0,)):
    s = _lib.ReduceSpec()
    s.nfields = nfields
    for f, op in enumerate(ops):
        s.op[f] = op
    return s


def test_scan_reduce_argument_checks_need_no_device(mtblx_lib):
    """a bad spec, NULL outputs, a misaligned or short workspace: MTBLX_E_INVAL before any device
    call (no address given here is ever dereferenced); nq == 0: MTBLX_OK with zero totals"""
    from mtblx import _lib
    L = mtblx_lib
    need = L.mtblx_scan_workspace_bytes(1)
    host = np.zeros(need + 512, np.uint8)
    wp = (host.ctypes.data + 255) & ~255
    p = C.c_void_p(host.ctypes.data)
    ty = np.ascontiguousarray([2], np.int32)
    INVAL = _lib.MTBLX_E_INVAL

    def call(spec=_spec(_lib), fields=p, nbad=p, wsp=wp, wsb=need, nq=1, totals=True, version=1):
        tot = (C.c_uint64 * 4)(7, 7, 7, 7)
        rc = L.mtblx_scan_reduce(p, 1000, version, 0, 0, 100, None, None, None, None, 0, None,
                                 C.c_void_p(ty.ctypes.data), p, p, p, p, None, 64, nq, p, tot if totals else None,
                                 C.c_void_p(wsp) if wsp else None, wsb, C.byref(spec) if spec is not None else None,
                                 fields, nbad, None)
        return rc, list(tot)

    assert call(spec=None)[0] == INVAL
    assert call(spec=_spec(_lib, 0, ()))[0] == INVAL
    assert call(spec=_spec(_lib, 9, (0,) * 8))[0] == INVAL
    assert call(spec=_spec(_lib, 2, (0, 3)))[0] == INVAL           # an op above MTBLX_REDUCE_MAX
    assert call(spec=_spec(_lib, 8, (0,) * 7 + (200,)))[0] == INVAL
    assert call(fields=None)[0] == INVAL
    assert call(nbad=None)[0] == INVAL
    assert call(totals=False)[0] == INVAL
    assert call(fields=C.c_void_p(host.ctypes.data + 4))[0] == INVAL      # outputs that are not 8-byte aligned
    assert call(nbad=C.c_void_p(host.ctypes.data + 4))[0] == INVAL
    assert call(wsp=None)[0] == INVAL
    assert call(wsp=wp + 8)[0] == INVAL
    assert call(wsb=need - 1)[0] == INVAL
    assert call(version=2)[0] == INVAL
    rc, tot = call(nq=0)
    assert rc == _lib.MTBLX_OK and tot == [0, 0, 0, 0]
    rc, tot = call(nq=0, spec=_spec(_lib, 8, (0, 1, 2, 0, 1, 2, 0, 1)))
    assert rc == _lib.MTBLX_OK and tot == [0, 0, 0, 0]


def test_reduce_segments_argument_checks_need_no_device(mtblx_lib):
    from mtblx import _lib
    L = mtblx_lib
    host = np.zeros(64, np.uint64)
    p = C.c_void_p(host.ctypes.data)
    rec = _lib.Records(0, 0, host.ctypes.data, host.ctypes.data, 4)
    INVAL = _lib.MTBLX_E_INVAL

    def call(recs=rec, lo=p, hi=p, nseg=1, spec=_spec(_lib), fields=p, nbad=p, flags=p):
        return L.mtblx_reduce_segments(C.byref(recs) if recs is not None else None, lo, hi, nseg,
                                       C.byref(spec) if spec is not None else None, fields, nbad, flags, None)

    assert call(spec=None) == INVAL
    assert call(spec=_spec(_lib, 0, ())) == INVAL
    assert call(spec=_spec(_lib, 9, (0,) * 8)) == INVAL
    assert call(spec=_spec(_lib, 1, (3,))) == INVAL
    assert call(fields=None) == INVAL
    assert call(nbad=None) == INVAL
    assert call(flags=None) == INVAL
    assert call(recs=None) == INVAL
    assert call(lo=None) == INVAL
    assert call(hi=None) == INVAL
    assert call(recs=_lib.Records(0, 0, host.ctypes.data, 0, 4)) == INVAL                     # records without ENDs
    assert call(recs=_lib.Records(0, 0, host.ctypes.data, host.ctypes.data, (1 << 32) - 16)) == INVAL
    # the kernels load and update these as aligned words: refused, not faulted on
    odd8, odd4 = C.c_void_p(host.ctypes.data + 4), C.c_void_p(host.ctypes.data + 2)
    for kw in (dict(fields=odd8), dict(nbad=odd8), dict(lo=odd8), dict(hi=odd8), dict(flags=odd4),
               dict(recs=_lib.Records(0, 0, host.ctypes.data, host.ctypes.data + 4, 4))):
        assert call(**kw) == INVAL, kw
    assert call(nseg=_lib.REDUCE_MAX_SEGMENTS + 1) == INVAL
    assert call(nseg=0, lo=None, hi=None) == _lib.MTBLX_OK                                    # nothing to do
    assert (host == 0).all()


# ---------------------------------------------------------------- Python argument errors
def test_python_argument_checks():
    """refused before any reader or source is touched (the objects here are neither)"""
    from mtblx import Reduce, ReduceBatch, merger, reader, reduce_segments
    assert callable(reduce_segments) and callable(ReduceBatch.values) and callable(ReduceBatch.value_bytes)
    for a in ("served_by_kernel", "end", "err", "check"):
        assert callable(getattr(ReduceBatch, a))
    red = Reduce("sum", "min", "max")
    m = merger.Merger([object()], red)
    for call in [lambda qs, **kw: m.reduce_batch(qs, **kw)]:
        for q in [("scan", b"k")], [("range", b"a")], [("get", b"a", b"b")], [b"k"], [()]:
            with pytest.raises(ValueError, match="bad query"):
                call(q)
        with pytest.raises(ValueError, match="one per query"):
            call([("get", b"a"), ("get", b"b")], max_records=[1])
        with pytest.raises(ValueError, match="negative"):
            call([("get", b"a")], max_records=-1)
    with pytest.raises(ValueError, match="not a Reduce"):
        reader.Reader.reduce_batch(object(), [("get", b"a")], "concat")
    with pytest.raises(ValueError, match="callable"):
        merger.Merger([object()], lambda k, vs: vs[0]).reduce_batch([("get", b"a")], red)
    for name in ("concat", "first", "last"):
        with pytest.raises(ValueError, match="pass a Reduce"):
            merger.Merger([object()], name).reduce_batch([("get", b"a")])       # reduce=None without a Reduce
    with pytest.raises(ValueError, match="not a Reduce"):
        merger.Merger([object()], "concat").reduce_batch([("get", b"a")], "first")

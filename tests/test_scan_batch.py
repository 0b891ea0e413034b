"""Batched scans (mtblx_scan_plan / mtblx_scan_emit, Reader.scan_batch), the parts that need no
GPU: the ABI surface, the argument checks, and the test helper that predicts how many data blocks
a query opens, checked against the oracle alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import scan_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("mtblx_scan_workspace_bytes", "mtblx_scan_plan", "mtblx_scan_emit")


def test_symbols_exported_and_declared(mtblx_lib):
    from mtblx import _lib
    hdr = open(os.path.join(ROOT, "include", "mtblx.h")).read()
    for s in SYMS:
        assert s in _lib.EXPORTS
        assert getattr(mtblx_lib, s) is not None
        assert re.search(r"\b%s\(" % s, hdr), s
    for name in ("MTBLX_SCAN_OK 0", "MTBLX_SCAN_LARGE 1", "MTBLX_SCAN_FALLBACK 2", "MTBLX_SCAN_OVERFLOW 1u",
                 "MTBLX_SCAN_NOT_PLANNED 2u", "MTBLX_SCAN_INTERNAL 4u", "MTBLX_SCAN_MAX_KEY %d" % _lib.SCAN_MAX_KEY):
        assert "#define " + name in hdr, name
    assert (_lib.SCAN_OK, _lib.SCAN_LARGE, _lib.SCAN_FALLBACK) == (0, 1, 2)
    assert (_lib.SCAN_OVERFLOW, _lib.SCAN_NOT_PLANNED, _lib.SCAN_INTERNAL) == (1, 2, 4)


def test_struct_sizes_and_abi_version(mtblx_lib):
    from mtblx import _lib
    assert C.sizeof(_lib.ScanResult) == 64
    assert C.sizeof(_lib.Scanned) == 64
    assert _lib.ScanResult.status.offset == 0 and _lib.ScanResult.nrec.offset == 8
    assert _lib.ScanResult.rec_base.offset == 32 and _lib.ScanResult.blocks.offset == 56
    assert _lib.Scanned.key_end.offset == 32 and _lib.Scanned.flags.offset == 56
    assert mtblx_lib.mtblx_abi_version() == 3
    hdr = open(os.path.join(ROOT, "include", "mtblx.h")).read()
    assert re.search(r"#define MTBLX_ABI_VERSION 3\b", hdr)


def test_reader_methods_exist():
    from mtblx import reader
    assert callable(reader.Reader.scan_batch) and callable(reader.Reader.count_batch)
    for a in ("scan", "records", "served_by_kernel"):
        assert callable(getattr(reader.ScanBatch, a))


def test_workspace_bytes(mtblx_lib):
    L = mtblx_lib
    sizes = [L.mtblx_scan_workspace_bytes(n) for n in (0, 1, 2, 63, 64, 65, 257, 1000, 100000, 1 << 20)]
    assert sizes[0] > 0
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert all(s % 256 == 0 for s in sizes)


def _plan(L, wp, wsb, nq=1, version=1, types=(2,), keys2=True, file=True, totals=True):
    """mtblx_scan_plan with never-dereferenced host addresses where the checks want non-NULL"""
    host = np.zeros(64, np.uint64)
    p = C.c_void_p(host.ctypes.data)
    ty = np.ascontiguousarray(types, np.int32)
    tot = (C.c_uint64 * 4)(7, 7, 7, 7)
    rc = L.mtblx_scan_plan(p if file else None, 1000, version, 0, 0, 100, None, None, None, None, 0, None,
                           C.c_void_p(ty.ctypes.data), p, p, p if keys2 else None, p if keys2 else None, None, 64, nq,
                           p, tot if totals else None, wp, wsb, None)
    return rc, list(tot)


def test_argument_checks_need_no_device(mtblx_lib):
    """NULL / misaligned / small workspace, a bad type, version > 1: MTBLX_E_INVAL before any device
    call; nq == 0: MTBLX_OK with zero totals"""
    from mtblx import _lib
    L = mtblx_lib
    need = L.mtblx_scan_workspace_bytes(1)
    host = np.zeros(need + 512, np.uint8)           # an aligned, non-NULL address; never dereferenced
    wp = (host.ctypes.data + 255) & ~255
    INVAL = _lib.MTBLX_E_INVAL
    assert _plan(L, None, need)[0] == INVAL
    assert _plan(L, C.c_void_p(wp + 8), need)[0] == INVAL
    assert _plan(L, C.c_void_p(wp), need - 1)[0] == INVAL
    assert _plan(L, C.c_void_p(wp), need, version=2)[0] == INVAL
    assert _plan(L, C.c_void_p(wp), need, types=(4,))[0] == INVAL
    assert _plan(L, C.c_void_p(wp), need, types=(-1,))[0] == INVAL
    assert _plan(L, C.c_void_p(wp), need, types=(3,), keys2=False)[0] == INVAL   # a range without end keys
    assert _plan(L, C.c_void_p(wp), need, file=False)[0] == INVAL
    assert _plan(L, C.c_void_p(wp), need, totals=False)[0] == INVAL
    assert _plan(L, C.c_void_p(wp), L.mtblx_scan_workspace_bytes(2) - 1, nq=2, types=(0, 1))[0] == INVAL
    rc, tot = _plan(L, C.c_void_p(wp), need, nq=0)
    assert rc == _lib.MTBLX_OK and tot == [0, 0, 0, 0]

    flags = np.zeros(1, np.uint32)
    out = _lib.Scanned(0, 0, 0, 0, 0, 0, 0, flags.ctypes.data)
    p = C.c_void_p(host.ctypes.data)

    def emit(wsp, wsb, nq=1, version=1, o=out):
        return L.mtblx_scan_emit(p, 1000, version, 0, 100, None, None, None, None, 0, None, nq,
                                 C.byref(o) if o is not None else None, wsp, wsb, None)

    assert emit(None, need) == INVAL
    assert emit(C.c_void_p(wp + 8), need) == INVAL
    assert emit(C.c_void_p(wp), need - 1) == INVAL
    assert emit(C.c_void_p(wp), need, version=2) == INVAL
    assert emit(C.c_void_p(wp), need, o=None) == INVAL
    assert emit(C.c_void_p(wp), need, o=_lib.Scanned(0, 0, 0, 0, 0, 0, 0, 0)) == INVAL          # no flags word
    assert emit(C.c_void_p(wp), need, o=_lib.Scanned(0, 8, 0, 0, 0, 0, 0, flags.ctypes.data)) == INVAL
    assert emit(C.c_void_p(wp), need, nq=0) == _lib.MTBLX_OK
    assert flags[0] == 0


@pytest.mark.parametrize("name", su.CPU_FILES)
def test_span_helper_against_oracle(oracle, name):
    """scan_util.span: the records between its first and stop positions are the oracle's records of
    every query, so the blocks it counts are the blocks the iteration opens; and at most 40 % of the
    prefix / range queries open more than 4"""
    data, recs, qs, lim = su.case(name)
    keys = [k for k, _ in recs]
    ikeys = [k for k, _ in oracle.index_records(data)]
    assert len(ikeys) > 64
    large = scans = 0
    for q, m in zip(qs, lim):
        e = su.expected(oracle, data, q, m, True, tag=name)
        assert e["end"] == 0
        first, stop, opened = su.span(ikeys, keys, q, len(e["records"]))
        assert recs[first:stop] == e["records"], (q, m)
        if q[0] in ("prefix", "range"):
            scans += 1
            large += opened > 4
    assert scans >= 215 and large <= 0.4 * scans, (large, scans)

"""Device merge functions, the parts that need no GPU: the Reduce spec, Reduce.host against
hand-computed vectors, and the argument checks of mtblx_merge_emit_reduce / mtblx_sort_emit_reduce,
which come before any HIP call (include/mtblx.h "Device merge functions")."""
import ctypes as C

import pytest

M = (1 << 64) - 1


def u(*xs):
    return b"".join(int(x).to_bytes(8, "little") for x in xs)


def test_reduce_construction():
    import mtblx
    assert mtblx.Reduce("sum").ops == ("sum",) and mtblx.Reduce("sum").width == 8
    assert mtblx.Reduce(*["max"] * 8).width == 64
    with pytest.raises(ValueError):
        mtblx.Reduce()
    with pytest.raises(ValueError):
        mtblx.Reduce(*["sum"] * 9)
    for bad in ("avg", "SUM", "sum_u64", 0, None):
        with pytest.raises(ValueError):
            mtblx.Reduce(bad)
    assert not callable(mtblx.Reduce("sum"))   # a callable would take the host path
    assert issubclass(mtblx.MergeError, RuntimeError)
    assert "Reduce" in mtblx.__all__ and "MergeError" in mtblx.__all__


def test_shorthands():
    from mtblx import reduce
    assert reduce.as_reduce("sum_u64") == reduce.Reduce("sum")
    assert reduce.as_reduce("min_u64") == reduce.Reduce("min")
    assert reduce.as_reduce("max_u64") == reduce.Reduce("max")
    assert reduce.as_reduce("concat") is None and reduce.as_reduce(len) is None
    assert reduce.check_merge("concat") == "concat" and reduce.check_merge(len) is len
    with pytest.raises(ValueError):
        reduce.check_merge("sum")


def test_host_vectors():
    import mtblx
    R = mtblx.Reduce
    assert R("sum").host(b"k", [u(M), u(2)]) == u(1)                       # 2^64 - 1 + 2 wraps to 1
    assert R("sum").host(b"k", [u(1), u(2), u(3)]) == u(6)
    top = 1 << 63                                                          # negative if read as signed
    assert R("min").host(b"k", [u(top), u(5), u(top + 9)]) == u(5)
    assert R("max").host(b"k", [u(top), u(5), u(top + 9)]) == u(top + 9)
    assert R("min").host(b"k", [u(M), u(top)]) == u(top)
    assert R("max").host(b"k", [u(0), u(M)]) == u(M)
    got = R("sum", "min", "max").host(b"k", [u(1, 100, 100), u(1, 90, 250), u(M, 95, 120)])
    assert got == u(1, 90, 250)                                            # (count, time_first, time_last)
    assert R("sum").host(b"k", [bytes(range(8)), bytes(8)]) == bytes(range(8))


def test_host_wrong_length():
    import mtblx
    for vals in ([u(1), b"\x01" * 7], [b"\x01" * 7, u(1)], [u(1, 2), u(1, 2)], [b"", b""]):
        with pytest.raises(mtblx.MergeError):
            mtblx.Reduce("sum").host(b"k", vals)
    with pytest.raises(mtblx.MergeError):
        mtblx.Reduce("sum", "max").host(b"k", [u(1, 2), u(1)])


def test_abi_version_still_3(mtblx_lib):
    assert mtblx_lib.mtblx_abi_version() == 3


def test_emit_reduce_rejects_bad_specs(mtblx_lib):
    """NULL spec, nfields 0, nfields 9, an op of 3: MTBLX_E_INVAL before any HIP call (the other
    arguments are NULL too, so a call that got past the spec check would still be refused, but one
    that touched the device would not return at all on a machine without one)"""
    from mtblx import _lib
    assert _lib.MERGE_BADVALUE == 4 and _lib.REDUCE_MAX_FIELDS == 8
    assert (_lib.REDUCE_SUM, _lib.REDUCE_MIN, _lib.REDUCE_MAX) == (0, 1, 2)
    assert C.sizeof(_lib.ReduceSpec) == 12
    flags = C.c_uint32(0x5A5A)
    out = _lib.Merged(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, C.addressof(flags))
    rec = _lib.Records(0, 0, 0, 0, 0)
    ws = C.create_string_buffer(1 << 16)
    wp = (C.addressof(ws) + 255) & ~255
    wsb = (1 << 16) - 256
    assert wsb >= mtblx_lib.mtblx_sort_workspace_bytes(0) and wsb >= mtblx_lib.mtblx_merge_workspace_bytes(0, 1)

    def spec(nfields, ops=()):
        s = _lib.ReduceSpec()
        s.nfields = nfields
        for i, o in enumerate(ops):
            s.op[i] = o
        return s

    bad = [None, spec(0), spec(9), spec(1, [3]), spec(3, [0, 1, 3]), spec(8, [2] * 7 + [255])]
    for s in bad:
        p = C.byref(s) if s is not None else None
        assert mtblx_lib.mtblx_sort_emit_reduce(C.byref(rec), p, C.byref(out), C.c_void_p(wp), wsb, None) == _lib.MTBLX_E_INVAL
        assert mtblx_lib.mtblx_merge_emit_reduce(C.byref(rec), 1, p, C.byref(out), C.c_void_p(wp), wsb, None) == _lib.MTBLX_E_INVAL
    assert flags.value == 0x5A5A
    # a good spec still meets everything the plain emits refuse
    good = spec(2, [0, 2])
    assert mtblx_lib.mtblx_sort_emit_reduce(C.byref(rec), C.byref(good), None, C.c_void_p(wp), wsb, None) == _lib.MTBLX_E_INVAL
    assert mtblx_lib.mtblx_sort_emit_reduce(C.byref(rec), C.byref(good), C.byref(out), None, wsb, None) == _lib.MTBLX_E_INVAL
    assert mtblx_lib.mtblx_sort_emit_reduce(None, C.byref(good), C.byref(out), C.c_void_p(wp), wsb, None) == _lib.MTBLX_E_INVAL
    assert mtblx_lib.mtblx_merge_emit_reduce(C.byref(rec), 65, C.byref(good), C.byref(out), C.c_void_p(wp), wsb, None) == _lib.MTBLX_E_INVAL
    assert mtblx_lib.mtblx_merge_emit_reduce(C.byref(rec), 1, C.byref(good), C.byref(out), C.c_void_p(wp + 8), wsb, None) == _lib.MTBLX_E_INVAL
    assert mtblx_lib.mtblx_merge_emit_reduce(C.byref(rec), 1, C.byref(good), C.byref(out), C.c_void_p(wp), 0, None) == _lib.MTBLX_E_INVAL


def test_workspace_holds_the_edge_array(mtblx_lib):
    """both workspace sizes grow by at least the per-tile edge records (144 B per 1024 records) over
    the arrays of the plain emits (~90 B per record), and agree"""
    n = 1_000_000
    a, b = mtblx_lib.mtblx_sort_workspace_bytes(n), mtblx_lib.mtblx_merge_workspace_bytes(n, 3)
    assert a == b
    per_record = 16 + 16 + 1 + 4 + 4 + 8 * 4
    tiles = (n + 1023) // 1024
    assert a >= per_record * n + 48 * tiles + 144 * tiles

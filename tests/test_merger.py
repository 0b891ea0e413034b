"""The Merger without a GPU: the model the GPU tests compare with (tests/merger_model.py, a
restatement of src/merger.rs's MergerIter / MultiIter) against the reference's own test
scenarios and the empty-key quirk worked out by hand; the new symbols; the argument checks."""
import ctypes as C

import numpy as np

import merger_model as mm


def test_model_easy_scenario(oracle):
    """src/merger.rs:267-304: ten overlapping sources of {:010} keys, all values empty; the merged
    keys are strictly increasing (and here: exactly 0 .. 299), through real .mtbl files"""
    src = [mm.source_records(mm.make_source(s)) for s in mm.easy_sources()]
    assert src == mm.easy_sources()
    out = mm.merge_iter(src, mm.concat)
    keys = [k for k, _ in out]
    assert all(a < b for a, b in zip(keys, keys[1:]))
    assert keys == [b"%010d" % j for j in range(300)]
    assert all(v == b"" for _, v in out)
    multi = dict(mm.multi_iter(src))
    assert len(multi[b"%010d" % 0]) == 1 and len(multi[b"%010d" % 9]) == 10 and len(multi[b"%010d" % 299]) == 1


def test_model_sorter_simple():
    """src/sorter.rs:265-295 for concat: abstract -> lollol, allo -> lol, hello -> kiki"""
    s0 = [(b"abstract", b"lol"), (b"allo", b"lol"), (b"hello", b"kiki")]
    s1 = [(b"abstract", b"lol")]
    assert mm.merge_iter([s0, s1], mm.concat) == [(b"abstract", b"lollol"), (b"allo", b"lol"), (b"hello", b"kiki")]


def test_model_empty_key_quirk():
    """src/merger.rs:182-186 by hand.  E = sources whose first record has the empty key."""
    # E = 1 with followers: "" is adopted, its value pushed; the next entry re-adopts (cur_key is
    # still empty) and clears cur_vals: the empty-key record vanishes
    a = [(b"", b"x"), (b"a", b"1")]
    b = [(b"a", b"2"), (b"b", b"3")]
    assert mm.canon(mm.multi_iter([a, b])) == [(b"a", [b"1", b"2"]), (b"b", [b"3"])]
    assert mm.merge_iter([a, b], mm.concat) in ([(b"a", b"12"), (b"b", b"3")], [(b"a", b"21"), (b"b", b"3")])
    # E = 1 alone: the heap empties with pending set: one item, the merge function not called
    assert mm.multi_iter([[(b"", b"x")]]) == [(b"", [b"x"])]
    assert mm.merge_iter([[(b"", b"x")]], mm.concat) == [(b"", b"x")]
    # E = 3 with followers: all three vanish, and the followers group as usual
    s = [[(b"", b"x%d" % i), (b"k", b"v%d" % i)] for i in range(3)]
    assert mm.canon(mm.multi_iter(s)) == [(b"k", [b"v0", b"v1", b"v2"])]
    # E = 3 alone: every adoption clears cur_vals: one item holding one value (which one is heap order)
    out = mm.multi_iter([[(b"", b"x%d" % i)] for i in range(3)])
    assert len(out) == 1 and out[0][0] == b"" and len(out[0][1]) == 1


def test_symbols_bound(mtblx_lib):
    import mtblx
    from mtblx import _lib
    for n in ("mtblx_merge_workspace_bytes", "mtblx_merge_plan", "mtblx_merge_emit"):
        assert n in mtblx.EXPORTS
        assert getattr(mtblx_lib, n).argtypes is not None
    assert mtblx_lib.mtblx_abi_version() == 3
    assert C.sizeof(_lib.Merged) == 88 and C.sizeof(_lib.Records) == 40
    assert mtblx_lib.mtblx_merge_workspace_bytes(1000, 8) >= 2 * 16 * 1000
    assert mtblx_lib.mtblx_merge_workspace_bytes(0, 0) > 0
    assert {"Merger", "MergerBuilder"} <= set(mtblx.__all__)


def test_argument_checks_need_no_device(mtblx_lib):
    """NULL workspace, more than 64 sources, a workspace too small: MTBLX_E_INVAL before any device call"""
    from mtblx import _lib
    L = mtblx_lib
    tot = (C.c_uint64 * 6)()
    host = np.zeros(4096 + 256, np.uint8)           # an aligned, non-NULL address; never dereferenced
    wp = (host.ctypes.data + 255) & ~255
    one = (_lib.Records * 1)()
    one[0] = _lib.Records(0, 0, 0, 0, 1000)
    need = L.mtblx_merge_workspace_bytes(1000, 1)
    flags = np.zeros(1, np.uint32)
    out = _lib.Merged(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, flags.ctypes.data)
    assert L.mtblx_merge_plan(one, 1, tot, None, need, None) == _lib.MTBLX_E_INVAL
    assert L.mtblx_merge_emit(one, 1, _lib.MERGE_CONCAT, C.byref(out), None, need, None) == _lib.MTBLX_E_INVAL
    many = (_lib.Records * 65)()
    assert L.mtblx_merge_plan(many, 65, tot, C.c_void_p(wp), 1 << 40, None) == _lib.MTBLX_E_INVAL
    assert L.mtblx_merge_emit(many, 65, _lib.MERGE_CONCAT, C.byref(out), C.c_void_p(wp), 1 << 40, None) == \
        _lib.MTBLX_E_INVAL
    assert need > 4096
    assert L.mtblx_merge_plan(one, 1, tot, C.c_void_p(wp), 4096, None) == _lib.MTBLX_E_INVAL
    assert L.mtblx_merge_emit(one, 1, _lib.MERGE_CONCAT, C.byref(out), C.c_void_p(wp), need - 1, None) == \
        _lib.MTBLX_E_INVAL
    assert L.mtblx_merge_plan(one, 1, tot, C.c_void_p(wp + 8), need, None) == _lib.MTBLX_E_INVAL   # misaligned
    assert L.mtblx_merge_emit(one, 1, 7, C.byref(out), C.c_void_p(wp), need, None) == _lib.MTBLX_E_INVAL   # mode

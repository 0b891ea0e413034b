"""The Sorter without a GPU: the model the GPU tests compare with (tests/sorter_model.py, a
restatement of src/sorter.rs) against the reference's own test and cut positions worked out by
hand; the new symbols; the argument checks; and the Python Sorter's chunk rule against the model,
with host stand-ins where the device sort and merge would run."""
import ctypes as C

import numpy as np
import pytest

import merger_model as mm
import sorter_model as sm

MIN = sm.MIN_SORTER_MEMORY


def test_model_simple():
    """src/sorter.rs:264-295: the merge function asserts that it never sees one value"""
    out, s = sm.run([(b"hello", b"kiki"), (b"abstract", b"lol"), (b"allo", b"lol"), (b"abstract", b"lol")], mm.concat)
    assert out == [(b"abstract", b"lollol"), (b"allo", b"lol"), (b"hello", b"kiki")]
    assert s.chunk_sizes == [4] and s.merges == 0


def test_model_cut_1024_byte_entries():
    """max_memory at its minimum, 8 B key + 1016 B value: 6144 * 1024 + 131 072 * 32 = 6 291 456 +
    4 194 304 = 10 485 760: the 6144th insert cuts, and so does every 6144th after it"""
    s = sm.Sorter(sm.concat_any, max_memory=0)
    assert s.max_memory == MIN
    for i in range(2 * 6144 + 5):
        s.insert(b"%08d" % i, b"v" * 1016)
        if i == 6142:
            assert s.cuts == []
    assert s.cuts == [6144, 12288] and s.chunk_sizes == [6144, 6144] and s.capacity == 131_072


def test_model_cut_16_byte_entries():
    """16-byte entries: insert 131 073 finds the Vec full and doubles it to 262 144, and
    131 073 * 16 + 262 144 * 32 = 2 097 168 + 8 388 608 >= 10 485 760 cuts; the capacity survives
    the drain, so every later cut comes 131 072 inserts after the one before (2 097 152 + 8 388 608)"""
    s = sm.Sorter(sm.concat_any, max_memory=MIN)
    for i in range(131_073 + 2 * 131_072 + 1):
        s.insert(b"%08d" % i, b"12345678")
    assert s.cuts == [131_073, 131_073 + 131_072, 131_073 + 2 * 131_072]
    assert s.chunk_sizes == [131_073, 131_072, 131_072] and s.capacity == 262_144


def test_model_empty_keys():
    """write_chunk keeps the empty-key group (an Option, :154); the Merger of into_iter then applies
    its quirk: the group vanishes when another record follows and survives alone"""
    out, _ = sm.run([(b"", b"a"), (b"", b"b"), (b"x", b"c")], sm.concat_any)
    assert out == [(b"x", b"c")]
    out, _ = sm.run([(b"", b"a"), (b"", b"b")], sm.concat_any)
    assert out == [(b"", b"ab")]


def test_symbols(mtblx_lib):
    import mtblx
    from mtblx import _lib
    L = mtblx_lib
    for name in ("mtblx_sort_workspace_bytes", "mtblx_sort_plan", "mtblx_sort_plan_timed", "mtblx_sort_emit"):
        assert name in mtblx.EXPORTS
        assert getattr(L, name).argtypes, name
    assert L.mtblx_abi_version() == 3
    assert L.mtblx_sort_workspace_bytes(1000) >= 2 * 16 * 1000
    assert L.mtblx_sort_workspace_bytes(0) > 0
    assert "Sorter" in mtblx.__all__ and "SorterBuilder" in mtblx.__all__
    assert _lib.SORT_TILE >= 2 and _lib.SORT_TILE & (_lib.SORT_TILE - 1) == 0
    from mtblx import sorter
    assert mtblx.Sorter is sorter.Sorter and mtblx.SorterBuilder is sorter.SorterBuilder


def test_argument_checks_need_no_device(mtblx_lib):
    """every case MTBLX_E_INVAL before any device call"""
    from mtblx import _lib
    L = mtblx_lib
    tot = (C.c_uint64 * 6)()
    host = np.zeros((1 << 17) + 256, np.uint8)      # an aligned, non-NULL address; never dereferenced
    wp = (host.ctypes.data + 255) & ~255
    ends = np.zeros(1000, np.uint64)                # non-NULL END arrays; never dereferenced
    one = _lib.Records(0, ends.ctypes.data, 0, ends.ctypes.data, 1000)
    need = L.mtblx_sort_workspace_bytes(1000)
    assert 0 < need <= 1 << 17
    flags = np.zeros(1, np.uint32)
    out = _lib.Merged(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, flags.ctypes.data)
    E = _lib.MTBLX_E_INVAL

    def plan(rec, ws, wsb):
        return L.mtblx_sort_plan(C.byref(rec), tot, ws, wsb, None)

    def emit(rec, mode, ws, wsb):
        return L.mtblx_sort_emit(C.byref(rec), mode, C.byref(out), ws, wsb, None)

    ph = (C.c_float * 32)()
    assert plan(one, None, need) == E                                             # NULL workspace
    assert emit(one, _lib.MERGE_CONCAT, None, need) == E
    assert L.mtblx_sort_plan_timed(C.byref(one), tot, None, need, None, ph, 32) == E
    assert plan(one, C.c_void_p(wp + 8), need) == E                               # misaligned
    assert emit(one, _lib.MERGE_CONCAT, C.c_void_p(wp + 8), need) == E
    assert plan(one, C.c_void_p(wp), need - 1) == E                               # one byte too small
    assert emit(one, _lib.MERGE_CONCAT, C.c_void_p(wp), need - 1) == E
    assert emit(one, 4, C.c_void_p(wp), need) == E and emit(one, -1, C.c_void_p(wp), need) == E   # mode
    big = _lib.Records(0, ends.ctypes.data, 0, ends.ctypes.data, (1 << 32) - 16)
    assert L.mtblx_sort_workspace_bytes((1 << 32) - 16) == 0
    assert plan(big, C.c_void_p(wp), 1 << 60) == E                                # n = 2^32 - 16
    assert emit(big, _lib.MERGE_CONCAT, C.c_void_p(wp), 1 << 60) == E
    nokey = _lib.Records(0, 0, 0, ends.ctypes.data, 1000)
    assert plan(nokey, C.c_void_p(wp), need) == E                                 # NULL key_end, n > 0
    assert emit(nokey, _lib.MERGE_CONCAT, C.c_void_p(wp), need) == E
    assert host.sum() == 0 and flags[0] == 0 and list(tot) == [0] * 6


# ---------------------------------------------------------------- the Python Sorter's chunk rule
def _host_sorter(monkeypatch, merge="concat", **kw):
    """mtblx.sorter.Sorter on CPU tensors, sort_records / merge_all replaced by the model's steps"""
    torch = pytest.importorskip("torch")
    from mtblx import encode, merger, sorter

    def sort_records(recs, mode, stream=None):
        assert mode == "concat"
        w = sm.Sorter(sm.concat_any)
        w.entries = merger._records_list(recs)
        w.write_chunk()
        return encode.DeviceRecords.from_list(w.chunks[0], device="cpu")

    def merge_all(chunks, mode, stream=None, device=None):
        assert mode == "concat"
        return encode.DeviceRecords.from_list(mm.merge_iter([merger._records_list(c) for c in chunks], sm.concat_any),
                                              device="cpu")

    monkeypatch.setattr(sorter, "sort_records", sort_records)
    monkeypatch.setattr(sorter, "merge_all", merge_all)
    b = sorter.Sorter.builder(merge, device="cpu")
    for k, v in kw.items():
        getattr(b, k)(v)
    return b.build()


def _batch(records):
    ks, vs = b"".join(k for k, _ in records), b"".join(v for _, v in records)
    return (np.frombuffer(ks, np.uint8), np.cumsum([len(k) for k, _ in records]).astype(np.uint64),
            np.frombuffer(vs, np.uint8), np.cumsum([len(v) for _, v in records]).astype(np.uint64))


def test_builder_defaults_and_clamps():
    pytest.importorskip("torch")
    from mtblx import CompressionType, sorter
    s = sorter.Sorter("concat", device="cpu")
    assert (s.max_memory, s.max_nb_chunks) == (1_073_741_824, 25)
    assert (s.chunk_compression_type, s.chunk_compression_level) == (CompressionType.Snappy, 0)
    s = sorter.SorterBuilder("first", device="cpu").max_memory(5).max_nb_chunks(0) \
        .chunk_compression_type(CompressionType.Zlib).chunk_compression_level(7).build()
    assert (s.max_memory, s.max_nb_chunks) == (MIN, 1)
    assert (s.chunk_compression_type, s.chunk_compression_level) == (CompressionType.Zlib, 7)
    assert isinstance(s, sorter.Sorter) and isinstance(sorter.Sorter.builder("last", device="cpu"), sorter.SorterBuilder)
    with pytest.raises(ValueError):
        sorter.Sorter("sum", device="cpu")


@pytest.mark.parametrize("how", ["insert", "insert_batch", "mixed"])
def test_cuts_1024_byte_entries(monkeypatch, how):
    """three chunks' worth and 100 more with max_nb_chunks(1): cuts at every 6144th insert, two
    runs of merge_chunks, and the model's result"""
    rng = np.random.default_rng(3)
    keys = rng.integers(0, 9000, size=3 * 6144 + 100)
    records = [(b"%08d" % k, bytes([i & 0xFF]) * 1016) for i, k in enumerate(keys)]
    want, model = sm.run(records, sm.concat_any, max_memory=MIN, max_nb_chunks=1)
    assert model.chunk_sizes == [6144, 6144, 6144, 100] and model.merges == 2
    s = _host_sorter(monkeypatch, max_memory=0, max_nb_chunks=1)
    if how == "insert":
        for k, v in records:
            s.insert(k, v)
    elif how == "insert_batch":
        s.insert_batch(*_batch(records))
    else:   # single inserts between batches that end just before, at and just after a cut
        s.insert_batch(*_batch(records[:6143]))
        s.insert(*records[6143])
        s.insert(*records[6144])
        s.insert_batch(*_batch(records[6145: 2 * 6144]))
        s.insert_batch(*_batch(records[2 * 6144: 3 * 6144 + 1]))
        for k, v in records[3 * 6144 + 1:]:
            s.insert(k, v)
    assert s.chunk_sizes == [6144, 6144, 6144] and s.merges == 2
    got = list(s.into_iter())
    assert s.chunk_sizes == model.chunk_sizes and s.merges == model.merges
    assert [k for k, _ in got] == [k for k, _ in want]
    piece = lambda v: sorted(v[i: i + 1016] for i in range(0, len(v), 1016))   # noqa: E731
    assert [piece(v) for _, v in got] == [piece(v) for _, v in want]


def test_cuts_16_byte_entries_batch(monkeypatch):
    """the capacity doubling inside insert_batch: chunk_sizes starts [131 073, 131 072], as the model's"""
    n = 131_073 + 131_072 + 10
    keys = np.arange(n, dtype=np.uint64)[::-1].copy().byteswap().view(np.uint8)   # 8-byte big-endian, descending
    ends = (np.arange(1, n + 1, dtype=np.uint64) * 8)
    s = _host_sorter(monkeypatch, max_memory=MIN)
    s.insert_batch(keys, ends, keys, ends)
    assert s.chunk_sizes == [131_073, 131_072] and s._capacity == 262_144 and s._len == 10
    assert s.entry_bytes == 160 and s.merges == 0
    r = s.records()
    assert s.chunk_sizes == [131_073, 131_072, 10] and r.n == n
    assert bytes(r.keys[:16].tolist()) == (0).to_bytes(8, "big") + (1).to_bytes(8, "big")
    with pytest.raises(RuntimeError):
        s.records()


def test_empty_sorter_pushes_an_empty_chunk(monkeypatch):
    """into_iter runs write_chunk also when nothing is pending (:246)"""
    s = _host_sorter(monkeypatch)
    assert list(s.into_iter()) == [] and s.chunk_sizes == [0] and len(s.chunks) == 1

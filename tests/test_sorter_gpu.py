"""The device Sorter (mtblx/sorter.py over mtblx_sort_plan / mtblx_sort_emit, csrc/sort.hip) against
this library's promise and against tests/sorter_model.py (src/sorter.rs restated).

The yardstick is `promised(records)`, worked out here: a stable sort by key, then grouping -- no
quirk for sort_records, the Sorter's quirk rule (the empty-key group vanishes when any other key
exists) for the Sorter.  Where the model is deterministic, i.e. with a single chunk, it must give
the same; across chunks the model's heap order is one of several the reference allows, so there
the key sequence and the multiset of values per key are compared."""
import ctypes as C

import numpy as np
import pytest

import merger_model as mm
import sorter_model as sm

pytestmark = pytest.mark.gpu

PICK = {"concat": b"".join, "first": lambda vs: vs[0], "last": lambda vs: vs[-1]}


def _mods():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mtblx import _lib, encode, merger, sorter
    return torch, _lib, encode, merger, sorter


def promised(records, quirk=False):
    """[(key, [values in input order])]"""
    out = []
    for k, v in sorted(records, key=lambda r: r[0]):   # stable
        if out and out[-1][0] == k:
            out[-1][1].append(v)
        else:
            out.append((k, [v]))
    if quirk and len(out) > 1 and out[0][0] == b"":
        out = out[1:]
    return out


def _check_sort(records, oracle=None):
    """sort_records in all four modes; with `oracle`, the written file too"""
    torch, _lib, encode, merger, sorter = _mods()
    want = promised(records)
    recs = encode.DeviceRecords.from_list(records)
    got = sorter.sort_records(recs, "groups")
    assert got.to_list() == want
    for mode, pick in PICK.items():
        r = sorter.sort_records(recs, mode)
        exp = [(k, pick(vs)) for k, vs in want]
        assert merger._records_list(r) == exp, mode
        if oracle is not None and mode == "concat":
            file = encode.write_file(r, 1024, 16).cpu().numpy().tobytes()
            assert file == oracle.write_file(exp, 1024, 16)
    if len(records) < 20_000:   # single chunk: the model is deterministic and has the Merger's quirk
        model, _ = sm.run(records, sm.concat_any)
        assert model == [(k, b"".join(vs)) for k, vs in promised(records, quirk=True)]
    return want


def _dup_records(n, seed):
    """n records, about half of the keys occurring twice or more, every value its input position"""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, max(n * 2 // 3, 1), size=n)
    return [(b"key-%07d" % k, b"%d," % i) for i, k in enumerate(keys)]


def _tile():
    from mtblx import _lib
    return _lib.SORT_TILE


@pytest.mark.parametrize("shape", ["0", "1", "2", "T-1", "T", "T+1", "2T+1", "5T+7"])
def test_sizes_around_the_tile(oracle, shape):
    """2T+1: three runs, an unpaired one in the first pass; 5T+7: an odd run count at two levels"""
    T = _tile()
    n = {"0": 0, "1": 1, "2": 2, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+1": 2 * T + 1, "5T+7": 5 * T + 7}[shape]
    want = _check_sort(_dup_records(n, 40 + n % 13), oracle)
    assert sum(len(vs) for _, vs in want) == n


def _pool_records(n, seed, common=b""):
    """the key pool of test_merger_gpu._random_sources, drawn with replacement, in random order"""
    rng = np.random.default_rng(seed)

    def word(alpha, lo, hi):
        return bytes(rng.choice(alpha, size=int(rng.integers(lo, hi + 1))).tolist())

    pool = set()
    for _ in range(700):
        pool.add(common + word([0x61, 0x62, 0x00], 1, 6))                           # "ab" < "ab\0", duplicates
        pool.add(common + word([0x7F, 0x80, 0xFF], 1, 5))                           # a signed compare would misorder
        pool.add(common + b"shared-run-" + word([0x61, 0x62, 0x00], 0, 29 - len(common)))   # > 8 equal leading bytes
    pool = sorted(k for k in pool if len(k) <= 40)
    idx = rng.integers(0, len(pool), size=n)
    return [(pool[j], bytes([i & 0xFF]) * int(rng.integers(0, 40)) + b"#%d" % i) for i, j in enumerate(idx)]


@pytest.mark.parametrize("shape", ["pool", "common12", "all_equal", "sorted", "reversed", "empty_values",
                                   "empty_keys", "long_keys"])
def test_key_shapes(oracle, shape):
    n = 3000
    with_file = oracle
    if shape == "pool":
        records = _pool_records(n, 1)
    elif shape == "common12":   # the handle's prefix is taken after the 12 shared bytes
        records = _pool_records(n, 2, common=b"common-12-by")
        assert all(k.startswith(b"common-12-by") for k, _ in records)
    elif shape == "all_equal":  # one group of 3000 values, in input order
        records = [(b"the-one-key", b"%d;" % i) for i in range(n)]
    elif shape == "sorted":
        records = [(b"k%06d" % (i // 2), b"%d" % i) for i in range(n)]
    elif shape == "reversed":
        records = [(b"k%06d" % ((n - i) // 2), b"%d" % i) for i in range(n)]
    elif shape == "empty_values":
        records = [(k, b"") for k, _ in _pool_records(n, 3)]
    elif shape == "empty_keys":  # the group is kept by sort_records, values in input order
        records = [(b"" if i % 7 == 0 else k, v) for i, (k, v) in enumerate(_pool_records(n, 4))]
        with_file = None         # the Writer refuses an empty first key
    else:                        # two keys of 70 000 bytes that differ in the last byte
        a = bytes(np.random.default_rng(5).integers(0, 256, size=69_999, dtype=np.uint8).tolist())
        records = [(a + b"\x02", b"v0"), (a + b"\x01", b"v1"), (a + b"\x02", b"v2"), (a + b"\x01", b"v3")]
    want = _check_sort(records, with_file)
    if shape == "all_equal":
        assert want == [(b"the-one-key", [b"%d;" % i for i in range(n)])]
    if shape == "empty_keys":
        assert want[0][0] == b"" and len(want[0][1]) == len(range(0, n, 7))
    if shape == "long_keys":
        assert [vs for _, vs in want] == [[b"v1", b"v3"], [b"v0", b"v2"]]


def test_all_keys_and_values_empty():
    """keys and vals NULL-able: every key and every value empty"""
    want = _check_sort([(b"", b"")] * 1500)
    assert want == [(b"", [b""] * 1500)]


def test_200k_records():
    """~8 passes, every pass spanning ~200 workgroup slices"""
    torch, _lib, encode, merger, sorter = _mods()
    rng = np.random.default_rng(21)
    n = 200_003
    keys = rng.integers(0, 150_000, size=n)
    records = [(b"%08d" % k, bytes([i & 0xFF]) * (i % 5)) for i, k in enumerate(keys)]
    want = promised(records)
    recs = encode.DeviceRecords.from_list(records)
    assert sorter.sort_records(recs, "groups").to_list() == want
    assert merger._records_list(sorter.sort_records(recs, "last")) == [(k, vs[-1]) for k, vs in want]


# ---------------------------------------------------------------- the bare C ABI
class _Raw:
    """plan + emit (each the sort's or the merge's) over ONE batch with buffers the test owns: every
    output is a slice of a 0xA5-filled buffer, `short[name]` bytes smaller than the plan's size,
    with a 64-byte guard on both sides"""

    def __init__(self, records, mode, plan="sort", emit="sort", short=None):
        torch, _lib, encode, merger, sorter = _mods()
        L = __import__("mtblx").lib()
        short = short or {}
        self.rec = encode.DeviceRecords.from_list(records)
        one = (_lib.Records * 1)()
        one[0] = self.rec.cstruct()
        n = self.rec.n
        wsb = max(int(L.mtblx_sort_workspace_bytes(n)), int(L.mtblx_merge_workspace_bytes(n, 1)))
        ws = torch.empty(wsb + 256, dtype=torch.uint8, device="cuda")
        wp = (ws.data_ptr() + 255) & ~255
        tot = (C.c_uint64 * 6)()
        if plan == "sort":
            self.rc_plan = L.mtblx_sort_plan(one, tot, C.c_void_p(wp), wsb, None)
        else:
            self.rc_plan = L.mtblx_merge_plan(one, 1, tot, C.c_void_p(wp), wsb, None)
        self.totals = [int(x) for x in tot]
        groups, kb, nv, vb = self.totals[:4]
        grouped = mode == _lib.MERGE_GROUPS
        self.size = {"keys": kb, "key_end": 8 * groups, "vals": vb, "val_end": 8 * (nv if grouped else groups),
                     "grp_end": 8 * groups if grouped else 0}
        self.cap, self.buf, ptr = {}, {}, {}
        for name, sz in self.size.items():
            self.cap[name] = max(sz - short.get(name, 0), 0)
            t = torch.full((64 + sz + 64 + 16,), 0xA5, dtype=torch.uint8, device="cuda")
            ptr[name] = (t.data_ptr() + 64 + 15) & ~15
            self.buf[name] = (t, ptr[name] - t.data_ptr())
        flags = torch.full((1,), 0x5A5A, dtype=torch.int32, device="cuda")
        out = _lib.Merged(ptr["keys"], self.cap["keys"], ptr["key_end"], self.cap["key_end"], ptr["vals"],
                          self.cap["vals"], ptr["val_end"], self.cap["val_end"], ptr["grp_end"], self.cap["grp_end"],
                          flags.data_ptr())
        if emit == "sort":
            self.rc_emit = L.mtblx_sort_emit(one, mode, C.byref(out), C.c_void_p(wp), wsb, None)
        else:
            self.rc_emit = L.mtblx_merge_emit(one, 1, mode, C.byref(out), C.c_void_p(wp), wsb, None)
        torch.cuda.synchronize()
        self.flags = int(flags.item())

    def bytes(self, name):
        t, off = self.buf[name]
        return t[off: off + self.size[name]].cpu().numpy().tobytes()

    def untouched_from(self, name, start):
        t, off = self.buf[name]
        return bool((t[off + start:] == 0xA5).all()) and bool((t[:off] == 0xA5).all())


def _sorted_unique(n):
    return [(b"k%05d" % i, b"v%d" % i) for i in range(n)]


@pytest.mark.parametrize("n", [300, 2500])
def test_emit_refuses_the_other_kind_of_plan(n):
    """an emit of one kind over a workspace planned by the other: NOT_PLANNED, nothing written
    (2500 records: the sort's result lies in the other handle array than the merge's)"""
    torch, _lib, encode, merger, sorter = _mods()
    records = _sorted_unique(n)   # legal input of both
    for plan, emit in (("merge", "sort"), ("sort", "merge")):
        r = _Raw(records, _lib.MERGE_CONCAT, plan=plan, emit=emit)
        assert r.rc_plan == 0 and r.totals[0] == n
        assert r.rc_emit == 0 and r.flags == _lib.MERGE_NOT_PLANNED
        assert all(r.untouched_from(name, 0) for name in r.size)
    ok = _Raw(records, _lib.MERGE_CONCAT)
    assert ok.rc_emit == 0 and ok.flags == 0 and ok.totals[4:] == [0, 0]
    assert ok.bytes("keys") == b"".join(k for k, _ in records)


@pytest.mark.parametrize("name", ["keys", "key_end", "vals", "val_end", "grp_end"])
def test_capacity_one_byte_short(name):
    """the overflow flag is set, nothing is written from the (short) capacity on, the guards stay"""
    torch, _lib, encode, merger, sorter = _mods()
    records = [(b"k%03d" % (i % 37) + b"x" * (i % 5), bytes([i & 0xFF]) * [0, 1, 15, 16, 17, 300][i % 6])
               for i in range(1500)]
    full = _Raw(records, _lib.MERGE_GROUPS)
    assert full.rc_emit == 0 and full.flags == 0
    r = _Raw(records, _lib.MERGE_GROUPS, short={name: 1})
    assert r.rc_plan == 0 and r.rc_emit == 0
    assert r.flags == _lib.MERGE_OVERFLOW
    assert r.cap[name] == full.size[name] - 1
    assert r.untouched_from(name, r.cap[name])
    for other in r.size:   # every other output is complete and stays inside its size
        assert r.untouched_from(other, r.size[other])
        if other != name:
            assert r.bytes(other) == full.bytes(other)


# ---------------------------------------------------------------- the Sorter, single chunk
SIMPLE = [(b"hello", b"kiki"), (b"abstract", b"lol"), (b"allo", b"lol"), (b"abstract", b"lol")]


def test_sorter_simple(oracle):
    """src/sorter.rs:264-295 on the device, by the callable of that test and by the built-in modes"""
    torch, _lib, encode, merger, sorter = _mods()
    model, _ = sm.run(SIMPLE, mm.concat)
    assert model == [(b"abstract", b"lollol"), (b"allo", b"lol"), (b"hello", b"kiki")]
    calls = []

    def merge(key, vals):
        assert len(vals) != 1
        calls.append(key)
        return b"".join(vals)

    for m in (merge, "concat"):
        s = sorter.SorterBuilder(m).chunk_compression_type(__import__("mtblx").CompressionType.Snappy).build()
        for k, v in SIMPLE:
            s.insert(k, v)
        file = s.write_file(1024, 16).cpu().numpy().tobytes()
        assert file == oracle.write_file(model, 1024, 16)
        assert s.chunk_sizes == [4] and s.merges == 0
    assert calls == [b"abstract"]
    for mode in ("first", "last"):
        s = sorter.Sorter(mode)
        for i, (k, v) in enumerate(SIMPLE):
            s.insert(k, v + b"%d" % i)
        assert dict(s.into_iter())[b"abstract"] == (b"lol1" if mode == "first" else b"lol3")
    s = sorter.Sorter("concat")
    s.insert_batch(*_host_batch(SIMPLE))
    w = __import__("mtblx").WriterBuilder().block_size(1024).memory()
    s.write_into(w)
    assert w.into_inner() == oracle.write_file(model, 1024, 16)


def _host_batch(records):
    ks, vs = b"".join(k for k, _ in records), b"".join(v for _, v in records)
    return (np.frombuffer(ks, np.uint8), np.cumsum([len(k) for k, _ in records]).astype(np.uint64),
            np.frombuffer(vs, np.uint8), np.cumsum([len(v) for _, v in records]).astype(np.uint64))


@pytest.mark.parametrize("records, want", [
    ([(b"", b"a"), (b"", b"b"), (b"x", b"c")], [(b"x", b"c")]),
    ([(b"", b"a"), (b"", b"b")], [(b"", b"ab")]),
    ([], []),
])
def test_sorter_empty_keys(records, want):
    """write_chunk keeps the empty-key group; the Merger of into_iter applies its quirk (as the model)"""
    torch, _lib, encode, merger, sorter = _mods()
    assert sm.run(records, sm.concat_any)[0] == want
    assert [(k, b"".join(vs)) for k, vs in promised(records, quirk=True)] == want
    s = sorter.Sorter("concat")
    for k, v in records:
        s.insert(k, v)
    assert list(s.into_iter()) == want


def test_sorter_callable_never_sees_one_value():
    torch, _lib, encode, merger, sorter = _mods()
    records = _dup_records(2000, 8)
    seen = []

    def merge(key, vals):
        seen.append(len(vals))
        return b"|".join(vals)

    s = sorter.Sorter(merge)
    for k, v in records:
        s.insert(k, v)
    got = list(s.into_iter())
    want = promised(records)
    assert got == [(k, vs[0] if len(vs) == 1 else b"|".join(vs)) for k, vs in want]
    assert seen and min(seen) >= 2 and len(seen) == sum(len(vs) > 1 for _, vs in want)
    assert any(len(vs) == 1 for _, vs in want)


# ---------------------------------------------------------------- the Sorter, several chunks
N_BIG = 3 * 6144 + 100


@pytest.fixture(scope="module")
def big():
    """3 * 6144 + 100 records of 8 B key + 1016 B value (1024-byte entries: a cut at every 6144th
    insert with max_memory at its minimum); the last third repeats keys of the first two chunks, so a
    third of the keys occur in two different chunks.  Shared, never changed."""
    rng = np.random.default_rng(17)
    m = N_BIG - N_BIG // 3
    keys = np.concatenate([rng.permutation(m), rng.permutation(m)[: N_BIG - m]])
    records = [(b"%08d" % k, (b"%07d:" % i) * 127) for i, k in enumerate(keys)]
    assert all(len(v) == 1016 for _, v in records[:3])
    chunk_of = {}
    for i, k in enumerate(keys):
        chunk_of.setdefault(int(k), set()).add(i // 6144)
    assert sum(len(c) > 1 for c in chunk_of.values()) >= m // 3
    want = [(k, b"".join(vs)) for k, vs in promised(records)]
    model = {}
    for nb in (25, 1):
        out, s = sm.run(records, sm.concat_any, max_memory=0, max_nb_chunks=nb)
        model[nb] = (out, s.chunk_sizes, s.merges)
    return records, want, model


def _pieces(v):
    return sorted(v[i: i + 1016] for i in range(0, len(v), 1016))


@pytest.mark.parametrize("nb, how", [(25, "insert"), (1, "insert"), (1, "insert_batch")])
def test_sorter_several_chunks(big, nb, how):
    torch, _lib, encode, merger, sorter = _mods()
    records, want, model = big
    out, chunk_sizes, merges = model[nb]
    assert chunk_sizes == [6144, 6144, 6144, 100] and merges == (2 if nb == 1 else 0)
    b = sorter.Sorter.builder("concat").max_memory(0)
    if nb != 25:
        b.max_nb_chunks(nb)
    s = b.build()
    if how == "insert":
        for k, v in records:
            s.insert(k, v)
    else:
        ks, ke, vs, ve = _host_batch(records)
        half = 9000
        s.insert_batch(ks[: int(ke[half - 1])], ke[:half], vs[: int(ve[half - 1])], ve[:half])
        dev = [torch.from_numpy(np.array(x)).cuda() for x in
               (ks[int(ke[half - 1]):], (ke[half:] - ke[half - 1]).astype(np.int64),
                vs[int(ve[half - 1]):], (ve[half:] - ve[half - 1]).astype(np.int64))]
        s.insert_batch(*dev)
    got = list(s.into_iter())
    assert s.chunk_sizes == chunk_sizes and s.merges == merges
    assert got == want                                               # insertion order inside every key
    assert [k for k, _ in got] == [k for k, _ in out]                # the model: keys and multisets
    assert [_pieces(v) for _, v in got] == [_pieces(v) for _, v in out]


def test_sorter_16_byte_entries_batch(oracle):
    """262 145+ records of 8 B + 8 B through insert_batch on device tensors: the capacity doubles at
    insert 131 073, which cuts; the next cut comes 131 072 later"""
    torch, _lib, encode, merger, sorter = _mods()
    n = 131_073 + 131_072 + 50
    rng = np.random.default_rng(23)
    ids = rng.permutation(n).astype(np.uint64)
    ids[n // 2:] = ids[: n - n // 2]                                  # every id of the first half twice
    kb = ids.byteswap().view(np.uint8)                                # 8-byte big-endian keys
    vb = np.arange(n, dtype=np.uint64).view(np.uint8)                 # the value: the input position
    ends = np.arange(1, n + 1, dtype=np.int64) * 8
    s = sorter.Sorter.builder("last").max_memory(0).build()
    s.insert_batch(*(torch.from_numpy(x).cuda() for x in (kb, ends, vb, ends)))
    assert s.chunk_sizes == [131_073, 131_072]
    r = s.records()
    assert s.chunk_sizes == [131_073, 131_072, 50] and s.merges == 0
    uniq = np.unique(ids)
    assert r.n == uniq.size
    keys = r.keys.cpu().numpy().view(">u8").astype(np.uint64)
    assert (keys == uniq).all()
    last = np.zeros(n, np.int64)
    last[ids.astype(np.int64)] = np.arange(n)                         # the last position of every id
    assert (r.vals.cpu().numpy().view(np.uint64).astype(np.int64) == last[uniq.astype(np.int64)]).all()

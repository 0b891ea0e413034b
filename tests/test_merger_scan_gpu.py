"""Merger.scan_batch / scan_batch_groups / get_batch and the segmented merge under them
(mtblx_merge_seg_plan / _emit, csrc/merge_seg.hip) on the device.

Expected values: per query, the record lists oracle.file_scan yields per source, fed into
tests/merger_model.py (tests/merger_scan_util.py).  Both yardsticks of tests/test_merger_gpu.py
apply per query: the reference's (key sequence and multiset of values per key, mm.canon) and this
library's promise (exact lists, values in source order: U.promised_groups)."""
import ctypes as C
import functools

import numpy as np
import pytest

import merger_model as mm
import merger_scan_util as U
import scan_util

pytestmark = pytest.mark.gpu

KTILE = 1024   # csrc/merge_dev.h kTile: handles per workgroup of the merge pass and the grouping scan


def _mods():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mtblx import _lib, encode, merger, reader
    return torch, _lib, encode, merger, reader


def _readers(datas):
    reader = _mods()[4]
    return [reader.Reader(d) for d in datas]


def _merger(datas, merge):
    merger = _mods()[3]
    return merger.Merger.builder(merge).extend(_readers(datas)).build()


_small = U.small_sources


def _expect(oracle, datas, qs, tag):
    """-> per query (promised groups, model groups), unlimited"""
    out = []
    for q in qs:
        lists = U.per_source(oracle, datas, q, tag)
        out.append((U.promised_groups(lists), U.model_groups(lists)))
    return out


def _check_groups(res, exp, limits=None):
    for q, (want, model) in enumerate(exp):
        m = None if limits is None else limits[q]
        got = res.groups(q)
        assert got == U.cut(want, m), q                                     # this library's promise
        assert mm.canon(got) == mm.canon(U.cut(model, m)), q                # the reference
        assert int(res.count[q]) == len(got)


def _check_records(res, exp, pick, limits=None):
    for q, (want, _) in enumerate(exp):
        m = None if limits is None else limits[q]
        assert res.records(q) == U.merged(U.cut(want, m), pick), q


@pytest.mark.parametrize("bs", [256, 1024])
def test_model_small(oracle, bs):
    """every query kind over 3 overlapping sources: the groups, the three built-in modes, a callable"""
    datas, lists, qs = _small(bs, False)
    assert sum(len({k for k, _ in r}) for r in lists) > len({k for r in lists for k, _ in r}) + 300   # shared keys
    exp = _expect(oracle, datas, qs, ("small", bs))
    assert any(len(vs) == 3 for want, _ in exp for _, vs in want)
    res = _merger(datas, "concat").scan_batch_groups(qs)
    _check_groups(res, exp)
    assert any(res.served_by_kernel(q) for q in range(len(qs)))
    for mode in ("concat", "first", "last"):
        _check_records(_merger(datas, mode).scan_batch(qs), exp, U.PICK[mode])
    calls = []

    def cat(key, values):
        calls.append(len(values))
        return b"".join(values)

    _check_records(_merger(datas, cat).scan_batch(qs), exp, U.PICK["concat"])
    assert calls and min(calls) >= 2


def test_model_small_reduce(oracle):
    from mtblx import Reduce
    datas, lists, qs = _small(1024, True)
    exp = _expect(oracle, datas, qs, ("small-u64", 1024))
    _check_records(_merger(datas, Reduce("sum")).scan_batch(qs), exp, U.sum_u64)


@pytest.mark.parametrize("limit", [0, 1, 37, "list"])
def test_limits(oracle, limit):
    """the first m items of the UNLIMITED merged result (every source is asked for m + 1 records)"""
    datas, lists, qs = _small(1024, False)
    qs = [q for q in qs if q[0] == "from"]
    exp = _expect(oracle, datas, qs, ("small", 1024))
    limits = [[0, 1, 2, 37, None, 5][i % 6] for i in range(len(qs))] if limit == "list" else [limit] * len(qs)
    assert any(m is not None and len(want) > m for (want, _), m in zip(exp, limits)) or limit == 0
    res = _merger(datas, "concat").scan_batch_groups(qs, max_records=limits if limit == "list" else limit)
    _check_groups(res, exp, limits)
    _check_records(_merger(datas, "last").scan_batch(qs, max_records=limits if limit == "list" else limit), exp,
                   U.PICK["last"], limits)


# ---------------------------------------------------------------- tile edges
def _counter_sources():
    """key i lies in source i % 4, and in all four when i % 10 == 0"""
    return [[(b"k%06d" % i, b"%d:%05d" % (s, i)) for i in range(6000) if i % 4 == s or i % 10 == 0] for s in range(4)]


def _nrec(i):
    return 4 if i % 10 == 0 else 1


def _tile_queries():
    """one range of exactly 3 * KTILE merged records, 1 500 queries that match nothing, then queries
    of 1 - 2 records that add up to exactly KTILE more"""
    lo, hi, n = 1, 1, 0
    while n < 3 * KTILE:            # [k(lo), k(hi - 1)]
        n += _nrec(hi)
        hi += 1
    while n > 3 * KTILE:            # a key in all four sources overshot: give up records at the low end
        n -= _nrec(lo)
        lo += 1
    assert n == 3 * KTILE
    qs = [("range", b"k%06d" % lo, b"k%06d" % (hi - 1))]
    nothing = [("get", b"k9"), ("prefix", b"j"), ("range", b"k000003x", b"k000003y"), ("from", b"l")]
    qs += [nothing[i % 4] for i in range(1500)]
    i, n, want = 3001, 0, 2
    while n < KTILE:
        while i % 10 == 0 or (i + 1) % 10 == 0:
            i += 1
        if want == 2 and n + 2 <= KTILE:
            qs.append(("range", b"k%06d" % i, b"k%06d" % (i + 1)))
            n += 2
        else:
            qs.append(("get", b"k%06d" % i))
            n += 1
        want = 3 - want
        i += 2
    return qs


@functools.lru_cache(maxsize=None)
def _tile_case():
    lists = _counter_sources()
    return [mm.make_source(r, 1024, 16) for r in lists], _tile_queries()


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_tile_edges(oracle, order):
    """segments that end exactly on a tile boundary of the merged handle order, 1 500 empty segments
    between them, and (reversed) later segments whose keys lie below earlier ones'"""
    datas, qs = _tile_case()
    if order == "reversed":
        qs = qs[::-1]
    exp = _expect(oracle, datas, qs, "tile")
    # the construction, from the expected lists: merged records before each segment
    per_q = [sum(len(vs) for _, vs in want) for want, _ in exp]
    start = np.concatenate([[0], np.cumsum(per_q)])
    assert max(per_q) == 3 * KTILE and start[-1] == 4 * KTILE and per_q.count(0) == 1500
    edges = {int(start[q + 1]) for q in range(len(qs)) if per_q[q]} & {int(start[q]) for q in range(len(qs)) if per_q[q]}
    assert (3 * KTILE if order == "forward" else KTILE) in edges      # one segment ends on 1024 j - 1, the next starts on 1024 j
    if order == "reversed":
        assert qs[0][1] > qs[-1][1]                                   # a later segment's keys lie below an earlier one's
    m = _merger(datas, "concat")
    res = m.scan_batch_groups(qs)
    assert all(res.served_by_kernel(q) for q in range(len(qs))) and res.n_large == 0 and res.n_fallback == 0
    _check_groups(res, exp)
    assert res.grp_off.cpu().tolist() == np.concatenate([[0], np.cumsum([len(w) for w, _ in exp])]).tolist()
    _check_records(m.scan_batch(qs), exp, U.PICK["concat"])


# ---------------------------------------------------------------- the quirk per query
def test_quirk_per_query(oracle):
    datas = [mm.make_source(r) for r in U.QUIRK_SOURCES]
    qs = [q for q, _ in U.QUIRK_QUERIES]
    limits = [m for _, m in U.QUIRK_QUERIES]
    exp = _expect(oracle, datas, qs, "quirk")
    res = _merger(datas, "concat").scan_batch_groups(qs, max_records=limits)
    for q, (want, model) in enumerate(exp):
        got = res.groups(q)
        assert got == U.cut(want, limits[q]), qs[q]
        if want and want[0][0] == b"":   # only empty keys match: which value is the heap's choice in the reference
            assert [(k, len(vs)) for k, vs in got] == [(k, len(vs)) for k, vs in U.cut(model, limits[q])]
        else:
            assert mm.canon(got) == mm.canon(U.cut(model, limits[q]))
    everything = [(b"k1", [b"x", b"y"]), (b"k2", [b"z"])]
    assert [res.groups(q) for q in range(7)] == [[(b"", [b"c"])], [(b"", [b"c"])], everything, everything, [],
                                                 everything[:1], everything]
    cat = _merger(datas, "concat").scan_batch(qs, max_records=limits)
    assert cat.records(0) == [(b"", b"c")] and cat.records(2) == [(b"k1", b"xy"), (b"k2", b"z")]


def test_prefix_empty_equals_the_full_merge(oracle):
    """("prefix", b"") with every block allowed is Merger.into_iter() / into_merge_iter(), item for item"""
    for bs in (256, 1024):
        datas, lists, _ = _small(bs, False)
        m = _merger(datas, "concat")
        res = m.scan_batch_groups([("prefix", b"")], max_blocks=1 << 20)
        assert res.served_by_kernel(0)
        assert res.groups(0) == list(m.into_iter())
        assert m.scan_batch([("prefix", b"")], max_blocks=1 << 20).records(0) == list(m.into_merge_iter())
    # quirk included: the sources whose first key is empty
    datas = [mm.make_source(r) for r in U.QUIRK_SOURCES]
    m = _merger(datas, "concat")
    assert m.scan_batch_groups([("prefix", b"")]).groups(0) == list(m.into_iter()) == [(b"k1", [b"x", b"y"]), (b"k2", [b"z"])]
    m = _merger(datas[1:2], "concat")
    assert m.scan_batch_groups([("prefix", b"")]).groups(0) == list(m.into_iter()) == [(b"", [b"b"])]


def test_mixed_paths(oracle, monkeypatch):
    """an uncompressed, a Snappy and a zlib source; with max_blocks=1 some queries are handed back by
    some sources only: same results, served_by_kernel False exactly for those, one segmented merge"""
    torch, _lib, encode, merger, reader = _mods()
    _, lists, qs = _small(1024, False)
    datas = [scan_util.write(r, 1024, 4, comp) for r, comp in zip(lists, (0, 1, 2))]
    readers = _readers(datas)
    m = merger.Merger.builder("concat").extend(readers).build()
    wide = m.scan_batch_groups(qs, max_blocks=64)
    calls = []
    real = merger._merge_segments_64
    monkeypatch.setattr(merger, "_merge_segments_64", lambda *a: (calls.append(len(a[0])), real(*a))[1])
    narrow = m.scan_batch_groups(qs, max_blocks=1)
    assert calls == [3]
    handed = [any(not r.scan_batch([q], max_blocks=1).served_by_kernel(0) for r in readers) for q in qs]
    some = [sum(not r.scan_batch([q], max_blocks=1).served_by_kernel(0) for r in readers) for q in qs]
    assert any(handed) and not all(handed) and any(0 < n < 3 for n in some)
    assert [narrow.served_by_kernel(q) for q in range(len(qs))] == [not h for h in handed]
    assert narrow.n_large + narrow.n_fallback == sum(some)
    exp = _expect(oracle, datas, qs, "mixed")
    _check_groups(narrow, exp)
    _check_groups(wide, exp)
    assert [narrow.groups(q) for q in range(len(qs))] == [wide.groups(q) for q in range(len(qs))]


# ---------------------------------------------------------------- sizes
def test_sizes(oracle):
    torch, _lib, encode, merger, reader = _mods()
    datas, lists, qs = _small(1024, False)
    m = _merger(datas, "concat")
    res = m.scan_batch([])                                       # nq == 0
    assert res.nq == 0 and res.grp_off.tolist() == [0] and res.count.numel() == 0 and res.keys.numel() == 0
    none = merger.Merger([], "concat")                          # no sources
    res = none.scan_batch(qs[:5])
    assert res.grp_off.tolist() == [0] * 6 and [res.records(q) for q in range(5)] == [[]] * 5
    assert none.scan_batch_groups(qs[:5]).groups(4) == []
    # one source: its own scan_batch, the quirk applied (an empty-key record vanishes when another follows)
    one = [(b"", b"e"), (b"a", b"1"), (b"ab", b"2"), (b"b", b"3")]
    data = mm.make_source(one)
    q1 = [("prefix", b""), ("get", b""), ("prefix", b"a"), ("range", b"", b"a"), ("from", b"b"), ("get", b"zz")]
    sb = reader.Reader(data).scan_batch(q1)
    own = [sb.records(q) for q in range(len(q1))]
    assert own[0] == one and own[1] == one[:1]
    quirk = [r[1:] if len(r) > 1 and r[0][0] == b"" else r for r in own]
    res = _merger([data], "first").scan_batch(q1)
    assert [res.records(q) for q in range(len(q1))] == quirk
    assert quirk[0] == one[1:] and quirk[1] == one[:1] and quirk[3] == [(b"a", b"1")]
    # the same query 65 times
    q = qs[1]
    exp = _expect(oracle, datas, [q], ("small", 1024)) * 65
    _check_groups(m.scan_batch_groups([q] * 65), exp)


def test_65_sources_in_rounds(oracle):
    """rounds of 64 with the same mode; "groups" through the two-CONCAT regrouping, segmented"""
    from mtblx import Reduce
    rng = np.random.default_rng(65)
    lists = []
    for s in range(65):
        ks = np.unique(rng.integers(0, 60, size=12))
        lists.append([(b"%03d" % k, (s * 100 + int(k)).to_bytes(8, "little")) for k in ks])
    lists[64] = [(b"", b"dropped!")] + lists[64]
    datas = [mm.make_source(r) for r in lists]
    qs = [("prefix", b"00"), ("get", b"017"), ("range", b"010", b"030"), ("from", b"05"), ("prefix", b""), ("get", b""),
          ("prefix", b"9")]
    limits = [None, None, None, 3, None, None, None]
    exp = _expect(oracle, datas, qs, "r65")
    assert any(len(vs) > 1 and 64 in [int.from_bytes(v, "little") // 100 for v in vs] for w, _ in exp for _, vs in w)
    assert exp[5][0] == [(b"", [b"dropped!"])]
    _check_groups(_merger(datas, "concat").scan_batch_groups(qs, max_records=limits), exp, limits)
    for mode in ("concat", "first", "last"):
        _check_records(_merger(datas, mode).scan_batch(qs, max_records=limits), exp, U.PICK[mode], limits)
    _check_records(_merger(datas, Reduce("sum")).scan_batch(qs, max_records=limits), exp, U.sum_u64, limits)


# ---------------------------------------------------------------- reduce
def test_get_batch_reduce_sum(oracle):
    """the total count of 1 000 keys across 8 shards; a key found in one shard passes through"""
    from mtblx import MergeError, Reduce
    rng = np.random.default_rng(8)
    lists = []
    for s in range(8):
        ks = np.unique(rng.integers(0, 3000, size=700 if s else 2600))
        lists.append([(b"key-%05d" % k, int(rng.integers(1, 1 << 50)).to_bytes(8, "little")) for k in ks])
    lists[3] = sorted(lists[3] + [(b"odd-alone", b"4444"), (b"odd-pair", b"4444")])
    lists[5] = sorted(lists[5] + [(b"odd-pair", (7).to_bytes(8, "little"))])
    datas = [mm.make_source(r, 4096) for r in lists]
    total = {}
    for r in lists:
        for k, v in r:
            total.setdefault(k, []).append(v)
    keys = [b"key-%05d" % k for k in rng.integers(0, 3300, size=999)] + [b"odd-alone"]
    m = _merger(datas, Reduce("sum"))
    res = m.get_batch(keys)
    n1 = 0
    for q, k in enumerate(keys):
        vs = total.get(k, [])
        n1 += len(vs) == 1
        want = [] if not vs else [(k, vs[0] if len(vs) == 1 else U.sum_u64(vs))]
        assert res.records(q) == want, k
    assert n1 > 50 and res.records(999) == [(b"odd-alone", b"4444")] and int(res.count.sum()) == sum(k in total for k in keys)
    assert all(res.served_by_kernel(q) for q in range(1000))
    with pytest.raises(MergeError):
        m.get_batch([b"key-00001", b"odd-pair"])
    assert _merger(datas, "concat").get_batch([b"odd-pair"]).records(0) == [(b"odd-pair", b"4444" + (7).to_bytes(8, "little"))]


# ---------------------------------------------------------------- the bare C ABI
class _RawSeg:
    """mtblx_merge_seg_plan + mtblx_merge_seg_emit with buffers the test owns: every output is a
    slice of a 0xA5-filled buffer, `short[name]` bytes smaller than the plan's size, followed by a
    64-byte guard.  `sources`: per source a list of segments (record lists)."""

    def __init__(self, sources, mode=1, short=None, offs=None, plan=True, emit_nseg=None, emit=True):
        torch, _lib, encode, merger, reader = _mods()
        L = __import__("mtblx").lib()
        short = short or {}
        nseg = len(sources[0])
        self.src = [encode.DeviceRecords.from_list([r for seg in s for r in seg]) for s in sources]
        if offs is None:
            offs = [np.concatenate([[0], np.cumsum([len(seg) for seg in s])]) for s in sources]
        self.offs = [torch.tensor(np.asarray(o, dtype=np.int64), device="cuda") for o in offs]
        arr = (_lib.Records * len(self.src))()
        op = (C.c_void_p * len(self.src))()
        for i, r in enumerate(self.src):
            arr[i] = r.cstruct()
            op[i] = self.offs[i].data_ptr()
        n = sum(r.n for r in self.src)
        wsb = int(L.mtblx_merge_seg_workspace_bytes(n, len(self.src), max(nseg, emit_nseg or 0)))
        ws = torch.zeros(wsb + 256, dtype=torch.uint8, device="cuda")
        wp = (ws.data_ptr() + 255) & ~255
        tot = (C.c_uint64 * 6)()
        self.seg_end = torch.full((nseg + 8,), -1, dtype=torch.int64, device="cuda")
        self.rc_plan, self.totals = None, [8, 64, 8, 64, 0, 0]
        if plan:
            self.rc_plan = L.mtblx_merge_seg_plan(arr, op, len(self.src), nseg, tot, C.c_void_p(self.seg_end.data_ptr()),
                                                  C.c_void_p(wp), wsb, None)
            self.totals = [int(x) for x in tot]
            if self.rc_plan != 0:
                self.totals[:4] = [8, 64, 8, 64]
        if not emit:
            return
        groups, kb, nv, vb = self.totals[:4]
        size = {"keys": kb, "key_end": 8 * groups, "vals": vb, "val_end": 8 * (nv if mode == 0 else groups),
                "grp_end": 8 * groups if mode == 0 else 0}
        self.size, self.cap, self.buf, ptr = size, {}, {}, {}
        for name, sz in size.items():
            self.cap[name] = max(sz - short.get(name, 0), 0)
            self.buf[name] = torch.full((16 + sz + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            ptr[name] = (self.buf[name].data_ptr() + 15) & ~15
            self.buf[name] = (self.buf[name], ptr[name] - self.buf[name].data_ptr())
        flags = torch.full((1,), 0x5A5A, dtype=torch.int32, device="cuda")
        out = _lib.Merged(ptr["keys"], self.cap["keys"], ptr["key_end"], self.cap["key_end"], ptr["vals"],
                          self.cap["vals"], ptr["val_end"], self.cap["val_end"], ptr["grp_end"], self.cap["grp_end"],
                          flags.data_ptr())
        self.rc_emit = L.mtblx_merge_seg_emit(arr, op, len(self.src), nseg if emit_nseg is None else emit_nseg, mode,
                                              C.byref(out), C.c_void_p(wp), wsb, None)
        torch.cuda.synchronize()
        self.flags = int(flags.item())

    def untouched_from(self, name, start):
        t, off = self.buf[name]
        return bool((t[off + start:] == 0xA5).all()) and bool((t[:off] == 0xA5).all())

    def bytes(self, name, n=None):
        t, off = self.buf[name]
        return t[off: off + (self.size[name] if n is None else n)].cpu().numpy().tobytes()

    def records(self):
        ke = np.frombuffer(self.bytes("key_end"), np.uint64).tolist()
        ve = np.frombuffer(self.bytes("val_end"), np.uint64).tolist()
        k, v = self.bytes("keys"), self.bytes("vals")
        return [(k[(ke[i - 1] if i else 0): ke[i]], v[(ve[i - 1] if i else 0): ve[i]]) for i in range(len(ke))]


RAW = [[[(b"b", b"0b"), (b"c", b"0c")], [], [(b"a", b"0a")]],
       [[(b"c", b"1c")], [(b"", b"1e")], [(b"a", b"1a"), (b"b", b"1b")]]]


def test_raw_abi():
    """the plain case, then every refusal: each is an error return or a flag, never a write outside
    the capacities"""
    torch, _lib, encode, merger, reader = _mods()
    r = _RawSeg(RAW)
    assert (r.rc_plan, r.rc_emit, r.flags) == (0, 0, 0)
    assert r.records() == [(b"b", b"0b"), (b"c", b"0c1c"), (b"", b"1e"), (b"a", b"0a1a"), (b"b", b"1b")]
    assert r.seg_end.tolist() == [2, 3, 5] + [-1] * 8 and r.totals == [5, 4, 7, 14, 0, 0]
    assert all(r.untouched_from(n, r.size[n]) for n in r.size)
    # a capacity too small: MTBLX_MERGE_OVERFLOW, nothing past it
    for name, cut in (("keys", 1), ("key_end", 8), ("vals", 2), ("val_end", 8)):
        r = _RawSeg(RAW, short={name: cut})
        assert r.rc_emit == 0 and r.flags == _lib.MERGE_OVERFLOW, name
        assert r.untouched_from(name, r.cap[name]), name
    # an unplanned (zeroed) workspace, and one planned for another segment count: NOT_PLANNED, nothing written
    for kw in ({"plan": False}, {"emit_nseg": 4}):
        r = _RawSeg(RAW, **kw)
        assert r.rc_emit == 0 and r.flags == _lib.MERGE_NOT_PLANNED, kw
        assert all(r.untouched_from(n, 0) for n in r.size)
    # out of order inside a segment: refused; the same two keys in different segments: fine
    r = _RawSeg([[[(b"b", b""), (b"a", b"")]]], emit=False)
    assert r.rc_plan == _lib.MTBLX_E_FORMAT and r.totals[5] == _lib.MERGE_UNSORTED
    r = _RawSeg([[[(b"a", b""), (b"a", b"")]]], emit=False)                  # equal keys are out of order too
    assert r.rc_plan == _lib.MTBLX_E_FORMAT and r.totals[5] == _lib.MERGE_UNSORTED
    r = _RawSeg([[[(b"b", b"1")], [(b"a", b"2")]]])
    assert (r.rc_plan, r.flags) == (0, 0) and r.records() == [(b"b", b"1"), (b"a", b"2")]
    # seg_off decreasing, not starting at 0, or not ending at n: BADSEG, before anything is indexed with it
    good = [[0, 2, 2, 3], [0, 1, 2, 4]]
    assert _RawSeg(RAW, offs=good, emit=False).rc_plan == 0
    for offs in ([[0, 2, 1, 3], good[1]], [good[0], [1, 1, 2, 4]], [good[0], [0, 1, 2, 3]], [[0, 2, 2, 4], good[1]],
                 [good[0], [0, 1, 2, 1 << 40]], [[0, 3, 2, 3], good[1]]):
        r = _RawSeg(RAW, offs=offs, emit=False)
        assert r.rc_plan == _lib.MTBLX_E_FORMAT and r.totals[5] == _lib.MERGE_BADSEG, offs
        assert r.seg_end.tolist() == [-1] * 11


def test_write_file(oracle):
    """device_records(q) feeds the device Writer as it stands"""
    torch, _lib, encode, merger, reader = _mods()
    datas, lists, qs = _small(1024, False)
    q = max((q for q in qs if q[0] == "prefix" and q[1]), key=lambda q: len(U.promised_groups(U.per_source(oracle, datas, q))))
    want = U.merged(U.promised_groups(U.per_source(oracle, datas, q)), U.PICK["concat"])
    assert len(want) >= 2
    res = _merger(datas, "concat").scan_batch([("get", b"nothing"), q, ("from", b"")], max_records=[None, None, 3])
    file = encode.write_file(res.device_records(1), 1024, 16).cpu().numpy().tobytes()
    assert file == oracle.write_file(want, 1024, 16)
    assert encode.write_file(res.device_records(2), 1024, 16).cpu().numpy().tobytes() == oracle.write_file(
        res.records(2), 1024, 16) and len(res.records(2)) == 3

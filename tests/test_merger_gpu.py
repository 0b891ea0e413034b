"""The device Merger (mtblx/merger.py over mtblx_merge_plan / mtblx_merge_emit, csrc/merge.hip)
against tests/merger_model.py (src/merger.rs restated) and against this library's own promise.

Two yardsticks, kept apart:
  * the reference fixes the key sequence and the MULTISET of values per key (its BinaryHeap
    leaves the order of equal keys unspecified): `mm.canon` of the device result == `mm.canon` of
    the model's;
  * this library promises the values of a key in source order: the exact lists equal `promised()`,
    worked out here from the sources with a stable sort, the empty-key quirk applied by its rule.
Sources are .mtbl files made by pyoracle.write_file; the model reads them through pyoracle.file_scan,
the device through mtblx.reader.Reader."""
import ctypes as C

import numpy as np
import pytest

import merger_model as mm

pytestmark = pytest.mark.gpu


def _mods():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mtblx import _lib, encode, merger, reader
    return torch, _lib, encode, merger, reader


def promised(sources):
    """[(key, [values in source order])]: a stable sort by key, then the quirk of
    src/merger.rs:182-186: the empty-key records vanish when any other record exists; when none
    does, one group holding the highest-numbered source's value remains"""
    flat = sorted(((k, s, v) for s, recs in enumerate(sources) for k, v in recs), key=lambda t: (t[0], t[1]))
    out = []
    for k, _, v in flat:
        if out and out[-1][0] == k:
            out[-1][1].append(v)
        else:
            out.append((k, [v]))
    if out and out[0][0] == b"":
        out = out[1:] if len(out) > 1 else [(b"", out[0][1][-1:])]
    return out


def _files(sources, block_size=1024):
    return [mm.make_source(s, block_size) for s in sources]


def _check(sources, model=True, block_size=1024):
    """every mode and both iterators over `sources` (lists of sorted records)"""
    torch, _lib, encode, merger, reader = _mods()
    files = _files(sources, block_size)
    recs = [mm.source_records(f) for f in files]
    assert recs == [list(s) for s in sources]
    readers = [reader.Reader(f) for f in files]
    want = promised(recs)
    got = list(merger.Merger.builder("concat").extend(readers).build().into_iter())
    if model:
        exp = mm.multi_iter(recs)
        assert [k for k, _ in got] == [k for k, _ in exp]
        assert mm.canon(got) == mm.canon(exp)
    assert got == want                                   # source order inside every group
    for mode, pick in (("concat", b"".join), ("first", lambda vs: vs[0]), ("last", lambda vs: vs[-1])):
        m = merger.Merger.builder(mode).extend(readers).build()
        assert list(m.into_merge_iter()) == [(k, pick(vs)) for k, vs in want], mode
    return readers, recs, want


def test_easy_scenario(oracle):
    """src/merger.rs:267-304 on the device: all four modes, both iterators, and the written file"""
    torch, _lib, encode, merger, reader = _mods()
    readers, recs, want = _check(mm.easy_sources())
    keys = [k for k, _ in want]
    assert keys == [b"%010d" % j for j in range(300)] and all(a < b for a, b in zip(keys, keys[1:]))
    model = mm.merge_iter(recs, mm.concat)
    m = merger.Merger.builder("concat").extend(readers).build()
    file = m.write_file(1024, 16).cpu().numpy().tobytes()
    assert file == oracle.write_file(model, 1024, 16)
    assert oracle.file_scan(file)["records"] == model
    w = __import__("mtblx").WriterBuilder().block_size(1024).memory()
    m.write_into(w)
    assert w.into_inner() == file


def _random_sources(nsrc, total, seed, common=b""):
    rng = np.random.default_rng(seed)

    def word(alpha, lo, hi):
        return bytes(rng.choice(alpha, size=int(rng.integers(lo, hi + 1))).tolist())

    pool = set()
    for _ in range(1500):
        pool.add(common + word([0x61, 0x62, 0x00], 0, 6))                           # "ab" < "ab\0", duplicates
        pool.add(common + word([0x7F, 0x80, 0xFF], 1, 5))                           # a signed compare would misorder
        pool.add(common + b"shared-run-" + word([0x61, 0x62, 0x00], 0, 29 - len(common)))   # > 8 equal leading bytes
    pool = sorted(k for k in pool if len(k) <= 40)
    sources = []
    for s in range(nsrc):
        n = 0 if (nsrc >= 3 and s == 1) else 1 if (nsrc >= 3 and s == 2) else max(1, total // max(nsrc - 2 if nsrc >= 3 else nsrc, 1))
        n = min(n, len(pool))
        idx = np.sort(rng.choice(len(pool), size=n, replace=False))
        sources.append([(pool[i], bytes([s]) * int(rng.integers(0, 301))) for i in idx])
    return sources


@pytest.mark.parametrize("nsrc", [0, 1, 2, 3, 5, 7, 16, 64])
def test_random_sources(oracle, nsrc):
    _check(_random_sources(nsrc, 3000, 100 + nsrc))


def test_all_keys_share_a_prefix(oracle):
    """every key starts with the same 12 bytes: the handle's prefix is taken after them"""
    src = _random_sources(5, 2500, 7, common=b"common-12-by")
    assert all(k.startswith(b"common-12-by") for s in src for k, _ in s)
    _check(src)


def test_many_slices_unpaired_runs(oracle):
    """~200 000 records in 7 sources: every pass spans ~200 workgroup slices and carries an unpaired run"""
    torch, _lib, encode, merger, reader = _mods()
    rng = np.random.default_rng(11)
    sources = []
    for s in range(7):
        ks = np.unique(rng.integers(0, 400_000, size=31_000 - 1000 * s))
        sources.append([(b"%08d" % k, bytes([s]) * (int(k) % 5)) for k in ks])
    files = _files(sources, 8192)
    recs = [mm.source_records(f) for f in files]
    assert sum(len(r) for r in recs) > 180_000
    readers = [reader.Reader(f) for f in files]
    want = promised(recs)
    got = merger.Merger.builder("concat").extend(readers).build().groups().to_list()
    assert got == want
    assert mm.canon(got) == mm.canon(mm.multi_iter(recs))
    m = merger.Merger.builder("last").extend(readers).build()
    assert list(m.into_merge_iter()) == [(k, vs[-1]) for k, vs in want]


def test_stability_groups_of_64(oracle):
    """3 000 consecutive keys present in all 64 sources: groups of 64 straddle every slice boundary;
    the grouped values must be the source numbers 0 .. 63 in order"""
    torch, _lib, encode, merger, reader = _mods()
    sources = [[(b"key-%06d" % j, bytes([s])) for j in range(3000)] for s in range(64)]
    readers = [reader.Reader(f) for f in _files(sources, 8192)]
    got = merger.Merger.builder("concat").extend(readers).build().groups().to_list()
    assert len(got) == 3000
    order = [bytes([s]) for s in range(64)]
    assert all(k == b"key-%06d" % j and vs == order for j, (k, vs) in enumerate(got))
    cat = list(merger.Merger.builder("concat").extend(readers).build().into_merge_iter())
    assert cat == [(b"key-%06d" % j, bytes(range(64))) for j in range(3000)]


@pytest.mark.parametrize("layout", ["identical", "interleaved", "stacked"])
def test_simple_layouts(oracle, layout):
    n, ns = 400, 5
    if layout == "identical":
        src = [[(b"k%05d" % j, b"v%d" % s) for j in range(n)] for s in range(ns)]
    elif layout == "interleaved":
        src = [[(b"k%05d" % (j * ns + s), b"v%d" % s) for j in range(n)] for s in range(ns)]
    else:
        src = [[(b"k%05d" % (s * n + j), b"v%d" % s) for j in range(n)] for s in range(ns)]
    _check(src)


@pytest.mark.parametrize("case", ["E1_followers", "E1_alone", "E2_followers", "E2_alone"])
def test_empty_key_quirk(oracle, case):
    """src/merger.rs:182-186.  E2_alone: the reference keeps whichever value its BinaryHeap pops
    last, which std does not specify; this library documents the highest-numbered source's
    (include/mtblx.h), so that single case is checked against the documented choice, not the model"""
    src = {
        "E1_followers": [[(b"", b"x0"), (b"a", b"1")], [(b"a", b"2"), (b"b", b"3")]],
        "E1_alone": [[(b"", b"x0")], []],
        "E2_followers": [[(b"", b"x0"), (b"b", b"1")], [(b"", b"x1")], [(b"a", b"2")]],
        "E2_alone": [[(b"", b"x0")], [(b"", b"x1")]],
    }[case]
    _, _, want = _check(src, model=case != "E2_alone")
    assert want == {
        "E1_followers": [(b"a", [b"1", b"2"]), (b"b", [b"3"])],
        "E1_alone": [(b"", [b"x0"])],
        "E2_followers": [(b"a", [b"2"]), (b"b", [b"1"])],
        "E2_alone": [(b"", [b"x1"])],
    }[case]


def test_callable_merge_function(oracle):
    """sum of little-endian u64s, applied on the host; never called for a group of one"""
    torch, _lib, encode, merger, reader = _mods()
    rng = np.random.default_rng(5)
    sources = []
    for s in range(6):
        ks = np.unique(rng.integers(0, 600, size=300))
        sources.append([(b"%05d" % k, int(rng.integers(0, 1 << 40)).to_bytes(8, "little")) for k in ks])
    calls = []

    def add(key, values):
        calls.append(len(values))
        return (sum(int.from_bytes(v, "little") for v in values) & ((1 << 64) - 1)).to_bytes(8, "little")

    files = _files(sources)
    recs = [mm.source_records(f) for f in files]
    m = merger.Merger.builder(add).extend([reader.Reader(f) for f in files]).build()
    got = list(m.into_merge_iter())
    assert calls and min(calls) >= 2
    ncalls = len(calls)
    assert got == mm.merge_iter(recs, add)
    assert any(len(vs) == 1 for _, vs in promised(recs)) and ncalls == sum(len(vs) > 1 for _, vs in promised(recs))
    assert oracle.file_scan(m.write_file(1024, 16).cpu().numpy().tobytes())["records"] == got


def test_more_than_64_sources(oracle):
    """130 sources through Python: rounds of 64 with the same mode"""
    rng = np.random.default_rng(9)
    sources = []
    for s in range(130):
        ks = np.unique(rng.integers(0, 200, size=20))
        sources.append([(b"%04d" % k, b"s%03d" % s) for k in ks])
    sources[70] = [(b"", b"dropped")] + sources[70]
    _check(sources)


# ---------------------------------------------------------------- the bare C ABI
class _Raw:
    """mtblx_merge_plan + mtblx_merge_emit with buffers the test owns: every output is a slice of
    a 0xA5-filled buffer starting `shift` bytes after a 16-byte boundary, `short[name]` bytes
    smaller than the plan's size, followed by a 64-byte guard"""

    def __init__(self, sources, mode, short=None, shift=0, emit_after_error=False):
        torch, _lib, encode, merger, reader = _mods()
        L = __import__("mtblx").lib()
        short = short or {}
        self.src = [encode.DeviceRecords.from_list(s) for s in sources]
        arr = (_lib.Records * max(len(self.src), 1))()
        for i, r in enumerate(self.src):
            arr[i] = r.cstruct()
        n = sum(r.n for r in self.src)
        wsb = int(L.mtblx_merge_workspace_bytes(n, len(self.src)))
        ws = torch.empty(wsb + 256, dtype=torch.uint8, device="cuda")
        wp = (ws.data_ptr() + 255) & ~255
        tot = (C.c_uint64 * 6)()
        self.rc_plan = L.mtblx_merge_plan(arr, len(self.src), tot, C.c_void_p(wp), wsb, None)
        self.totals = [int(x) for x in tot]
        if self.rc_plan != 0 and not emit_after_error:
            return
        groups, kb, nv, vb = self.totals[:4]
        if self.rc_plan != 0:
            groups, kb, nv, vb = 8, 64, 8, 64
        grouped = mode == _lib.MERGE_GROUPS
        size = {"keys": kb, "key_end": 8 * groups, "vals": vb, "val_end": 8 * (nv if grouped else groups),
                "grp_end": 8 * groups if grouped else 0}
        self.cap, self.buf, ptr = {}, {}, {}
        for name, sz in size.items():
            off = 16 + (shift if name in ("keys", "vals") else 0)
            self.cap[name] = max(sz - short.get(name, 0), 0)
            self.buf[name] = torch.full((off + sz + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            base = (self.buf[name].data_ptr() + 15) & ~15
            ptr[name] = base + (shift if name in ("keys", "vals") else 0)
            self.buf[name] = (self.buf[name], ptr[name] - self.buf[name].data_ptr())
        flags = torch.full((1,), 0x5A5A, dtype=torch.int32, device="cuda")
        out = _lib.Merged(ptr["keys"], self.cap["keys"], ptr["key_end"], self.cap["key_end"], ptr["vals"],
                          self.cap["vals"], ptr["val_end"], self.cap["val_end"], ptr["grp_end"], self.cap["grp_end"],
                          flags.data_ptr())
        self.rc_emit = L.mtblx_merge_emit(arr, len(self.src), mode, C.byref(out), C.c_void_p(wp), wsb, None)
        torch.cuda.synchronize()
        self.flags = int(flags.item())
        self.size = size

    def bytes(self, name, n=None):
        t, off = self.buf[name]
        n = self.size[name] if n is None else n
        return t[off: off + n].cpu().numpy().tobytes()

    def untouched_from(self, name, start):
        t, off = self.buf[name]
        return bool((t[off + start:] == 0xA5).all()) and bool((t[:off] == 0xA5).all())

    def ends(self, name):
        return np.frombuffer(self.bytes(name), np.uint64).tolist()

    def groups(self):
        ke, ve, ge = self.ends("key_end"), self.ends("val_end"), self.ends("grp_end")
        k, v = self.bytes("keys"), self.bytes("vals")
        out, pk, pv, pg = [], 0, 0, 0
        for g in range(len(ke)):
            vs = []
            for j in range(pg, ge[g]):
                vs.append(v[pv: ve[j]])
                pv = ve[j]
            out.append((k[pk: ke[g]], vs))
            pk, pg = ke[g], ge[g]
        return out

    def records(self):
        ke, ve = self.ends("key_end"), self.ends("val_end")
        k, v = self.bytes("keys"), self.bytes("vals", ve[-1] if ve else 0)
        return [(k[(ke[i - 1] if i else 0): ke[i]], v[(ve[i - 1] if i else 0): ve[i]]) for i in range(len(ke))]


def _alignment_sources():
    lens = [0, 1, 15, 16, 17, 4096]
    src = []
    for s in range(4):
        recs = []
        for j in range(24):
            if (j + s) % 3 == 0:
                continue
            n = lens[(j + s) % len(lens)]
            recs.append((b"k%03d" % j + b"x" * ((j * 7) % 23), bytes([(s * 40 + j + i) & 0xFF for i in range(n)])))
        for j in range(3):   # groups of one
            recs.append((b"u%d%03d" % (s, j), bytes([s + 1]) * lens[(2 * j + s) % len(lens)]))
        src.append(recs)
    return src


@pytest.mark.parametrize("shift", [0, 1])
def test_value_lengths_and_alignments(shift):
    """values of 0 / 1 / 15 / 16 / 17 / 4096 bytes at whatever alignment their predecessors leave,
    into key and value buffers `shift` bytes off a 16-byte boundary; nothing outside the outputs"""
    torch, _lib, encode, merger, reader = _mods()
    src = _alignment_sources()
    want = promised(src)
    r = _Raw(src, _lib.MERGE_GROUPS, shift=shift)
    assert r.rc_plan == 0 and r.rc_emit == 0 and r.flags == 0
    assert r.totals[:5] == [len(want), sum(len(k) for k, _ in want), sum(len(vs) for _, vs in want),
                            sum(len(v) for _, vs in want for v in vs), 0]
    assert r.groups() == want
    assert all(r.untouched_from(n, r.size[n]) for n in r.size)
    for mode, pick in ((_lib.MERGE_CONCAT, b"".join), (_lib.MERGE_FIRST, lambda vs: vs[0]),
                       (_lib.MERGE_LAST, lambda vs: vs[-1])):
        r = _Raw(src, mode, shift=shift)
        assert r.rc_emit == 0 and r.flags == 0
        exp = [(k, pick(vs)) for k, vs in want]
        assert r.records() == exp
        assert r.untouched_from("vals", sum(len(v) for _, v in exp)) and r.untouched_from("grp_end", 0)


def test_out_of_order_source():
    """a key <= its predecessor: MTBLX_E_FORMAT with MTBLX_MERGE_UNSORTED, and an emit over that
    workspace writes nothing"""
    torch, _lib, encode, merger, reader = _mods()
    good = [(b"a", b"1"), (b"c", b"2")]
    for bad in ([(b"b", b"1"), (b"a", b"2")], [(b"b", b"1"), (b"b", b"2")]):
        r = _Raw([good, bad, good], _lib.MERGE_CONCAT, emit_after_error=True)
        assert r.rc_plan == _lib.MTBLX_E_FORMAT and r.totals[5] & _lib.MERGE_UNSORTED
        assert r.rc_emit == 0 and r.flags == _lib.MERGE_NOT_PLANNED
        assert all(r.untouched_from(n, 0) for n in r.size)
        with pytest.raises(merger.UnsortedSource) as e:
            merger.merge_records([encode.DeviceRecords.from_list(s) for s in (good, bad)], "concat")
        assert e.value.flags & _lib.MERGE_UNSORTED


@pytest.mark.parametrize("name", ["keys", "vals", "val_end", "grp_end"])
def test_capacity_one_byte_short(name):
    """the overflow flag is set and nothing is written from the (short) capacity on"""
    torch, _lib, encode, merger, reader = _mods()
    src = _alignment_sources()
    full = _Raw(src, _lib.MERGE_GROUPS)
    r = _Raw(src, _lib.MERGE_GROUPS, short={name: 1})
    assert r.rc_plan == 0 and r.rc_emit == 0
    assert r.flags == _lib.MERGE_OVERFLOW
    assert r.cap[name] == full.size[name] - 1
    assert r.untouched_from(name, r.cap[name])
    for other in r.size:   # every other output is complete and stays inside its size
        assert r.untouched_from(other, r.size[other])
        if other != name:
            assert r.bytes(other) == full.bytes(other)

"""Device merge functions (mtblx.Reduce over mtblx_merge_emit_reduce / mtblx_sort_emit_reduce,
csrc/reduce_dev.h) against three things that do not run the code under test: the few-line reducer
defined here fed to tests/merger_model.py and tests/sorter_model.py (src/merger.rs, src/sorter.rs
restated), and the same reducer as a callable through this library's host path
(Merger.builder(fn), Sorter(fn)).  sum / min / max are commutative, so the model's heap order
cannot show: the bytes must be equal."""
import ctypes as C

import numpy as np
import pytest

import merger_model as mm
import sorter_model as sm

pytestmark = pytest.mark.gpu

M = (1 << 64) - 1
TILE, WAVE = 1024, 64   # records per workgroup of k_reduce_tile, lanes of a wave (4 records per lane)


def _mods():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mtblx
    from mtblx import _lib, encode, merger, reader, sorter
    return torch, mtblx, _lib, encode, merger, reader, sorter


class BadLength(Exception):
    pass


def reducer(*ops):
    """the reducer of these tests: never the library's own"""
    def fn(_key, values):
        if any(len(v) != 8 * len(ops) for v in values):
            raise BadLength()
        out = b""
        for f, op in enumerate(ops):
            xs = [int.from_bytes(v[8 * f: 8 * f + 8], "little") for v in values]
            x = sum(xs) % 2 ** 64 if op == "sum" else min(xs) if op == "min" else max(xs)
            out += x.to_bytes(8, "little")
        return out
    return fn


def u(*xs):
    return b"".join(int(x).to_bytes(8, "little") for x in xs)


def _tensors(r):
    return tuple(t.cpu().numpy().tobytes() for t in (r.keys[: int(r.key_end[-1]) if r.n else 0], r.key_end,
                                                     r.vals[: int(r.val_end[-1]) if r.n else 0], r.val_end))


def _check_sort(records, ops):
    """sort_records(Reduce) == the model == the callable path, bytes and offsets"""
    torch, mtblx, _lib, encode, merger, reader, sorter = _mods()
    fn = reducer(*ops)
    recs = encode.DeviceRecords.from_list(records)
    got = sorter.sort_records(recs, mtblx.Reduce(*ops))
    want, _ = sm.run(records, fn)
    lst = merger._records_list(got)
    assert lst == want
    s = sorter.Sorter(fn)
    s.insert_batch(recs.keys[: sum(len(k) for k, _ in records)], recs.key_end, recs.vals[: sum(len(v) for _, v in records)],
                   recs.val_end)
    assert _tensors(got) == _tensors(s.records())
    return lst


# ---------------------------------------------------------------- every boundary the scan has
def _boundary_sizes():
    """group sizes in sorted order and the (first, last) record of the groups the test is about"""
    sizes, pos, marks = [], 0, {}

    def add(size, name=None):
        nonlocal pos
        if name:
            marks[name] = (pos, pos + size - 1)
        sizes.append(size)
        pos += size

    def fill(to):   # singletons interleaved with groups of two and three
        i = 0
        while pos < to:
            add(min((1, 2, 1, 3)[i % 4], to - pos))
            i += 1

    add(1)
    add(5, "in_wave")
    fill(60)
    add(8, "rec_63_64")              # records 60 .. 67: straddles 63|64 (lanes 15 .. 16 at 4 records a lane)
    fill(250)
    add(9, "wave_edge")              # 250 .. 258: lanes 62 .. 64, the edge between waves 0 and 1
    fill(900)
    add(2200, "long")                # 900 .. 3099: tiles 1 and 2 hold no head
    fill(4090)
    add(10, "tile_edge")             # 4090 .. 4099: straddles 4095|4096
    fill(5112)
    add(8, "ends_on_tile")           # 5112 .. 5119
    add(7, "begins_on_tile")         # 5120 .. 5126
    fill(6001)
    add(4, "last")                   # the batch ends inside a group, in a partial tile
    return sizes, marks


@pytest.fixture(scope="module")
def boundary():
    """keys: the group number, 8 bytes big-endian; 8 random u64 per record, a fifth of them near
    2^64 so that sums wrap and a signed compare would misorder; input order shuffled.  Shared."""
    sizes, marks = _boundary_sizes()
    assert marks["in_wave"][1] < WAVE * 4 and marks["in_wave"][0] // 4 != marks["in_wave"][1] // 4
    assert marks["rec_63_64"] == (60, 67) and marks["wave_edge"][0] // (4 * WAVE) != marks["wave_edge"][1] // (4 * WAVE)
    a, b = marks["long"]
    assert b - a + 1 >= 2100 and a // TILE == 0 and b // TILE == 3
    assert marks["tile_edge"][0] // TILE == 3 and marks["tile_edge"][1] // TILE == 4
    assert (marks["ends_on_tile"][1] + 1) % TILE == 0 and marks["begins_on_tile"][0] % TILE == 0
    assert sum(sizes) % 4 != 0 and sizes.count(1) > 500
    rng = np.random.default_rng(31)
    n = sum(sizes)
    f = rng.integers(0, 1 << 63, size=(n, 8), dtype=np.uint64) * 2 + rng.integers(0, 2, size=(n, 8), dtype=np.uint64)
    f[rng.random((n, 8)) < 0.2] |= np.uint64(0xFFFF_FFFF_0000_0000)
    keys = np.repeat(np.arange(len(sizes)), sizes)
    order = rng.permutation(n)
    return keys, f, order


@pytest.mark.parametrize("ops", [("sum",), ("sum", "min", "max"), ("max",) * 8], ids=["F1_sum", "F3_mixed", "F8_max"])
def test_sort_every_boundary(boundary, ops):
    keys, f, order = boundary
    records = [(int(keys[i]).to_bytes(8, "big"), f[i, : len(ops)].astype("<u8").tobytes()) for i in order]
    got = _check_sort(records, ops)
    assert len(got) == int(keys[-1]) + 1
    if ops == ("sum",):   # and once against numpy, group by group
        want = np.zeros(len(got), np.uint64)
        np.add.at(want, keys, f[:, 0])
        assert [v for _, v in got] == [int(x).to_bytes(8, "little") for x in want]


@pytest.mark.parametrize("ops", [("min",), ("sum", "sum")])
def test_sort_boundaries_other_ops(boundary, ops):
    keys, f, order = boundary
    records = [(int(keys[i]).to_bytes(8, "big"), f[i, 2: 2 + len(ops)].astype("<u8").tobytes()) for i in order]
    _check_sort(records, ops)


def test_one_record_one_group_nothing():
    assert _check_sort([], ("sum",)) == []
    assert _check_sort([(b"k", u(7))], ("sum",)) == [(b"k", u(7))]
    assert _check_sort([(b"k", u(7, 9))], ("sum",)) == [(b"k", u(7, 9))]
    assert _check_sort([(b"k", u(i)) for i in range(1, 4)], ("sum",)) == [(b"k", u(6))]
    assert _check_sort([(b"k", u(4)), (b"k", u(9))], ("max",)) == [(b"k", u(9))]


def test_unsigned_and_wrapping():
    top = 1 << 63
    got = _check_sort([(b"a", u(M)), (b"a", u(2)), (b"b", u(top)), (b"b", u(5)), (b"b", u(top + 9))], ("sum",))
    assert got == [(b"a", u(1)), (b"b", u((2 * top + 14) & M))]
    recs = [(b"b", u(top)), (b"b", u(5)), (b"b", u(top + 9)), (b"c", u(M)), (b"c", u(top))]
    assert _check_sort(recs, ("min",)) == [(b"b", u(5)), (b"c", u(top))]
    assert _check_sort(recs, ("max",)) == [(b"b", u(top + 9)), (b"c", u(M))]
    got = _check_sort([(b"k", u(1, 100, 100)), (b"k", u(1, 90, 250)), (b"k", u(M, 95, 120))], ("sum", "min", "max"))
    assert got == [(b"k", u(1, 90, 250))]


def test_pass_through():
    """a 3-byte value alone in its group stays a 3-byte value and is no error, next to real groups"""
    got = _check_sort([(b"b", u(1)), (b"a", b"xyz"), (b"b", u(2)), (b"c", b""), (b"d", b"x" * 100)], ("sum",))
    assert got == [(b"a", b"xyz"), (b"b", u(3)), (b"c", b""), (b"d", b"x" * 100)]


# ---------------------------------------------------------------- the bare C ABI
class _Raw:
    """mtblx_sort_plan + mtblx_sort_emit_reduce with buffers the test owns: the input values and every
    output lie `shift` bytes after a 16-byte boundary in 0xA5-filled buffers, the outputs `short[name]`
    bytes smaller than the plan's size and with a 64-byte guard on both sides"""

    def __init__(self, records, ops, shift=0, short=None, plan=True):
        torch, mtblx, _lib, encode, merger, reader, sorter = _mods()
        L = mtblx.lib()
        short = short or {}
        rec = encode.DeviceRecords.from_list(records)
        vb = sum(len(v) for _, v in records)
        self.vin = torch.zeros(vb + 32, dtype=torch.uint8, device="cuda")
        o = ((self.vin.data_ptr() + 15) & ~15) - self.vin.data_ptr() + shift
        self.vin[o: o + vb] = rec.vals[:vb]
        self.rec = encode.DeviceRecords(rec.keys, rec.key_end, self.vin[o: o + vb], rec.val_end)
        self.val_ptr = self.vin.data_ptr() + o
        one = (_lib.Records * 1)()
        one[0] = self.rec.cstruct()
        n = self.rec.n
        wsb = int(L.mtblx_sort_workspace_bytes(n))
        ws = torch.zeros(wsb + 256, dtype=torch.uint8, device="cuda")
        wp = (ws.data_ptr() + 255) & ~255
        tot = (C.c_uint64 * 6)()
        if plan:
            assert L.mtblx_sort_plan(one, tot, C.c_void_p(wp), wsb, None) == 0
            groups, kb, nv, vbytes = (int(x) for x in tot[:4])
        else:
            groups, kb, nv, vbytes = 8, 64, 8, 64
        self.totals = [int(x) for x in tot]
        self.size = {"keys": kb, "key_end": 8 * groups, "vals": vbytes, "val_end": 8 * groups}
        self.cap, self.buf, ptr = {}, {}, {}
        for name, sz in self.size.items():
            self.cap[name] = max(sz - short.get(name, 0), 0)
            t = torch.full((64 + sz + 64 + 32,), 0xA5, dtype=torch.uint8, device="cuda")
            ptr[name] = ((t.data_ptr() + 64 + 15) & ~15) + (shift if name in ("keys", "vals") else 0)
            self.buf[name] = (t, ptr[name] - t.data_ptr())
        self.vals_ptr = ptr["vals"]
        flags = torch.full((1,), 0x5A5A, dtype=torch.int32, device="cuda")
        out = _lib.Merged(ptr["keys"], self.cap["keys"], ptr["key_end"], self.cap["key_end"], ptr["vals"],
                          self.cap["vals"], ptr["val_end"], self.cap["val_end"], 0, 0, flags.data_ptr())
        spec = mtblx.Reduce(*ops).cstruct()
        self.rc_emit = L.mtblx_sort_emit_reduce(one, C.byref(spec), C.byref(out), C.c_void_p(wp), wsb, None)
        torch.cuda.synchronize()
        self.flags = int(flags.item())

    def bytes(self, name, n=None):
        t, off = self.buf[name]
        return t[off: off + (self.size[name] if n is None else n)].cpu().numpy().tobytes()

    def untouched_from(self, name, start):
        t, off = self.buf[name]
        return bool((t[off + start:] == 0xA5).all()) and bool((t[:off] == 0xA5).all())

    def records(self):
        ke, ve = (np.frombuffer(self.bytes(n), np.uint64).tolist() for n in ("key_end", "val_end"))
        k, v = self.bytes("keys"), self.bytes("vals", ve[-1] if ve else 0)
        return [(k[(ke[i - 1] if i else 0): ke[i]], v[(ve[i - 1] if i else 0): ve[i]]) for i in range(len(ke))]


def _alignment_records():
    """sorted input: a singleton of odd length before every group, so the groups' source values and
    output slots walk through every residue mod 8"""
    odd, recs = [1, 3, 7, 9, 17], []
    for j in range(40):
        recs.append((b"k%03da" % j, bytes([j + 1]) * odd[j % 5]))
        for i in range(2 + j % 3):
            recs.append((b"k%03db" % j, u((M - 3 * j + i) & M, j * 1000 + i)))
    return recs


@pytest.mark.parametrize("shift", [0, 1])
def test_alignment(shift):
    records = _alignment_records()
    fn = reducer("sum", "max")
    want, _ = sm.run(records, fn)
    r = _Raw(records, ("sum", "max"), shift=shift)
    assert r.rc_emit == 0 and r.flags == 0
    assert r.records() == want
    src, dst, so, do = set(), set(), 0, 0
    for k, v in records:
        if len(v) == 16:
            src.add((r.val_ptr + so) % 8)
        so += len(v)
    for k, v in want:
        if len(v) == 16:
            dst.add((r.vals_ptr + do) % 8)
        do += len(v)
    assert src == set(range(8)) and dst == set(range(8))
    assert r.untouched_from("vals", do) and all(r.untouched_from(n, r.size[n]) for n in ("keys", "key_end", "val_end"))


def _capacity_records():
    return [(b"k%03d" % (i % 37) + b"x" * (i % 5), u(i, i * i)) for i in range(1500)] + [(b"a-solo", b"abc")]


@pytest.mark.parametrize("name", ["vals", "val_end", "keys"])
def test_capacity_one_byte_short(name):
    """MTBLX_MERGE_OVERFLOW, nothing written from the short capacity on, the guards untouched.  vals is
    sized by its upper bound (totals[3]), so for it the capacity is cut to one byte less than used"""
    torch, mtblx, _lib, encode, merger, reader, sorter = _mods()
    records = _capacity_records()
    full = _Raw(records, ("sum", "min"))
    assert full.rc_emit == 0 and full.flags == 0
    want, _ = sm.run(records, reducer("sum", "min"))
    assert full.records() == want
    used = sum(len(v) for _, v in want)
    short = {name: 1 if name != "vals" else full.size["vals"] - used + 1}
    r = _Raw(records, ("sum", "min"), short=short)
    assert r.rc_emit == 0 and r.flags == _lib.MERGE_OVERFLOW
    assert r.cap[name] == (full.size[name] if name != "vals" else used) - 1
    assert r.untouched_from(name, r.cap[name])
    for other in r.size:
        assert r.untouched_from(other, r.size[other] if other != "vals" else used)
        if other != name:
            assert r.bytes(other, used if other == "vals" else None) == full.bytes(other, used if other == "vals" else None)


def test_not_planned():
    """an emit over a zeroed workspace: MTBLX_MERGE_NOT_PLANNED, nothing written"""
    torch, mtblx, _lib, encode, merger, reader, sorter = _mods()
    r = _Raw([(b"k%04d" % (i // 3), u(i)) for i in range(3000)], ("sum",), plan=False)
    assert r.rc_emit == 0 and r.flags == _lib.MERGE_NOT_PLANNED
    assert all(r.untouched_from(n, 0) for n in r.size)


# ---------------------------------------------------------------- BADVALUE
def _bad_cases():
    pad = [(b"a%04d" % i, u(i)) for i in range(40)]
    long = [(b"m", u(i)) for i in range(1200)]
    return {
        "first": pad + [(b"m", b"\x01" * 7), (b"m", u(2))],
        "last": pad + [(b"m", u(2)), (b"m", b"\x01" * 7)],
        "other_tile": pad + long[:1150] + [(b"m", b"\x01" * 7)] + long[1150:],   # the head in tile 0, the bad value in tile 1
        "other_tile_first": pad + [(b"m", b"\x01" * 7)] + long,
        "too_long": pad + [(b"m", u(1, 2)), (b"m", u(1, 2))],
        "empty": pad + [(b"m", b""), (b"m", b"")],
    }


@pytest.mark.parametrize("case", ["first", "last", "other_tile", "other_tile_first", "too_long", "empty"])
def test_bad_value(case):
    torch, mtblx, _lib, encode, merger, reader, sorter = _mods()
    records = _bad_cases()[case]
    recs = encode.DeviceRecords.from_list(records)
    with pytest.raises(mtblx.MergeError):
        sorter.sort_records(recs, "sum_u64")
    with pytest.raises(BadLength):   # the callable path, and the model, for the same input
        s = sorter.Sorter(reducer("sum"))
        for k, v in records:
            s.insert(k, v)
        s.records()
    with pytest.raises(BadLength):
        sm.run(records, reducer("sum"))
    r = _Raw(records, ("sum",))
    assert r.rc_emit == 0 and r.flags == _lib.MERGE_BADVALUE
    got = r.records()
    assert got[:40] == records[:40] and got[40][0] == b"m"       # the other groups are right, the bad one inside its slot
    assert all(r.untouched_from(n, r.size[n]) for n in ("keys", "key_end", "val_end"))
    assert r.untouched_from("vals", sum(len(v) for _, v in got))
    # the same through the Sorter: the value meets its partner in the same chunk
    s = sorter.Sorter(mtblx.Reduce("sum"))
    for k, v in records:
        s.insert(k, v)
    with pytest.raises(mtblx.MergeError):
        s.records()


def test_bad_value_across_chunks_and_sources():
    """a 7-byte value alone in its chunk passes through it and fails where it meets a partner"""
    torch, mtblx, _lib, encode, merger, reader, sorter = _mods()
    a = encode.DeviceRecords.from_list([(b"a", u(1)), (b"m", b"\x01" * 7)])
    b = encode.DeviceRecords.from_list([(b"m", u(5)), (b"z", u(1))])
    assert merger._records_list(merger.merge_records([a], "sum_u64")) == [(b"a", u(1)), (b"m", b"\x01" * 7)]
    with pytest.raises(mtblx.MergeError):
        merger.merge_records([a, b], mtblx.Reduce("sum"))
    with pytest.raises(mtblx.MergeError):
        merger.merge_records([b, a], mtblx.Reduce("sum"))
    with pytest.raises(BadLength):
        mm.merge_iter([[(b"a", u(1)), (b"m", b"\x01" * 7)], [(b"m", u(5)), (b"z", u(1))]], reducer("sum"))


# ---------------------------------------------------------------- the Merger
def _sources(nsrc, per, seed):
    """sorted sources of 8-byte values; a third of a source's keys come from one pool that every
    source draws four fifths of, the rest are its own"""
    rng = np.random.default_rng(seed)
    pool = [b"s%06d" % k for k in range(per // 3 * 5 // 4)]
    out = []
    for s in range(nsrc):
        shared = {k for k in pool if rng.random() < 0.8}
        private = rng.choice(per * 2, size=per - per // 3, replace=False)
        keys = sorted(shared | {b"p%02d-%06d" % (s, k) for k in private})
        out.append([(k, u(int(rng.integers(0, 1 << 63)) * 2 + 1)) for k in keys])
    return out


def _check_merger(sources, ops, model=True):
    torch, mtblx, _lib, encode, merger, reader, sorter = _mods()
    fn = reducer(*ops)
    files = [mm.make_source(s) for s in sources]
    recs = [mm.source_records(f) for f in files]
    readers = [reader.Reader(f) for f in files]
    m = merger.Merger.builder(mtblx.Reduce(*ops)).extend(readers).build()
    got = m.records()
    lst = merger._records_list(got)
    if model:
        assert lst == mm.merge_iter(recs, fn)
    host = merger.Merger.builder(fn).extend(readers).build()
    assert _tensors(got) == _tensors(host.records())
    assert list(m.into_merge_iter()) == lst
    return m, host, lst


@pytest.mark.parametrize("nsrc", [1, 2, 7, 64])
def test_merger_random_sources(oracle, nsrc):
    src = _sources(nsrc, 3000 // nsrc + 30, 50 + nsrc)
    m, host, lst = _check_merger(src, ("sum",))
    assert nsrc == 1 or len(lst) < sum(len(s) for s in src) * 0.95   # groups of two or more exist
    if nsrc == 7:
        assert m.write_file(1024, 16).cpu().numpy().tobytes() == host.write_file(1024, 16).cpu().numpy().tobytes()


def test_merger_three_fields(oracle):
    rng = np.random.default_rng(77)
    src = [[(b"k%05d" % k, u(1, int(rng.integers(0, 1 << 62)), int(rng.integers(0, 1 << 62))))
            for k in sorted(rng.choice(900, size=500, replace=False))] for _ in range(5)]
    _check_merger(src, ("sum", "min", "max"))


@pytest.mark.parametrize("case", ["E1_followers", "E1_alone", "E2_followers", "E2_alone"])
def test_merger_empty_key_quirk(oracle, case):
    """the four cases of test_merger_gpu.test_empty_key_quirk with 8-byte values.  E2_alone: the
    reference keeps whichever value its BinaryHeap pops last; this library documents the
    highest-numbered source's, so that case is checked against the documented choice"""
    src = {
        "E1_followers": [[(b"", u(10)), (b"a", u(1))], [(b"a", u(2)), (b"b", u(3))]],
        "E1_alone": [[(b"", u(10))], []],
        "E2_followers": [[(b"", u(10)), (b"b", u(1))], [(b"", u(11))], [(b"a", u(2))]],
        "E2_alone": [[(b"", u(10))], [(b"", u(11))]],
    }[case]
    _, _, lst = _check_merger(src, ("sum",), model=case != "E2_alone")
    assert lst == {
        "E1_followers": [(b"a", u(3)), (b"b", u(3))],
        "E1_alone": [(b"", u(10))],
        "E2_followers": [(b"a", u(2)), (b"b", u(1))],
        "E2_alone": [(b"", u(11))],
    }[case]


def test_merger_70_sources(oracle):
    """two rounds of 64: the common key's sum covers 70 values"""
    src = [sorted([(b"common", u(M - s if s % 9 == 0 else s + 1))] + [(b"p%02d-%d" % (s, j), u(s * 10 + j)) for j in range(3)])
           for s in range(70)]
    _, _, lst = _check_merger(src, ("sum",))
    want = sum(M - s if s % 9 == 0 else s + 1 for s in range(70)) & M
    assert dict(lst)[b"common"] == u(want) and len(lst) == 1 + 70 * 3


# ---------------------------------------------------------------- the Sorter, several chunks
N3 = 131_073 + 131_072 + 40_000


@pytest.fixture(scope="module")
def three_chunks():
    """8-byte key + 8-byte value records that cut into three chunks with max_memory at its minimum
    (the capacity doubles at insert 131 073, which cuts; the next cut comes 131 072 later); a quarter
    of the keys lie in more than one chunk.  Shared, never changed."""
    rng = np.random.default_rng(41)
    ids = rng.permutation(N3).astype(np.uint64)
    q = N3 // 4
    ids[-q:] = ids[:q]
    vals = rng.integers(0, 1 << 63, size=N3, dtype=np.uint64) * 2 + 1
    vals[rng.random(N3) < 0.2] |= np.uint64(0xFFFF_FFFF_0000_0000)
    kb, vb = ids.astype(">u8").view(np.uint8), vals.astype("<u8").view(np.uint8)
    ends = np.arange(1, N3 + 1, dtype=np.int64) * 8
    pos = np.arange(N3)
    chunk = np.where(pos < 131_073, 0, np.where(pos < 131_073 + 131_072, 1, 2))
    first = {}
    multi = set()
    for i, c in zip(ids.tolist(), chunk.tolist()):
        if first.setdefault(i, c) != c:
            multi.add(i)
    assert len(multi) >= len(first) // 5
    kbytes, vbytes = kb.tobytes(), vb.tobytes()
    records = [(kbytes[8 * i: 8 * i + 8], vbytes[8 * i: 8 * i + 8]) for i in range(N3)]
    model = {}
    for nb in (25, 1):
        out, s = sm.run(records, reducer("sum"), max_memory=0, max_nb_chunks=nb)
        model[nb] = (out, s.chunk_sizes, s.merges)
    return (kb, ends, vb), records, model


@pytest.mark.parametrize("nb, snappy", [(25, False), (1, False), (25, True)])
def test_sorter_three_chunks(three_chunks, nb, snappy):
    torch, mtblx, _lib, encode, merger, reader, sorter = _mods()
    (kb, ends, vb), records, model = three_chunks
    out, chunk_sizes, merges = model[nb]
    assert chunk_sizes == [131_073, 131_072, 40_000] and merges == (1 if nb == 1 else 0)
    comp = mtblx.CompressionType.Snappy if snappy else mtblx.CompressionType.None_
    files = []
    for merge in (mtblx.Reduce("sum"), reducer("sum")):
        b = sorter.Sorter.builder(merge).max_memory(0)
        if nb != 25:
            b.max_nb_chunks(nb)
        s = b.build()
        s.insert_batch(*(torch.from_numpy(x).cuda() for x in (kb, ends, vb, ends)))
        files.append(s.write_file(compression=comp).cpu().numpy().tobytes())
        assert s.chunk_sizes == chunk_sizes and s.merges == merges
    assert files[0] == files[1]
    if not snappy and nb == 25:   # and against the model, once
        s = sorter.Sorter.builder("sum_u64").max_memory(0).build()
        s.insert_batch(*(torch.from_numpy(x).cuda() for x in (kb, ends, vb, ends)))
        assert merger._records_list(s.records()) == out

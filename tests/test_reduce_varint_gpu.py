"""Varint-coded values through the reduce family on the GPU (mtblx.Reduce(..., encoding="varint") over
mtblx_merge_emit_reduce / mtblx_sort_emit_reduce / mtblx_merge_seg_emit_reduce / mtblx_scan_reduce /
mtblx_reduce_segments with MTBLX_REDUCE_VARINT).

Expected values never come from the code under test: the few-line reducer below, written over
pyoracle.varint_decode64 / varint_encode64 (src/varint.rs restated in C), is fed to
tests/merger_model.py and tests/sorter_model.py and, as a callable, to this library's host path;
files and tensors of the device path and of the callable path must be byte-identical.  The
aggregating calls are checked against Reduce.fold, itself checked in tests/test_reduce_varint.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import merger_model as mm
import merger_scan_util as msu
import scan_util as su
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


def V(*ops):
    import mtblx
    return mtblx.Reduce(*ops, encoding="varint")


class BadValue(Exception):
    pass


def reducer(*ops):
    """the reducer of these tests, over the oracle's coder: never the library's own"""
    import pyoracle

    def fields(v):
        out, p = [], 0
        for _ in ops:
            if p >= len(v):
                raise BadValue()          # an empty rest: the reference would panic
            x, used = pyoracle.varint_decode64(v[p:])
            if used <= 0:
                raise BadValue()
            out.append(x)
            p += used
        if p != len(v):
            raise BadValue()
        return out

    def fn(_key, values):
        rows = [fields(v) for v in values]
        out = b""
        for f, op in enumerate(ops):
            xs = [r[f] for r in rows]
            out += pyoracle.varint_encode64(sum(xs) % 2 ** 64 if op == "sum" else min(xs) if op == "min" else max(xs))
        return out
    return fn


def enc(*xs):
    out = bytearray()
    for x in xs:
        while x >= 128:
            out.append((x & 127) | 128)
            x >>= 7
        out.append(x)
    return bytes(out)


def rand_fields(rng, n, F):
    """[n, F] u64 whose bit lengths are uniform over 1 .. 64, so all ten varint lengths occur"""
    bits = rng.integers(1, 65, size=(n, F))
    x = rng.integers(0, 1 << 63, size=(n, F), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, F), dtype=np.uint64)
    x >>= (64 - bits).astype(np.uint64)
    return x | (np.uint64(1) << (bits - 1).astype(np.uint64))


def _tensors(r):
    return tuple(t.cpu().numpy().tobytes() for t in (r.keys[: int(r.key_end[-1]) if r.n else 0], r.key_end,
                                                     r.vals[: int(r.val_end[-1]) if r.n else 0], r.val_end))


def _check_sort(records, ops):
    """sort_records(Reduce) == the model == the callable path: keys, key_end, vals, val_end"""
    torch, mtblx, _lib, encode, merger, reader, sorter = _mods()
    fn = reducer(*ops)
    recs = encode.DeviceRecords.from_list(records)
    got = sorter.sort_records(recs, V(*ops))
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
    add(3, "in_lane")                # records 1 .. 3: one lane's four records
    add(5, "across_lanes")           # 4 .. 8
    fill(250)
    add(9, "across_waves")           # 250 .. 258: lanes 62 .. 64, the edge between waves 0 and 1
    fill(900)
    add(2200, "three_edges")         # 900 .. 3099: tiles 1 and 2 hold no head
    fill(4090)
    add(10, "one_edge")              # 4090 .. 4099: straddles 4095|4096
    fill(5112)
    add(8, "ends_on_tile")           # 5112 .. 5119
    add(7, "begins_on_tile")         # 5120 .. 5126
    fill(6001)
    add(4, "last")                   # the batch ends inside a group, in a partial tile
    return sizes, marks


@pytest.fixture(scope="module")
def boundary():
    """keys: the group number, 16 bytes big-endian; 8 random fields per record of every varint length;
    in every seventh group of two the fields are M - r and r + 1 + t, so that the sum wraps to t and
    the result is shorter than the group's first value.  Input order shuffled.  Shared."""
    sizes, marks = _boundary_sizes()
    a, b = marks["in_lane"]
    assert a // 4 == b // 4
    a, b = marks["across_lanes"]
    assert a // 4 != b // 4 and a // (4 * WAVE) == b // (4 * WAVE)
    a, b = marks["across_waves"]
    assert a // (4 * WAVE) != b // (4 * WAVE) and a // TILE == b // TILE
    a, b = marks["three_edges"]
    assert a // TILE == 0 and b // TILE == 3
    assert marks["one_edge"][0] // TILE == 3 and marks["one_edge"][1] // TILE == 4
    assert (marks["ends_on_tile"][1] + 1) % TILE == 0 and marks["begins_on_tile"][0] % TILE == 0
    assert sum(sizes) % 4 != 0 and sizes.count(1) > 500
    rng = np.random.default_rng(131)
    n = sum(sizes)
    f = rand_fields(rng, n, 8)
    keys = np.repeat(np.arange(len(sizes)), sizes)
    start = np.cumsum([0] + sizes[:-1])
    for g in [g for g, s in enumerate(sizes) if s == 2][::7]:
        r = rng.integers(0, 1 << 40, size=8, dtype=np.uint64)
        f[start[g]] = np.uint64(M) - r
        f[start[g] + 1] = r + np.uint64(1) + rng.integers(0, 300, size=8, dtype=np.uint64)
    order = rng.permutation(n)
    return keys, f, order


@pytest.mark.parametrize("ops", [("sum",), ("min", "max", "sum"), ("sum", "min", "max", "max", "min", "sum", "sum", "min")],
                         ids=["F1_sum", "F3_mixed", "F8"])
def test_sort_every_boundary(oracle, boundary, ops):
    keys, f, order = boundary
    F = len(ops)
    records = [(int(keys[i]).to_bytes(16, "big"), enc(*(int(x) for x in f[i, :F]))) for i in order]
    assert {len(enc(int(x))) for x in f[:, :F].ravel()} == set(range(1, 11))
    got = _check_sort(records, ops)
    assert len(got) == int(keys[-1]) + 1
    # the result against the group's first value (the first inserted: the sort is stable): longer, equal, shorter
    first, size = {}, {}
    for k, v in records:
        first.setdefault(k, len(v))
        size[k] = size.get(k, 0) + 1
    rel = {(len(v) > first[k]) - (len(v) < first[k]) for k, v in got if size[k] > 1}
    assert rel == {-1, 0, 1}
    if ops == ("sum",):   # and once against numpy, group by group
        want = np.zeros(len(got), np.uint64)
        np.add.at(want, keys, f[:, 0])
        assert [v for _, v in got] == [enc(int(x)) for x in want]


def test_pass_through_of_singles(oracle):
    """alone in its group a value stays as it is: bad, non-canonical, empty or 100 bytes long"""
    recs = [(b"b", enc(1)), (b"a", b"\x80\x80"), (b"b", enc(2)), (b"c", b""), (b"d", b"\xff" * 100), (b"e", b"\x85\x00"),
            (b"f", b"\x81\x00"), (b"f", b"\x82\x00"), (b"g", b"\x80" * 11)]
    got = _check_sort(recs, ("sum",))
    assert got == [(b"a", b"\x80\x80"), (b"b", b"\x03"), (b"c", b""), (b"d", b"\xff" * 100), (b"e", b"\x85\x00"),
                   (b"f", b"\x03"), (b"g", b"\x80" * 11)]
    assert _check_sort([], ("sum",)) == []
    assert _check_sort([(b"k", b"\x80\x00")], ("max", "min")) == [(b"k", b"\x80\x00")]


# ---------------------------------------------------------------- the bare C ABI
class _Raw:
    """mtblx_sort_plan + mtblx_sort_emit_reduce with buffers the test owns.  The input values lie
    `shift` bytes after a 16-byte boundary and end with their tensor; every output lies (keys and
    vals: `shift` bytes after a 16-byte boundary) in a 0xA5-filled buffer, `short[name]` bytes
    smaller than the plan's size, with a 64-byte guard on both sides"""

    def __init__(self, records, ops, shift=0, short=None, plan=True):
        torch, mtblx, _lib, encode, merger, reader, sorter = _mods()
        L = mtblx.lib()
        short = short or {}
        rec = encode.DeviceRecords.from_list(records)
        vb = sum(len(v) for _, v in records)
        self.vin = torch.zeros(16 + shift + vb, dtype=torch.uint8, device="cuda")   # the last value ends the tensor
        o = 16 + shift
        assert self.vin.data_ptr() % 16 == 0
        self.vin[o:] = rec.vals[:vb]
        self.rec = encode.DeviceRecords(rec.keys, rec.key_end, self.vin[o:], rec.val_end)
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
        spec = V(*ops).cstruct()
        self.rc_emit = L.mtblx_sort_emit_reduce(one, C.byref(spec), C.byref(out), C.c_void_p(wp), wsb, None)
        torch.cuda.synchronize()
        self.flags = int(flags.item())

    def bytes(self, name, n=None):
        t, off = self.buf[name]
        return t[off: off + (self.size[name] if n is None else n)].cpu().numpy().tobytes()

    def untouched_from(self, name, start):
        """nothing written from byte `start` of the output on, nor before the output"""
        t, off = self.buf[name]
        return bool((t[off + start:] == 0xA5).all()) and bool((t[:off] == 0xA5).all())

    def records(self):
        ke, ve = (np.frombuffer(self.bytes(n), np.uint64).tolist() for n in ("key_end", "val_end"))
        k, v = self.bytes("keys"), self.bytes("vals", ve[-1] if ve else 0)
        return [(k[(ke[i - 1] if i else 0): ke[i]], v[(ve[i - 1] if i else 0): ve[i]]) for i in range(len(ke))]


def _alignment_records():
    """sorted input: a singleton of odd length before every group, so the groups' source values and
    output slots walk through every residue mod 8; the very last value is a ten-byte varint of a
    group of two, ending with the tensor"""
    odd, recs = [1, 3, 7, 9, 17], []
    for j in range(40):
        recs.append((b"k%03da" % j, bytes([0x80 + j]) * odd[j % 5]))
        for i in range(2 + j % 3):
            recs.append((b"k%03db" % j, enc((M - 3 * j + i) & M, j * 1000 + i)))
    recs += [(b"zz", enc(5, M)), (b"zz", enc(6, M))]
    return recs


@pytest.mark.parametrize("shift", [0, 1])
def test_end_of_allocation_and_alignment(oracle, shift):
    """the last value's last byte is the last byte of its tensor, and source values and output slots
    lie at every residue mod 8: the results must be right at every alignment.  This does not by itself
    catch a read past a value's end (the byte after the tensor still lies in the allocator's block, and
    the emit kernels' source reads are not bounds-checked): that rule rests on the loader's loop, whose
    every byte load is guarded by the value's length, and on test_bad_value's unterminated value, which
    a read of the next value's first byte would turn into a good one"""
    records = _alignment_records()
    want, _ = sm.run(records, reducer("sum", "max"))
    r = _Raw(records, ("sum", "max"), shift=shift)
    assert r.vin.numel() == 16 + shift + sum(len(v) for _, v in records) and records[-1][1][-10:] == enc(M)
    assert r.rc_emit == 0 and r.flags == 0
    assert r.records() == want
    src, so = set(), 0
    for k, v in records:
        src.add((r.val_ptr + so) % 8)
        so += len(v)
    assert src == set(range(8))
    used = sum(len(v) for _, v in want)
    assert r.untouched_from("vals", used) and all(r.untouched_from(n, r.size[n]) for n in ("keys", "key_end", "val_end"))


def _capacity_records():
    return [(b"k%03d" % (i % 37) + b"x" * (i % 5), enc(i, i * i)) for i in range(1500)] + [(b"a-solo", b"\x80\x80\x80")]


@pytest.mark.parametrize("name", ["vals", "val_end", "keys"])
def test_capacity_one_byte_short(oracle, name):
    """MTBLX_MERGE_OVERFLOW, nothing written from the short capacity on, the guards untouched.  vals is
    sized by its upper bound (totals[3]), so for it the capacity is cut to one byte less than used"""
    torch, mtblx, _lib, encode, merger, reader, sorter = _mods()
    records = _capacity_records()
    full = _Raw(records, ("sum", "min"))
    assert full.rc_emit == 0 and full.flags == 0
    want, _ = sm.run(records, reducer("sum", "min"))
    assert full.records() == want
    used = sum(len(v) for _, v in want)
    assert used < full.size["vals"]
    short = {name: 1 if name != "vals" else full.size["vals"] - used + 1}
    r = _Raw(records, ("sum", "min"), short=short)
    assert r.rc_emit == 0 and r.flags == _lib.MERGE_OVERFLOW
    assert r.cap[name] == (full.size[name] if name != "vals" else used) - 1
    assert r.untouched_from(name, r.cap[name])
    for other in r.size:
        assert r.untouched_from(other, r.size[other] if other != "vals" else used)
    if name != "val_end":   # val_end decides where every value goes: the other outputs are whole only when it is
        for other in ("keys", "key_end", "val_end"):
            if other != name:
                assert r.bytes(other) == full.bytes(other)
    else:                   # every group but the last has its slot
        assert r.bytes("val_end", r.cap["val_end"] // 8 * 8) == full.bytes("val_end", r.cap["val_end"] // 8 * 8)
        assert r.bytes("keys") == full.bytes("keys") and r.bytes("key_end") == full.bytes("key_end")


def test_not_planned(oracle):
    """an emit over a zeroed workspace: MTBLX_MERGE_NOT_PLANNED, nothing written"""
    torch, mtblx, _lib, encode, merger, reader, sorter = _mods()
    r = _Raw([(b"k%04d" % (i // 3), enc(i)) for i in range(3000)], ("sum",), plan=False)
    assert r.rc_emit == 0 and r.flags == _lib.MERGE_NOT_PLANNED
    assert all(r.untouched_from(n, 0) for n in r.size)


@pytest.mark.parametrize("plan, emit", [("merge", "sort"), ("sort", "merge")])
def test_emit_refuses_the_other_kind_of_plan(oracle, plan, emit):
    """a varint reduce emit of one kind over a workspace planned by the other kind over the same
    records: MTBLX_MERGE_NOT_PLANNED and nothing written.  The workspace is a real plan's: it holds
    heads, groups of two and three, groups of one, group numbers and a group count, so a length pass,
    a scan of val_end, a store pass or a copy of the singles that ran would write val_end and vals."""
    torch, mtblx, _lib, encode, merger, reader, sorter = _mods()
    L = mtblx.lib()
    keys = [b"k%05d" % i for i in range(2600)]
    a = [(k, enc(i, 3 * i)) for i, k in enumerate(keys)]                              # every key
    b = [(k, enc(M - i, i)) for i, k in enumerate(keys) if i % 3 == 0]                # a third of them twice
    c = [(k, enc(7, i)) for i, k in enumerate(keys) if i % 6 == 0]                    # a sixth three times
    srcs = [encode.DeviceRecords.from_list(s) for s in (a, b, c)]
    whole = encode.DeviceRecords.from_list(a + b + c)                                 # the Sorter's batch: the same records
    n = whole.n
    many = (_lib.Records * 3)()
    for i, s in enumerate(srcs):
        many[i] = s.cstruct()
    one = (_lib.Records * 1)()
    one[0] = whole.cstruct()
    wsb = max(int(L.mtblx_sort_workspace_bytes(n)), int(L.mtblx_merge_workspace_bytes(n, 3)))
    ws = torch.zeros(wsb + 256, dtype=torch.uint8, device="cuda")
    wp = C.c_void_p((ws.data_ptr() + 255) & ~255)
    tot = (C.c_uint64 * 6)()
    rc = L.mtblx_merge_plan(many, 3, tot, wp, wsb, None) if plan == "merge" else L.mtblx_sort_plan(one, tot, wp, wsb, None)
    groups, kb, nv, vbytes = (int(x) for x in tot[:4])
    assert rc == 0 and groups == len(keys) and nv == n and n > 3 * TILE     # four tiles of records
    size = {"keys": kb, "key_end": 8 * groups, "vals": vbytes, "val_end": 8 * groups}
    buf = {name: torch.full((64 + sz + 64,), 0xA5, dtype=torch.uint8, device="cuda") for name, sz in size.items()}
    ptr = {name: t.data_ptr() + 64 for name, t in buf.items()}
    flags = torch.full((1,), 0x5A5A, dtype=torch.int32, device="cuda")
    out = _lib.Merged(ptr["keys"], size["keys"], ptr["key_end"], size["key_end"], ptr["vals"], size["vals"], ptr["val_end"],
                      size["val_end"], 0, 0, flags.data_ptr())
    spec = V("sum", "max").cstruct()
    if emit == "sort":
        rc = L.mtblx_sort_emit_reduce(one, C.byref(spec), C.byref(out), wp, wsb, None)
    else:
        rc = L.mtblx_merge_emit_reduce(many, 3, C.byref(spec), C.byref(out), wp, wsb, None)
    torch.cuda.synchronize()
    assert rc == 0 and int(flags.item()) == _lib.MERGE_NOT_PLANNED
    for name, t in buf.items():
        assert bool((t == 0xA5).all()), name
    # the same emit over its own kind of plan writes all four outputs
    rc = L.mtblx_sort_plan(one, tot, wp, wsb, None) if emit == "sort" else L.mtblx_merge_plan(many, 3, tot, wp, wsb, None)
    assert rc == 0 and [int(x) for x in tot[:4]] == [groups, kb, nv, vbytes]
    if emit == "sort":
        rc = L.mtblx_sort_emit_reduce(one, C.byref(spec), C.byref(out), wp, wsb, None)
    else:
        rc = L.mtblx_merge_emit_reduce(many, 3, C.byref(spec), C.byref(out), wp, wsb, None)
    torch.cuda.synchronize()
    assert rc == 0 and int(flags.item()) == 0
    ve = np.frombuffer(buf["val_end"][64: 64 + size["val_end"]].cpu().numpy().tobytes(), np.uint64)
    vals = buf["vals"][64: 64 + int(ve[-1])].cpu().numpy().tobytes()
    fn = reducer("sum", "max")
    want = [fn(k, [v for s in (a, b, c) for kk, v in s if kk == k]) if i % 3 == 0 else a[i][1] for i, k in enumerate(keys[:12])]
    assert [vals[(int(ve[i - 1]) if i else 0): int(ve[i])] for i in range(12)] == want


# ---------------------------------------------------------------- BADVALUE
BAD = {                                 # (fields, the bad value)
    "empty": (2, b""),
    "unterminated": (1, b"\x81"),         # the next value's first byte would end it: nothing past the value is read
    "too_few_fields": (3, b"\x01\x02"),
    "trailing_byte": (2, b"\x01\x02\x03"),
    "eleventh_continuation": (1, b"\x80" * 10 + b"\x01"),
}


@pytest.mark.parametrize("where", ["first", "last", "other_tile"])
@pytest.mark.parametrize("shape", sorted(BAD))
def test_bad_value(oracle, shape, where):
    torch, mtblx, _lib, encode, merger, reader, sorter = _mods()
    nf, bad = BAD[shape]
    ops = ("sum", "min", "max")[:nf]
    good = lambda i: enc(*range(i + 1, i + 1 + nf))   # noqa: E731
    pad = [(b"a%04d" % i, good(i)) for i in range(40)]
    long = [(b"m", good(i)) for i in range(1200)]
    records = {"first": pad + [(b"m", bad), (b"m", good(2))],
               "last": pad + [(b"m", good(2)), (b"m", bad)],
               "other_tile": pad + long[:1150] + [(b"m", bad)] + long[1150:]}[where]   # the head in tile 0, the bad value in tile 1
    records = records + [(b"z", good(7)), (b"z", good(8))]
    recs = encode.DeviceRecords.from_list(records)
    with pytest.raises(mtblx.MergeError):
        sorter.sort_records(recs, V(*ops))
    with pytest.raises(BadValue):   # the callable path, and the model, for the same input
        s = sorter.Sorter(reducer(*ops))
        for k, v in records:
            s.insert(k, v)
        s.records()
    with pytest.raises(BadValue):
        sm.run(records, reducer(*ops))
    r = _Raw(records, ops)
    assert r.rc_emit == 0 and r.flags == _lib.MERGE_BADVALUE
    got = r.records()
    # the other groups are right, the bad one holds its first value: the layout stays defined
    assert got[:40] == records[:40] and got[40] == (b"m", records[40][1]) and got[41] == (b"z", reducer(*ops)(b"z", [good(7), good(8)]))
    assert len(got) == 42
    assert all(r.untouched_from(n, r.size[n]) for n in ("keys", "key_end", "val_end"))
    assert r.untouched_from("vals", sum(len(v) for _, v in got))
    s = sorter.Sorter(V(*ops))   # the same through the Sorter: the value meets its partner in the same chunk
    for k, v in records:
        s.insert(k, v)
    with pytest.raises(mtblx.MergeError):
        s.records()


def test_bad_value_across_sources(oracle):
    """a bad value alone in its source passes through it and fails where it meets a partner"""
    torch, mtblx, _lib, encode, merger, reader, sorter = _mods()
    a = encode.DeviceRecords.from_list([(b"a", enc(1)), (b"m", b"\x80\x80")])
    b = encode.DeviceRecords.from_list([(b"m", enc(5)), (b"z", enc(1))])
    assert merger._records_list(merger.merge_records([a], V("sum"))) == [(b"a", enc(1)), (b"m", b"\x80\x80")]
    for srcs in ([a, b], [b, a]):
        with pytest.raises(mtblx.MergeError):
            merger.merge_records(srcs, V("sum"))
    with pytest.raises(BadValue):
        mm.merge_iter([[(b"a", enc(1)), (b"m", b"\x80\x80")], [(b"m", enc(5)), (b"z", enc(1))]], reducer("sum"))


# ---------------------------------------------------------------- the Merger
def _sources(nsrc, per, seed, F=1):
    """sorted sources; a third of a source's keys come from one pool that every source draws four
    fifths of, the rest are its own"""
    rng = np.random.default_rng(seed)
    pool = [b"s%06d" % k for k in range(per // 3 * 5 // 4)]
    out = []
    for s in range(nsrc):
        shared = {k for k in pool if rng.random() < 0.8}
        private = rng.choice(per * 2, size=per - per // 3, replace=False)
        keys = sorted(shared | {b"p%02d-%06d" % (s, k) for k in private})
        f = rand_fields(rng, len(keys), F)
        out.append([(k, enc(*(int(x) for x in f[i]))) for i, k in enumerate(keys)])
    return out


def _check_merger(sources, ops, model=True):
    torch, mtblx, _lib, encode, merger, reader, sorter = _mods()
    fn = reducer(*ops)
    files = [mm.make_source(s) for s in sources]
    recs = [mm.source_records(f) for f in files]
    readers = [reader.Reader(f) for f in files]
    m = merger.Merger.builder(V(*ops)).extend(readers).build()
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
    src = _sources(nsrc, 3000 // nsrc + 30, 150 + nsrc)
    m, host, lst = _check_merger(src, ("sum",))
    assert nsrc == 1 or len(lst) < sum(len(s) for s in src) * 0.95   # groups of two or more exist
    if nsrc == 7:
        assert m.write_file(1024, 16).cpu().numpy().tobytes() == host.write_file(1024, 16).cpu().numpy().tobytes()


def test_merger_three_fields(oracle):
    _check_merger(_sources(5, 500, 177, F=3), ("min", "max", "sum"))


@pytest.mark.parametrize("case", ["E1_followers", "E1_alone", "E2_followers", "E2_alone"])
def test_merger_empty_key_quirk(oracle, case):
    """the four cases of test_merger_gpu.test_empty_key_quirk with varint values.  E2_alone: the
    reference keeps whichever value its BinaryHeap pops last; this library documents the
    highest-numbered source's, so that case is checked against the documented choice"""
    src = {
        "E1_followers": [[(b"", enc(10)), (b"a", enc(127))], [(b"a", enc(1)), (b"b", enc(3))]],
        "E1_alone": [[(b"", enc(10))], []],
        "E2_followers": [[(b"", enc(10)), (b"b", enc(1))], [(b"", enc(11))], [(b"a", enc(2))]],
        "E2_alone": [[(b"", enc(10))], [(b"", enc(300))]],
    }[case]
    _, _, lst = _check_merger(src, ("sum",), model=case != "E2_alone")
    assert lst == {
        "E1_followers": [(b"a", b"\x80\x01"), (b"b", enc(3))],
        "E1_alone": [(b"", enc(10))],
        "E2_followers": [(b"a", enc(2)), (b"b", enc(1))],
        "E2_alone": [(b"", enc(300))],
    }[case]


def test_merger_70_sources(oracle):
    """two rounds of 64: the common key's sum covers 70 values, and a round's canonical partial result
    goes into the next round as a source value"""
    src = [sorted([(b"common", enc(M - s if s % 9 == 0 else s + 1))] + [(b"p%02d-%d" % (s, j), enc(s * 10 + j)) for j in range(3)])
           for s in range(70)]
    src[3][0] = (b"common", b"\x84\x80\x00")   # 4, not canonical
    _, _, lst = _check_merger(src, ("sum",))
    want = sum(M - s if s % 9 == 0 else s + 1 for s in range(70)) & M
    assert dict(lst)[b"common"] == enc(want) and len(lst) == 1 + 70 * 3


@functools.lru_cache(maxsize=None)
def _varint_small_sources(bs):
    """merger_scan_util.small_sources with every 8-byte value (below 4000) re-coded as one varint of 1 to 9 bytes"""
    datas, lists, qs = msu.small_sources(bs, True)
    lists = [[(k, enc(int.from_bytes(v, "little") << (7 * (i % 8)))) for i, (k, v) in enumerate(r)] for r in lists]
    return [mm.make_source(r, bs, 4) for r in lists], lists, qs


def test_merger_scan_batch(oracle):
    """Merger.scan_batch with a varint Reduce: mtblx_merge_seg_emit_reduce"""
    torch, mtblx, _lib, encode, merger, reader, sorter = _mods()
    datas, lists, qs = _varint_small_sources(1024)
    fn = reducer("sum")
    m = merger.Merger.builder(V("sum")).extend([reader.Reader(d) for d in datas]).build()
    res = m.scan_batch(qs)
    multi = 0
    for q, query in enumerate(qs):
        groups = msu.promised_groups(msu.per_source(oracle, datas, query, ("varint-small", 1024)))
        assert res.records(q) == [(k, vs[0] if len(vs) == 1 else fn(k, vs)) for k, vs in groups], query
        multi += sum(len(vs) > 1 for _, vs in groups)
    assert multi > 50 and any(res.served_by_kernel(q) for q in range(len(qs)))


# ---------------------------------------------------------------- the Sorter, several chunks
N3 = 360_000   # 8-byte keys and values of 5.5 bytes on average: the chunks are cut near 160 000 and 315 000 records


@pytest.fixture(scope="module")
def three_chunks(oracle):
    """8-byte key + one-varint value records that cut into three chunks with max_memory at its minimum
    (a cut comes when the entries' bytes reach 2 MiB beside the doubled vector of 8 MiB);
    a quarter of the keys lie in more than one chunk.  Shared, never changed."""
    rng = np.random.default_rng(141)
    ids = rng.permutation(N3).astype(np.uint64)
    q = N3 // 4
    ids[-q:] = ids[:q]
    vals = rand_fields(rng, N3, 1)[:, 0]
    kb = ids.astype(">u8").view(np.uint8)
    venc = [enc(int(x)) for x in vals]
    vb = np.frombuffer(b"".join(venc), np.uint8).copy()
    kends = np.arange(1, N3 + 1, dtype=np.int64) * 8
    vends = np.cumsum([len(v) for v in venc], dtype=np.int64)
    kbytes = kb.tobytes()
    records = [(kbytes[8 * i: 8 * i + 8], venc[i]) for i in range(N3)]
    out, s = sm.run(records, reducer("sum"), max_memory=0, max_nb_chunks=25)
    assert len(s.chunk_sizes) == 3 and s.merges == 0
    return (kb, kends, vb, vends), records, out, s.chunk_sizes


@pytest.mark.parametrize("nb, snappy", [(25, False), (1, False), (25, True)])
def test_sorter_three_chunks(oracle, three_chunks, nb, snappy):
    torch, mtblx, _lib, encode, merger, reader, sorter = _mods()
    arrays, records, out, chunk_sizes = three_chunks
    comp = mtblx.CompressionType.Snappy if snappy else mtblx.CompressionType.None_
    files = []
    for merge in (V("sum"), reducer("sum")):
        b = sorter.Sorter.builder(merge).max_memory(0)
        if nb != 25:
            b.max_nb_chunks(nb)
        s = b.build()
        s.insert_batch(*(torch.from_numpy(x).cuda() for x in arrays))
        files.append(s.write_file(compression=comp).cpu().numpy().tobytes())
        assert s.chunk_sizes == chunk_sizes and s.merges == (1 if nb == 1 else 0)
    assert files[0] == files[1]
    if not snappy and nb == 25:   # and against the model, once
        s = sorter.Sorter.builder(V("sum")).max_memory(0).build()
        s.insert_batch(*(torch.from_numpy(x).cuda() for x in arrays))
        assert merger._records_list(s.records()) == out


def test_sorter_bad_value_meets_its_partner_when_the_chunks_merge(oracle, three_chunks):
    """a bad value alone in the first chunk passes through it; its partner arrives in the last chunk"""
    torch, mtblx, _lib, encode, merger, reader, sorter = _mods()
    (kb, kends, vb, vends), records, out, chunk_sizes = three_chunks
    key = b"\xff" * 8            # above every id: in no chunk
    s = sorter.Sorter.builder(V("sum")).max_memory(0).build()
    s.insert(key, b"\x80\x80")
    s.insert_batch(*(torch.from_numpy(x).cuda() for x in (kb, kends, vb, vends)))
    assert len(s.chunk_sizes) >= 2
    alone = merger._records_list(s.records())
    assert alone[-1] == (key, b"\x80\x80") and alone[:-1] == out     # no partner: it passes through every round
    s = sorter.Sorter.builder(V("sum")).max_memory(0).build()
    s.insert(key, b"\x80\x80")
    s.insert_batch(*(torch.from_numpy(x).cuda() for x in (kb, kends, vb, vends)))
    assert len(s.chunk_sizes) >= 2   # the first chunk is cut: the bad value went through it alone
    s.insert(key, enc(5))
    with pytest.raises(mtblx.MergeError):
        s.records()


# ---------------------------------------------------------------- the aggregating calls
OPS3 = ("min", "max", "sum")


def _values(rng, n, F):
    """n values of F varints of every length; about 4 % bad in every shape"""
    f = rand_fields(rng, n, F)
    out = []
    for i in range(n):
        v = enc(*(int(x) for x in f[i]))
        r = rng.random()
        if r < 0.01:
            v = v[:-1] + bytes([v[-1] | 0x80])       # unterminated
        elif r < 0.02:
            v = v + b"\x01"                          # a trailing byte
        elif r < 0.03:
            v = b""
        elif r < 0.04:
            v = b"\x80" * 10 + v                     # an eleventh continuation byte
        elif r < 0.08:
            v = b"\x80" + v if v[0] < 0x80 else v    # not canonical, or two fields where one is asked
        out.append(v)
    return out


@functools.lru_cache(maxsize=None)
def _file_case(comp):
    """-> (data, records, queries, limits): 1500 records in blocks of 512 bytes"""
    rng = np.random.default_rng(900 + comp)
    keys = sorted({b"k%02d-%05d" % (int(i) // 100, int(i)) for i in rng.choice(3000, size=1500, replace=False)})
    recs = list(zip(keys, _values(rng, len(keys), 3)))
    data = su.write(recs, 512, 4, comp)
    qs = [("get", keys[7]), ("get", keys[-1]), ("get", b"nothing"), ("prefix", b"k03-"), ("prefix", b"k1"),
          ("range", keys[100], keys[400]), ("range", keys[5], keys[5]), ("from", keys[-3]), ("from", keys[600]),
          ("from", b""), ("prefix", b"zz"), ("from", keys[50])]
    lim = [None] * 8 + [40, None, None, 0]
    return data, recs, qs, lim


@pytest.mark.parametrize("comp", [0, 1], ids=["plain", "snappy"])
def test_reader_reduce_batch(oracle, comp):
    torch, mtblx, _lib, encode, merger, reader, sorter = _mods()
    data, recs, qs, lim = _file_case(comp)
    red = V(*OPS3)
    r = reader.Reader(data)
    # a matched value that is the last bytes of its data block, and one that is the last value of the file
    ikeys = [k for k, _ in r._index_records()]
    keys = [k for k, _ in recs]
    assert len(ikeys) > 20
    qs = qs + [("get", max(k for k in keys if k <= ikeys[3]))]   # block 3's last record: its separator is at or above it
    lim = lim + [None]
    rb = r.reduce_batch(qs, red, max_blocks=8, max_records=lim)
    nbad = 0
    for i, (q, m) in enumerate(zip(qs, lim)):
        e = su.expected(oracle, data, q, m, True)
        want = red.fold([v for _, v in e["records"]])
        assert (rb.values(i),) + rb.counts(i) == want, (i, q, m)
        vb = rb.value_bytes(i)
        assert vb == (None if want[1] == want[2] else enc(*want[0])), (i, q)
        nbad += want[2]
    assert nbad > 10 and rb.counts(1)[0] == 1 and rb.counts(len(qs) - 1)[0] == 1
    served = [rb.served_by_kernel(i) for i in range(len(qs))]
    assert any(served) and not all(served) and rb.n_large > 0      # ("from", b"") opens every block: the seek path
    with pytest.raises(mtblx.MergeError):
        rb.check()


def test_merger_reduce_batch(oracle):
    torch, mtblx, _lib, encode, merger, reader, sorter = _mods()
    datas, lists, qs = _varint_small_sources(256)
    fn, red = reducer("sum"), V("sum")
    m = merger.Merger.builder(red).extend([reader.Reader(d) for d in datas]).build()
    rb = m.reduce_batch(qs)
    for q, query in enumerate(qs):
        groups = msu.promised_groups(msu.per_source(oracle, datas, query, ("varint-small", 256)))
        items = [vs[0] if len(vs) == 1 else fn(k, vs) for k, vs in groups]
        assert (rb.values(q),) + rb.counts(q) == red.fold(items), query
    rb.check()
    # another spec than the merge function: "concat" joins two or three varints, which one field does not hold
    rc = merger.Merger.builder("concat").extend([reader.Reader(d) for d in datas]).build().reduce_batch(qs, V("max"))
    for q, query in enumerate(qs):
        groups = msu.promised_groups(msu.per_source(oracle, datas, query, ("varint-small", 256)))
        assert (rc.values(q),) + rc.counts(q) == V("max").fold([b"".join(vs) for _, vs in groups]), query
    assert sum(rc.counts(q)[1] for q in range(len(qs))) > 10


def _device_records(values, lead=1):
    """values as DeviceRecords whose vals start `lead` bytes into their allocation and end with it"""
    import torch
    from mtblx.encode import DeviceRecords
    blob = b"\xee" * lead + b"".join(values)
    buf = torch.frombuffer(bytearray(blob or b"\0"), dtype=torch.uint8).cuda()
    ve = torch.from_numpy(np.cumsum([len(v) for v in values], dtype=np.int64) if values else np.zeros(0, np.int64)).cuda()
    z = torch.zeros(0, dtype=torch.uint8, device="cuda")
    return DeviceRecords(z, ve.clone(), buf[lead:], ve)


def _seg_check(red, vals, segs, fields, nbad):
    f, nb = fields.cpu().numpy().view(np.uint64), nbad.cpu().numpy()
    assert f.shape == (len(segs), len(red.ops)) and nb.shape == (len(segs),)
    for s, (lo, hi) in enumerate(segs):
        want = red.fold(vals[lo:hi])
        assert (tuple(int(x) for x in f[s]), int(nb[s])) == (want[0], want[2]), (s, lo, hi)


@functools.lru_cache(maxsize=None)
def _segments_case():
    T = 1024
    n = 4 * T + 300
    vals = _values(np.random.default_rng(277), n, 3)
    segs = [(0, 0), (0, 1), (1, 4), (4, 4), (5, 40), (40, 300), (310, T + 5), (T + 5, T + 5),
            (T + 10, 4 * T + 7),                       # spans three tile edges, two whole tiles inside
            (4 * T + 7, 4 * T + 8), (4 * T + 100, n), (n, n)]
    return T, n, vals, segs


@pytest.mark.parametrize("F", [1, 3, 8])
def test_reduce_segments(oracle, F):
    torch, mtblx, _lib, encode, merger, reader, sorter = _mods()
    T, n, vals, segs = _segments_case()
    assert int(_lib.lib().mtblx_reduce_seg_tile()) == T
    if F != 3:
        vals = _values(np.random.default_rng(F), n, F)
    red = V(*(OPS3 * 3)[:F])
    rec = _device_records(vals)
    assert rec.vals.data_ptr() % 2 == 1
    fields, nbad = mtblx.reduce_segments(rec, [a for a, _ in segs], [b for _, b in segs], red)
    _seg_check(red, vals, segs, fields, nbad)
    assert sum(red.fold(vals[a:b])[2] for a, b in segs) > 20
    for sg in ([(0, n)], [(i, min(i + 7, n)) for i in range(0, n, 11)]):
        f, nb = mtblx.reduce_segments(rec, [a for a, _ in sg], [b for _, b in sg], red)
        _seg_check(red, vals, sg, f, nb)


# ---------------------------------------------------------------- a non-default stream
@pytest.fixture(scope="module")
def stream():
    import stream_util as S
    _mods()
    return S.pick_streams(1)[0]


@pytest.mark.parametrize("family", ["sort", "merge", "merger_scan", "reader_reduce", "merger_reduce", "segments"])
def test_non_default_stream(oracle, stream, family):
    """one varint call of each family under stream_util's "own-held" configuration: the stream the call
    is given is busy, so a launch, a fill or a read-back on any other stream shows as wrong bytes"""
    import stream_util as S
    torch, mtblx, _lib, encode, merger, reader, sorter = _mods()
    red = V(*OPS3)
    if family in ("sort", "merge"):
        src = _sources(2, 400, 31, F=3)
        if family == "sort":
            records = src[0] + src[1]
            recs = encode.DeviceRecords.from_list(records)
            call = lambda st: sorter.sort_records(recs, red, stream=st)                        # noqa: E731
            want, _ = sm.run(records, reducer(*OPS3))
        else:
            recs = [encode.DeviceRecords.from_list(s) for s in src]
            call = lambda st: merger.merge_records(recs, red, stream=st)                       # noqa: E731
            want = mm.merge_iter(src, reducer(*OPS3))
        call(None)                                    # loads the kernels before any hold
        got = S.run("own-held", call, stream)
        with torch.cuda.stream(stream):
            assert merger._records_list(got) == want
    elif family in ("merger_scan", "merger_reduce"):
        datas, lists, qs = _varint_small_sources(1024)
        qs = qs[:30]
        readers = [reader.Reader(d) for d in datas]
        for r in readers:
            r.index_regular()
        fn = reducer("sum")
        exp = [msu.promised_groups(msu.per_source(oracle, datas, q, ("varint-small", 1024))) for q in qs]
        items = [[(k, vs[0] if len(vs) == 1 else fn(k, vs)) for k, vs in g] for g in exp]
        if family == "merger_scan":
            call = lambda st: merger.Merger(readers, V("sum")).scan_batch(qs, stream=st)        # noqa: E731
            call(None)
            res = S.run("own-held", call, stream)
            assert [res.records(q) for q in range(len(qs))] == items
        else:
            call = lambda st: merger.Merger(readers, V("sum")).reduce_batch(qs, stream=st)      # noqa: E731
            call(None)
            rb = S.run("own-held", call, stream)
            assert [(rb.values(q),) + rb.counts(q) for q in range(len(qs))] == [V("sum").fold([v for _, v in it]) for it in items]
    elif family == "reader_reduce":
        data, recs, qs, lim = _file_case(1)
        r = reader.Reader(data)
        r.index_regular()
        call = lambda st: r.reduce_batch(qs, red, max_blocks=8, max_records=lim, stream=st)     # noqa: E731
        call(None)
        rb = S.run("own-held", call, stream)
        for i, (q, m) in enumerate(zip(qs, lim)):
            e = su.expected(oracle, data, q, m, True)
            assert (rb.values(i),) + rb.counts(i) == red.fold([v for _, v in e["records"]]), (i, q)
    else:
        T, n, vals, segs = _segments_case()
        rec = _device_records(vals)
        lo = torch.tensor([a for a, _ in segs], dtype=torch.int64, device="cuda")
        hi = torch.tensor([b for _, b in segs], dtype=torch.int64, device="cuda")
        call = lambda st: mtblx.reduce_segments(rec, lo, hi, red, stream=st)                   # noqa: E731
        call(None)
        f, nb = S.run("own-held", call, stream)
        with torch.cuda.stream(stream):
            _seg_check(red, vals, segs, f, nb)

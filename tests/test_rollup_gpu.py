"""Rollups on the GPU: rollup_records (mtblx_rollup_plan / _emit, mtblx_reduce_segments,
mtblx_reduce_encode), Reader.rollup / rollup_batch, Merger.rollup / rollup_batch, Rollup.write_file.

Expected values never come from the code under test: they are tests/rollup_model.py (the host
definition, pinned by hand in tests/test_rollup.py) over the test's own record lists, over what the
oracle's iteration yields for a query, or over the Merger's model.  Every comparison is bit for bit:
keys, key_end, values, val_end, fields, nrec, nbad, grp_rec and seg_grp."""
import ctypes as C
import functools

import numpy as np
import pytest

import corpus
import merger_scan_util as msu
import rollup_model as rm
import scan_util as su

pytestmark = pytest.mark.gpu

M = (1 << 64) - 1
OPS = {1: ("sum",), 3: ("sum", "min", "max"), 8: ("sum", "min", "max", "max", "min", "sum", "sum", "min")}


def _mods():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mtblx import reader
    return reader


def _tile():
    _mods()
    import mtblx
    return int(mtblx.lib().mtblx_rollup_tile())


def _red(F, encoding="u64le"):
    from mtblx import Reduce
    return Reduce(*OPS[F], encoding=encoding)


def _device_records(recs, lead=0):
    """DeviceRecords of a record list; `lead`: the key and value bytes start that far into their buffers"""
    import torch
    from mtblx.encode import DeviceRecords
    _mods()
    ks = b"\xa5" * lead + b"".join(k for k, _ in recs)
    vs = b"\x5a" * lead + b"".join(v for _, v in recs)
    ke = np.cumsum([len(k) for k, _ in recs], dtype=np.int64) if recs else np.zeros(0, np.int64)
    ve = np.cumsum([len(v) for _, v in recs], dtype=np.int64) if recs else np.zeros(0, np.int64)
    t = lambda b: torch.frombuffer(bytearray(b or b"\0"), dtype=torch.uint8).cuda()[lead if b else 0:]  # noqa: E731
    return DeviceRecords(t(ks), torch.from_numpy(ke).cuda(), t(vs), torch.from_numpy(ve).cuda())


def _ends(parts):
    return np.cumsum([len(p) for p in parts], dtype=np.int64) if parts else np.zeros(0, np.int64)


def _compare(ro, m, stream=None):
    """a Rollup against the model, bit for bit"""
    import torch
    with torch.cuda.stream(stream):
        r = ro.records
        got = dict(keys=r.keys.cpu().numpy().tobytes(), key_end=r.key_end.cpu().numpy(),
                   vals=r.vals.cpu().numpy().tobytes(), val_end=r.val_end.cpu().numpy(),
                   fields=ro.fields.cpu().numpy().view(np.uint64), nrec=ro.nrec.cpu().numpy(),
                   nbad=ro.nbad.cpu().numpy(), grp_rec=ro.grp_rec.cpu().numpy(), seg_grp=ro.seg_grp.cpu().numpy())
    G = len(m["keys"])
    assert ro.ngroups == G
    assert got["grp_rec"].tolist() == m["grp_rec"]
    assert got["seg_grp"].tolist() == m["seg_grp"]
    assert got["key_end"].tolist() == _ends(m["keys"]).tolist()
    assert got["keys"] == b"".join(m["keys"])
    assert got["nrec"].tolist() == m["nrec"]
    assert got["nbad"].tolist() == m["nbad"]
    assert got["fields"].shape == (G, len(ro.reduce.ops))
    assert [tuple(int(x) for x in row) for row in got["fields"]] == m["fields"]
    assert got["val_end"].tolist() == _ends(m["values"]).tolist()
    assert got["vals"] == b"".join(m["values"])
    assert r.stream is ro._stream


def _roll(recs, group, red, seg_off=None, lead=0, stream=None):
    from mtblx import rollup_records
    ro = rollup_records(_device_records(recs, lead), group, red, seg_off, stream)
    m = rm.rollup(recs, group, red, seg_off)
    _compare(ro, m)
    return ro, m


def _u64(*xs):
    return b"".join((x & M).to_bytes(8, "little") for x in xs)


def _values(rng, n, red, bad=0.03):
    """n values of `red`'s shape: random u64 fields, bit 63 set in a third; about `bad` of them bad"""
    F = len(red.ops)
    out = []
    for _ in range(n):
        w = [int(x) for x in rng.integers(0, 1 << 62, F, dtype=np.uint64)]
        w = [x | (1 << 63) if rng.random() < 0.33 else x >> int(rng.integers(0, 62)) for x in w]
        v = red.encode(w)
        if rng.random() < bad:
            v = [v[:-1], v + b"\x00", b"", v[:-1] + b"\x80"][int(rng.integers(0, 4))]
        out.append(v)
    return out


# ---------------------------------------------------------------- 1. the tile edges
def _shaped(n, shape, T, rng):
    """n sorted keys "g<group>.<record>" whose groups have the asked shape"""
    if shape == "own":
        gid = list(range(n))
    elif shape == "one":
        gid = [0] * n
    else:
        sizes = [2 * T + 2] if n > 3 * T else []     # spans three tiles wherever it starts
        while sum(sizes) < n:
            sizes.append(int(rng.integers(1, 40)))
        rng.shuffle(sizes)
        gid = [g for g, s in enumerate(sizes) for _ in range(s)][:n]
    return [b"g%05d." % g + b"%07d" % i for i, g in enumerate(gid)]


@pytest.mark.parametrize("shape", ["own", "one", "random"])
@pytest.mark.parametrize("nname", ["0", "1", "2", "T-1", "T", "T+1", "3T+5"])
def test_tile_edges(nname, shape):
    from mtblx import GroupBy
    T = _tile()
    n = {"0": 0, "1": 1, "2": 2, "T-1": T - 1, "T": T, "T+1": T + 1, "3T+5": 3 * T + 5}[nname]
    rng = np.random.default_rng(n + len(shape))
    keys = _shaped(n, shape, T, rng)
    assert keys == sorted(keys)
    red = _red(3)
    recs = list(zip(keys, _values(rng, n, red)))
    for group in (GroupBy.length(7), GroupBy.delimiter(0x2e)):
        ro, m = _roll(recs, group, red)
        G = len(m["keys"])
        # the inputs hold the shape they are named for
        if shape == "own":
            assert G == n
        elif shape == "one":
            assert G == min(n, 1)
        elif n > 3 * T:
            assert any(m["grp_rec"][g] // T + 2 <= (m["grp_rec"][g + 1] - 1) // T for g in range(G))
            assert len(set(m["nrec"])) > 5
        assert m["keys"] == sorted(set(m["keys"]))          # strictly increasing: a Writer's input
        assert ro.groups(0) == rm.groups_of(m, 0)


# ---------------------------------------------------------------- 2. the length rule
@pytest.mark.parametrize("L", [1, 8, 9, 257])
def test_length_rule(L):
    from mtblx import GroupBy, Reduce
    base = bytes((i * 7) % 200 + 2 for i in range(300))
    d = bytearray(base[:L])
    d[L - 1] += 1
    z = b"\xf0" * 300
    keys = [b""]                                            # an empty first key
    if L > 1:
        keys.append(base[: L - 1])                          # shorter than L, a strict prefix of the next
    keys += [base[:L],                                      # exactly L
             base[:L] + b"\x01", base[:L] + b"\x02tail",    # longer; they differ only at byte L: one group
             bytes(d) + b"\x02tail",                        # differs from its predecessor only at byte L - 1
             z, z[:299] + b"\xf1",                          # 300-byte keys that differ at byte 299: one group
             z[: L - 1] + b"\xf1" + z[L:]]                  # and one that differs at byte L - 1
    assert keys == sorted(keys) and len(keys[-1]) == 300
    want_heads = [True] + ([True] if L > 1 else []) + [True, False, False, True, True, False, True]
    red = Reduce("sum")
    recs = [(k, _u64(i + 1)) for i, k in enumerate(keys)]
    assert rm.heads(recs, ("length", L)) == want_heads
    for lead in (0, 3):
        ro, m = _roll(recs, GroupBy.length(L), red, lead=lead)
    assert m["keys"][0] == b"" and m["keys"][-1] == keys[-1][:L] and sum(m["nrec"]) == len(keys)
    ro.check()


# ---------------------------------------------------------------- 3. the delimiter rule
@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("byte", [0x00, 0x2e, 0xff])
def test_delimiter_rule(byte, count):
    from mtblx import GroupBy, Reduce
    D = bytes([byte])
    long = bytearray(b"w" * 300)
    for p in (10, 20)[: count - 1]:
        long[p] = byte
    long[290] = byte                                        # the count-th delimiter at byte 290
    long[295] = byte                                        # and one more after it
    l2 = bytearray(long)
    l2[299] = 0x41                                          # equal up to the delimiter, differs after: one group
    l3 = bytearray(long)
    l3[289] = 0x41                                          # differs just before it: another group
    keys = [b"", b"abc", b"abd",                            # no delimiter: each key its own group key
            b"f" + D + b"g", b"f" + D + b"h",               # count 1: one group; count 3: fewer than count, two
            D + b"rest", D + b"rest2",                      # the delimiter as the first byte
            b"q" + D + D + D + b"r", b"q" + D + D + D + b"s",   # consecutive delimiters: one group either way
            b"t" + D + b"u" + D + b"v" + D,                 # the delimiter as the last byte
            b"t" + D + b"u" + D + b"v" + D + b"x",
            bytes(long), bytes(l2), bytes(l3)]
    rule = ("delimiter", byte, count)
    assert rm.gkey(bytes(long), rule) == bytes(long[:291]) == rm.gkey(bytes(l2), rule) != rm.gkey(bytes(l3), rule)
    assert rm.gkey(keys[9], rule) == keys[9][: 2 if count == 1 else 6]
    recs = [(k, _u64(i + 1)) for i, k in enumerate(keys)]
    want = [True, True, True, True, count == 3, True, count == 3, True, False, True, False, True, False, True]
    assert rm.heads(recs, rule) == want
    red = Reduce("sum")
    for lead in (0, 5):
        ro, m = _roll(recs, GroupBy.delimiter(byte, count), red, lead=lead)
    assert sum(m["nrec"]) == len(keys) and m["nbad"] == [0] * len(m["keys"])
    # keys that are the delimiter alone, over more than one 16-byte chunk
    recs = [(D * i, _u64(i)) for i in range(0, 70)]
    _roll(recs, GroupBy.delimiter(byte, count), red, lead=1)
    _roll(recs, GroupBy.delimiter(byte, 33), red)


# ---------------------------------------------------------------- 4. segments
@functools.lru_cache(maxsize=None)
def _seg_case():
    T = _tile()
    n = 3 * T + 5
    rng = np.random.default_rng(77)
    keys = _shaped(n, "random", T, rng)
    red = _red(3)
    return T, n, list(zip(keys, _values(rng, n, red))), red


@pytest.mark.parametrize("nseg", [1, 63, 64, 65, 257])
def test_segments(nseg):
    from mtblx import GroupBy
    T, n, recs, red = _seg_case()
    group = GroupBy.length(7)
    whole = rm.rollup(recs, group, red)
    big = max(range(len(whole["nrec"])), key=lambda g: whole["nrec"][g])
    inside = whole["grp_rec"][big] + 5                       # splits the run of the largest group
    if nseg == 1:
        seg = [0, n]
    else:
        rng = np.random.default_rng(nseg)
        cuts = [0, 0, inside, T, 2 * T, 2 * T, 2 * T, n, n]  # empty segments at the start, in the middle, at the end
        cuts += [int(x) for x in rng.integers(0, n + 1, nseg + 1 - len(cuts))]
        seg = sorted(cuts)
    assert len(seg) == nseg + 1
    ro, m = _roll(recs, group, red, seg)
    if nseg > 1:
        q = seg.index(inside)
        assert m["keys"][m["seg_grp"][q] - 1] == m["keys"][m["seg_grp"][q]]     # two groups with equal keys
        assert m["seg_grp"][0] == m["seg_grp"][1] == 0 and m["seg_grp"][-1] == m["seg_grp"][-2] == len(m["keys"])
        e = seg.index(2 * T)
        assert m["seg_grp"][e] == m["seg_grp"][e + 1] == m["seg_grp"][e + 2]   # empty segments in the middle
        assert T in m["grp_rec"] and 2 * T in m["grp_rec"]                      # boundaries at tile boundaries
    for q in sorted({0, min(1, nseg - 1), nseg // 2, nseg - 1}):
        assert ro.groups(q) == rm.groups_of(m, q)
    with pytest.raises(IndexError):
        ro.groups(nseg)
    ro, m = _roll(recs, GroupBy.delimiter(0x2e), red, seg, lead=7)


def _raw(rec, group, seg, nseg, caps=None, plan=True, ws_fill=None):
    """the two C calls over sentinel-filled outputs -> (rc of the emit, flags, outputs unchanged?, totals)"""
    import torch
    from mtblx import _lib, codec
    L = _lib.lib()
    n = rec.n
    r = _lib.Records(codec._u(rec.keys), codec._u(rec.key_end), 0, 0, n)
    g = group.cstruct()
    wsb = int(L.mtblx_rollup_workspace_bytes(n, nseg))
    ws = torch.zeros(wsb, dtype=torch.uint8, device="cuda")
    totals = torch.full((2,), 0x11, dtype=torch.int64, device="cuda")
    segt = torch.tensor(seg, dtype=torch.int64, device="cuda")
    if plan:
        assert L.mtblx_rollup_plan(C.byref(r), C.byref(g), C.c_void_p(segt.data_ptr()), nseg,
                                   C.c_void_p(totals.data_ptr()), C.c_void_p(ws.data_ptr()), wsb, None) == 0
    caps = caps or dict(keys=1 << 16, key_end=8 * n, grp_rec=8 * (n + 1), seg_grp=8 * (nseg + 1))
    keys = torch.full((1 << 16,), 0x5c, dtype=torch.uint8, device="cuda")
    key_end = torch.full((n,), 0x5555, dtype=torch.int64, device="cuda")
    grp_rec = torch.full((n + 1,), 0x6666, dtype=torch.int64, device="cuda")
    seg_grp = torch.full((nseg + 1,), 0x7777, dtype=torch.int64, device="cuda")
    flags = torch.full((2,), 0x33, dtype=torch.int32, device="cuda")
    out = _lib.Rolled(keys=keys.data_ptr(), keys_cap=caps["keys"], key_end=key_end.data_ptr(),
                      key_end_cap=caps["key_end"], grp_rec=grp_rec.data_ptr(), grp_rec_cap=caps["grp_rec"],
                      seg_grp=seg_grp.data_ptr(), seg_grp_cap=caps["seg_grp"], flags=flags.data_ptr())
    rc = L.mtblx_rollup_emit(C.byref(r), C.byref(g), C.c_void_p(segt.data_ptr()), nseg, C.byref(out),
                             C.c_void_p(ws.data_ptr()), wsb, None)
    torch.cuda.synchronize()
    same = bool((keys == 0x5c).all() and (key_end == 0x5555).all() and (grp_rec == 0x6666).all() and
                (seg_grp == 0x7777).all())
    return rc, flags.tolist(), same, totals.tolist()


@pytest.mark.parametrize("seg", [[0, 900, 700, 2000], [0, 700, 900, 1999], [0, 700, 900, 2001], [1, 700, 900, 2000],
                                 [0, 1 << 40, 900, 2000]],
                         ids=["decreasing", "ends-before-n", "ends-after-n", "starts-after-0", "far-out"])
def test_bad_seg_off_leaves_the_outputs(seg):
    from mtblx import GroupBy, Reduce, _lib, rollup_records
    T, n, recs, red = _seg_case()
    rec = _device_records(recs[:2000])
    for group in (GroupBy.length(7), GroupBy.delimiter(0x2e)):
        with pytest.raises(ValueError, match="seg_off"):
            rollup_records(rec, group, Reduce("sum"), seg)
        rc, flags, same, totals = _raw(rec, group, seg, 3)
        assert rc == 0 and flags == [_lib.ROLLUP_BADSEG, 0x33] and same and totals == [0, 0]


def test_emit_refuses_an_unplanned_workspace_and_small_capacities():
    from mtblx import GroupBy, _lib
    T, n, recs, red = _seg_case()
    rec = _device_records(recs[:2000])
    group, seg = GroupBy.length(7), [0, 700, 900, 2000]
    m = rm.rollup(recs[:2000], group, red, seg)
    G, kb = len(m["keys"]), sum(len(k) for k in m["keys"])
    rc, flags, same, totals = _raw(rec, group, seg, 3)                       # the control: it writes
    assert rc == 0 and flags == [0, 0x33] and not same and totals == [G, kb]
    rc, flags, same, _ = _raw(rec, group, seg, 3, plan=False)                # a zeroed workspace
    assert rc == 0 and flags == [_lib.ROLLUP_NOT_PLANNED, 0x33] and same
    exact = dict(keys=kb, key_end=8 * G, grp_rec=8 * (G + 1), seg_grp=8 * 4)
    rc, flags, same, _ = _raw(rec, group, seg, 3, caps=exact)
    assert rc == 0 and flags == [0, 0x33] and not same
    for name, short in (("keys", 1), ("key_end", 8), ("grp_rec", 8), ("seg_grp", 8)):
        rc, flags, same, _ = _raw(rec, group, seg, 3, caps=dict(exact, **{name: exact[name] - short}))
        assert rc == 0 and flags == [_lib.ROLLUP_OVERFLOW, 0x33] and same, name


# ---------------------------------------------------------------- 5. values
def _value_records(red, rng):
    """groups "g000" .. by length 4: the bad-value shapes, the varint length changes, then random groups"""
    F = len(red.ops)
    good = lambda *w: red.encode((list(w) + [7] * F)[:F])           # noqa: E731
    bad = [b"\x80" * 3, good(1)[:-1] + b"\x80", good(1) + b"\x00"] if red.varint else [b"", good(1)[:-1], good(1) + b"\x00"]
    groups = [[bad[1]],                                   # a bad value in a group of one
              [bad[0], bad[1], bad[2]],                   # a whole group of bad values
              [good(5), bad[2], good(9, 1)],              # a bad value among good ones
              [good(0x7f), good(0x01)],                   # varint: the sum needs one byte more than either input
              [good(M), good(1)],                         # varint: the sum wraps to 0, shorter than either input
              [good(1 << 63, 1 << 63, 1 << 63)] if F >= 3 else [good(1 << 63)]]
    while len(groups) < 60:
        groups.append(_values(rng, int(rng.integers(1, 30)), red, bad=0.0))
    return [(b"g%03d-%04d" % (g, i), v) for g, vs in enumerate(groups) for i, v in enumerate(vs)]


@pytest.mark.parametrize("encoding", ["u64le", "varint"])
@pytest.mark.parametrize("F", [1, 3, 8])
def test_values(F, encoding):
    from mtblx import GroupBy, MergeError
    red = _red(F, encoding)
    rng = np.random.default_rng(10 * F + len(encoding))
    recs = _value_records(red, rng)
    ro, m = _roll(recs, GroupBy.length(4), red, lead=1)
    ident = tuple(red.identities())
    assert m["nrec"][:3] == [1, 3, 3] and m["nbad"][:3] == [1, 3, 1]
    assert m["fields"][0] == m["fields"][1] == ident and m["values"][0] == red.encode(ident)
    assert any(x >> 63 for f in m["fields"] for x in f)
    if red.varint:      # field 0 is a sum: longer and shorter than every input
        assert m["values"][3][:2] == b"\x80\x01" and len(recs[7][1]) == len(recs[8][1]) == F
        assert m["values"][4][:1] == b"\x00" and len(m["values"][4]) == F and len(recs[9][1]) == 9 + F
    with pytest.raises(MergeError):
        ro.check()
    clean = [r for r in recs if not r[0].startswith((b"g000", b"g001", b"g002"))]
    ro, m = _roll(clean, GroupBy.length(4), red)
    assert sum(m["nbad"]) == 0
    ro.check()


@pytest.mark.parametrize("encoding", ["u64le", "varint"])
@pytest.mark.parametrize("F", [1, 3, 8])
def test_reduce_encode(F, encoding):
    import torch
    from mtblx import reduce_encode
    T = _tile()
    red = _red(F, encoding)
    rng = np.random.default_rng(F)
    edge = [0, 1, 127, 128, (1 << 14) - 1, 1 << 14, (1 << 56) - 1, 1 << 56, (1 << 63) - 1, 1 << 63, M]
    for n in (0, 1, T, T + 1):
        rows = [[edge[int(rng.integers(0, len(edge)))] if rng.random() < 0.5 else int(rng.integers(0, 1 << 62)) >>
                 int(rng.integers(0, 62)) for _ in range(F)] for _ in range(n)]
        t = torch.from_numpy(np.array(rows, dtype=np.uint64).reshape(n, F).view(np.int64)).cuda()
        vals, val_end = reduce_encode(t, red)
        want = [red.encode(r) for r in rows]
        assert val_end.cpu().numpy().tolist() == _ends(want).tolist()
        assert vals.cpu().numpy().tobytes() == b"".join(want)


# ---------------------------------------------------------------- 6. files
def _file_case(name):
    """the corpus files of tests/test_scan_reduce_gpu.py (F = 3) and every query of the mix once, unlimited"""
    import test_scan_reduce_gpu as tsr
    data, recs, qs, _ = tsr._case("1024-4-snappy" if name == "snappy" else "1024-4", 3)
    if name == "v1":
        data = corpus.to_v1(data)
    seen, out = set(), []
    for q in qs:
        if q not in seen:
            seen.add(q)
            out.append(q)
    return data, recs, out[:160], tsr._red(3)


def _file_groups(recs):
    """two rules that cut these random keys into groups of more than one record"""
    from collections import Counter
    from mtblx import GroupBy
    common = Counter(b for k, _ in recs for b in k[1:6]).most_common(1)[0][0]
    return [GroupBy.length(2), GroupBy.delimiter(common, 1)]


@pytest.mark.parametrize("name", ["plain", "snappy", "v1"])
def test_reader_rollup_batch(oracle, name):
    rd = _mods()
    data, recs, qs, red = _file_case(name)
    exps = [su.expected(oracle, data, q, None, True, tag=("rollup", name))["records"] for q in qs]
    assert any(not e for e in exps) and any(len(e) > 1000 for e in exps)
    for group in _file_groups(recs):
        models = [rm.rollup(e, group, red) for e in exps]
        assert any(max(m["nrec"], default=0) > 1 for m in models) and any(sum(m["nbad"]) for m in models)
        wide = rd.Reader(data).rollup_batch(qs, group, red, max_blocks=1 << 20)
        narrow = rd.Reader(data).rollup_batch(qs, group, red, max_blocks=1)      # hands queries back
        assert all(wide.served_by_kernel(q) for q in range(len(qs)))
        back = [q for q in range(len(qs)) if not narrow.served_by_kernel(q)]
        assert 0 < len(back) < len(qs)
        assert wide.nseg == narrow.nseg == len(qs)
        for q, m in enumerate(models):
            want = rm.groups_of(m, 0)
            assert wide.groups(q) == want, (q, qs[q])
            assert narrow.groups(q) == want, (q, qs[q])                          # whichever path answered it
            assert narrow.end(q) == rd.END_NONE and narrow.err(q) == "None"
        # the kernel path's answer is one rollup whose segments are the queries
        flat = [r for e in exps for r in e]
        seg = [0] + np.cumsum([len(e) for e in exps]).tolist()
        _compare(wide, rm.rollup(flat, group, red, seg))


@pytest.mark.parametrize("name", ["plain", "snappy", "v1"])
def test_reader_rollup(oracle, name):
    from mtblx import MergeError
    rd = _mods()
    data, recs, _, red = _file_case(name)
    for group in _file_groups(recs):
        ro = rd.Reader(data).rollup(group, red)
        m = rm.rollup(recs, group, red)
        _compare(ro, m)
        assert m["keys"] == sorted(set(m["keys"])) and 1 < len(m["keys"]) < len(recs)
        assert ro.groups() == rm.groups_of(m, 0)
        assert sum(m["nbad"]) > 0
        with pytest.raises(MergeError):
            ro.write_file()


# ---------------------------------------------------------------- 7. the merged view
@functools.lru_cache(maxsize=None)
def _merge_case(encoding):
    """three sources that share keys, values of three fields; sources 0 and 2 hold the empty key"""
    import merger_model as mm
    from mtblx import Reduce
    red = Reduce("sum", "min", "max", encoding=encoding)
    rng = np.random.default_rng(5 + len(encoding))
    pool = sorted({b"%c%c.%03d" % (97 + int(a), 97 + int(b), int(c))
                   for a, b, c in zip(rng.integers(0, 4, 900), rng.integers(0, 5, 900), rng.integers(0, 400, 900))})
    lists = []
    for s in range(3):
        idx = np.sort(rng.choice(len(pool), size=350, replace=False))
        lst = [(pool[i], v) for i, v in zip(idx, _values(rng, 350, red, bad=0.0))]
        if s != 1:
            lst.insert(0, (b"", red.encode([1, 2, 3])))
        lists.append(lst)
    datas = [mm.make_source(r, 512, 4) for r in lists]
    qs = [("from", b""), ("prefix", b""), ("prefix", b"a"), ("prefix", b"bc."), ("range", b"ab", b"cd.1"),
          ("range", b"", b""), ("get", b""), ("get", pool[7]), ("get", b"zz"), ("from", b"cc"), ("prefix", b"dd.39"),
          ("range", b"b", b"a"), ("from", b"\xff")]
    return red, lists, datas, qs


def _merger(datas, merge):
    rd = _mods()
    from mtblx import merger
    return merger.Merger.builder(merge).extend([rd.Reader(d) for d in datas]).build()


@pytest.mark.parametrize("encoding", ["u64le", "varint"])
def test_merger_rollup(oracle, encoding):
    import merger_model as mm
    from mtblx import GroupBy
    red, lists, datas, qs = _merge_case(encoding)
    merged = mm.merge_iter(lists, red.host)
    assert merged[0][0] != b"" and sum(len(x) for x in lists) > len(merged) + 100    # the quirk; shared keys
    for group in (GroupBy.delimiter(0x2e), GroupBy.length(1)):
        ro = _merger(datas, red).rollup(group)               # reduce=None: the Merger's Reduce
        m = rm.rollup(merged, group, red)
        _compare(ro, m)
        assert max(m["nrec"]) > 20 and m["keys"] == sorted(set(m["keys"]))
        ro.check()
    # another spec over another merge function: "first" picks, a max of field 0 folds
    from mtblx import Reduce
    r1 = Reduce("max", "max", "max", encoding=encoding)
    first = msu.merged(msu.promised_groups(lists), msu.PICK["first"])     # the lowest-numbered source's value
    _compare(_merger(datas, "first").rollup(GroupBy.length(2), r1), rm.rollup(first, GroupBy.length(2), r1))


@pytest.mark.parametrize("encoding", ["u64le", "varint"])
def test_merger_rollup_batch(oracle, encoding):
    from mtblx import GroupBy
    red, lists, datas, qs = _merge_case(encoding)
    group = GroupBy.delimiter(0x2e)
    exps = []
    for q in qs:
        groups = msu.promised_groups(msu.per_source(oracle, datas, q, ("rollup-merge", encoding)))
        exps.append(msu.merged(groups, lambda vs: red.host(b"", vs)))
    assert exps[6] == [(b"", lists[2][0][1])] and exps[0][0][0] != b""          # the empty-key quirk, per query
    assert any(not e for e in exps)
    wide = _merger(datas, red).rollup_batch(qs, group, max_blocks=1 << 20)
    narrow = _merger(datas, red).rollup_batch(qs, group, max_blocks=1)
    assert all(wide.served_by_kernel(q) for q in range(len(qs)))
    assert 0 < sum(not narrow.served_by_kernel(q) for q in range(len(qs))) < len(qs)
    for q, e in enumerate(exps):
        want = rm.groups_of(rm.rollup(e, group, red), 0)
        assert wide.groups(q) == want, qs[q]
        assert narrow.groups(q) == want, qs[q]
    flat = [r for e in exps for r in e]
    _compare(wide, rm.rollup(flat, group, red, [0] + np.cumsum([len(e) for e in exps]).tolist()))
    wide.check()
    narrow.check()


def test_merger_rollup_refuses():
    from mtblx import GroupBy
    red, lists, datas, qs = _merge_case("u64le")
    g = GroupBy.length(1)
    with pytest.raises(ValueError, match="callable"):
        _merger(datas, lambda k, vs: vs[0]).rollup(g, red)
    with pytest.raises(ValueError, match="callable"):
        _merger(datas, lambda k, vs: vs[0]).rollup_batch(qs, g, red)
    with pytest.raises(ValueError, match="Reduce"):
        _merger(datas, "concat").rollup(g)
    with pytest.raises(ValueError, match="GroupBy"):
        _merger(datas, red).rollup(("length", 1))
    with pytest.raises(ValueError, match="bad query"):
        _merger(datas, red).rollup_batch([("between", b"a")], g)


# ---------------------------------------------------------------- 8. the round trip
@pytest.mark.parametrize("compression", [0, 1], ids=["none", "snappy"])
@pytest.mark.parametrize("encoding", ["u64le", "varint"])
def test_write_file_round_trip(oracle, encoding, compression):
    from mtblx import GroupBy
    red, lists, datas, _ = _merge_case(encoding)
    group = GroupBy.delimiter(0x2e)
    rd = _mods()
    ro = rd.Reader(datas[1]).rollup(group, red)
    m = rm.rollup(lists[1], group, red)
    _compare(ro, m)
    out = ro.write_file(block_size=1024, restart_interval=4, compression=compression)
    back = oracle.file_scan(out.cpu().numpy().tobytes())
    assert back["end"] == 0 and back["records"] == list(zip(m["keys"], m["values"]))
    assert len(back["records"]) > 10
    # the rolled-up file is a source like any other: rolling it up again by a shorter prefix folds the partials
    again = rd.Reader(out.cpu().numpy().tobytes()).rollup(GroupBy.length(1), red)
    _compare(again, rm.rollup(list(zip(m["keys"], m["values"])), GroupBy.length(1), red))
    assert [f for _, f, _, _ in again.groups()] == rm.rollup(lists[1], GroupBy.length(1), red)["fields"]


# ---------------------------------------------------------------- 9. streams
@pytest.fixture(scope="module")
def stream_case():
    """the three surfaces run once unheld (which also loads their kernels before any hold, as
    stream_util's docstring asks) -> what the held runs must give"""
    import stream_util as S
    from mtblx import GroupBy
    rd = _mods()
    T, n, recs, red = _seg_case()
    seg = [0, 0, 100, T, 2 * T + 9, n, n]
    _roll(recs, GroupBy.length(7), red, seg)
    data, frecs, qs, fred = _file_case("snappy")
    qs = qs[:48]
    group = GroupBy.length(2)
    rb = rd.Reader(data).rollup_batch(qs, group, fred, max_blocks=2)
    assert 0 < sum(not rb.served_by_kernel(q) for q in range(len(qs))) < len(qs)
    want_r = [rb.groups(q) for q in range(len(qs))]
    mred, lists, datas, _ = _merge_case("varint")
    _merger(datas, mred).rollup(GroupBy.delimiter(0x2e))
    return dict(recs=recs, red=red, seg=seg, data=data, qs=qs, fred=fred, group=group, want_r=want_r, mred=mred,
                lists=lists, datas=datas, streams=S.pick_streams(2))


@pytest.mark.parametrize("config", ["current-held", "own-held", "ambient"])
def test_streams_rollup_records(stream_case, config):
    import stream_util as S
    from mtblx import GroupBy, rollup_records
    c = stream_case
    rec = _device_records(c["recs"])
    s = c["streams"][1]
    ro = S.run(config, lambda st: rollup_records(rec, GroupBy.length(7), c["red"], c["seg"], stream=st), s)
    m = rm.rollup(c["recs"], ("length", 7), c["red"], c["seg"])
    assert ro.groups(3) == rm.groups_of(m, 3)               # the result's own read-back, on its stream
    _compare(ro, m, s)


@pytest.mark.parametrize("config", ["current-held", "own-held", "ambient"])
def test_streams_reader_rollup_batch(stream_case, config):
    import stream_util as S
    rd = _mods()
    c = stream_case
    r = rd.Reader(c["data"])
    r.index_regular()          # mtblx_entry_offsets: the documented exception, before the hold
    s = c["streams"][0]
    rb = S.run(config, lambda st: r.rollup_batch(c["qs"], c["group"], c["fred"], max_blocks=2, stream=st), s)
    assert [rb.groups(q) for q in range(len(c["qs"]))] == c["want_r"]


@pytest.mark.parametrize("config", ["current-held", "own-held", "ambient"])
def test_streams_merger_rollup(stream_case, config):
    import merger_model as mm
    import stream_util as S
    from mtblx import GroupBy, merger
    rd = _mods()
    c = stream_case
    readers = []
    for d in c["datas"]:
        r = rd.Reader(d)
        r.index_regular()
        readers.append(r)
    s = c["streams"][0]
    group = GroupBy.delimiter(0x2e)
    ro = S.run(config, lambda st: merger.Merger(readers, c["mred"]).rollup(group, stream=st), s)
    _compare(ro, rm.rollup(mm.merge_iter(c["lists"], c["mred"].host), group, c["mred"]), s)


# ---------------------------------------------------------------- 10. above 4 GiB
def test_rollup_above_4gib():
    """two giant keys and two giant values first: every small key and value starts above 2^32 in its
    buffer.  GroupBy.length(8): the giants' group keys are their first 8 bytes; their values are bad"""
    import torch
    from mtblx import GroupBy, rollup_records
    from mtblx.encode import DeviceRecords
    from test_line4g_gpu import GIANT, _fill_giant
    _mods()
    free, _ = torch.cuda.mem_get_info()
    if free < (24 << 30):
        pytest.skip(f"{free >> 30} GiB of device memory free, this test wants 24")
    red = _red(3)
    rng = np.random.default_rng(12)
    small = [(b"k%04d/%05d" % (i // 9, i), v) for i, v in enumerate(_values(rng, 3000, red))]
    kblob, vblob = b"".join(k for k, _ in small), b"".join(v for _, v in small)
    keys = torch.empty(2 * GIANT + len(kblob), dtype=torch.uint8, device="cuda")
    vals = torch.empty(2 * GIANT + len(vblob), dtype=torch.uint8, device="cuda")
    for g in range(2):
        _fill_giant(keys[g * GIANT: (g + 1) * GIANT], 3 + 2 * g)
        _fill_giant(vals[g * GIANT: (g + 1) * GIANT], 7 + 2 * g)
    keys[2 * GIANT:].copy_(torch.frombuffer(bytearray(kblob), dtype=torch.uint8))
    vals[2 * GIANT:].copy_(torch.frombuffer(bytearray(vblob), dtype=torch.uint8))
    ke = torch.from_numpy(np.concatenate([[GIANT, 2 * GIANT], 2 * GIANT + _ends([k for k, _ in small])])).cuda()
    ve = torch.from_numpy(np.concatenate([[GIANT, 2 * GIANT], 2 * GIANT + _ends([v for _, v in small])])).cuda()
    assert int(ke[1]) > 1 << 32 and int(ve[1]) > 1 << 32
    # the model sees the giants through stand-ins with the same first 8 bytes and a bad value
    head = [b"".join(((j + 1) * mul).to_bytes(4, "little") for j in range(2)) for mul in (3, 5)]
    assert keys[:8].cpu().numpy().tobytes() == head[0] and keys[GIANT: GIANT + 8].cpu().numpy().tobytes() == head[1]
    model = [(head[0] + b"<giant>", b"bad"), (head[1] + b"<giant>", b"bad")] + small
    seg = [0, 1, 2, 1500, 3002]
    m = rm.rollup(model, ("length", 8), red, seg)
    assert m["keys"][:2] == head and m["nbad"][:2] == [1, 1] and m["grp_rec"][:3] == [0, 1, 2]
    ro = rollup_records(DeviceRecords(keys, ke, vals, ve), GroupBy.length(8), red, seg)
    _compare(ro, m)
    del keys, vals, ro
    torch.cuda.empty_cache()

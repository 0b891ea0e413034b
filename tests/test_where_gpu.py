"""Value predicates on the GPU: filter_records (mtblx_where_plan / _emit) and the surfaces that sit on it.

Expected values never come from the code under test: they are tests/where_model.py (the host
definition, pinned by hand in tests/test_where.py) over the test's own record lists, over what the
oracle's iteration yields for a query, or over the Merger's model.  Every comparison is bit for bit:
keys, key_end, values, val_end, seg_end, seg_bad, src_idx and the totals."""
import ctypes as C
import functools

import numpy as np
import pytest

import where_model as wm

pytestmark = pytest.mark.gpu

M = (1 << 64) - 1
OPS = {1: ("sum",), 3: ("sum", "min", "max"), 8: ("sum", "min", "max", "max", "min", "sum", "sum", "min")}
PATTERNS = ("all", "none", "alternating", "tile-last", "next-tile-first")


def _mods():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mtblx import reader
    return reader


def _tile():
    _mods()
    import mtblx
    return int(mtblx.lib().mtblx_where_tile())


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


def _compare(f, m, stream=None):
    """a Filtered against the model, bit for bit"""
    import torch
    with torch.cuda.stream(stream):
        r = f.records
        got = dict(keys=r.keys.cpu().numpy().tobytes(), key_end=r.key_end.cpu().numpy(),
                   vals=r.vals.cpu().numpy().tobytes(), val_end=r.val_end.cpu().numpy(),
                   src_idx=f.src_idx.cpu().numpy(), seg_end=f.seg_end.cpu().numpy(), seg_bad=f.seg_bad.cpu().numpy())
    keys, vals = [k for k, _ in m["records"]], [v for _, v in m["records"]]
    assert [f.nkept, len(got["keys"]), len(got["vals"]), f.nbad, f.nrejected] == m["totals"]
    assert got["src_idx"].tolist() == m["src_idx"]
    assert got["key_end"].tolist() == _ends(keys).tolist()
    assert got["keys"] == b"".join(keys)
    assert got["val_end"].tolist() == _ends(vals).tolist()
    assert got["vals"] == b"".join(vals)
    assert got["seg_end"].tolist() == m["seg_end"]
    assert got["seg_bad"].tolist() == m["seg_bad"]
    assert r.stream is f._stream and r.n == f.nkept


def _filter(recs, where, seg_off=None, lead=0, stream=None):
    from mtblx import filter_records
    f = filter_records(_device_records(recs, lead), where, seg_off, stream)
    m = wm.filter_records(recs, where, seg_off)
    _compare(f, m)
    return f, m


def _u64(*xs):
    return b"".join((x & M).to_bytes(8, "little") for x in xs)


def _spoil(rng, v):
    """a value made bad as tests/test_rollup_gpu.py's _values makes them (the last shape stays 8 * F
    bytes long: bad as varints, another well-formed value as u64le)"""
    return [v[:-1], v + b"\x00", b"", v[:-1] + b"\x80"][int(rng.integers(0, 4))]


def _values(rng, n, red, bad=0.03):
    """n values of `red`'s shape: random u64 fields, bit 63 set in a third; about `bad` of them bad"""
    F = len(red.ops)
    out = []
    for _ in range(n):
        w = [int(x) for x in rng.integers(0, 1 << 62, F, dtype=np.uint64)]
        w = [x | (1 << 63) if rng.random() < 0.33 else x >> int(rng.integers(0, 62)) for x in w]
        v = red.encode(w)
        out.append(_spoil(rng, v) if rng.random() < bad else v)
    return out


def _keys(rng, n):
    """n keys of 0 to 40 bytes in no order (a filter does not look at them); empty ones among them"""
    return [bytes(rng.integers(0, 256, int(rng.integers(0, 41)) if rng.random() > 0.05 else 0, dtype=np.uint8))
            for _ in range(n)]


# ---------------------------------------------------------------- 1. the grid
LO, HI = 1000, 1 << 40                 # the kept band of field 0


def _patterned(rng, n, red, pattern, T, bad=0.03):
    """values whose field 0 lies in [LO, HI] exactly where `pattern` keeps the record"""
    F = len(red.ops)
    want = {"all": lambda i: True, "none": lambda i: False, "alternating": lambda i: i % 2 == 0,
            "tile-last": lambda i: i % T == T - 1, "next-tile-first": lambda i: i % T == 0 and i > 0}[pattern]
    out = []
    for i in range(n):
        w = [int(x) >> int(rng.integers(0, 62)) for x in rng.integers(0, 1 << 62, F, dtype=np.uint64)]
        if want(i):
            w[0] = int(rng.integers(LO, HI + 1)) if rng.random() > 0.2 else (LO if rng.random() < 0.5 else HI)
        else:
            w[0] = [int(rng.integers(0, LO)), LO - 1, HI + 1, int(rng.integers(HI + 1, 1 << 63)) | (1 << 63)][i % 4]
        v = red.encode(w)
        out.append(_spoil(rng, v) if rng.random() < bad else v)
    if bad and n >= 8:
        out[n // 3] = b""                                  # an empty value, whatever the draws gave
    return out


@pytest.mark.parametrize("encoding", ["u64le", "varint"])
@pytest.mark.parametrize("F", [1, 3, 8])
@pytest.mark.parametrize("nname", ["0", "1", "T-1", "T", "T+1", "2T+1"])
def test_grid(nname, F, encoding):
    from mtblx import Where
    T = _tile()
    n = {"0": 0, "1": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+1": 2 * T + 1}[nname]
    red = _red(F, encoding)
    w = Where.like(red, [(0, LO, HI)])
    for pi, pattern in enumerate(PATTERNS):
        rng = np.random.default_rng(1000 * n + 10 * F + pi)
        recs = list(zip(_keys(rng, n), _patterned(rng, n, red, pattern, T)))
        lead = 3 if pi % 2 else 0                          # the buffers start 3 bytes into their allocation
        f, m = _filter(recs, w, None if pi % 2 else [0, n], lead)
        kept, _, _, nbad, nrej = m["totals"]
        # the inputs hold the pattern they are named for (the spoilt values apart: about 3 %)
        assert kept + nbad + nrej == n
        if pattern == "all":
            assert kept >= 0.9 * n - 2
        elif pattern == "none":
            assert kept == 0
        elif pattern == "alternating":
            assert abs(kept - (n + 1) // 2) <= 0.06 * n + 2 and all(i % 2 == 0 for i in m["src_idx"])
        elif pattern == "tile-last":
            assert set(m["src_idx"]) <= {T - 1, 2 * T - 1} and kept <= n // T
        else:
            assert set(m["src_idx"]) <= {T, 2 * T} and kept <= max(n - 1, 0) // T
        if n >= T:
            assert nbad > 0 and any(k == b"" for k, _ in recs) and any(v == b"" for _, v in recs)


def test_grid_edges_are_kept():
    """the two single-record patterns with clean values: exactly the record at the tile's edge comes out"""
    from mtblx import Where
    T = _tile()
    red = _red(3)
    w = Where.like(red, [(0, LO, HI)])
    rng = np.random.default_rng(3)
    for pattern, idx in (("tile-last", [T - 1, 2 * T - 1]), ("next-tile-first", [T, 2 * T])):
        recs = list(zip(_keys(rng, 2 * T + 1), _patterned(rng, 2 * T + 1, red, pattern, T, bad=0.0)))
        f, m = _filter(recs, w, [0, T - 1, T, T + 1, 2 * T + 1], lead=3)
        assert m["src_idx"] == idx
        assert m["seg_end"] == ([0, 1, 1, 2] if pattern == "tile-last" else [0, 0, 1, 2])


@pytest.mark.parametrize("mode", ["all", "any"])
@pytest.mark.parametrize("encoding", ["u64le", "varint"])
def test_clauses(encoding, mode):
    """every kind of clause at once over random fields: inside, outside, lo == hi, lo > hi, the ends"""
    from mtblx import Where
    T = _tile()
    red = _red(8, encoding)
    rng = np.random.default_rng(len(encoding) + len(mode))
    vals = _values(rng, T + 77, red)
    point = next(red.decode(v) for v in vals if red.decode(v) is not None)[2]
    if mode == "all":
        clauses = [(0, 1 << 20, 1 << 62), (1, 1 << 10, 1 << 63, "outside"), (4, 9, 3, "outside"), (5, None, None),
                   (7, 1 << 63, None)]
    else:
        clauses = [(0, 1 << 61, 1 << 62), (1, 1 << 2, 1 << 63, "outside"), (2, point, point), (3, 9, 3), (4, None, 0)]
    recs = list(zip(_keys(rng, len(vals)), vals))
    f, m = _filter(recs, Where.like(red, clauses, mode), lead=1)
    assert 0 < m["totals"][0] < len(recs) and m["totals"][3] > 0
    for w in (Where.like(red, [], mode), Where.like(red, [(3, 9, 3)], mode), Where.like(red, [(3, 9, 3, "outside")], mode)):
        f, m = _filter(recs, w)
    assert m["totals"][0] == len(recs) - m["totals"][3]     # the last: everything well-formed


# ---------------------------------------------------------------- 2. segments
@functools.lru_cache(maxsize=None)
def _seg_case():
    T = _tile()
    n = 3 * T + 5
    rng = np.random.default_rng(77)
    red = _red(3)
    recs = list(zip(_keys(rng, n), _patterned(rng, n, red, "alternating", T)))
    # a stretch of rejected records across a tile edge, so that some segment boundaries fall between kept ones
    for i in range(T - 20, T + 20):
        recs[i] = (recs[i][0], red.encode([0, 1, 2]))
    return T, n, recs, red


@pytest.mark.parametrize("shape", ["one", "empties", "tile-edges", "three-tiles", "thousand"])
def test_segments(shape):
    from mtblx import Where
    T, n, recs, red = _seg_case()
    rng = np.random.default_rng(len(shape))
    if shape == "one":
        seg = [0, n]
    elif shape == "empties":                                  # at the front, in the middle and at the end
        seg = [0, 0, 0, 100, 100, 100, T + 3, T + 3, n, n, n]
    elif shape == "tile-edges":
        seg = [0, T, 2 * T, 3 * T, n]
    elif shape == "three-tiles":
        seg = [0, T - 1, 3 * T + 1, n]
    else:
        sizes = rng.integers(0, 4, 1000)
        seg = [0] + np.cumsum(sizes).tolist()
        recs = recs[: seg[-1]]
        assert seg[-1] > T and len(seg) == 1001
    w = Where.like(red, [(0, LO, HI)])
    for lead in (0, 3):
        f, m = _filter(recs, w, seg, lead)
    assert sum(m["seg_bad"]) == m["totals"][3] > 0 and m["seg_end"][-1] == m["totals"][0]
    if shape == "empties":
        assert m["seg_end"][0] == m["seg_end"][1] == 0 and m["seg_end"][3] == m["seg_end"][4]
        assert m["seg_end"][-1] == m["seg_end"][-2] == m["seg_end"][-3]
    fo = f.seg_off().cpu().numpy().tolist()
    assert fo == [0] + m["seg_end"]


# ---------------------------------------------------------------- 3. long keys and values
def test_long_key_between_short_ones():
    from mtblx import Where
    red = _red(1)
    rng = np.random.default_rng(70000)
    long = bytes(rng.integers(0, 256, 70000, dtype=np.uint8))
    good, drop = red.encode([LO]), red.encode([0])
    recs = [(b"a", good), (b"bb", drop), (long, good), (b"c", drop), (b"dd", good), (long[:5000], drop), (b"e", good)]
    w = Where.like(red, [(0, LO, HI)])
    for lead in (0, 3, 16):
        f, m = _filter(recs, w, [0, 3, 7], lead)
    assert m["src_idx"] == [0, 2, 4, 6] and m["totals"][1] == 70004
    # the long key first, last, and next to a kept neighbour: one run of two records
    for order in ([2, 0, 1], [0, 1, 2], [0, 2, 4, 6, 1]):
        f, m = _filter([recs[i] for i in order], w, None, 5)
    assert m["totals"][0] == 4


def test_long_value_is_bad():
    from mtblx import Where
    rng = np.random.default_rng(300000)
    long = bytes(rng.integers(0, 256, 300000, dtype=np.uint8))
    for encoding in ("u64le", "varint"):
        red = _red(3, encoding)
        good = red.encode([LO, 1, 2])
        recs = [(b"a", good), (b"long", long), (b"b", good), (b"c", long[:81]), (b"d", good)]
        f, m = _filter(recs, Where.like(red, [(0, LO, HI)]), [0, 2, 5], 3)
        assert m["src_idx"] == [0, 2, 4] and m["totals"][3] == 2 and m["seg_bad"] == [1, 1]


# ---------------------------------------------------------------- 4. the C calls: flags, capacities, guards
GUARD = 64


def _raw(rec, where, seg=None, short=None, plan=True, src_idx=True):
    """the two C calls over outputs of exactly the planned size, each between two guards -> (rc of the
    plan, totals, rc of the emit, flags, outputs unchanged?, guards intact?, the outputs).  short: the
    name of the one capacity that is one byte or one record too small"""
    import torch
    from mtblx import _lib, codec
    L = _lib.lib()
    n = rec.n
    r = _lib.Records(codec._u(rec.keys), codec._u(rec.key_end), codec._u(rec.vals), codec._u(rec.val_end), n)
    nseg = len(seg) - 1 if seg is not None else 0
    wsb = int(L.mtblx_where_workspace_bytes(n, nseg))
    ws = torch.zeros(wsb, dtype=torch.uint8, device="cuda")
    totals = (C.c_uint64 * 6)(*([0x11] * 6))
    segt = torch.tensor(seg if seg is not None else [0], dtype=torch.int64, device="cuda")
    seg_end = torch.full((2 * max(nseg, 1),), 0x7777, dtype=torch.int64, device="cuda")
    spec = where.cstruct()
    rcp = None
    if plan:
        rcp = L.mtblx_where_plan(C.byref(r), C.byref(spec), C.c_void_p(segt.data_ptr()) if nseg else None, nseg, totals,
                                 C.c_void_p(seg_end.data_ptr()) if nseg else None,
                                 C.c_void_p(seg_end.data_ptr() + 8 * nseg) if nseg else None, C.c_void_p(ws.data_ptr()),
                                 wsb, None)
    K, kb, vb = (int(totals[i]) for i in range(3)) if plan and rcp == 0 else (n, 1 << 12, 1 << 12)
    size = dict(keys=kb, vals=vb, key_end=8 * K, val_end=8 * K, src_idx=8 * K)
    bufs = {name: torch.full((2 * GUARD + sz,), 0x5c, dtype=torch.uint8, device="cuda") for name, sz in size.items()}
    flags = torch.full((2,), 0x33, dtype=torch.int32, device="cuda")
    p = {name: b.data_ptr() + GUARD for name, b in bufs.items()}
    out = _lib.Filtered(keys=p["keys"], keys_cap=kb - (short == "keys"), vals=p["vals"], vals_cap=vb - (short == "vals"),
                        key_end=p["key_end"], val_end=p["val_end"], src_idx=p["src_idx"] if src_idx else None,
                        rec_cap=K - (short == "rec"), flags=flags.data_ptr())
    rce = L.mtblx_where_emit(C.byref(r), C.byref(out), C.c_void_p(ws.data_ptr()), wsb, None)
    torch.cuda.synchronize()
    same = all(bool((b == 0x5c).all()) for b in bufs.values())
    guards = all(bool((b[:GUARD] == 0x5c).all() and (b[GUARD + size[name]:] == 0x5c).all()) for name, b in bufs.items())
    body = {name: b[GUARD: GUARD + size[name]].cpu().numpy() for name, b in bufs.items()}
    return rcp, [int(x) for x in totals], rce, flags.tolist(), same, guards, body, seg_end.cpu().numpy().tolist()


def _raw_case():
    T, n, recs, red = _seg_case()
    from mtblx import Where
    recs = recs[:2000]
    return recs, _device_records(recs, 3), Where.like(red, [(0, LO, HI)])


def test_emit_writes_exactly_the_planned_sizes():
    from mtblx import _lib
    recs, rec, w = _raw_case()
    seg = [0, 700, 900, 2000]
    m = wm.filter_records(recs, w, seg)
    rcp, totals, rce, flags, same, guards, body, segs = _raw(rec, w, seg)
    assert rcp == 0 and totals == m["totals"] + [0] and rce == 0 and flags == [0, 0x33] and not same and guards
    assert body["keys"].tobytes() == b"".join(k for k, _ in m["records"])
    assert body["vals"].tobytes() == b"".join(v for _, v in m["records"])
    assert body["src_idx"].view(np.int64).tolist() == m["src_idx"]
    assert segs == m["seg_end"] + m["seg_bad"]
    rcp, totals, rce, flags, same, guards, body, _ = _raw(rec, w, None, src_idx=False)     # no segments, no src_idx
    assert rcp == 0 and totals == m["totals"] + [0] and flags == [0, 0x33] and guards
    assert (body["src_idx"] == 0x5c).all() and body["key_end"].view(np.int64).tolist() == \
        _ends([k for k, _ in m["records"]]).tolist()
    for short in ("keys", "vals", "rec"):
        rcp, _, rce, flags, same, guards, _, _ = _raw(rec, w, seg, short=short)
        assert rcp == 0 and rce == 0 and flags == [_lib.WHERE_OVERFLOW, 0x33] and same and guards, short


def test_emit_refuses_an_unplanned_workspace():
    from mtblx import _lib
    recs, rec, w = _raw_case()
    _, _, rce, flags, same, guards, _, _ = _raw(rec, w, [0, 2000], plan=False)             # a zeroed workspace
    assert rce == 0 and flags == [_lib.WHERE_NOT_PLANNED, 0x33] and same and guards
    # a workspace another call has planned: the rollup's mark is not the filter's
    import torch
    from mtblx import GroupBy, codec
    L = _lib.lib()
    r = rec.cstruct()
    wsb = max(int(L.mtblx_where_workspace_bytes(rec.n, 1)), int(L.mtblx_rollup_workspace_bytes(rec.n, 1)))
    ws = torch.zeros(wsb, dtype=torch.uint8, device="cuda")
    tot = torch.zeros(2, dtype=torch.int64, device="cuda")
    g = GroupBy.length(2).cstruct()
    assert L.mtblx_rollup_plan(C.byref(r), C.byref(g), None, 0, C.c_void_p(tot.data_ptr()), C.c_void_p(ws.data_ptr()),
                               wsb, None) == 0
    buf = torch.full((1 << 16,), 0x5c, dtype=torch.uint8, device="cuda")
    flags = torch.full((2,), 0x33, dtype=torch.int32, device="cuda")
    p = buf.data_ptr()
    out = _lib.Filtered(keys=p, keys_cap=1 << 12, vals=p + (1 << 12), vals_cap=1 << 12, key_end=p + (2 << 12),
                        val_end=p + (3 << 12), src_idx=None, rec_cap=64, flags=flags.data_ptr())
    assert L.mtblx_where_emit(C.byref(r), C.byref(out), C.c_void_p(ws.data_ptr()), wsb, None) == 0
    torch.cuda.synchronize()
    assert flags.tolist() == [_lib.WHERE_NOT_PLANNED, 0x33] and bool((buf == 0x5c).all())
    del codec


@pytest.mark.parametrize("seg", [[0, 900, 700, 2000], [0, 700, 900, 1999], [0, 700, 900, 2001], [1, 700, 900, 2000],
                                 [0, 1 << 40, 900, 2000]],
                         ids=["decreasing", "ends-before-n", "ends-after-n", "starts-after-0", "far-out"])
def test_bad_seg_off_writes_nothing(seg):
    from mtblx import _lib, filter_records
    recs, rec, w = _raw_case()
    with pytest.raises(ValueError, match="seg_off"):
        filter_records(rec, w, seg)
    rcp, totals, rce, flags, same, guards, _, segs = _raw(rec, w, seg)
    assert rcp == _lib.MTBLX_E_FORMAT and totals == [0, 0, 0, 0, 0, _lib.WHERE_BADSEG]
    assert rce == 0 and flags == [_lib.WHERE_BADSEG, 0x33] and same and guards and segs == [0x7777] * 6
    with pytest.raises(ValueError, match="seg_off"):
        filter_records(rec, w, [[0, 2000]])
    with pytest.raises(ValueError, match="no segment"):
        filter_records(rec, w, [0])


# ---------------------------------------------------------------- 5. files: the fused walk and the batched surfaces
FILES = {"plain": (1024, 4, 0), "snappy": (1024, 4, 1)}
DENSE = (256, 1, 0)                    # every index entry a restart: the irregular-index case corrupts one
BAND = (1 << 40, 1 << 62)              # field 0 of the file cases' predicate; the last field must not be tiny


@functools.lru_cache(maxsize=None)
def _file_case(name, encoding):
    """-> (data, records, queries, limits, Reduce, Where): 4000 random keys, values of 3 fields (3 % bad),
    scan_util's queries: all four kinds, max_records of 0, 1 and 37 (inside a block)"""
    import corpus
    import scan_util as su
    from mtblx import Where
    bs, iv, comp = DENSE if name == "dense" else FILES[name]
    red = _red(3, encoding)
    rng = np.random.default_rng(bs + iv + comp + len(encoding))
    keys = [k for k, _ in corpus.random_records(rng, 4000, 0, 30, 0, 0)]
    recs = list(zip(keys, _values(rng, len(keys), red)))
    qs, lim = su.queries_for(su.probe_keys(rng, recs, 18))
    w = Where.like(red, [(0, BAND[0], BAND[1]), (2, 1 << 8, None)])
    return su.write(recs, bs, iv, comp), recs, qs, lim, red, w


def _expected(oracle, name, encoding, verify=True):
    import scan_util as su
    data, _, qs, lim, _, _ = _file_case(name, encoding)
    return [su.expected(oracle, data, q, m, verify, tag=("where", name, encoding))["records"] for q, m in zip(qs, lim)]


def _fold_where(red, w, records):
    """what reduce_batch(where=) reports for a query that yields `records`: (fields, nrec, nbad, nmatch)"""
    vd = wm.verdicts(records, w)
    kept = [v for (_, v), x in zip(records, vd) if x is True]
    fields, nkept, none = red.fold(kept)
    assert none == 0 and nkept == len(kept)
    return fields, len(records), sum(1 for x in vd if x is None), len(kept)


def _check_reduce(rb, red, w, exps):
    nm = rb.nmatch.cpu().numpy()
    assert rb.nq == len(exps) == nm.size
    for i, e in enumerate(exps):
        assert (rb.values(i),) + rb.counts(i) + (int(nm[i]),) == _fold_where(red, w, e), i


@pytest.mark.parametrize("encoding", ["u64le", "varint"])
@pytest.mark.parametrize("name", list(FILES))
def test_reduce_batch_where(oracle, name, encoding):
    from mtblx import Where, _lib
    rd = _mods()
    data, recs, qs, lim, red, w = _file_case(name, encoding)
    exps = _expected(oracle, name, encoding)
    want = [_fold_where(red, w, e) for e in exps]
    assert any(x[2] for x in want) and any(0 < x[3] < x[1] - x[2] for x in want) and any(x[1] == 0 for x in want)
    assert {q[0] for q in qs} == {"from", "get", "prefix", "range"} and {0, 1, 37, None} <= set(lim)
    wide = rd.Reader(data).reduce_batch(qs, red, max_blocks=1 << 20, max_records=lim, where=w)
    assert wide.n_large == 0 and wide.n_fallback == 0
    _check_reduce(wide, red, w, exps)
    narrow = rd.Reader(data).reduce_batch(qs, red, max_blocks=1, max_records=lim, where=w)    # hands queries back
    assert 0 < narrow.n_large < len(qs) and narrow.n_fallback == 0
    _check_reduce(narrow, red, w, exps)
    # the counts of the plan do not see the predicate
    plain = rd.Reader(data).reduce_batch(qs, red, max_blocks=1 << 20, max_records=lim)
    assert plain.nmatch is None
    assert (wide.nrec.cpu() == plain.nrec.cpu()).all() and (wide.status.cpu() == plain.status.cpu()).all()
    assert (wide.nbad.cpu() == plain.nbad.cpu()).all()
    # no clause: everything well-formed is kept, the fold is the plain one
    for mb in (1 << 20, 1):
        free = rd.Reader(data).reduce_batch(qs, red, max_blocks=mb, max_records=lim, where=Where.like(red))
        assert (free.fields.cpu() == plain.fields.cpu()).all() and (free.nbad.cpu() == plain.nbad.cpu()).all()
        assert (free.nmatch.cpu() == plain.nrec.cpu() - plain.nbad.cpu()).all()
    # "any" without a clause keeps nothing: the identities
    none = rd.Reader(data).reduce_batch(qs[:40], red, max_records=lim[:40], where=Where.like(red, mode="any"))
    assert int(none.nmatch.sum()) == 0 and all(none.values(i) == red.identities() for i in range(40))
    assert (none.nbad.cpu() == plain.nbad.cpu()[:40]).all()
    del _lib


def test_reduce_batch_where_clause_kinds(oracle):
    """outside, lo == hi, lo > hi and "any" through the fused walk, F = 3 in both encodings"""
    from mtblx import Where
    rd = _mods()
    for encoding in ("u64le", "varint"):
        data, recs, qs, lim, red, _ = _file_case("plain", encoding)
        exps = _expected(oracle, "plain", encoding)
        point = next(red.decode(v) for _, v in recs if red.decode(v) is not None)[1]
        for w in (Where.like(red, [(0, BAND[0], BAND[1], "outside"), (1, 1 << 63, None)], "any"),
                  Where.like(red, [(1, point, point)]), Where.like(red, [(1, point, point, "outside"), (2, 9, 3)], "any"),
                  Where.like(red, [(2, 9, 3)]), Where.like(red, [(2, 9, 3, "outside"), (0, None, BAND[0])])):
            rb = rd.Reader(data).reduce_batch(qs[:150], red, max_records=lim[:150], where=w)
            _check_reduce(rb, red, w, exps[:150])


def test_reduce_batch_where_refuses():
    from mtblx import GroupBy, Reduce, Where
    rd = _mods()
    data, recs, qs, lim, red, w = _file_case("plain", "u64le")
    r = rd.Reader(data)
    for bad in (Where(2, [(0, 1, 2)]), Where(3, [(0, 1, 2)], encoding="varint")):
        with pytest.raises(ValueError, match="layout"):
            r.reduce_batch(qs[:4], red, where=bad)
    with pytest.raises(ValueError, match="Where"):
        r.reduce_batch(qs[:4], red, where=(0, 1, 2))
    with pytest.raises(ValueError, match="Where"):
        r.scan_batch(qs[:4], where="count > 5")
    with pytest.raises(ValueError, match="Where"):
        r.rollup_batch(qs[:4], GroupBy.length(2), Reduce("sum"), where=7)


def test_irregular_index(oracle):
    """an index block whose restart entries carry shared != 0: every query goes through the seek path,
    filter_records and reduce_segments"""
    import scan_util as su
    import test_seek_gpu as ts
    rd = _mods()
    data, recs, qs, lim, red, w = _file_case("dense", "u64le")
    rng = np.random.default_rng(12)
    seen = 0
    for _ in range(6):
        bad = ts._corrupt_index(data, rng, "restart")
        try:
            r = rd.ReaderBuilder().verify_checksums(False).read(bad)
        except (rd.MtblError, rd.ReferencePanic):
            continue
        if r.index_regular():
            continue
        seen += 1
        rb = r.reduce_batch(qs[:45], red, max_records=lim[:45], where=w)
        sb = r.scan_batch(qs[:45], max_records=lim[:45], where=w)
        assert rb.n_fallback == 45 and not any(rb.served_by_kernel(i) for i in range(45))
        exps = [su.expected(oracle, bad, q, m, False)["records"] for q, m in zip(qs[:45], lim[:45])]
        _check_reduce(rb, red, w, exps)
        for i, e in enumerate(exps):
            assert sb.records(i) == wm.filter_records(e, w)["records"]
        break
    assert seen


@pytest.mark.parametrize("name", list(FILES))
def test_scan_batch_where(oracle, name):
    rd = _mods()
    data, recs, qs, lim, red, w = _file_case(name, "varint")
    exps = _expected(oracle, name, "varint")
    models = [wm.filter_records(e, w) for e in exps]
    for mb in (1 << 20, 1):
        sb = rd.Reader(data).scan_batch(qs, max_blocks=mb, max_records=lim, where=w)
        assert (sb.n_large > 0) == (mb == 1)
        nbad = sb.nbad.cpu().numpy()
        for i, m in enumerate(models):
            assert sb.records(i) == m["records"], (i, qs[i], lim[i])          # max_records cuts before the filter
            assert sb.scan(i).records() == m["records"] and sb.scan(i).nrec == m["totals"][0]
            assert int(nbad[i]) == m["totals"][3]
        if mb > 1:   # the kernel path's buffers are one mtblx_records whose segments are the queries
            flat = [r for m in models for r in m["records"]]
            assert sb.keys.cpu().numpy().tobytes() == b"".join(k for k, _ in flat)
            assert sb.val_end.cpu().numpy().tolist() == _ends([v for _, v in flat]).tolist()
            assert sb.rec_off.cpu().numpy().tolist() == [0] + np.cumsum([m["totals"][0] for m in models]).tolist()
    assert any(m["totals"][0] for m in models) and any(m["totals"][4] for m in models)


def test_rollup_where(oracle):
    """Reader.rollup_batch(where=), Reader.rollup(where=) and rollup_records(where=): the kept records rolled up"""
    import rollup_model as rm
    import test_rollup_gpu as trg
    from mtblx import GroupBy, rollup_records
    rd = _mods()
    data, recs, qs, lim, red, w = _file_case("plain", "u64le")
    qs = [q for q, m in zip(qs, lim) if m is None][:120]                  # rollup_batch takes no limits
    import scan_util as su
    exps = [su.expected(oracle, data, q, None, True, tag=("where-rollup",))["records"] for q in qs]
    group = GroupBy.length(2)
    kept = [wm.filter_records(e, w)["records"] for e in exps]
    assert any(len(k) > 50 for k in kept) and any(len(k) < len(e) for k, e in zip(kept, exps))
    for mb in (1 << 20, 1):
        ro = rd.Reader(data).rollup_batch(qs, group, red, max_blocks=mb, where=w)
        assert (sum(not ro.served_by_kernel(q) for q in range(len(qs))) > 0) == (mb == 1)
        for q, k in enumerate(kept):
            assert ro.groups(q) == rm.groups_of(rm.rollup(k, group, red), 0), (q, qs[q])
        if mb > 1:
            flat = [r for k in kept for r in k]
            trg._compare(ro, rm.rollup(flat, group, red, [0] + np.cumsum([len(k) for k in kept]).tolist()))
    whole = wm.filter_records(recs, w)["records"]
    m = rm.rollup(whole, group, red)
    trg._compare(rd.Reader(data).rollup(group, red, where=w), m)
    assert sum(m["nbad"]) == 0 and sum(m["nrec"]) == len(whole) < len(recs)
    seg = [0, 0, 1500, 1500, 4000]
    mk = wm.filter_records(recs, w, seg)
    trg._compare(rollup_records(_device_records(recs, 3), group, red, seg, where=w),
                 rm.rollup(mk["records"], group, red, [0] + mk["seg_end"]))


@pytest.mark.parametrize("encoding", ["u64le", "varint"])
def test_having(encoding):
    """HAVING is a composition: a Rollup's values are encoded in its Reduce's layout, so filter_records
    over ro.records with seg_off = ro.seg_grp keeps groups, and src_idx gathers their side arrays"""
    import rollup_model as rm
    import torch
    from mtblx import GroupBy, Where, filter_records, rollup_records
    T = _tile()
    red = _red(3, encoding)
    rng = np.random.default_rng(len(encoding))
    n = 3 * T + 5
    keys = sorted({b"g%03d.%05d" % (int(g), i) for i, g in enumerate(rng.integers(0, 400, n))})
    recs = list(zip(keys, _values(rng, len(keys), red)))
    seg = [0, 0, 700, T, 2 * T + 9, len(recs), len(recs)]
    group = GroupBy.delimiter(0x2e)
    ro = rollup_records(_device_records(recs), group, red, seg)
    m = rm.rollup(recs, group, red, seg)
    counts = sorted(f[2] for f in m["fields"])
    having = Where.like(ro.reduce, [(2, counts[len(counts) // 2], None)])     # max(field 2) at least the median
    f = filter_records(ro.records, having, seg_off=ro.seg_grp)
    rolled = list(zip(m["keys"], m["values"]))
    mh = wm.filter_records(rolled, having, m["seg_grp"])
    _compare(f, mh)
    assert 0 < mh["totals"][0] < len(rolled) and mh["totals"][3] == 0        # a Rollup's values are never bad
    idx = torch.as_tensor(mh["src_idx"], device="cuda")
    assert (f.src_idx == idx).all()
    got = ro.fields[f.src_idx].cpu().numpy().view(np.uint64)
    assert [tuple(int(x) for x in row) for row in got] == [m["fields"][g] for g in mh["src_idx"]]
    assert ro.nrec[f.src_idx].cpu().tolist() == [m["nrec"][g] for g in mh["src_idx"]]
    assert all(fl[2] >= counts[len(counts) // 2] for fl in (m["fields"][g] for g in mh["src_idx"]))


# ---------------------------------------------------------------- 6. the merged view, the Sorter, files written
@pytest.mark.parametrize("encoding", ["u64le", "varint"])
def test_merger_write_file_where(oracle, encoding):
    """the predicate sees the MERGED value: after the Reduce, the empty-key quirk and the Select"""
    import merger_model as mm
    import scan_util as su
    import select_model as sm
    import test_rollup_gpu as trg
    from mtblx import Select, Where, merger
    rd = _mods()
    red, lists, datas, _ = trg._merge_case(encoding)
    merged = mm.merge_iter(lists, red.host)
    sums = sorted(red.decode(v)[0] for _, v in merged)
    w = Where.like(red, [(0, sums[len(sums) // 3], None)])                     # the SUM of the group, not a source's value
    single = [v for lst in lists for _, v in lst]
    kept = wm.filter_records(merged, w)["records"]
    assert 0 < len(kept) < len(merged)
    assert any(w.keeps(v) is True and v not in single for _, v in kept)       # kept only because it was merged
    got = trg._merger(datas, red).write_file(block_size=1024, restart_interval=4, where=w).cpu().numpy().tobytes()
    assert got == oracle.write_file(kept, 1024, 4) == su.write(kept, 1024, 4)
    assert trg._merger(datas, red).records(where=w).n == len(kept)
    # with a Select: the semi-join's groups, merged, then filtered
    sel = Select(require=[0, 2])
    chosen = sm.select_merge(lists, sel, red.host)
    kept = wm.filter_records(chosen, w)["records"]
    assert 0 < len(kept) < len(chosen) < len(merged)
    mg = merger.Merger.builder(red).extend([rd.Reader(d) for d in datas]).select(sel).build()
    got = mg.write_file(block_size=512, restart_interval=16, where=w).cpu().numpy().tobytes()
    assert got == oracle.write_file(kept, 512, 16) == su.write(kept, 512, 16)
    with pytest.raises(ValueError, match="Where"):
        trg._merger(datas, red).write_file(where="sum > 3")


def test_sorter_write_file_where(oracle):
    import scan_util as su
    import sorter_model as som
    from mtblx import Where, sorter
    _mods()
    red = _red(3)
    rng = np.random.default_rng(31)
    pool = [b"key-%04d" % i for i in range(700)]
    recs = [(pool[int(rng.integers(0, len(pool)))], v) for v in _values(rng, 2500, red, bad=0.0)]
    model, _ = som.run(recs, red.host)
    sums = sorted(red.decode(v)[0] for _, v in model)
    w = Where.like(red, [(0, None, sums[len(sums) // 2])])
    kept = wm.filter_records(model, w)["records"]
    assert 0 < len(kept) < len(model) < len(recs)
    s = sorter.Sorter(red)
    for k, v in recs:
        s.insert(k, v)
    got = s.write_file(1024, 16, where=w).cpu().numpy().tobytes()
    assert got == oracle.write_file(kept, 1024, 16) == su.write(kept, 1024, 16)
    s = sorter.Sorter(red)
    with pytest.raises(ValueError, match="Where"):
        s.records(where=3)
    assert not s._done                                                        # the refusal did not consume it


def test_filter_file(oracle):
    import scan_util as su
    from mtblx import where as W
    rd = _mods()
    red = _red(3, "varint")
    rng = np.random.default_rng(8)
    keys = sorted({bytes(rng.integers(97, 123, int(rng.integers(1, 12)), dtype=np.uint8)) for _ in range(60)})
    recs = list(zip(keys, _values(rng, len(keys), red, bad=0.1)))
    data = su.write(recs, 512, 4)
    assert len(oracle.index_records(data)) == 2                               # a two-block file
    w = W.Where.like(red, [(1, None, 1 << 50)])
    kept = wm.filter_records(recs, w)
    assert 0 < kept["totals"][0] < len(recs) and kept["totals"][3] > 0
    got = W.filter_file(rd.Reader(data), w, block_size=256, restart_interval=2).cpu().numpy().tobytes()
    assert got == oracle.write_file(kept["records"], 256, 2)
    assert W.filter_file(data, w, block_size=256, restart_interval=2).cpu().numpy().tobytes() == got
    assert oracle.file_scan(got)["records"] == kept["records"]
    none = W.filter_file(data, W.Where.like(red, mode="any")).cpu().numpy().tobytes()
    assert none == oracle.write_file([], 8192, 16)


# ---------------------------------------------------------------- 7. streams
@pytest.fixture(scope="module")
def stream_case(oracle):
    """both surfaces run once unheld (which also loads their kernels before any hold, as stream_util's
    docstring asks) -> what the held runs must give"""
    import stream_util as S
    rd = _mods()
    T, n, recs, red = _seg_case()
    from mtblx import Where
    w = Where.like(red, [(0, LO, HI)])
    seg = [0, 0, 100, T, 2 * T + 9, n, n]
    _filter(recs, w, seg)
    data, frecs, qs, lim, fred, fw = _file_case("snappy", "u64le")
    qs, lim = qs[:48], lim[:48]
    rb = rd.Reader(data).reduce_batch(qs, fred, max_blocks=2, max_records=lim, where=fw)
    assert 0 < rb.n_large < len(qs)
    exps = _expected(oracle, "snappy", "u64le")[:48]
    return dict(recs=recs, w=w, seg=seg, data=data, qs=qs, lim=lim, fred=fred, fw=fw, exps=exps,
                streams=S.pick_streams(2))


@pytest.mark.parametrize("config", ["current-held", "own-held", "ambient"])
def test_streams_filter_records(stream_case, config):
    import stream_util as S
    from mtblx import filter_records
    c = stream_case
    rec = _device_records(c["recs"])
    s = c["streams"][1]
    f = S.run(config, lambda st: filter_records(rec, c["w"], c["seg"], stream=st), s)
    _compare(f, wm.filter_records(c["recs"], c["w"], c["seg"]), s)


@pytest.mark.parametrize("config", ["current-held", "own-held", "ambient"])
def test_streams_reduce_batch_where(stream_case, config):
    import stream_util as S
    rd = _mods()
    c = stream_case
    r = rd.Reader(c["data"])
    r.index_regular()          # mtblx_entry_offsets: the documented exception, before the hold
    s = c["streams"][0]
    rb = S.run(config, lambda st: r.reduce_batch(c["qs"], c["fred"], max_blocks=2, max_records=c["lim"], where=c["fw"],
                                                 stream=st), s)
    nm = S.host(rb.nmatch, s)
    for i, e in enumerate(c["exps"]):
        assert (rb.values(i),) + rb.counts(i) + (int(nm[i]),) == _fold_where(c["fred"], c["fw"], e), i


# ---------------------------------------------------------------- 8. above 4 GiB
def test_filter_above_4gib():
    """two giant keys and two giant values first: every small key and value starts above 2^32 in its
    buffer, and a DECOY -- other keys, and values whose verdicts are the opposite -- lies at exactly
    those offsets minus 2^32: a position cut to 32 bits reads the decoy and the comparison fails"""
    import torch
    from mtblx import Where, filter_records
    from mtblx.encode import DeviceRecords
    from test_line4g_gpu import GIANT, _fill_giant
    _mods()
    free, _ = torch.cuda.mem_get_info()
    if free < (24 << 30):
        pytest.skip(f"{free >> 30} GiB of device memory free, this test wants 24")
    T = _tile()
    red = _red(3)
    w = Where.like(red, [(0, LO, HI)])
    rng = np.random.default_rng(12)
    n = T + 300
    small = list(zip(_keys(rng, n), _patterned(rng, n, red, "alternating", T, bad=0.0)))
    flipped = [red.encode([0 if w.keeps(v) else LO] + red.decode(v)[1:]) for _, v in small]
    assert all(len(a) == len(b[1]) and w.keeps(a) is not w.keeps(b[1]) for a, b in zip(flipped, small))
    kblob, vblob = b"".join(k for k, _ in small), b"".join(v for _, v in small)
    kdecoy, vdecoy = bytes(b ^ 0xFF for b in kblob), b"".join(flipped)
    keys = torch.empty(2 * GIANT + len(kblob), dtype=torch.uint8, device="cuda")
    vals = torch.empty(2 * GIANT + len(vblob), dtype=torch.uint8, device="cuda")
    for g in range(2):
        _fill_giant(keys[g * GIANT: (g + 1) * GIANT], 3 + 2 * g)
        _fill_giant(vals[g * GIANT: (g + 1) * GIANT], 7 + 2 * g)
    low = 2 * GIANT - (1 << 32)                             # where a 32-bit position lands: inside giant 0
    assert 0 < low and low + max(len(kblob), len(vblob)) < GIANT
    for buf, blob, decoy in ((keys, kblob, kdecoy), (vals, vblob, vdecoy)):
        buf[2 * GIANT:].copy_(torch.frombuffer(bytearray(blob), dtype=torch.uint8))
        buf[low: low + len(decoy)].copy_(torch.frombuffer(bytearray(decoy), dtype=torch.uint8))
    ke = torch.from_numpy(np.concatenate([[GIANT, 2 * GIANT], 2 * GIANT + _ends([k for k, _ in small])])).cuda()
    ve = torch.from_numpy(np.concatenate([[GIANT, 2 * GIANT], 2 * GIANT + _ends([v for _, v in small])])).cuda()
    assert int(ke[1]) > 1 << 32 and int(ve[1]) > 1 << 32
    # the model sees the giants through stand-ins: their values are bad, so their keys are never copied
    model = [(b"<giant key 0>", b"bad"), (b"<giant key 1>", b"bad")] + small
    seg = [0, 1, 2, 900, n + 2]
    m = wm.filter_records(model, w, seg)
    assert m["seg_bad"] == [1, 1, 0, 0] and m["src_idx"][0] == 2 and m["totals"][0] == (n + 1) // 2
    f = filter_records(DeviceRecords(keys, ke, vals, ve), w, seg)
    _compare(f, m)
    del keys, vals, f
    torch.cuda.empty_cache()

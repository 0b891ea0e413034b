"""Snappy files in the Reader on the GPU: the device stage (mtblx_stage_plan / mtblx_stage_emit)
through ctypes against the oracle's snappy decoder and the host stage, corrupt stored bytes with
verification on and off, the counters that show nothing is staged on the host, the on-demand
table of get_batch / scan_batch (mtblx_scan_touch, mtblx_bitmap_compact, mtblx_table_gather), the
full device-staged table of an irregular index, and a Merger over Snappy sources."""
import ctypes as C
import functools

import numpy as np
import pytest

import corpus

pytestmark = pytest.mark.gpu

PHRASES = [b"the quick brown fox ", b"jumps over the lazy dog ", b"lorem ipsum dolor sit amet ", b"0123456789abcdef",
           b"consectetur adipiscing elit ", b"sed do eiusmod tempor ", b"\x00\x01\x02\x03\x04\x05\x06\x07"]


def _mods():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mtblx
    from mtblx import _lib, reader
    return torch, mtblx, _lib, reader


def _write(recs, bs, iv=16, comp=1):
    from mtblx.writer import Writer
    w = Writer(bs, iv, comp)
    for k, v in recs:
        w.insert(k, v)
    data = bytes(w.into_inner())
    off, ln = w.block_dir
    return data, np.asarray(off, np.int64), np.asarray(ln, np.int64)


def _phrase_records(seed, n, vmin, vmax):
    """sorted random keys, values that repeat phrases from a small pool: blocks compress >= 2x"""
    rng = np.random.default_rng(seed)
    keys = [k for k, _ in corpus.random_records(rng, n, 4, 24, 0, 0)]
    out = []
    for k in keys:
        want = int(rng.integers(vmin, vmax + 1))
        v = b"".join(PHRASES[int(i)] for i in rng.integers(0, len(PHRASES), want // 12 + 1))[:want]
        out.append((k, v))
    return out


@functools.lru_cache(maxsize=None)
def _corpus(kind, bs):
    """records filling well over 65 blocks of `bs` bytes"""
    per = {1024: 200, 4096: 400, 65536: 2400}[bs]           # the longest value
    n = 90 * bs // (per // 2 + 14) + 50
    if kind == "random":
        return corpus.random_records(np.random.default_rng(bs), n, 4, 24, 0, per)
    return _phrase_records(bs + 1, n, 0, per)


@functools.lru_cache(maxsize=None)
def _full(kind, bs):
    data, off, ln = _write(_corpus(kind, bs), bs)
    assert len(off) >= 66, len(off)
    return data, off, ln


@functools.lru_cache(maxsize=None)
def _file(oracle_mod, kind, bs, nblk):
    """a Snappy file of exactly nblk data blocks: the Writer's cut of a prefix of the corpus"""
    recs = _corpus(kind, bs)
    data, off, ln = _full(kind, bs)
    if nblk is not None:
        ikeys = [k for k, _ in oracle_mod.index_records(data)]
        recs = [r for r in recs if r[0] <= ikeys[nblk - 1]] if nblk else []
        data, off, ln = _write(recs, bs)
        assert len(off) == nblk
    return data, off, ln, recs


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _stage(r, off, ln, st, bad=None, sel=None, base=0, by_ordinal=False):
    """mtblx_stage_plan + mtblx_stage_emit through ctypes -> dict of host arrays and the totals"""
    torch, mtblx, _lib, reader = _mods()
    L = _lib.lib()
    dev = r.file.device
    ndir = int(off.numel())
    n = int(sel.numel()) if sel is not None else ndir
    wsb = int(L.mtblx_stage_workspace_bytes(n))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    totals = (C.c_uint64 * 3)()
    rc = L.mtblx_stage_plan(_p(r.file), r.len, _p(off), _p(ln), _p(st), _p(bad), ndir, _p(sel),
                            n if sel is not None else 0, totals, _p(ws), wsb, None)
    assert rc == 0, rc
    total, mx, ncorrupt = (int(x) for x in totals)
    assert total % 16 == 0
    dst = torch.full((base + total + 64,), 0xEE, dtype=torch.uint8, device=dev)
    nrow = ndir if by_ordinal else n
    doff = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
    dlen = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    ts, tdo, tdl = (torch.full((max(nrow, 1),), -7, dtype=torch.int64, device=dev) for _ in range(3))
    tst = torch.full((max(nrow, 1),), -7, dtype=torch.int32, device=dev)
    rc = L.mtblx_stage_emit(_p(r.file), r.len, _p(off), ndir, _p(sel), n if sel is not None else 0, _p(dst),
                            base + total, base, total, mx, _p(doff), _p(dlen), _p(ts), _p(tdo), _p(tdl), _p(tst),
                            1 if by_ordinal else 0, _p(ws), wsb, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    h = dst.cpu().numpy()
    assert (h[:base] == 0xEE).all() and (h[base + total:] == 0xEE).all()      # nothing outside [base, base + total)
    return dict(dst=h, doff=doff[:n].cpu().numpy(), dlen=dlen[:n].cpu().numpy().view(np.uint32).astype(np.int64),
                ts=ts[:nrow].cpu().numpy(), tdo=tdo[:nrow].cpu().numpy(), tdl=tdl[:nrow].cpu().numpy(),
                tst=tst[:nrow].cpu().numpy(), total=total, mx=mx, ncorrupt=ncorrupt)


def _blocks(res):
    return [res["dst"][int(o): int(o) + int(n)].tobytes() for o, n in zip(res["doff"], res["dlen"])]


# ---------------------------------------------------------------- 1. the stage ABI
@pytest.mark.parametrize("nblk", [0, 1, 63, 64, 65])
@pytest.mark.parametrize("bs", [1024, 4096, 65536])
def test_stage_abi(oracle, bs, nblk):
    torch, mtblx, _lib, reader = _mods()
    kind = "phrases" if bs != 4096 else "random"
    data, boff, bln, recs = _file(oracle, kind, bs, nblk)
    r = reader.ReaderBuilder().read(data)
    rh = reader.ReaderBuilder(snappy_stage="host").read(data)
    off, ln, st = r._framing()
    assert int(off.numel()) == nblk and (off.cpu().numpy() == boff).all()
    want = [oracle.snappy_decompress(data[int(o): int(o) + int(n)]) for o, n in zip(boff, bln)]
    assert all(w is not None for w in want)
    if kind == "phrases" and nblk:
        assert sum(len(w) for w in want) >= 2 * int(bln.sum())                # the copy elements are exercised
    res = _stage(r, off, ln, st, base=32)
    assert res["ncorrupt"] == 0 and res["mx"] == max([len(w) for w in want] or [0])
    assert _blocks(res) == want
    # the rows mtblx_get_decompressed takes, and the host stage's layout and bytes
    assert (res["ts"] == boff).all() and (res["tdo"] == res["doff"]).all() and (res["tdl"] == res["dlen"]).all()
    assert (res["tst"] == 0).all() and (res["doff"] % 16 == 0).all()
    hbuf, hoff, hlen, hzerr = rh._host_stage(off, ln, st)
    assert (hlen.astype(np.int64) == res["dlen"]).all() and (hoff.astype(np.int64) + 32 == res["doff"]).all()
    assert not hzerr.any()
    assert [hbuf[int(o): int(o) + int(n)].tobytes() for o, n in zip(hoff, hlen)] == want
    if nblk < 2:
        return
    # a selection: the same blocks, compact rows and per-ordinal rows
    pick = np.arange(0, nblk, 3, dtype=np.int32)
    sel = torch.from_numpy(pick).to(r.file.device)
    sub = _stage(r, off, ln, st, sel=sel)
    assert _blocks(sub) == [want[i] for i in pick] and (sub["ts"] == boff[pick]).all() and (sub["tst"] == 0).all()
    byo = _stage(r, off, ln, st, sel=sel, base=16, by_ordinal=True)
    assert (byo["ts"][pick] == boff[pick]).all() and (byo["tdl"][pick] == sub["dlen"]).all()
    assert (byo["tdo"][pick] == sub["doff"] + 16).all() and (byo["tst"][pick] == 0).all()
    rest = np.setdiff1d(np.arange(nblk), pick)
    assert (byo["ts"][rest] == -7).all() and (byo["tst"][rest] == -7).all()  # rows not selected: untouched
    # entries the reference panics on before it decompresses: length 0 and no error
    st2 = st.clone()
    st2[1] = _lib.DIR_PANIC
    bad = torch.zeros(nblk, dtype=torch.uint8, device=r.file.device)
    bad[0] = 1
    bad[nblk - 1] = 1
    m = _stage(r, off, ln, st2, bad=bad)
    masked = {0, 1, nblk - 1}
    assert m["ncorrupt"] == 0
    for i in range(nblk):
        assert m["tst"][i] == 0
        assert m["dlen"][i] == (0 if i in masked else len(want[i])) == m["tdl"][i]
    assert [b for i, b in enumerate(_blocks(m)) if i not in masked] == [w for i, w in enumerate(want) if i not in masked]


def test_stage_large_value(oracle):
    """one value of 200 KiB: a block the large-block kernel variant decompresses"""
    torch, mtblx, _lib, reader = _mods()
    rng = np.random.default_rng(3)
    big = b"".join(PHRASES[int(i)] for i in rng.integers(0, len(PHRASES), 20000))[: 200 * 1024]
    assert len(big) == 200 * 1024
    recs = [(b"k%04d" % i, b"v%d" % i * 7) for i in range(300)]
    recs.insert(150, (b"k0149x", big))
    data, boff, bln = _write(recs, 4096)
    r = reader.ReaderBuilder().read(data)
    off, ln, st = r._framing()
    want = [oracle.snappy_decompress(data[int(o): int(o) + int(n)]) for o, n in zip(boff, bln)]
    res = _stage(r, off, ln, st)
    assert res["mx"] > 200 * 1024 and _blocks(res) == want and (res["tst"] == 0).all()
    assert r.iter().records() == recs and r.stage_stats["host_blocks"] == 0
    st_, vo, vl = r.get_batch([b"k0149x", b"k0000", b"k0299"])
    src = r.value_source.cpu().numpy()
    assert st_.tolist() == [0, 0, 0] and src[int(vo[0]): int(vo[0]) + int(vl[0])].tobytes() == big


# ---------------------------------------------------------------- 2. corrupt stored bytes
def _check_iter(oracle, reader, data, verify, stage="device"):
    exp = oracle.file_scan(data, "iter", verify=verify)
    r = reader.ReaderBuilder(snappy_stage=stage).verify_checksums(verify).read(data)
    s = r.iter()
    errs = (reader.END_ERR_OPEN, reader.END_ERR_NEXT)
    assert (s.end, s.err if s.end in errs else None) == (exp["end"], exp["err"] if exp["end"] in errs else None)
    assert s.records() == exp["records"]
    return r, exp


def _check_get(oracle, reader, _lib, r, data, queries, verify):
    st, vo, vl = r.get_batch(queries)
    st, vo, vl = st.cpu().numpy(), vo.cpu().numpy(), vl.cpu().numpy()
    src = r.value_source.cpu().numpy()
    end_of = {reader.END_NONE: _lib.GET_NONE, reader.END_PANIC: _lib.GET_PANIC, reader.END_ERR_OPEN: _lib.GET_ERR,
              reader.END_ERR_NEXT: _lib.GET_ERR, reader.END_LOOP: _lib.GET_LOOP}
    seen = set()
    for q, key in enumerate(queries):
        exp = oracle.file_scan(data, "get", key=key, verify=verify)
        if exp["records"]:
            assert st[q] == _lib.GET_FOUND, (q, key, st[q])
            assert src[vo[q]: vo[q] + vl[q]].tobytes() == exp["records"][0][1]
        else:
            assert st[q] == end_of[exp["end"]], (q, key, st[q], exp["end"])
        seen.add(int(st[q]))
    return seen


def _mutations(oracle, data, boff, bln, b):
    """(name, file) with block b's stored bytes corrupted; "+crc": the stored checksum made to match,
    so the decompress step is reached with verification on as well"""
    o, n = int(boff[b]), int(bln[b])
    assert n >= 128 and data[o] & 0x80 and not data[o + 1] & 0x80           # a two-byte preamble
    out = []

    def fixed(d, start, size):
        d = bytearray(d)
        d[start - 4: start] = oracle.crc32c(bytes(d[start: start + size])).to_bytes(4, "little")
        return bytes(d)

    d = bytearray(data)
    d[o + n // 2] ^= 0x5A
    out += [("flip", bytes(d)), ("flip+crc", fixed(d, o, n))]
    d = bytearray(data)
    d[o + 1] += 1                                                           # the preamble claims 128 bytes more
    out += [("raised", bytes(d)), ("raised+crc", fixed(d, o, n))]
    d = bytearray(data)
    assert d[o + 1] > 1
    d[o + 1] -= 1                                                           # ... and 128 bytes fewer
    out += [("lowered", bytes(d)), ("lowered+crc", fixed(d, o, n))]
    # a stored length of 0: the frame's length varint (two bytes: 128 <= n < 16384) becomes the single byte 0
    d = bytearray(data)
    ll = 2 if n < 16384 else 3
    d[o - 4 - ll] = 0
    out.append(("len0", bytes(d)))
    d[o - 4 - ll + 1: o - ll + 1] = bytes(4)                                 # crc32c(b"") == 0 right after it
    out.append(("len0+crc", bytes(d)))
    return out


def test_corrupt_stored_bytes(oracle):
    torch, mtblx, _lib, reader = _mods()
    data, boff, bln, recs = _file(oracle, "phrases", 1024, 65)
    keys = [k for k, _ in recs]
    rng = np.random.default_rng(9)
    b = 20
    ikeys = [k for k, _ in oracle.index_records(data)]
    inb = [k for k in keys if ikeys[b - 1] < k <= ikeys[b]]
    qs = inb[:4] + [inb[-1], inb[-1] + b"\x00", keys[0], keys[-1]] + [keys[int(i)] for i in rng.integers(0, len(keys), 12)]
    ends, gets = set(), set()
    for name, d in _mutations(oracle, data, boff, bln, b):
        for verify in (True, False):
            r, exp = _check_iter(oracle, reader, d, verify)
            ends.add((exp["end"], exp["err"] if exp["end"] in (1, 2) else None))
            if not name.startswith("flip+crc") and not (name == "flip" and not verify):
                assert exp["end"] != reader.END_NONE, (name, verify)         # (a flipped literal byte may decode)
            gets |= _check_get(oracle, reader, _lib, r, d, qs, verify)
            assert r.stage_stats["host_blocks"] == 0, (name, verify)
    assert (reader.END_PANIC, None) in ends and (reader.END_ERR_NEXT, "Io") in ends
    assert {_lib.GET_FOUND, _lib.GET_PANIC, _lib.GET_ERR} <= gets


# ---------------------------------------------------------------- 3. nothing staged on the host
def test_no_host_staging(oracle):
    torch, mtblx, _lib, reader = _mods()
    data, boff, bln, recs = _file(oracle, "random", 4096, 65)
    keys = [k for k, _ in recs]
    r = reader.ReaderBuilder().read(data)
    assert r.iter().records() == recs == oracle.file_scan(data, "iter")["records"]
    p = keys[len(keys) // 2][:2]
    assert r.iter_prefix(p).records() == oracle.file_scan(data, "prefix", p)["records"] != []
    qs = [("prefix", p), ("get", keys[7]), ("range", keys[100], keys[130]), ("from", keys[-3])]
    sb = r.scan_batch(qs)
    for i, q in enumerate(qs):
        assert sb.records(i) == oracle.file_scan(data, q[0], q[1], q[2] if q[0] == "range" else b"")["records"], q
    assert sb.n_fallback == 0
    st, vo, vl = r.get_batch(keys[::97])
    assert (st == _lib.GET_FOUND).all()
    s = r.stage_stats
    assert s["host_blocks"] == 0 and s["device_blocks"] >= 65, s
    # the A/B baseline stages on the host and reads the same records
    rh = reader.ReaderBuilder(snappy_stage="host").read(data)
    assert rh.iter().records() == recs
    assert rh.stage_stats["host_blocks"] == 65 and rh.stage_stats["device_blocks"] == 0


# ---------------------------------------------------------------- 4. the on-demand table
@functools.lru_cache(maxsize=None)
def _file300():
    recs = _phrase_records(300, 5200, 20, 90)
    data, boff, bln = _write(recs, 1024, 4)
    assert len(boff) >= 300, len(boff)
    return data, boff, bln, recs


def _values(r, vo, vl):
    src = r.value_source.cpu().numpy()
    return [src[int(o): int(o) + int(n)].tobytes() for o, n in zip(vo.cpu().numpy(), vl.cpu().numpy())]


def test_on_demand_get(oracle):
    torch, mtblx, _lib, reader = _mods()
    data, boff, bln, recs = _file300()
    nblk = len(boff)
    ikeys = [k for k, _ in oracle.index_records(data)]
    by_block = [[kv for kv in recs if (ikeys[b - 1] if b else b"") < kv[0] <= ikeys[b]] for b in (3, 77, 150, 222, nblk - 1)]
    first = [blk[len(blk) // 2] for blk in by_block]
    r = reader.ReaderBuilder().read(data)
    assert r.table_mode == "on-demand"
    st, vo, vl = r.get_batch([k for k, _ in first])
    assert (st == _lib.GET_FOUND).all() and _values(r, vo, vl) == [v for _, v in first]
    s1 = r.stage_stats
    assert 5 <= s1["resident_blocks"] <= 10 and s1["host_blocks"] == 0 and s1["device_blocks"] == s1["resident_blocks"], s1
    assert r._dec_table()[4] == s1["resident_blocks"]
    assert s1["arena_bytes"] < int(sum(len(k) + len(v) for k, v in recs)) // 8    # not the file
    # other keys: residency only grows, the arena grows (by doubling), the first batch's values stay readable
    rng = np.random.default_rng(11)
    more = [recs[int(i)] for i in rng.integers(0, len(recs), 120)] + [(b"", None), (recs[-1][0] + b"\x00", None)]
    st2, vo2, vl2 = r.get_batch([k for k, _ in more])
    exp2 = [oracle.file_scan(data, "get", key=k)["records"] for k, _ in more]
    assert [s == _lib.GET_FOUND for s in st2.tolist()] == [bool(e) for e in exp2]
    got2 = _values(r, vo2, vl2)
    assert [g for g, e in zip(got2, exp2) if e] == [e[0][1] for e in exp2 if e]
    s2 = r.stage_stats
    assert s2["resident_blocks"] > s1["resident_blocks"] and s2["resident_blocks"] <= s1["resident_blocks"] + 2 * 122
    assert s2["arena_bytes"] > s1["arena_bytes"] and s2["arena_used"] <= s2["arena_bytes"] and s2["host_blocks"] == 0
    assert _values(r, vo, vl) == [v for _, v in first]                        # offsets are relative to the base
    st3, vo3, vl3 = r.get_batch([k for k, _ in first])                        # all resident: nothing staged
    assert r.stage_stats["device_blocks"] == s2["device_blocks"] and _values(r, vo3, vl3) == [v for _, v in first]


def test_on_demand_scan_batch(oracle):
    torch, mtblx, _lib, reader = _mods()
    data, boff, bln, recs = _file300()
    keys = [k for k, _ in recs]
    ikeys = [k for k, _ in oracle.index_records(data)]
    last_first = next(k for k in keys if k > ikeys[-2])                       # the last block's first key
    qs = [("prefix", keys[900][:3]), ("prefix", keys[2000]), ("range", keys[1500], keys[1540]),
          ("from", keys[-2]), ("get", keys[33]), ("get", keys[33] + b"\x00"),
          ("from", last_first), ("get", keys[-1]), ("prefix", last_first[:4]),         # landing in the last block
          ("range", b"", keys[2]), ("get", b""), ("prefix", b"\x00"),                  # before the first key
          ("range", keys[100], keys[3000]),                                           # wider than max_blocks
          ("range", ikeys[40], ikeys[40] + b"\x00"), ("prefix", b"\xff\xff"), ("from", keys[-1] + b"\x01")]
    wide = 12
    r = reader.ReaderBuilder().read(data)
    sb = r.scan_batch(qs, max_blocks=8)
    st = sb.status.cpu().numpy()
    for i, q in enumerate(qs):
        it = (r.iter_prefix(q[1]) if q[0] == "prefix" else r.iter_range(q[1], q[2]) if q[0] == "range"
              else r.iter_from(q[1]) if q[0] == "from" else None)
        want = it.records() if it is not None else oracle.file_scan(data, "get", q[1])["records"]
        assert sb.records(i) == want, q
        assert want == oracle.file_scan(data, q[0], q[1], q[2] if q[0] == "range" else b"")["records"], q
    assert sb.n_fallback == 0                                                 # an under-marking touch fails here
    assert st[wide] == _lib.SCAN_LARGE and int((st == _lib.SCAN_OK).sum()) >= 12
    s = r.stage_stats
    assert s["host_blocks"] == 0 and r.table_mode == "on-demand"
    assert s["resident_blocks"] <= 8 * len(qs)
    # count_batch takes the same route
    r2 = reader.ReaderBuilder().read(data)
    cst, cn, ckb, cvb = r2.count_batch(qs, max_blocks=8)
    assert cst.cpu().numpy().tolist() == st.tolist()
    assert cn.tolist() == [len(sb.records(i)) if st[i] == _lib.SCAN_OK else 0 for i in range(len(qs))]
    assert r2.stage_stats["host_blocks"] == 0 and 0 < r2.stage_stats["resident_blocks"] < len(boff)


def test_touch_is_only_a_hint(oracle, monkeypatch):
    """with a touch that marks nothing the lookup kernels report every block missing: get_batch
    stages what they name (still on the device) and scan_batch hands every query to bulk()"""
    torch, mtblx, _lib, reader = _mods()
    data, boff, bln, recs = _file300()
    r = reader.ReaderBuilder().read(data)
    assert r.table_mode == "on-demand"
    monkeypatch.setattr(r, "_od_touch", lambda *a, **k: None)
    rng = np.random.default_rng(12)
    picks = [recs[int(i)] for i in rng.integers(0, len(recs), 20)]
    st, vo, vl = r.get_batch([k for k, _ in picks] + [b"nokey"])
    assert st.tolist() == [_lib.GET_FOUND] * 20 + [_lib.GET_NONE]
    assert _values(r, vo[:20], vl[:20]) == [v for _, v in picks]
    s = r.stage_stats
    assert s["host_blocks"] == 0 and 1 <= s["resident_blocks"] <= 42 and r.table_mode == "on-demand"
    qs = [("prefix", recs[4000][0][:5]), ("range", recs[10][0], recs[12][0])]
    sb = r.scan_batch(qs)
    for i, q in enumerate(qs):
        assert sb.records(i) == oracle.file_scan(data, q[0], q[1], q[2] if q[0] == "range" else b"")["records"], q
    assert r.stage_stats["host_blocks"] == 0


def test_touch_and_compact_abi(oracle):
    """mtblx_scan_touch marks [lo, min(hi, lo + cap - 1)]; mtblx_bitmap_compact lists bits & ~exclude"""
    torch, mtblx, _lib, reader = _mods()
    import bisect
    data, boff, bln, recs = _file300()
    nblk = len(boff)
    ikeys = [k for k, _ in oracle.index_records(data)]
    r = reader.ReaderBuilder().read(data)
    od = r._on_demand()
    assert od
    dev = r.file.device
    starts = [b"", ikeys[5], ikeys[5] + b"\x00", ikeys[-1], ikeys[-1] + b"\x00", ikeys[64], ikeys[100]]
    bounds = [b"", ikeys[5], ikeys[9], b"", b"", ikeys[64], ikeys[299] if nblk > 299 else ikeys[-1]]
    caps = [3, 2, 64, 64, 64, 1, 40]

    def blob(ks):
        b = torch.frombuffer(bytearray(b"".join(ks) or b"\0"), dtype=torch.uint8).to(dev)
        return b, torch.from_numpy(np.cumsum([len(k) for k in ks], dtype=np.int64)).to(dev)

    kb, ke = blob(starts)
    bb, be = blob(bounds)
    cap = torch.from_numpy(np.array(caps, np.int32)).to(dev)
    want = torch.zeros(od.nwords, dtype=torch.int32, device=dev)
    L = _lib.lib()
    rc = L.mtblx_scan_touch(_p(r.file), r.len, r.index_off, r.index_len, _p(od.eoffs), nblk, _p(kb), _p(ke), _p(bb),
                            _p(be), _p(cap), 0, len(starts), _p(want), od.nwords, None)
    assert rc == 0
    exp = set()
    for s, b, c in zip(starts, bounds, caps):
        lo = bisect.bisect_left(ikeys, s)
        if lo >= nblk:
            continue
        hi = min(bisect.bisect_left(ikeys, b) + 1, nblk - 1) if b else nblk - 1
        exp |= set(range(lo, min(max(hi, lo), lo + c - 1) + 1))
    lst = torch.full((nblk,), -1, dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    assert L.mtblx_bitmap_compact(_p(want), None, nblk, _p(lst), nblk, _p(cnt), None) == 0
    n = int(cnt.item())
    assert lst[:n].tolist() == sorted(exp) and (lst[n:] == -1).all()
    # an exclusion mask, and a list shorter than the count
    excl = torch.from_numpy(np.array([0x5555AAAA] * od.nwords, np.uint32).view(np.int32)).to(dev)
    keep = [i for i in sorted(exp) if not (0x5555AAAA >> (i & 31)) & 1]
    lst.fill_(-1)
    assert L.mtblx_bitmap_compact(_p(want), _p(excl), nblk, _p(lst), 4, _p(cnt), None) == 0
    assert int(cnt.item()) == len(keep) and lst[:4].tolist() == keep[:4] and (lst[4:] == -1).all()


# ---------------------------------------------------------------- 5. an irregular index
def _index_entry_offsets(data: bytes):
    """(content start, entry offsets, restart points) of a V2 file's index block, every header a
    1-byte varint triple"""
    p, ln, sh = int.from_bytes(data[-512:-504], "little"), 0, 0
    while True:
        b = data[p]
        ln |= (b & 0x7F) << sh
        p += 1
        sh += 7
        if b < 0x80:
            break
    c0 = p + 4
    content = data[c0: c0 + ln]
    n = int.from_bytes(content[-4:], "little")
    R = ln - 4 * (n + 1)
    restarts = [int.from_bytes(content[R + 4 * i: R + 4 * i + 4], "little") for i in range(n)]
    offs, q = [], restarts[0]
    while q < R:
        offs.append(q)
        q += 3 + content[q + 1] + content[q + 2]
    return c0, offs, restarts


def test_irregular_index_full_device_table(oracle):
    """the corruption of test_get_batch_compressed_seek_past_linear_walk: the index is corrupt
    mid-chain, so the table is the full one, staged on the device; blocks past the corruption reach
    it through MTBLX_GET_MISSING and the host path"""
    torch, mtblx, _lib, reader = _mods()
    rng = np.random.default_rng(91)
    recs = corpus.random_records(rng, 3000, 8, 40, 40, 120)
    data, boff, bln = _write(recs, 1024, 16)
    c0, offs, restarts = _index_entry_offsets(data)
    assert len(restarts) >= 4
    bad_entry = offs.index(restarts[1]) + 3
    d = bytearray(data)
    d[c0 + offs[bad_entry]] = 0x7F
    d = bytes(d)
    keys = [k for k, _ in recs]
    qs = [keys[int(i)] for i in rng.integers(0, len(keys), 100)] + [keys[-1], keys[0], keys[-1] + b"\x01"]
    r = reader.ReaderBuilder().verify_checksums(False).read(d)
    assert r.table_mode == "full"
    ntab0 = r._dec_table()[4]
    s0 = r.stage_stats
    assert 0 < ntab0 <= bad_entry and s0["host_blocks"] == 0 and s0["device_blocks"] == ntab0 == s0["resident_blocks"]
    seen = _check_get(oracle, reader, _lib, r, d, qs, False)
    assert _lib.GET_FOUND in seen
    s1 = r.stage_stats
    assert r._dec_table()[4] > ntab0 and s1["host_blocks"] == r._dec_table()[4] - ntab0 and r.table_mode == "full"
    sb = r.scan_batch([("get", qs[0]), ("prefix", qs[1][:3])])                # irregular: every query through bulk()
    assert sb.records(0) == oracle.file_scan(d, "get", qs[0], verify=False)["records"]


# ---------------------------------------------------------------- 6. a Merger over Snappy sources
def test_merger_over_snappy_sources(oracle):
    torch, mtblx, _lib, reader = _mods()
    from mtblx import merger
    snappy = mtblx.CompressionType.Snappy
    rng = np.random.default_rng(17)
    pool = [b"key%05d" % i for i in range(1200)]
    srcs = []
    for s in range(3):
        ks = sorted(set(pool[int(i)] for i in rng.integers(0, len(pool), 700)))
        srcs.append([(k, PHRASES[(s + len(k)) % len(PHRASES)] * int(rng.integers(1, 4)) + b"%d" % s) for k in ks])
    out = {}
    for comp in (1, 0):
        readers = [reader.ReaderBuilder().read(_write(s, 1024, 16, comp)[0]) for s in srcs]
        assert all(r.compression == comp for r in readers)
        f = merger.Merger.builder("concat").extend(readers).build().write_file(1024, 16, compression=snappy)
        out[comp] = f.cpu().numpy().tobytes()
        for r in readers:
            assert r.stage_stats["host_blocks"] == 0
            assert (r.stage_stats["device_blocks"] > 0) == (comp == 1)
    assert out[1] == out[0]
    got = oracle.file_scan(out[1], verify=True)
    assert got["end"] == 0 and len(got["records"]) == len(set(k for s in srcs for k, _ in s))

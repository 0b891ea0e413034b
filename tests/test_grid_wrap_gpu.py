"""The wrap-around trip of every capped launch, at small sizes.

Most launches cap their grid at a multiple of the device's compute units and let every workgroup,
wave or lane loop over the rest; on a whole MI355X the second trip of those loops needs inputs no
other test reaches.  Here the library's diagnostic CU limit (grid_util.cu_limit) lowers the cap to 1
and 3 compute units, the library reports what a launch then starts (grid_util.items -- no launch
constant is copied into this file), and every case feeds 3 * cap + r items: each worker makes at
least three trips, the last one ragged.

Every expectation is the reference the kernel's own test file uses -- the oracle, merger_model,
sorter_model, where_model, Reduce.fold, numpy -- never the code under test at another limit."""
import bisect
import ctypes as C
import functools

import numpy as np
import pytest

import corpus
import grid_util as gu
import merger_model as mm
import scan_util as su
import sorter_model as sm

pytestmark = pytest.mark.gpu

OPS = ("sum", "min", "max")


def _mods():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mtblx
    from mtblx import _lib, codec, encode, merger, reader, sorter
    return torch, mtblx, _lib, codec, encode, merger, reader, sorter


@pytest.fixture(autouse=True)
def _no_limit_leaks():
    """every test starts and ends with no limit in force"""
    import mtblx
    assert mtblx.lib().mtblx_debug_cu_limit(0) == 0
    yield
    assert mtblx.lib().mtblx_debug_cu_limit(0) == 0


# ---------------------------------------------------------------- the seam itself
def test_limit_only_lowers_and_restores():
    torch, mtblx, _lib, *_ = _mods()
    L = mtblx.lib()
    free = [gu.items(f) for f in range(_lib.GRID_DECODE_TILES + 1)]
    with gu.cu_limit(1):
        one = [gu.items(f) for f in range(_lib.GRID_DECODE_TILES + 1)]
        with gu.cu_limit(3):
            three = [gu.items(f) for f in range(_lib.GRID_DECODE_TILES + 1)]
        assert [gu.items(f) for f in range(_lib.GRID_DECODE_TILES + 1)] == one     # the inner block restored 1
    assert all(a < b < c for a, b, c in zip(one, three, free)), (one, three, free)
    assert all(3 * a == b for a, b in zip(one, three))
    with gu.cu_limit(1 << 20):                                                    # never above the device
        assert [gu.items(f) for f in range(_lib.GRID_DECODE_TILES + 1)] == free
    with gu.cu_limit(-5):                                                         # at least one compute unit
        assert [gu.items(f) for f in range(_lib.GRID_DECODE_TILES + 1)] == one
    with pytest.raises(ZeroDivisionError):
        with gu.cu_limit(1):
            1 // 0
    assert L.mtblx_debug_cu_limit(0) == 0 and L.mtblx_debug_grid_items(99, 0) == 0


# ---------------------------------------------------------------- scans
SCAN_FILES = ("plain", "snappy", "v1")


@functools.lru_cache(maxsize=None)
def _scan_file(name, encoding):
    """-> (data, queries, limits, Reduce, Where) of tests/test_where_gpu.py's file cases; "v1": the
    uncompressed file re-framed as format version 1"""
    import test_where_gpu as wg
    data, _, qs, lim, red, w = wg._file_case("plain" if name == "v1" else name, encoding)
    return (corpus.to_v1(data) if name == "v1" else data), qs, lim, red, w


def _scan_expected(oracle, name, encoding):
    data, qs, lim, _, _ = _scan_file(name, encoding)
    return [su.expected(oracle, data, q, m, True, tag=("wrap", name, encoding)) for q, m in zip(qs, lim)]


def _wave_order(exps, qs, lim, cap, n):
    """n picks of the base queries, ordered so that the queries one wave meets on its successive trips
    (positions p, p + cap, p + 2 cap, ...) alternate between answers with records and empty answers,
    and change kind: a wave goes from a full accumulator to an empty answer and back"""
    full = [i for i, e in enumerate(exps) if e["records"]]
    empty = [i for i, e in enumerate(exps) if not e["records"]]
    assert len(full) > 20 and len(empty) > 10
    pick = []
    for p in range(n):
        trip = p // cap
        pool = empty if trip & 1 else full
        pick.append(pool[(7 * p + 3 * trip) % len(pool)])
    for p in range(n - cap):
        assert bool(exps[pick[p]]["records"]) != bool(exps[pick[p + cap]]["records"])
    return pick


@pytest.mark.parametrize("encoding", ["u64le", "varint"])
@pytest.mark.parametrize("name", SCAN_FILES)
@pytest.mark.parametrize("limit", gu.LIMITS)
def test_scans(oracle, limit, name, encoding):
    """scan_batch, count_batch, reduce_batch and reduce_batch(where=) over 3 * cap + r queries"""
    torch, mtblx, _lib, codec, encode, merger, reader, sorter = _mods()
    import test_where_gpu as wg
    data, qs0, lim0, red, w = _scan_file(name, encoding)
    exps0 = _scan_expected(oracle, name, encoding)
    with gu.cu_limit(limit):
        cap = gu.items(_lib.GRID_SCAN_PLAN)
        n = gu.wrapped(cap, 5)
        assert n > 2 * cap and n > 2 * gu.items(_lib.GRID_SCAN_EMIT)
        pick = _wave_order(exps0, qs0, lim0, cap, n)
        qs, lim, exps = [qs0[i] for i in pick], [lim0[i] for i in pick], [exps0[i] for i in pick]
        late = range(2 * cap, n)   # the third and fourth trips
        assert {qs[p][0] for p in late} == {"from", "get", "prefix", "range"}
        assert any(lim[p] is not None and len(exps[p]["records"]) == lim[p] > 0 for p in late)   # stopped by max_records
        r = reader.Reader(data)
        # the records
        sb = r.scan_batch(qs, max_blocks=1 << 20, max_records=lim)
        assert sb.n_fallback == 0 and sb.n_large == 0
        for p in range(n):
            su.check(reader, sb, p, exps[p], qs[p])
        # the counts (count_batch takes no limits)
        st, nr, kb, vb = (t.cpu().numpy() for t in r.count_batch(qs, max_blocks=1 << 20))
        assert (st == _lib.SCAN_OK).all()
        for p in range(n):
            e = su.expected(oracle, data, qs[p], None, True, tag=("wrap", name, encoding))["records"]
            assert (int(nr[p]), int(kb[p]), int(vb[p])) == (len(e), sum(len(k) for k, _ in e),
                                                             sum(len(v) for _, v in e)), (p, qs[p])
        # the folds; some values of the file are malformed for the Reduce
        rb = r.reduce_batch(qs, red, max_blocks=1 << 20, max_records=lim)
        assert rb.n_fallback == 0 and rb.n_large == 0
        want = [red.fold([v for _, v in e["records"]]) for e in exps]
        assert any(want[p][2] for p in late)
        for p in range(n):
            assert (rb.values(p),) + rb.counts(p) == want[p], (p, qs[p], lim[p])
        # the fused predicate
        wb = r.reduce_batch(qs, red, max_blocks=1 << 20, max_records=lim, where=w)
        assert wb.n_fallback == 0 and wb.n_large == 0
        wg._check_reduce(wb, red, w, [e["records"] for e in exps])
        # max_blocks = 1 hands a share of the queries back, among them late ones; the others keep
        # their neighbours' trips
        nb = reader.Reader(data).reduce_batch(qs, red, max_blocks=1, max_records=lim)
        stn = nb.status.cpu().numpy()
        assert nb.n_fallback == 0 and 0 < nb.n_large < n and (stn[2 * cap:] == _lib.SCAN_LARGE).any()
        assert (stn[2 * cap:] == _lib.SCAN_OK).any()
        for p in range(n):
            assert (nb.values(p),) + nb.counts(p) == want[p], (p, qs[p], lim[p])


def test_scan_offsets_second_pass(oracle):
    """k_scan_offsets is one workgroup of 1024 threads whatever the limit: 3 077 queries give every thread
    a fourth query, the last pass ragged"""
    torch, mtblx, _lib, codec, encode, merger, reader, sorter = _mods()
    data, qs0, lim0, red, _ = _scan_file("plain", "u64le")
    exps0 = _scan_expected(oracle, "plain", "u64le")
    n = 3077
    pick = [(5 * p + p // 1024) % len(qs0) for p in range(n)]
    qs, lim = [qs0[i] for i in pick], [lim0[i] for i in pick]
    r = reader.Reader(data)
    sb = r.scan_batch(qs, max_blocks=1 << 20, max_records=lim)
    assert sb.n_fallback == 0 and sb.n_large == 0
    for p in range(n):
        su.check(reader, sb, p, exps0[pick[p]], qs[p])


# ---------------------------------------------------------------- get
class _Memo:
    """the oracle with file_scan remembered per argument list: the get cases repeat their keys"""

    def __init__(self, oracle):
        self._o, self._m = oracle, {}

    def __getattr__(self, name):
        return getattr(self._o, name)

    def file_scan(self, data, mode="iter", **kw):
        k = (id(data), mode, tuple(sorted(kw.items())))
        if k not in self._m:
            self._m[k] = self._o.file_scan(data, mode, **kw)
        return self._m[k]


@functools.lru_cache(maxsize=None)
def _get_pool(name):
    """hits, misses between two keys, before the first and after the last key, every block's last
    entry and the miss just after it"""
    import pyoracle
    data = _scan_file(name, "u64le")[0]
    keys = [k for k, _ in pyoracle.file_scan(data)["records"]]
    ikeys = [k for k, _ in pyoracle.index_records(data)]
    last = [keys[bisect.bisect_right(keys, s) - 1] for s in ikeys]
    pool = keys[::3] + [k + b"\x00" for k in keys[1::9]] + [k[:-1] for k in keys[2::9] if k]
    pool += [b"", b"\x00", keys[0], keys[0][:-1], keys[-1], keys[-1] + b"\x01", b"\xff" * 40]
    pool += last + [k + b"\x00" for k in last]
    return data, pool


@pytest.mark.parametrize("kernel", ["lanes", "wave"])
@pytest.mark.parametrize("verify", [True, False])
@pytest.mark.parametrize("name", SCAN_FILES)
@pytest.mark.parametrize("limit", gu.LIMITS)
def test_get(oracle, limit, name, verify, kernel):
    torch, mtblx, _lib, *_ = _mods()
    import test_reader_gpu as tr
    data, pool = _get_pool(name)
    with gu.env("MTBLX_GET_KERNEL", kernel), gu.cu_limit(limit):
        cap = gu.items(_lib.GRID_GET)
        n = gu.wrapped(cap, 7)
        assert n > 2 * cap
        keys = [pool[(11 * p + p // cap) % len(pool)] for p in range(n)]
        tr._check_get(_memo(oracle), data, keys, verify=verify)


_memos = {}


def _memo(oracle):
    return _memos.setdefault(id(oracle), _Memo(oracle))


# ---------------------------------------------------------------- merge, segmented merge, sort
COMMON = b"common-12-by"


def _values(rng, n, kind):
    if kind == "bytes":
        return [bytes(rng.integers(0, 256, int(m), dtype=np.uint8)) for m in rng.integers(0, 24, n)]
    import test_reduce_varint_gpu as tv
    f = tv.rand_fields(rng, n, len(OPS))
    if kind == "varint":
        return [tv.enc(*(int(x) for x in row)) for row in f]
    return [row.astype("<u8").tobytes() for row in f]


def _sources(n, kind, seed, nsrc=5):
    """nsrc sorted sources of n records in all, about half of the keys in two sources or more.  Every key
    starts with the same 12 bytes except the first key of the LAST source (a record index above
    0.8 n), which differs in byte 3: the launch that takes the shared prefix length down must see it"""
    rng = np.random.default_rng(seed)
    per = [n // nsrc + (1 if s < n % nsrc else 0) for s in range(nsrc)]
    span = max(per) * 2
    out = []
    for s in range(nsrc):
        idx = np.sort(rng.choice(span, size=per[s], replace=False))
        ks = [COMMON + b"%08d" % int(i) for i in idx]
        if s == nsrc - 1:
            ks[0] = b"com" + b"!" + ks[0][4:]
        out.append(list(zip(ks, _values(rng, per[s], kind))))
        assert all(a < b for a, b in zip(ks, ks[1:]))
    assert sum(per) == n and sum(per[:-1]) > 0.79 * n
    return out


def _reducers(kind):
    _, mtblx, *_ = _mods()
    if kind == "varint":
        import test_reduce_varint_gpu as tv
        return tv.V(*OPS), tv.reducer(*OPS)
    import test_reduce_gpu as tg
    return mtblx.Reduce(*OPS), tg.reducer(*OPS)


@pytest.mark.parametrize("mode", ["groups", "concat", "u64le", "varint"])
@pytest.mark.parametrize("limit", gu.LIMITS)
def test_merge_records(limit, mode):
    """five sources, 3 * cap + r records.  Also the regression test of k_merge_prefix: the smallest
    first key lies in the last source and differs from every other key in byte 3, so the shared
    length is 3, not 12; a kernel that keeps source 0's first key as the smallest merges that record
    into the group of the key with the same last 8 bytes ("Looping launches")"""
    torch, mtblx, _lib, codec, encode, merger, reader, sorter = _mods()
    from test_merger_gpu import promised
    with gu.cu_limit(limit):
        cap = gu.items(_lib.GRID_MERGE_BUILD)
        n = gu.wrapped(cap, 37)
        assert n > 2 * cap
        srcs = _sources(n, "bytes" if mode in ("groups", "concat") else mode, 10 * limit + len(mode))
        assert sum(len(s) for s in srcs[:-1]) > 2 * cap      # the odd key lies in the wrapped part
        d = [encode.DeviceRecords.from_list(s) for s in srcs]
        if mode == "groups":
            want = promised(srcs)
            assert mm.canon(want) == mm.canon(mm.multi_iter(srcs))
            assert merger.merge_records(d, "groups").to_list() == want
        elif mode == "concat":
            # the values of a group in source order (the model's heap fixes their multiset only: mm.canon)
            want = promised(srcs)
            assert mm.canon(want) == mm.canon(mm.multi_iter(srcs))
            assert merger._records_list(merger.merge_records(d, "concat")) == [(k, b"".join(vs)) for k, vs in want]
        else:
            red, fn = _reducers(mode)
            want = mm.merge_iter(srcs, fn)
            assert sum(1 for k, vs in promised(srcs) if len(vs) > 1) > n // 8
            assert merger._records_list(merger.merge_records(d, red)) == want


@pytest.mark.parametrize("mode", ["groups", "last"])
@pytest.mark.parametrize("limit", gu.LIMITS)
def test_merge_segments(limit, mode):
    """three segments cut at the same two keys in every source: segment q of the result is the merge of
    segment q of every source"""
    torch, mtblx, _lib, codec, encode, merger, reader, sorter = _mods()
    from test_merger_gpu import promised
    with gu.cu_limit(limit):
        cap = gu.items(_lib.GRID_SEG_BUILD)
        n = gu.wrapped(cap, 41)
        assert n > 2 * cap
        srcs = _sources(n, "bytes", 20 + limit)
        allk = sorted({k for s in srcs for k, _ in s})
        cuts = [allk[len(allk) // 3], allk[2 * len(allk) // 3]]
        offs, segs = [], [[], [], []]
        for s in srcs:
            ks = [k for k, _ in s]
            o = [0] + [bisect.bisect_left(ks, c) for c in cuts] + [len(ks)]
            offs.append(torch.tensor(o, dtype=torch.int64, device="cuda"))
            for q in range(3):
                segs[q].append(s[o[q]: o[q + 1]])
        d = [encode.DeviceRecords.from_list(s) for s in srcs]
        r, seg_end = merger.merge_segments(d, offs, mode)
        want = [promised(x) for x in segs]
        assert seg_end.cpu().numpy().tolist() == np.cumsum([len(x) for x in want]).tolist()
        flat = [g for x in want for g in x]
        if mode == "groups":
            assert r.to_list() == flat
        else:
            assert merger._records_list(r) == [(k, vs[-1]) for k, vs in flat]


@pytest.mark.parametrize("mode", ["groups", "concat", "u64le"])
@pytest.mark.parametrize("limit", gu.LIMITS)
def test_sort_records(limit, mode):
    """every key shares 12 bytes except one record beyond 2 * cap, whose key differs in byte 3: a
    k_sort_skip that never visits the wrapped records sorts by the wrong eight bytes"""
    torch, mtblx, _lib, codec, encode, merger, reader, sorter = _mods()
    import test_sorter_gpu as ts
    with gu.cu_limit(limit):
        cap = gu.items(_lib.GRID_SORT_SKIP)
        n = gu.wrapped(cap, 29)
        assert n > 2 * cap
        rng = np.random.default_rng(30 + limit)
        ids = rng.integers(0, 2 * n // 3, size=n)
        keys = [COMMON + b"%08d" % int(i) for i in ids]
        odd = 2 * cap + cap // 2 + 3
        keys[odd] = b"com" + b"z" + keys[odd][4:]
        assert odd > 2 * cap and len({k[:12] for k in keys}) == 2
        vals = _values(rng, n, "bytes" if mode != "u64le" else "u64le")
        records = list(zip(keys, vals))
        recs = encode.DeviceRecords.from_list(records)
        want = ts.promised(records)
        if mode == "groups":
            assert sorter.sort_records(recs, "groups").to_list() == want
        elif mode == "concat":
            exp = [(k, b"".join(vs)) for k, vs in want]
            if n < 20_000:   # one chunk: the Sorter's model is deterministic
                assert sm.run(records, sm.concat_any)[0] == exp
            assert merger._records_list(sorter.sort_records(recs, "concat")) == exp
        else:
            red, fn = _reducers("u64le")
            exp = [(k, vs[0] if len(vs) == 1 else fn(k, vs)) for k, vs in want]
            if n < 20_000:
                assert sm.run(records, fn)[0] == exp
            assert merger._records_list(sorter.sort_records(recs, red)) == exp


# ---------------------------------------------------------------- CRC
@pytest.mark.parametrize("kernel", ["mfma", "lanes"])
@pytest.mark.parametrize("limit", gu.LIMITS)
def test_crc(oracle, limit, kernel):
    """unframed blocks of mixed lengths and the framed blocks of a file, a corrupted block among the
    wrapped ones"""
    torch, mtblx, _lib, codec, *_ = _mods()
    from mtblx import synth
    with gu.env("MTBLX_CRC_KERNEL", kernel), gu.cu_limit(limit):
        cap = gu.items(_lib.GRID_CRC)
        n = gu.wrapped(cap, 9)
        assert n > 2 * cap
        rng = np.random.default_rng(40 + limit)
        lens = [0, 1, 3, 4, 63, 64, 65, 4096, 17, 300]
        blocks = [bytes(rng.integers(0, 256, lens[(p + p // cap) % len(lens)], dtype=np.uint8)) for p in range(n)]
        blocks[2 * cap + 5] = bytes(rng.integers(0, 256, 70_000, dtype=np.uint8))
        d, o, l = corpus.pack(blocks, rng=rng, lead=3)
        crc, _ = codec.crc32c_blocks(codec.DeviceBatch.from_host(d, o, l), framed=False)
        exp = np.array([oracle.crc32c(b) for b in blocks], np.uint32)
        got = crc.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:10]
        # framed: the stored checksum of one wrapped block and a content byte of another are corrupted
        data, off, ln = synth.cfg2_file(n, block_size=1024)
        assert off.size > 2 * cap
        nb = off.size
        bad_exp = sorted({1, 2 * cap + 1, nb - 2})
        data = data.copy()
        data[int(off[bad_exp[0]]) - 2] ^= 0x40
        data[int(off[bad_exp[1]]) - 3] ^= 0x01
        data[int(off[bad_exp[2]]) + 7] ^= 0x10
        crc, bad = codec.crc32c_blocks(codec.DeviceBatch.from_host(data, off, ln), framed=True)
        exp = np.array([oracle.crc32c(bytes(data[int(a): int(a) + int(m)])) for a, m in zip(off, ln)], np.uint32)
        assert np.array_equal(crc.cpu().numpy().view(np.uint32), exp)
        assert np.nonzero(bad.cpu().numpy())[0].tolist() == bad_exp


# ---------------------------------------------------------------- decode
def _tiles(nblk, max_len, verify):
    import mtblx
    k = C.c_int(-1)
    return int(mtblx.lib().mtblx_debug_decode_tiles(nblk, max_len, 1 if verify else 0, C.byref(k))), k.value


@functools.lru_cache(maxsize=None)
def _decode_blocks(shape):
    """the blocks that select each kernel, irregular (quirk) blocks mixed in so that the exact serial
    path runs in a wrapped tile: 4 KiB cfg2 blocks (the small pipeline: twelve per tile), 64 KiB cfg2
    blocks (the large pipeline: one per tile) and builder blocks above 70 000 bytes (k_decode_tiles)"""
    import pyoracle
    from mtblx import synth
    quirks = [b for _, b, _ in corpus.quirk_blocks()]
    if shape == "small":
        d, o, l = synth.cfg2_file(144)
    elif shape == "large":
        d, o, l = synth.cfg2_file(11, block_size=65536)
    else:
        rng = np.random.default_rng(51)
        big = [pyoracle.build_block(corpus.random_records(rng, 1400, 8, 60, 40, 60)) for _ in range(3)]
        assert min(len(b) for b in big) > 70_000
        return big, quirks
    return [bytes(d[int(a): int(a) + int(m)]) for a, m in zip(o, l)], quirks


def _decode_batch(shape, family, arg, verify_plans):
    """blocks of `shape`, a quirk block after every seventh, until every plan of the batch has at least
    3 * G + 2 tiles; -> (blocks, G)"""
    base, quirks = _decode_blocks(shape)
    G = gu.items(family, arg)
    blocks, i = [], 0
    while True:
        blocks.append(base[i % len(base)])
        if i % 7 == 6:
            blocks.append(quirks[(i // 7) % len(quirks)])
        i += 1
        mx = max(len(b) for b in blocks)
        if all(_tiles(len(blocks), mx, v)[0] >= 3 * G + 2 for v in verify_plans) and i >= 8:
            return blocks, G
        assert i < 4000


def _decode_surfaces(oracle, blocks, G, kind, ws=None):
    """every decode surface over one batch against the oracle (the steps of
    tests/test_decode_gpu.py::test_kernel_choice_edges)"""
    torch, mtblx, _lib, codec, *_ = _mods()
    import valpos_util as vu
    from test_decode_gpu import assert_same
    d, o, l = corpus.pack(blocks, lead=3)
    mx = int(l.max())
    for v in (False, True):
        nt, k = _tiles(len(blocks), mx, v)
        assert nt > 2 * G and nt >= 3 * G + 2 and k in kind, (nt, G, k, kind)
    orc = oracle.decode_blocks(d, o, l)
    clean = bool((orc.status != _lib.ST_OVERFLOW).all())
    exp_crc = np.array([oracle.crc32c(x) for x in blocks], np.uint32)
    nr = int(orc.nrec.sum())
    batch = codec.DeviceBatch.from_host(d, o, l)
    ws = ws if ws is not None else codec.Workspace(batch.nblk)
    out = codec.DecodedBlocks(batch.nblk, nr, orc.keys.size, orc.vals.size)
    codec.decode_into(batch, out, ws)
    torch.cuda.synchronize()
    assert_same(out.to_host(), orc, o.size)
    out = codec.DecodedBlocks(batch.nblk, nr, orc.keys.size, orc.vals.size)
    codec.count_blocks(batch, out, ws)
    torch.cuda.synchronize()
    assert out.totals_host() == (nr, orc.keys.size, orc.vals.size, 0)
    codec.decode_counted(batch, out, ws)
    torch.cuda.synchronize()
    assert_same(out.to_host(), orc, o.size)
    for fused in (True, False):
        out, crc, bad = codec.decode_verify(batch, framed=False, fused=fused)
        torch.cuda.synchronize()
        if clean:
            assert_same(out.to_host(), orc, o.size)
        assert np.array_equal(crc.cpu().numpy().view(np.uint32), exp_crc), fused
        assert not bad.cpu().numpy().any()
    out, vp = codec.decode_positions(batch)
    dev = out.to_host()
    for f in ("status", "nrec", "rec_base", "key_base", "val_base", "key_end", "val_end", "keys"):
        assert np.array_equal(getattr(dev, f), getattr(orc, f)), f
    assert tuple(dev.totals) == (nr, orc.keys.size, orc.vals.size, 0)
    vu.check_positions(d, o, l, orc, vp.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("shape", ["small", "large", "tiles"])
@pytest.mark.parametrize("limit", gu.LIMITS)
def test_decode(oracle, limit, shape):
    """G = the limit (k_decode_tiles: the limit times its occupancy): a look-back window of 0 and of 2
    workgroups, every workgroup taking three tiles or more.  small: PipeSmall / PipeSmallV /
    PipeSmallP; large: PipeLarge / PipeLargeV / PipeLargeP; tiles: k_decode_tiles<CfgLarge, CfgLargeP>"""
    torch, mtblx, _lib, *_ = _mods()
    with gu.cu_limit(limit):
        if shape == "tiles":
            G = max(gu.items(_lib.GRID_DECODE_TILES, 0), gu.items(_lib.GRID_DECODE_TILES, 1))
            blocks, _ = _decode_batch(shape, _lib.GRID_DECODE_TILES, 0, (False, True))
            while _tiles(len(blocks), max(len(b) for b in blocks), False)[0] < 3 * G + 2:
                blocks = blocks + blocks[:3]
            _decode_surfaces(oracle, blocks, G, (2,))
        else:
            assert gu.items(_lib.GRID_DECODE_PIPE) == limit
            blocks, G = _decode_batch(shape, _lib.GRID_DECODE_PIPE, 0, (False, True))
            _decode_surfaces(oracle, blocks, G, (0,) if shape == "small" else (1,))


def test_decode_one_workspace_across_limits(oracle):
    """one Workspace through a limit-1 launch, a limit-3 launch and a launch with no limit: every launch
    leaves the look-back words ready for a grid of another size"""
    torch, mtblx, _lib, codec, *_ = _mods()
    with gu.cu_limit(3):
        blocks, _ = _decode_batch("small", _lib.GRID_DECODE_PIPE, 0, (False, True))
    ws = codec.Workspace(len(blocks))
    for limit in (1, 3, 0, 3, 1):
        with gu.cu_limit(limit):
            # the step with no limit is there for the workspace hand-over, not for the wrap: its tiles are
            # checked against the G the batch was built for, not against the whole device's cap
            G = gu.items(_lib.GRID_DECODE_PIPE) if limit else 3
            _decode_surfaces(oracle, blocks, G, (0,), ws=ws)


# ---------------------------------------------------------------- snappy
def _snappy_inputs(rng, n, cap):
    """n inputs of at most 4608 bytes: tests/test_snappy_gpu.py's compressible shapes, 1 KiB cfg2 blocks
    and a few incompressible ones, so that neighbours in a wave differ"""
    import test_snappy_gpu as tsn
    from mtblx import synth
    data, off, ln = synth.cfg2_file(40, block_size=1024)
    pool = [bytes(data[int(a): int(a) + int(m)]) for a, m in zip(off, ln)]
    pool += [x for x in tsn._compressible(rng) if len(x) <= 4608]
    pool += [rng.integers(0, 256, int(m), dtype=np.uint8).tobytes() for m in (1, 2, 3, 15, 16, 17, 59, 60, 61, 4608)]
    return [pool[(5 * p + p // cap) % len(pool)] for p in range(n)]


@pytest.mark.parametrize("kernel", ["auto", "lanes", "two", "waves"])
@pytest.mark.parametrize("limit", gu.LIMITS)
def test_snappy_decompress(oracle, limit, kernel):
    torch, mtblx, _lib, codec, *_ = _mods()
    import test_snappy_gpu as tsn
    with gu.env("MTBLX_SNAPPY_KERNEL", None if kernel == "auto" else kernel), gu.cu_limit(limit):
        cap = gu.items(_lib.GRID_SNAPPY_SMALL)
        n = gu.wrapped(cap, 11)
        assert n > 2 * cap
        rng = np.random.default_rng(60 + limit)
        streams = tsn._streams(_snappy_inputs(rng, n, cap))
        z = bytearray(streams[2 * cap + 3])
        z[0] ^= 0x7F                                  # a preamble that no longer matches the body
        streams[2 * cap + 3] = bytes(z)
        streams[2 * cap + 9] = streams[2 * cap + 9][:-1] if len(streams[2 * cap + 9]) > 1 else b"\x05ab"
        got, st, o = tsn._device(codec, streams, rng, lead=3)
        tsn._check(oracle, streams, got, st)
        assert st[2 * cap + 3] == 1 and (st == 0).sum() >= n - 2


@pytest.mark.parametrize("limit", gu.LIMITS)
def test_snappy_decompress_large(oracle, limit):
    """outputs above 4608 bytes: k_snappy_blocks<Large>, one block per wave"""
    torch, mtblx, _lib, codec, *_ = _mods()
    import test_snappy_gpu as tsn
    with gu.env("MTBLX_SNAPPY_KERNEL", None), gu.cu_limit(limit):
        cap = gu.items(_lib.GRID_SNAPPY_LARGE)
        n = gu.wrapped(cap, 5)
        assert n > 2 * cap
        rng = np.random.default_rng(70 + limit)
        pool = tsn._compressible(rng) + [rng.integers(0, 256, 9000, dtype=np.uint8).tobytes()]
        xs = [pool[(3 * p + p // cap) % len(pool)] for p in range(n)]
        xs[0] = b"abcd" * 16_000
        streams = tsn._streams(xs)
        streams[2 * cap + 1] = streams[2 * cap + 1][:-1] + b"\xff\xff\xff"
        got, st, o = tsn._device(codec, streams, rng, lead=3)
        tsn._check(oracle, streams, got, st)


@pytest.mark.parametrize("limit", gu.LIMITS)
def test_snappy_compress(oracle, limit):
    """every compressed stream decompresses, by the oracle, to its input, and is the stream the same
    input gives at no limit in a batch of its own"""
    torch, mtblx, _lib, codec, *_ = _mods()

    def compress(blocks):
        d, o, l = corpus.pack(blocks, lead=3)
        sbatch, st = codec.snappy_compress(codec.DeviceBatch.from_host(d, o, l))
        torch.cuda.synchronize()
        assert (st.cpu().numpy() == 0).all()
        host = sbatch.data.cpu().numpy()
        so = sbatch.src_off.cpu().numpy().view(np.uint64)
        sl = sbatch.src_len.cpu().numpy().view(np.uint32)
        return [bytes(host[int(a): int(a) + int(m)]) for a, m in zip(so, sl)]

    with gu.cu_limit(limit):
        cap = gu.items(_lib.GRID_SNAPPY_COMP)
        n = gu.wrapped(cap, 3)
        assert n > 2 * cap
        xs = _snappy_inputs(np.random.default_rng(80 + limit), n, cap)
        got = compress(xs)
    for x, z in zip(xs, got):
        assert oracle.snappy_decompress(z) == x
    alone = {}
    for x, z in zip(xs, got):
        if x not in alone:
            alone[x] = compress([x])[0]
        assert z == alone[x]


@functools.lru_cache(maxsize=None)
def _staging_file():
    rng = np.random.default_rng(90)
    recs = corpus.random_records(rng, 34000, 4, 24, 0, 40)
    return su.write(recs, 256, 4, 1), recs


def test_len_scan_second_pass(oracle):
    """k_len_scan is one workgroup of 1 024 threads whatever the limit: 3 077 blocks through snappy_compress
    give every thread a fourth block, the last pass ragged"""
    torch, mtblx, _lib, codec, *_ = _mods()
    xs = _snappy_inputs(np.random.default_rng(85), 3077, 1024)
    d, o, l = corpus.pack(xs, lead=3)
    sbatch, st = codec.snappy_compress(codec.DeviceBatch.from_host(d, o, l))
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all()
    host = sbatch.data.cpu().numpy()
    so = sbatch.src_off.cpu().numpy().view(np.uint64)
    sl = sbatch.src_len.cpu().numpy().view(np.uint32)
    assert (so % 16 == 0).all()
    for x, a, m in zip(xs, so, sl):
        assert oracle.snappy_decompress(bytes(host[int(a): int(a) + int(m)])) == x


@pytest.mark.parametrize("comp", [0, 1], ids=["plain", "snappy"])
@pytest.mark.parametrize("limit", gu.LIMITS)
def test_device_writer_above_1024_blocks(oracle, limit, comp):
    """the device Writer on a file of more than 1 024 data blocks: the index kernel's single-workgroup scan
    (k_scan2) and, for Snappy, the frame layout (k_len_scan) make a second trip, and k_snappy_compress /
    k_frame_write wrap under the limit.  The plain file is the oracle's Writer byte for byte; the Snappy
    file scans, by the oracle, to the records.  Read back, the index block's 1 024 + entries go through
    k_entry_offsets"""
    torch, mtblx, _lib, codec, encode, merger, reader, sorter = _mods()
    recs = _staging_file()[1]
    with gu.cu_limit(limit):
        cap = gu.items(_lib.GRID_SNAPPY_COMP)
        file = encode.write_file(encode.DeviceRecords.from_list(recs), 256, 4, compression=comp)
        data = file.cpu().numpy().tobytes()
        nblk = len(oracle.index_records(data))
        assert nblk > 1024 and nblk > 2 * cap
        if comp == 0:
            assert data == oracle.write_file(recs, 256, 4)
        assert oracle.file_scan(data)["records"] == recs
        keys = [k for k, _ in recs]
        qs = [("get", keys[5]), ("get", keys[-1]), ("prefix", keys[len(keys) // 2][:3]), ("from", keys[-3]),
              ("range", keys[7000], keys[7040]), ("get", b"\xff" * 30)]
        r = reader.Reader(data)
        sb = r.scan_batch(qs, max_blocks=1 << 20)
        assert sb.n_fallback == 0
        for i, q in enumerate(qs):
            su.check(reader, sb, i, su.expected(oracle, data, q, None, True), q)


@pytest.mark.parametrize("limit", gu.LIMITS)
def test_snappy_file_staging(oracle, limit):
    """a Snappy file of 256-byte blocks read through the device staging path.  More than 1 024 blocks: the
    single-workgroup pass over the index block's entries (k_entry_offsets) makes a second trip too"""
    torch, mtblx, _lib, codec, encode, merger, reader, sorter = _mods()
    data, recs = _staging_file()
    with gu.cu_limit(limit):
        cap = gu.items(_lib.GRID_SNAPPY_SMALL)
        r = reader.Reader(data)
        nblk = len(oracle.index_records(data))
        assert nblk > 2 * cap and nblk > 1024
        got = r.iter().records()
        assert r.stage_stats["host_blocks"] == 0
    assert got == oracle.file_scan(data)["records"] == recs


# ---------------------------------------------------------------- copy
@pytest.mark.parametrize("limit", gu.LIMITS)
def test_copy_ranges(limit):
    torch, mtblx, _lib, codec, *_ = _mods()
    with gu.cu_limit(limit):
        cap = gu.items(_lib.GRID_COPY_RANGES)
        n = gu.wrapped(cap, 13)
        assert n > 2 * cap
        rng = np.random.default_rng(100 + limit)
        lens = []
        while sum((m + 15) // 16 for m in lens) < n:
            lens += [int(x) for x in rng.integers(0, 41, 50)] + [int(rng.integers(1000, 9000)), 0, 16, 4099]
        ch = [(m + 15) // 16 for m in lens]
        assert sum(ch) > 2 * cap
        src = rng.integers(0, 256, 1 << 20, dtype=np.uint8)
        so = [int(rng.integers(0, src.size - m + 1)) for m in lens]
        do, acc = [], 5
        for m in lens:
            do.append(acc)
            acc += m + int(rng.integers(0, 3))
        dst = np.zeros(acc + 16, np.uint8)
        cb = np.concatenate([[0], np.cumsum(ch)[:-1]]).astype(np.int64)
        t = lambda a: torch.tensor(np.asarray(a, np.int64), device="cuda")   # noqa: E731
        ds, dd = torch.from_numpy(src).to("cuda"), torch.from_numpy(dst).to("cuda")
        args = [t(so), t(do), t(lens), t(cb)]
        rc = mtblx.lib().mtblx_copy_ranges(C.c_void_p(ds.data_ptr()), C.c_void_p(args[0].data_ptr()),
                                           C.c_void_p(dd.data_ptr()), C.c_void_p(args[1].data_ptr()),
                                           C.c_void_p(args[2].data_ptr()), C.c_void_p(args[3].data_ptr()), len(lens),
                                           int(sum(ch)), C.c_void_p(codec._stream_handle(None)))
        assert rc == 0
        torch.cuda.synchronize()
    for a, b, m in zip(so, do, lens):
        dst[b: b + m] = src[a: a + m]
    assert np.array_equal(dd.cpu().numpy(), dst)


@pytest.mark.parametrize("variant", [0, 1, 2, 3, 2 | 4, 3 | 8, 1 | 4 | 8])
@pytest.mark.parametrize("limit", gu.LIMITS)
def test_stream_copy(limit, variant):
    """every unroll and the non-temporal variants (MTBLX_COPY_NT_STORES = 4, MTBLX_COPY_NT_LOADS = 8)"""
    torch, mtblx, _lib, codec, *_ = _mods()
    with gu.cu_limit(limit):
        cap = gu.items(_lib.GRID_STREAM_COPY, variant)
        n = gu.wrapped(cap, 77)                       # chunks of 16 bytes
        assert n > 2 * cap
        rng = np.random.default_rng(110 + variant)
        src = rng.integers(0, 256, 16 * n + 32, dtype=np.uint8)
        ds = torch.from_numpy(src).to("cuda")
        dd = torch.full((16 * n + 32,), 0xA5, dtype=torch.uint8, device="cuda")
        assert ds.data_ptr() % 16 == 0 and dd.data_ptr() % 16 == 0
        rc = mtblx.lib().mtblx_stream_copy(C.c_void_p(dd.data_ptr()), C.c_void_p(ds.data_ptr()), 16 * n, variant,
                                           C.c_void_p(codec._stream_handle(None)))
        assert rc == 0
        torch.cuda.synchronize()
    got = dd.cpu().numpy()
    assert np.array_equal(got[: 16 * n], src[: 16 * n]) and (got[16 * n:] == 0xA5).all()

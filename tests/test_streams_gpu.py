"""The stream contract ("Streams"; include/mtblx.h): every entry point that
takes `stream=` on a non-default stream, compared with the same reference its own test uses.

Everything else in the suite runs on torch's default stream, the legacy null stream, where one
queue serialises every ordering mistake away.  Here each surface runs in the three configurations
of tests/stream_util.py (a 200 ms hold on the current stream, on the call's own stream, and the
call made ambiently inside torch.cuda.stream(s)); the two positive controls at the top show, with
torch ops alone, that the hold turns a fill on the wrong stream and a read-back on the wrong
stream into wrong bytes every time.

What a hold cannot reach: "own-held" catches a mis-ordered read-back only up to the call's first
synchronise of its stream; what a call does after that synchronise (Reader.scan_batch's flags word
and rec_off after the plan, the reads of merge_records after its plan, write_file after its first
size) is ordered by construction -- the whole body of every wrapper runs under torch.cuda.stream(S)
-- and was checked by reading, not by these tests.  The allocation check at the end covers the
part of that which the allocator can see.

Reader surfaces: mtblx_entry_offsets (once per Reader, behind index_regular()) allocates and frees
device memory itself, a documented exception to C6, so the fixtures call index_regular() before a
hold is armed; everything else a Reader builds lazily (the directory, the on-demand table) is
built under the hold.  write_file surfaces reach mtblx_encode_index_c, the other exception, and
do not assert `pending`.
"""
import numpy as np
import pytest

import corpus
import merger_model as mm
import merger_scan_util as U
import scan_util as su
import valpos_util as vu

pytestmark = pytest.mark.gpu

CONFIGS = ("current-held", "own-held", "ambient")


def _mods():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mtblx
    import stream_util
    from mtblx import _lib, codec, encode, merger, reader, sorter
    return torch, mtblx, stream_util, _lib, codec, encode, merger, reader, sorter


@pytest.fixture(scope="module")
def streams():
    """two non-default streams, shared by the module, each with a hardware queue of its own
    (stream_util.pick_streams): late in a long process the runtime hands out streams that share a
    queue with the default stream, and a hold would then delay both"""
    return _mods()[2].pick_streams(2)


@pytest.fixture(autouse=True)
def _default_snappy_routing(monkeypatch):
    monkeypatch.delenv("MTBLX_SNAPPY_KERNEL", raising=False)


# ---------------------------------------------------------------- positive controls: torch ops only
def test_control_late_fill_wins(streams):
    """a zero fill queued on a held stream lands after another stream's write of the same buffer:
    the buffer ends up all zero.  This is what a wrapper does that zero-fills on the current stream
    and launches on `stream`."""
    torch, _, S = _mods()[:3]
    s = streams[0]
    n = 1 << 16
    ones = torch.ones(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    pending = S.hold(S.default_stream())
    t = torch.zeros(n, dtype=torch.int32, device="cuda")     # allocated now, filled after the hold
    with torch.cuda.stream(s):
        t.copy_(ones)
    s.synchronize()
    assert not pending.query() or S.bounds_build()
    torch.cuda.synchronize()
    assert int(t.sum().item()) == 0


def test_control_early_read_back(streams):
    """a read-back on the current stream does not wait for a kernel queued on a held stream: it
    sees the bytes from before the kernel"""
    torch, _, S = _mods()[:3]
    s = streams[0]
    n = 1 << 16
    u = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    pending = S.hold(s)
    with torch.cuda.stream(s):
        u.fill_(1)
    early = u.cpu()                                           # default stream: nothing orders it after s
    assert not pending.query() or S.bounds_build()
    assert int(early.sum().item()) == 0
    s.synchronize()
    assert int(u.sum().item()) == n


# ---------------------------------------------------------------- raw decode and codec family
@pytest.fixture(scope="module")
def cfg2(oracle):
    """synth.cfg2_file(300) on the device, with the oracle's decode, value positions and checksums"""
    codec = _mods()[4]
    data, off, ln, exp, pos = vu.cfg2(oracle, 300)
    crc = np.array([oracle.crc32c(bytes(data[int(o): int(o) + int(n)])) for o, n in zip(off, ln)], np.uint32)
    return codec.DeviceBatch.from_host(data, off, ln), exp, pos, crc


def _caps(exp):
    return int(exp.nrec.sum()), int(exp.keys.size), int(exp.vals.size)


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("surface", ["decode_into", "count_then_decode_counted"])
def test_decode_into_family(cfg2, streams, surface, config):
    """the asynchronous launches into caller buffers; to_host() reads on the stream that wrote them"""
    torch, _, S, _, codec = _mods()[:5]
    from test_decode_gpu import assert_same
    batch, exp, _, _ = cfg2
    out = codec.DecodedBlocks(batch.nblk, *_caps(exp))
    ws = codec.Workspace(batch.nblk)

    def call(st):
        if surface == "decode_into":
            codec.decode_into(batch, out, ws, st)
        else:
            codec.count_blocks(batch, out, ws, st)
            codec.decode_counted(batch, out, ws, st)
        return out

    S.run(config, call, streams[0], asynchronous=True)
    assert_same(out.to_host(), exp, batch.nblk)


@pytest.mark.parametrize("config", CONFIGS)
def test_decode_blocks(cfg2, streams, config):
    torch, _, S, _, codec = _mods()[:5]
    from test_decode_gpu import assert_same
    batch, exp, _, _ = cfg2
    out = S.run(config, lambda st: codec.decode_blocks(batch, stream=st), streams[0])
    assert_same(out.to_host(), exp, batch.nblk)


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("fused", [False, True])
def test_decode_verify(cfg2, streams, fused, config):
    torch, _, S, _, codec = _mods()[:5]
    from test_decode_gpu import assert_same
    batch, exp, _, crc_exp = cfg2
    s = streams[0]
    out, crc, bad = S.run(config, lambda st: codec.decode_verify(batch, framed=True, stream=st, fused=fused), s)
    assert_same(out.to_host(), exp, batch.nblk)
    assert np.array_equal(S.host(crc, s).view(np.uint32), crc_exp)
    assert not S.host(bad, s).any()


@pytest.mark.parametrize("config", CONFIGS)
def test_decode_positions(cfg2, streams, config):
    torch, _, S, _, codec = _mods()[:5]
    from test_valpos_gpu import _assert_decoded
    batch, exp, pos, _ = cfg2
    s = streams[0]
    out, val_pos = S.run(config, lambda st: codec.decode_positions(batch, stream=st), s)
    dev = out.to_host()
    assert dev.vals.size == 0
    _assert_decoded(dev, exp)
    assert np.array_equal(S.host(val_pos, s).view(np.uint32), pos)


@pytest.mark.parametrize("config", CONFIGS)
def test_crc32c_blocks_framed(cfg2, streams, config):
    torch, _, S, _, codec = _mods()[:5]
    batch, _, _, crc_exp = cfg2
    s = streams[0]
    crc, bad = S.run(config, lambda st: codec.crc32c_blocks(batch, framed=True, stream=st), s, asynchronous=True)
    assert np.array_equal(S.host(crc, s).view(np.uint32), crc_exp)
    assert not S.host(bad, s).any()


@pytest.fixture(scope="module")
def snappy_inputs(oracle):
    """about 40 raw inputs (test_snappy_gpu._compressible + cfg2 blocks) and their Snappy streams"""
    from mtblx import pipe, synth
    from test_snappy_gpu import _compressible
    data, off, ln = synth.cfg2_file(30)
    xs = _compressible(np.random.default_rng(1)) + [bytes(data[int(a): int(a) + int(n)]) for a, n in zip(off, ln)]
    zs = [pipe.snappy_compress(x) for x in xs]
    assert all(oracle.snappy_decompress(z) == x for x, z in zip(xs, zs))
    return xs, zs


def _blocks(S, dec, s):
    """the blocks of a DeviceBatch on the host, read in stream order on s"""
    hostb = S.host(dec.data, s)
    o = S.host(dec.blk_off, s).view(np.uint64)
    n = S.host(dec.blk_len, s).view(np.uint32)
    return [bytes(hostb[int(a): int(a) + int(b)]) for a, b in zip(o, n)]


@pytest.mark.parametrize("config", CONFIGS)
def test_snappy_decompress(oracle, snappy_inputs, streams, config):
    torch, _, S, _, codec = _mods()[:5]
    xs, zs = snappy_inputs
    s = streams[0]
    data, off, ln = corpus.pack(zs, rng=np.random.default_rng(2), lead=3)
    batch = codec.SnappyBatch.from_host(data, off, ln)
    dec, st = S.run(config, lambda q: codec.snappy_decompress(batch, stream=q), s)
    assert not S.host(st, s).any()
    assert _blocks(S, dec, s) == [oracle.snappy_decompress(z) for z in zs] == xs


@pytest.mark.parametrize("config", CONFIGS)
def test_snappy_compress_then_decompress(oracle, snappy_inputs, streams, config):
    """the compressed bytes are this library's own: each must decode to its input by the oracle's
    decoder, and by the device decompressor on the same stream"""
    torch, _, S, _, codec = _mods()[:5]
    xs, _ = snappy_inputs
    s = streams[0]
    data, off, ln = corpus.pack(xs, align=1, lead=3)
    batch = codec.DeviceBatch.from_host(data, off, ln)

    def call(q):
        comp, cst = codec.snappy_compress(batch, stream=q)
        dec, dst = codec.snappy_decompress(comp, stream=q)
        return comp, cst, dec, dst

    comp, cst, dec, dst = S.run(config, call, s)
    assert not S.host(cst, s).any() and not S.host(dst, s).any()
    zb = S.host(comp.data, s)
    zo, zn = S.host(comp.src_off, s).view(np.uint64), S.host(comp.src_len, s).view(np.uint32)
    assert [oracle.snappy_decompress(bytes(zb[int(a): int(a) + int(n)])) for a, n in zip(zo, zn)] == xs
    assert _blocks(S, dec, s) == xs


# ---------------------------------------------------------------- Reader
N_READER = 6000


@pytest.fixture(scope="module")
def reader_case(oracle):
    """about 6 000 records in 1 024-byte blocks, as an uncompressed and as a Snappy file, and 64
    queries of all four kinds with the oracle's answers; max_blocks=1 hands some of them back"""
    rng = np.random.default_rng(64)
    recs = corpus.random_records(rng, N_READER, 0, 30, 0, 120)
    files = {comp: su.write(recs, 1024, 4, comp) for comp in (0, 1)}
    keys = su.probe_keys(rng, recs, n=13)
    qs = []
    for k in keys:
        qs += [("get", k), ("prefix", k[:3]), ("range", k, k + b"\xff"), ("from", k)]
    qs, lim = qs[:64], [7 if q[0] == "from" else None for q in qs[:64]]
    lim[3] = None                                     # one unlimited "from": far more than one block
    assert len(qs) == 64 and {q[0] for q in qs} == {"get", "prefix", "range", "from"}
    exp = [su.expected(oracle, files[0], q, m, True) for q, m in zip(qs, lim)]
    assert [e["records"] for e in exp] == [su.expected(oracle, files[1], q, m, True)["records"] for q, m in zip(qs, lim)]
    got = {k: v for k, v in recs}
    gets = [recs[187 * i][0] for i in range(32)] + [recs[187 * i][0] + b"\x00\x01" for i in range(32)]
    # The first scan_batch of a process pays for loading every kernel it and torch use: measured 508 ms
    # of host time against 31 ms for later calls, and it returned while a 2 s hold of the default
    # stream still ran, so it waits for nothing -- it only outlasts a 200 ms hold.  Pay that once here,
    # on a Reader no test uses; every test builds its own Reader, so all per-Reader work stays under
    # the holds.
    warm = _reader(files[1])[1]
    warm.scan_batch(qs, max_blocks=1, max_records=lim)
    warm.get_batch(gets)
    return files, qs, lim, exp, gets, got


def _reader(data):
    """a fresh Reader per test, so its directory and on-demand table are built under the hold;
    index_regular() first: mtblx_entry_offsets is a documented exception to C6 (module docstring)"""
    reader = _mods()[7]
    r = reader.Reader(data)
    r.index_regular()
    return reader, r


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("comp", [0, 1])
def test_reader_scan_batch(reader_case, streams, comp, config):
    torch, _, S = _mods()[:3]
    files, qs, lim, exp, _, _ = reader_case
    rd, r = _reader(files[comp])
    sb = S.run(config, lambda st: r.scan_batch(qs, max_blocks=1, max_records=lim, stream=st), streams[0])
    assert 1 <= sb.n_large < len(qs) and sb.n_fallback == 0 and not sb.served_by_kernel(3)
    for i, (q, e) in enumerate(zip(qs, exp)):
        su.check(rd, sb, i, e, q)
    if comp:
        assert r.table_mode == "on-demand" and 0 < r.stage_stats["resident_blocks"]


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("comp", [0, 1])
def test_reader_count_batch(reader_case, streams, comp, config):
    from mtblx import _lib
    torch, _, S = _mods()[:3]
    files, qs, lim, exp, _, _ = reader_case
    s = streams[0]
    rd, r = _reader(files[comp])
    st, nrec, kb, vb = (S.host(t, s) for t in S.run(config, lambda q: r.count_batch(qs, max_blocks=1, stream=q), s))
    assert (st == _lib.SCAN_LARGE).sum() >= 1 and (st == _lib.SCAN_OK).sum() >= 1
    for i, (q, m, e) in enumerate(zip(qs, lim, exp)):
        if st[i] != _lib.SCAN_OK:
            assert st[i] == _lib.SCAN_LARGE and nrec[i] == 0, q
        elif m is None:   # count_batch applies no limit: compare where the oracle's answer is unlimited too
            assert nrec[i] == len(e["records"]), q
            assert kb[i] == sum(len(k) for k, _ in e["records"]) and vb[i] == sum(len(v) for _, v in e["records"]), q


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("comp", [0, 1])
def test_reader_get_batch(reader_case, streams, comp, config):
    """uncompressed get_batch is asynchronous; the compressed one synchronises for its table"""
    from mtblx import _lib
    torch, _, S = _mods()[:3]
    files, _, _, _, gets, got = reader_case
    s = streams[0]
    rd, r = _reader(files[comp])
    st, vo, vl = S.run(config, lambda q: r.get_batch(gets, stream=q), s, asynchronous=comp == 0)
    st, vo, vl = (S.host(t, s) for t in (st, vo, vl))
    src = S.host(r.value_source, s)
    assert len(st) == len(gets) == 64
    for i, k in enumerate(gets):
        if k in got:
            assert st[i] == _lib.GET_FOUND and bytes(src[int(vo[i]): int(vo[i]) + int(vl[i])]) == got[k], k
        else:
            assert st[i] == _lib.GET_NONE, k
    assert sum(k in got for k in gets) >= 8 and sum(k not in got for k in gets) >= 8


# ---------------------------------------------------------------- encode and Writer
@pytest.fixture(scope="module")
def writer_case(oracle):
    rng = np.random.default_rng(5)
    recs = corpus.random_records(rng, 3000, 0, 60, 0, 300)
    return recs, oracle.write_file(recs, 1024, 16)


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("keep", [False, True])
def test_plan_and_encode_blocks(writer_case, streams, keep, config):
    """the framed blocks are the oracle Writer's data region, byte for byte"""
    torch, _, S, _, codec, encode = _mods()[:6]
    recs, want = writer_case
    s = streams[0]
    d = encode.DeviceRecords.from_list(recs)

    def call(st):
        if keep:
            blk, kept = encode.plan(d, 1024, 16, stream=st, keep=True)
        else:
            blk, kept = encode.plan(d, 1024, 16, stream=st), None
        return encode.encode_blocks(d, blk, 16, True, stream=st, plan=kept)

    e = S.run(config, call, s)
    e.check()
    n = int(S.host(e.totals, s)[0])
    index_off = int.from_bytes(want[len(want) - 512: len(want) - 504], "little")
    assert n == index_off and S.host(e.out, s)[:n].tobytes() == want[:n]
    assert not S.host(e.status, s).any()


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("snappy", [False, True])
def test_write_file(oracle, writer_case, streams, snappy, config):
    """None: the oracle Writer's file byte for byte; Snappy: the oracle Reader decodes the records"""
    torch, mtblx, S, _, codec, encode = _mods()[:6]
    recs, want = writer_case
    s = streams[0]
    d = encode.DeviceRecords.from_list(recs)
    comp = mtblx.CompressionType.Snappy if snappy else mtblx.CompressionType.None_
    f = S.run(config, lambda st: encode.write_file(d, 1024, 16, stream=st, compression=comp), s, device_wide=True)
    f = S.host(f, s).tobytes()
    if snappy:
        scan = oracle.file_scan(f, verify=True)
        assert scan["err"] == oracle.ERR_NAMES[0] and scan["records"] == recs
        assert int.from_bytes(f[len(f) - 512 + 16: len(f) - 512 + 24], "little") == 1   # footer: compression
    else:
        assert f == want


# ---------------------------------------------------------------- merge and sort
@pytest.fixture(scope="module")
def merge_case():
    """5 overlapping sources (one empty, one of a single record) and 65 tiny ones, with what the
    Merger promises for them (tests/test_merger_gpu.py::promised, the model's canonical form)"""
    from test_merger_gpu import _random_sources, promised
    five = _random_sources(5, 600, 105)
    rng = np.random.default_rng(65)
    tiny = [sorted({(b"t%03d" % int(k), bytes([i])) for k in rng.integers(0, 200, 6)}) for i in range(65)]
    tiny = [[(k, v) for j, (k, v) in enumerate(t) if not j or t[j - 1][0] != k] for t in tiny]
    u64 = [[(k, (1000 * i + j).to_bytes(8, "little")) for j, (k, _) in enumerate(src)] for i, src in enumerate(five)]
    out = {}
    for name, srcs in (("five", five), ("tiny", tiny), ("u64", u64)):
        want = promised(srcs)
        assert mm.canon(want) == mm.canon(mm.multi_iter(srcs))
        out[name] = (srcs, want)
    return out


def _dev_sources(srcs):
    encode = _mods()[5]
    return [encode.DeviceRecords.from_list(s) for s in srcs]


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("mode", ["groups", "concat", "first", "last", "sum"])
def test_merge_records(merge_case, streams, mode, config):
    torch, mtblx, S, _, codec, encode, merger = _mods()[:7]
    srcs, want = merge_case["u64" if mode == "sum" else "five"]
    d = _dev_sources(srcs)
    m = mtblx.Reduce("sum") if mode == "sum" else mode
    r = S.run(config, lambda st: merger.merge_records(d, m, stream=st), streams[0])
    if mode == "groups":
        assert r.to_list() == want
    else:
        pick = U.sum_u64 if mode == "sum" else U.PICK[mode]
        assert merger._records_list(r) == U.merged(want, pick)


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("mode", ["groups", "concat"])
def test_merge_all_65_sources(merge_case, streams, mode, config):
    """two rounds of 64; "groups" goes through the two-CONCAT regrouping between them"""
    torch, mtblx, S, _, codec, encode, merger = _mods()[:7]
    srcs, want = merge_case["tiny"]
    d = _dev_sources(srcs)
    r = S.run(config, lambda st: merger.merge_all(d, mode, stream=st), streams[0])
    if mode == "groups":
        assert r.to_list() == want
    else:
        assert merger._records_list(r) == [(k, b"".join(vs)) for k, vs in want]


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("mode", ["groups", "last"])
def test_merge_segments(merge_case, streams, mode, config):
    """every source cut into 3 segments at the same two keys: segment q of the result is the merge
    of segment q of every source"""
    import bisect
    torch, mtblx, S, _, codec, encode, merger = _mods()[:7]
    from test_merger_gpu import promised
    srcs, _ = merge_case["five"]
    s = streams[0]
    allk = sorted({k for src in srcs for k, _ in src})
    cuts = [allk[len(allk) // 3], allk[2 * len(allk) // 3]]
    offs, segs = [], [[], [], []]
    for src in srcs:
        ks = [k for k, _ in src]
        o = [0] + [bisect.bisect_left(ks, c) for c in cuts] + [len(ks)]
        offs.append(torch.tensor(o, dtype=torch.int64, device="cuda"))
        for q in range(3):
            segs[q].append(src[o[q]: o[q + 1]])
    d = _dev_sources(srcs)
    r, seg_end = S.run(config, lambda st: merger.merge_segments(d, offs, mode, stream=st), s)
    want = [promised(x) for x in segs]
    assert S.host(seg_end, s).tolist() == np.cumsum([len(w) for w in want]).tolist()
    flat = [g for w in want for g in w]
    if mode == "groups":
        assert r.to_list() == flat
    else:
        assert merger._records_list(r) == [(k, vs[-1]) for k, vs in flat]


@pytest.fixture(scope="module")
def merger_files(merge_case):
    srcs, want = merge_case["five"]
    return [mm.make_source(x, 1024) for x in srcs], want


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("surface", ["groups", "records", "write_file"])
def test_merger_on_a_stream(oracle, merger_files, streams, surface, config):
    """Merger(stream=s) scans its sources on s (Reader.iter() of fresh Readers, under the hold)"""
    torch, mtblx, S, _, codec, encode, merger, reader = _mods()[:8]
    files, want = merger_files
    s = streams[0]
    readers = [reader.Reader(f) for f in files]
    model = [(k, b"".join(vs)) for k, vs in want]
    assert all(r.index_regular() for r in readers)   # mtblx_entry_offsets, the exception to C6: before the hold

    def call(st):
        m = merger.Merger(readers, "concat", stream=st)
        return m.groups() if surface == "groups" else m.records() if surface == "records" else m.write_file(1024, 16)

    r = S.run(config, call, s, device_wide=surface == "write_file")
    if surface == "groups":
        assert r.to_list() == want
    elif surface == "records":
        assert merger._records_list(r) == model
    else:
        assert S.host(r, s).tobytes() == oracle.write_file(model, 1024, 16)


@pytest.fixture(scope="module")
def merger_scan_case(oracle):
    datas, lists, qs = U.small_sources(1024, False)
    qs = qs[:40]
    exp = []
    for q in qs:
        per = U.per_source(oracle, datas, q, ("streams", 1024))
        exp.append(U.promised_groups(per))
    return datas, qs, exp


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("how", ["argument", "constructor"])
def test_merger_scan_batch(merger_scan_case, streams, how, config):
    """Merger.scan_batch(..., stream=s) and Merger(stream=s).scan_batch(...): the sources' scans, the
    segmented merge and the seek-path answers (max_blocks=1 hands some queries back) on s"""
    torch, mtblx, S, _, codec, encode, merger, reader = _mods()[:8]
    datas, qs, exp = merger_scan_case
    readers = []
    for d in datas:
        r = reader.Reader(d)
        r.index_regular()          # mtblx_entry_offsets: the documented exception to C6, before the hold
        readers.append(r)

    def call(st):
        if how == "argument":
            return merger.Merger(readers, "concat").scan_batch(qs, max_blocks=1, stream=st)
        return merger.Merger(readers, "concat", stream=st).scan_batch(qs, max_blocks=1)

    res = S.run(config, call, streams[0])
    served = [res.served_by_kernel(q) for q in range(len(qs))]
    assert any(served) and not all(served)
    count = S.host(res.count, streams[0])
    for q, want in enumerate(exp):
        assert res.records(q) == U.merged(want, U.PICK["concat"]), qs[q]
        assert int(count[q]) == len(want)
    q = served.index(True)
    assert merger._records_list(res.device_records(q)) == U.merged(exp[q], U.PICK["concat"])


@pytest.fixture(scope="module")
def sort_case():
    from test_sorter_gpu import _dup_records, promised
    records = _dup_records(3000, 31)
    return records, promised(records)


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("mode", ["groups", "concat"])
def test_sort_records(sort_case, streams, mode, config):
    torch, mtblx, S, _, codec, encode, merger, reader, sorter = _mods()
    records, want = sort_case
    d = encode.DeviceRecords.from_list(records)
    r = S.run(config, lambda st: sorter.sort_records(d, mode, stream=st), streams[0])
    if mode == "groups":
        assert r.to_list() == want
    else:
        assert merger._records_list(r) == [(k, b"".join(vs)) for k, vs in want]


N_SORTER = 6144 + 500


@pytest.fixture(scope="module")
def sorter_case(oracle):
    """6144 + 500 entries of 8 B key + 1016 B value: with max_memory at its minimum the 6144th insert
    cuts, so the Sorter holds two chunks; a third of the second chunk's keys repeat the first's"""
    from test_sorter_gpu import _host_batch, promised
    rng = np.random.default_rng(18)
    keys = np.concatenate([rng.permutation(6144), rng.permutation(6144)[:500]])
    records = [(b"%08d" % k, (b"%07d:" % i) * 127) for i, k in enumerate(keys)]
    want = [(k, b"".join(vs)) for k, vs in promised(records)]
    return _host_batch(records), want, oracle.write_file(want, 8192, 16)


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("how", ["host", "device"])
def test_sorter_two_chunks_write_file(sorter_case, streams, how, config):
    """Sorter(stream=s): the staging of the inserted batches (host arrays, or device tensors that
    are ready before the hold), both chunk sorts, the merge and the Writer on s"""
    torch, mtblx, S, _, codec, encode, merger, reader, sorter = _mods()
    (ks, ke, vs, ve), want, file = sorter_case
    s = streams[0]
    batch = (ks, ke, vs, ve)
    if how == "device":
        batch = tuple(torch.from_numpy(np.array(x)).cuda() for x in (ks, ke.astype(np.int64), vs, ve.astype(np.int64)))
    made = []

    def call(st):
        so = sorter.Sorter.builder("concat", stream=st).max_memory(0).build()
        made.append(so)
        so.insert_batch(*batch)
        return so.write_file(8192, 16)

    f = S.run(config, call, s, device_wide=True)
    assert made[0].chunk_sizes == [6144, 500] and made[0].merges == 0
    assert S.host(f, s).tobytes() == file


# ---------------------------------------------------------------- two calls at once
def test_two_calls_on_two_streams(reader_case, merge_case, streams):
    """re-entrancy: Reader.scan_batch on s1 and merge_records on s2, issued back to back with no
    synchronise in between, each behind a hold on its own stream so that both are in flight at
    once; each owns its workspace (the shared-workspace rule is test_workspace_one_launch_at_a_time's)"""
    torch, mtblx, S, _, codec, encode, merger = _mods()[:7]
    files, qs, lim, exp, _, _ = reader_case
    srcs, want = merge_case["five"]
    s1, s2 = streams
    rd, r = _reader(files[1])
    d = _dev_sources(srcs)
    torch.cuda.synchronize()
    S.hold(s1, 50)
    S.hold(s2, 50)
    sb = r.scan_batch(qs, max_blocks=1, max_records=lim, stream=s1)
    g = merger.merge_records(d, "groups", stream=s2)
    for i, (q, e) in enumerate(zip(qs, exp)):
        su.check(rd, sb, i, e, q)
    assert g.to_list() == want


# ---------------------------------------------------------------- C3 by the allocator's own record
def _alloc_streams(torch, fn):
    """the streams of every allocation the caching allocator made during fn(), from its history"""
    torch.cuda.synchronize()
    torch.cuda.memory._record_memory_history(enabled="all", context=None, stacks="python")
    try:
        before = sum(len(t) for t in torch.cuda.memory._snapshot()["device_traces"])
        out = fn()
        traces = [e for t in torch.cuda.memory._snapshot()["device_traces"] for e in t][before:]
    finally:
        torch.cuda.memory._record_memory_history(enabled=None)
    return out, [e for e in traces if e.get("action") == "alloc"]


@pytest.mark.parametrize("surface", ["scan_batch", "decode_blocks", "plan", "merge_records"])
def test_allocations_are_on_the_call_stream(cfg2, reader_case, writer_case, merge_case, streams, surface):
    """every block the caching allocator hands out during the call belongs to `stream`: this reaches
    the temporaries freed on return and the allocations made after an internal synchronise, which
    no hold can show"""
    torch, mtblx, S, _, codec, encode, merger = _mods()[:7]
    s = streams[0]
    if surface == "scan_batch":
        files, qs, lim, _, _, _ = reader_case
        r = _reader(files[1])[1]
        fn = lambda: r.scan_batch(qs, max_blocks=1, max_records=lim, stream=s)   # noqa: E731
    elif surface == "decode_blocks":
        fn = lambda: codec.decode_blocks(cfg2[0], stream=s)                       # noqa: E731
    elif surface == "plan":
        d = encode.DeviceRecords.from_list(writer_case[0])
        fn = lambda: encode.plan(d, 1024, 16, stream=s, keep=True)                # noqa: E731
    else:
        d = _dev_sources(merge_case["five"][0])
        fn = lambda: merger.merge_records(d, "groups", stream=s)                  # noqa: E731
    _, allocs = _alloc_streams(torch, fn)
    s.synchronize()
    assert allocs and all("stream" in e for e in allocs), "the allocator recorded no usable history"
    assert {e["stream"] for e in allocs} == {s.cuda_stream}

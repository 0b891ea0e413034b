"""Aggregating scans on the GPU: Reader.reduce_batch (mtblx_scan_reduce), reduce_segments
(mtblx_reduce_segments) and Merger.reduce_batch.

Expected values never come from the code under test: per query they are Reduce.fold (pinned by hand
in tests/test_scan_reduce.py) over the records oracle.file_scan yields (scan_util.expected); for the
merged view, Reduce.fold over the model of tests/merger_scan_util.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import corpus
import merger_scan_util as msu
import scan_util as su

pytestmark = pytest.mark.gpu

M = (1 << 64) - 1
# name -> (block size, restart interval, compression)
FILES = {"1024-4": (1024, 4, 0), "256-1": (256, 1, 0), "1024-4-snappy": (1024, 4, 1), "2048-3-zlib": (2048, 3, 2)}
OPS = {1: ("sum",), 3: ("sum", "min", "max"), 8: ("sum", "min", "max", "max", "min", "sum", "sum", "min")}


def _mods():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mtblx import reader
    return reader


def _reader(data, verify=True):
    rd = _mods()
    return rd, rd.ReaderBuilder().verify_checksums(verify).read(data)


def _red(F):
    from mtblx import Reduce
    return Reduce(*OPS[F])


def _values(rng, n, F):
    """n values of F random u64, the top bit set in a third of the words; about 3 % of other lengths"""
    W = 8 * F
    odd = [0, W - 1, W + 1, 200] + ([8] if W != 8 else [])
    out = []
    for _ in range(n):
        if rng.random() < 0.03:
            out.append(rng.integers(0, 256, odd[int(rng.integers(0, len(odd)))], dtype=np.uint8).tobytes())
            continue
        w = rng.integers(0, 1 << 62, F, dtype=np.uint64)
        w |= (rng.random(F) < 0.33).astype(np.uint64) << np.uint64(63)
        w[rng.random(F) < 0.05] = M
        out.append(w.astype("<u8").tobytes())
    return out


@functools.lru_cache(maxsize=None)
def _case(name, F):
    """-> (data, records, queries, limits): 4000 random keys, values of F fields, su.queries_for's queries"""
    bs, iv, comp = FILES[name]
    rng = np.random.default_rng(100 * F + bs + iv + comp)
    keys = [k for k, _ in corpus.random_records(rng, 4000, 0, 30, 0, 0)]
    recs = list(zip(keys, _values(rng, len(keys), F)))
    qs, lim = su.queries_for(su.probe_keys(rng, recs))
    return su.write(recs, bs, iv, comp), recs, qs, lim


def _fold(red, exp):
    return red.fold([v for _, v in exp["records"]])


def _check(oracle, rb, red, data, qs, lim, verify, tag):
    """every query's (values, nrec, nbad) against the model; -> the expectations"""
    assert rb.nq == len(qs) and tuple(rb.fields.shape) == (len(qs), len(red.ops))
    assert rb.nrec.numel() == rb.nbad.numel() == rb.status.numel() == len(qs)
    exps = []
    for i, (q, m) in enumerate(zip(qs, lim)):
        e = su.expected(oracle, data, q, m, verify, tag=tag)
        want = _fold(red, e)
        assert (rb.values(i),) + rb.counts(i) == want, (i, q, m)
        vb = rb.value_bytes(i)
        assert (vb is None) == (want[1] == want[2])
        if vb is not None:
            assert vb == b"".join(x.to_bytes(8, "little") for x in want[0])
        exps.append(e)
    return exps


# ---------------------------------------------------------------- 1. files, fields, verify
@pytest.mark.parametrize("verify", [True, False])
@pytest.mark.parametrize("F", [1, 3, 8])
@pytest.mark.parametrize("name", list(FILES))
def test_files(oracle, name, F, verify):
    from mtblx import _lib
    data, recs, qs, lim = _case(name, F)
    red = _red(F)
    rd, r = _reader(data, verify)
    rb = r.reduce_batch(qs, red, max_records=lim)
    exps = _check(oracle, rb, red, data, qs, lim, verify, (name, F))
    assert rb.n_fallback == 0 and rb.n_large < len(qs) // 2
    assert any(_fold(red, e)[2] for e in exps)                       # limits and ranges that land on bad values
    assert any(not e["records"] for e in exps)
    # nrec is count_batch's where the kernel served an unlimited query
    st, n, _, _ = (t.cpu().numpy() for t in r.count_batch(qs))
    nrec = rb.nrec.cpu().numpy()
    status = rb.status.cpu().numpy()
    for i, m in enumerate(lim):
        assert rb.served_by_kernel(i) == (status[i] == _lib.SCAN_OK)
        assert rb.end(i) == rd.END_NONE and rb.err(i) == "None"
        if m is None:                      # count_batch takes no limits
            assert status[i] == st[i]
            if st[i] == _lib.SCAN_OK:
                assert nrec[i] == n[i]
    if any(_fold(red, e)[2] for e in exps):
        from mtblx import MergeError
        with pytest.raises(MergeError):
            rb.check()


def test_v1_file(oracle):
    data, recs, qs, lim = _case("1024-4", 3)
    v1 = corpus.to_v1(data)
    red = _red(3)
    for verify in (True, False):
        rd, r = _reader(v1, verify)
        rb = r.reduce_batch(qs[:120], red, max_records=lim[:120])
        _check(oracle, rb, red, v1, qs[:120], lim[:120], verify, None)
        assert rb.n_fallback == 0


# ---------------------------------------------------------------- 2. paths
@pytest.mark.parametrize("name", ["1024-4", "1024-4-snappy"])
def test_handed_back_queries_equal_the_kernel_path(oracle, name):
    """max_blocks=2 hands a share of the queries back, max_blocks=0 every query that opens a block:
    the seek path's records reduced by reduce_segments give what the walk gives"""
    from mtblx import _lib
    data, recs, qs, lim = _case(name, 3)
    red = _red(3)
    rd, r = _reader(data)
    wide = r.reduce_batch(qs, red, max_blocks=1 << 20, max_records=lim)
    assert wide.n_large == 0 and wide.n_fallback == 0
    exps = _check(oracle, wide, red, data, qs, lim, True, (name, 3))
    for mb in (2, 0):
        rb = _reader(data)[1].reduce_batch(qs, red, max_blocks=mb, max_records=lim)
        _check(oracle, rb, red, data, qs, lim, True, (name, 3))
        st = rb.status.cpu().numpy()
        assert rb.n_fallback == 0 and rb.n_large == int((st == _lib.SCAN_LARGE).sum())
        assert (rb.fields.cpu() == wide.fields.cpu()).all() and (rb.nrec.cpu() == wide.nrec.cpu()).all()
        assert (rb.nbad.cpu() == wide.nbad.cpu()).all()
        if mb == 2:
            assert 0 < rb.n_large < len(qs)
        else:   # only a query whose seek runs past the last block opens none
            assert all(not e["records"] for e, s in zip(exps, st) if s == _lib.SCAN_OK)
            assert rb.n_large >= sum(bool(e["records"]) for e in exps) > 0


def test_whole_file_from_one_wave(oracle):
    data, recs, _, _ = _case("1024-4", 3)
    red = _red(3)
    qs = [("from", b""), ("prefix", b""), ("range", b"", b"\xff" * 40)]
    rb = _reader(data)[1].reduce_batch(qs, red, max_blocks=1 << 20)
    want = red.fold([v for _, v in recs])
    assert want[2] > 50 and want[1] == len(recs)
    for i in range(3):
        assert (rb.values(i),) + rb.counts(i) == want
    assert rb.n_large == 0 and rb.n_fallback == 0 and all(rb.served_by_kernel(i) for i in range(3))


def test_checksum_mismatch_reports_through_end(oracle):
    """verify on and one flipped content byte: a query whose iteration opens that block is FALLBACK;
    end(q) / err(q) say how the reference's iteration ends (a panic), and the records before it are
    reduced"""
    import test_seek_gpu as ts
    from mtblx import _lib
    rng = np.random.default_rng(43)
    red = _red(3)
    keys = [k for k, _ in corpus.random_records(rng, 3000, 1, 24, 0, 0)]
    recs = list(zip(keys, _values(rng, len(keys), 3)))
    data, (off, ln) = ts._write(recs, 1024, 4)
    b = off.size // 2
    d = bytearray(data)
    d[int(off[b]) + int(ln[b]) // 2] ^= 0x40
    bad = bytes(d)
    rd, r = _reader(bad, True)
    qs, lim = su.queries_for(su.probe_keys(rng, recs, 24))
    rb = r.reduce_batch(qs, red, max_blocks=1 << 20, max_records=lim)
    sb = r.scan_batch(qs, max_blocks=1 << 20, max_records=lim)
    st = rb.status.cpu().numpy()
    hit = some = 0
    errs = (rd.END_ERR_OPEN, rd.END_ERR_NEXT)
    for i, (q, m) in enumerate(zip(qs, lim)):
        e = su.expected(oracle, bad, q, m, True)
        assert (rb.values(i),) + rb.counts(i) == _fold(red, e), (q, m)
        assert (st[i] == _lib.SCAN_FALLBACK) == (e["end"] == rd.END_PANIC)
        assert rb.end(i) == e["end"] == sb.scan(i).end
        assert (rb.err(i) if rb.end(i) in errs else None) == (e["err"] if e["end"] in errs else None)
        assert rb.served_by_kernel(i) == (e["end"] != rd.END_PANIC)
        hit += e["end"] == rd.END_PANIC
        some += e["end"] == rd.END_PANIC and len(e["records"]) > 0
    assert 0 < hit < len(qs) and some


def test_empty_batch_and_tiny_files(oracle):
    red = _red(3)
    data, recs, qs, lim = _case("256-1", 3)
    rb = _reader(data)[1].reduce_batch([], red)
    assert rb.nq == 0 and tuple(rb.fields.shape) == (0, 3) and rb.nrec.numel() == 0 and rb.n_large == 0
    rb.check()
    one = (b"only", b"".join(x.to_bytes(8, "little") for x in (5, 6, 7)))
    for n in (0, 1):
        data = su.write([one][:n])
        qs = [("from", b""), ("prefix", b""), ("prefix", b"on"), ("get", b"only"), ("get", b"onlx"),
              ("range", b"a", b"z"), ("range", b"p", b"z"), ("from", b"zz")]
        rb = _reader(data)[1].reduce_batch(qs, red)
        _check(oracle, rb, red, data, qs, [None] * len(qs), True, None)
        assert rb.n_fallback == 0 and rb.n_large == 0
        if n:
            assert rb.values(3) == (5, 6, 7) and rb.counts(3) == (1, 0) and rb.values(4) == (0, M, 0)


def test_reader_argument_errors():
    data, recs, qs, lim = _case("256-1", 3)
    red = _red(3)
    r = _reader(data)[1]
    for q in [("scan", b"k")], [("range", b"a")], [("get", b"a", b"b")]:
        with pytest.raises(ValueError, match="bad query"):
            r.reduce_batch(q, red)
    with pytest.raises(ValueError, match="one per query"):
        r.reduce_batch([("get", b"a"), ("get", b"b")], red, max_records=[1])
    with pytest.raises(ValueError, match="negative"):
        r.reduce_batch([("get", b"a")], red, max_records=-1)
    with pytest.raises(ValueError, match="not a Reduce"):
        r.reduce_batch([("get", b"a")], "first")


def test_irregular_index(oracle):
    """an index block whose restart entries carry shared != 0: every query goes through the seek path
    and reduce_segments"""
    import test_seek_gpu as ts
    data, recs, qs, lim = _case("256-1", 3)
    red = _red(3)
    rd = _mods()
    rng = np.random.default_rng(12)
    seen = 0
    for _ in range(4):
        bad = ts._corrupt_index(data, rng, "restart")
        try:
            r = rd.ReaderBuilder().verify_checksums(False).read(bad)
        except (rd.MtblError, rd.ReferencePanic):
            continue
        if r.index_regular():
            continue
        seen += 1
        rb = r.reduce_batch(qs[:45], red, max_records=lim[:45])
        sb = r.scan_batch(qs[:45], max_records=lim[:45])
        assert rb.n_fallback == 45 and not any(rb.served_by_kernel(i) for i in range(45))
        for i, (q, m) in enumerate(zip(qs[:45], lim[:45])):
            e = su.expected(oracle, bad, q, m, False)
            assert (rb.values(i),) + rb.counts(i) == _fold(red, e), q
            assert rb.end(i) == sb.scan(i).end
        break
    assert seen


# ---------------------------------------------------------------- 3. shapes
@pytest.mark.parametrize("nq", [1, 63, 64, 65, 257])
def test_batch_sizes(oracle, nq):
    data, recs, qs, lim = _case("1024-4", 3)
    red = _red(3)
    sel = [(5 * i) % len(qs) for i in range(nq)]
    q2, l2 = [qs[i] for i in sel], [lim[i] for i in sel]
    rb = _reader(data)[1].reduce_batch(q2, red, max_records=l2)
    _check(oracle, rb, red, data, q2, l2, True, ("1024-4", 3))
    assert rb.n_fallback == 0


def test_same_query_65_times(oracle):
    data, recs, qs, lim = _case("1024-4", 8)
    red = _red(8)
    q = next(q for q, m in zip(qs, lim) if q[0] == "prefix" and
             3 < len(su.expected(oracle, data, q, None, True, tag=("1024-4", 8))["records"]) < 200)
    rb = _reader(data)[1].reduce_batch([q] * 65, red)
    _check(oracle, rb, red, data, [q] * 65, [None] * 65, True, ("1024-4", 8))
    assert rb.n_fallback == 0 and rb.n_large == 0 and rb.values(0) == rb.values(64)


@pytest.mark.parametrize("F", [1, 3])
def test_value_placement(oracle, F):
    """key lengths 1 .. 8 with restart interval 1, so that the values' offsets walk through all
    eight byte alignments; the last value of every block ends where the block's entries end"""
    rng = np.random.default_rng(7 + F)
    red = _red(F)
    recs = []
    for i in range(1600):
        key = bytes([1 + i // 8]) + b"\x01" * (i % 8)
        recs.append((key, rng.integers(1, 1 << 63, F, dtype=np.uint64).astype("<u8").tobytes()))
    assert recs == sorted(recs) and len({k for k, _ in recs}) == len(recs)
    data = su.write(recs, 512, 1)
    assert {data.index(v) % 8 for _, v in recs} == set(range(8))
    ikeys = [k for k, _ in oracle.index_records(data)]
    assert len(ikeys) > 20
    qs = [("from", b""), ("prefix", b"\x01"), ("range", recs[100][0], recs[1500][0])]
    qs += [("get", k) for k, _ in recs[:64]] + [("range", k, k + b"\x01\x01\x01") for k, _ in recs[500:540]]
    qs += [("range", recs[0][0], k) for k in ikeys[:12]]           # ends on a block's last record
    rb = _reader(data)[1].reduce_batch(qs, red, max_blocks=1 << 20)
    _check(oracle, rb, red, data, qs, [None] * len(qs), True, None)
    assert rb.n_large == 0 and rb.n_fallback == 0 and rb.counts(0) == (1600, 0)


# ---------------------------------------------------------------- 4. raw ABI: the workspace is left planned
def test_emit_after_scan_reduce(oracle):
    """mtblx_scan_emit over the workspace mtblx_scan_reduce left writes the records scan_batch gives"""
    import test_scan_batch_gpu as tsb
    from mtblx import _lib
    name = "1024-4"
    data, recs, qs, lim = _case(name, 3)
    qs = qs[:90]
    red = _red(3)
    rd, r = _reader(data)
    res, totals, ws, wsb, _, _, _, (fields, nbad) = r._scan_plan(qs, 64, None, None, red)
    nrec, kb, vb, nbadq = totals
    exp = [su.expected(oracle, data, q, None, True, tag=(name, 3)) for q in qs]
    host = np.frombuffer(res.cpu().numpy().tobytes(), np.dtype(_lib.ScanResult))[: len(qs)]
    ok = host["status"] == _lib.SCAN_OK
    assert nbadq == int((~ok).sum()) and nrec == sum(len(e["records"]) for e, o in zip(exp, ok) if o) and nrec > 0
    f, nb = fields.cpu().numpy().view(np.uint64), nbad.cpu().numpy()
    for i, e in enumerate(exp):
        want = _fold(red, e) if ok[i] else ((0, 0, 0), 0, 0)       # not OK: zero fields, zero nbad, zero counts
        assert (tuple(int(x) for x in f[i]), int(host["nrec"][i]), int(nb[i])) == want
    fl, (k, v, ke, ve), intact = tsb._emit(r, len(qs), ws, wsb, kb, vb, nrec)
    assert fl == 0 and intact
    want = [x for e, o in zip(exp, ok) if o for x in e["records"]]
    assert k[:kb].tobytes() == b"".join(x[0] for x in want) and v[:vb].tobytes() == b"".join(x[1] for x in want)
    ve = ve[: 8 * nrec].view(np.uint64)
    assert list(np.diff(np.concatenate([[0], ve]))) == [len(x[1]) for x in want]
    sb = r.scan_batch(qs)
    assert [sb.records(i) for i in range(len(qs)) if ok[i]] == [e["records"] for e, o in zip(exp, ok) if o]


# ---------------------------------------------------------------- 5. reduce_segments
def _device_records(values, lead=3):
    """values on the device, the vals tensor sliced at an odd offset of its allocation"""
    import torch
    from mtblx.encode import DeviceRecords
    blob = b"\xee" * lead + b"".join(values)
    buf = torch.frombuffer(bytearray(blob or b"\0"), dtype=torch.uint8).cuda()
    ve = torch.from_numpy(np.cumsum([len(v) for v in values], dtype=np.int64) if values else np.zeros(0, np.int64)).cuda()
    z = torch.zeros(0, dtype=torch.uint8, device="cuda")
    return DeviceRecords(z, ve.clone(), buf[lead:], ve)


def _segments_case():
    from mtblx import _lib
    T = int(_lib.lib().mtblx_reduce_seg_tile())
    assert T == _lib.REDUCE_SEG_TILE and T % 256 == 0
    per, n = T // 256, 5 * T + 880                 # records per thread; about 6000 records at T = 1024
    rng = np.random.default_rng(77)
    vals = _values(rng, n, 3)
    segs = [(0, 0), (0, 1),                        # empty; one record, the tile's first
            (1, per), (per, per),                  # inside one thread's run; empty
            (per + 1, 40), (40, 300),              # across lanes; across waves
            (310, T + 5), (T + 5, T + 5),          # 300 .. 310 unowned; across a tile edge; empty
            (T + 10, 4 * T + 7),                   # across four tiles, two whole tiles inside
            (4 * T + 7, 4 * T + 7), (4 * T + 7, 4 * T + 8),
            (5 * T, 5 * T + 20),                   # starts on a tile's first record
            (5 * T + 100, n), (n, n)]              # ends on the last record; empty at the end
    for i in range(5 * T, 5 * T + 20):             # a MIN field whose good values are all 2^64 - 1
        w = np.frombuffer(vals[i], "<u8").copy() if len(vals[i]) == 24 else np.zeros(3, "<u8")
        w[1] = M
        vals[i] = w.tobytes()
    vals[5 * T + 3] = b"bad"
    for i in (2, 45, 299, T - 1, T, 2 * T + 1, 3 * T, n - 1):   # bad lengths inside several segments
        vals[i] = b"x" * (25 if i % 2 else 23)
    for i in range(40, 300):                       # a sum that wraps many times
        if len(vals[i]) == 24:
            w = np.frombuffer(vals[i], "<u8").copy()
            w[0] |= np.uint64(1 << 63)
            vals[i] = w.tobytes()
    return T, n, vals, segs


def _seg_check(red, vals, segs, fields, nbad):
    f, nb = fields.cpu().numpy().view(np.uint64), nbad.cpu().numpy()
    assert f.shape == (len(segs), len(red.ops)) and nb.shape == (len(segs),)
    for s, (lo, hi) in enumerate(segs):
        want = red.fold(vals[lo:hi])
        assert (tuple(int(x) for x in f[s]), int(nb[s])) == (want[0], want[2]), (s, lo, hi)


def test_reduce_segments_every_boundary():
    _mods()
    from mtblx import reduce_segments
    T, n, vals, segs = _segments_case()
    red = _red(3)
    rec = _device_records(vals)
    assert rec.vals.data_ptr() % 2 == 1
    fields, nbad = reduce_segments(rec, [a for a, _ in segs], [b for _, b in segs], red)
    _seg_check(red, vals, segs, fields, nbad)
    want = [red.fold(vals[a:b]) for a, b in segs]
    assert want[5][0][0] != sum(int.from_bytes(v[:8], "little") for v in vals[40:300] if len(v) == 24)   # it wrapped
    assert want[11][0][1] == M and want[11][2] == 1 and sum(w[2] for w in want) >= 8
    # one segment over everything; every record its own segment; thread-sized segments
    for sg in ([(0, n)], [(i, i + 1) for i in range(n)], [(i, min(i + T // 256, n)) for i in range(0, n, T // 256)],
               [(i, min(i + 7, n)) for i in range(0, n, 11)]):
        f, nb = reduce_segments(rec, [a for a, _ in sg], [b for _, b in sg], red)
        _seg_check(red, vals, sg, f, nb)
    # the other field counts on the same bytes
    for F in (1, 8):
        r2 = _red(F)
        v2 = _values(np.random.default_rng(F), 2 * T + 3, F)
        sg = [(0, 5), (5, T + 1), (T + 1, 2 * T + 3)]
        f, nb = reduce_segments(_device_records(v2, lead=1), [a for a, _ in sg], [b for _, b in sg], r2)
        _seg_check(r2, v2, sg, f, nb)


def test_reduce_segments_nothing_to_do():
    import torch
    _mods()
    from mtblx import reduce_segments
    red = _red(3)
    T, n, vals, segs = _segments_case()
    f, nb = reduce_segments(_device_records(vals), [], [], red)                  # nseg = 0
    assert tuple(f.shape) == (0, 3) and nb.numel() == 0
    f, nb = reduce_segments(_device_records([]), [0, 0], [0, 0], red)            # n = 0: the identities
    assert f.cpu().numpy().view(np.uint64).tolist() == [[0, M, 0]] * 2 and nb.tolist() == [0, 0]
    lo = torch.tensor([3, 9], dtype=torch.int64, device="cuda")                  # device tensors as they are
    f, nb = reduce_segments(_device_records(vals), lo, lo + 4, red)
    _seg_check(red, vals, [(3, 7), (9, 13)], f, nb)


@pytest.mark.parametrize("segs", [[(10, 20), (5, 8)], [(0, 5), (3, 8)], [(0, 5), (5, 10 ** 6)], [(7, 6)]],
                         ids=["unsorted", "overlapping", "out-of-range", "lo-above-hi"])
def test_reduce_segments_badseg_leaves_the_outputs(segs):
    import torch
    _mods()
    from mtblx import _lib, codec, reduce_segments
    red = _red(3)
    T, n, vals, _ = _segments_case()
    rec = _device_records(vals)
    with pytest.raises(ValueError, match="seg_lo"):
        reduce_segments(rec, [a for a, _ in segs], [b for _, b in segs], red)
    # the raw call: MTBLX_REDUCE_BADSEG in *flags, fields and nbad as they were
    lo = torch.tensor([a for a, _ in segs], dtype=torch.int64, device="cuda")
    hi = torch.tensor([b for _, b in segs], dtype=torch.int64, device="cuda")
    fields = torch.full((len(segs), 3), 0x5555, dtype=torch.int64, device="cuda")
    nbad = torch.full((len(segs),), 0x77, dtype=torch.int64, device="cuda")
    flags = torch.full((2,), 0x33, dtype=torch.int32, device="cuda")
    c = _lib.Records(0, 0, rec.vals.data_ptr(), rec.val_end.data_ptr(), n)
    spec = red.cstruct()
    rc = _lib.lib().mtblx_reduce_segments(C.byref(c), C.c_void_p(lo.data_ptr()), C.c_void_p(hi.data_ptr()), len(segs),
                                          C.byref(spec), C.c_void_p(fields.data_ptr()), C.c_void_p(nbad.data_ptr()),
                                          C.c_void_p(flags.data_ptr()), C.c_void_p(codec._stream_handle(None)))
    assert rc == 0
    torch.cuda.synchronize()
    assert flags.tolist() == [_lib.REDUCE_BADSEG, 0x33]
    assert (fields == 0x5555).all() and (nbad == 0x77).all()


# ---------------------------------------------------------------- 6. the merged view
def _merger(datas, merge):
    rd = _mods()
    from mtblx import merger
    return merger.Merger.builder(merge).extend([rd.Reader(d) for d in datas]).build()


def _merged_expect(oracle, datas, qs, tag, pick, limits=None):
    out = []
    for i, q in enumerate(qs):
        groups = msu.promised_groups(msu.per_source(oracle, datas, q, tag))
        out.append(msu.merged(msu.cut(groups, None if limits is None else limits[i]), pick))
    return out


def _check_merged(rb, red, exp):
    assert rb.nq == len(exp)
    for q, items in enumerate(exp):
        assert (rb.values(q),) + rb.counts(q) == red.fold([v for _, v in items]), q


@pytest.mark.parametrize("bs", [1024, 256])
def test_merger_reduce_batch(oracle, bs):
    from mtblx import Reduce
    datas, lists, qs = msu.small_sources(bs, True)
    red = Reduce("sum")
    tag = ("reduce-small", bs)
    # "concat": most merged values are 16 or 24 bytes long, so they are counted in nbad
    exp = _merged_expect(oracle, datas, qs, tag, msu.PICK["concat"])
    rb = _merger(datas, "concat").reduce_batch(qs, red)
    _check_merged(rb, red, exp)
    assert sum(rb.counts(q)[1] for q in range(len(qs))) > 10
    # the Merger's own Reduce (reduce=None) joins each key's values, then the same spec folds the keys
    exp = _merged_expect(oracle, datas, qs, tag, msu.sum_u64)
    rb = _merger(datas, red).reduce_batch(qs)
    _check_merged(rb, red, exp)
    assert all(rb.counts(q)[1] == 0 for q in range(len(qs)))
    rb.check()
    # "first" under a max: another spec than the merge function
    exp = _merged_expect(oracle, datas, qs, tag, msu.PICK["first"])
    _check_merged(_merger(datas, "first").reduce_batch(qs, Reduce("max")), Reduce("max"), exp)
    # limits: the first m merged items of the unlimited result
    fq = [q for q in qs if q[0] == "from"]
    limits = [[0, 1, 2, 37, None, 5][i % 6] for i in range(len(fq))]
    exp = _merged_expect(oracle, datas, fq, tag, msu.PICK["first"], limits)
    _check_merged(_merger(datas, "first").reduce_batch(fq, red, max_records=limits), red, exp)


def test_merger_reduce_batch_quirk_and_handed_back(oracle):
    import merger_model as mm
    from mtblx import Reduce
    red = Reduce("sum")
    # the empty-key quirk inside every query (values of 8 bytes)
    srcs = [[(k, (100 * s + i).to_bytes(8, "little")) for i, (k, _) in enumerate(r)] for s, r in enumerate(msu.QUIRK_SOURCES)]
    datas = [mm.make_source(r) for r in srcs]
    qs = [q for q, _ in msu.QUIRK_QUERIES]
    limits = [m for _, m in msu.QUIRK_QUERIES]
    exp = _merged_expect(oracle, datas, qs, "reduce-quirk", msu.PICK["last"], limits)
    _check_merged(_merger(datas, "last").reduce_batch(qs, red, max_records=limits), red, exp)
    # max_blocks=1: some queries are handed back by some source and merged by merge_all
    datas, lists, qs = msu.small_sources(256, True)
    exp = _merged_expect(oracle, datas, qs, ("reduce-small", 256), msu.sum_u64)
    rb = _merger(datas, red).reduce_batch(qs, max_blocks=1)
    _check_merged(rb, red, exp)
    served = [rb.served_by_kernel(q) for q in range(len(qs))]
    assert any(served) and not all(served) and rb.n_large > 0


# ---------------------------------------------------------------- 7. streams
@pytest.fixture(scope="module")
def stream_case():
    """the three surfaces run once unheld (which also loads their kernels before any hold, as
    stream_util's docstring asks) -> what the held runs must give"""
    import stream_util as S
    _mods()
    from mtblx import Reduce, reduce_segments
    data, recs, qs, lim = _case("1024-4-snappy", 3)
    qs, lim = qs[:64], lim[:64]
    red = _red(3)
    rb = _reader(data)[1].reduce_batch(qs, red, max_blocks=2, max_records=lim)
    assert 0 < rb.n_large < len(qs)
    want_r = [(rb.values(i),) + rb.counts(i) for i in range(len(qs))]
    datas, lists, mqs = msu.small_sources(1024, True)
    mqs = mqs[:40]
    mb = _merger(datas, Reduce("sum")).reduce_batch(mqs, max_blocks=1)
    want_m = [(mb.values(i),) + mb.counts(i) for i in range(len(mqs))]
    assert not all(mb.served_by_kernel(i) for i in range(len(mqs)))
    T, n, vals, segs = _segments_case()
    f, nb = reduce_segments(_device_records(vals), [a for a, _ in segs], [b for _, b in segs], red)
    _seg_check(red, vals, segs, f, nb)
    return dict(data=data, qs=qs, lim=lim, red=red, want_r=want_r, datas=datas, mqs=mqs, want_m=want_m, vals=vals,
                segs=segs, streams=S.pick_streams(2))


@pytest.mark.parametrize("config", ["current-held", "own-held", "ambient"])
def test_streams_reader_reduce_batch(stream_case, config):
    import stream_util as S
    c = stream_case
    rd, r = _reader(c["data"])
    r.index_regular()          # mtblx_entry_offsets: the documented exception, before the hold
    s = c["streams"][0]
    rb = S.run(config, lambda st: r.reduce_batch(c["qs"], c["red"], max_blocks=2, max_records=c["lim"], stream=st), s)
    assert [(rb.values(i),) + rb.counts(i) for i in range(len(c["qs"]))] == c["want_r"]
    f = S.host(rb.fields, s).view(np.uint64)
    assert [tuple(int(x) for x in row) for row in f] == [w[0] for w in c["want_r"]]


@pytest.mark.parametrize("config", ["current-held", "own-held", "ambient"])
def test_streams_merger_reduce_batch(stream_case, config):
    import stream_util as S
    from mtblx import Reduce, merger
    rd = _mods()
    c = stream_case
    readers = []
    for d in c["datas"]:
        r = rd.Reader(d)
        r.index_regular()
        readers.append(r)
    s = c["streams"][0]
    rb = S.run(config, lambda st: merger.Merger(readers, Reduce("sum")).reduce_batch(c["mqs"], max_blocks=1, stream=st), s)
    assert [(rb.values(i),) + rb.counts(i) for i in range(len(c["mqs"]))] == c["want_m"]


@pytest.mark.parametrize("config", ["current-held", "own-held", "ambient"])
def test_streams_reduce_segments(stream_case, config):
    import stream_util as S
    import torch
    from mtblx import reduce_segments
    c = stream_case
    rec = _device_records(c["vals"])
    lo = torch.tensor([a for a, _ in c["segs"]], dtype=torch.int64, device="cuda")
    hi = torch.tensor([b for _, b in c["segs"]], dtype=torch.int64, device="cuda")
    s = c["streams"][1]
    f, nb = S.run(config, lambda st: reduce_segments(rec, lo, hi, c["red"], stream=st), s)
    with torch.cuda.stream(s):
        _seg_check(c["red"], c["vals"], c["segs"], f, nb)

"""Batched scans on the GPU: Reader.scan_batch / count_batch and the raw mtblx_scan_plan /
mtblx_scan_emit calls against the oracle's restatement of ReaderIntoIter (oracle_file_scan modes
from / get / prefix / range with max_records), one query at a time on the oracle's side and one
batch on the device's."""
import ctypes as C

import numpy as np
import pytest

import corpus
import scan_util as su

pytestmark = pytest.mark.gpu


def _mods():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mtblx import reader
    return reader


def _reader(data, verify=True):
    rd = _mods()
    return rd, rd.ReaderBuilder().verify_checksums(verify).read(data)


def _check_all(oracle, data, qs, lim, verify, tag=None, max_blocks=64):
    rd, r = _reader(data, verify)
    sb = r.scan_batch(qs, max_blocks=max_blocks, max_records=lim)
    assert sb.nq == len(qs) and sb.status.numel() == len(qs) and sb.rec_off.numel() == len(qs) + 1
    for i, (q, m) in enumerate(zip(qs, lim)):
        su.check(rd, sb, i, su.expected(oracle, data, q, m, verify, tag=tag), q)
    return sb


# ---------------------------------------------------------------- 1. well-formed files
@pytest.mark.parametrize("verify", [True, False])
@pytest.mark.parametrize("name", list(su.FILES))
def test_well_formed_files(oracle, name, verify):
    data, recs, qs, lim = su.case(name)
    sb = _check_all(oracle, data, qs, lim, verify, tag=name)
    assert sb.n_fallback == 0          # nothing here may lean on bulk() but the LARGE scans
    st = sb.status.cpu().numpy()
    assert int((st == 0).sum()) + sb.n_large == len(qs) and int((st == 0).sum()) > len(qs) // 2
    assert int(sb.rec_off[-1].item()) == sb.key_end.numel() == sb.val_end.numel()


# ---------------------------------------------------------------- 2. the LARGE rule
@pytest.mark.parametrize("name", list(su.FILES))
def test_large_rule_exact(oracle, name):
    """status == LARGE exactly for the queries that open more than max_blocks = 4 data blocks"""
    from mtblx import _lib
    data, recs, qs, lim = su.case(name)
    keys = [k for k, _ in recs]
    ikeys = [k for k, _ in oracle.index_records(data)]
    rd, r = _reader(data)
    sb = r.scan_batch(qs, max_blocks=4, max_records=lim)
    st = sb.status.cpu().numpy()
    scans = large = 0
    for i, (q, m) in enumerate(zip(qs, lim)):
        e = su.expected(oracle, data, q, m, True, tag=name)
        su.check(rd, sb, i, e, q)
        if q[0] == "from":
            continue
        opened = su.span(ikeys, keys, q, len(e["records"]))[2]
        assert (st[i] == _lib.SCAN_LARGE) == (opened > 4), (q, opened, st[i])
        assert st[i] in (_lib.SCAN_OK, _lib.SCAN_LARGE)
        assert sb.served_by_kernel(i) == (st[i] == _lib.SCAN_OK)
        if q[0] != "get":
            scans += 1
            large += st[i] == _lib.SCAN_LARGE
    assert large <= 0.4 * scans, (large, scans)
    assert sb.n_fallback == 0


# ---------------------------------------------------------------- 3. shapes
@pytest.mark.parametrize("nq", [1, 63, 64, 65, 257])
def test_batch_sizes(oracle, nq):
    data, recs, qs, lim = su.case("random-1024-4")
    sel = [(5 * i) % len(qs) for i in range(nq)]
    sb = _check_all(oracle, data, [qs[i] for i in sel], [lim[i] for i in sel], True, tag="random-1024-4")
    assert sb.n_fallback == 0


def test_same_query_65_times(oracle):
    data, recs, qs, lim = su.case("counter-1024-16")
    q = ("prefix", b"k0123")
    sb = _check_all(oracle, data, [q] * 65, [None] * 65, True, tag="counter-1024-16")
    assert sb.n_fallback == 0 and sb.n_large == 0
    assert sb.records(64) == [x for x in recs if x[0].startswith(b"k0123")]


def test_block_boundaries_and_ff_prefixes(oracle):
    """a start equal to a block's first key; a start just past a block's last key (the seek runs past
    the block and the next one is opened); prefixes ending in 0xff"""
    name = "random-1024-4"
    data, recs, _, _ = su.case(name)
    keys = [k for k, _ in recs]
    ikeys = [k for k, _ in oracle.index_records(data)]
    import bisect
    qs = []
    for b in (0, 1, 7, len(ikeys) // 2, len(ikeys) - 2, len(ikeys) - 1):
        last = bisect.bisect_right(keys, ikeys[b]) - 1          # the block's last record
        starts = [keys[last] + b"\0"]
        if last + 1 < len(keys):
            starts.append(keys[last + 1])                       # the next block's first key
        for s in starts:
            qs += [("from", s), ("get", s), ("prefix", s), ("prefix", s[:2]), ("range", s, s + b"\xff\xff"),
                   ("range", s, s)]
    ff = [k for k in keys if b"\xff" in k][:12]
    assert ff
    for k in ff:
        j = k.index(b"\xff")
        qs += [("prefix", k[: j + 1]), ("range", k[: j + 1], k[: j + 1] + b"\xff")]
    qs += [("prefix", b"\xff"), ("prefix", b"\xff\xff"), ("range", b"\xff", b"\xff\xff\xff")]
    lim = [5 if q[0] == "from" else None for q in qs]
    sb = _check_all(oracle, data, qs, lim, True, tag=name)
    assert sb.n_fallback == 0


def test_whole_file_from_one_wave(oracle):
    name = "random-1024-4"
    data, recs, _, _ = su.case(name)
    qs = [("prefix", b""), ("from", b""), ("range", b"", b"\xff" * 40)]
    sb = _check_all(oracle, data, qs, [None] * 3, True, tag=name, max_blocks=1 << 20)
    assert sb.n_fallback == 0 and sb.n_large == 0
    assert sb.records(0) == recs and int(sb.rec_off[-1].item()) == 3 * len(recs)


@pytest.mark.parametrize("nrec", [0, 1])
def test_tiny_files(oracle, nrec):
    data = su.write([(b"only", b"value")][:nrec])
    qs = [("from", b""), ("prefix", b""), ("prefix", b"on"), ("get", b"only"), ("get", b"onlx"), ("range", b"a", b"z"),
          ("range", b"p", b"z"), ("from", b"zz")]
    sb = _check_all(oracle, data, qs, [None] * len(qs), True)
    assert sb.n_fallback == 0 and sb.n_large == 0


def test_value_sizes_and_alignments(oracle):
    """values of 0 bytes and of 4 KiB and more (16 bytes per lane with ragged ends): the value's
    source and destination take every alignment 0..15"""
    rng = np.random.default_rng(5)
    recs = []
    for i in range(64):
        vl = (0, 5000 + 7 * i, 4096 + i, 1)[i % 4]
        recs.append((b"k%03d" % i + b"x" * (i % 16), rng.integers(0, 256, vl, dtype=np.uint8).tobytes()))
    data = su.write(recs, 8192, 16)
    src = {data.index(v) % 16 for _, v in recs if len(v) >= 4096}
    assert src == set(range(16))
    qs = [("from", b""), ("prefix", b"k0"), ("range", b"k003", b"k02"), ("get", b"k001x"), ("get", b"k000"), ("from", b"k01")]
    sb = _check_all(oracle, data, qs, [None, None, None, None, None, 7], True)
    assert sb.n_fallback == 0 and sb.n_large == 0
    assert sb.records(0) == recs
    ve = sb.val_end.cpu().numpy()
    dst = {int(a) % 16 for a, b in zip(np.concatenate([[0], ve[:-1]]), ve) if b - a >= 4096}
    assert dst == set(range(16))


def test_key_length_limit(oracle):
    """a key of MTBLX_SCAN_MAX_KEY bytes is served by the kernels; one byte more is FALLBACK and
    still equals the oracle"""
    from mtblx import _lib
    qs = [("from", b""), ("prefix", b"b"), ("get", b"c"), ("range", b"a", b"c"), ("get", b"a")]
    for extra, fallback in ((0, set()), (1, {0, 1, 2, 3})):
        recs = [(b"a", b"1"), (b"b" * (_lib.SCAN_MAX_KEY + extra), b"2"), (b"c", b"3")]
        data = su.write(recs, 8192, 16)           # one block, one restart interval
        sb = _check_all(oracle, data, qs, [None] * len(qs), True)
        st = sb.status.cpu().numpy()
        assert {i for i in range(len(qs)) if st[i] == _lib.SCAN_FALLBACK} == fallback
        assert sb.n_large == 0 and sb.records(0) == recs


def test_v1_file(oracle):
    data, recs, qs, lim = su.case("random-1024-4")
    v1 = corpus.to_v1(data)
    for verify in (True, False):
        sb = _check_all(oracle, v1, qs[:120], lim[:120], verify)
        assert sb.n_fallback == 0


# ---------------------------------------------------------------- 4. raw ABI
def _emit(r, nq, ws, wsb, keys_cap, vals_cap, rec_cap):
    """mtblx_scan_emit into buffers of exactly the given capacities followed by 64 guard bytes
    -> (flags, keys, vals, key_end, val_end, guards intact)"""
    import torch
    from mtblx import _lib, codec
    dev = r.file.device
    G = 64
    bufs = [torch.full((n + G,), 0xAB, dtype=torch.uint8, device=dev)
            for n in (keys_cap, vals_cap, 8 * rec_cap, 8 * rec_cap)]
    flags = torch.full((1,), 0x55, dtype=torch.int32, device=dev)
    out = _lib.Scanned(bufs[0].data_ptr(), keys_cap, bufs[1].data_ptr(), vals_cap, bufs[2].data_ptr(),
                       bufs[3].data_ptr(), rec_cap, flags.data_ptr())
    rc = _lib.lib().mtblx_scan_emit(C.c_void_p(r.file.data_ptr()), r.len, r.version, r.index_off, r.index_len,
                                    None, None, None, None, 0, None, nq, C.byref(out), C.c_void_p(ws.data_ptr()), wsb,
                                    C.c_void_p(codec._stream_handle(None)))
    assert rc == 0
    torch.cuda.synchronize()
    host = [b.cpu().numpy() for b in bufs]
    intact = all((h[-G:] == 0xAB).all() for h in host)
    return int(flags.item()), host, intact


def test_raw_abi_capacities_and_mark(oracle):
    import torch
    from mtblx import _lib
    name = "random-1024-4"
    data, recs, qs, lim = su.case(name)
    qs = qs[:90]
    rd, r = _reader(data)
    res, totals, ws, wsb, _, _, _ = r._scan_plan(qs, 64, None, None)
    nrec, kb, vb, nbad = totals
    exp = [su.expected(oracle, data, q, None, True, tag=name) for q in qs]
    host = np.frombuffer(res.cpu().numpy().tobytes(), np.dtype(_lib.ScanResult))[: len(qs)]
    ok = host["status"] == _lib.SCAN_OK
    assert nbad == int((~ok).sum()) and nrec == sum(len(e["records"]) for e, o in zip(exp, ok) if o) and nrec > 0
    assert (host["blocks"][ok] <= 64).all() and (host["nrec"][~ok] == 0).all()
    # exact capacities: everything written, nothing past them
    fl, (k, v, ke, ve), intact = _emit(r, len(qs), ws, wsb, kb, vb, nrec)
    assert fl == 0 and intact
    ke, ve = ke[: 8 * nrec].view(np.uint64), ve[: 8 * nrec].view(np.uint64)
    assert int(ke[-1]) == kb and int(ve[-1]) == vb
    want = [x for e, o in zip(exp, ok) if o for x in e["records"]]
    assert k[:kb].tobytes() == b"".join(x[0] for x in want) and v[:vb].tobytes() == b"".join(x[1] for x in want)
    assert list(np.diff(np.concatenate([[0], ke]))) == [len(x[0]) for x in want]
    # each capacity one short in turn
    for caps in ((kb - 1, vb, nrec), (kb, vb - 1, nrec), (kb, vb, nrec - 1)):
        fl, _, intact = _emit(r, len(qs), ws, wsb, *caps)
        assert fl == _lib.SCAN_OVERFLOW and intact, caps
    # a workspace no plan has marked: nothing is written
    zero = torch.zeros_like(ws)
    fl, host_bufs, intact = _emit(r, len(qs), zero, wsb, kb, vb, nrec)
    assert fl == _lib.SCAN_NOT_PLANNED and all((h == 0xAB).all() for h in host_bufs)
    # a plan of another batch size is not this batch's plan either
    fl, host_bufs, _ = _emit(r, len(qs) - 1, ws, wsb, kb, vb, nrec)
    assert fl == _lib.SCAN_NOT_PLANNED and all((h == 0xAB).all() for h in host_bufs)


def test_count_batch(oracle):
    from mtblx import _lib
    name = "counter-1024-16"
    data, recs, qs, lim = su.case(name)
    sel = [i for i, m in enumerate(lim) if m is None]
    qs = [qs[i] for i in sel]
    rd, r = _reader(data)
    st, n, kb, vb = (t.cpu().numpy() for t in r.count_batch(qs, max_blocks=1 << 20))
    assert (st == _lib.SCAN_OK).all()
    for i, q in enumerate(qs):
        e = su.expected(oracle, data, q, None, True, tag=name)["records"]
        assert (int(n[i]), int(kb[i]), int(vb[i])) == (len(e), sum(len(k) for k, _ in e), sum(len(v) for _, v in e)), q


# ---------------------------------------------------------------- 5. corrupt files
def _corrupt_case(seed):
    import test_seek_gpu as ts
    rng = np.random.default_rng(40 + seed)
    recs = corpus.random_records(rng, 3000, 1, 24, 0, 60)
    data, (off, ln) = ts._write(recs, 1024, 4)
    return rng, recs, bytes(data), off, ln


@pytest.mark.parametrize("seed", [1, 2])
def test_corrupt_files_unverified(oracle, seed):
    """restart entries with shared != 0 and 30 random byte flips, read with verification off:
    every query equals the oracle through whichever path served it"""
    import test_seek_gpu as ts
    rng, recs, data, off, ln = _corrupt_case(seed)
    d = bytearray(ts._corrupt_restart_shared(data, off, ln, rng, 12))
    for _ in range(30):
        b = int(rng.integers(0, off.size))
        d[int(off[b]) + int(rng.integers(0, int(ln[b])))] ^= int(rng.integers(1, 256))
    bad = bytes(d)
    assert bad != data
    qs, lim = su.queries_for(su.probe_keys(rng, recs, 24))
    sb = _check_all(oracle, bad, qs, lim, False)
    assert (sb.status.cpu().numpy() == 0).sum() > len(qs) // 4     # the kernels still serve their share


def test_checksum_mismatch_is_fallback(oracle):
    """verify on and one flipped content byte: the queries whose iteration opens that block are
    FALLBACK (the reference panics there), the others OK"""
    from mtblx import _lib
    rng, recs, data, off, ln = _corrupt_case(3)
    b = off.size // 2
    d = bytearray(data)
    d[int(off[b]) + int(ln[b]) // 2] ^= 0x40
    bad = bytes(d)
    rd, r = _reader(bad, True)
    qs, lim = su.queries_for(su.probe_keys(rng, recs, 24))
    sb = r.scan_batch(qs, max_blocks=1 << 20, max_records=lim)
    st = sb.status.cpu().numpy()
    hit = 0
    for i, (q, m) in enumerate(zip(qs, lim)):
        e = su.expected(oracle, bad, q, m, True)
        su.check(rd, sb, i, e, q)
        assert (st[i] == _lib.SCAN_FALLBACK) == (e["end"] == rd.END_PANIC), (q, st[i], e["end"])
        assert st[i] in (_lib.SCAN_OK, _lib.SCAN_FALLBACK)
        hit += e["end"] == rd.END_PANIC
    assert 0 < hit < len(qs)


def test_empty_batch_and_irregular_index(oracle):
    """no query at all; and an index block whose restart entries carry shared != 0 (read with
    verification off): its seeks depend on the live iterator, so every query goes to bulk()"""
    import test_seek_gpu as ts
    from mtblx import _lib
    data, recs, qs, lim = su.case("random-256-1")
    rd, r = _reader(data)
    sb = r.scan_batch([])
    assert sb.nq == 0 and sb.n_large == 0 and sb.n_fallback == 0 and sb.rec_off.tolist() == [0]
    assert [t.numel() for t in r.count_batch([])] == [0, 0, 0, 0]
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
        sb = _check_all(oracle, bad, qs[:45], lim[:45], False)
        assert sb.n_fallback == 45 and (sb.status.cpu().numpy() == _lib.SCAN_FALLBACK).all()
        assert int(sb.rec_off[-1].item()) == 0 and sb.keys.numel() == 0
        break
    assert seen

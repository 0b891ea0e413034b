"""Shared by test_scan_batch.py and test_scan_batch_gpu.py: the files, the query sets, the oracle
side of a query and the number of data blocks its iteration opens."""
import bisect
import functools

import numpy as np

import corpus

# name -> (records kind, block size, restart interval, compression)
FILES = {
    "random-1024-4": ("random", 1024, 4, 0),
    "random-256-1": ("random", 256, 1, 0),
    "random-4096-16": ("random", 4096, 16, 0),
    "random-2048-3-zlib": ("random", 2048, 3, 2),
    "random-1024-4-snappy": ("random", 1024, 4, 1),
    "counter-1024-16": ("counter", 1024, 16, 0),
}
CPU_FILES = ("random-1024-4", "random-256-1", "counter-1024-16")
MODE = {"from": "from", "get": "get", "prefix": "prefix", "range": "range"}


def write(records, bs=1024, iv=4, comp=0):
    from mtblx.writer import Writer
    w = Writer(bs, iv, comp, 1)
    for k, v in records:
        w.insert(k, v)
    return bytes(w.into_inner())


def probe_keys(rng, recs, n=40):
    """tests/test_seek_gpu.py::_probe_keys: present keys, just after, a prefix, a neighbour"""
    keys = [k for k, _ in recs]
    out = [b"", b"\x00", b"\xff" * 8]
    for _ in range(n):
        k = keys[int(rng.integers(0, len(keys)))]
        c = int(rng.integers(0, 4))
        if c == 0:
            out.append(k)
        elif c == 1:
            out.append(k + b"\x00")
        elif c == 2:
            out.append(k[: max(0, len(k) - 1)])
        else:
            out.append(k[:-1] + bytes([(k[-1] + 1) & 0xFF]) if k else b"\x01")
    return out


def queries_for(keys, counter=False):
    """-> (queries, max_records per query)"""
    qs, lim = [], []
    for k in keys:
        for q in (("prefix", k[:3]), ("prefix", k), ("range", k, k + b"\xff"), ("range", k[:2], k),
                  ("range", k + b"\x01", k), ("get", k)):
            qs.append(q)
            lim.append(None)
        for m in (0, 1, 37):
            qs.append(("from", k))
            lim.append(m)
    if counter:
        for q in (("prefix", b"k0123"), ("prefix", b"k012"), ("prefix", b"k01"), ("range", b"k000100", b"k000130")):
            qs.append(q)
            lim.append(None)
    return qs, lim


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (data, records, queries, limits) of one of FILES, built once per process"""
    kind, bs, iv, comp = FILES[name]
    rng = np.random.default_rng(bs + iv + comp)
    if kind == "counter":
        recs = [(b"k%06d" % i, b"v" * (i % 50)) for i in range(6000)]
    else:
        recs = corpus.random_records(rng, 4000, 0, 30, 0, 120)
    data = write(recs, bs, iv, comp)
    qs, lim = queries_for(probe_keys(rng, recs), counter=kind == "counter")
    return data, recs, qs, lim


_expected = {}


def expected(oracle, data, q, limit, verify, tag=None):
    """oracle.file_scan of one query; cached per (tag, query, limit, verify) when tag is given"""
    key = (tag, q, limit, verify)
    if tag is not None and key in _expected:
        return _expected[key]
    e = oracle.file_scan(data, MODE[q[0]], q[1], q[2] if q[0] == "range" else b"", verify=verify,
                         max_records=(1 << 62) if limit is None else limit)
    if tag is not None:
        _expected[key] = e
    return e


def span(ikeys, keys, q, nrec):
    """(first, stop, opened): file-order positions of the first record >= the start key and of the
    record the iteration stops at, and the data blocks the iteration opens (every Reader::block
    call, the sought block included): the index entry the seek lands on up to the entry of the block
    that holds the stop record."""
    first = bisect.bisect_left(keys, q[1])
    e0 = bisect.bisect_left(ikeys, q[1])
    if e0 == len(ikeys):
        return first, first, 0
    s = first + nrec
    e1 = len(ikeys) - 1 if s >= len(keys) else bisect.bisect_left(ikeys, keys[s])
    return first, s, e1 - e0 + 1


def check(rd, sb, i, exp, q):
    """ScanBatch query i against the oracle's result, as tests/test_seek_gpu.py::_bulk_check"""
    s = sb.scan(i)
    errs = (rd.END_ERR_OPEN, rd.END_ERR_NEXT)
    assert (s.end, s.err if s.end in errs else None) == (exp["end"], exp["err"] if exp["end"] in errs else None), q
    got = sb.records(i)
    assert got == exp["records"], (q, len(got), len(exp["records"]))
    assert s.nrec == len(got)

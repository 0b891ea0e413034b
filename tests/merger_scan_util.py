"""Shared by test_merger_scan.py, test_merger_scan_gpu.py and test_cpp_merger_scan.py: the
per-query model of Merger.scan_batch.

Query q over sources 0 .. S-1 is MergerIter / MultiIter (tests/merger_model.py) fed with the record
lists the oracle's iter_from / get / iter_prefix / iter_range returns per source
(scan_util.expected): `model_groups`.  The reference leaves the order inside a group to its heap,
so a comparison with it goes through mm.canon; what this library promises on top (values in source
order, the highest-numbered source's value where only empty keys match) is `promised_groups`, a
stable sort with the empty-key quirk of src/merger.rs:182-186 applied inside the query.  A limit m
keeps the first m items of the UNLIMITED result."""
import functools

import numpy as np

import corpus
import merger_model as mm
import scan_util


def per_source(oracle, datas, q, tag=None):
    """the record list every source yields for query q, unlimited"""
    return [scan_util.expected(oracle, d, q, None, True, tag=None if tag is None else (tag, i))["records"]
            for i, d in enumerate(datas)]


def model_groups(lists):
    return mm.multi_iter(lists)


def promised_groups(lists):
    flat = sorted(((k, s, v) for s, recs in enumerate(lists) for k, v in recs), key=lambda t: (t[0], t[1]))
    out = []
    for k, _, v in flat:
        if out and out[-1][0] == k:
            out[-1][1].append(v)
        else:
            out.append((k, [v]))
    if out and out[0][0] == b"":
        out = out[1:] if len(out) > 1 else [(b"", out[0][1][-1:])]
    return out


def cut(items, m):
    return items if m is None else items[:m]


def merged(groups, pick):
    """MergerIter's items from MultiIter's: the merge function is not called for a group of one"""
    return [(k, vs[0] if len(vs) == 1 else pick(vs)) for k, vs in groups]


PICK = {"concat": b"".join, "first": lambda vs: vs[0], "last": lambda vs: vs[-1]}


def sum_u64(vs):
    return (sum(int.from_bytes(v, "little") for v in vs) & ((1 << 64) - 1)).to_bytes(8, "little")


# the quirk's sources of the issue: "" in every source, followers in two
QUIRK_SOURCES = [[(b"", b"a"), (b"k1", b"x")], [(b"", b"b")], [(b"", b"c"), (b"k1", b"y"), (b"k2", b"z")]]
QUIRK_QUERIES = [(("range", b"", b""), None), (("get", b""), None), (("prefix", b""), None), (("from", b""), None),
                 (("from", b""), 0), (("from", b""), 1), (("from", b""), 2)]


@functools.lru_cache(maxsize=None)
def small_sources(bs, u64):
    """3 sources of 400 records over a shared pool of 600 keys, most keys in 2 - 3 sources
    -> (files, record lists, queries of every kind without limits)"""
    rng = np.random.default_rng(1000 + bs)
    pool = corpus.random_records(rng, 600, 0, 30, 0, 60)
    lists = []
    for s in range(3):
        idx = np.sort(rng.choice(len(pool), size=400, replace=False))
        lists.append([(pool[i][0], (1000 * s + int(i)).to_bytes(8, "little") if u64 else bytes([65 + s]) + pool[i][1][: 7 * s])
                      for i in idx])
    qs, _ = scan_util.queries_for(scan_util.probe_keys(rng, pool, n=12))
    return [mm.make_source(r, bs, 4) for r in lists], lists, qs

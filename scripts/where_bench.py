"""Value predicates (mtblx_scan_reduce_where, filter_records: mtblx_where_plan / _emit) against the calls
next to them and the path a user had before them (DESIGN.md §4 "Value predicates").

Records: reduce_bench's 0.88 M cfg2-shaped records (16-byte keys), each key once, with three u64 fields
(reduce_varint_bench.fields_of) as 24-byte values and as three varints.  Field 2 is uniform in 0..1023:
a bound on it sets the keep rate.
Legs, median of --runs after a warm-up, alternated in this process:
  fused    the scan_reduce_bench workload, --ranges range queries of 1000 records, (sum, min, max), both
           encodings: mtblx_scan_reduce_where (a predicate that keeps about half) against mtblx_scan_reduce
           over the same query tensors, by HIP events around the (synchronous) calls and by the host clock
  filter   mtblx_where_plan + mtblx_where_emit over all records (u64le) and buffers allocated beforehand at
           keep rates of 1 %, 50 % and 100 %, by HIP events; against mtblx_stream_copy of the kept bytes (the
           in-repo ceiling) and against mtblx_rollup_plan + mtblx_rollup_emit over the same records
           (GroupBy.length(8): every record its own group; the nearest sibling)
  e2e      Reader.reduce_batch(where=) as a user calls it against Reader.scan_batch, the records' read-back
           and Where.keeps + Reduce.fold on the host (over a --sample of the queries, scaled to the batch)
Reported besides: that the sampled results are equal on every path.

Prints one JSON object, writes it and a README.md with the ratios to --out (a directory).  Needs the GPU."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oxidized-mtbl_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

OPS = ("sum", "min", "max")


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def med(xs):
    return statistics.median(xs)


def host_fold(records, red, where):
    """what reduce_batch(where=) reports for one query, on the host: (fields, nrec, nbad, nmatch)"""
    vd = [where.keeps(v) for _, v in records]
    kept = [v for (_, v), x in zip(records, vd) if x is True]
    return red.fold(kept)[0], len(records), sum(1 for x in vd if x is None), len(kept)


def leg_fused(r, queries, red, where, runs):
    """mtblx_scan_reduce and mtblx_scan_reduce_where alone, alternated, queries already on the device"""
    from mtblx import _lib, codec, iterator
    L = _lib.lib()
    dev = r.file.device
    nq = len(queries)
    up = lambda xs: (torch.frombuffer(bytearray(b"".join(xs) or b"\0"), dtype=torch.uint8).to(dev),   # noqa: E731
                     torch.from_numpy(np.cumsum([len(x) for x in xs], dtype=np.int64)).to(dev))
    kb, ke = up([q[1] for q in queries])
    k2b, k2e = up([q[2] for q in queries])
    types = np.ascontiguousarray([iterator.KINDS[q[0]] for q in queries], dtype=np.int32)
    wsb = int(L.mtblx_scan_workspace_bytes(nq))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    res = torch.zeros(nq * 64, dtype=torch.uint8, device=dev)
    z = lambda *s: torch.zeros(s, dtype=torch.int64, device=dev)   # noqa: E731
    fields, nbad, wfields, wnbad, nmatch = z(nq, len(red.ops)), z(nq), z(nq, len(red.ops)), z(nq), z(nq)
    totals = (C.c_uint64 * 4)()
    spec, wspec = red.cstruct(), where.cstruct()
    p = C.c_void_p
    args = (p(r.file.data_ptr()), r.len, r.version, 1 if r.verify else 0, r.index_off, r.index_len, None, None, None, None,
            0, None, p(types.ctypes.data), p(kb.data_ptr()), p(ke.data_ptr()), p(k2b.data_ptr()), p(k2e.data_ptr()), None,
            64, nq, p(res.data_ptr()), totals, p(ws.data_ptr()), wsb)
    sh = p(codec._stream_handle(None))
    plain = lambda: L.mtblx_scan_reduce(*args, C.byref(spec), p(fields.data_ptr()), p(nbad.data_ptr()), sh)   # noqa: E731
    fused = lambda: L.mtblx_scan_reduce_where(*args, C.byref(spec), p(wfields.data_ptr()), p(wnbad.data_ptr()),   # noqa: E731
                                              C.byref(wspec), p(nmatch.data_ptr()), sh)
    t = {k: [] for k in ("plain_ev", "fused_ev", "plain", "fused")}
    for i in range(runs + 1):
        for name, fn in (("plain", plain), ("fused", fused)):
            w, _ = wall(fn)
            e, rc = events(fn)
            assert rc == 0
            if i:
                t[name].append(w)
                t[name + "_ev"].append(e)
    nrec = int(np.frombuffer(res.cpu().numpy().tobytes(), np.dtype(_lib.ScanResult))["nrec"].sum())
    assert torch.equal(nbad, wnbad) and int(nmatch.sum()) <= nrec
    return {"queries": nq, "records": nrec, "kept": int(nmatch.sum()),
            "scan_reduce_events_ms": round(med(t["plain_ev"]), 3), "scan_reduce_where_events_ms": round(med(t["fused_ev"]), 3),
            "where_over_plain_events": round(med(t["fused_ev"]) / med(t["plain_ev"]), 3),
            "scan_reduce_ms": round(med(t["plain"]), 3), "scan_reduce_where_ms": round(med(t["fused"]), 3),
            "where_over_plain": round(med(t["fused"]) / med(t["plain"]), 3)}


def leg_filter(rec, red, rates, runs):
    """plan + emit over buffers allocated beforehand, the copy ceiling over the kept bytes, the rollup's plan + emit"""
    from mtblx import GroupBy, Where, _lib, codec, filter_records
    L = _lib.lib()
    dev = rec.key_end.device
    n = rec.n
    p = C.c_void_p
    c = _lib.Records(codec._u(rec.keys), codec._u(rec.key_end), codec._u(rec.vals), codec._u(rec.val_end), n)
    sh = p(codec._stream_handle(None))
    wsb = int(L.mtblx_where_workspace_bytes(n, 0))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    keys, vals = torch.empty_like(rec.keys), torch.empty_like(rec.vals)
    ends = torch.empty(3 * n, dtype=torch.int64, device=dev)
    flags = torch.zeros(2, dtype=torch.int32, device=dev)
    out = _lib.Filtered(keys=keys.data_ptr(), keys_cap=int(keys.numel()), vals=vals.data_ptr(), vals_cap=int(vals.numel()),
                        key_end=ends.data_ptr(), val_end=ends.data_ptr() + 8 * n, src_idx=ends.data_ptr() + 16 * n,
                        rec_cap=n, flags=flags.data_ptr())
    totals = (C.c_uint64 * 6)()
    # the sibling: the rollup's plan + emit with every record its own group (key_end and grp_rec for n groups)
    g = GroupBy.length(8).cstruct()
    rwsb = int(L.mtblx_rollup_workspace_bytes(n, 0))
    rws = torch.empty(rwsb, dtype=torch.uint8, device=dev)
    rtot = torch.zeros(2, dtype=torch.int64, device=dev)
    rends = torch.empty(2 * n + 2, dtype=torch.int64, device=dev)
    rout = _lib.Rolled(keys=keys.data_ptr(), keys_cap=int(keys.numel()), key_end=rends.data_ptr(), key_end_cap=8 * n,
                       grp_rec=rends.data_ptr() + 8 * n, grp_rec_cap=8 * (n + 1), seg_grp=None, seg_grp_cap=0,
                       flags=flags.data_ptr() + 4)

    def rollup():
        assert L.mtblx_rollup_plan(C.byref(c), C.byref(g), None, 0, p(rtot.data_ptr()), p(rws.data_ptr()), rwsb, sh) == 0
        assert L.mtblx_rollup_emit(C.byref(c), C.byref(g), None, 0, C.byref(rout), p(rws.data_ptr()), rwsb, sh) == 0

    rows = []
    for name, clauses in rates:
        w = Where.like(red, clauses)
        spec = w.cstruct()

        def plan():
            assert L.mtblx_where_plan(C.byref(c), C.byref(spec), None, 0, totals, None, None, p(ws.data_ptr()), wsb, sh) == 0

        def both():
            plan()
            assert L.mtblx_where_emit(C.byref(c), C.byref(out), p(ws.data_ptr()), wsb, sh) == 0

        both()
        torch.cuda.synchronize()
        assert flags[0].item() == 0
        K, kb, vb = int(totals[0]), int(totals[1]), int(totals[2])
        f = filter_records(rec, w)                      # the Python surface gives the same bytes
        assert f.nkept == K and torch.equal(f.records.keys, keys[:kb]) and torch.equal(f.records.vals, vals[:vb])
        assert torch.equal(f.src_idx, ends[2 * n: 2 * n + K])
        nbytes = (kb + vb + 15) & ~15
        src = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        copy = lambda: L.mtblx_stream_copy(p(dst.data_ptr()), p(src.data_ptr()), nbytes, 0, sh)   # noqa: E731
        t = {k: [] for k in ("plan", "both", "copy", "rollup", "records")}
        for i in range(runs + 1):
            ms = {"plan": events(plan)[0], "both": events(both)[0], "rollup": events(rollup)[0],
                  "copy": events(copy)[0] if nbytes else 0.0, "records": wall(lambda: filter_records(rec, w))[0]}
            if i:
                for k in t:
                    t[k].append(ms[k])
        m = {k: med(v) for k, v in t.items()}
        rows.append({"keep": name, "records": n, "kept": K, "kept_bytes": kb + vb,
                     "where_plan_events_ms": round(m["plan"], 3), "where_plan_emit_events_ms": round(m["both"], 3),
                     "stream_copy_kept_bytes_events_ms": round(m["copy"], 4),
                     "rollup_plan_emit_events_ms": round(m["rollup"], 3),
                     "where_over_rollup": round(m["both"] / m["rollup"], 3),
                     "where_over_copy": round(m["both"] / m["copy"], 1) if m["copy"] else None,
                     "filter_records_ms": round(m["records"], 3),
                     "plan_emit_Mrec_per_s": round(n / m["both"] / 1e3, 1),
                     "plan_emit_GBps_read_and_written": round((int(rec.keys.numel()) + int(rec.vals.numel()) + 16 * n +
                                                               2 * (kb + vb) + 24 * K) / m["both"] / 1e6, 1)})
    assert flags[1].item() == 0
    return rows


def leg_e2e(r, queries, red, where, sample, runs):
    nq = len(queries)
    rng = np.random.default_rng(7)
    pick = sorted(rng.choice(nq, size=min(sample, nq), replace=False).tolist())
    rb = r.reduce_batch(queries, red, where=where)
    sb = r.scan_batch(queries)
    nm = rb.nmatch.cpu().numpy()
    for i in pick:                                     # correctness first
        assert (rb.values(i),) + rb.counts(i) + (int(nm[i]),) == host_fold(sb.records(i), red, where), i
    t = {k: [] for k in ("fused", "scan", "readback", "fold", "scanwhere")}
    for i in range(runs + 1):
        ms = {}
        ms["fused"], _ = wall(lambda: r.reduce_batch(queries, red, where=where))
        ms["scan"], sb = wall(lambda: r.scan_batch(queries))
        t0 = time.perf_counter()
        sb.records(pick[0])                            # copies the whole batch to the host once
        t1 = time.perf_counter()
        for j in pick:
            host_fold(sb.records(j), red, where)
        t2 = time.perf_counter()
        ms["readback"], ms["fold"] = (t1 - t0) * 1e3, (t2 - t1) * 1e3 * nq / len(pick)
        ms["scanwhere"], _ = wall(lambda: r.scan_batch(queries, where=where))
        if i:
            for k in t:
                t[k].append(ms[k])
    m = {k: med(v) for k, v in t.items()}
    host_ms = m["scan"] + m["readback"] + m["fold"]
    return {"queries": nq, "n_large": rb.n_large, "n_fallback": rb.n_fallback,
            "reduce_batch_where_ms": round(m["fused"], 2), "scan_batch_ms": round(m["scan"], 2),
            "readback_ms": round(m["readback"], 2), "host_filter_fold_ms_scaled": round(m["fold"], 1),
            "host_sample": len(pick), "scan_plus_host_ms": round(host_ms, 1),
            "scan_plus_host_over_reduce_batch_where": round(host_ms / m["fused"], 1),
            "scan_batch_where_ms": round(m["scanwhere"], 2), "sample_results_equal": True}


README = """# Value predicates: the bench's record

`scripts/where_bench.py` on {device}: {records} cfg2-shaped records (16-byte keys, three u64 fields as 24-byte
values and as three varints), median of {runs} runs.  The JSON beside this file holds every figure; the legs are
described in the script's docstring.  No ratio is a pass condition; the tests are.

## The fused walk: mtblx_scan_reduce_where against mtblx_scan_reduce

{nq} range queries of 1000 records, (sum, min, max), a predicate that keeps about half, HIP events around the calls.

| encoding | records walked | kept | scan_reduce, ms | scan_reduce_where, ms | ratio |
|---|---|---|---|---|---|
{fused}

## The filter: mtblx_where_plan + mtblx_where_emit

All records with 24-byte values, buffers allocated beforehand, HIP events.  The copy is mtblx_stream_copy over as many
bytes as the kept keys and values; the rollup is mtblx_rollup_plan + _emit with every record its own group.

| keep | kept records | plan, ms | plan + emit, ms | copy of the kept bytes, ms | rollup plan + emit, ms | filter / rollup | filter_records (host clock), ms |
|---|---|---|---|---|---|---|---|
{filt}

## End to end: Reader.reduce_batch(where=) against scan_batch, the read-back and a host filter and fold

| encoding | queries | reduce_batch(where=), ms | scan_batch, ms | read-back, ms | host filter + fold (scaled), ms | host path / reduce_batch(where=) | scan_batch(where=), ms |
|---|---|---|---|---|---|---|---|
{e2e}
"""


def main():
    from reduce_bench import make_records
    from reduce_varint_bench import encode_varints, fields_of
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=880_000)
    ap.add_argument("--ranges", type=int, default=10_000)
    ap.add_argument("--sample", type=int, default=100, help="queries the host filter and fold run")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "where"))
    a = ap.parse_args()
    from mtblx import Reduce, Where, reader, sorter
    from mtblx.encode import DeviceRecords
    keys, vals8 = make_records(a.records, "dup10")
    f = fields_of(vals8)
    n = keys.shape[0]
    _, uniq = np.unique(keys.view(">u8").reshape(n, 2), axis=0, return_index=True)   # each key once, in key order
    keys, f = np.ascontiguousarray(keys[uniq]), f[uniq]
    n = keys.shape[0]
    rng = np.random.default_rng(11)
    rg = [("range", keys[i].tobytes(), keys[i + 999].tobytes()) for i in rng.integers(0, n - 1000, a.ranges)]
    vb, ve = encode_varints(f)
    u64 = f.astype("<u8").view(np.uint8).reshape(-1)
    inputs = {"u64le": (u64, np.arange(1, n + 1, dtype=np.uint64) * 24), "varint": (vb, ve.astype(np.uint64))}
    half = [(2, 512, None)]
    res = {"device": torch.cuda.get_device_name(0), "records": int(n), "runs": a.runs, "fused": [], "e2e": []}
    for enc, (vbytes, vends) in inputs.items():
        red = Reduce(*OPS, encoding=enc)
        w = Where.like(red, half)
        s = sorter.Sorter("first")
        s.insert_batch(keys.reshape(-1), np.arange(1, n + 1, dtype=np.uint64) * 16, vbytes, vends)
        r = reader.ReaderBuilder().verify_checksums(False).read(s.write_file(4096, 16))
        res["fused"].append(dict(encoding=enc, **leg_fused(r, rg, red, w, a.runs)))
        res["e2e"].append(dict(encoding=enc, **leg_e2e(r, rg, red, w, a.sample, max(a.runs // 2, 2))))
        del r, s
        torch.cuda.empty_cache()
    ends = lambda w: torch.arange(1, n + 1, dtype=torch.int64, device="cuda") * w   # noqa: E731
    rec = DeviceRecords(torch.from_numpy(keys.reshape(-1)).cuda(), ends(16), torch.from_numpy(u64).cuda(), ends(24))
    res["filter"] = leg_filter(rec, Reduce(*OPS), [("1 %", [(2, None, 9)]), ("50 %", half), ("100 %", [])], a.runs)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "where_bench.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    fused = "\n".join(f"| {x['encoding']} | {x['records']} | {x['kept']} | {x['scan_reduce_events_ms']} | "
                      f"{x['scan_reduce_where_events_ms']} | {x['where_over_plain_events']} |" for x in res["fused"])
    filt = "\n".join(f"| {x['keep']} | {x['kept']} | {x['where_plan_events_ms']} | {x['where_plan_emit_events_ms']} | "
                     f"{x['stream_copy_kept_bytes_events_ms']} | {x['rollup_plan_emit_events_ms']} | {x['where_over_rollup']} | "
                     f"{x['filter_records_ms']} |" for x in res["filter"])
    e2e = "\n".join(f"| {x['encoding']} | {x['queries']} | {x['reduce_batch_where_ms']} | {x['scan_batch_ms']} | "
                    f"{x['readback_ms']} | {x['host_filter_fold_ms_scaled']} | {x['scan_plus_host_over_reduce_batch_where']} | "
                    f"{x['scan_batch_where_ms']} |" for x in res["e2e"])
    with open(os.path.join(a.out, "README.md"), "w") as fh:
        fh.write(README.format(device=res["device"], records=n, runs=a.runs, nq=a.ranges, fused=fused, filt=filt, e2e=e2e))
    print(json.dumps(res))


if __name__ == "__main__":
    main()

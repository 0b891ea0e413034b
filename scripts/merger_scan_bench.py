"""Merger.scan_batch on 8 sources of the cfg2 record shape against the per-query path (DESIGN.md §4
"Merged batched scans").

Sources: scripts/merge_bench.py's: one cfg2 key stream (16 B keys = be64 counter || 8 random bytes,
64 B values) dealt to 8 sources, about a tenth of the keys also given to a second source.
Batches, over the keys of the whole stream drawn uniformly:
  prefix14   --queries prefix queries, the first 14 bytes of a key: that key's record from every
             source that holds it
  get        --queries gets of whole keys
Per batch, --runs times after a warm-up, every run kept in the JSON and the median reported:
  scan_ms[s]       Reader.scan_batch of source s as Merger.scan_batch calls it (host clock ending in
                   a synchronize: query upload, plan, allocation, emit, read-back)
  plan_phase_ms    mtblx_merge_seg_plan_timed over the S scan results resident on the device: HIP
                   events around [0] offsets check + per-segment skips + handles, [1 .. passes] the
                   merge passes, [passes + 1] grouping + segment ends; plan_call_ms is the host
                   clock around the synchronous call (its two read-backs included)
  emit_ms          mtblx_merge_seg_emit (CONCAT), HIP events
  total_ms         Merger("concat").scan_batch(queries) as a user calls it, host clock ending in a
                   synchronize
  loop             this library's own per-query path (code unchanged by the segmented merge):
                   Reader.iter_prefix / iter_range per source, then merge_all over the pieces, on a
                   --sample of the same queries, alternated with the batched run; reported per query
The batch's records of the sampled queries are compared with the loop's before any time is
reported.  Rust cannot be built here, so no reference timing exists.  No threshold: the numbers are
reported as found.

Prints one JSON object (and writes it to --out).  Needs the GPU."""
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

from merge_bench import make_sources, write_files  # noqa: E402


def med(xs):
    return round(statistics.median(xs), 4)


def loop_query(readers, q):
    """the per-query path: one seek-based scan per source, then the Merger over the pieces"""
    from mtblx import merger
    scans = [r.iter_prefix(q[1]) if q[0] == "prefix" else r.iter_range(q[1], q[1]) for r in readers]
    return merger.merge_all([merger._clean_scan(s) for s in scans], "concat")


def seg_times(sbs, nq, runs):
    """the segmented plan (per phase) and emit over the scan results -> dict of per-run lists"""
    from mtblx import _lib, codec, encode
    L = _lib.lib()
    dev = sbs[0].keys.device
    nsrc = len(sbs)
    recs = [encode.DeviceRecords(sb.keys, sb.key_end, sb.vals, sb.val_end) for sb in sbs]
    offs = [sb.rec_off.contiguous() for sb in sbs]
    arr = (_lib.Records * nsrc)()
    op = (C.c_void_p * nsrc)()
    for i in range(nsrc):
        arr[i] = recs[i].cstruct()
        op[i] = offs[i].data_ptr()
    n = sum(r.n for r in recs)
    wsb = int(L.mtblx_merge_seg_workspace_bytes(n, nsrc, nq))
    ws = torch.empty(wsb + 256, dtype=torch.uint8, device=dev)
    wp = (ws.data_ptr() + 255) & ~255
    seg_end = torch.empty(nq, dtype=torch.int64, device=dev)
    tot = (C.c_uint64 * 6)()
    passes = max(nsrc - 1, 0).bit_length()
    ph = (C.c_float * (passes + 2))()
    sh = C.c_void_p(codec._stream_handle(None))
    out = {"plan_call_ms": [], "plan_phase_ms": [], "emit_ms": []}
    for i in range(runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = L.mtblx_merge_seg_plan_timed(arr, op, nsrc, nq, tot, C.c_void_p(seg_end.data_ptr()), C.c_void_p(wp), wsb,
                                          sh, ph, passes + 2)
        t1 = time.perf_counter()
        assert rc == 0, rc
        groups, kb, nv, vb = (int(tot[j]) for j in range(4))
        keys = torch.empty(kb, dtype=torch.uint8, device=dev)
        key_end = torch.empty(groups, dtype=torch.int64, device=dev)
        vals = torch.empty(vb, dtype=torch.uint8, device=dev)
        val_end = torch.empty(groups, dtype=torch.int64, device=dev)
        flags = torch.zeros(1, dtype=torch.int32, device=dev)
        u = codec._u
        mo = _lib.Merged(u(keys), kb, u(key_end), 8 * groups, u(vals), vb, u(val_end), 8 * groups, 0, 0, flags.data_ptr())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = L.mtblx_merge_seg_emit(arr, op, nsrc, nq, _lib.MERGE_CONCAT, C.byref(mo), C.c_void_p(wp), wsb, sh)
        e1.record()
        torch.cuda.synchronize()
        assert rc == 0 and int(flags.item()) == 0
        if i:
            out["plan_call_ms"].append(round((t1 - t0) * 1e3, 4))
            out["plan_phase_ms"].append([round(float(x), 4) for x in ph])
            out["emit_ms"].append(round(e0.elapsed_time(e1), 4))
    out.update(records_in=n, groups_out=groups, key_bytes=kb, value_bytes=vb, passes=passes)
    return out


def batch(name, readers, queries, sample, runs):
    from mtblx import merger
    nq = len(queries)
    m = merger.Merger(readers, "concat")
    rng = np.random.default_rng(7)
    pick = sorted(rng.choice(nq, size=min(sample, nq), replace=False).tolist())
    res = m.scan_batch(queries)
    for i in pick:   # correctness first
        assert res.records(i) == merger._records_list(loop_query(readers, queries[i])), (name, queries[i])
    total, loop = [], []
    for i in range(runs + 1):   # alternated: one batched run, one pass of the loop
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = m.scan_batch(queries)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for j in pick:
            loop_query(readers, queries[j])
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if i:
            total.append(round((t1 - t0) * 1e3, 3))
            loop.append(round((t2 - t1) * 1e3, 3))
    scans = [[] for _ in readers]
    sbs = None
    for i in range(runs + 1):
        sbs = []
        for s, r in enumerate(readers):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sbs.append(r.scan_batch(queries))
            torch.cuda.synchronize()
            if i:
                scans[s].append(round((time.perf_counter() - t0) * 1e3, 3))
    seg = seg_times(sbs, nq, runs)
    phases = [med([run[p] for run in seg["plan_phase_ms"]]) for p in range(seg["passes"] + 2)]
    row = {"batch": name, "queries": nq, "sources": len(readers), "n_large": res.n_large, "n_fallback": res.n_fallback,
           "records_in": seg["records_in"], "items_out": seg["groups_out"],
           "scan_ms_per_source": [med(x) for x in scans], "scan_ms_sum": round(sum(med(x) for x in scans), 3),
           "plan_call_ms": med(seg["plan_call_ms"]), "plan_phase_ms": phases, "plan_phases_sum_ms": round(sum(phases), 4),
           "emit_ms": med(seg["emit_ms"]), "total_ms": med(total), "total_us_per_query": round(med(total) * 1e3 / nq, 3),
           "loop_sample": len(pick), "loop_ms": med(loop), "loop_us_per_query": round(med(loop) * 1e3 / len(pick), 1),
           "sample_outputs_equal": True,
           "runs": {"scan_ms": scans, "plan_call_ms": seg["plan_call_ms"], "plan_phase_ms": seg["plan_phase_ms"],
                    "emit_ms": seg["emit_ms"], "total_ms": total, "loop_ms": loop}}
    row["loop_over_batch"] = round(row["loop_us_per_query"] / row["total_us_per_query"], 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1_000_000, help="keys of the cfg2 stream dealt to the 8 sources")
    ap.add_argument("--queries", type=int, default=100_000)
    ap.add_argument("--sample", type=int, default=300, help="queries the per-query loop runs")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merger_scan", "merger_scan_bench.json"))
    a = ap.parse_args()
    from mtblx import reader
    sources, ndup = make_sources(a.keys)
    files = write_files(sources)
    readers = [reader.Reader(f) for f in files]
    allkeys = np.concatenate([k for k, _ in sources])
    rng = np.random.default_rng(11)
    pre = [("prefix", allkeys[i, :14].tobytes()) for i in rng.integers(0, allkeys.shape[0], a.queries)]
    get = [("get", allkeys[i].tobytes()) for i in rng.integers(0, allkeys.shape[0], a.queries)]
    res = {"device": torch.cuda.get_device_name(0), "keys": a.keys, "keys_in_two_sources": ndup,
           "source_records": [int(k.shape[0]) for k, _ in sources], "file_bytes": [len(f) for f in files],
           "runs": a.runs, "rows": [batch("prefix14", readers, pre, a.sample, a.runs),
                                    batch("get", readers, get, a.sample, a.runs)]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "rows"}))
    for row in res["rows"]:
        print(json.dumps({k: v for k, v in row.items() if k != "runs"}))


if __name__ == "__main__":
    main()

"""Aggregating scans (Reader.reduce_batch, reduce_segments) on a cfg2-shaped file against the paths a
user had before them (DESIGN.md §4 "Aggregating scans").

File: cfg2's keys (16 B = be64 counter || 8 random bytes, mtblx/synth.py) with 24-byte values of three
u64 fields reduced as (sum, min, max), ~4 KiB blocks.
Shapes, as scripts/scan_bench.py:
  prefix14   --queries prefix queries on the first 14 bytes of a key drawn from the file (one record)
  range1000  --queries / 10 range queries [key[i], key[i + 999]]: 1000 records, ~8 blocks
Legs, median of --runs after a warm-up, alternated in this process:
  reduce_batch        Reader.reduce_batch as a user calls it (host clock ending in a synchronize)
  count_batch         Reader.count_batch likewise: the floor, the same walk without the value loads
  reduce_call / plan_call   mtblx_scan_reduce / mtblx_scan_plan alone over query tensors already on the
                      device.  Both calls are synchronous, so each is measured twice: by HIP events
                      recorded on the stream around the call (the type upload, the walk, the offsets
                      kernel and the totals' read-back: device time) and by the host clock around it
                      (the same plus the launches and the stream synchronise)
  scan+host           the path of the parent commit: scan_batch, the records' read-back, and the fold on
                      the host (Reduce.fold over a --sample of the queries, scaled to the batch)
  scan+segments       scan_batch, then reduce_segments over its records: everything on the device; the
                      reduce_segments part also by HIP events
Reported besides: the bytes allocated for the answer on each path, and that the sampled queries' results
are equal on all paths.
Skew: --skew records of 24 bytes as ONE segment against the same records in segments of 10, by HIP
events: the ratio is recorded, no threshold is set.

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


def call_ms(r, queries, red, runs):
    """mtblx_scan_plan and mtblx_scan_reduce alone, alternated, queries already on the device"""
    from mtblx import _lib, codec, iterator
    L = _lib.lib()
    dev = r.file.device
    nq = len(queries)
    up = lambda xs: (torch.frombuffer(bytearray(b"".join(xs) or b"\0"), dtype=torch.uint8).to(dev),   # noqa: E731
                     torch.from_numpy(np.cumsum([len(x) for x in xs], dtype=np.int64)).to(dev))
    kb, ke = up([q[1] for q in queries])
    k2b, k2e = up([q[2] if q[0] == "range" else b"" for q in queries])
    types = np.ascontiguousarray([iterator.KINDS[q[0]] for q in queries], dtype=np.int32)
    wsb = int(L.mtblx_scan_workspace_bytes(nq))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    res = torch.zeros(nq * 64, dtype=torch.uint8, device=dev)
    fields = torch.zeros((nq, len(red.ops)), dtype=torch.int64, device=dev)
    nbad = torch.zeros(nq, dtype=torch.int64, device=dev)
    totals = (C.c_uint64 * 4)()
    spec = red.cstruct()
    args = (C.c_void_p(r.file.data_ptr()), r.len, r.version, 1 if r.verify else 0, r.index_off, r.index_len, None, None,
            None, None, 0, None, C.c_void_p(types.ctypes.data), C.c_void_p(kb.data_ptr()), C.c_void_p(ke.data_ptr()),
            C.c_void_p(k2b.data_ptr()), C.c_void_p(k2e.data_ptr()), None, 64, nq, C.c_void_p(res.data_ptr()), totals,
            C.c_void_p(ws.data_ptr()), wsb)
    sh = C.c_void_p(codec._stream_handle(None))
    plan, reduce, plan_ev, reduce_ev = [], [], [], []
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for i in range(runs + 1):
        torch.cuda.synchronize()
        ev[0].record()
        t0 = time.perf_counter()
        rc0 = L.mtblx_scan_plan(*args, sh)
        t1 = time.perf_counter()
        ev[1].record()
        torch.cuda.synchronize()
        ev[2].record()
        t2 = time.perf_counter()
        rc1 = L.mtblx_scan_reduce(*args, C.byref(spec), C.c_void_p(fields.data_ptr()), C.c_void_p(nbad.data_ptr()), sh)
        t3 = time.perf_counter()
        ev[3].record()
        torch.cuda.synchronize()
        assert rc0 == 0 and rc1 == 0
        if i:
            plan.append((t1 - t0) * 1e3)
            reduce.append((t3 - t2) * 1e3)
            plan_ev.append(ev[0].elapsed_time(ev[1]))
            reduce_ev.append(ev[2].elapsed_time(ev[3]))
    return tuple(statistics.median(x) for x in (plan, reduce, plan_ev, reduce_ev))


def segments_of(sb):
    from mtblx.encode import DeviceRecords
    lo = sb.rec_off[:-1].contiguous()
    return DeviceRecords(sb.keys, sb.key_end, sb.vals, sb.val_end), lo, sb.rec_off[1:].contiguous()


def shape(r, name, queries, red, sample, runs):
    from mtblx import reduce_segments
    nq, nf = len(queries), len(red.ops)
    rng = np.random.default_rng(7)
    pick = sorted(rng.choice(nq, size=min(sample, nq), replace=False).tolist())
    # correctness first: the three paths on the sampled queries
    rb = r.reduce_batch(queries, red)
    sb = r.scan_batch(queries)
    f, nb = reduce_segments(*segments_of(sb), red)
    fh, nbh = f.cpu().numpy().view(np.uint64), nb.cpu().numpy()
    for i in pick:
        want = red.fold([v for _, v in sb.records(i)])
        assert (rb.values(i),) + rb.counts(i) == want, (name, i)
        assert (tuple(int(x) for x in fh[i]), int(nbh[i])) == (want[0], want[2]), (name, i)
    t = {k: [] for k in ("reduce", "count", "scan", "readback", "fold", "scanseg", "seg_events")}
    for i in range(runs + 1):
        ms = {}
        ms["reduce"], rb = wall(lambda: r.reduce_batch(queries, red))
        ms["count"], _ = wall(lambda: r.count_batch(queries))
        ms["scan"], sb = wall(lambda: r.scan_batch(queries))
        t0 = time.perf_counter()
        sb.records(pick[0])                       # copies the whole batch to the host once
        t1 = time.perf_counter()
        for j in pick:
            red.fold([v for _, v in sb.records(j)])
        t2 = time.perf_counter()
        ms["readback"], ms["fold"] = (t1 - t0) * 1e3, (t2 - t1) * 1e3 * nq / len(pick)

        def both():
            s2 = r.scan_batch(queries)
            return s2, reduce_segments(*segments_of(s2), red)

        ms["scanseg"], (s2, _) = wall(both)
        recs, lo, hi = segments_of(s2)
        ms["seg_events"], _ = events(lambda: reduce_segments(recs, lo, hi, red))
        if i:
            for k in t:
                t[k].append(ms[k])
    med = {k: statistics.median(v) for k, v in t.items()}
    plan_ms, reduce_ms, plan_ev, reduce_ev = call_ms(r, queries, red, runs)
    nrec = int(sb.rec_off[-1].item())
    scan_bytes = int(sb.keys.numel() + sb.vals.numel() + 16 * nrec + 8)
    host_ms = med["scan"] + med["readback"] + med["fold"]
    return {"shape": name, "verify": bool(r.verify), "queries": nq, "records": nrec, "n_large": rb.n_large,
            "n_fallback": rb.n_fallback,
            "reduce_batch_ms": round(med["reduce"], 2), "count_batch_ms": round(med["count"], 2),
            "reduce_call_ms": round(reduce_ms, 3), "plan_call_ms": round(plan_ms, 3),
            "reduce_call_over_plan_call": round(reduce_ms / plan_ms, 3),
            "reduce_call_events_ms": round(reduce_ev, 3), "plan_call_events_ms": round(plan_ev, 3),
            "reduce_events_over_plan_events": round(reduce_ev / plan_ev, 3),
            "scan_batch_ms": round(med["scan"], 2), "readback_ms": round(med["readback"], 2),
            "host_fold_ms_scaled": round(med["fold"], 1), "host_fold_sample": len(pick),
            "scan_plus_host_ms": round(host_ms, 1),
            "scan_plus_segments_ms": round(med["scanseg"], 2), "reduce_segments_events_ms": round(med["seg_events"], 3),
            "scan_plus_host_over_reduce_batch": round(host_ms / med["reduce"], 1),
            "scan_plus_segments_over_reduce_batch": round(med["scanseg"] / med["reduce"], 2),
            "answer_bytes_reduce_batch": nq * (8 * nf + 16), "answer_bytes_scan_batch": scan_bytes,
            "sample_results_equal": True}


def skew(n, runs):
    """n records of 24 bytes as one segment against segments of 10 records"""
    from mtblx import Reduce, reduce_segments
    from mtblx.encode import DeviceRecords
    red = Reduce("sum", "min", "max")
    g = torch.Generator(device="cuda").manual_seed(5)
    vals = torch.randint(0, 256, (24 * n,), dtype=torch.uint8, device="cuda", generator=g)
    ve = torch.arange(1, n + 1, dtype=torch.int64, device="cuda") * 24
    z = torch.zeros(0, dtype=torch.uint8, device="cuda")
    rec = DeviceRecords(z, ve, vals, ve)
    one = (torch.zeros(1, dtype=torch.int64, device="cuda"), torch.full((1,), n, dtype=torch.int64, device="cuda"))
    lo = torch.arange(0, n, 10, dtype=torch.int64, device="cuda")
    many = (lo, torch.clamp(lo + 10, max=n))
    t1, tm = [], []
    f1 = fm = None
    for i in range(runs + 1):
        a, (f1, _) = events(lambda: reduce_segments(rec, one[0], one[1], red))
        b, (fm, _) = events(lambda: reduce_segments(rec, many[0], many[1], red))
        if i:
            t1.append(a)
            tm.append(b)
    # the same records either way: the short segments' sums add up to the long one's, their minima's minimum is its minimum
    f1, fm = f1.cpu().numpy().view(np.uint64), fm.cpu().numpy().view(np.uint64)
    assert int(fm[:, 0].sum(dtype=np.uint64)) == int(f1[0, 0]) and fm[:, 1].min() == f1[0, 1] and fm[:, 2].max() == f1[0, 2]
    a, b = statistics.median(t1), statistics.median(tm)
    return {"records": n, "segments_short": int(lo.numel()), "one_segment_ms": round(a, 3), "short_segments_ms": round(b, 3),
            "one_over_short": round(a / b, 3), "one_segment_GBps_read": round(32 * n / a / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=20000, help="sizes the file: the records of a cfg2 file of this many data blocks")
    ap.add_argument("--queries", type=int, default=100_000)
    ap.add_argument("--sample", type=int, default=500, help="queries the host fold runs")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--skew", type=int, default=8_800_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_reduce", "scan_reduce_bench.json"))
    a = ap.parse_args()
    from mtblx import Reduce, reader, synth
    n = synth.cfg2_file_nrec(a.blocks)
    keys = synth.cfg2_keys(n)
    rng = np.random.default_rng(11)
    vals = rng.integers(0, 256, (n, 24), dtype=np.uint8)
    data, off, ln = synth.write_arrays(np.ascontiguousarray(keys).reshape(-1), vals.reshape(-1), 16, 24)
    red = Reduce("sum", "min", "max")
    pre = [("prefix", keys[i, :14].tobytes()) for i in rng.integers(0, n, a.queries)]
    rg = [("range", keys[i].tobytes(), keys[i + 999].tobytes()) for i in rng.integers(0, n - 1000, max(a.queries // 10, 1))]
    res = {"device": torch.cuda.get_device_name(0), "file_bytes": int(data.size), "file_records": int(n),
           "file_blocks": int(off.size), "runs": a.runs, "rows": []}
    for verify in (True, False):
        r = reader.ReaderBuilder().verify_checksums(verify).read(data)
        res["rows"].append(shape(r, "prefix14", pre, red, a.sample, a.runs))
        res["rows"].append(shape(r, "range1000", rg, red, max(a.sample // 5, 1), a.runs))
    res["skew"] = skew(a.skew, a.runs)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Batched scans (Reader.scan_batch) on the cfg2 file against the per-query loop (DESIGN.md §4
"Batched scans").

File: cfg2 (16 B keys = be64 counter || 8 random bytes, 64 B values, ~4 KiB blocks, mtblx/synth.py).
Shapes:
  prefix14   --queries prefix queries: the first 14 bytes of a key drawn uniformly from the file's
             keys, so each matches that key's record (one block, two when the seek lands on a
             block's end)
  range1000  --queries / 10 range queries [key[i], key[i + 999]], i uniform: 1000 records, ~20 blocks
Per shape and verify on / off, median of --runs after a warm-up, all in this process:
  plan_ms / emit_ms   mtblx_scan_plan (synchronous: host clock) and mtblx_scan_emit (HIP events) over
                      query tensors already on the device
  batch_ms            Reader.scan_batch(queries) as a user calls it, host clock ending in a
                      synchronize: query upload, plan, allocation, emit, the read-back, and bulk() for
                      whatever the kernels handed back
  loop                the path a user had before: a Python loop of Reader.iter_prefix /
                      iter_range over a --sample of the same queries, alternated with the batched run
  copy                mtblx_stream_copy moving as many bytes as the emit wrote (read + write), the
                      in-process copy ceiling: a reported ratio, not a gate
The batched records of the sampled queries are compared with the loop's before any time is reported.

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


def copy_ms(nbytes, runs=5):
    """mtblx_stream_copy moving nbytes in all (half read, half written), best variant, median ms"""
    from mtblx import _lib
    L = _lib.lib()
    half = max(((nbytes // 2) + 15) & ~15, 16)
    a = torch.empty(half, dtype=torch.uint8, device="cuda")
    b = torch.empty(half, dtype=torch.uint8, device="cuda")
    best = None
    for variant in (2, 3, 2 | 4, 3 | 4):
        ts = []
        for i in range(runs + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = L.mtblx_stream_copy(C.c_void_p(b.data_ptr()), C.c_void_p(a.data_ptr()), half, variant,
                                     C.c_void_p(int(torch.cuda.current_stream().cuda_stream)))
            e1.record()
            torch.cuda.synchronize()
            assert rc == 0
            if i:
                ts.append(e0.elapsed_time(e1))
        m = statistics.median(ts)
        best = m if best is None else min(best, m)
    return best


def raw_times(r, queries, runs):
    """plan (host clock, the call is synchronous) and emit (HIP events) over device-resident queries"""
    from mtblx import _lib, codec
    L = _lib.lib()
    nq = len(queries)
    plan, emit = [], []
    tot = None
    for i in range(runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res, totals, ws, wsb, _, tab, _ = r._scan_plan(queries, 64, None, None)
        t1 = time.perf_counter()
        # _scan_plan uploads the queries first; plan_call_ms below times the C call alone
        nrec, kb, vb, nbad = totals
        buf = torch.empty(kb + vb + 16 * nrec + 8, dtype=torch.uint8, device="cuda")
        out = _lib.Scanned(keys=buf.data_ptr() + 16 * nrec + 8, keys_cap=kb, vals=buf.data_ptr() + 16 * nrec + 8 + kb,
                           vals_cap=vb, key_end=buf.data_ptr(), val_end=buf.data_ptr() + 8 * nrec, rec_cap=nrec,
                           flags=buf.data_ptr() + 16 * nrec)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = L.mtblx_scan_emit(C.c_void_p(r.file.data_ptr()), r.len, r.version, r.index_off, r.index_len, *tab, nq,
                               C.byref(out), C.c_void_p(ws.data_ptr()), wsb, C.c_void_p(codec._stream_handle(None)))
        e1.record()
        torch.cuda.synchronize()
        assert rc == 0 and int(buf[16 * nrec: 16 * nrec + 4].view(torch.int32).item()) == 0
        if i:
            plan.append((t1 - t0) * 1e3)
            emit.append(e0.elapsed_time(e1))
        tot = totals
    return statistics.median(plan), statistics.median(emit), tot


def plan_call_ms(r, queries, runs):
    """mtblx_scan_plan alone (queries already on the device): host clock around the synchronous call"""
    from mtblx import _lib, codec, iterator
    L = _lib.lib()
    dev = r.file.device
    nq = len(queries)
    ks = [q[1] for q in queries]
    k2 = [q[2] if q[0] == "range" else b"" for q in queries]
    up = lambda xs: (torch.frombuffer(bytearray(b"".join(xs) or b"\0"), dtype=torch.uint8).to(dev),
                     torch.from_numpy(np.cumsum([len(x) for x in xs], dtype=np.int64)).to(dev))
    kb, ke = up(ks)
    k2b, k2e = up(k2)
    types = np.ascontiguousarray([iterator.KINDS[q[0]] for q in queries], dtype=np.int32)
    wsb = int(L.mtblx_scan_workspace_bytes(nq))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    res = torch.zeros(nq * 64, dtype=torch.uint8, device=dev)
    totals = (C.c_uint64 * 4)()
    ts = []
    for i in range(runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = L.mtblx_scan_plan(C.c_void_p(r.file.data_ptr()), r.len, r.version, 1 if r.verify else 0, r.index_off,
                               r.index_len, None, None, None, None, 0, None, C.c_void_p(types.ctypes.data),
                               C.c_void_p(kb.data_ptr()), C.c_void_p(ke.data_ptr()), C.c_void_p(k2b.data_ptr()),
                               C.c_void_p(k2e.data_ptr()), None, 64, nq, C.c_void_p(res.data_ptr()), totals,
                               C.c_void_p(ws.data_ptr()), wsb, C.c_void_p(codec._stream_handle(None)))
        t1 = time.perf_counter()
        assert rc == 0
        if i:
            ts.append((t1 - t0) * 1e3)
    return statistics.median(ts)


def one_query(r, q):
    return r.iter_prefix(q[1]) if q[0] == "prefix" else r.iter_range(q[1], q[2])


def shape(r, name, queries, sample, runs):
    nq = len(queries)
    rng = np.random.default_rng(7)
    pick = sorted(rng.choice(nq, size=min(sample, nq), replace=False).tolist())
    # correctness first: the batch against the loop on the sampled queries
    sb = r.scan_batch(queries)
    for i in pick:
        assert sb.records(i) == one_query(r, queries[i]).records(), (name, queries[i])
    batch, loop = [], []
    for i in range(runs + 1):           # alternated: one batched run, one pass of the loop
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sb = r.scan_batch(queries)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for j in pick:
            one_query(r, queries[j])
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if i:
            batch.append((t1 - t0) * 1e3)
            loop.append((t2 - t1) * 1e3)
    plan_up_ms, emit_ms, (nrec, kb, vb, nbad) = raw_times(r, queries, runs)
    plan_ms = plan_call_ms(r, queries, runs)
    out_bytes = kb + vb + 16 * nrec
    cms = copy_ms(2 * out_bytes)
    b_ms, l_ms = statistics.median(batch), statistics.median(loop)
    per_b, per_l = b_ms * 1e3 / nq, l_ms * 1e3 / len(pick)
    return {"shape": name, "verify": bool(r.verify), "queries": nq, "not_ok": nbad, "n_large": sb.n_large,
            "n_fallback": sb.n_fallback, "records": nrec, "key_bytes": kb, "value_bytes": vb,
            "plan_ms": round(plan_ms, 3), "upload_plus_plan_ms": round(plan_up_ms, 3), "emit_ms": round(emit_ms, 3),
            "kernel_queries_per_s": round(nq / ((plan_ms + emit_ms) * 1e-3)),
            "emit_GBps_written": round(out_bytes / emit_ms / 1e6, 2),
            "copy_ms_same_bytes": round(cms, 4), "emit_fraction_of_copy": round(cms / emit_ms, 4),
            "batch_ms": round(b_ms, 2), "batch_us_per_query": round(per_b, 3), "loop_sample": len(pick),
            "loop_ms": round(l_ms, 2), "loop_us_per_query": round(per_l, 1), "loop_over_batch": round(per_l / per_b, 1),
            "sample_outputs_equal": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=20000, help="data blocks of the cfg2 file")
    ap.add_argument("--queries", type=int, default=100_000)
    ap.add_argument("--sample", type=int, default=500, help="queries the per-query loop runs")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan", "scan_bench.json"))
    a = ap.parse_args()
    from mtblx import reader, synth
    data, off, ln = synth.cfg2_file(a.blocks)
    keys = synth.cfg2_keys(synth.cfg2_file_nrec(a.blocks))
    rng = np.random.default_rng(11)
    n = keys.shape[0]
    pre = [("prefix", keys[i, :14].tobytes()) for i in rng.integers(0, n, a.queries)]
    rg = [("range", keys[i].tobytes(), keys[i + 999].tobytes()) for i in rng.integers(0, n - 1000, max(a.queries // 10, 1))]
    res = {"device": torch.cuda.get_device_name(0), "file_bytes": int(data.size), "file_records": int(n),
           "file_blocks": int(off.size), "runs": a.runs, "rows": []}
    for verify in (True, False):
        r = reader.ReaderBuilder().verify_checksums(verify).read(data)
        res["rows"].append(shape(r, "prefix14", pre, a.sample, a.runs))
        res["rows"].append(shape(r, "range1000", rg, max(a.sample // 5, 1), a.runs))
    res["accepted"] = all(x["batch_us_per_query"] < x["loop_us_per_query"] for x in res["rows"])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    if not res["accepted"]:
        sys.exit("batched per-query time is not below the loop's")


if __name__ == "__main__":
    main()

"""Rollups (rollup_records: mtblx_rollup_plan / _emit, mtblx_reduce_segments, mtblx_reduce_encode) on
cfg2-shaped records against the floor below them and the path a user had before them (DESIGN.md §4
"Rollups").

Records: cfg2's shape (16-byte keys, mtblx/synth.py) with 24-byte values of three u64 fields reduced
as (sum, min, max).  Key i = be64(i // g) || be64(i): GroupBy.length(8) cuts them into groups of g
records; g = 2, 1000 and n (every record in one group).
Legs per g, median of --runs after a warm-up, alternated in this process:
  rollup_calls     (a) the four C calls back to back over buffers allocated beforehand, by HIP events:
                   plan + emit + reduce_segments over grp_rec + reduce_encode, no read-back in between
  rollup_records   the same as a user calls it: host clock ending in a synchronize, with its three
                   read-backs (the totals, the emit's flags, reduce_segments' flags) and its allocations
  segments_only    (b) mtblx_reduce_segments alone over the same groups handed to it precomputed, by HIP
                   events: the floor; (a) / (b) is what finding the groups, their keys and values adds
  scan+host        (c) the parent commit's only way to the same table: Reader.scan_batch of the whole
                   file, the records' read-back, and itertools.groupby + Reduce.fold on the host (over
                   the first --host-records records, scaled to the file).  One ("from", "") query is one
                   wave walking every block, so scan_batch_ms is that walk, on both sides of the ratio
  reader_rollup    Reader.rollup of the same file with a fresh Reader: the parallel decode of iter() and
                   the rollup behind it, host clock ending in a synchronize
Reported besides: that the three paths give equal fields on the sampled groups.

Prints one JSON object, writes it and a README.md with the ratios to --out (a directory).  Needs the GPU."""
import argparse
import ctypes as C
import itertools
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


def make_keys(n, g):
    keys = np.empty((n, 16), np.uint8)
    i = np.arange(n, dtype=np.uint64)
    keys[:, :8] = (i // np.uint64(g)).astype(">u8").view(np.uint8).reshape(n, 8)
    keys[:, 8:] = i.astype(">u8").view(np.uint8).reshape(n, 8)
    return keys


class Calls:
    """the four C calls over buffers allocated once, sized from a first rollup_records"""

    def __init__(self, rec, group, red, ro):
        from mtblx import _lib, codec
        self.L, self.rec, self.red = _lib.lib(), rec, red
        dev = rec.key_end.device
        n, G, nf = rec.n, ro.ngroups, len(red.ops)
        self.n, self.G = n, G
        self.c = _lib.Records(codec._u(rec.keys), codec._u(rec.key_end), codec._u(rec.vals), codec._u(rec.val_end), n)
        self.g, self.spec = group.cstruct(), red.cstruct()
        self.seg = torch.tensor([0, n], dtype=torch.int64, device=dev)
        self.wsb = int(self.L.mtblx_rollup_workspace_bytes(n, 1))
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device=dev)
        self.totals = torch.zeros(2, dtype=torch.int64, device=dev)
        kb = int(ro.records.keys.numel())
        self.keys = torch.empty(max(kb, 1), dtype=torch.uint8, device=dev)
        self.key_end = torch.empty(G, dtype=torch.int64, device=dev)
        self.grp_rec = torch.empty(G + 1, dtype=torch.int64, device=dev)
        self.seg_grp = torch.empty(2, dtype=torch.int64, device=dev)
        self.flags = torch.zeros(4, dtype=torch.int32, device=dev)
        self.out = _lib.Rolled(keys=self.keys.data_ptr(), keys_cap=kb, key_end=self.key_end.data_ptr(), key_end_cap=8 * G,
                               grp_rec=self.grp_rec.data_ptr(), grp_rec_cap=8 * (G + 1), seg_grp=self.seg_grp.data_ptr(),
                               seg_grp_cap=16, flags=self.flags.data_ptr())
        self.fields = torch.empty((G, nf), dtype=torch.int64, device=dev)
        self.nbad = torch.empty(G, dtype=torch.int64, device=dev)
        self.vals = torch.empty(8 * nf * G, dtype=torch.uint8, device=dev)
        self.val_end = torch.empty(G, dtype=torch.int64, device=dev)
        self.ewsb = int(self.L.mtblx_reduce_encode_workspace_bytes(G))
        self.ews = torch.empty(self.ewsb, dtype=torch.uint8, device=dev)
        self.sh = C.c_void_p(codec._stream_handle(None))

    def segments(self):
        p = C.c_void_p
        rc = self.L.mtblx_reduce_segments(C.byref(self.c), p(self.grp_rec.data_ptr()), p(self.grp_rec.data_ptr() + 8),
                                          self.G, C.byref(self.spec), p(self.fields.data_ptr()),
                                          p(self.nbad.data_ptr()), p(self.flags.data_ptr() + 8), self.sh)
        assert rc == 0

    def rollup(self):
        p = C.c_void_p
        L = self.L
        rc = L.mtblx_rollup_plan(C.byref(self.c), C.byref(self.g), p(self.seg.data_ptr()), 1, p(self.totals.data_ptr()),
                                 p(self.ws.data_ptr()), self.wsb, self.sh)
        assert rc == 0
        rc = L.mtblx_rollup_emit(C.byref(self.c), C.byref(self.g), p(self.seg.data_ptr()), 1, C.byref(self.out),
                                 p(self.ws.data_ptr()), self.wsb, self.sh)
        assert rc == 0
        self.segments()
        rc = L.mtblx_reduce_encode(p(self.fields.data_ptr()), self.G, C.byref(self.spec), p(self.vals.data_ptr()),
                                   p(self.val_end.data_ptr()), int(self.vals.numel()), p(self.ews.data_ptr()), self.ewsb,
                                   self.sh)
        assert rc == 0


def host_groups(records, red):
    """the table on the host: itertools.groupby on the first 8 bytes, Reduce.fold per group"""
    return [(k, red.fold([v for _, v in grp])) for k, grp in itertools.groupby(records, key=lambda r: r[0][:8])]


def shape(n, g, vals, red, host_records, runs):
    from mtblx import GroupBy, reader, rollup_records, synth
    from mtblx.encode import DeviceRecords
    group = GroupBy.length(8)
    keys = make_keys(n, g)
    data, _, _ = synth.write_arrays(np.ascontiguousarray(keys).reshape(-1), vals.reshape(-1), 16, 24)
    r = reader.Reader(data)
    ends = lambda w: torch.arange(1, n + 1, dtype=torch.int64, device="cuda") * w   # noqa: E731
    rec = DeviceRecords(torch.from_numpy(keys.reshape(-1)).cuda(), ends(16), torch.from_numpy(vals.reshape(-1)).cuda(),
                        ends(24))
    whole = [("from", b"")]
    # correctness first: the three paths on the first host_records records
    ro = rollup_records(rec, group, red)
    calls = Calls(rec, group, red, ro)
    calls.rollup()
    torch.cuda.synchronize()
    assert calls.flags[0].item() == 0 and calls.totals.tolist() == [ro.ngroups, int(ro.records.keys.numel())]
    assert torch.equal(calls.fields, ro.fields) and torch.equal(calls.key_end, ro.records.key_end)
    assert torch.equal(calls.vals, ro.records.vals) and torch.equal(calls.grp_rec, ro.grp_rec)
    sb = r.scan_batch(whole, max_blocks=1 << 30)
    assert sb.served_by_kernel(0)
    m = min(host_records, n)
    table = host_groups(sb.records(0)[:m], red)
    got = ro.groups()
    for i, (k, (f, nrec, nbad)) in enumerate(table[:-1] if m < n else table):   # the last group may be cut at m
        assert got[i] == (k, f, nrec, nbad), (g, i)
    t = {k: [] for k in ("calls", "records", "segments", "scan", "readback", "fold", "reader")}
    for i in range(runs + 1):
        ms = {}
        ms["calls"], _ = events(calls.rollup)
        ms["records"], _ = wall(lambda: rollup_records(rec, group, red))
        ms["segments"], _ = events(calls.segments)
        ms["scan"], sb = wall(lambda: r.scan_batch(whole, max_blocks=1 << 30))
        ms["reader"], r2 = wall(lambda: reader.Reader(data).rollup(group, red))
        assert r2.ngroups == ro.ngroups
        t0 = time.perf_counter()
        recs = sb.records(0)                      # copies the whole batch to the host and cuts it into records
        t1 = time.perf_counter()
        host_groups(recs[:m], red)
        t2 = time.perf_counter()
        ms["readback"], ms["fold"] = (t1 - t0) * 1e3, (t2 - t1) * 1e3 * n / m
        if i:
            for k in t:
                t[k].append(ms[k])
    med = {k: statistics.median(v) for k, v in t.items()}
    host_ms = med["scan"] + med["readback"] + med["fold"]
    return {"group_size": g, "records": n, "groups": ro.ngroups,
            "rollup_calls_events_ms": round(med["calls"], 3), "segments_only_events_ms": round(med["segments"], 3),
            "rollup_calls_over_segments_only": round(med["calls"] / med["segments"], 2),
            "rollup_records_ms": round(med["records"], 2),
            "scan_batch_ms": round(med["scan"], 2), "readback_ms": round(med["readback"], 1),
            "host_groupby_fold_ms_scaled": round(med["fold"], 1), "host_records": m,
            "scan_plus_host_ms": round(host_ms, 1),
            "scan_plus_host_over_scan_plus_rollup": round(host_ms / (med["scan"] + med["records"]), 1),
            "reader_rollup_ms": round(med["reader"], 2),
            "scan_plus_host_over_reader_rollup": round(host_ms / med["reader"], 1),
            "rollup_calls_Mrec_per_s": round(n / med["calls"] / 1e3, 1), "sample_results_equal": True}


README = """# Rollups: the bench's record

`scripts/rollup_bench.py` on {device}: {records} cfg2-shaped records (16-byte keys, 24-byte values of three
u64 fields reduced as sum / min / max), `GroupBy.length(8)`, median of {runs} runs.  The JSON beside this file
holds every figure; the legs are described in the script's docstring.

| group size | groups | (a) rollup calls, ms | (b) reduce_segments alone, ms | (a) / (b) | rollup_records, ms | (c) scan + read-back + host groupby, ms | (c) / (scan + rollup_records) | Reader.rollup, ms | (c) / Reader.rollup |
|---|---|---|---|---|---|---|---|---|---|
{rows}

(a) and (b) are HIP-event times of the C calls over buffers allocated beforehand; rollup_records and (c) are host
clocks that end in a synchronize.  (c)'s groupby and fold ran over the first {host} records and is scaled to the file;
its scan is one ("from", "") query, one wave walking every block of the file, which is most of its time and is also in
the denominator of the first (c) ratio.  Reader.rollup takes a fresh Reader through iter() (the parallel decode).
No ratio is a pass condition; the tests are.
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=20000, help="sizes the input: the records of a cfg2 file of this many data blocks")
    ap.add_argument("--host-records", type=int, default=200_000, help="records the host groupby + fold runs over")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollup"))
    a = ap.parse_args()
    from mtblx import Reduce, synth
    n = synth.cfg2_file_nrec(a.blocks)
    rng = np.random.default_rng(11)
    vals = rng.integers(0, 256, (n, 24), dtype=np.uint8)
    red = Reduce("sum", "min", "max")
    res = {"device": torch.cuda.get_device_name(0), "records": int(n), "runs": a.runs, "rows": []}
    for g in (2, 1000, n):
        res["rows"].append(shape(n, g, vals, red, a.host_records, a.runs))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "rollup_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    rows = "\n".join(
        f"| {r['group_size']} | {r['groups']} | {r['rollup_calls_events_ms']} | {r['segments_only_events_ms']} | "
        f"{r['rollup_calls_over_segments_only']} | {r['rollup_records_ms']} | {r['scan_plus_host_ms']} | "
        f"{r['scan_plus_host_over_scan_plus_rollup']} | {r['reader_rollup_ms']} | {r['scan_plus_host_over_reader_rollup']} |"
        for r in res["rows"])
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write(README.format(device=res["device"], records=n, runs=a.runs, rows=rows, host=min(a.host_records, n)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()

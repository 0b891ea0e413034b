"""Varint-coded values in the reduce family against the fixed-width ones (DESIGN.md §4 "Varint-coded
values"), on the inputs of scripts/reduce_bench.py and scripts/scan_reduce_bench.py.

Records: reduce_bench's `dup10` and `hot` shapes (0.88 M records, 16 B cfg2 keys), every value three
numbers derived from the shape's random u64 x -- (x mod 2^32, that plus 16 bits of x, 10 bits of x), the
sizes of (time_first, time_last, count) -- reduced as (min, max, sum), once as 24 bytes of u64le and
once as three varints (12 bytes on average).

Leg (a), the Sorter's emit, alternating in one process, HIP events, median of --runs after a warm-up,
each leg over its own plan of the same keys:
    first     mtblx_sort_emit(FIRST) over the varint records
    u64le     mtblx_sort_emit_reduce over the 24-byte records
    varint    mtblx_sort_emit_reduce over the varint records (length pass, scan, store pass, singles)
with the plan + emit pair timed beside the emit alone.  The varint result is decoded on the host and
compared with numpy's min / max / sum per key, as is the u64le result.
Leg (b), whole path, wall time: host arrays -> Sorter(Reduce(..., encoding="varint")).insert_batch ->
write_file against the same through the callable path (decode, reduce, re-encode per group in Python):
this library's own host path, NOT the reference crate.  The two files must be byte-identical.
Leg (c), the scan walk: a file of the dup10 keys (each once) written twice, with the 24-byte and with
the varint values; mtblx_scan_plan (the counting walk) against mtblx_scan_reduce on each file, by
scan_reduce_bench.call_ms (alternating, HIP events and host clock), prefix and range queries.
No threshold is set for any leg.

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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

OPS = ("min", "max", "sum")
M = (1 << 64) - 1


def fields_of(vals8):
    """reduce_bench's 8-byte values -> u64 [n, 3]"""
    x = np.ascontiguousarray(vals8).view("<u8").reshape(-1)
    a = x & np.uint64(0xFFFFFFFF)
    return np.stack([a, a + ((x >> np.uint64(32)) & np.uint64(0xFFFF)), (x >> np.uint64(48)) & np.uint64(0x3FF)], axis=1)


def encode_varints(f):
    """u64 [n, F] -> (bytes u8 [total], END offsets i64 [n]): every row its F canonical varints back to back"""
    n, F = f.shape
    j = np.arange(10, dtype=np.uint64)
    sh = f[:, :, None] >> (np.uint64(7) * j)                       # [n, F, 10]
    more = np.zeros_like(sh, dtype=bool)
    more[:, :, :-1] = sh[:, :, 1:] != 0
    used = (sh != 0) | (j == 0)
    b = ((sh & np.uint64(0x7F)) | (more.astype(np.uint64) << np.uint64(7))).astype(np.uint8)
    return b[used], np.cumsum(used.reshape(n, -1).sum(axis=1), dtype=np.int64)


def decode_varints(buf, ends, F):
    """the inverse, in Python: -> list of F-tuples"""
    out, p = [], 0
    for e in ends:
        row = []
        for _ in range(F):
            x = s = 0
            while True:
                c = buf[p]
                p += 1
                x |= (c & 0x7F) << s
                s += 7
                if not c & 0x80:
                    break
            row.append(x)
        assert p == e
        out.append(tuple(row))
    return out


def want_groups(keys, f):
    """numpy's (min, max, sum) per key in key order -> u64 [groups, 3], the longest group"""
    n = keys.shape[0]
    k64 = keys.view(">u8").reshape(n, 2)
    order = np.lexsort((k64[:, 1], k64[:, 0]))
    sk = k64[order]
    head = np.ones(n, bool)
    head[1:] = (sk[1:] != sk[:-1]).any(axis=1)
    at = np.flatnonzero(head)
    fo = f[order]
    want = np.stack([np.minimum.reduceat(fo[:, 0], at), np.maximum.reduceat(fo[:, 1], at), np.add.reduceat(fo[:, 2], at)], axis=1)
    return want, int(np.diff(np.append(at, n)).max())


class Leg:
    """one plan over (keys, values) resident on the device, its outputs, and an emit to time"""

    def __init__(self, keys, vbytes, vends, spec):
        from mtblx import _lib, codec, encode
        self.L = codec._require_device()
        self._lib = _lib
        n = keys.shape[0]
        kends = torch.arange(1, n + 1, dtype=torch.int64, device="cuda") * 16
        self.recs = encode.DeviceRecords(torch.from_numpy(keys.reshape(-1)).cuda(), kends, torch.from_numpy(vbytes).cuda(),
                                         torch.from_numpy(vends).cuda())
        self.rec = self.recs.cstruct()
        self.wsb = int(self.L.mtblx_sort_workspace_bytes(n))
        self.ws = torch.empty(self.wsb + 256, dtype=torch.uint8, device="cuda")
        self.wp = (self.ws.data_ptr() + 255) & ~255
        self.tot = (C.c_uint64 * 6)()
        self.st = C.c_void_p(int(torch.cuda.current_stream().cuda_stream))
        self.spec = spec
        assert self.plan() == 0
        self.groups, kb, nv, vb = (int(self.tot[j]) for j in range(4))
        self.okeys = torch.empty(kb, dtype=torch.uint8, device="cuda")
        self.key_end = torch.empty(self.groups, dtype=torch.int64, device="cuda")
        self.ovals = torch.empty(vb, dtype=torch.uint8, device="cuda")
        self.val_end = torch.empty(self.groups, dtype=torch.int64, device="cuda")
        self.flags = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.out = _lib.Merged(self.okeys.data_ptr(), kb, self.key_end.data_ptr(), 8 * self.groups, self.ovals.data_ptr(), vb,
                               self.val_end.data_ptr(), 8 * self.groups, 0, 0, self.flags.data_ptr())

    def plan(self):
        return self.L.mtblx_sort_plan(C.byref(self.rec), self.tot, C.c_void_p(self.wp), self.wsb, self.st)

    def emit(self):
        if self.spec is None:
            return self.L.mtblx_sort_emit(C.byref(self.rec), self._lib.MERGE_FIRST, C.byref(self.out), C.c_void_p(self.wp),
                                          self.wsb, self.st)
        return self.L.mtblx_sort_emit_reduce(C.byref(self.rec), C.byref(self.spec), C.byref(self.out), C.c_void_p(self.wp),
                                             self.wsb, self.st)


def leg_emit(keys, vals8, runs):
    import mtblx
    n = keys.shape[0]
    f = fields_of(vals8)
    vb, ve = encode_varints(f)
    u64b, u64e = f.astype("<u8").view(np.uint8).reshape(-1), np.arange(1, n + 1, dtype=np.int64) * 24
    legs = {"first": Leg(keys, vb, ve, None), "u64le": Leg(keys, u64b, u64e, mtblx.Reduce(*OPS).cstruct()),
            "varint": Leg(keys, vb, ve, mtblx.Reduce(*OPS, encoding="varint").cstruct())}
    t = {w: {"both": [], "emit": []} for w in legs}
    for i in range(runs + 1):
        for which, g in legs.items():   # alternating
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            rc = g.plan()
            e[1].record()
            rc |= g.emit()
            e[2].record()
            torch.cuda.synchronize()
            assert rc == 0 and int(g.flags.item()) == 0, (which, rc)
            if i:   # run 0 warms up
                t[which]["both"].append(e[0].elapsed_time(e[2]))
                t[which]["emit"].append(e[1].elapsed_time(e[2]))
    want, longest = want_groups(keys, f)
    g = legs["u64le"]
    ok_u64 = bool(g.groups == len(want) and (g.ovals[: 24 * g.groups].cpu().numpy().view("<u8").reshape(-1, 3) == want).all())
    g = legs["varint"]
    ends = g.val_end.cpu().numpy()
    wb, we = encode_varints(want)
    ok_var = bool(g.groups == len(want) and (ends == we).all() and (g.ovals[: int(ends[-1])].cpu().numpy() == wb).all())
    sample = decode_varints(g.ovals[: int(ends[999])].cpu().numpy().tolist(), ends[:1000].tolist(), 3)
    ok_var = ok_var and sample == [tuple(int(x) for x in r) for r in want[:1000]]
    med = {w: {k: round(statistics.median(v), 4) for k, v in d.items()} for w, d in t.items()}
    return {"records": n, "groups": legs["varint"].groups, "longest_group": longest, "runs": runs,
            "value_bytes_in_varint": int(ve[-1]), "value_bytes_in_u64le": 24 * n, "value_bytes_out_varint": int(ends[-1]),
            "emit_first_ms": med["first"]["emit"], "emit_reduce_u64le_ms": med["u64le"]["emit"],
            "emit_reduce_varint_ms": med["varint"]["emit"],
            "plan_plus_emit_first_ms": med["first"]["both"], "plan_plus_emit_reduce_u64le_ms": med["u64le"]["both"],
            "plan_plus_emit_reduce_varint_ms": med["varint"]["both"],
            "varint_over_u64le_emit": round(med["varint"]["emit"] / med["u64le"]["emit"], 3),
            "varint_over_first_emit": round(med["varint"]["emit"] / med["first"]["emit"], 3),
            "varint_emit_over_plan_plus_emit_first": round(med["varint"]["emit"] / med["first"]["both"], 3),
            "all_emit_ms": {w: [round(x, 4) for x in d["emit"]] for w, d in t.items()},
            "u64le_correct": ok_u64, "varint_correct": ok_var}


def leg_whole(keys, vals8, runs):
    import mtblx
    from mtblx import sorter
    n = keys.shape[0]
    vb, ve = encode_varints(fields_of(vals8))
    kf, ke = keys.reshape(-1), np.arange(1, n + 1, dtype=np.uint64) * 16
    red = mtblx.Reduce(*OPS, encoding="varint")

    def dec(v):
        row, x, s = [], 0, 0
        for c in v:
            x |= (c & 0x7F) << s
            s += 7
            if not c & 0x80:
                row.append(x)
                x = s = 0
        return row

    def merge(_key, values):
        rows = [dec(v) for v in values]
        return red.encode((min(r[0] for r in rows), max(r[1] for r in rows), sum(r[2] for r in rows) & M))

    files, times = {}, {"device": [], "callable": []}
    warm = {"device": 3, "callable": 1}   # untimed runs: the device path's first ones grow the allocator's pool
    for name, m, reps in (("device", red, runs + 3), ("callable", merge, max(runs // 2, 1) + 1)):
        for i in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s = sorter.Sorter(m)
            s.insert_batch(kf, ke, vb, ve.astype(np.uint64))
            f = s.write_file(4096, 16)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if i >= warm[name]:
                times[name].append(t1 - t0)
            files[name] = f.cpu().numpy().tobytes()
    return {"records": n, "device_path_s": [round(x, 4) for x in times["device"]],
            "device_path_median_s": round(statistics.median(times["device"]), 4),
            "callable_path_s": [round(x, 4) for x in times["callable"]],
            "callable_path_median_s": round(statistics.median(times["callable"]), 4),
            "warmup_runs": warm,
            "files_identical": files["device"] == files["callable"], "file_bytes": len(files["device"]),
            "note": "callable path = the same Sorter with a Python merge function (decode, reduce, re-encode): this "
                    "library's own host path; no reference (Rust) timing exists"}


def leg_scan(keys, vals8, queries, runs):
    """the counting walk and the reducing walk over the same keys with 24-byte and with varint values"""
    import mtblx
    from mtblx import reader, sorter
    from scan_reduce_bench import call_ms
    n = keys.shape[0]
    f = fields_of(vals8)
    k64 = keys.view(">u8").reshape(n, 2)
    _, uniq = np.unique(k64, axis=0, return_index=True)       # each key once: a file holds no key twice
    keys, f = np.ascontiguousarray(keys[uniq]), f[uniq]
    n = keys.shape[0]
    rng = np.random.default_rng(11)
    pre = [("prefix", keys[i, :14].tobytes()) for i in rng.integers(0, n, queries)]
    rg = [("range", keys[i].tobytes(), keys[i + 999].tobytes()) for i in rng.integers(0, n - 1000, max(queries // 10, 1))]
    vb, ve = encode_varints(f)
    inputs = {"u64le": (f.astype("<u8").view(np.uint8).reshape(-1), np.arange(1, n + 1, dtype=np.uint64) * 24, mtblx.Reduce(*OPS)),
              "varint": (vb, ve.astype(np.uint64), mtblx.Reduce(*OPS, encoding="varint"))}
    rows, answers = [], {}
    for enc, (vbytes, vends, red) in inputs.items():
        s = sorter.Sorter("first")
        s.insert_batch(keys.reshape(-1), np.arange(1, n + 1, dtype=np.uint64) * 16, vbytes, vends)
        data = s.write_file(4096, 16)
        r = reader.ReaderBuilder().verify_checksums(False).read(data)
        for name, qs in (("prefix14", pre), ("range1000", rg)):
            rb = r.reduce_batch(qs, red)
            answers[(enc, name)] = [(rb.values(i),) + rb.counts(i) for i in range(0, len(qs), max(len(qs) // 200, 1))]
            plan_ms, reduce_ms, plan_ev, reduce_ev = call_ms(r, qs, red, runs)
            rows.append({"encoding": enc, "shape": name, "queries": len(qs), "file_bytes": int(data.numel()),
                         "plan_call_events_ms": round(plan_ev, 3), "reduce_call_events_ms": round(reduce_ev, 3),
                         "reduce_events_over_plan_events": round(reduce_ev / plan_ev, 3),
                         "plan_call_ms": round(plan_ms, 3), "reduce_call_ms": round(reduce_ms, 3)})
    same = all(answers[("u64le", s)] == answers[("varint", s)] for s in ("prefix14", "range1000"))
    return {"records": n, "rows": rows, "sampled_answers_equal_across_encodings": same}


def main():
    from reduce_bench import make_records
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=880_000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--queries", type=int, default=100_000)
    ap.add_argument("--leg", choices=["emit", "whole", "scan", "all"], default="all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reduce_varint", "reduce_varint_bench.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "records": a.records, "ops": list(OPS)}
    if a.leg in ("emit", "all"):
        res["sorter_emit"] = {}
        for shape in ("dup10", "hot"):
            keys, vals = make_records(a.records, shape)
            res["sorter_emit"][shape] = leg_emit(keys, vals, a.runs)
            torch.cuda.empty_cache()
    if a.leg in ("whole", "all"):
        keys, vals = make_records(a.records, "dup10")
        res["whole_path"] = leg_whole(keys, vals, max(a.runs // 2, 2))
    if a.leg in ("scan", "all"):
        keys, vals = make_records(a.records, "dup10")
        res["scan_walk"] = leg_scan(keys, vals, a.queries, a.runs)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

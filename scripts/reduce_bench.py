"""The device merge functions (mtblx.Reduce, csrc/reduce_dev.h) on records of the cfg2 key shape
(DESIGN.md §4 "Device merge functions").

Records: one cfg2 key stream (16 B keys = be64 counter || 8 random bytes, mtblx/synth.py) with
8-byte values (one little-endian u64 each), 0.88 M records, shuffled with a fixed seed, in two shapes:
  dup10   a tenth of the keys occur twice (the shape of scripts/sort_bench.py)
  hot     half of all records carry one key: one group of 0.44 M values, 430 tiles long

Leg (a), the Sorter's emit: mtblx_sort_plan + mtblx_sort_emit_reduce(sum) against mtblx_sort_plan +
mtblx_sort_emit(FIRST) over the records resident on the device, alternating in one process, `--runs`
times each after a warm-up, HIP events around the plan + emit pair and around the emit alone.  FIRST
has the same layout and writes the same number of bytes, so the difference is the reduction
(k_reduce_tile + k_reduce_edges).  The ratio of the two shapes' reduce times shows whether long
groups cost more than short ones.
Leg (b), whole path, wall time: unsorted records in host memory -> Sorter(Reduce("sum")).insert_batch
-> write_file, against the same through the callable path (Sorter(lambda k, vs: ...) with the same
function: the groups copied to the host, cut into bytes, summed per group in Python, uploaded
again).  The two files must be byte-identical.  That comparator is this library's own host path, NOT
the reference crate: Rust cannot be built here, so no reference timing exists.  No threshold is set
for either leg.

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


def make_records(n, shape, seed=0x6D74626C04):
    """-> keys u8 [n, 16], vals u8 [n, 8], shuffled"""
    from mtblx import synth
    rng = np.random.default_rng(seed + 1)
    if shape == "dup10":
        nkeys = int(round(n / 1.1))
        extra = n - nkeys
    else:
        nkeys = n - n // 2 + 1
        extra = n // 2 - 1
    keys, _, kl, _ = synth.cfg2_arrays(nkeys, seed)
    keys = keys.reshape(nkeys, kl)
    again = rng.choice(nkeys, size=extra, replace=False) if shape == "dup10" else np.full(extra, nkeys // 2)
    keys = np.concatenate([keys, keys[again]])
    vals = rng.integers(0, 1 << 63, size=n, dtype=np.uint64).astype("<u8").view(np.uint8).reshape(n, 8)
    order = rng.permutation(n)
    return np.ascontiguousarray(keys[order]), np.ascontiguousarray(vals[order])


def leg_emit(keys, vals, runs):
    import mtblx
    from mtblx import _lib, codec, encode
    L = codec._require_device()
    n = keys.shape[0]
    ends = torch.arange(1, n + 1, dtype=torch.int64, device="cuda")
    recs = encode.DeviceRecords(torch.from_numpy(keys.reshape(-1)).cuda(), ends * 16,
                                torch.from_numpy(vals.reshape(-1)).cuda(), ends * 8)
    rec = recs.cstruct()
    wsb = int(L.mtblx_sort_workspace_bytes(n))
    ws = torch.empty(wsb + 256, dtype=torch.uint8, device="cuda")
    wp = (ws.data_ptr() + 255) & ~255
    tot = (C.c_uint64 * 6)()
    st = C.c_void_p(int(torch.cuda.current_stream().cuda_stream))
    spec = mtblx.Reduce("sum").cstruct()
    assert L.mtblx_sort_plan(C.byref(rec), tot, C.c_void_p(wp), wsb, st) == 0
    groups, kb, nv, vb = (int(tot[j]) for j in range(4))
    okeys = torch.empty(kb, dtype=torch.uint8, device="cuda")
    key_end = torch.empty(groups, dtype=torch.int64, device="cuda")
    ovals = torch.empty(vb, dtype=torch.uint8, device="cuda")
    val_end = torch.empty(groups, dtype=torch.int64, device="cuda")
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = _lib.Merged(okeys.data_ptr(), kb, key_end.data_ptr(), 8 * groups, ovals.data_ptr(), vb, val_end.data_ptr(),
                      8 * groups, 0, 0, flags.data_ptr())
    t = {"first": {"both": [], "emit": []}, "reduce": {"both": [], "emit": []}}
    for i in range(runs + 1):
        for which in ("first", "reduce"):   # alternating
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            rc = L.mtblx_sort_plan(C.byref(rec), tot, C.c_void_p(wp), wsb, st)
            e[1].record()
            if which == "first":
                rc |= L.mtblx_sort_emit(C.byref(rec), _lib.MERGE_FIRST, C.byref(out), C.c_void_p(wp), wsb, st)
            else:
                rc |= L.mtblx_sort_emit_reduce(C.byref(rec), C.byref(spec), C.byref(out), C.c_void_p(wp), wsb, st)
            e[2].record()
            torch.cuda.synchronize()
            assert rc == 0 and int(flags.item()) == 0
            if i:   # run 0 warms up
                t[which]["both"].append(e[0].elapsed_time(e[2]))
                t[which]["emit"].append(e[1].elapsed_time(e[2]))
    # the result, once, against numpy: the sum per key in key order
    k64 = keys.view(">u8").reshape(n, 2)
    order = np.lexsort((k64[:, 1], k64[:, 0]))
    sk = k64[order]
    head = np.ones(n, bool)
    head[1:] = (sk[1:] != sk[:-1]).any(axis=1)
    want = np.add.reduceat(vals.view("<u8").reshape(n)[order], np.flatnonzero(head))
    correct = bool(groups == int(head.sum()) and (ovals[: 8 * groups].cpu().numpy().view("<u8") == want).all())
    med = {w: {k: round(statistics.median(v), 4) for k, v in d.items()} for w, d in t.items()}
    return {"records": n, "groups": groups, "longest_group": int(np.diff(np.append(np.flatnonzero(head), n)).max()),
            "runs": runs, "plan_plus_emit_first_ms": med["first"]["both"], "plan_plus_emit_reduce_ms": med["reduce"]["both"],
            "emit_first_ms": med["first"]["emit"], "emit_reduce_ms": med["reduce"]["emit"],
            "reduction_ms": round(med["reduce"]["emit"] - med["first"]["emit"], 4),
            "all_emit_first_ms": [round(x, 4) for x in t["first"]["emit"]],
            "all_emit_reduce_ms": [round(x, 4) for x in t["reduce"]["emit"]], "sums_correct": correct}


def leg_whole(keys, vals, runs):
    import mtblx
    from mtblx import sorter
    n = keys.shape[0]
    kf, vf = keys.reshape(-1), vals.reshape(-1)
    ke, ve = np.arange(1, n + 1, dtype=np.uint64) * 16, np.arange(1, n + 1, dtype=np.uint64) * 8
    mask = (1 << 64) - 1

    def add(_key, values):
        return (sum(int.from_bytes(v, "little") for v in values) & mask).to_bytes(8, "little")

    files, times = {}, {"device": [], "callable": []}
    for name, merge, reps in (("device", mtblx.Reduce("sum"), runs + 1), ("callable", add, max(runs // 2, 1) + 1)):
        for i in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s = sorter.Sorter(merge)
            s.insert_batch(kf, ke, vf, ve)
            f = s.write_file(4096, 16)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if i:   # run 0 warms up
                times[name].append(t1 - t0)
            files[name] = f.cpu().numpy().tobytes()
    return {"records": n, "device_path_s": [round(x, 4) for x in times["device"]],
            "device_path_median_s": round(statistics.median(times["device"]), 4),
            "callable_path_s": [round(x, 4) for x in times["callable"]],
            "callable_path_median_s": round(statistics.median(times["callable"]), 4),
            "files_identical": files["device"] == files["callable"], "file_bytes": len(files["device"]),
            "note": "device path = host arrays -> Sorter(Reduce('sum')).insert_batch -> write_file (upload included); "
                    "callable path = the same with Sorter(lambda): this library's own host path; no reference (Rust) "
                    "timing exists"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=880_000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--leg", choices=["emit", "whole", "both"], default="both")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reduce", "reduce_bench.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "records": a.records}
    if a.leg in ("emit", "both"):
        res["sorter_emit"] = {}
        for shape in ("dup10", "hot"):
            keys, vals = make_records(a.records, shape)
            res["sorter_emit"][shape] = leg_emit(keys, vals, a.runs)
            torch.cuda.empty_cache()
        d, h = res["sorter_emit"]["dup10"], res["sorter_emit"]["hot"]
        res["sorter_emit"]["hot_over_dup10_emit_reduce"] = round(h["emit_reduce_ms"] / d["emit_reduce_ms"], 3)
    if a.leg in ("whole", "both"):
        keys, vals = make_records(a.records, "dup10")
        res["whole_path"] = leg_whole(keys, vals, max(a.runs // 2, 2))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

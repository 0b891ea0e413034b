"""Set operations on the device Merger: what the selection costs (DESIGN.md §4 "Set operations").

Sources: the 8 cfg2-shaped sources of scripts/merge_bench.py (16 B keys, 64 B values, about 0.88 M
records, a tenth of the keys in two sources).

Leg (a), the plans, HIP events around each synchronous call, `--runs` rounds after a warm-up round,
the variants alternating inside every round so that they share whatever else the machine does:
  plan          mtblx_merge_plan, the plan as it was before the selection existed
  union         mtblx_merge_plan_select with {0, 0, 1, 64}: the same plan plus k_group_select, which
                rejects nothing -- the difference to `plan` is the kernel's cost
  exactly_one   max_count = 1
  difference    require = source 0, exclude = the other seven
and mtblx_merge_plan_timed in the same rounds: its per-pass time (one k_merge_pass over all
handles) is the yardstick the selection's cost is reported against, its grouping phase the part of
the plan the new kernel sits in.
Leg (b), `new \\ old` end to end, wall time: two .mtbl files of the same shape in host memory (0.88 M
records together, half of the keys in both) -> setops.diff_files, against the only way to get that
file without the selection: Merger([new, old]).groups(), the read-back of every group, a Python
filter and the host Writer.  A group does not say which source a value came from, so the filter
reads it off the value's first byte, where these synthetic sources carry their number; the bytes
of the two files must be identical.

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

import merge_bench as mb  # noqa: E402

NSRC = mb.NSRC


def _device_records(sources):
    from mtblx import encode
    return [encode.DeviceRecords(torch.from_numpy(k.reshape(-1).copy()).cuda(),
                                 torch.arange(1, k.shape[0] + 1, dtype=torch.int64, device="cuda") * 16,
                                 torch.from_numpy(v.reshape(-1).copy()).cuda(),
                                 torch.arange(1, k.shape[0] + 1, dtype=torch.int64, device="cuda") * 64)
            for k, v in sources]


def leg_plans(sources, runs):
    from mtblx import Select, _lib, codec
    L = codec._require_device()
    dev = _device_records(sources)
    arr = (_lib.Records * NSRC)()
    for i, r in enumerate(dev):
        arr[i] = r.cstruct()
    n = sum(r.n for r in dev)
    wsb = int(L.mtblx_merge_workspace_bytes(n, NSRC))
    ws = torch.empty(wsb + 256, dtype=torch.uint8, device="cuda")
    wp = C.c_void_p((ws.data_ptr() + 255) & ~255)
    st = C.c_void_p(int(torch.cuda.current_stream().cuda_stream))
    npass = 3
    rules = {"union": Select.union(), "exactly_one": Select.exactly_one(),
             "difference": Select.difference(0, range(1, NSRC))}
    specs = {k: v.cstruct() for k, v in rules.items()}
    tot = (C.c_uint64 * 8)()
    ms = (C.c_float * (npass + 2))()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = fn()
        e1.record()
        torch.cuda.synchronize()
        assert rc == 0, rc
        return e0.elapsed_time(e1)

    calls = {"plan": lambda: L.mtblx_merge_plan(arr, NSRC, tot, wp, wsb, st)}
    for name, spec in specs.items():
        calls[name] = (lambda sp: lambda: L.mtblx_merge_plan_select(arr, NSRC, C.byref(sp), tot, wp, wsb, st))(spec)
    t = {k: [] for k in calls}
    totals, phases = {}, []
    for i in range(runs + 1):
        order = list(calls)
        order = order[i % len(order):] + order[: i % len(order)]      # every variant takes every place in the round
        for name in order:
            x = timed(calls[name])
            totals[name] = [int(v) for v in tot] if name != "plan" else [int(v) for v in tot][:6]
            if i:   # round 0 warms up
                t[name].append(x)
        rc = L.mtblx_merge_plan_timed(arr, NSRC, tot, wp, wsb, st, ms, npass + 2)
        assert rc == 0, rc
        if i:
            phases.append([float(v) for v in ms])
    med = {k: statistics.median(v) for k, v in t.items()}
    pass_ms = statistics.median(statistics.median(r[1 + p] for p in range(npass)) for r in phases)
    grouping_ms = statistics.median(r[npass + 1] for r in phases)
    paired = {k: statistics.median(a - b for a, b in zip(t[k], t["plan"])) for k in specs}
    # the kept groups of the union plan are the plain plan's, and what a rule leaves out adds up
    assert totals["union"][:6] == totals["plan"] and totals["union"][6:] == [0, 0]
    for k in specs:
        assert totals[k][0] + totals[k][6] == totals["plan"][0] and totals[k][2] + totals[k][7] == totals["plan"][2]
    return {
        "records": n, "runs": runs, "passes": npass,
        "call_ms_median": {k: round(v, 4) for k, v in med.items()},
        "call_ms_min": {k: round(min(v), 4) for k, v in t.items()},
        "call_ms_spread": {k: round(max(v) - min(v), 4) for k, v in t.items()},
        "select_minus_plan_ms_paired_median": {k: round(v, 4) for k, v in paired.items()},
        "merge_pass_ms": round(pass_ms, 4), "grouping_phase_ms": round(grouping_ms, 4),
        "union_cost_in_passes": round(paired["union"] / pass_ms, 3),
        # one 4-byte source word (a 16-byte handle's sector) and a flag byte read, a flag byte written
        "select_bytes_model": (16 + 1 + 1) * n,
        "totals": totals,
    }


def two_files(nkeys, seed=0x6D74626C03):
    """`new` and `old`: one cfg2 key stream dealt to two sources, half of the keys in both; a value's
    first byte is its source's number (0 = new)"""
    from mtblx import synth
    keys, vals, kl, vl = synth.cfg2_arrays(nkeys, seed)
    keys, vals = keys.reshape(nkeys, kl), vals.reshape(nkeys, vl)
    rng = np.random.default_rng(seed + 1)
    home = rng.integers(0, 2, nkeys)
    both = rng.random(nkeys) < 0.5
    out = []
    for s in range(2):
        m = (home == s) | both
        v = vals[m].copy()
        v[:, 0] = s
        out.append((keys[m], v))
    return mb.write_files(out), sum(int(k.shape[0]) for k, _ in out)


def leg_diff(files, runs):
    from mtblx import merger, reader, setops, writer
    new, old = files
    dev_t, host_t = [], []
    out_dev = out_host = None
    for i in range(runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f = setops.diff_files(new, old, block_size=4096, restart_interval=16)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if i:
            dev_t.append(t1 - t0)
        out_dev = f
    kept = 0
    for i in range(max(runs // 2, 1)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        groups = merger.Merger([reader.Reader(new), reader.Reader(old)], "first").groups().to_list()
        w = writer.Writer(4096, 16)
        kept = 0
        for k, vs in groups:
            if len(vs) == 1 and vs[0][0] == 0:      # held by `new` alone
                w.insert(k, vs[0])
                kept += 1
        out_host = w.into_inner()
        t1 = time.perf_counter()
        host_t.append(t1 - t0)
    same = out_dev.cpu().numpy().tobytes() == out_host
    assert same, "diff_files and the host path wrote different files"
    return {"device_path_s": [round(x, 4) for x in dev_t], "device_path_median_s": round(statistics.median(dev_t), 4),
            "host_path_s": [round(x, 4) for x in host_t], "host_path_median_s": round(statistics.median(host_t), 4),
            "files_identical": same, "file_bytes": len(out_host), "records_kept": kept,
            "note": "host path = Merger.groups(), its read-back, a Python filter on the value's source byte, the host "
                    "Writer"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=800_000, help="distinct keys dealt to the 8 sources")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--no-diff", action="store_true", help="leg (a) only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select", "select_bench.json"))
    a = ap.parse_args()
    sources, shared = mb.make_sources(a.keys, 0.1)
    res = {"device": torch.cuda.get_device_name(0), "keys": a.keys, "keys_in_two_sources": shared, "nsrc": NSRC}
    res["plans"] = leg_plans(sources, a.runs)
    if not a.no_diff:
        files, nrec = two_files(int(a.keys * 1.1 / 1.5))   # 1.5 records per key there, 1.1 here: the same record count
        res["diff_files"] = leg_diff(files, max(a.runs // 4, 2))
        res["diff_files"]["records_in"] = nrec
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

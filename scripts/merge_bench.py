"""The device Merger on 8 sources of the cfg2 record shape (DESIGN.md "Merger").

Sources: one cfg2 key stream (16 B keys = be64 counter || 8 random bytes, 64 B values,
mtblx/synth.py) dealt to 8 sources by rank; about a tenth of the keys are also given to a second
source, so about a tenth of the keys collide across sources.

Leg (a), phases: mtblx_merge_plan_timed + mtblx_merge_emit (CONCAT) over the sources' records
resident on the device, `--runs` times after a warm-up; per phase (handle build, each merge pass,
grouping, emit) the median HIP-event time, the bytes the phase must read and write (the formulas
are in `phase_bytes` below: handle and grouping arrays, END offsets, key and value bytes; the key
bytes a tie-break reads are NOT counted), and that traffic as a fraction of what mtblx_stream_copy
reaches moving the same number of bytes in this process (the in-repo copy ceiling).
Leg (b), whole path, wall time: 8 .mtbl files in host memory -> Reader (upload + device scan) ->
Merger("concat") -> write_file, everything after the upload resident on the device; against the
path a user has without the device merge: the same 8 files scanned by the same Reader, their
records pulled to the host (Reader.iter().records()), merged by Python's heapq.merge with the
groups' values joined, and written by the host Writer.  That comparator is this library's own
host path, NOT the reference crate: Rust cannot be built here, so no reference timing exists.

Prints one JSON object (and writes it to --out).  Needs the GPU."""
import argparse
import ctypes as C
import heapq
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

NSRC = 8


def make_sources(nkeys, dup=0.1, seed=0x6D74626C02):
    """-> per source (keys u8 [n,16], vals u8 [n,64]) sorted by key"""
    from mtblx import synth
    keys, vals, kl, vl = synth.cfg2_arrays(nkeys, seed)
    keys, vals = keys.reshape(nkeys, kl), vals.reshape(nkeys, vl)
    rng = np.random.default_rng(seed + 1)
    home = rng.integers(0, NSRC, nkeys)
    also = np.where(rng.random(nkeys) < dup, (home + rng.integers(1, NSRC, nkeys)) % NSRC, -1)
    out = []
    for s in range(NSRC):
        m = (home == s) | (also == s)
        v = vals[m].copy()
        v[:, 0] = s   # the copies of a key differ by source
        out.append((keys[m], v))
    return out, int((also >= 0).sum())


def write_files(sources):
    from mtblx import synth
    return [synth.write_arrays(k.reshape(-1), v.reshape(-1), 16, 64)[0].tobytes() for k, v in sources]


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


def leg_phases(sources, runs):
    from mtblx import _lib, codec, encode
    L = codec._require_device()
    dev = [encode.DeviceRecords(torch.from_numpy(k.reshape(-1).copy()).cuda(),
                                torch.arange(1, k.shape[0] + 1, dtype=torch.int64, device="cuda") * 16,
                                torch.from_numpy(v.reshape(-1).copy()).cuda(),
                                torch.arange(1, k.shape[0] + 1, dtype=torch.int64, device="cuda") * 64)
           for k, v in sources]
    arr = (_lib.Records * NSRC)()
    for i, r in enumerate(dev):
        arr[i] = r.cstruct()
    n = sum(r.n for r in dev)
    wsb = int(L.mtblx_merge_workspace_bytes(n, NSRC))
    ws = torch.empty(wsb + 256, dtype=torch.uint8, device="cuda")
    wp = (ws.data_ptr() + 255) & ~255
    tot = (C.c_uint64 * 6)()
    npass = 3
    ms = (C.c_float * (npass + 2))()
    st = C.c_void_p(int(torch.cuda.current_stream().cuda_stream))
    rows, emit = [], []
    out = None
    for i in range(runs + 1):
        rc = L.mtblx_merge_plan_timed(arr, NSRC, tot, C.c_void_p(wp), wsb, st, ms, npass + 2)
        assert rc == 0, rc
        groups, kb, nv, vb = (int(tot[j]) for j in range(4))
        if out is None:
            keys = torch.empty(kb, dtype=torch.uint8, device="cuda")
            key_end = torch.empty(groups, dtype=torch.int64, device="cuda")
            vals = torch.empty(vb, dtype=torch.uint8, device="cuda")
            val_end = torch.empty(groups, dtype=torch.int64, device="cuda")
            flags = torch.zeros(1, dtype=torch.int32, device="cuda")
            out = _lib.Merged(keys.data_ptr(), kb, key_end.data_ptr(), 8 * groups, vals.data_ptr(), vb,
                              val_end.data_ptr(), 8 * groups, 0, 0, flags.data_ptr())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = L.mtblx_merge_emit(arr, NSRC, _lib.MERGE_CONCAT, C.byref(out), C.c_void_p(wp), wsb, st)
        e1.record()
        torch.cuda.synchronize()
        assert rc == 0 and int(flags.item()) == 0
        if i:   # run 0 warms up
            rows.append([float(x) for x in ms])
            emit.append(e0.elapsed_time(e1))
    med = [statistics.median(r[j] for r in rows) for j in range(npass + 2)]
    kin = sum(int(r.keys.numel()) for r in dev)
    vin = sum(int(r.vals.numel()) for r in dev)
    # what each phase must move (read + written), in bytes
    phase_bytes = {
        "build": 8 * n + kin + 16 * n,                       # key END offsets + key bytes (order check) -> handles
        "pass": 16 * n + 16 * n,                             # handles in -> handles out
        "grouping": (16 + 8) * n + n                         # flags: handles, key ENDs -> flag bytes
                    + 2 * ((16 + 1 + 16) * n) + 40 * n,      # sums + apply: handles, flags, both ENDs -> 40 B of sums
        "emit": (16 + 1 + 40 + 16) * n + kb + vb             # handles, flags, sums, ENDs, the bytes gathered
                + kb + vb + 16 * groups,                     # -> keys, values, two END arrays
    }
    names = ["build"] + [f"pass{p}" for p in range(npass)] + ["grouping", "emit"]
    times = med + [statistics.median(emit)]
    phases = []
    for name, t in zip(names, times):
        b = phase_bytes["pass" if name.startswith("pass") else name]
        c = copy_ms(b)
        phases.append({"phase": name, "ms": round(t, 4), "bytes": b, "GBps": round(b / t / 1e6, 1),
                       "copy_ms_same_bytes": round(c, 4), "fraction_of_copy": round(c / t, 3)})
    return {"records": n, "groups": groups, "key_bytes_in": kin, "value_bytes_in": vin, "key_bytes_out": kb,
            "value_bytes_out": vb, "runs": runs, "phases": phases,
            "plan_plus_emit_ms": round(sum(times), 4)}, (keys, key_end, vals, val_end)


def leg_whole(files, runs):
    from mtblx import merger, reader, writer
    dev_t, host_t = [], []
    out_dev = out_host = None
    for i in range(runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rd = [reader.Reader(f) for f in files]
        f = merger.Merger.builder("concat").extend(rd).build().write_file(4096, 16)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if i:
            dev_t.append(t1 - t0)
        out_dev = f
    for i in range(max(runs // 2, 1)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        recs = [reader.Reader(f).iter().records() for f in files]
        w = writer.Writer(4096, 16)
        pk, pv = None, None
        for k, _, v in heapq.merge(*[[(k, s, v) for k, v in r] for s, r in enumerate(recs)]):
            if k == pk:
                pv += v
                continue
            if pk is not None:
                w.insert(pk, pv)
            pk, pv = k, v
        if pk is not None:
            w.insert(pk, pv)
        out_host = w.into_inner()
        t1 = time.perf_counter()
        host_t.append(t1 - t0)
    same = out_dev.cpu().numpy().tobytes() == out_host
    return {"device_path_s": [round(x, 4) for x in dev_t], "device_path_median_s": round(statistics.median(dev_t), 4),
            "host_path_s": [round(x, 4) for x in host_t], "host_path_median_s": round(statistics.median(host_t), 4),
            "files_identical": same, "file_bytes": len(out_host),
            "note": "host path = this library's Reader + Python heapq.merge + host Writer; no reference (Rust) timing exists"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=800_000, help="distinct keys dealt to the 8 sources")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--dup", type=float, default=0.1, help="fraction of the keys given to a second source")
    ap.add_argument("--no-whole", action="store_true", help="leg (a) only (a large --keys makes the Python host path slow)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge", "merge_bench.json"))
    a = ap.parse_args()
    sources, shared = make_sources(a.keys, a.dup)
    res = {"device": torch.cuda.get_device_name(0), "keys": a.keys, "keys_in_two_sources": shared, "nsrc": NSRC}
    res["phases"], _ = leg_phases(sources, a.runs)
    if not a.no_whole:
        res["whole_path"] = leg_whole(write_files(sources), max(a.runs // 2, 2))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

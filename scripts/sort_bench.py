"""The device Sorter on unsorted records of the cfg2 record shape (DESIGN.md "The Sorter").

Records: one cfg2 key stream (16 B keys = be64 counter || 8 random bytes, 64 B values,
mtblx/synth.py); a tenth of the keys occur twice (the copies differ in their first value byte);
the order is shuffled with a fixed seed.  Sizes: 0.88 M and 8.8 M records (--keys 800000 8000000).

Leg (a), phases: mtblx_sort_plan_timed + mtblx_sort_emit (CONCAT) over the records resident on the
device, `--runs` times after a warm-up; per phase (shared-prefix scan, tile sort, each merge pass,
grouping, emit) the median HIP-event time, the bytes the phase must read and write (the formulas are
in `phase_bytes` below; the key bytes a tie-break reads are NOT counted), and that traffic as a
fraction of what mtblx_stream_copy reaches moving the same number of bytes in this process (the
in-repo copy ceiling).  Beside it, in the same process: torch.sort of the records' 8-byte key
prefixes alone, i.e. what a fixed-width-key sort of the same count costs.  That is recorded, not a
bar: it moves no key or value bytes and settles no tie.
Leg (b), whole path, wall time: unsorted records in host memory -> Sorter("concat").insert_batch ->
write_file, against the path a user has without the device sort: the same records sorted by
Python's `sorted`, grouped with the values joined, and written by the host Writer.  The two files
must be byte-identical.  That comparator is this library's own host path, NOT the reference crate:
Rust cannot be built here, so no reference timing exists.  Run for the sizes up to --whole-max
records (the Python path takes minutes at 8.8 M).

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

from merge_bench import copy_ms  # noqa: E402  (scripts/ is sys.path[0] when this file is run)


def make_records(nkeys, dup=0.1, seed=0x6D74626C03):
    """-> keys u8 [n, 16], vals u8 [n, 64], n = nkeys + dup * nkeys, shuffled"""
    from mtblx import synth
    keys, vals, kl, vl = synth.cfg2_arrays(nkeys, seed)
    keys, vals = keys.reshape(nkeys, kl), vals.reshape(nkeys, vl)
    rng = np.random.default_rng(seed + 1)
    twice = rng.choice(nkeys, size=int(nkeys * dup), replace=False)
    keys = np.concatenate([keys, keys[twice]])
    vals = np.concatenate([vals, vals[twice]])
    vals[nkeys:, 0] ^= 0xFF   # the copies of a key differ
    order = rng.permutation(keys.shape[0])
    return np.ascontiguousarray(keys[order]), np.ascontiguousarray(vals[order])


def leg_phases(keys, vals, runs):
    from mtblx import _lib, codec, encode
    L = codec._require_device()
    n = keys.shape[0]
    recs = encode.DeviceRecords(torch.from_numpy(keys.reshape(-1)).cuda(),
                                torch.arange(1, n + 1, dtype=torch.int64, device="cuda") * 16,
                                torch.from_numpy(vals.reshape(-1)).cuda(),
                                torch.arange(1, n + 1, dtype=torch.int64, device="cuda") * 64)
    rec = recs.cstruct()
    wsb = int(L.mtblx_sort_workspace_bytes(n))
    ws = torch.empty(wsb + 256, dtype=torch.uint8, device="cuda")
    wp = (ws.data_ptr() + 255) & ~255
    tot = (C.c_uint64 * 6)()
    tiles = (n + _lib.SORT_TILE - 1) // _lib.SORT_TILE
    npass = max(tiles - 1, 0).bit_length()
    ms = (C.c_float * (npass + 3))()
    st = C.c_void_p(int(torch.cuda.current_stream().cuda_stream))
    rows, emit = [], []
    out = None
    for i in range(runs + 1):
        rc = L.mtblx_sort_plan_timed(C.byref(rec), tot, C.c_void_p(wp), wsb, st, ms, npass + 3)
        assert rc == 0, rc
        groups, kb, nv, vb = (int(tot[j]) for j in range(4))
        if out is None:
            okeys = torch.empty(kb, dtype=torch.uint8, device="cuda")
            key_end = torch.empty(groups, dtype=torch.int64, device="cuda")
            ovals = torch.empty(vb, dtype=torch.uint8, device="cuda")
            val_end = torch.empty(groups, dtype=torch.int64, device="cuda")
            flags = torch.zeros(1, dtype=torch.int32, device="cuda")
            out = _lib.Merged(okeys.data_ptr(), kb, key_end.data_ptr(), 8 * groups, ovals.data_ptr(), vb,
                              val_end.data_ptr(), 8 * groups, 0, 0, flags.data_ptr())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = L.mtblx_sort_emit(C.byref(rec), _lib.MERGE_CONCAT, C.byref(out), C.c_void_p(wp), wsb, st)
        e1.record()
        torch.cuda.synchronize()
        assert rc == 0 and int(flags.item()) == 0
        if i:   # run 0 warms up
            rows.append([float(x) for x in ms])
            emit.append(e0.elapsed_time(e1))
    med = [statistics.median(r[j] for r in rows) for j in range(npass + 3)]
    kin, vin = int(recs.keys.numel()), int(recs.vals.numel())
    # what each phase must move (read + written), in bytes
    phase_bytes = {
        "skip": 8 * n + kin,                                 # key END offsets + key bytes (at most: up to the shared length)
        "tile_sort": 8 * n + kin + 16 * n,                   # key END offsets + key bytes -> sorted handles
        "pass": 16 * n + 16 * n,                             # handles in -> handles out
        "grouping": (16 + 8) * n + n                         # flags: handles, key ENDs -> flag bytes
                    + 2 * ((16 + 1 + 16) * n) + 40 * n,      # sums + apply: handles, flags, both ENDs -> 40 B of sums
        "emit": (16 + 1 + 40 + 16) * n + kb + vb             # handles, flags, sums, ENDs, the bytes gathered
                + kb + vb + 16 * groups,                     # -> keys, values, two END arrays
    }
    names = ["skip", "tile_sort"] + [f"pass{p}" for p in range(npass)] + ["grouping", "emit"]
    times = med + [statistics.median(emit)]
    copies = {}
    phases = []
    for name, t in zip(names, times):
        b = phase_bytes["pass" if name.startswith("pass") else name]
        if b not in copies:
            copies[b] = copy_ms(b)
        c = copies[b]
        phases.append({"phase": name, "ms": round(t, 4), "bytes": b, "GBps": round(b / t / 1e6, 1),
                       "copy_ms_same_bytes": round(c, 4), "fraction_of_copy": round(c / t, 3)})
    # a fixed-width-key sort of the same count: torch.sort of the first 8 key bytes as one word
    pre = torch.from_numpy(keys[:, :8].copy().view(">u8").astype(np.int64).reshape(-1)).cuda()
    ts = []
    for i in range(runs + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.sort(pre)
        e1.record()
        torch.cuda.synchronize()
        if i:
            ts.append(e0.elapsed_time(e1))
    return {"records": n, "groups": groups, "tiles": tiles, "passes": npass, "key_bytes_in": kin, "value_bytes_in": vin,
            "key_bytes_out": kb, "value_bytes_out": vb, "runs": runs, "phases": phases,
            "plan_ms": round(sum(med), 4), "plan_plus_emit_ms": round(sum(times), 4),
            "torch_sort_8B_prefixes_ms": round(statistics.median(ts), 4),
            "torch_sort_note": "values and indices of n int64 words; no key or value bytes moved, no ties settled: "
                               "recorded for scale, not a bar"}


def leg_whole(keys, vals, runs):
    from mtblx import sorter, writer
    n = keys.shape[0]
    kf, vf = keys.reshape(-1), vals.reshape(-1)
    ke, ve = np.arange(1, n + 1, dtype=np.uint64) * 16, np.arange(1, n + 1, dtype=np.uint64) * 64
    dev_t, host_t = [], []
    out_dev = out_host = None
    for i in range(runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = sorter.Sorter("concat")
        s.insert_batch(kf, ke, vf, ve)
        f = s.write_file(4096, 16)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if i:
            dev_t.append(t1 - t0)
        out_dev, chunks = f, list(s.chunk_sizes)
    for i in range(max(runs // 2, 1)):
        t0 = time.perf_counter()
        kb, vb = kf.tobytes(), vf.tobytes()
        recs = sorted(((kb[16 * j: 16 * j + 16], vb[64 * j: 64 * j + 64]) for j in range(n)), key=lambda r: r[0])
        w = writer.Writer(4096, 16)
        pk, pv = None, None
        for k, v in recs:
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
    return {"records": n, "chunk_sizes": chunks,
            "device_path_s": [round(x, 4) for x in dev_t], "device_path_median_s": round(statistics.median(dev_t), 4),
            "host_path_s": [round(x, 4) for x in host_t], "host_path_median_s": round(statistics.median(host_t), 4),
            "files_identical": same, "file_bytes": len(out_host),
            "note": "device path = host arrays -> Sorter('concat').insert_batch -> write_file (upload included); host "
                    "path = this library's own: Python sorted + grouping + host Writer; no reference (Rust) timing exists"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, nargs="+", default=[800_000, 8_000_000], help="distinct keys per size")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--dup", type=float, default=0.1, help="fraction of the keys that occur twice")
    ap.add_argument("--whole-max", type=int, default=1_000_000, help="largest record count that runs the whole-path leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sort", "sort_bench.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "dup": a.dup, "sizes": []}
    for nkeys in a.keys:
        keys, vals = make_records(nkeys, a.dup)
        row = {"keys": nkeys, "phases": leg_phases(keys, vals, a.runs)}
        if keys.shape[0] <= a.whole_max:
            row["whole_path"] = leg_whole(keys, vals, max(a.runs // 2, 2))
        res["sizes"].append(row)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Snappy files in the Reader: the device stage against the host stage, and the on-demand table
against the full one (DESIGN.md §4 "Snappy files in the Reader").  One process, one box.

Files (the product Writer, CompressionType::Snappy, 4 KiB blocks):
  cfg5          the cfg2 records (16 B keys, 64 B random values: Snappy stores them as literals),
                --blocks data blocks
  compressible  cfg1-style records (a 10-digit key, the key repeated 1-8 times as the value, ~4.5x),
                --records records
Measured, host clock ending in a synchronize, on a fresh Reader each time (the file already on the
device), the two sides alternated, median of --runs after a warm-up:
  iter     Reader.iter() with snappy_stage="host" (the file copied to the host, decompressed by 16 CPU
           threads, uploaded) and with snappy_stage="device" (mtblx_stage_plan / _emit)
  get1000  the FIRST get_batch of 1 000 keys drawn uniformly from the file: the full table staged on
           the host (what the Reader did before), the full table staged on the device, and the
           on-demand table; with the table's arena bytes and resident blocks
The records / values of the two sides are compared before any time is reported.

Prints one JSON object (and writes it to --out).  Needs the GPU."""
import argparse
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


def cfg5_file(nblocks):
    from mtblx import synth
    from mtblx.writer import Writer
    n = synth.cfg2_file_nrec(nblocks)
    keys, vals, kl, vl = synth.cfg2_arrays(n)
    w = Writer(4096, 16, 1)
    w.insert_batch(keys[: n * kl], np.arange(1, n + 1, dtype=np.uint64) * np.uint64(kl), vals[: n * vl],
                   np.arange(1, n + 1, dtype=np.uint64) * np.uint64(vl))
    data = w.into_inner_np()
    qkeys = [keys[i * kl: (i + 1) * kl].tobytes() for i in np.random.default_rng(1).integers(0, n, 1000)]
    return data, len(w.block_dir[0]), qkeys


def compressible_file(nrec):
    from mtblx import synth
    from mtblx.writer import Writer
    w = Writer(4096, 16, 1)
    keys = []
    for k, v in synth.cfg1_records(nrec):
        w.insert(k, v)
        keys.append(k)
    data = np.frombuffer(w.into_inner(), np.uint8).copy()
    qkeys = [keys[int(i)] for i in np.random.default_rng(2).integers(0, nrec, 1000)]
    return data, len(w.block_dir[0]), qkeys


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def bench_file(name, data, nblk, qkeys, runs):
    from mtblx import _lib, reader
    dfile = torch.from_numpy(data).cuda()
    res = {"file_bytes": int(data.size), "blocks": nblk}

    def fresh(stage):
        return reader.ReaderBuilder(snappy_stage=stage).read(dfile)

    # ---- iter ----
    ms = {"host": [], "device": []}
    ref = None
    for i in range(runs + 1):
        for stage in ("host", "device"):
            r = fresh(stage)
            t, s = timed(r.iter)
            assert s.end == 0
            if i == 0:
                sig = (s.nrec, int(s.keys.sum(dtype=torch.int64).item()), int(s.vals.sum(dtype=torch.int64).item()),
                       int(s.val_end[-1].item()))
                assert ref in (None, sig), (ref, sig)
                ref = sig
                assert r.stage_stats["host_blocks"] == (nblk if stage == "host" else 0)
            else:
                ms[stage].append(t)
            del r, s
    res["iter"] = {"records": ref[0], "host_ms": statistics.median(ms["host"]),
                   "device_ms": statistics.median(ms["device"]), "host_runs_ms": ms["host"], "device_runs_ms": ms["device"]}
    res["iter"]["host_over_device"] = res["iter"]["host_ms"] / res["iter"]["device_ms"]

    # ---- the first get_batch of 1 000 keys ----
    modes = {"full_host": ("host", False), "full_device": ("device", False), "on_demand": ("device", True)}
    ms = {m: [] for m in modes}
    info, vals = {}, None
    for i in range(runs + 1):
        for m, (stage, od) in modes.items():
            r = fresh(stage)
            r.index_regular()                       # the index chain is read once per Reader either way
            if not od:
                r._od = False                       # the full table
            t, (st, vo, vl) = timed(lambda: r.get_batch(qkeys))
            assert (st == _lib.GET_FOUND).all()
            if i == 0:
                src = r.value_source
                got = [src[int(o): int(o) + int(n)].cpu().numpy().tobytes() for o, n in
                       zip(vo[:50].tolist(), vl[:50].tolist())]
                assert vals in (None, got)
                vals = got
                s = r.stage_stats
                info[m] = {"table_mode": r.table_mode, "resident_blocks": s["resident_blocks"],
                           "arena_bytes": s["arena_bytes"], "host_blocks": s["host_blocks"],
                           "device_blocks": s["device_blocks"]}
            else:
                ms[m].append(t)
            del r
    res["get1000"] = {m: dict(info[m], ms=statistics.median(ms[m]), runs_ms=ms[m]) for m in modes}
    g = res["get1000"]
    g["full_device_over_on_demand"] = g["full_device"]["ms"] / g["on_demand"]["ms"]
    g["full_host_over_on_demand"] = g["full_host"]["ms"] / g["on_demand"]["ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=20000, help="data blocks of the cfg5 file")
    ap.add_argument("--records", type=int, default=400000, help="records of the compressible file")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    out = {"device": torch.cuda.get_device_name(0), "runs": a.runs}
    out["cfg5"] = bench_file("cfg5", *cfg5_file(a.blocks), a.runs)
    out["compressible"] = bench_file("compressible", *compressible_file(a.records), a.runs)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

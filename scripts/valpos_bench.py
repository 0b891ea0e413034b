"""Positions mode against the plain decode on cfg2 (DESIGN.md "Positions instead of values").

Leg (a), device-resident: codec.decode_into and codec.decode_positions_into alternate in one
process on one workspace, `--alternations` times `--launches` launches each after a warm-up, every
run timed with HIP events; decode_into is also timed against itself (A/A), whose spread is the
yardstick -- the positions launch does strictly less work, so it must not be slower than the
plain one by more than that spread.
Leg (b), end to end: HostPipe.decode and HostPipe.decode_positions alternate on one pipe with
bench.py's pipe settings over the pinned file, read beside bench.py's pcie_ceiling() taken in the
same run; the PCIe floor is computed as bench.py's end_to_end does.

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

CPU_SCAN_GIBS = 72.3   # BENCH_r06.json: the 16-thread CPU scan of the same file


def leg_device(data, off, ln, alternations, launches):
    from mtblx import codec
    batch = codec.DeviceBatch.from_host(data, off, ln)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ws = codec.Workspace(batch.nblk)
        plain = codec.decode_blocks(batch, stream=s)
    torch.cuda.synchronize()
    nr, kb, vb, flags = plain.totals_host()
    assert flags == 0
    with torch.cuda.stream(s):
        pos = codec.DecodedBlocks(batch.nblk, nr, kb, 0, values=False)
        val_pos = torch.zeros(max(nr, 1), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            e0.record(s)
            for _ in range(launches):
                fn()
            e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / launches

    run_plain = lambda: codec.decode_into(batch, plain, ws, s)   # noqa: E731
    run_pos = lambda: codec.decode_positions_into(batch, pos, val_pos, ws, s)   # noqa: E731
    for fn in (run_plain, run_pos):
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.3:
            timed(fn)
    t_plain, t_plain2, t_pos = [], [], []
    for _ in range(alternations):
        t_plain.append(timed(run_plain))
        t_pos.append(timed(run_pos))
        t_plain2.append(timed(run_plain))   # A/A: the plain launch against itself
    if pos.totals_host() != (nr, kb, vb, 0) or not bool((pos.status[: batch.nblk] == 0).all()):
        raise RuntimeError(f"positions decode failed: totals={pos.totals_host(False)}")
    if not (torch.equal(pos.key_end[:nr], plain.key_end[:nr]) and torch.equal(pos.val_end[:nr], plain.val_end[:nr]) and
            torch.equal(pos.keys[:kb], plain.keys[:kb])):
        raise RuntimeError("positions decode: keys / ends differ from the plain decode")
    allp = t_plain + t_plain2
    spread = max(allp) - min(allp)
    mp, mq = statistics.median(allp), statistics.median(t_pos)
    in_bytes = int(ln.sum(dtype=np.uint64))
    base = in_bytes + 12 * batch.nblk + 32 * batch.nblk + kb + 8 * nr   # read once + written once
    return {
        "blocks": batch.nblk, "records": nr, "key_bytes": kb, "value_bytes": vb, "block_bytes": in_bytes,
        "launches_per_run": launches, "alternations": alternations,
        "plain_ms": [round(x, 4) for x in t_plain], "plain_again_ms": [round(x, 4) for x in t_plain2],
        "positions_ms": [round(x, 4) for x in t_pos],
        "plain_median_ms": round(mp, 4), "positions_median_ms": round(mq, 4),
        "aa_spread_ms": round(spread, 4),
        "positions_not_slower_than_plain_plus_spread": bool(mq <= mp + spread),
        "algorithmic_MB_plain": round((base + vb) / 1e6, 1), "algorithmic_MB_positions": round((base + 4 * nr) / 1e6, 1),
        "plain_GiB_per_s": round(in_bytes / (mp * 1e-3) / 2**30, 1),
        "positions_GiB_per_s": round(in_bytes / (mq * 1e-3) / 2**30, 1),
    }


def leg_end_to_end(data, off, ln, nr, kb, vb, rounds, reps):
    import bench
    from mtblx import pipe
    pc = bench.pcie_ceiling()
    block_bytes = int(ln.sum(dtype=np.uint64))
    p = pipe.HostPipe(chunk_bytes=64 << 20, max_blocks=1 << 16, threads=16, device_snappy=False)   # bench.py's settings
    outs = {"plain": pipe.HostOutputs(off.size, nr, kb, vb), "positions": pipe.HostOutputs(off.size, nr, kb, 0, positions=True)}
    call = {"plain": lambda o: p.decode(data, off, ln, o), "positions": lambda o: p.decode_positions(data, off, ln, o)}
    acc = {m: {"el": 0.0, "h2d": 0, "d2h": 0, "dec": 0.0, "n": 0, "per_round_GiBs": []} for m in outs}
    pipe.register(data)
    try:
        for _ in range(2):   # warm-up: first touch of the pinned pages, the slots laid out for either mode
            for m in outs:
                for _ in range(reps):
                    call[m](outs[m])
        for _ in range(rounds):
            for m in outs:
                t0 = time.perf_counter()
                for _ in range(reps):
                    st = call[m](outs[m])
                    acc[m]["h2d"] += st.h2d_bytes
                    acc[m]["d2h"] += st.d2h_bytes
                    acc[m]["dec"] += st.decode_ms
                el = time.perf_counter() - t0
                acc[m]["el"] += el
                acc[m]["n"] += reps
                acc[m]["per_round_GiBs"].append(round(block_bytes * reps / el / 2**30, 2))
                tot = outs[m].totals
                if [int(x) for x in tot[:4]] != [nr, kb, vb, 0] or not (outs[m].status[: off.size] == 0).all():
                    raise RuntimeError(f"end-to-end decode ({m}) failed: totals={list(tot)}")
    finally:
        pipe.unregister(data)
    res = {"pcie_ceiling": pc, "cpu_scan_GiB_per_s": CPU_SCAN_GIBS, "rounds": rounds, "passes_per_round": reps}
    for m, a in acc.items():
        n, el = a["n"], a["el"]
        bound = max(a["h2d"] / n / (pc["h2d_GBs"] * 1e9), a["d2h"] / n / (pc["d2h_GBs"] * 1e9))
        res[m] = {"GiB_per_s": round(block_bytes * n / el / 2**30, 2), "per_round_GiB_per_s": a["per_round_GiBs"],
                  "median_round_GiB_per_s": statistics.median(a["per_round_GiBs"]),
                  "ms_per_pass": round(el * 1e3 / n, 3),
                  "h2d_GB_per_pass": round(a["h2d"] / n / 1e9, 4), "d2h_GB_per_pass": round(a["d2h"] / n / 1e9, 4),
                  "decode_ms_per_pass": round(a["dec"] / n, 3),
                  "pcie_floor_ms_per_pass": round(bound * 1e3, 3), "frac_of_pcie_floor": round(bound / (el / n), 3)}
        res[m]["faster_than_cpu_scan"] = bool(res[m]["GiB_per_s"] > CPU_SCAN_GIBS)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=100_000)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("valpos_bench needs the GPU")
    from mtblx import synth
    data, off, ln = synth.cfg2_file(a.blocks)
    res = {"device": torch.cuda.get_device_name(0), "config": "cfg2", "device_resident": leg_device(data, off, ln, a.alternations, a.launches)}
    d = res["device_resident"]
    res["end_to_end"] = leg_end_to_end(data, off, ln, d["records"], d["key_bytes"], d["value_bytes"], a.rounds, a.passes)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()

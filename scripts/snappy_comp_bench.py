"""The device Snappy writer, measured (DESIGN.md §4 "The Snappy writer").

Leg (a), kernels, HIP events, median of --runs after a warm-up, GB/s of INPUT (uncompressed block
bytes), on three batches of raw 4 KiB blocks resident on the device:
  compressible   the stream bench.py's compressible_snappy decompresses: cfg1-style records (a
                 10-digit key, the key repeated 1-8 times as the value), the file's blocks 4x over
  cfg2           cfg2 blocks (random keys' tails and values: incompressible)
  cfg1           synth.cfg1_records(10000): 125 blocks, a launch-bound batch
per batch: mtblx_snappy_compress_dev alone; mtblx_snappy_slots + mtblx_frame_blocks (layout, CRC
of the stored bytes, headers, payload copy); mtblx_stream_copy of the same number of input bytes
in this process, for scale; the compressed size against the host compressor's on a sample of
blocks.
Leg (b), whole path, wall time: 8 cfg2-shaped sources in host memory -> Reader -> Merger("concat")
-> write_file(compression=Snappy), against the path a user had before the device compressor:
the same Merger's write_into a host Writer(Snappy).  The comparator is this library's own host
path, NOT the reference crate (Rust cannot be built here, so no reference timing exists).  The
two files must decode to identical records.

Prints one JSON object (and writes it to --out).  Needs the GPU."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "oxidized-mtbl_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def raw_blocks(kind, tile):
    """-> (file bytes u8, blk_off, blk_len) of uncompressed 4 KiB blocks, the file `tile` times over"""
    from mtblx import synth
    from mtblx.writer import Writer
    if kind == "cfg2":
        data, off, ln = synth.cfg2_file(100_000)
    else:
        w = Writer(4096, 16, 0)
        for k, v in synth.cfg1_records(2_000_000 if kind == "compressible" else 10_000):
            w.insert(k, v)
        data = np.frombuffer(w.into_inner(), np.uint8).copy()
        off, ln = w.block_dir
    if tile > 1:
        off = np.concatenate([off.astype(np.uint64) + np.uint64(i * data.size) for i in range(tile)])
        ln = np.tile(ln, tile)
        data = np.tile(data, tile)
    return data, off, ln


def timed(fn, runs, stream):
    """median HIP-event ms of fn() over `runs` after one warm-up (plus ~40 ms of launches: the GPU
    drops its clocks when idle)"""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.04:
        fn()
        torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), ts


def leg_kernels(kind, tile, runs):
    from merge_bench import copy_ms
    from mtblx import codec, pipe
    L = codec._require_device()
    data, off, ln = raw_blocks(kind, tile)
    batch = codec.DeviceBatch.from_host(data, off, ln)
    nblk = batch.nblk
    raw = int(ln.astype(np.uint64).sum())
    s = torch.cuda.current_stream()
    sh = C.c_void_p(int(s.cuda_stream))
    slots = codec.SnappySlots(nblk)
    codec.snappy_slots(batch, slots, s)
    torch.cuda.synchronize()
    total = int(slots.totals[0].item())
    dst = torch.empty(total, dtype=torch.uint8, device="cuda")
    dst_len = torch.zeros(nblk, dtype=torch.int32, device="cuda")
    status = torch.zeros(nblk, dtype=torch.int32, device="cuda")
    comp_ms, comp_all = timed(lambda: codec.snappy_compress_into(batch, slots, dst, dst_len, status, s), runs, s)
    assert int((status != 0).sum().item()) == 0
    stored = int(dst_len.to(torch.int64).sum().item())
    out = torch.empty(stored + 14 * nblk, dtype=torch.uint8, device="cuda")
    blk_off = torch.empty(nblk, dtype=torch.int64, device="cuda")
    ftot = torch.zeros(2, dtype=torch.int64, device="cuda")
    u = codec._u

    def frame():
        codec.snappy_slots(batch, slots, s)
        rc = L.mtblx_frame_blocks(C.c_void_p(u(dst)), C.c_void_p(u(slots.dst_off)), C.c_void_p(u(dst_len)), nblk,
                                  C.c_void_p(u(out)), int(out.numel()), C.c_void_p(u(blk_off)), C.c_void_p(u(ftot)),
                                  C.c_void_p(u(slots.ws)), slots.ws_bytes, sh)
        assert rc == 0, rc
    frame_ms, frame_all = timed(frame, runs, s)
    framed, fflags = (int(x) for x in ftot.tolist())
    assert fflags == 0
    # compressed size against the host compressor on a sample of the blocks
    step = max(nblk // 500, 1)
    dl = dst_len.cpu().numpy().view(np.uint32)
    host = dev = smp = 0
    for b in range(0, nblk, step):
        x = data[int(off[b]): int(off[b]) + int(ln[b])].tobytes()
        host += len(pipe.snappy_compress(x))
        dev += int(dl[b])
        smp += len(x)
    cp = copy_ms(2 * raw)   # `raw` bytes read and `raw` bytes written
    return {"batch": kind, "blocks": nblk, "input_bytes": raw, "stored_bytes": stored, "framed_bytes": framed,
            "stored_over_input": round(stored / raw, 4), "runs": runs,
            "compress_ms": round(comp_ms, 4), "compress_ms_all": [round(t, 4) for t in comp_all],
            "compress_GBps_in": round(raw / comp_ms / 1e6, 2),
            "slots_frame_ms": round(frame_ms, 4), "slots_frame_ms_all": [round(t, 4) for t in frame_all],
            "slots_frame_GBps_in": round(raw / frame_ms / 1e6, 2),
            "stream_copy_ms_same_input": round(cp, 4), "stream_copy_GBps": round(raw / cp / 1e6, 1),
            "sample": {"blocks": len(range(0, nblk, step)), "input_bytes": smp, "host_bytes": host, "device_bytes": dev,
                       "host_over_input": round(host / smp, 4), "device_over_input": round(dev / smp, 4),
                       "device_over_host": round(dev / host, 4)}}


def leg_whole(keys, runs):
    from merge_bench import make_sources, write_files
    from mtblx import CompressionType, merger, reader, writer
    files = write_files(make_sources(keys)[0])
    dev_t, host_t = [], []
    out_dev = out_host = None
    for i in range(runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rd = [reader.Reader(f) for f in files]
        f = merger.Merger.builder("concat").extend(rd).build().write_file(4096, 16, compression=CompressionType.Snappy)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if i:
            dev_t.append(t1 - t0)
        out_dev = f.cpu().numpy().tobytes()
    for i in range(max(runs // 2, 2)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rd = [reader.Reader(f) for f in files]
        w = writer.Writer(4096, 16, CompressionType.Snappy)
        merger.Merger.builder("concat").extend(rd).build().write_into(w)
        out_host = w.into_inner()
        t1 = time.perf_counter()
        host_t.append(t1 - t0)
    a = reader.Reader(np.frombuffer(out_dev, np.uint8)).iter().records()
    b = reader.Reader(np.frombuffer(out_host, np.uint8)).iter().records()
    return {"keys": keys, "records_out": len(a), "records_identical": a == b,
            "device_path_s": [round(x, 4) for x in dev_t], "device_path_median_s": round(statistics.median(dev_t), 4),
            "host_path_s": [round(x, 4) for x in host_t], "host_path_median_s": round(statistics.median(host_t), 4),
            "device_file_bytes": len(out_dev), "host_file_bytes": len(out_host),
            "note": "host path = this library's Merger.write_into a host Writer(Snappy) (single-threaded host "
                    "compressor); no reference (Rust) timing exists"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--keys", type=int, default=800_000, help="distinct keys dealt to the 8 sources of leg (b)")
    ap.add_argument("--no-whole", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snappy_comp", "snappy_comp_bench.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "kernels": []}
    for kind, tile in (("compressible", 4), ("cfg2", 1), ("cfg1", 1)):
        res["kernels"].append(leg_kernels(kind, tile, a.runs))
        print(json.dumps(res["kernels"][-1]), flush=True)
    if not a.no_whole:
        res["whole_path"] = leg_whole(a.keys, a.runs)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

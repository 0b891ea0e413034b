"""bench.py's command line: a plain run prints the headline line only (the other legs sit behind
--full), --steps sets the timed steps, and --dump-outputs writes what the last timed step decoded
-- checked here against the oracle's decode of the same seeded batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("cpu_baseline", "crc32c_verify", "get_batch", "end_to_end")


def _bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_full_and_dump_options_default_off():
    bench = _bench()
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_samples_are_fixed_and_bounded(tmp_path):
    """arrays above their cap are written as the same seeded sample every time, integers exactly,
    and a dump stays below 64 MB"""
    from mtblx import codec
    bench = _bench()
    nblk, nr = 500_001, 1_000_001           # one past the per-block and per-record caps
    kb, vb = 16 * nr, 3 * nr                # keys and values past theirs
    o = codec.DecodedBlocks(nblk, nr, kb, vb, device="cpu")
    o.totals[:] = torch.tensor([nr, kb, vb, 0])
    o.rec_base[:] = torch.arange(nblk) * 2
    o.key_base[:] = torch.arange(nblk) + (1 << 40)
    o.key_end[:] = -2                       # u32 0xFFFFFFFE in torch's int32
    o.keys[:] = torch.arange(kb) % 251
    dirs = [tmp_path / "a", tmp_path / "b"]
    for d in dirs:
        bench.dump_outputs(str(d), o)
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(n + ".npy" for n in ("totals", "status", "nrec", "rec_base", "key_base", "val_base",
                                                "key_end", "val_end", "keys", "vals"))
    assert sum(os.path.getsize(dirs[0] / n) for n in names) <= 64_000_000
    got = {n[:-4]: np.load(dirs[0] / n) for n in names}
    for n in names:
        assert got[n[:-4]].dtype in (np.float32, np.float64)
        assert np.array_equal(got[n[:-4]], np.load(dirs[1] / n)), n
    assert list(got["totals"]) == [nr, kb, vb, 0]
    assert got["rec_base"].size == 500_000 and got["key_end"].size == 1_000_000 and got["keys"].size == 2_500_000
    assert np.all(got["rec_base"] % 2 == 0) and np.all(np.diff(got["rec_base"]) >= 0)     # a sorted sample of 2 * i
    kbi = got["key_base"] - float(1 << 40)                                                # exact above 2^32
    assert np.all(kbi == np.floor(kbi)) and kbi.min() >= 0 and kbi.max() < nblk and np.all(np.diff(kbi) >= 0)
    assert not np.array_equal(kbi, got["rec_base"] / 2)                                   # each name has its own sample
    assert np.all(got["key_end"] == 4294967294.0)
    assert set(np.unique(got["keys"])) <= set(range(251)) and got["keys"].max() == 250


@pytest.mark.gpu
def test_plain_run_dumps_the_decoded_batch(tmp_path, oracle):
    from mtblx import synth
    nblk = 500
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--blocks", str(nblk), "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "GiB/s" and d["dtype"] == "u8" and d["higher_is_better"] is True
    assert not [k for k in FULL_ONLY if k in d] and d["roofline"]["stream_copy_ceiling_GBs"] is None
    # all of this batch's arrays are below their caps: the dump is the whole decode
    data, off, ln = synth.cfg2_shard(0, 1, nblk)
    orc = oracle.decode_blocks(data, off, ln)
    got = {n: np.load(tmp_path / "out" / (n + ".npy")) for n in
           ("totals", "status", "nrec", "rec_base", "key_base", "val_base", "key_end", "val_end", "keys", "vals")}
    assert list(got["totals"]) == [int(orc.nrec.sum()), orc.keys.size, orc.vals.size, 0]
    for n in ("status", "nrec", "rec_base", "key_base", "val_base", "key_end", "val_end", "keys", "vals"):
        assert np.array_equal(got[n], getattr(orc, n).astype(got[n].dtype)), n

"""mtbl::Reader::reduce_batch of the C++ surface (include/mtbl.hpp) on the GPU:
tests/cpp/test_scan_reduce.cpp reads a file and a list of queries with the answers this side wrote
from the model -- Reduce.fold over the oracle's records -- for one uncompressed file (the kernel's
walk, one query wide enough to be handed back) and one Snappy file (the host fold)."""
import os
import subprocess

import numpy as np
import pytest

import corpus
import scan_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "oxidized-mtbl_amd", "build", "test_scan_reduce")
KIND = {"from": 0, "get": 1, "prefix": 2, "range": 3}


def test_cpp_scan_reduce_is_built():
    """no GPU needed: the `cpp` target of the Makefile builds the binary against libmtblx.so"""
    assert os.path.exists(EXE), "build/test_scan_reduce not built (make -C oxidized-mtbl_amd cpp)"
    out = subprocess.run(["nm", "-D", "--undefined-only", EXE], capture_output=True, text=True).stdout
    assert "mtblx_scan_reduce" in out and "mtblx_scan_workspace_bytes" in out


def _hex(b):
    return b.hex() or "-"


@pytest.mark.gpu
@pytest.mark.parametrize("comp", [0, 1], ids=["plain", "snappy"])
def test_cpp_scan_reduce(oracle, tmp_path, comp):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mtblx import Reduce
    assert os.path.exists(EXE), "build/test_scan_reduce not built (make -C oxidized-mtbl_amd cpp)"
    rng = np.random.default_rng(21 + comp)
    red = Reduce("sum", "min", "max")
    keys = [k for k, _ in corpus.random_records(rng, 3000, 1, 24, 0, 0)]
    vals = []
    for i in range(len(keys)):
        w = rng.integers(0, 1 << 63, 3, dtype=np.uint64)
        w[0] |= np.uint64(1 << 63) if i % 3 == 0 else np.uint64(0)
        vals.append(w.astype("<u8").tobytes() if i % 29 else b"x" * (23 + i % 3))     # some of 23 and 25 bytes
    recs = list(zip(keys, vals))
    data = su.write(recs, 1024, 4, comp)
    qs, lim = su.queries_for(su.probe_keys(rng, recs, n=12))
    qs.append(("prefix", b""))                 # the whole file: far more than max_blocks data blocks
    lim.append(None)
    lines = ["ops 0 1 2", "max_blocks 8"]
    for q, m in zip(qs, lim):
        e = su.expected(oracle, data, q, m, True)
        assert e["end"] == 0
        fields, nrec, nbad = red.fold([v for _, v in e["records"]])
        served = -1 if comp == 0 else 0       # a compressed file is folded on the host
        lines.append(" ".join([str(KIND[q[0]]), _hex(q[1]), _hex(q[2]) if q[0] == "range" else "-",
                               str(-1 if m is None else m)] + [str(x) for x in fields] + [str(nrec), str(nbad),
                                                                                           str(served)]))
    if comp == 0:
        lines[-1] = lines[-1][: lines[-1].rindex(" ")] + " 0"      # LARGE: handed back
    (tmp_path / "file.mtbl").write_bytes(data)
    (tmp_path / "case.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([EXE, str(tmp_path / "file.mtbl"), str(tmp_path / "case.txt")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("OK ")
    kernel = int(r.stdout.split()[3])
    assert (kernel > len(qs) // 2) if comp == 0 else kernel == 0

"""mtbl::Reader of the C++ surface (include/mtbl.hpp) over Snappy files on the GPU:
tests/cpp/test_snappy_reader.cpp iterates a file and dumps its records, how the iteration ended and
the Reader's count of host-decompressed blocks.  The dump equals the oracle's scan (oracle_file_scan),
the blocks are staged on the device (zero host-decompressed blocks), and a corrupt stored block ends
the iteration as the reference does: the checksum panic with verification on, Err(Io) with it off."""
import os
import subprocess

import numpy as np
import pytest

import corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "oxidized-mtbl_amd", "build", "test_snappy_reader")


def test_cpp_snappy_reader_is_built():
    """no GPU needed: the `cpp` target of the Makefile builds the binary against libmtblx.so"""
    assert os.path.exists(EXE), "build/test_snappy_reader not built (make -C oxidized-mtbl_amd cpp)"
    out = subprocess.run(["nm", "-D", "--undefined-only", EXE], capture_output=True, text=True).stdout
    assert "mtblx_stage_plan" in out and "mtblx_stage_emit" in out and "mtblx_stage_workspace_bytes" in out


def _dump(path, verify):
    r = subprocess.run([EXE, path] + ([] if verify else ["noverify"]), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[-2].startswith("END ") and lines[-1].startswith("HOSTDEC ")
    recs = [tuple(bytes.fromhex(h) for h in (ln.split(" ") + [""])[:2]) for ln in lines[:-2]]
    return recs, lines[-2][4:], int(lines[-1].split()[1])


@pytest.mark.gpu
def test_cpp_snappy_reader(oracle, tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert os.path.exists(EXE), "build/test_snappy_reader not built (make -C oxidized-mtbl_amd cpp)"
    from mtblx.writer import Writer
    rng = np.random.default_rng(77)
    recs = corpus.random_records(rng, 1500, 1, 40, 0, 120)
    w = Writer(1024, 8, 1)
    for k, v in recs:
        w.insert(k, v)
    data = w.into_inner()
    off, ln = w.block_dir
    assert len(off) > 64
    ends = {0: "none", 3: "panic"}                       # the oracle's END_* codes
    b = len(off) // 2
    bad = bytearray(data)
    bad[int(off[b]) + int(ln[b]) // 2] ^= 0x5A           # a stored byte of block b
    o = int(off[b])
    assert data[o] & 0x80 and not data[o + 1] & 0x80      # a two-byte preamble
    raised = bytearray(data)
    raised[o + 1] += 1                                   # it claims 128 bytes more than the stream holds
    for name, d, verify in (("valid", data, True), ("flip-verify", bytes(bad), True), ("flip-noverify", bytes(bad), False),
                            ("raised-noverify", bytes(raised), False)):
        p = tmp_path / (name + ".mtbl")
        p.write_bytes(d)
        exp = oracle.file_scan(d, "iter", verify=verify)
        got, end, hostdec = _dump(str(p), verify)
        want_end = ends[exp["end"]] if exp["end"] in ends else "err " + str(exp["err"])
        assert end == want_end, (name, end, want_end)
        assert got == exp["records"], (name, len(got), len(exp["records"]))
        assert hostdec == 0, (name, hostdec)
        if name == "valid":
            assert got == recs
        elif verify:
            assert end == "panic" and 0 < len(got) < len(recs)
        elif name == "raised-noverify":
            assert end == "err Io" and 0 < len(got) < len(recs)

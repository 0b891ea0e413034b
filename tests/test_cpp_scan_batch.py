"""mtbl::Reader::scan_batch of the C++ surface (include/mtbl.hpp) on the GPU:
tests/cpp/test_scan_batch.cpp runs a batch of from / get / prefix / range queries and compares every
query with the same one through iter_from / iter_prefix / iter_range / get, with the default block
limit and with one small enough to hand the wide scans back."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "oxidized-mtbl_amd", "build", "test_scan_batch")


def test_cpp_scan_batch_is_built():
    """no GPU needed: the `cpp` target of the Makefile builds the binary against libmtblx.so"""
    assert os.path.exists(EXE), "build/test_scan_batch not built (make -C oxidized-mtbl_amd cpp)"
    out = subprocess.run(["nm", "-D", "--undefined-only", EXE], capture_output=True, text=True).stdout
    assert "mtblx_scan_plan" in out and "mtblx_scan_emit" in out and "mtblx_scan_workspace_bytes" in out


@pytest.mark.gpu
def test_cpp_scan_batch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert os.path.exists(EXE), "build/test_scan_batch not built (make -C oxidized-mtbl_amd cpp)"
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("OK ")

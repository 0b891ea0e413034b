"""mtbl::SorterBuilder / mtbl::Sorter of the C++ surface (include/mtbl.hpp) on the GPU:
tests/cpp/test_sorter.cpp repeats the reference's `simple` test (src/sorter.rs:264-295), the
stability case (3000 records over 30 keys: every group's values in insertion order) and the chunk
rule with 1024-byte entries."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "oxidized-mtbl_amd", "build", "test_sorter")


def test_cpp_sorter_is_built():
    """no GPU needed: the `cpp` target of the Makefile builds the binary against libmtblx.so"""
    assert os.path.exists(EXE), "build/test_sorter not built (make -C oxidized-mtbl_amd cpp)"
    out = subprocess.run(["nm", "-D", "--undefined-only", EXE], capture_output=True, text=True).stdout
    assert "mtblx_sort_plan" in out and "mtblx_sort_emit" in out
    assert "mtblx_merge_plan" in out and "mtblx_merge_emit" in out   # the chunks go through the Merger


@pytest.mark.gpu
def test_cpp_sorter():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert os.path.exists(EXE), "build/test_sorter not built (make -C oxidized-mtbl_amd cpp)"
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("OK ")

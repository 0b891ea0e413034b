"""detail::decode_batch_positions of the C++ surface (include/mtbl.hpp) on the GPU:
tests/cpp/test_valpos.cpp decodes a cfg1 file written by the C++ Writer both ways and reads every
value through its position.  (Its build is checked without a GPU in tests/test_valpos.py.)"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "oxidized-mtbl_amd", "build", "test_valpos")


@pytest.mark.gpu
def test_cpp_decode_batch_positions():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert os.path.exists(EXE), "build/test_valpos not built (make -C oxidized-mtbl_amd cpp)"
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("OK ")

"""Positions mode (mtblx_decode_blocks_valpos / mtblx_pipe_decode_valpos) without a GPU: the
yardstick of the GPU tests, the two symbols, the argument check, the C++ test's build.

The oracle yields records, not positions; valpos_util.walk_block restates decode_entry
(src/block.rs:216-238) from pyoracle.varint_decode32.  The first test pins that walker against
the oracle itself -- for every record it yielded, on every status, block[pos:pos+len] is the
oracle's value -- so exact equality of val_pos with the walker is a fair demand on the device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import corpus
import valpos_util as vu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "oxidized-mtbl_amd")


def test_walker_matches_oracle(oracle):
    """820+ blocks (builder, mutated, golden quirks, four of 81-235 KB): OK / INVALID / CORRUPT /
    LOOP all present; every yielded record's value sits at the walker's position"""
    data, off, ln, exp, pos = vu.mixed_corpus(oracle, large=True)
    assert off.size >= 820 and pos.size > 20000
    assert {0, 1, 2, 3} <= set(exp.status.tolist())
    assert int(exp.nrec[exp.status == 2].sum()) > 0   # CORRUPT blocks that yield records first
    vu.check_positions(data, off, ln, exp, pos)


def test_walker_unterminated_varint_quirk(oracle):
    """a consumed length of 0 (varint_decode32 on an unterminated varint) is legal in the walk"""
    names = set()
    for name, b, _ in corpus.quirk_blocks():
        st, recs = oracle.decode_block(b)
        got = vu.walk_block(oracle, b, len(recs))
        assert [b[p:p + n] for p, n in got] == [v for _, v in recs], name
        if recs:
            names.add(name)
    assert {"unterminated_loop", "noncanonical_varints", "second_entry_corrupt"} <= names
    assert oracle.varint_decode32(b"\x80\x80")[1] == 0


def test_symbols_exported_and_bound(mtblx_lib):
    import mtblx
    out = subprocess.run(["nm", "-D", "--defined-only", mtblx.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln_.split()[-1] for ln_ in out.splitlines() if " T " in ln_}
    for name in ("mtblx_decode_blocks_valpos", "mtblx_pipe_decode_valpos"):
        assert name in exported and name in mtblx.EXPORTS
        assert getattr(mtblx_lib, name).restype is C.c_int
    assert mtblx_lib.mtblx_abi_version() == 3   # two added symbols, no version bump


def test_null_val_pos_is_invalid(mtblx_lib):
    """val_pos == NULL with rec_cap != 0 -> MTBLX_E_INVAL, before any HIP call (every other
    argument here is a plausible non-NULL address that a launch would fault on)"""
    from mtblx._lib import BlockBatch, Decoded
    buf = (C.c_uint8 * 4096)()
    a = C.addressof(buf)
    b = BlockBatch(a, 64, a + 64, a + 128, 1, 64)
    o = Decoded(a + 256, a + 320, a + 384, a + 448, a + 512, a + 576, a + 640, 1, a + 704, 16, 0, 0, a + 768)
    rc = mtblx_lib.mtblx_decode_blocks_valpos(C.byref(b), C.byref(o), None, C.c_void_p(a + 1024), 1 << 20, None)
    assert rc == -1
    # the pipe's twin checks it before it looks at the pipe
    rc = mtblx_lib.mtblx_pipe_decode_valpos(None, None, 0, None, None, 0, C.byref(o), None, None)
    assert rc == -1


def test_cpp_valpos_builds():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    subprocess.run(["make", "-s", "-C", PKG, "cpp"], check=True)
    exe = os.path.join(PKG, "build", "test_valpos")
    assert os.path.exists(exe)
    out = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libmtblx.so" in out and "not found" not in out.split("libmtblx.so")[1].splitlines()[0], out


def test_python_mirrors_present():
    from mtblx import codec, pipe
    assert callable(codec.decode_positions_into) and callable(codec.decode_positions)
    assert callable(pipe.HostPipe.decode_positions) and callable(pipe.HostOutputs.records_from)
    out = pipe.HostOutputs(3, 10, 100, 12345, pinned=False, positions=True)
    assert out.vals is None and out.c.vals is None and out.c.vals_cap == 0
    assert out.val_pos.dtype == np.uint32 and out.val_pos.size == 10

"""Snappy files in the Reader, the parts that need no GPU: the prefix bound the host glue hands to
mtblx_scan_touch, and the new C ABI calls declared in include/mtblx.h, exported by libmtblx.so
and bound in mtblx._lib."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mtblx_stage_workspace_bytes", "mtblx_stage_plan", "mtblx_stage_emit", "mtblx_scan_touch",
       "mtblx_bitmap_compact", "mtblx_table_gather", "mtblx_dir_ascends"]


@pytest.mark.parametrize("prefix,bound", [(b"", None), (b"a", b"b"), (b"a\xff", b"b"), (b"\xff\xff", None),
                                          (b"ab\xff\xff", b"ac"), (b"\x00", b"\x01"), (b"a\xfe", b"a\xff")])
def test_prefix_bound(prefix, bound):
    from mtblx.reader import prefix_bound
    assert prefix_bound(prefix) == bound
    if bound is not None:   # above every key with the prefix, and no key between them lacks it
        assert bound > prefix + b"\xff" * 8 and not bound.startswith(prefix)


def test_new_symbols_declared_exported_and_bound(mtblx_lib):
    import mtblx
    header = open(os.path.join(ROOT, "include", "mtblx.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", mtblx.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in NEW:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in mtblx.EXPORTS and name in exported, name
        fn = getattr(mtblx_lib, name)
        assert fn.argtypes, name          # bound with a signature, not ctypes' int-everything default
        decl = re.search(r"\b" + name + r"\((.*?)\);", header, re.S).group(1)
        assert len(fn.argtypes) == decl.count(",") + 1, (name, len(fn.argtypes), decl)


def test_builder_keyword():
    from mtblx.reader import ReaderBuilder
    assert ReaderBuilder()._snappy_stage == "device"
    assert ReaderBuilder(snappy_stage="host")._snappy_stage == "host"
    assert ReaderBuilder().snappy_stage("host").verify_checksums(False)._snappy_stage == "host"
    with pytest.raises(ValueError):
        ReaderBuilder(snappy_stage="cpu")

"""The device Snappy writer's host-visible surface (no GPU): the C ABI exports the compressor,
the framing and the compression-aware index call, and encode.write_file takes `compression` and
refuses what the device cannot write before it looks for a device."""
import inspect
import subprocess

import pytest

NEW = ["mtblx_snappy_compress_dev", "mtblx_snappy_slots", "mtblx_snappy_compress_workspace_bytes",
       "mtblx_frame_blocks", "mtblx_encode_index_c"]


def test_library_exports_snappy_writer(mtblx_lib):
    import mtblx
    out = subprocess.run(["nm", "-D", "--defined-only", mtblx.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert set(NEW) <= exported
    assert set(NEW) <= set(mtblx.EXPORTS)
    for n in NEW:
        assert getattr(mtblx_lib, n).argtypes is not None, n
    assert mtblx_lib.mtblx_abi_version() == 3   # the ABI is only added to
    a = mtblx_lib.mtblx_snappy_compress_workspace_bytes(1000)
    assert 0 < a <= mtblx_lib.mtblx_snappy_compress_workspace_bytes(100000)


def test_write_file_compression_keyword():
    from mtblx import CompressionType, encode, merger, sorter
    for fn in (encode.write_file, merger.Merger.write_file, sorter.Sorter.write_file):
        p = inspect.signature(fn).parameters["compression"]
        assert p.default == CompressionType.None_


@pytest.mark.parametrize("name", ["Zlib", "Lz4", "Lz4hc", "Zstd"])
def test_write_file_rejects_host_only_codecs_without_a_device(name):
    """the check runs before the device is looked for, and points at the host path"""
    from mtblx import CompressionType, encode
    with pytest.raises(ValueError, match=r"write_into\(Writer\("):
        encode.write_file(None, compression=getattr(CompressionType, name))
    with pytest.raises(ValueError):
        encode.write_file(None, 4096, 16, None, 17)

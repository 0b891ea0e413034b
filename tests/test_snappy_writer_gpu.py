"""The device Writer with CompressionType::Snappy, file level: encode.write_file(compression=Snappy)
= plan + encode_blocks (unframed) + mtblx_snappy_compress_dev + mtblx_frame_blocks +
mtblx_encode_index_c.  The compressed bytes are this library's own, so the file is checked by
what a reader must see: the restated reference Reader (oracle.file_scan, verify=True: CRC of the
stored bytes, decompress, decode) and the device Reader yield exactly the records, the footer and
the index follow from the stored blocks, and every block decompresses to the block of the
CompressionType::None file, which the existing tests pin to the oracle Writer byte for byte."""
import numpy as np
import pytest

import corpus
import merger_model as mm

pytestmark = pytest.mark.gpu


def _mods():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mtblx
    from mtblx import encode, merger, reader, sorter
    return torch, mtblx, encode, merger, reader, sorter


def _big_value_records():
    """one 70 000-byte compressible value: a block of two 64 KiB fragments"""
    rng = np.random.default_rng(70)
    words = [b"lorem", b"ipsum", b"dolor", b"sit", b"amet", b"consectetur"]
    big = b" ".join(rng.choice(words, 14000).tolist())[:70000]
    assert len(big) == 70000
    recs = [(b"k%04d" % i, b"v%d" % i * 5) for i in range(40)]
    recs.insert(20, (b"k0019x", big))
    return recs


def _cases():
    from mtblx import synth
    rng = np.random.default_rng(5)
    rr = corpus.random_records(rng, 3000, 0, 60, 0, 300)
    return {
        "random-1024-16": (rr, 1024, 16),
        "random-4096-3": (rr, 4096, 3),
        "random-65536-16": (rr, 65536, 16),
        "cfg1-4096-16": (list(synth.cfg1_records(10000)), 4096, 16),
        "bigvalue-8192-16": (_big_value_records(), 8192, 16),
    }


def _frames(o, data):
    """[(frame offset, stored content)] of every data block, from the index"""
    out = []
    for _, val in o.index_records(data):
        off, _ = o.varint_decode64(val)
        n, ll = o.varint_decode64(data[off: off + 10])
        out.append((off, ll + 4 + n, data[off + ll + 4: off + ll + 4 + n]))
    return out


def _meta(data):
    return [int.from_bytes(data[len(data) - 512 + 8 * i: len(data) - 504 + 8 * i], "little") for i in range(9)]


@pytest.mark.parametrize("case", ["random-1024-16", "random-4096-3", "random-65536-16", "cfg1-4096-16",
                                  "bigvalue-8192-16"])
def test_snappy_file(oracle, case):
    torch, mtblx, encode, merger, reader, sorter = _mods()
    recs, bs, iv = _cases()[case]
    d = encode.DeviceRecords.from_list(recs)
    f = encode.write_file(d, bs, iv, compression=mtblx.CompressionType.Snappy).cpu().numpy().tobytes()
    g = encode.write_file(d, bs, iv).cpu().numpy().tobytes()
    # the restated reference Reader and the device Reader
    scan = oracle.file_scan(f, verify=True)
    assert scan["err"] == oracle.ERR_NAMES[0] and scan["records"] == recs
    assert reader.Reader(np.frombuffer(f, np.uint8)).iter().records() == recs
    # footer (src/metadata.rs:61-79): [0] index_block_offset [1] data_block_size [2] compression
    # [3] count_entries [4] count_data_blocks [5] bytes_data_blocks [6] bytes_index_block
    # [7] bytes_keys [8] bytes_values
    mf, mg = _meta(f), _meta(g)
    assert mf[2] == 1 and mg[2] == 0
    assert [mf[i] for i in (1, 3, 4, 7, 8)] == [mg[i] for i in (1, 3, 4, 7, 8)]
    ff, fg = _frames(oracle, f), _frames(oracle, g)
    assert mf[0] == mf[5] == sum(n for _, n, _ in ff)
    assert len(f) == mf[5] + mf[6] + 512
    # index: the None file's keys, values = running sums of the stored frames
    assert [k for k, _ in oracle.index_records(f)] == [k for k, _ in oracle.index_records(g)]
    run = 0
    for (_, val), (off, n, _) in zip(oracle.index_records(f), ff):
        assert val == oracle.varint_encode64(run) and off == run
        run += n
    # block b decompresses to block b of the None file; its checksum is of the stored bytes
    assert len(ff) == len(fg) == mf[4]
    for (off, n, z), (_, _, x) in zip(ff, fg):
        assert oracle.snappy_decompress(z) == x
        assert int.from_bytes(f[off + n - len(z) - 4: off + n - len(z)], "little") == oracle.crc32c(z)
    if case.startswith("bigvalue"):
        assert max(len(x) for _, _, x in fg) > 65536
    if case.startswith("cfg1"):
        assert len(f) < len(g) // 2


def test_empty_file_equals_host_writer():
    """no records: no compressed bytes are involved, so the file is the host Writer's byte for byte"""
    torch, mtblx, encode, merger, reader, sorter = _mods()
    d = encode.DeviceRecords.from_list([])
    f = encode.write_file(d, 8192, 16, compression=mtblx.CompressionType.Snappy).cpu().numpy().tobytes()
    w = mtblx.Writer(8192, 16, compression=mtblx.CompressionType.Snappy)
    assert f == w.into_inner()
    assert _meta(f)[2] == 1


def test_none_keyword_is_todays_path():
    torch, mtblx, encode, merger, reader, sorter = _mods()
    rng = np.random.default_rng(8)
    d = encode.DeviceRecords.from_list(corpus.random_records(rng, 1500, 0, 40, 0, 120))
    a = encode.write_file(d, 2048, 16)
    b = encode.write_file(d, 2048, 16, compression=mtblx.CompressionType.None_)
    assert torch.equal(a, b)


def test_merger_and_sorter_write_snappy(oracle):
    torch, mtblx, encode, merger, reader, sorter = _mods()
    snappy = mtblx.CompressionType.Snappy
    rng = np.random.default_rng(13)
    pool = [b"key%05d" % i for i in range(900)]
    sources = []
    for s in range(3):   # overlapping key sets
        keys = sorted(set(rng.choice(len(pool), 500, replace=False).tolist()))
        sources.append([(pool[i], b"src%d-" % s + b"payload " * int(rng.integers(1, 9))) for i in keys])
    readers = [reader.Reader(mm.make_source(s, 1024)) for s in sources]
    want = merger._records_list(merger.Merger.builder("concat").extend(readers).build().records())
    assert len(want) > 500
    f = merger.Merger.builder("concat").extend(readers).build().write_file(1024, 16, compression=snappy)
    f = f.cpu().numpy().tobytes()
    assert _meta(f)[2] == 1
    assert oracle.file_scan(f, verify=True)["records"] == want
    assert reader.Reader(np.frombuffer(f, np.uint8)).iter().records() == want

    recs = [(b"%06d" % int(rng.integers(0, 1500)), b"value-%d " % i * 3) for i in range(2000)]
    order = rng.permutation(len(recs))

    def filled():
        s = sorter.Sorter("concat")
        for i in order:
            s.insert(*recs[int(i)])
        return s
    want = merger._records_list(filled().records())
    assert 0 < len(want) < 2000
    f = filled().write_file(1024, 16, compression=snappy).cpu().numpy().tobytes()
    assert _meta(f)[2] == 1
    assert oracle.file_scan(f, verify=True)["records"] == want

"""Every batched entry point with positions on both sides of byte offset 2^32.

The C ABI promises 64-bit positions ("Positions are 64-bit").  Inputs live
in one sparse device allocation of 2^32 + 64 MiB (tests/line4g_util.py): a block straddles the
line at LINE - r for r in 1, 7, 15, 16, 17 (a 16-byte staging load, a dword and a single byte
each cross it) or starts exactly at LINE / LINE + 1, and every block at or above the line has a
different valid block at its offset - 2^32, where a truncated position reads.  Expected results
come from the oracle on the same blocks packed compactly on the host: no output depends on
blk_off.  Outputs are placed above the line by the caller where the ABI lets it.
tests/test_line4g.py shows on the CPU that the decoys make these comparisons able to fail.
"""
import ctypes as C
import os

import numpy as np
import pytest

import corpus
import line4g_util as u
import valpos_util as vu
from line4g_util import LINE
from test_decode_gpu import assert_same

pytestmark = pytest.mark.gpu

NEED_FREE = 24 << 30


@pytest.fixture(scope="module")
def win():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mtblx import codec
    codec._require_device()
    free, _ = torch.cuda.mem_get_info()
    if free < NEED_FREE:
        pytest.skip(f"{free >> 30} GiB of device memory free, these tests want {NEED_FREE >> 30}")
    w = u.Window("cuda")
    yield w
    del w.buf
    del w
    torch.cuda.empty_cache()


_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _decode_ref(oracle, kind):
    """(blocks, decoys, compact data / off / len, the oracle's decode, its CRCs), computed once"""
    def make():
        blocks, decoys = u.decode_batch(oracle, kind)
        d, o, l = corpus.pack(blocks)
        orc = oracle.decode_blocks(d, o, l)
        crc = np.array([oracle.crc32c(b) for b in blocks], np.uint32)
        return blocks, decoys, (d, o, l), orc, crc
    return _once(("decode", kind), make)


def _batch(win, lay, off, ln):
    from mtblx import codec
    return codec.DeviceBatch(win.buf, off, ln, int(lay.ln.max()))


# ------------------------------------------------------------------ A. inputs above the line
@pytest.mark.parametrize("r", u.STARTS)
@pytest.mark.parametrize("kind", u.DECODE_KINDS)
def test_decode_inputs(oracle, win, kind, r):
    """mtblx_decode_blocks, _valpos, _verify (two launches and fused) and mtblx_count_blocks on
    blocks around the line.  The batch's longest block picks the kernel (make_plan): "small" and
    "mutated" run k_decode_pipe<PipeSmall> (PipeSmallP for positions; fused PipeSmallV, whose
    smaller tile takes blocks up to 49 089 B: these batches stay below it), "large"
    k_decode_pipe<PipeLarge> (V / P likewise), "tiles" k_decode_tiles<CfgLarge> (its verify is the
    separate CRC launch); "mutated" takes the irregular walk and yields every status."""
    import torch
    from mtblx import codec
    blocks, decoys, (d, o, l), orc, crc_exp = _decode_ref(oracle, kind)
    if kind == "mutated":
        assert {0, 1, 2} <= set(orc.status.tolist())
    else:
        assert (orc.status == 0).all()
    lay, (off, ln) = win.place(blocks, decoys, np.random.default_rng(100 + r), r)
    batch = _batch(win, lay, off, ln)
    nr = int(orc.nrec.sum())
    want = (nr, orc.keys.size, orc.vals.size, 0)

    probe = codec.DecodedBlocks(batch.nblk, 0, 0, 0)
    codec.count_blocks(batch, probe, codec.Workspace(batch.nblk))
    assert probe.totals_host() == want

    assert_same(codec.decode_blocks(batch).to_host(), orc, len(blocks))

    for fused in (False, True):
        out, crc, bad = codec.decode_verify(batch, framed=False, fused=fused)
        assert_same(out.to_host(), orc, len(blocks))
        got = crc.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, crc_exp), (fused, np.nonzero(got != crc_exp)[0][:10])
        assert not bad.cpu().numpy().any()

    out, vp = codec.decode_positions(batch)
    dev = out.to_host()
    for f in ("status", "nrec", "rec_base", "key_base", "val_base", "key_end", "val_end", "keys"):
        assert np.array_equal(getattr(dev, f), getattr(orc, f)), f
    assert tuple(dev.totals) == want
    vu.check_positions(d, o, l, orc, vp.cpu().numpy().view(np.uint32))
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", ["small", "large", "tiles"])
def test_decode_window_past_data_len(oracle, win, kind):
    """one block whose window runs one byte past data_len: MTBLX_ST_CORRUPT, no records; the other
    blocks, above the line, are unaffected.  The block's own valid bytes lie under the window, at the
    end of the allocation, and the batch is given a data_len one byte short of them: a missing bound
    check, or one on a truncated end (which lies far inside the buffer), decodes the block's records
    with status 0 instead."""
    from mtblx import codec
    import torch
    blocks, decoys, _, orc, _ = _decode_ref(oracle, kind)
    lay, (off, ln) = win.place(blocks, decoys, np.random.default_rng(7), 16)
    j = max(range(len(blocks)), key=lambda i: (orc.nrec[i] > 0 and i != lay.first, -len(blocks[i])))
    assert orc.status[j] == 0 and orc.nrec[j] > 0
    at = u.SIZE - len(blocks[j])
    win.write(at - u.PAD, np.zeros(u.PAD, np.uint8))
    win.write(at, blocks[j])                     # the whole valid block, ending with the allocation
    off = off.clone()
    off[j] = at
    whole = codec.DeviceBatch(win.buf, off, ln, int(lay.ln.max()))
    assert codec.decode_blocks(whole).to_host().records(j) == orc.records(j)     # in bounds: decoded
    short = codec.DeviceBatch(win.buf[: u.SIZE - 1], off, ln, int(lay.ln.max()))   # data_len one byte short
    assert short.cstruct().data_len == u.SIZE - 1
    dev = codec.decode_blocks(short).to_host()
    torch.cuda.synchronize()
    assert dev.status[j] == 2 and dev.nrec[j] == 0
    keep = np.arange(len(blocks)) != j
    assert np.array_equal(dev.status[keep], orc.status[keep]) and np.array_equal(dev.nrec[keep], orc.nrec[keep])
    for b in (lay.first, (j + 1) % len(blocks), len(blocks) - 1):
        assert b == j or dev.records(b) == orc.records(b)


def _crc_env(kernel):
    old = os.environ.get("MTBLX_CRC_KERNEL")
    os.environ["MTBLX_CRC_KERNEL"] = kernel
    return old


def _crc_restore(old):
    if old is None:
        del os.environ["MTBLX_CRC_KERNEL"]
    else:
        os.environ["MTBLX_CRC_KERNEL"] = old


def _crc_run(win, lay, off, ln, kernel, framed):
    import torch
    from mtblx import codec
    old = _crc_env(kernel)
    try:
        crc, bad = codec.crc32c_blocks(_batch(win, lay, off, ln), framed=framed)
        torch.cuda.synchronize()
    finally:
        _crc_restore(old)
    return crc.cpu().numpy().view(np.uint32), (bad.cpu().numpy() if framed else None)


@pytest.mark.parametrize("r", u.STARTS)
@pytest.mark.parametrize("framed", [False, True])
@pytest.mark.parametrize("kernel", ["mfma", "lanes"])
def test_crc_inputs(oracle, win, kernel, framed, r):
    """mtblx_crc32c_blocks (k_crc32c_mfma / the VALU table kernel) on contents of every length
    0..600 around the line; framed: the stored checksum precedes each content and, for r = 1,
    that of the straddling block itself crosses the line"""
    lead = 4 if framed else 0
    blocks, decoys = _once(("crc", framed), lambda: u.crc_batch(oracle, framed))
    exp = _once(("crcexp", framed), lambda: np.array([oracle.crc32c(b[lead:]) for b in blocks], np.uint32))
    lay, (off, ln) = win.place(blocks, decoys, np.random.default_rng(200 + r), r, lead)
    got, bad = _crc_run(win, lay, off, ln, kernel, framed)
    assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:10]
    if framed:
        assert not bad.any()
        j = int(np.nonzero(lay.high)[0][3])          # a wrong stored checksum above the line is seen
        win.write(int(lay.off[j]) - 2, b"\x5a" if blocks[j][2] != 0x5a else b"\x5b")
        got, bad = _crc_run(win, lay, off, ln, kernel, framed)
        assert np.array_equal(got, exp) and np.nonzero(bad)[0].tolist() == [j]


@pytest.mark.parametrize("kernel", ["mfma", "lanes"])
def test_crc_split_pass_straddles(oracle, win, kernel):
    """a content above 256 KiB (the split pass: 16 columns of one block) that starts at LINE - r
    and so has the line inside its first columns, framed, among the short contents"""
    blocks, decoys = _once(("crcbig",), lambda: u.crc_batch(oracle, True, big=300_000))
    exp = _once(("crcbigexp",), lambda: np.array([oracle.crc32c(b[4:]) for b in blocks], np.uint32))
    big = max(range(len(blocks)), key=lambda i: len(blocks[i]))
    for r in (1, 16, 150_001):
        lay, (off, ln) = win.place(blocks, decoys, np.random.default_rng(r), r, 4, first=big)
        got, bad = _crc_run(win, lay, off, ln, kernel, True)
        assert np.array_equal(got, exp), (r, np.nonzero(got != exp)[0][:10])
        assert not bad.any()


SNAPPY_KERNELS = ["auto", "lanes", "two", "waves"]


@pytest.fixture
def snappy_kernel(request, monkeypatch):
    if request.param == "auto":
        monkeypatch.delenv("MTBLX_SNAPPY_KERNEL", raising=False)
    else:
        monkeypatch.setenv("MTBLX_SNAPPY_KERNEL", request.param)
    return request.param


def _snappy_ref(oracle, size):
    def make():
        streams, decoys = u.snappy_batch(oracle, small=size == "small")
        exp = [oracle.snappy_decompress(z) for z in streams]
        mx = max(len(e) for e in exp if e is not None)
        assert mx == u.SNAPPY_QUAD_OUT if size == "small" else mx > 65 * 1024
        return streams, decoys, exp
    return _once(("snappy", size), make)


# the largest output of a batch picks the kernels (mtblx_snappy_decompress_dev): at or below
# quad::OUT = 4608 B the knobs choose among k_snappy_quads, k_snappy_lanes, k_snappy_parse +
# k_snappy_exec, k_snappy_waves and k_snappy_deferred ("small"); above it every block runs
# k_snappy_blocks<Large>, or k_snappy_lanes under "lanes" ("large": outputs above 65 KiB, assembled in HBM)
SNAPPY_SIZES = ["small", "large"]


@pytest.mark.parametrize("r", u.STARTS)
@pytest.mark.parametrize("size", SNAPPY_SIZES)
@pytest.mark.parametrize("snappy_kernel", SNAPPY_KERNELS, indirect=True)
def test_snappy_decompress_inputs(oracle, win, snappy_kernel, size, r):
    """mtblx_snappy_dir + mtblx_snappy_decompress_dev with src_off around the line, under every
    knob, for a batch of small outputs (the quad kernel and, for the blocks expanding more than
    2x, k_snappy_lanes / parse + exec / the waves kernel; the deferred pass) and one with outputs
    above 65 KiB (k_snappy_blocks<Large>, assembled in HBM); hand-made wasteful encodings and one
    corrupt stream in both"""
    import torch
    from mtblx import codec
    streams, decoys, exp = _snappy_ref(oracle, size)
    lay, (off, ln) = win.place(streams, decoys, np.random.default_rng(300 + r), r)
    dec, st = codec.snappy_decompress(codec.SnappyBatch(win.buf, off, ln))
    torch.cuda.synchronize()
    host = dec.data.cpu().numpy()
    o = dec.blk_off.cpu().numpy().view(np.uint64)
    n = dec.blk_len.cpu().numpy().view(np.uint32)
    st = st.cpu().numpy()
    assert (o % 16 == 0).all()
    for i, e in enumerate(exp):
        if e is None:
            assert st[i] == 1, i
        else:
            assert st[i] == 0, (i, st[i])
            assert bytes(host[int(o[i]): int(o[i]) + int(n[i])]) == e, i


def _compress_ref(oracle):
    """the blocks the compressor and the framing take: the "tiles" decode batch (builder blocks
    of every shape up to 100 KB, so some cross a 64 KiB fragment) and the compressible inputs"""
    def make():
        import test_snappy_gpu as tsg
        blocks, decoys = u.decode_batch(oracle, "tiles", seed=77)
        rng = np.random.default_rng(78)
        for x in tsg._compressible(rng):
            if len(x) >= 24:
                blocks.append(x)
                decoys.append(bytes(rng.integers(0, 256, len(x), dtype=np.uint8)))
        return blocks, decoys
    return _once(("compress",), make)


def _low_copy(lay):
    """the real region of a layout as a compact device buffer with the same offsets mod 16"""
    import torch
    pos, real = lay.regions[1]
    pad = pos % 16
    t = torch.from_numpy(np.concatenate([np.zeros(pad, np.uint8), real])).to("cuda")
    off = (lay.off - np.uint64(pos - pad)).view(np.int64)
    return t, torch.from_numpy(off.copy()).to("cuda")


@pytest.mark.parametrize("r", u.STARTS)
def test_snappy_compress_inputs(oracle, win, r):
    """mtblx_snappy_slots + mtblx_snappy_compress_dev with the source blocks around the line:
    every stream decompresses (oracle) to its block, and equals the stream of the same call on a
    compact copy below the line with the same src_off % 16 (the compressor is position-free)"""
    import torch
    from mtblx import codec
    blocks, decoys = _compress_ref(oracle)
    lay, (off, ln) = win.place(blocks, decoys, np.random.default_rng(400 + r), r)
    comp, st = codec.snappy_compress(_batch(win, lay, off, ln))
    low, low_off = _low_copy(lay)
    comp2, st2 = codec.snappy_compress(codec.DeviceBatch(low, low_off, ln, int(lay.ln.max())))
    torch.cuda.synchronize()
    assert not st.cpu().numpy().any() and not st2.cpu().numpy().any()
    outs = []
    for c in (comp, comp2):
        h, o, n = c.data.cpu().numpy(), c.src_off.cpu().numpy(), c.src_len.cpu().numpy()
        outs.append([bytes(h[int(a): int(a) + int(b)]) for a, b in zip(o, n)])
    for i, b in enumerate(blocks):
        assert oracle.snappy_decompress(outs[0][i]) == b, i
    assert outs[0] == outs[1]


def _varint64(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


@pytest.mark.parametrize("r", u.STARTS)
def test_frame_blocks_inputs(oracle, win, r):
    """mtblx_frame_blocks over stored contents around the line: varint64(len) | crc32c LE |
    content back to back, blk_off the content starts (its checksums: the mtblx_crc32c_blocks
    kernel, its copies: src_off in 64 bits)"""
    import torch
    from mtblx import _lib, codec
    blocks, decoys = _compress_ref(oracle)
    lay, (off, ln) = win.place(blocks, decoys, np.random.default_rng(500 + r), r)
    exp, eoff = bytearray(), []
    for b in blocks:
        exp += _varint64(len(b)) + oracle.crc32c(b).to_bytes(4, "little")
        eoff.append(len(exp))
        exp += b
    nblk = len(blocks)
    L = _lib.lib()
    out = torch.full((len(exp) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    boff = torch.zeros(nblk, dtype=torch.int64, device="cuda")
    tot = torch.zeros(2, dtype=torch.int64, device="cuda")
    wsb = int(L.mtblx_snappy_compress_workspace_bytes(nblk))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    rc = L.mtblx_frame_blocks(C.c_void_p(win.buf.data_ptr()), C.c_void_p(off.data_ptr()), C.c_void_p(ln.data_ptr()),
                              nblk, C.c_void_p(out.data_ptr()), len(exp), C.c_void_p(boff.data_ptr()),
                              C.c_void_p(tot.data_ptr()), C.c_void_p(ws.data_ptr()), wsb,
                              C.c_void_p(codec._stream_handle(None)))
    assert rc == 0
    torch.cuda.synchronize()
    assert tot.tolist() == [len(exp), 0]
    assert boff.tolist() == eoff
    h = out.cpu().numpy()
    assert bytes(h[: len(exp)]) == bytes(exp)
    assert (h[len(exp):] == 0xA5).all()


@pytest.mark.parametrize("r", u.STARTS)
def test_copy_ranges_inputs(oracle, win, r):
    """mtblx_copy_ranges with ragged, unaligned source ranges (0..40 B, tens of KB) around the
    line, among them ranges that cross it at every alignment, against the host copy"""
    import torch
    from mtblx import _lib, codec
    blocks, decoys = _compress_ref(oracle)
    lay, (off, ln) = win.place(blocks, decoys, np.random.default_rng(600 + r), r)
    pos, real = lay.regions[1]
    rng = np.random.default_rng(r + 9)
    lens = [int(x) for x in rng.integers(0, 41, 200)] + [70_001, 17, 0, 4099]
    so = [pos + int(rng.integers(u.PAD, real.size - u.PAD - n)) for n in lens]
    for i in range(0, 60):                      # ranges that cross the line, every start residue
        so[i] = LINE - (i % 33)
        lens[i] = max(lens[i], (i % 33) + 1)
    so += [int(a) for a in lay.off]             # and every placed block
    lens += [int(n) for n in lay.ln]
    do, acc = [], 5
    for n in lens:
        do.append(acc)
        acc += n + int(rng.integers(0, 3))
    dst = np.zeros(acc + 16, np.uint8)
    ch = [(n + 15) // 16 for n in lens]
    cb = np.concatenate([[0], np.cumsum(ch)[:-1]]).astype(np.int64)
    t = lambda a: torch.tensor(np.asarray(a, np.int64), device="cuda")   # noqa: E731
    dd = torch.from_numpy(dst).to("cuda")
    args = [t(so), t(do), t(lens), t(cb)]
    rc = _lib.lib().mtblx_copy_ranges(C.c_void_p(win.buf.data_ptr()), C.c_void_p(args[0].data_ptr()),
                                      C.c_void_p(dd.data_ptr()), C.c_void_p(args[1].data_ptr()),
                                      C.c_void_p(args[2].data_ptr()), C.c_void_p(args[3].data_ptr()), len(lens),
                                      int(sum(ch)), C.c_void_p(codec._stream_handle(None)))
    assert rc == 0
    torch.cuda.synchronize()
    for a, b, n in zip(so, do, lens):
        dst[b: b + n] = real[a - pos: a - pos + n]
    assert np.array_equal(dd.cpu().numpy(), dst)


# ------------------------------------------------------------------ B. outputs above the line
def _untouched(dst, upto):
    """dst[:upto] is still all 0xA5 (checked on the device, in chunks); upto % 8 == 0"""
    import torch
    assert upto % 8 == 0
    words = dst[:upto].view(torch.int64)
    fill = int.from_bytes(b"\xA5" * 8, "little", signed=True)
    step = 1 << 27
    for a in range(0, words.numel(), step):
        if not bool((words[a: a + step] == fill).all()):
            return False
    return True


def _bases(dst_off, dst_len):
    """offsets to add to a 16-byte aligned layout so that, in turn, a long block and a short one
    straddle the line (it falls 16 bytes into the block) and start exactly on it"""
    big = int(np.argmax(dst_len))
    small = next(i for i in range(len(dst_len) // 2, len(dst_len)) if 32 <= dst_len[i] < 4000)
    out = []
    for j in (big, small):
        out += [LINE - int(dst_off[j]) - 16, LINE - int(dst_off[j])]
    return out


@pytest.mark.parametrize("size", SNAPPY_SIZES)
@pytest.mark.parametrize("snappy_kernel", SNAPPY_KERNELS, indirect=True)
def test_snappy_decompress_outputs_above(oracle, win, snappy_kernel, size):
    """mtblx_snappy_decompress_dev with every dst_off moved up by LINE - k (sources above the
    line as well): the outputs are where the layout says, and nothing below them was written"""
    import torch
    from mtblx import codec
    streams, decoys, exp = _snappy_ref(oracle, size)
    lay, (off, ln) = win.place(streams, decoys, np.random.default_rng(31), 7)
    batch = codec.SnappyBatch(win.buf, off, ln)
    sl = codec.SnappyLayout(batch.nblk)
    codec.snappy_dir(batch, sl)
    total, mx = int(sl.totals[0].item()), int(sl.totals[1].item())
    o0 = sl.dst_off.cpu().numpy().copy()
    n0 = sl.dst_len.cpu().numpy().view(np.uint32)
    dst = torch.empty(LINE + total + 64, dtype=torch.uint8, device="cuda")
    for base in _bases(o0, n0):
        assert base % 16 == 0
        dst.fill_(0xA5)
        sl.dst_off.copy_(torch.from_numpy(o0 + base))
        st = torch.full((batch.nblk,), -1, dtype=torch.int32, device="cuda")
        dl = torch.full((batch.nblk,), -1, dtype=torch.int32, device="cuda")
        codec.snappy_decompress_into(batch, sl, dst, st, dl, mx)
        torch.cuda.synchronize()
        st, dl = st.cpu().numpy(), dl.cpu().numpy()
        h = dst[base: base + total].cpu().numpy()
        for i, e in enumerate(exp):
            if e is None:
                assert st[i] == 1 and dl[i] == 0, i
            else:
                assert st[i] == 0 and dl[i] == len(e), (i, st[i])
                assert bytes(h[int(o0[i]): int(o0[i]) + len(e)]) == e, (base, i)
        assert _untouched(dst, base), base
    del dst
    torch.cuda.empty_cache()


def test_snappy_compress_outputs_above(oracle, win):
    """mtblx_snappy_compress_dev with every slot moved up by LINE - k: each stream, read back
    from above the line, decompresses to its block; nothing below the slots was written"""
    import torch
    from mtblx import codec
    blocks, decoys = _compress_ref(oracle)
    lay, (off, ln) = win.place(blocks, decoys, np.random.default_rng(32), 15)
    batch = _batch(win, lay, off, ln)
    slots = codec.SnappySlots(batch.nblk)
    codec.snappy_slots(batch, slots)
    total = int(slots.totals[0].item())
    o0 = slots.dst_off.cpu().numpy().copy()
    dst = torch.empty(LINE + total + 64, dtype=torch.uint8, device="cuda")
    for base in _bases(o0, lay.ln):
        dst.fill_(0xA5)
        slots.dst_off.copy_(torch.from_numpy(o0 + base))
        dl = torch.full((batch.nblk,), -1, dtype=torch.int32, device="cuda")
        st = torch.full((batch.nblk,), -1, dtype=torch.int32, device="cuda")
        codec.snappy_compress_into(batch, slots, dst, dl, st)
        torch.cuda.synchronize()
        assert not st.cpu().numpy().any()
        dl = dl.cpu().numpy()
        h = dst[base: base + total].cpu().numpy()
        for i, b in enumerate(blocks):
            assert oracle.snappy_decompress(bytes(h[int(o0[i]): int(o0[i]) + int(dl[i])])) == b, (base, i)
        assert _untouched(dst, base), base
    del dst
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ C. a file with blocks above the line
# the length varint of a 4 KiB block is 2 bytes, its checksum the next 4: block j's frame starts at
# LINE - r, so the varint (1), the checksum (4) and the content (7, 100) cross the line in turn
FILE_RESIDUES = (1, 4, 7, 100)


def _file(oracle, comp, fields=0):
    """a compact V2 file (6000 random records, 4 KiB blocks; fields > 0: values of that many u64),
    its records, frames and the block that moves to the line"""
    def make():
        from mtblx.writer import Writer
        rng = np.random.default_rng(9 + comp + 10 * fields)
        recs = corpus.random_records(rng, 6000, 1, 40, 0, 0 if fields else 120)
        if fields:
            from test_scan_reduce_gpu import _values
            recs = list(zip([k for k, _ in recs], _values(rng, len(recs), fields)))
        w = Writer(4096, 16, comp)
        for k, v in recs:
            w.insert(k, v)
        data = bytes(w.into_inner())
        frames = u.v2_frames(data)
        return data, recs, frames, len(frames) // 2
    return _once(("file", comp, fields), make)


def _sparse(buf, data, j, r):
    """the spread file assembled in `buf` (a device allocation from offset 0) -> (view, displacement)"""
    (p0, head), (p1, tail), total, disp = u.spread(data, j, r)
    assert total <= buf.numel() and p1 + len(tail) == total and len(head) + u.PAD < p1
    import torch
    for p, b in ((p0, head), (p1, tail)):
        buf[p: p + len(b)].copy_(torch.from_numpy(np.frombuffer(b, np.uint8).copy()))
    return buf[:total], disp


def _gather(src, offs, lens):
    """bytes src[offs[i] : offs[i] + lens[i]] for every i, one device gather -> list of bytes"""
    import torch
    lens = np.asarray(lens, np.int64)
    offs = np.asarray(offs, np.int64)
    ends = np.cumsum(lens)
    idx = np.repeat(offs - (ends - lens), lens) + np.arange(int(ends[-1]) if ends.size else 0)
    h = src[torch.from_numpy(idx).to(src.device)].cpu().numpy() if idx.size else np.zeros(0, np.uint8)
    return [bytes(h[int(e - n): int(e)]) for e, n in zip(ends, lens)]


def _line_queries(recs, frames, j):
    """queries that begin in the blocks below the line and end above it, and their limits"""
    import bisect
    keys = [k for k, _ in recs]
    seps = [f[0] for f in frames]
    first = lambda b: keys[bisect.bisect_right(keys, seps[b - 1])]   # noqa: E731
    a, b, c = first(j - 2), first(j), first(j + 2)
    qs = [("range", a, c), ("range", first(j - 1), first(j + 1)), ("from", a), ("from", first(j - 1)),
          ("prefix", a[:1]), ("prefix", b[:1]), ("get", b), ("get", first(j + 1)), ("range", b, c), ("prefix", b"")]
    return qs, [None, None, 300, 150, None, None, None, None, None, None]


@pytest.mark.parametrize("r", FILE_RESIDUES)
@pytest.mark.parametrize("verify", [True, False])
@pytest.mark.parametrize("comp", [0, 1])
def test_reader_file_across_line(oracle, win, comp, verify, r, monkeypatch):
    """The device Reader on a file whose second half starts at LINE - r (5-byte offsets in the
    index: k_block_dir, k_get / k_get_lanes, the scan plan / emit, and for Snappy the stage plan /
    emit, mtblx_scan_touch and the on-demand table), every surface against the oracle on the
    compact file"""
    import scan_util as su
    from mtblx import _lib, reader as rd
    data, recs, frames, j = _file(oracle, comp)
    file, disp = _sparse(win.buf, data, j, r)
    R = rd.ReaderBuilder().verify_checksums(verify).read(file)
    # the moved blocks, the rebuilt index block, the footer
    assert R.len == int(file.numel()) == LINE - r + int.from_bytes(data[-512:-504], "little") - frames[j][1] + R.meta[6] + 512
    # directory: the known displacement, lengths and statuses unchanged
    off, ln, st, bad = R.directory()
    exp_off = np.array([o + ll + 4 + (disp if i >= j else 0) for i, (_, o, ll, _) in enumerate(frames)], np.int64)
    assert np.array_equal(off.cpu().numpy(), exp_off)
    assert exp_off[j] - frames[j][2] - 4 == LINE - r and len(oracle.varint_encode64(int(exp_off[-1]))) == 5
    assert np.array_equal(ln.cpu().numpy(), np.array([n for _, _, _, n in frames], np.int32))
    assert not st.cpu().numpy().any()
    assert (bad is None) == (not verify) and (bad is None or not bad.cpu().numpy().any())
    # point lookups on both kernels: every key and absent neighbours
    keys = [k for k, _ in recs]
    have = dict(recs)
    qs = keys + [k + b"\x00" for k in keys[::7]] + [k[:-1] for k in keys[::11] if k] + [b"", b"\xff" * 41]
    compact = rd.ReaderBuilder().verify_checksums(verify).read(data)
    for knob in ("lanes", "wave"):
        monkeypatch.setenv("MTBLX_GET_KERNEL", knob)
        gs, vo, vl = (t.cpu().numpy() for t in R.get_batch(qs))
        found = np.array([q in have for q in qs])
        assert np.array_equal(gs == _lib.GET_FOUND, found) and (gs[~found] == _lib.GET_NONE).all(), knob
        got = _gather(R.value_source, vo[found], vl[found])
        assert got == [have[q] for q, f in zip(qs, found) if f], knob
        if comp == 0:   # positions: the compact file's plus the displacement
            _, vo0, vl0 = (t.cpu().numpy() for t in compact.get_batch(qs))
            cut = frames[j][1]
            assert np.array_equal(vo[found], vo0[found] + np.where(vo0[found] >= cut, disp, 0))
            assert np.array_equal(vl[found], vl0[found])
    monkeypatch.delenv("MTBLX_GET_KERNEL")
    # batched scans and counts, all four query types, across the line
    lq, ll_ = _line_queries(recs, frames, j)
    pq, pl = su.queries_for(su.probe_keys(np.random.default_rng(r), recs, 12))
    qs2, lim = lq + pq, ll_ + pl
    tag = ("line4g", comp)
    sb = R.scan_batch(qs2, max_blocks=64, max_records=lim)
    for i, (q, m) in enumerate(zip(qs2, lim)):
        su.check(rd, sb, i, su.expected(oracle, data, q, m, verify, tag=tag), q)
    assert sb.n_fallback == 0 and any(sb.served_by_kernel(i) for i in range(len(lq)))
    cs, cn, ck, cv = (t.cpu().numpy() for t in R.count_batch(qs2))
    for i, q in enumerate(qs2):
        if cs[i] == _lib.SCAN_OK:
            e = su.expected(oracle, data, q, None, verify, tag=tag)["records"]
            assert (cn[i], ck[i], cv[i]) == (len(e), sum(len(k) for k, _ in e), sum(len(v) for _, v in e)), q
    assert (cs[: len(lq)] == _lib.SCAN_OK).sum() >= 6
    # the seek path and the whole scan
    a, b = lq[0][1], lq[0][2]
    for s, mode, k1, k2 in ((R.iter_from(b), "from", b, b""), (R.iter_prefix(a[:1]), "prefix", a[:1], b""),
                            (R.iter_range(a, b), "range", a, b), (R.iter(), "iter", b"", b"")):
        e = oracle.file_scan(data, mode, k1, k2, verify=verify)
        assert s.end == e["end"] and s.records() == e["records"], mode
    it = R.into_iter("from", a)
    got = [it.next(), None]
    it.seek(b)
    got[1] = it.next()
    assert got == oracle.iter_script(data, "from", a, b"", [1, ("seek", b), 1], verify=verify)["records"]
    if comp == 1:
        s = R.stage_stats
        assert s["host_blocks"] == 0 and s["device_blocks"] >= len(frames) and R.table_mode == "on-demand"
        assert 0 < s["resident_blocks"] <= len(frames)


@pytest.mark.parametrize("comp", [0, 1])
def test_reader_reduce_across_line(oracle, win, comp):
    """Reader.reduce_batch (mtblx_scan_reduce: the plan walk reads each value where it lies) on a
    file of 24-byte values whose second half lies above the line"""
    import scan_util as su
    from mtblx import reader as rd
    from test_scan_reduce_gpu import _check, _red
    data, recs, frames, j = _file(oracle, comp, fields=3)
    file, _ = _sparse(win.buf, data, j, 7)
    R = rd.ReaderBuilder().read(file)
    lq, ll_ = _line_queries(recs, frames, j)
    pq, pl = su.queries_for(su.probe_keys(np.random.default_rng(3), recs, 10))
    red = _red(3)
    rb = R.reduce_batch(lq + pq, red, max_records=ll_ + pl)
    _check(oracle, rb, red, data, lq + pq, ll_ + pl, True, ("line4g-red", comp))
    assert rb.n_fallback == 0


@pytest.mark.parametrize("comp", [0, 1])
def test_reader_corrupt_block_above_line(oracle, win, comp):
    """one flipped byte inside a block above the line, checksums on: reported exactly where the
    oracle reports it for the compact file with the same flip"""
    from mtblx import _lib, reader as rd
    data, recs, frames, j = _file(oracle, comp)
    _, o, ll, n = frames[j + 3]
    at = o + ll + 4 + n // 2
    bad = bytearray(data)
    bad[at] ^= 0x20
    bad = bytes(bad)
    file, disp = _sparse(win.buf, bad, j, 4)
    R = rd.ReaderBuilder().read(file)
    e = oracle.file_scan(bad, "iter", verify=True)
    s = R.iter()
    assert s.end == e["end"] == rd.END_PANIC and s.records() == e["records"]
    crc_bad = R.directory()[3].cpu().numpy()
    assert np.nonzero(crc_bad)[0].tolist() == [j + 3]
    import bisect
    keys = [k for k, _ in recs]
    lo = bisect.bisect_right(keys, frames[j + 2][0])
    qs = keys[lo - 2: lo + 3] + [keys[0], keys[-1]]
    gs = R.get_batch(qs)[0].cpu().numpy()
    want = []
    for q in qs:
        x = oracle.file_scan(bad, "get", key=q, verify=True)
        want.append(_lib.GET_FOUND if x["records"] else {rd.END_NONE: _lib.GET_NONE, rd.END_PANIC: _lib.GET_PANIC}[x["end"]])
    assert gs.tolist() == want and _lib.GET_PANIC in want and _lib.GET_FOUND in want


def test_merger_scan_two_sparse_files(oracle, win):
    """Merger.scan_batch, mode concat, over two files that both continue above the line: equal to
    the merge over the two compact files"""
    import torch
    from mtblx import merger, reader as rd
    d0, recs, frames, j = _file(oracle, 0)
    d1, recs1, frames1, j1 = _file(oracle, 1)
    second = torch.empty(LINE + (1 << 20), dtype=torch.uint8, device="cuda")
    f0, _ = _sparse(win.buf, d0, j, 7)
    f1, _ = _sparse(second, d1, j1 - 5, 1)
    lq, ll_ = _line_queries(recs, frames, j)
    lq1, ll1 = _line_queries(recs1, frames1, j1 - 5)
    qs, lim = lq[:-1] + lq1[:-1], ll_[:-1] + ll1[:-1]
    build = lambda rs: merger.Merger.builder("concat").extend(rs).build()   # noqa: E731
    got = build([rd.Reader(f0), rd.Reader(f1)]).scan_batch(qs, max_records=lim)
    exp = build([rd.Reader(d0), rd.Reader(d1)]).scan_batch(qs, max_records=lim)
    total = 0
    for q in range(len(qs)):
        a = got.records(q)
        assert a == exp.records(q), qs[q]
        total += len(a)
    assert total > 1000 and any(got.served_by_kernel(q) for q in range(len(qs)))
    del second, f1
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ B. kernel-placed outputs above the line
def _period_blocks(oracle, kind, swap):
    """P = 7 distinct blocks of the plan kind's size with unequal record counts and lengths; values
    (swap: unshared keys, restart interval 1) take over 95 % of each, and the bytes one period of
    the directory emits are odd in number, so later entries meet the line at odd offsets"""
    rng = np.random.default_rng(len(kind) + 2 * swap)
    target = {"small": 4000, "large": 60000, "tiles": 200000}[kind]
    blocks = []
    for i in range(7):
        n = 3 + i
        big = [(target - 300 * i) // n - 7 * k for k in range(n)]
        if i == 6 and (sum(sum(b[1]) for b in blocks) + sum(big)) % 2 == 0:
            big[0] += 1          # the period, the sum of all these lengths, comes out odd
        keys = sorted(bytes(rng.integers(0, 256, 8, dtype=np.uint8)) for _ in range(n))
        recs = []
        for k, m in zip(keys, big):
            body = bytes(rng.integers(0, 256, m, dtype=np.uint8))
            recs.append((k[:1] + body, k[:2]) if swap else (k, body))
        recs.sort()
        blocks.append((oracle.build_block(recs, restart_interval=1 if swap else 16), big))
    out = [b for b, _ in blocks]
    lo, hi = {"small": (3000, u.PLAN_MAX["small"]), "large": (u.PLAN_MAX["small"] + 1, u.PLAN_MAX["large"]),
              "tiles": (u.PLAN_MAX["large"] + 1, 1 << 20)}[kind]
    assert max(len(b) for b in out) <= hi and (kind == "small" or max(len(b) for b in out) >= lo)
    return out


def _periodic(t, period, total):
    """t[:total - period] == t[period:total] on the device, in chunks"""
    import torch
    step = 1 << 28
    for a in range(0, total - period, step):
        n = min(step, total - period - a)
        if not torch.equal(t[a: a + n], t[a + period: a + period + n]):
            return False
    return True


@pytest.mark.parametrize("kind,swap", [("small", False), ("large", False), ("tiles", False), ("small", True)])
def test_decode_outputs_above(oracle, kind, swap):
    """mtblx_decode_blocks writing past 2^32: a directory of N entries aliasing P = 7 blocks
    (entry i -> block i % 7), N the smallest multiple of 7 whose value bytes (swap: key bytes)
    reach LINE + 64 MiB -- about 1.5 M entries on k_decode_pipe<PipeSmall>, 74 k on <PipeLarge>,
    22 k on k_decode_tiles.  Bases and totals equal a u64 cumsum of the oracle's sizes, the first
    period equals the oracle's decode, and every later period equals the one before it (compared
    on the device; the 4.3 GiB never come to the host)."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mtblx import codec
    if torch.cuda.mem_get_info()[0] < NEED_FREE:
        pytest.skip("not enough free device memory")
    blocks = _period_blocks(oracle, kind, swap)
    P = len(blocks)
    d, o, l = corpus.pack(blocks, rng=np.random.default_rng(5), lead=3)
    orc = oracle.decode_blocks(d, o, l)
    assert (orc.status == 0).all() and len(set(orc.nrec.tolist())) == P
    kb = np.diff(np.append(orc.key_base, orc.keys.size)).astype(np.uint64)
    vb = np.diff(np.append(orc.val_base, orc.vals.size)).astype(np.uint64)
    K, S, Rp = int(kb.sum()), int(vb.sum()), int(orc.nrec.sum())
    per = K if swap else S
    assert per % 2 == 1 and (vb if not swap else kb).sum() > 0.95 * sum(len(b) for b in blocks)
    N = P * -(-(LINE + u.TAIL) // per)
    off, ln = np.tile(o, N // P), np.tile(l, N // P)
    batch = codec.DeviceBatch.from_host(d, off, ln)
    out = codec.decode_blocks(batch)
    nr, tk, tv, flags = out.totals_host()
    assert (nr, tk, tv, flags) == (N // P * Rp, N // P * K, N // P * S, 0)
    assert (tk if swap else tv) >= LINE + u.TAIL
    excl = lambda x: np.concatenate([[0], np.cumsum(np.tile(x, N // P).astype(np.uint64), dtype=np.uint64)[:-1]])  # noqa: E731
    g = lambda t: t[:N].cpu().numpy()   # noqa: E731
    assert not g(out.status).any()
    assert np.array_equal(g(out.nrec).view(np.uint32), np.tile(orc.nrec, N // P))
    assert np.array_equal(g(out.rec_base).view(np.uint64), excl(orc.nrec))
    assert np.array_equal(g(out.key_base).view(np.uint64), excl(kb))
    assert np.array_equal(g(out.val_base).view(np.uint64), excl(vb))
    assert int(excl(kb if swap else vb)[-1]) > LINE
    # the first period against the oracle, every later one against its predecessor
    assert np.array_equal(out.keys[:K].cpu().numpy(), orc.keys) and np.array_equal(out.vals[:S].cpu().numpy(), orc.vals)
    assert np.array_equal(out.key_end[:Rp].cpu().numpy().view(np.uint32), orc.key_end)
    assert np.array_equal(out.val_end[:Rp].cpu().numpy().view(np.uint32), orc.val_end)
    assert _periodic(out.vals, S, tv) and _periodic(out.keys, K, tk)
    assert _periodic(out.key_end, Rp, nr) and _periodic(out.val_end, Rp, nr)
    del out, batch
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ D. records whose bytes lie above the line
GIANT = (1 << 31) + 4099
STAND = (b"<giant value #0>", b"<giant value #1>")     # 16-byte stand-ins of the two giants in the host model


def _fill_giant(dst, mul):
    """dst (uint8 [GIANT], device) = the bytes of (arange * mul + mul) as int32"""
    import torch
    a = torch.arange((GIANT + 3) // 4, dtype=torch.int32, device=dst.device)
    a.mul_(mul).add_(mul)
    dst.copy_(a.view(torch.uint8)[:GIANT])


def _small_pool(n):
    """n records of tests/test_sorter_gpu.py's key pool with distinct keys, sorted; all after b"a1\""""
    from test_sorter_gpu import _pool_records
    uniq = {}
    for k, v in _pool_records(2 * n, 5, common=b"b") + _pool_records(2 * n, 6, common=b"c"):
        uniq.setdefault(k, v)
    recs = sorted(uniq.items())[:n]
    assert len(recs) == n and recs[0][0] > b"a1"
    return recs


def _records_with_giants(model):
    """DeviceRecords for `model` (host records whose giant values are the stand-ins): the value
    bytes are laid out on the device, the giants generated there"""
    import torch
    from mtblx.encode import DeviceRecords
    lens = np.array([GIANT if v in STAND else len(v) for _, v in model], np.int64)
    ve = np.cumsum(lens)
    vals = torch.empty(int(ve[-1]), dtype=torch.uint8, device="cuda")
    run, start = bytearray(), 0
    for (k, v), e in zip(model, ve):
        if v in STAND:
            if run:
                vals[start: start + len(run)].copy_(torch.frombuffer(run, dtype=torch.uint8))
            _fill_giant(vals[int(e) - GIANT: int(e)], 3 + 2 * STAND.index(v))
            run, start = bytearray(), int(e)
        else:
            run += v
    if run:
        vals[start: start + len(run)].copy_(torch.frombuffer(run, dtype=torch.uint8))
    keys = torch.frombuffer(bytearray(b"".join(k for k, _ in model)), dtype=torch.uint8).cuda()
    ke = torch.from_numpy(np.cumsum([len(k) for k, _ in model], dtype=np.int64)).cuda()
    return DeviceRecords(keys, ke, vals, torch.from_numpy(ve).cuda())


@pytest.fixture(scope="module")
def giants(win):
    """source 0: (a0, V0), (a1, V1), then 2000 small records -- every small value lies above the
    line -- and the two giants on their own, for comparisons; sources 1 and 2 are small and share
    a tenth of source 0's keys each, source 2 also holds a1"""
    import torch
    from mtblx.encode import DeviceRecords
    small = _small_pool(2000)
    model0 = [(b"a0", STAND[0]), (b"a1", STAND[1])] + small
    src0 = _records_with_giants(model0)
    ref = [src0.vals[:GIANT], src0.vals[GIANT: 2 * GIANT]]
    keys = [k for k, _ in small]
    m1 = sorted([(k, b"one:" + k[:9]) for k in keys[::10]] + [(b"c%05d" % i, b"1" * (i % 23)) for i in range(300)])
    m2 = sorted([(b"a1", b"the small a1")] + [(k, b"two:" + k[-7:]) for k in keys[5::10]] +
                [(b"b\xff\xff%04d" % i, b"") for i in range(200)])
    yield {"model": [model0, m1, m2], "dev": [src0, DeviceRecords.from_list(m1), DeviceRecords.from_list(m2)], "ref": ref}
    del src0, ref
    torch.cuda.empty_cache()


def _pieces(values):
    """model values -> [(true position, bytes | giant number)], the true END of every value"""
    out, ends, pos = [], [], 0
    for v in values:
        while v:
            cut = min((v.find(s) for s in STAND if s in v), default=-1)
            if cut == 0:
                g = STAND.index(v[:16])
                out.append((pos, g))
                pos, v = pos + GIANT, v[16:]
            else:
                part = v if cut < 0 else v[:cut]
                if out and isinstance(out[-1][1], bytes) and out[-1][0] + len(out[-1][1]) == pos:
                    out[-1] = (out[-1][0], out[-1][1] + part)
                else:
                    out.append((pos, part))
                pos, v = pos + len(part), v[len(part):]
        ends.append(pos)
    return out, np.array(ends, np.int64)


def _check_values(vals, val_end, values, ref):
    """device value bytes against the model: END offsets by exact arithmetic, small bytes on the
    host, the giants on the device against their source slices"""
    import torch
    pieces, ends = _pieces(values)
    assert np.array_equal(val_end.cpu().numpy(), ends)
    assert int(vals.numel()) == (int(ends[-1]) if ends.size else 0)
    for pos, p in pieces:
        if isinstance(p, bytes):
            assert vals[pos: pos + len(p)].cpu().numpy().tobytes() == p, pos
        else:
            assert torch.equal(vals[pos: pos + GIANT], ref[p]), (pos, p)
    return ends


def _check_keys(r, keys):
    assert r.keys.cpu().numpy().tobytes() == b"".join(keys)
    assert np.array_equal(r.key_end.cpu().numpy(), np.cumsum([len(k) for k in keys], dtype=np.int64))


PICK = {"concat": b"".join, "first": lambda vs: vs[0], "last": lambda vs: vs[-1]}


@pytest.mark.parametrize("mode", ["groups", "concat", "first", "last"])
def test_merger_records_above(giants, mode):
    """mtblx_merge_plan / mtblx_merge_emit: source 0's small values start past 2^32 in its value
    buffer, and (but for "last", which drops V1 for source 2's a1) in the merged output too"""
    import torch
    from mtblx import merger
    from test_merger_gpu import promised
    want = promised(giants["model"])
    assert want[1] == (b"a1", [STAND[1], b"the small a1"]) and sum(len(vs) == 2 for _, vs in want) >= 390
    out = merger.merge_records(giants["dev"], mode)
    torch.cuda.synchronize()
    _check_keys(out, [k for k, _ in want])
    if mode == "groups":
        ends = _check_values(out.vals, out.val_end, [v for _, vs in want for v in vs], giants["ref"])
        assert np.array_equal(out.grp_end.cpu().numpy(), np.cumsum([len(vs) for _, vs in want], dtype=np.int64))
    else:
        ends = _check_values(out.vals, out.val_end, [PICK[mode](vs) for _, vs in want], giants["ref"])
    assert ends[2] > LINE or mode == "last"
    del out
    torch.cuda.empty_cache()


@pytest.mark.parametrize("mode", ["groups", "concat"])
def test_sorter_records_above(giants, mode):
    """mtblx_sort_plan / mtblx_sort_emit on 2000 pool records in random order (duplicate keys) with
    the giants at input positions 700 and 1500: inputs after 1500 and every sorted small value lie
    above the line"""
    import torch
    from mtblx import sorter
    from test_sorter_gpu import _pool_records, promised
    model = _pool_records(2000, 11, common=b"b")
    model.insert(700, (b"a0", STAND[0]))
    model.insert(1500, (b"a1", STAND[1]))
    recs = _records_with_giants(model)
    want = promised(model)
    assert [k for k, _ in want[:2]] == [b"a0", b"a1"] and any(len(vs) > 1 for _, vs in want)
    out = sorter.sort_records(recs, mode)
    torch.cuda.synchronize()
    _check_keys(out, [k for k, _ in want])
    if mode == "groups":
        ends = _check_values(out.vals, out.val_end, [v for _, vs in want for v in vs], giants["ref"])
        assert np.array_equal(out.grp_end.cpu().numpy(), np.cumsum([len(vs) for _, vs in want], dtype=np.int64))
    else:
        ends = _check_values(out.vals, out.val_end, [b"".join(vs) for _, vs in want], giants["ref"])
    assert ends[2] > LINE
    del out, recs
    torch.cuda.empty_cache()


def test_reduce_segments_above(giants):
    """mtblx_reduce_segments over 24-byte values that follow the two giants (segments leave the
    giants out; fields with bit 63 set), against the Python fold"""
    import torch
    from mtblx import reduce_segments
    from mtblx.encode import DeviceRecords
    from test_scan_reduce_gpu import _red, _seg_check, _values
    vals = _values(np.random.default_rng(4), 3000, 3)
    assert any(len(v) == 24 and v[23] & 0x80 for v in vals) and any(len(v) != 24 for v in vals)
    src0 = giants["dev"][0]
    blob = torch.frombuffer(bytearray(b"".join(vals)), dtype=torch.uint8).cuda()
    allv = torch.cat([src0.vals[: 2 * GIANT], blob])
    ve = torch.from_numpy(2 * GIANT + np.cumsum([len(v) for v in vals], dtype=np.int64)).cuda()
    ve = torch.cat([src0.val_end[:2], ve])
    rec = DeviceRecords(torch.zeros(0, dtype=torch.uint8, device="cuda"), ve.clone(), allv, ve)
    segs = [(2, 2), (2, 3), (3, 50), (50, 1100), (1100, 1101), (1200, 3002), (3002, 3002)]
    red = _red(3)
    fields, nbad = reduce_segments(rec, [a for a, _ in segs], [b for _, b in segs], red)
    _seg_check(red, [b"", b""] + vals, segs, fields, nbad)
    fields, nbad = reduce_segments(rec, [2], [3002], red)
    _seg_check(red, [b"", b""] + vals, [(2, 3002)], fields, nbad)
    del allv, rec
    torch.cuda.empty_cache()


def _read_varint(h, p):
    v = sh = 0
    while True:
        b = int(h[p])
        v |= (b & 0x7F) << sh
        p, sh = p + 1, sh + 7
        if b < 0x80:
            return v, p


NBIG, BIG = 260, (16 << 20) + 4099      # 260 values of 16 MiB + 4099 B: 4161 MiB, past LINE + 64 MiB


@pytest.fixture(scope="module")
def bigs(win):
    """(a0000, B0) .. (a0259, B259), every B its own 16 MiB + 4099 hashed bytes generated on the device, then
    2000 small records: a Writer puts each B alone in a block, block 255 straddles the line, and
    every later block and every small value lies above it"""
    import torch
    from mtblx.encode import DeviceRecords
    small = _small_pool(2000)
    total = NBIG * BIG
    blob = b"".join(v for _, v in small)
    vals = torch.empty(total + len(blob), dtype=torch.uint8, device="cuda")
    a = torch.arange((total + 3) // 4, dtype=torch.int32, device="cuda")
    a.mul_(-1640531527)                   # a multiplicative hash of the position: no 4 bytes repeat nearby,
    a.bitwise_xor_(a >> 13)               # so the Snappy file is as long as the plain one and crosses the line too
    a.mul_(0x5bd1e995)
    vals[:total].copy_(a.view(torch.uint8)[:total])
    del a
    vals[total:].copy_(torch.frombuffer(bytearray(blob), dtype=torch.uint8))
    bkeys = [b"a%04d" % i for i in range(NBIG)]
    keys = torch.frombuffer(bytearray(b"".join(bkeys + [k for k, _ in small])), dtype=torch.uint8).cuda()
    ke = np.cumsum([5] * NBIG + [len(k) for k, _ in small], dtype=np.int64)
    ve = np.concatenate([BIG * np.arange(1, NBIG + 1, dtype=np.int64),
                         total + np.cumsum([len(v) for _, v in small], dtype=np.int64)])
    yield DeviceRecords(keys, torch.from_numpy(ke).cuda(), vals, torch.from_numpy(ve).cuda()), bkeys, small
    del vals, keys
    torch.cuda.empty_cache()


@pytest.mark.parametrize("comp", [0, 1])
def test_device_writer_above(oracle, bigs, comp):
    """encode.write_file(records, 8192, 16) for a file above 4 GiB: the block cut, the block emit
    and its running file offsets, the Snappy compressor and framing (comp = 1), the index with
    5-byte offsets and the footer.  Only the index, the footer, 16 bytes per big frame and the
    ~100 KB of blocks after the big ones come to the host."""
    import torch
    from mtblx import codec, encode, reader as rd
    recs, bkeys, small = bigs
    file = encode.write_file(recs, 8192, 16, compression=comp)
    torch.cuda.synchronize()
    flen = int(file.numel())
    foot = file[flen - 512:].cpu().numpy().tobytes()
    meta = [int.from_bytes(foot[8 * i: 8 * i + 8], "little") for i in range(9)]
    idx_off = meta[0]
    assert meta[2] == comp and meta[3] == NBIG + len(small)                # compression, count_entries
    assert meta[7] == 5 * NBIG + sum(len(k) for k, _ in small)
    assert meta[8] == NBIG * BIG + sum(len(v) for _, v in small)
    idx = file[idx_off: flen - 512].cpu().numpy().tobytes()
    n, p = _read_varint(idx, 0)
    assert len(idx) == p + 4 + n and int.from_bytes(idx[p: p + 4], "little") == oracle.crc32c(idx[p + 4:])
    assert meta[6] == len(idx)
    st, entries = oracle.decode_block(idx[p + 4:])
    assert st == 0
    offs = [oracle.varint_decode64(v)[0] for _, v in entries]
    assert offs[0] == 0 and offs == sorted(set(offs)) and meta[4] == len(offs) and meta[5] == idx_off
    assert [oracle.varint_encode64(o) for o in offs] == [v for _, v in entries]
    assert flen > LINE + u.TAIL and offs[255] < LINE < offs[256] and all(len(v) == 5 for _, v in entries[256:])
    # the big frames: one block each, length varint, stored checksum (on the device), the value bytes
    heads = _gather(file, offs[:NBIG], [16] * NBIG)
    ln, lead = zip(*(_read_varint(h, 0) for h in heads))
    assert all(o + ld + 4 + n_ == nxt for o, ld, n_, nxt in zip(offs[:NBIG], lead, ln, offs[1: NBIG + 1]))
    gb = codec.DeviceBatch(file, torch.tensor([o + ld + 4 for o, ld in zip(offs[:NBIG], lead)], dtype=torch.int64, device="cuda"),
                           torch.tensor(np.array(ln, np.uint32).view(np.int32), device="cuda"), max(ln))
    _, bad = codec.crc32c_blocks(gb, framed=True)
    assert not bad.cpu().numpy().any()
    if comp == 0:   # the one entry: varints (0, 5, BIG), the key, the value, one restart, the count
        vl = oracle.varint_encode32(BIG)
        assert all(n_ == 2 + len(vl) + 5 + BIG + 8 for n_ in ln)
        for g in range(NBIG):
            assert heads[g][lead[g] + 4:] == (b"\x00\x05" + vl + bkeys[g])[: 12 - lead[g]]
            v0 = offs[g] + lead[g] + 4 + 2 + len(vl) + 5
            assert torch.equal(file[v0: v0 + BIG], recs.vals[g * BIG: (g + 1) * BIG]), g
    # the tail: every block after the big ones, on the host
    t0 = offs[NBIG]
    tail = file[t0: idx_off].cpu().numpy().tobytes()
    assert len(tail) < (1 << 20)
    got, at = [], t0
    for o in offs[NBIG:]:
        assert o == at                                                    # contiguous, ascending
        n, p = _read_varint(tail, o - t0)
        content = tail[p + 4: p + 4 + n]
        assert int.from_bytes(tail[p: p + 4], "little") == oracle.crc32c(content)
        if comp:
            content = oracle.snappy_decompress(content)
            assert content is not None
        st, rs = oracle.decode_block(content)
        assert st == 0 and oracle.build_block(rs, 16) == content          # canonical encoding
        got += rs
        at = t0 + p + 4 + n
    assert at == idx_off and got == small
    seps = [k for k, _ in entries]
    assert seps == sorted(seps) and seps[-1] == small[-1][0]
    # and the device Reader on it: a big value below, across and above the line, three tail keys
    R = rd.Reader(file)
    picks = (3, 255, 258)
    gs, vo, vl_ = (t.cpu().numpy() for t in R.get_batch([bkeys[g] for g in picks]))
    src = R.value_source      # the file, or the blocks the Reader decompressed on the device
    for q, g in enumerate(picks):
        assert gs[q] == 0 and vl_[q] == BIG
        assert torch.equal(src[int(vo[q]): int(vo[q]) + BIG], recs.vals[g * BIG: (g + 1) * BIG]), g
    for k, v in (small[0], small[1000], small[-1]):
        assert R.get(k) == v
    del file, R, gb
    torch.cuda.empty_cache()

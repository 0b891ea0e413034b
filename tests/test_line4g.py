"""The layouts tests/test_line4g_gpu.py places around byte offset 2^32, checked on the CPU with
the oracle: every block at or above the line has, at its offset - 2^32, a decoy the oracle
accepts and whose result differs from the real block's, so a kernel that truncates an offset to
32 bits computes a plausible, wrong answer and the GPU comparison fails.  This file is what
shows that those comparisons can fail."""
import numpy as np
import pytest

import line4g_util as u
from line4g_util import LINE


def _peek(lay, pos, n):
    for p, a in lay.regions:
        if p <= pos and pos + n <= p + a.size:
            return bytes(a[pos - p: pos - p + n])
    raise AssertionError(f"[{pos}, +{n}) is not written by the layout")


@pytest.fixture(scope="module")
def batches(oracle):
    out = {k: (u.decode_batch(oracle, k), 0) for k in u.DECODE_KINDS}
    out["crc"] = (u.crc_batch(oracle, False, big=300_000), 0)
    out["crc_framed"] = (u.crc_batch(oracle, True, big=300_000), 4)
    out["snappy"] = (u.snappy_batch(oracle), 0)
    out["snappy_small"] = (u.snappy_batch(oracle, small=True), 0)
    return out


def _result(oracle, kind, item, lead):
    """the oracle's verdict and every compared field for one block of this kind"""
    c = item[lead:]
    if kind.startswith("crc"):
        if lead:
            assert int.from_bytes(item[:4], "little") == oracle.crc32c(c)
        return True, oracle.crc32c(c)
    if kind.startswith("snappy"):
        x = oracle.snappy_decompress(c)
        return x is not None, x
    st, recs = oracle.decode_block(c)
    return st == 0, recs


KINDS = list(u.DECODE_KINDS) + ["crc", "crc_framed", "snappy", "snappy_small"]


@pytest.mark.parametrize("r", u.STARTS)
@pytest.mark.parametrize("kind", KINDS)
def test_layout(oracle, batches, kind, r):
    (blocks, decoys), lead = batches[kind]
    lay = u.layout(blocks, decoys, np.random.default_rng(r + 5), r, lead)
    n = len(blocks)
    start = lay.off.astype(np.int64) - lead
    end = start + np.array([len(b) for b in blocks])
    # the real bytes are where the directory says, disjoint, inside the window
    order = np.argsort(start, kind="stable")
    assert (start[order][1:] >= end[order][:-1]).all()
    assert end.max() + u.PAD <= u.SIZE
    for i in range(n):
        assert _peek(lay, int(start[i]), len(blocks[i])) == blocks[i]
        assert int(lay.ln[i]) == len(blocks[i]) - lead
    # the start under test: a straddler for r > 0, a block exactly at LINE / LINE + 1 otherwise
    f = lay.first
    assert start[f] == LINE - r
    if r > 0:
        assert start[f] < LINE < end[f] and len(blocks[f]) >= 18
    else:
        assert start[f] in (LINE, LINE + 1)
    high = start >= LINE
    assert np.array_equal(high, lay.high)
    assert high.sum() >= n // 2 and (end <= LINE + (r < 0)).sum() >= n // 5
    # decoys: inside [0, 64 MiB), accepted by the oracle, different in every compared field
    for i in np.nonzero(high)[0]:
        d = decoys[i]
        assert d is not None
        a = int(start[i]) - LINE
        assert int(lay.decoy_off[i]) == a and 0 <= a and a + len(d) <= u.TAIL
        assert _peek(lay, a, len(d)) == d
        ok, res = _result(oracle, kind, d, lead)
        assert ok
        _, real = _result(oracle, kind, blocks[i], lead)
        assert res != real
    if r > 0:   # what an address that wraps at 2^32 reads after the straddler's first r bytes
        d = decoys[f]
        assert _peek(lay, 0, len(d) - r) == d[r:] and d[r:] != blocks[f][r:]
        assert _result(oracle, kind, d, lead)[1] != _result(oracle, kind, blocks[f], lead)[1]
    # the same seed gives the same bytes
    again = u.layout(blocks, decoys, np.random.default_rng(r + 5), r, lead)
    assert np.array_equal(again.off, lay.off)
    assert all(p == q and np.array_equal(a, b) for (p, a), (q, b) in zip(lay.regions, again.regions))


def test_big_crc_block_straddles(oracle, batches):
    (blocks, decoys), lead = batches["crc_framed"]
    big = max(range(len(blocks)), key=lambda i: len(blocks[i]))
    assert len(blocks[big]) > 256 * 1024
    lay = u.layout(blocks, decoys, np.random.default_rng(3), 1, lead, first=big)
    assert lay.off[big] == LINE - 1 + 4     # the stored checksum itself crosses the line
    assert _peek(lay, 0, 3) == decoys[big][1:4]


def test_batches_reach_what_they_name(oracle, batches):
    """the longest block of each decode batch selects the kernel the GPU test names"""
    mx = {k: max(len(b) for b in batches[k][0][0]) for k in u.DECODE_KINDS}
    assert mx["small"] <= 49089 and mx["mutated"] <= 49089       # PipeSmall and its fused twin PipeSmallV
    assert u.PLAN_MAX["small"] < mx["large"] <= u.PLAN_MAX["large"] < mx["tiles"]
    st = {oracle.decode_block(b)[0] for b in batches["mutated"][0][0]}
    assert {0, 1, 2} <= st
    streams = batches["snappy"][0][0]
    outs = [oracle.snappy_decompress(z) for z in streams]
    assert any(x is None for x in outs) and max(len(x) for x in outs if x is not None) > 65 * 1024
    small = batches["snappy_small"][0][0]
    outs = [oracle.snappy_decompress(z) for z in small]
    assert any(x is None for x in outs) and max(len(x) for x in outs if x is not None) == u.SNAPPY_QUAD_OUT
    ratio = [len(x) / len(z) for x, z in zip(outs, small) if x]
    assert sum(q > 2 for q in ratio) >= 8 and sum(q < 2 for q in ratio) >= 8     # both sides of the 2x routing rule


def test_literal_streams(oracle):
    x = bytes(np.random.default_rng(0).integers(0, 256, 70_000, dtype=np.uint8))
    for total in list(range(1, 400)) + [4752, 66_000]:
        z = u.snappy_literals(x, total)
        if total == 2:
            assert z is None
            continue
        y = oracle.snappy_decompress(z)
        assert len(z) == total and y is not None and x.startswith(y)


@pytest.mark.parametrize("r", [1, 4, 7, 100])
def test_spread_file(oracle, r):
    """spread() moves blocks [j, n) to LINE - r and rebuilds the index: every frame is found, byte
    for byte, at the offset the new index gives; the footer points at the new index block"""
    import corpus
    rng = np.random.default_rng(3)
    data = oracle.write_file(corpus.random_records(rng, 1500, 1, 40, 0, 120), 4096, 16)
    frames = u.v2_frames(data)
    j = len(frames) // 2
    (p0, head), (p1, tail), total, disp = u.spread(data, j, r)
    assert p0 == 0 and p1 == LINE - r == frames[j][1] + disp and total == p1 + len(tail)
    piece = lambda pos, n: head[pos: pos + n] if pos < len(head) else tail[pos - p1: pos - p1 + n]   # noqa: E731
    idx_off = int.from_bytes(tail[-512:-504], "little")
    assert idx_off == int.from_bytes(data[-512:-504], "little") + disp
    n, ll = oracle.varint_decode64(piece(idx_off, 10))
    ib = piece(idx_off + ll + 4, n)
    assert int.from_bytes(piece(idx_off + ll, 4), "little") == oracle.crc32c(ib)
    assert int.from_bytes(tail[-512 + 48:-512 + 56], "little") == ll + 4 + n
    st, entries = oracle.decode_block(ib)
    assert st == 0 and len(entries) == len(frames)
    for i, ((sep, val), (sep0, off0, ll0, n0)) in enumerate(zip(entries, frames)):
        off = oracle.varint_decode64(val)[0]
        assert sep == sep0 and off == off0 + (disp if i >= j else 0)
        assert len(val) == (5 if i >= j else len(oracle.varint_encode64(off0)))
        assert piece(off, ll0 + 4 + n0) == data[off0: off0 + ll0 + 4 + n0]
    assert tail[-512 + 8: -512 + 48] == data[-512 + 8: -512 + 48] and tail[-456:] == data[-456:]


def test_u32_lengths_of_2_gib_and_more():
    """block lengths of 2^31 bytes and more, which torch holds as negative int32: the Writer's file
    capacity (encode.stored_file_cap, what _write_file allocates for a Snappy file) and the
    max_blk_len of Encoded.batch() take them as u32.  Summed or compared as signed, a stored block
    above 2 GiB gave a negative capacity, and a batch's max_blk_len came from a shorter block."""
    import torch
    from mtblx import codec, encode
    giant = (1 << 31) + 4099
    ln = np.array([giant, 5, 4000, 0], np.uint32)
    t = torch.from_numpy(ln.view(np.int32).copy())
    assert int(t[0]) < 0
    assert codec.u32_sum(t) == giant + 4005 and codec.u32_max(t) == giant
    assert codec.u32_sum(t[:0]) == 0 and codec.u32_max(t[:0]) == 0
    assert encode.stored_file_cap(t, 1000) == giant + 4005 + 14 * 4 + 1000
    z = torch.zeros(4, dtype=torch.int64)
    e = encode.Encoded(torch.zeros(16, dtype=torch.uint8), z, t, torch.zeros(4, dtype=torch.int32), z[:2])
    b = e.batch()
    assert b.max_blk_len == giant and b.cstruct().max_blk_len == giant

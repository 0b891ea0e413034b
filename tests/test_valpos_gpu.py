"""GPU parity of the positions mode (mtblx_decode_blocks_valpos: k_decode_pipe<PipeSmallP>,
<PipeLargeP>, k_decode_tiles<CfgLargeP>) against the CPU oracle, bit-exact.

Every case compares nrec, status, the three bases, totals[0..2], key_end, val_end and keys with
the oracle's decode of the same bytes, val_pos[:records] with the walker of valpos_util (pinned
against the oracle in tests/test_valpos.py), reads every value through its position, and checks
that a value buffer handed in `out` (pre-filled with 0xA5) is untouched."""
import numpy as np
import pytest

import corpus
import valpos_util as vu

pytestmark = pytest.mark.gpu

SENTINEL = -1   # val_pos pre-fill (0xFFFFFFFF): never a position


def _dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mtblx import codec
    return codec


def _launch(codec, batch, exp, ws=None, caps=None, values=True):
    """one decode_positions_into launch -> (host outputs, val_pos u32 [rec_cap], raw vals tensor)"""
    import torch
    nr = int(exp.nrec.sum())
    rec_cap, keys_cap, vals_cap = caps or (nr, exp.keys.size, exp.vals.size)
    out = codec.DecodedBlocks(batch.nblk, rec_cap, keys_cap, vals_cap, values=values)
    out.vals.fill_(0xA5)
    val_pos = torch.full((max(rec_cap, 1),), SENTINEL, dtype=torch.int32, device="cuda")
    ws = ws or codec.Workspace(batch.nblk)
    codec.decode_positions_into(batch, out, val_pos, ws)
    torch.cuda.synchronize()
    assert bool((out.vals == 0xA5).all()), "the value buffer was written"
    return out.to_host(), val_pos.cpu().numpy().view(np.uint32), out


def _assert_decoded(dev, exp, flags=0):
    assert np.array_equal(dev.status, exp.status), np.nonzero(dev.status != exp.status)[0][:10]
    assert np.array_equal(dev.nrec, exp.nrec), np.nonzero(dev.nrec != exp.nrec)[0][:10]
    assert np.array_equal(dev.rec_base, exp.rec_base)
    assert np.array_equal(dev.key_base, exp.key_base)
    assert np.array_equal(dev.val_base, exp.val_base)
    assert dev.totals == (int(exp.nrec.sum()), exp.keys.size, exp.vals.size, flags)
    assert np.array_equal(dev.key_end, exp.key_end)
    assert np.array_equal(dev.val_end, exp.val_end)
    assert np.array_equal(dev.keys, exp.keys)


def _run(data, off, ln, exp, pos, ws=None, batch=None):
    codec = _dev()
    batch = batch or codec.DeviceBatch.from_host(data, off, ln)
    dev, vp, _ = _launch(codec, batch, exp, ws)
    _assert_decoded(dev, exp)
    nr = int(exp.nrec.sum())
    bad = np.nonzero(vp[:nr] != pos)[0]
    assert bad.size == 0, (bad[:10], vp[bad[:10]], pos[bad[:10]])
    vu.check_positions(data, off, ln, exp, vp[:nr])


def _run_blocks(oracle, blocks, rng=None, lead=0):
    data, off, ln = corpus.pack(blocks, lead=lead, rng=rng)
    exp = oracle.decode_blocks(data, off, ln)
    _run(data, off, ln, exp, vu.walker(oracle, data, off, ln, exp))
    return exp, ln


def test_cfg2_uniform_values(oracle):
    """4 KiB blocks whose values are all 64 B: the (skipped) uniform 16-byte-chunk path of
    copy_emit, on PipeSmallP"""
    _run(*vu.cfg2(oracle, 300))


def test_cfg2_more_tiles_than_workgroups(oracle):
    """4000 blocks = 334 tiles of 12: the persistent loop and the look-back of the new kernel"""
    data, off, ln, exp, pos = vu.cfg2(oracle, 4000)
    assert off.size > 12 * 256
    _run(data, off, ln, exp, pos)


@pytest.mark.parametrize("large", [False, True])
def test_mixed_corpus_every_status(oracle, large):
    """builder + mutated + quirk blocks at unaligned offsets with gaps: every status and the exact
    serial path.  large=False runs PipeSmallP (irregular blocks staged); large=True adds four
    81-235 KB blocks, so the batch runs k_decode_tiles<CfgLargeP> with those read unstaged"""
    data, off, ln, exp, pos = vu.mixed_corpus(oracle, large)
    assert {0, 1, 2, 3} <= set(exp.status.tolist())
    assert (int(ln.max()) > 81_000) == large
    _run(data, off, ln, exp, pos)


@pytest.mark.parametrize("lo,hi,count,mutated", [(49_088, 49_600, 12, 0), (49_700, 65_000, 40, 5)])
def test_size_bands(oracle, lo, hi, count, mutated):
    """(49 088, 49 600]: the upper edge of PipeSmallP (one block per tile, the largest that fits
    its staging); (49 700, 65 000]: PipeLargeP, plus mutated blocks of that size"""
    rng = np.random.default_rng(lo)
    recs = corpus.random_records(rng, 640 + count, 8, 200, 64, 64)
    blocks = []
    for j in range(count):
        target = hi if hi - lo < 600 else int(rng.integers(lo + 300, hi + 1))
        blocks.append(vu.block_in_band(oracle, recs, j, lo, hi, target))
    blocks[-1] = vu.block_in_band(oracle, recs, count, lo, hi, hi)   # the band's upper end
    for j in range(mutated):
        m = corpus.mutate(rng, blocks[3 + 7 * j])
        blocks.append(m if len(m) > lo else blocks[3 + 7 * j][:-5] + b"\x07\0\0\0\0")
    exp, ln = _run_blocks(oracle, blocks, rng=rng, lead=3)
    assert lo < int(ln.max()) <= hi
    assert mutated == 0 or (exp.status != 0).any()


def test_blocks_above_64k_multibyte_headers(oracle):
    """three blocks of 150-300 KB with values of 3000-5000 B (2-byte varint headers) and one
    200-byte block between them: k_decode_tiles<CfgLargeP>"""
    rng = np.random.default_rng(77)
    big = [oracle.build_block(corpus.random_records(rng, n, 8, 40, 3000, 5000)) for n in (42, 55, 68)]
    assert all(150_000 <= len(b) <= 300_000 for b in big), [len(b) for b in big]
    small = oracle.build_block([(b"a" * 20, b"x" * 70), (b"a" * 19 + b"b", b"y" * 95)])
    assert len(small) == 200
    exp, _ = _run_blocks(oracle, [big[0], small, big[1], big[2]], rng=rng, lead=1)
    assert (exp.status == 0).all() and int(exp.nrec.sum()) == 42 + 55 + 68 + 2


def test_edges(oracle):
    rng = np.random.default_rng(5)
    empty_vals = oracle.build_block(corpus.random_records(rng, 100, 4, 30, 0, 0))
    one = oracle.build_block([(b"k", b"v")])
    none = oracle.build_block([])
    keys = sorted({bytes(rng.integers(0, 256, 12, dtype=np.uint8)) for _ in range(40)})
    edge = oracle.build_block([(k, bytes([i & 255]) * (127 + (i & 1))) for i, k in enumerate(keys)])
    for blocks in ([empty_vals], [one], [none], [edge], [empty_vals, one, none, edge, none, one]):
        exp, _ = _run_blocks(oracle, blocks)
        assert (exp.status == 0).all()
    # a position is defined for an empty value too: the byte after the key suffix
    data, off, ln = corpus.pack([empty_vals])
    exp = oracle.decode_blocks(data, off, ln)
    pos = vu.walker(oracle, data, off, ln, exp)
    assert exp.vals.size == 0 and (np.diff(pos.astype(np.int64)) > 0).all()


@pytest.mark.parametrize("short", ["rec", "keys"])
def test_capacity_one_short(oracle, short):
    """rec_cap / keys_cap one short: the same blocks overflow as under decode_into with those
    caps, totals[0..2] stay exact, bit 0 is set, and an overflowing block writes no val_pos"""
    codec = _dev()
    import torch
    data, off, ln, exp, pos = vu.cfg2(oracle, 300)
    nr = int(exp.nrec.sum())
    caps = (nr - 1, exp.keys.size, exp.vals.size) if short == "rec" else (nr, exp.keys.size - 1, exp.vals.size)
    batch = codec.DeviceBatch.from_host(data, off, ln)
    ws = codec.Workspace(batch.nblk)
    plain = codec.DecodedBlocks(batch.nblk, *caps)
    codec.decode_into(batch, plain, ws)
    torch.cuda.synchronize()
    want = plain.status[: batch.nblk].cpu().numpy()
    dev, vp, _ = _launch(codec, batch, exp, ws, caps=caps)
    assert np.array_equal(dev.status, want)
    assert (want == 5).sum() == 1 and want[-1] == 5
    assert dev.totals == (nr, exp.keys.size, exp.vals.size, 1)
    assert np.array_equal(dev.nrec, exp.nrec) and np.array_equal(dev.rec_base, exp.rec_base)
    r_bad = int(exp.rec_base[-1])
    assert np.array_equal(vp[:r_bad], pos[:r_bad])
    assert (vp[r_bad:] == 0xFFFFFFFF).all()


def test_no_value_buffer_never_overflows(oracle):
    """vals = NULL, vals_cap = 0 and the other capacities exact: nothing overflows"""
    codec = _dev()
    data, off, ln, exp, pos = vu.cfg2(oracle, 300)
    batch = codec.DeviceBatch.from_host(data, off, ln)
    nr = int(exp.nrec.sum())
    dev, vp, out = _launch(codec, batch, exp, caps=(nr, exp.keys.size, 0), values=False)
    assert out.cstruct().vals is None and out.cstruct().vals_cap == 0
    _assert_decoded(dev, exp)
    assert np.array_equal(vp[:nr], pos)
    # and the convenience wrapper (count, allocate, decode, flags checked)
    out2, vp2 = codec.decode_positions(batch)
    _assert_decoded(out2.to_host(), exp)
    assert np.array_equal(vp2.cpu().numpy().view(np.uint32), pos)


def test_one_workspace_alternating_modes(oracle):
    """one workspace, four launches, decode_into and decode_positions_into alternating on two
    different batches (different tile counts, different kernels): every launch is right"""
    codec = _dev()
    import torch
    a = vu.cfg2(oracle, 300)
    b = vu.mixed_corpus(oracle, False)
    ba = codec.DeviceBatch.from_host(*a[:3])
    bb = codec.DeviceBatch.from_host(*b[:3])
    ws = codec.Workspace(max(ba.nblk, bb.nblk))
    for batch, c, positions in ((ba, a, False), (bb, b, True), (bb, b, False), (ba, a, True)):
        data, off, ln, exp, pos = c
        if positions:
            _run(data, off, ln, exp, pos, ws=ws, batch=batch)
        else:
            out = codec.DecodedBlocks(batch.nblk, int(exp.nrec.sum()), exp.keys.size, exp.vals.size)
            codec.decode_into(batch, out, ws)
            torch.cuda.synchronize()
            dev = out.to_host()
            _assert_decoded(dev, exp)
            assert np.array_equal(dev.vals, exp.vals)

"""End-to-end host -> device -> host decode with the values left in the file
(mtblx_pipe_decode_valpos, HostPipe.decode_positions), bit-exact against the oracle; the
positions against the walker of valpos_util (pinned in tests/test_valpos.py)."""
import numpy as np
import pytest

import corpus
import valpos_util as vu

pytestmark = pytest.mark.gpu


def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _assert_positions(out, data, off, ln, exp, pos):
    n = exp.nrec.size
    assert np.array_equal(out.status[:n], exp.status)
    assert np.array_equal(out.nrec[:n], exp.nrec)
    assert np.array_equal(out.rec_base[:n], exp.rec_base)
    assert np.array_equal(out.key_base[:n], exp.key_base)
    assert np.array_equal(out.val_base[:n], exp.val_base)
    nr = int(exp.nrec.sum())
    assert tuple(int(x) for x in out.totals[:4]) == (nr, exp.keys.size, exp.vals.size, 0)
    assert np.array_equal(out.key_end[:nr], exp.key_end)
    assert np.array_equal(out.val_end[:nr], exp.val_end)
    assert np.array_equal(out.keys[: exp.keys.size], exp.keys)
    assert np.array_equal(out.val_pos[:nr], pos)
    vu.check_positions(data, off, ln, exp, out.val_pos[:nr])


def _assert_plain(out, exp):
    n, nr = exp.nrec.size, int(exp.nrec.sum())
    assert np.array_equal(out.status[:n], exp.status) and np.array_equal(out.nrec[:n], exp.nrec)
    assert np.array_equal(out.val_base[:n], exp.val_base)
    assert tuple(int(x) for x in out.totals[:4]) == (nr, exp.keys.size, exp.vals.size, 0)
    assert np.array_equal(out.key_end[:nr], exp.key_end) and np.array_equal(out.val_end[:nr], exp.val_end)
    assert np.array_equal(out.keys[: exp.keys.size], exp.keys)
    assert np.array_equal(out.vals[: exp.vals.size], exp.vals)


def _outputs(pipe, off, exp, positions):
    return pipe.HostOutputs(off.size, int(exp.nrec.sum()), exp.keys.size, exp.vals.size, positions=positions)


def _decode_positions(data, off, ln, exp, chunk=1 << 20, max_blocks=1 << 16, pinned_src=False):
    from mtblx import pipe
    p = pipe.HostPipe(chunk_bytes=chunk, max_blocks=max_blocks, threads=8)
    out = _outputs(pipe, off, exp, True)
    out.val_pos[:] = 0xFFFFFFFF
    if pinned_src:
        pipe.register(data)
    try:
        st = p.decode_positions(data, off, ln, out)
        stats = (st.h2d_bytes, st.d2h_bytes, st.block_bytes, st.chunks)
        plain = p.decode(data, off, ln, _outputs(pipe, off, exp, False))   # the same pipe, the other mode
        h2d_plain = plain.h2d_bytes
    finally:
        if pinned_src:
            pipe.unregister(data)
    return out, stats, h2d_plain


def test_pipe_positions_chunkings(oracle):
    """the four chunkings of test_pipe_uncompressed_chunks: same outputs and positions whatever
    the cut (positions are block-relative); the D2H carries 12 B per record (key_end, val_end,
    val_pos), 32 B per block and the key bytes -- no value byte; the H2D is the plain pipe's"""
    _need_gpu()
    data, off, ln, exp, pos = vu.cfg2(oracle, 2000)
    nr = int(exp.nrec.sum())
    seen = []
    for chunk, mb, pinned in ((1 << 20, 1 << 16, False), (256 << 10, 37, False), (300_000, 1000, True),
                              (64 << 20, 1 << 16, True)):
        out, (h2d, d2h, bb, chunks), h2d_plain = _decode_positions(data, off, ln, exp, chunk, mb, pinned)
        _assert_positions(out, data, off, ln, exp, pos)
        assert d2h == exp.keys.size + 12 * nr + 32 * off.size
        assert h2d == h2d_plain and bb == int(ln.sum())
        seen.append((chunks, out.val_pos[:nr].copy(), out.key_end[:nr].copy()))
    assert len({c for c, _, _ in seen}) > 2                      # the cuts really differ
    assert all(np.array_equal(seen[0][1], s[1]) and np.array_equal(seen[0][2], s[2]) for s in seen)
    # values through the positions == records(), for a few blocks
    for b in (0, 1, off.size - 1):
        assert out.records_from(b, data, off) == exp.records(b)


def test_pipe_positions_mixed_and_odd_blocks(oracle):
    """the corpus of test_pipe_mixed_and_odd_blocks: every status, 64 KiB blocks, gaps"""
    _need_gpu()
    rng = np.random.default_rng(3)
    blocks = corpus.builder_blocks(oracle, seed=31, count=150, max_bytes=8000)
    blocks += corpus.mutated_blocks(oracle, seed=32, count=200)
    for _ in range(4):
        recs = corpus.random_records(rng, 600, 8, 200, 64, 64)
        b = oracle.build_block(recs)
        if len(b) < 65000:
            blocks.append(b)
    data, off, ln = corpus.pack(blocks, rng=rng, lead=5)
    exp = oracle.decode_blocks(data, off, ln)
    pos = vu.walker(oracle, data, off, ln, exp)
    out, _, _ = _decode_positions(data, off, ln, exp, chunk=200_000, max_blocks=64)
    _assert_positions(out, data, off, ln, exp, pos)
    for b in range(0, off.size, 17):
        assert out.records_from(b, data, off) == exp.records(b)


def test_pipe_positions_key_expansion_regrows_slot(oracle):
    """the file of test_pipe_key_expansion_regrows_slot (20 000 records, 240-byte shared prefix,
    empty values): the slot's key capacity overflows and the chunk is decoded again -- in
    positions mode"""
    _need_gpu()
    from mtblx.writer import Writer
    base = b"k" * 240
    w = Writer(4096, 16, 0)
    for i in range(20000):
        w.insert(base + i.to_bytes(4, "big"), b"")
    data = np.frombuffer(w.into_inner(), np.uint8).copy()
    off, ln = w.block_dir
    exp = oracle.decode_blocks(data, off, ln)
    assert exp.keys.size > 4 * int(ln.sum()) and exp.vals.size == 0
    pos = vu.walker(oracle, data, off, ln, exp)
    out, _, _ = _decode_positions(data, off, ln, exp, chunk=1 << 20)
    _assert_positions(out, data, off, ln, exp, pos)


def test_pipe_alternating_modes(oracle):
    """one HostPipe, decode and decode_positions alternating on two files (the second has larger
    chunks' worth of records per byte): a slot sized by one mode is re-sized by the other"""
    _need_gpu()
    from mtblx import pipe
    a = vu.cfg2(oracle, 300)
    b = vu.mixed_corpus(oracle, False)
    p = pipe.HostPipe(chunk_bytes=400_000, max_blocks=256, threads=4)
    for (data, off, ln, exp, pos), positions in ((a, False), (b, True), (a, True), (b, False), (a, True)):
        out = _outputs(pipe, off, exp, positions)
        if positions:
            p.decode_positions(data, off, ln, out)
            _assert_positions(out, data, off, ln, exp, pos)
        else:
            p.decode(data, off, ln, out)
            _assert_plain(out, exp)
    with pytest.raises(ValueError):
        p.decode_positions(a[0], a[1], a[2], _outputs(pipe, a[1], a[3], False))

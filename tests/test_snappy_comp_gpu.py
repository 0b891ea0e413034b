"""Device snappy raw compression (include/mtblx.h mtblx_snappy_slots / mtblx_snappy_compress_dev,
csrc/snappy_comp.hip), block level.

Compressed bytes are not pinned to any compressor, so every input is checked by
what the stream must be: status OK, no longer than mtblx_snappy_max_compressed_len, decoded back
to the input by the oracle's byte-at-a-time decoder, by the product's host decoder and by the
device decompressor, and written only inside [dst_off, dst_off + dst_len) of a buffer filled with
0xA5 beforehand.  The inputs are packed at unaligned offsets (corpus.pack, lead=3).  The whole
corpus is compressed ONCE (module fixture) and shared by the tests.

Planted repeats (`_planted`): the cap dst_len < n - L / 2 for L >= 64 holds where the repeat and
its source lie in one 64 KiB fragment.  The stream never matches across a fragment boundary
(include/mtblx.h), so the distance-65535 cases -- whose source is in the first fragment and whose
repeat starts in the second -- are held to every other check but not to the cap.
"""
import numpy as np
import pytest

import corpus

pytestmark = pytest.mark.gpu

ST_OK, ST_OVERFLOW = 0, 5
LS = (4, 11, 12, 63, 64, 65, 67, 68, 69, 128, 1000)


def _mods():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mtblx import _lib, codec, encode, pipe
    return torch, _lib, codec, encode, pipe


def _rand(rng, n):
    return rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()


def _planted(rng, pre, L, at_end=False):
    """`pre` random bytes, a copy of bytes [100, 100 + L) (self-overlapping where 100 + L > pre),
    a byte that differs from the one that would continue the match, 200 random bytes (or, at_end,
    nothing after the copy)"""
    x = bytearray(_rand(rng, pre))
    for i in range(L):
        x.append(x[100 + i])
    if not at_end:
        x.append(x[100 + L] ^ 0xFF)
        x += _rand(rng, 200)
    return bytes(x)


def _inputs():
    """[(name, bytes, planted L or 0 when the cap applies)]"""
    rng = np.random.default_rng(20)
    xs = [(f"len{n}", _rand(rng, n), 0) for n in range(21)]
    xs += [(f"rand{n}", _rand(rng, n), 0) for n in (59, 60, 61, 255, 256, 257, 65535, 65536, 65537, 131077)]
    xs += [("zeros", b"\0" * 4500, 0), ("ab", b"ab" * 2000, 0), ("abcd", b"abcd" * 16000, 0)]
    words = [b"alpha", b"beta", b"gamma", b"delta"]
    xs.append(("words", b"".join(rng.choice(words, 2000).tolist()), 0))
    from mtblx import synth
    xs.append(("cfg1", b"".join(v for _, v in synth.cfg1_records(400)), 0))
    recs = corpus.random_records(rng, 300, 0, 40, 0, 20)
    xs.append(("random_records", b"".join(k + v for k, v in recs), 0))
    for L in LS:
        cap = L if L >= 64 else 0
        xs.append((f"plant{L}", _planted(rng, 1000, L), cap))
        xs.append((f"plant{L}_end", _planted(rng, 1000, L, at_end=True), cap))
        for dist in (2047, 2048):
            xs.append((f"plant{L}_d{dist}", _planted(rng, 100 + dist, L), cap))
        xs.append((f"plant{L}_d65535", _planted(rng, 100 + 65535, L), 0))   # across the fragment cut: no cap
        # the cursor walks random data in steps of 64 positions from 0: the repeat starts at
        # position 63, 0 and 1 of a step (the first matching lane is the last one or the first)
        for pre in (1023, 1024, 1025):
            xs.append((f"plant{L}_w{pre}", _planted(rng, pre, L), cap))
    return xs


def _max_len(L, n):
    return int(L.mtblx_snappy_max_compressed_len(int(n)))


def _compress(xs, dst_off=None, dst_cap=None):
    """-> (dst bytes, dst_off, dst_len, status) of one mtblx_snappy_compress_dev over a 0xA5-filled dst"""
    torch, _lib, codec, encode, pipe = _mods()
    data, off, ln = corpus.pack(xs, align=1, lead=3)
    batch = codec.DeviceBatch.from_host(data, off, ln)
    slots = codec.SnappySlots(batch.nblk)
    codec.snappy_slots(batch, slots)
    torch.cuda.synchronize()
    total = int(slots.totals[0].item())
    L = _lib.lib()
    sizes = np.array([(_max_len(L, len(x)) + 15) & ~15 for x in xs], np.uint64)
    want = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    assert total == int(want[-1])
    assert np.array_equal(slots.dst_off.cpu().numpy().view(np.uint64)[: len(xs)], want[:-1])
    if dst_off is not None:
        slots.dst_off = torch.from_numpy(np.ascontiguousarray(dst_off, np.uint64).view(np.int64)).cuda()
        total = int(dst_cap)
    dst = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
    dst_len = torch.full((len(xs),), -1, dtype=torch.int32, device="cuda")
    status = torch.full((len(xs),), -1, dtype=torch.int32, device="cuda")
    codec.snappy_compress_into(batch, slots, dst, dst_len, status)
    torch.cuda.synchronize()
    return (dst.cpu().numpy(), slots.dst_off.cpu().numpy().view(np.uint64)[: len(xs)],
            dst_len.cpu().numpy().view(np.uint32), status.cpu().numpy())


@pytest.fixture(scope="module")
def corpus_run():
    xs = _inputs()
    return xs, _compress([x for _, x, _ in xs])


def _streams(run):
    dst, off, ln, _ = run
    return [dst[int(a): int(a) + int(n)].tobytes() for a, n in zip(off, ln)]


def test_status_and_bound(corpus_run):
    torch, _lib, codec, encode, pipe = _mods()
    xs, run = corpus_run
    L = _lib.lib()
    assert (run[3] == ST_OK).all(), [xs[i][0] for i in np.nonzero(run[3])[0]]
    for (name, x, _), n in zip(xs, run[2]):
        assert 1 <= int(n) <= _max_len(L, len(x)), name
    assert _streams(run)[0] == b"\x00"   # n == 0: the single byte 0x00


def test_decodes_to_input_oracle_and_host(oracle, corpus_run):
    torch, _lib, codec, encode, pipe = _mods()
    xs, run = corpus_run
    for (name, x, _), z in zip(xs, _streams(run)):
        assert oracle.snappy_decompress(z) == x, name
        assert pipe.snappy_decompress(z) == x, name


def test_decodes_to_input_device(corpus_run):
    torch, _lib, codec, encode, pipe = _mods()
    xs, run = corpus_run
    dst, off, ln, _ = run
    dec, st = codec.snappy_decompress(codec.SnappyBatch.from_host(dst, off, ln))
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all()
    host = dec.data.cpu().numpy()
    o, n = dec.blk_off.cpu().numpy().view(np.uint64), dec.blk_len.cpu().numpy().view(np.uint32)
    for (name, x, _), a, m in zip(xs, o, n):
        assert host[int(a): int(a) + int(m)].tobytes() == x, name


def test_guard_intact_outside_streams(corpus_run):
    xs, run = corpus_run
    dst, off, ln, _ = run
    inside = np.zeros(dst.size, bool)
    for a, n in zip(off, ln):
        inside[int(a): int(a) + int(n)] = True
    assert (dst[~inside] == 0xA5).all()


def test_planted_repeats_are_found(corpus_run):
    """a compressor that misses half of a planted repeat of L >= 64 bytes has a broken match
    finder (the host compressor saves about L - 6)"""
    xs, run = corpus_run
    checked = 0
    for (name, x, L), n in zip(xs, run[2]):
        if L:
            print(name, len(x), int(n))
            assert int(n) < len(x) - L / 2, (name, len(x), int(n))
            checked += 1
    assert checked == 7 * 7   # L in 64 .. 1000, seven placements each


def test_deterministic(corpus_run):
    xs, run = corpus_run
    again = _compress([x for _, x, _ in xs])
    assert np.array_equal(run[2], again[2]) and np.array_equal(run[0], again[0])


def test_codec_snappy_compress_roundtrip(oracle):
    """codec.snappy_compress -> (SnappyBatch, status), the counterpart of codec.snappy_decompress"""
    torch, _lib, codec, encode, pipe = _mods()
    rng = np.random.default_rng(3)
    xs = [b"", b"x", b"abc" * 1500, _rand(rng, 5000), bytes(range(256)) * 17]
    data, off, ln = corpus.pack(xs, align=1, lead=3)
    comp, st = codec.snappy_compress(codec.DeviceBatch.from_host(data, off, ln))
    torch.cuda.synchronize()
    assert isinstance(comp, codec.SnappyBatch) and (st.cpu().numpy() == 0).all()
    host = comp.data.cpu().numpy()
    o, n = comp.src_off.cpu().numpy().view(np.uint64), comp.src_len.cpu().numpy().view(np.uint32)
    assert (o % 16 == 0).all()
    for x, a, m in zip(xs, o, n):
        assert oracle.snappy_decompress(host[int(a): int(a) + int(m)].tobytes()) == x
    dec, dst = codec.snappy_decompress(comp)
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0).all()
    assert dec.blk_len.cpu().numpy().view(np.uint32).tolist() == [len(x) for x in xs]


@pytest.mark.parametrize("victim", [1, 3])
def test_slot_one_byte_too_small(oracle, victim):
    """the block whose slot is one byte short of max_compressed_len gets MTBLX_ST_OVERFLOW and
    nothing written; its neighbours are fine.  victim 3 is the last block: its slot is cut by
    dst_cap."""
    torch, _lib, codec, encode, pipe = _mods()
    rng = np.random.default_rng(9)
    xs = [b"ab" * 700, _rand(rng, 900), b"\0" * 300, _rand(rng, 77)]
    L = _lib.lib()
    sizes = [(_max_len(L, len(x)) + 15) & ~15 for x in xs]
    sizes[victim] = _max_len(L, len(xs[victim])) - 1
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    dst, o, n, st = _compress(xs, dst_off=off[:-1], dst_cap=int(off[-1]))
    assert st.tolist() == [ST_OVERFLOW if i == victim else ST_OK for i in range(4)]
    assert n[victim] == 0
    assert (dst[int(off[victim]): int(off[victim + 1])] == 0xA5).all()
    for i, x in enumerate(xs):
        if i != victim:
            assert oracle.snappy_decompress(dst[int(o[i]): int(o[i]) + int(n[i])].tobytes()) == x


def _ratio_corpora():
    from mtblx import synth
    rng = np.random.default_rng(11)
    vocab = [b"alpha", b"beta", b"gamma", b"delta", b"epsilon", b"zeta"]
    return {
        "cfg1": list(synth.cfg1_records(10000)),
        "constant": [(b"%08d" % i, b"\x5a" * 64) for i in range(5000)],
        "words": [(b"%08d" % i, b" ".join(rng.choice(vocab, 12).tolist())) for i in range(5000)],
    }


@pytest.mark.parametrize("name", ["cfg1", "constant", "words"])
def test_keeps_half_of_the_host_savings(oracle, name):
    """blocks cut by the device Writer at 1024 / 4096 / 65536: the device total is at most the
    midpoint between the host compressor's total and the raw total (a floor against a dead match
    finder, not a target; the measured ratios are in DESIGN.md §4)"""
    torch, _lib, codec, encode, pipe = _mods()
    recs = encode.DeviceRecords.from_list(_ratio_corpora()[name])
    for bs in (1024, 4096, 65536):
        blk = encode.plan(recs, bs, 16)
        e = encode.encode_blocks(recs, blk, 16, framed=False)
        torch.cuda.synchronize()
        comp, st = codec.snappy_compress(e.batch())
        torch.cuda.synchronize()
        assert (st.cpu().numpy() == 0).all()
        raw_h = e.out.cpu().numpy()
        ro, rn = e.blk_off.cpu().numpy().view(np.uint64), e.blk_len.cpu().numpy().view(np.uint32)
        ch = comp.data.cpu().numpy()
        co, cn = comp.src_off.cpu().numpy().view(np.uint64), comp.src_len.cpu().numpy().view(np.uint32)
        raw = host = 0
        for b in range(ro.size):
            x = raw_h[int(ro[b]): int(ro[b]) + int(rn[b])].tobytes()
            raw += len(x)
            host += len(pipe.snappy_compress(x))
            if b % 16 == 0 or ro.size <= 8:
                assert oracle.snappy_decompress(ch[int(co[b]): int(co[b]) + int(cn[b])].tobytes()) == x
        dev = int(cn.sum())
        print(f"{name} bs={bs} blocks={ro.size} raw={raw} host={host} ({host / raw:.3f}) device={dev} "
              f"({dev / raw:.3f}) device/host={dev / host:.3f}")
        assert dev <= (host + raw) / 2, (name, bs, raw, host, dev)


def test_incompressible_blocks_stay_in_bound(oracle):
    """cfg2-style random values: only the max_compressed_len bound applies"""
    torch, _lib, codec, encode, pipe = _mods()
    from mtblx import synth
    data, off, ln = synth.cfg2_file(64)
    comp, st = codec.snappy_compress(codec.DeviceBatch.from_host(data, off, ln))
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all()
    L = _lib.lib()
    host = comp.data.cpu().numpy()
    o, n = comp.src_off.cpu().numpy().view(np.uint64), comp.src_len.cpu().numpy().view(np.uint32)
    for b in range(off.size):
        assert int(n[b]) <= _max_len(L, int(ln[b]))
        x = data[int(off[b]): int(off[b]) + int(ln[b])].tobytes()
        assert oracle.snappy_decompress(host[int(o[b]): int(o[b]) + int(n[b])].tobytes()) == x

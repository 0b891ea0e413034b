"""Placement of small blocks around byte offset 2^32 of one device allocation.

The C ABI carries every position in 64 bits ("Positions are 64-bit").  A
kernel that drops the high word of one still reads or writes inside a buffer that starts at 0, so
nothing faults: it returns the bytes at `offset - 2^32`.  `layout` therefore puts, for every
block at or above the line, a different valid block of the same kind (its decoy) at exactly that
address, and the comparison with the oracle fails instead of passing by luck.

`layout` is plain numpy (tests/test_line4g.py checks it on the CPU); `Window` is the device
side: one uninitialised allocation of LINE + 64 MiB, into which `place` copies the two small
regions a layout consists of.  Every byte a kernel may read -- block bytes, the gaps between
them and 4 KiB on each side of both regions -- is written explicitly.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

LINE = 1 << 32
TAIL = 64 << 20
SIZE = LINE + TAIL
PAD = 4096
RESIDUES = (1, 7, 15, 16, 17)   # the straddling block starts at LINE - r
EXACT = (0, -1)                 # "residues" of the blocks that start at LINE and LINE + 1
STARTS = RESIDUES + EXACT
# A block that covers byte LINE and a block that starts at LINE cannot both be in one buffer
# without sharing bytes, so one layout holds one of the three: the tests run every start.


@dataclass
class Layout:
    off: np.ndarray        # u64 [n]: offset of block i (after its `lead` bytes) in the window
    ln: np.ndarray         # u32 [n]: its length (without the lead)
    first: int             # the block placed at LINE - r
    r: int
    regions: list          # [(position, uint8 array)]: the decoy region at 0, the real one around LINE
    decoy_off: np.ndarray  # u64 [n]: where block i's decoy starts (its lead included); ~0 = none
    high: np.ndarray       # bool [n]: block i starts at or above LINE


def layout(blocks, decoys, rng, r, lead=0, first=None) -> Layout:
    """Positions for `blocks` (bytes each, the first `lead` bytes of every one being framing that
    precedes the offset reported for it) around LINE.

    decoys[i] is None or bytes of the same length as blocks[i].  Blocks without a decoy, and
    about a quarter of the others, are packed just below the block `first` (default: the first
    block with a decoy that is long enough), which starts at LINE - r; the rest follow it with the
    0..8 byte random gaps corpus.pack uses.  Every block at or above LINE has its decoy at its own
    offset - LINE; the straddling block's decoy continues at offset 0 with decoy[r:].
    """
    n = len(blocks)
    assert len(decoys) == n and n >= 4
    for b, d in zip(blocks, decoys):
        assert d is None or (len(d) == len(b) and d != b)
    need = max(r + 1, 18) + lead
    if first is None:
        first = next(i for i in range(n) if decoys[i] is not None and len(blocks[i]) >= need)
    assert decoys[first] is not None and len(blocks[first]) >= need
    forced = [i for i in range(n) if decoys[i] is None]
    free = [i for i in range(n) if decoys[i] is not None and i != first]
    pick = rng.permutation(len(free))[: max(0, n // 4 - len(forced))]
    low = sorted(forced + [free[int(j)] for j in pick])
    lowset = set(low)
    above = [i for i in range(n) if i not in lowset and i != first]

    pos = np.zeros(n, np.int64)
    start0 = LINE - r
    p = start0
    for i in reversed(low):
        p -= len(blocks[i]) + int(rng.integers(0, 9))
        pos[i] = p
    lo = p
    pos[first] = start0
    p = start0 + len(blocks[first])
    for i in above:
        p += int(rng.integers(0, 9))
        pos[i] = p
        p += len(blocks[i])
    hi = p
    assert hi - LINE + PAD <= TAIL and lo - PAD > TAIL

    real = rng.integers(0, 256, hi - lo + 2 * PAD, dtype=np.uint8)
    for i in range(n):
        a = int(pos[i]) - (lo - PAD)
        real[a: a + len(blocks[i])] = np.frombuffer(blocks[i], np.uint8)
    dec = rng.integers(0, 256, hi - LINE + PAD, dtype=np.uint8)
    decoy_off = np.full(n, ~np.uint64(0), np.uint64)
    for i in [first] + above:
        a = int(pos[i]) - LINE
        d = np.frombuffer(decoys[i], np.uint8)
        if a < 0:            # the straddler: only what a wrapped address would read
            d, a = d[-a:], 0
            decoy_off[i] = 0
        else:
            decoy_off[i] = a
        dec[a: a + d.size] = d
    off = (pos + lead).astype(np.uint64)
    ln = np.array([len(b) - lead for b in blocks], np.uint32)
    return Layout(off, ln, first, r, [(0, dec), (lo - PAD, real)], decoy_off, pos >= LINE)


def snappy_literals(x: bytes, total: int):
    """a valid Snappy raw stream of exactly `total` bytes that decompresses to a prefix of x
    (the preamble, then literals of at most 60 bytes with 1-byte tags), or None where no such
    stream exists (total == 2, or x too short)"""
    for n in range(min(len(x), total), -1, -1):
        pre, v = bytearray(), n
        while True:
            pre.append((v & 0x7F) | (0x80 if v >> 7 else 0))
            v >>= 7
            if not v:
                break
        m = total - len(pre) - n          # one tag byte per literal
        if m < 0 or not (n + 59) // 60 <= m <= n:
            continue
        out, at = bytearray(pre), 0
        for k in range(m):                # m - 1 literals of 1 byte or more, the rest evenly
            s = min(60, n - at - (m - 1 - k))
            out += bytes([(s - 1) << 2]) + x[at: at + s]
            at += s
        assert at == n and len(out) == total
        return bytes(out)
    return None


class Window:
    """One uninitialised device allocation [0, LINE + 64 MiB): any offset a kernel truncates to
    32 bits still lies inside it."""

    def __init__(self, device="cuda"):
        import torch
        self.buf = torch.empty(SIZE, dtype=torch.uint8, device=device)

    def write(self, pos: int, data) -> None:
        import torch
        t = torch.from_numpy(np.ascontiguousarray(np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray))
                                                  else data))
        assert 0 <= pos and pos + t.numel() <= SIZE
        self.buf[pos: pos + t.numel()].copy_(t)

    def put(self, lay: Layout):
        """copy a layout's regions in -> (blk_off int64 tensor, blk_len int32 tensor)"""
        import torch
        for pos, data in lay.regions:
            self.write(pos, data)
        dev = self.buf.device
        return (torch.from_numpy(lay.off.view(np.int64).copy()).to(dev),
                torch.from_numpy(lay.ln.view(np.int32).copy()).to(dev))

    def place(self, blocks, decoys, rng, r, lead=0, first=None):
        lay = layout(blocks, decoys, rng, r, lead, first)
        return lay, self.put(lay)


# ---------------- the batches the tests place: (blocks, decoys) per kind ----------------
def filler_block(oracle, rng, length):
    """a valid BlockBuilder block of exactly `length` bytes (a few short keys, the values take
    the rest), or None below 24 bytes: the decoy of a decode block"""
    if length < 24:
        return None
    n = 1 if length < 200 else int(min(40, length // 100))
    keys = [(i * 1000 + int(rng.integers(0, 1000))).to_bytes(4, "big") for i in range(n)]
    base = len(oracle.build_block([(k, b"") for k in keys]))
    if base > length:
        return None
    vl = [(length - base) // n] * n
    for _ in range(8):
        b = oracle.build_block([(k, bytes(rng.integers(0, 256, v, dtype=np.uint8))) for k, v in zip(keys, vl)])
        if len(b) == length:
            return b
        vl[-1] += length - len(b)
        if vl[-1] < 0:
            return None
    return None


# make_plan (csrc/decode.hip): the batch's longest block picks the kernel through fit_plan: a block
# fits a tile of TB staging bytes when (len + 30) / 16 * 16 <= TB - 48.  PipeSmall::TB = 49 664
# (at most PipeSmall::MAXBLK = 16 blocks per tile) takes blocks up to 49 601 B, PipeLarge::TB =
# 65 664 (MAXBLK = 2) up to 65 601 B, anything longer runs k_decode_tiles<CfgLarge>.  The fused
# verify twin PipeSmallV stages 49 152 B, so it takes blocks up to 49 089 B.  The thresholds are
# restated here (the library does not export them); tests/test_decode_gpu.py::test_kernel_choice_edges
# pins the same four lengths.
PLAN_MAX = {"small": 49601, "large": 65601}
DECODE_KINDS = ("small", "large", "tiles", "mutated")


def decode_batch(oracle, kind, seed=0x4711):
    import corpus
    rng = np.random.default_rng(seed)
    if kind == "mutated":
        blocks = corpus.mutated_blocks(oracle, seed=seed, count=200)
    else:
        blocks = corpus.builder_blocks(oracle, seed=seed, count=200, max_bytes=8100)
        lo, hi = {"small": (20000, PLAN_MAX["small"]), "large": (PLAN_MAX["small"] + 1, PLAN_MAX["large"]),
                  "tiles": (PLAN_MAX["large"] + 1, 120000)}[kind]
        longer = []
        while len(longer) < 3:
            n = int(rng.integers(lo // 110, hi // 90 + 1))
            b = oracle.build_block(corpus.random_records(rng, n, 4, 60, 10, 120),
                                   restart_interval=int(rng.choice([1, 16, 16])))
            if lo <= len(b) <= hi:
                longer.append(b)
        for i, b in enumerate(longer):
            blocks.insert(20 + 60 * i, b)
    decoys = [filler_block(oracle, rng, len(b)) for b in blocks]
    return blocks, decoys


def crc_batch(oracle, framed, seed=41, big=0):
    """contents of every length 0..600 in permuted order (tests/test_crc_mfma_gpu.py
    test_every_length), `big` > 0 adding one of that many bytes; framed: every block preceded by
    its stored CRC-32C (lead = 4).  The decoy is other random content, framed with its own CRC."""
    rng = np.random.default_rng(seed)
    lens = [int(i) for i in rng.permutation(601)]
    if big:
        lens.insert(300, big)
    frame = (lambda c: oracle.crc32c(c).to_bytes(4, "little") + c) if framed else (lambda c: c)
    blocks, decoys = [], []
    for n in lens:
        c = bytes(rng.integers(0, 256, n, dtype=np.uint8))
        d = bytes(rng.integers(0, 256, n, dtype=np.uint8))
        blocks.append(frame(c))
        decoys.append(frame(d) if n and oracle.crc32c(d) != oracle.crc32c(c) else None)
    return blocks, decoys


SNAPPY_QUAD_OUT = 4608   # csrc/snappy_dev.hip quad::OUT: the largest output of the batch picks the kernels


def snappy_batch(oracle, seed=2, small=False):
    """compressed streams (the product host compressor over _compressible of
    tests/test_snappy_gpu.py), that file's hand-made encodings and one corrupt stream.
    small=False adds outputs above 65 KiB: the batch's largest output is then above quad::OUT and
    every block runs k_snappy_blocks<Large> (k_snappy_lanes under "lanes").  small=True keeps every
    output at or below quad::OUT, as tests/test_snappy_gpu.py does: k_snappy_quads, and for the
    blocks expanding more than 2x k_snappy_lanes / k_snappy_parse + k_snappy_exec / k_snappy_waves
    under the knobs, with k_snappy_deferred for the stream whose output catches up with its input.
    Decoy: a literal-only stream of the same length over random bytes."""
    from mtblx import pipe
    import test_snappy_gpu as tsg
    rng = np.random.default_rng(seed + small)
    xs = tsg._compressible(rng)
    if small:
        from mtblx import synth
        data, off, ln = synth.cfg2_file(12)
        xs = [x for x in xs if len(x) <= SNAPPY_QUAD_OUT] + [bytes(data[int(a): int(a) + int(n)]) for a, n in zip(off, ln)]
        xs += [b"q" * 4608, b"xyz" * 1536, bytes(rng.integers(0, 256, 4608, dtype=np.uint8))]
        xs += [b"".join(rng.choice([b"alpha", b"beta", b"gamma"], n).tolist())[:4600] for n in (40, 300, 1200)]
        xs += [b"\0" * 100, b"ab" * 50, bytes(range(64)) * 9]
    else:
        xs += [b"xy" * 40_000, bytes(rng.integers(0, 256, 70_000, dtype=np.uint8))]
    xs += [bytes(rng.integers(0, 256, int(n), dtype=np.uint8)) for n in (1, 15, 16, 17, 59, 60, 61, 3000)]
    streams = [pipe.snappy_compress(x) for x in xs]
    lits = bytes(rng.integers(0, 256, 1500, dtype=np.uint8))   # the deferred pass (tests/test_snappy_gpu.py)
    streams.append(tsg._varint(1 + 47 * 64 + 1500) + bytes([0]) + b"A" + tsg._copy2(64, 1) * 47 +
                   b"".join(bytes([0]) + lits[i: i + 1] for i in range(1500)))
    out = bytes(rng.integers(0, 256, 1000, dtype=np.uint8))
    streams.append(tsg._varint(1000) + b"".join(tsg._lit4(out[i: i + 1]) for i in range(1000)))
    streams.append(tsg._varint(3001) + bytes([0]) + b"A" + b"".join(tsg._copy4(1, 1) for _ in range(3000)))
    streams.append(tsg._varint(1 + 47 * 64) + bytes([0]) + b"A" + tsg._copy2(64, 1) * 47)
    bad = bytearray(streams[8])
    bad[len(bad) // 2] ^= 0x40
    bad[0] ^= 0x01
    streams.append(bytes(bad))
    noise = bytes(rng.integers(0, 256, 80_000, dtype=np.uint8))
    decoys = []
    for z in streams:
        d = snappy_literals(noise[int(rng.integers(0, 2000)):], len(z)) if len(z) else None
        decoys.append(d if d != z else None)
    return streams, decoys


# ---------------- a V2 file whose later blocks lie above the line ----------------
def v2_frames(data: bytes):
    """(separator, frame offset, varint length bytes, content length) of every data block of a
    V2 file, from its index"""
    import pyoracle as o
    out = []
    for sep, val in o.index_records(data):
        off, _ = o.varint_decode64(val)
        n, ll = o.varint_decode64(data[off: off + 10])
        out.append((sep, off, ll, n))
    return out


def spread(data: bytes, j: int, r: int, restart_interval=16):
    """Move blocks [j, n) of a compact V2 file up so that block j's frame (varint length | crc |
    content) starts at LINE - r; blocks [0, j) stay.  The index block is rebuilt with the same
    separators and the new offsets (the BlockBuilder the Writer uses for its index, as
    corpus.to_v1 does) and follows the last block, then the footer with the new index offset.
    -> ((0, head bytes), (LINE - r, tail bytes), file length, displacement): the bytes between
    the two pieces belong to no index entry."""
    import pyoracle as o
    data = bytes(data)
    meta = [int.from_bytes(data[len(data) - 512 + 8 * i: len(data) - 504 + 8 * i], "little") for i in range(9)]
    frames = v2_frames(data)
    cut, idx_off = frames[j][1], meta[0]
    disp = LINE - r - cut
    entries = [(sep, o.varint_encode64(off + (disp if i >= j else 0))) for i, (sep, off, _, _) in enumerate(frames)]
    ib = o.build_block(entries, restart_interval)
    index = o.varint_encode64(len(ib)) + o.crc32c(ib).to_bytes(4, "little") + ib
    meta[0], meta[6] = idx_off + disp, len(index)
    footer = b"".join(m.to_bytes(8, "little") for m in meta)
    footer += data[len(data) - 512 + len(footer):]
    tail = data[cut:idx_off] + index + footer
    return (0, data[:cut]), (LINE - r, tail), LINE - r + len(tail), disp

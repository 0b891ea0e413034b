"""Shared by the positions-mode tests (mtblx_decode_blocks_valpos / mtblx_pipe_decode_valpos).

The oracle (pyoracle.decode_blocks) yields the records but not where their values sit in the
block, so `walker` restates decode_entry (src/block.rs:216-238) from the oracle's own primitive
(pyoracle.varint_decode32) for exactly the records the oracle yielded:
    n = u32le(block[-4:]); R = L - 4 * (1 + n); p = u32le(block[R:R+4])      (seek_to_first)
    per record: three 1-byte varints (all header bytes < 128) -> p += 3, else three
    varint_decode32 calls (a consumed length of 0 is the unterminated-varint quirk and legal,
    only -1 is a panic); pos = p + non_shared; p = pos + value_length        (the linear chain)
tests/test_valpos.py pins it against the oracle's values without a GPU.
"""
from __future__ import annotations

import functools

import numpy as np

import corpus


def walk_block(oracle, block: bytes, nrec: int):
    """-> [(pos, value_length)] of the first nrec records of one block"""
    out = []
    if nrec == 0:
        return out
    L = len(block)
    n = int.from_bytes(block[L - 4:], "little")
    R = L - 4 * (1 + n)
    assert 0 <= R <= L - 8, (R, L)
    p = int.from_bytes(block[R:R + 4], "little")
    for _ in range(nrec):
        h = block[p:p + 3]
        if len(h) == 3 and h[0] < 128 and h[1] < 128 and h[2] < 128:
            ns, vl = h[1], h[2]
            p += 3
        else:
            f = []
            for _k in range(3):
                v, used = oracle.varint_decode32(block[p:])
                assert used != -1, "the oracle yielded this record: its header cannot panic"
                f.append(v)
                p += used
            ns, vl = f[1], f[2]
        pos = p + ns
        out.append((pos, vl))
        p = pos + vl
    return out


def walker(oracle, data: np.ndarray, off, ln, exp) -> np.ndarray:
    """val_pos (u32 [records]) of the batch, in the oracle's record order"""
    raw = data.tobytes()
    pos = np.zeros(int(exp.nrec.sum()), np.uint32)
    r = 0
    for b in range(len(off)):
        o, n = int(off[b]), int(ln[b])
        for q, _ in walk_block(oracle, raw[o:o + n], int(exp.nrec[b])):
            pos[r] = q
            r += 1
    assert r == pos.size
    return pos


def check_positions(data: np.ndarray, off, ln, exp, pos) -> None:
    """every value read through its position is the oracle's value and ends before the restart
    array's last word (pos + len <= L - 4)"""
    for b in range(len(off)):
        r0, vb, o, L = int(exp.rec_base[b]), int(exp.val_base[b]), int(off[b]), int(ln[b])
        pv = 0
        for i in range(int(exp.nrec[b])):
            ve = int(exp.val_end[r0 + i])
            q, n = int(pos[r0 + i]), ve - pv
            assert q + n <= L - 4, (b, i, q, n, L)
            assert np.array_equal(data[o + q: o + q + n], exp.vals[vb + pv: vb + ve]), (b, i)
            pv = ve


def block_in_band(oracle, recs, start: int, lo: int, hi: int, target: int) -> bytes:
    """a builder block with lo < len <= hi: the longest run recs[start:start+n] of a sorted record
    list that still fits `target` (lo + 300 <= target <= hi: a record adds less than 300 bytes)"""
    a, z = 1, len(recs) - start
    while a < z:   # largest n with len(build(recs[start:start+n])) <= target
        m = (a + z + 1) // 2
        if len(oracle.build_block(recs[start:start + m])) <= target:
            a = m
        else:
            z = m - 1
    b = oracle.build_block(recs[start:start + a])
    assert lo < len(b) <= hi, (len(b), lo, hi)
    return b


_cache = {}


def mixed_corpus(oracle, large: bool):
    """builder blocks of every shape, mutated blocks (every status), the golden quirk blocks and,
    with large=True, four builder blocks of 81-235 KB (which send the whole batch to the tiled
    fallback kernel, the small blocks staged and the large ones not); packed at unaligned offsets
    with gaps.  -> (data, off, ln, oracle decode, walker positions), computed once"""
    if large not in _cache:
        blocks = corpus.builder_blocks(oracle, seed=31, count=200, max_bytes=8000)
        blocks += corpus.mutated_blocks(oracle, seed=32, count=600)
        blocks += [b for _, b, _ in corpus.quirk_blocks()]
        if large:
            rng = np.random.default_rng(33)
            for n in (610, 950, 1300, 1690):
                blocks.append(oracle.build_block(corpus.random_records(rng, n, 8, 200, 64, 64)))
            assert all(81_000 <= len(b) <= 235_000 for b in blocks[-4:]), [len(b) for b in blocks[-4:]]
        data, off, ln = corpus.pack(blocks, lead=5, rng=np.random.default_rng(34))
        exp = oracle.decode_blocks(data, off, ln)
        _cache[large] = (data, off, ln, exp, walker(oracle, data, off, ln, exp))
    return _cache[large]


@functools.lru_cache(maxsize=None)
def _cfg2(nblk: int):
    from mtblx import synth
    return synth.cfg2_file(nblk)


def cfg2(oracle, nblk: int):
    key = ("cfg2", nblk)
    if key not in _cache:
        data, off, ln = _cfg2(nblk)
        exp = oracle.decode_blocks(data, off, ln)
        _cache[key] = (data, off, ln, exp, walker(oracle, data, off, ln, exp))
    return _cache[key]

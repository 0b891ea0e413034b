"""Varint-coded values in the reduce family, the part that needs no GPU: the spec object, Reduce.host /
Reduce.fold against hand-computed vectors and against pyoracle's varint coder (src/varint.rs
restated in C), every shape of bad value, and the C ABI's argument checks for MTBLX_REDUCE_VARINT
(include/mtblx.h "Varint-coded values")."""
import ctypes as C

import numpy as np
import pytest

M = (1 << 64) - 1


def enc(*xs):
    """the canonical bytes, written out by hand: never the library's coder"""
    out = bytearray()
    for x in xs:
        while x >= 128:
            out.append((x & 127) | 128)
            x >>= 7
        out.append(x)
    return bytes(out)


def V(*ops):
    import mtblx
    return mtblx.Reduce(*ops, encoding="varint")


# ---------------------------------------------------------------- the spec
def test_spec_object():
    import mtblx
    with pytest.raises(ValueError):
        mtblx.Reduce("sum", encoding="leb128")
    with pytest.raises(ValueError):
        mtblx.Reduce("sum", encoding=None)
    a, b, c = mtblx.Reduce("sum", "min"), mtblx.Reduce("sum", "min", encoding="varint"), V("sum", "min")
    assert a != b and b == c and hash(b) == hash(c) and len({a, b, c}) == 2
    assert a == mtblx.Reduce("sum", "min", encoding="u64le") and hash(a) == hash(mtblx.Reduce("sum", "min", encoding="u64le"))
    assert a.encoding == "u64le" and b.encoding == "varint"
    assert a.width == 16 and b.width is None
    assert "varint" in repr(b) and "varint" not in repr(a) and eval(repr(b), {"Reduce": mtblx.Reduce}) == b
    assert b.identities() == (0, M)
    with pytest.raises(ValueError):
        mtblx.Reduce(encoding="varint")
    with pytest.raises(ValueError):
        mtblx.Reduce(*["sum"] * 9, encoding="varint")


def test_cstruct_carries_the_flag_on_every_op():
    from mtblx import _lib
    assert _lib.REDUCE_VARINT == 0x10
    s = V("sum", "min", "max").cstruct()
    assert s.nfields == 3 and list(s.op)[:3] == [0x10, 0x11, 0x12] and C.sizeof(s) == 12
    import mtblx
    assert list(mtblx.Reduce("sum", "min", "max").cstruct().op)[:3] == [0, 1, 2]


# ---------------------------------------------------------------- host / fold: hand-computed vectors
def test_host_results_longer_and_shorter_than_the_first_value():
    assert V("sum").host(b"k", [b"\x7f", b"\x01"]) == b"\x80\x01"          # 127 + 1: one byte in, two out
    assert V("sum").host(b"k", [b"\xff" * 9 + b"\x01", b"\x01"]) == b"\x00"   # (2^64 - 1) + 1 wraps: ten in, one out
    assert V("sum").host(b"k", [enc(M), enc(M), enc(3)]) == enc(1)
    assert V("sum", "min", "max").host(b"k", [enc(1, 100, 100), enc(1, 90, 250), enc(M, 95, 120)]) == enc(1, 90, 250)


@pytest.mark.parametrize("k", range(1, 10))
def test_min_max_at_every_length_boundary(k):
    lo, hi = (1 << (7 * k)) - 1, 1 << (7 * k)
    assert len(enc(lo)) == k and len(enc(hi)) == k + 1
    assert enc(lo) == b"\xff" * (k - 1) + b"\x7f" and enc(hi) == b"\x80" * k + b"\x01"
    for vals in ([enc(lo), enc(hi)], [enc(hi), enc(lo)]):
        assert V("min").host(b"", vals) == enc(lo)
        assert V("max").host(b"", vals) == enc(hi)
        assert V("sum").host(b"", vals) == enc(lo + hi)
    assert V("min", "max").fold([enc(lo, lo), enc(hi, hi), enc(hi, lo)]) == ((lo, hi), 3, 0)


def test_unsigned_compare_at_the_top_bit():
    top = 1 << 63
    assert V("min").host(b"", [enc(top), enc(5), enc(top + 9)]) == enc(5)
    assert V("max").host(b"", [enc(top), enc(5), enc(top + 9)]) == enc(top + 9)
    assert V("max").host(b"", [enc(M), enc(top)]) == enc(M) == b"\xff" * 9 + b"\x01"


def test_non_canonical_in_canonical_out():
    assert V("sum").host(b"", [b"\x80\x00", b"\x81\x80\x80\x00"]) == b"\x01"
    assert V("max").host(b"", [b"\x85\x00", b"\x03"]) == b"\x05"
    assert V("sum").fold([b"\x80\x00", b"\x82\x00"]) == ((2,), 2, 0)
    assert V("min", "sum").host(b"", [b"\x80\x80\x00\x01", b"\x07\x80\x00"]) == b"\x00\x01"


def test_tenth_byte_high_bits_are_dropped_as_the_oracle_reads_them(oracle):
    ten = b"\x80" * 9 + b"\x7f"
    val, used = oracle.varint_decode64(ten)
    assert (val, used) == (1 << 63, 10)                      # bit 0 of the tenth byte is bit 63; the rest falls off
    assert V("sum").fold([ten]) == ((1 << 63,), 1, 0)
    assert V("sum").host(b"", [ten, ten]) == b"\x00"         # 2^63 + 2^63 wraps
    assert V("max").host(b"", [ten, b"\x01"]) == enc(1 << 63) == b"\x80" * 9 + b"\x01"
    full = b"\xff" * 9 + b"\x7f"
    assert oracle.varint_decode64(full) == (M, 10) and V("min").fold([full]) == ((M,), 1, 0)


def test_decoder_agrees_with_the_oracle_on_random_bytes(oracle):
    """one field: Reduce.fold sees a value as good iff the oracle's decoder consumes all of it"""
    rng = np.random.default_rng(5)
    r = V("sum")
    for _ in range(3000):
        n = int(rng.integers(1, 13))
        d = bytes(int(x) for x in rng.choice([0x80, 0xff, 0x7f, 0x00, 0x01, int(rng.integers(256))], size=n))
        val, used = oracle.varint_decode64(d)
        if used == n:
            assert r.fold([d]) == ((val,), 1, 0), d
            assert r.host(b"", [d, b"\x00"]) == oracle.varint_encode64(val) == enc(val)
        else:
            assert r.fold([d]) == ((0,), 1, 1), d


# ---------------------------------------------------------------- every bad shape
BAD = {
    "empty": (2, b""),
    "unterminated": (1, b"\x80\x80"),
    "unterminated_second_field": (2, b"\x01\xff"),
    "too_few_fields": (3, b"\x01\x02"),
    "trailing_byte": (2, b"\x01\x02\x03"),
    "eleventh_continuation": (1, b"\x80" * 10 + b"\x01"),
    "ten_continuations": (1, b"\xff" * 10),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_shapes(case):
    import mtblx
    nf, bad = BAD[case]
    r = V(*["sum"] * nf)
    good = enc(*range(1, nf + 1))
    for vals in ([bad, good], [good, bad], [good, good, bad]):
        with pytest.raises(mtblx.MergeError):
            r.host(b"k", vals)
    assert r.fold([bad]) == ((0,) * nf, 1, 1)
    assert r.fold([good, bad, good, bad]) == (tuple(2 * x for x in range(1, nf + 1)), 4, 2)
    assert r.decode(bad) is None and r.decode(good) == list(range(1, nf + 1))


def test_value_bytes_is_the_varint_encoding():
    """ReduceBatch.value_bytes over host arrays (nothing here touches a device)"""
    import torch
    from mtblx import ReduceBatch
    fields = torch.tensor([[127 + 1, -1], [0, 0], [5, 300]], dtype=torch.int64)    # -1: the bit pattern of 2^64 - 1
    nrec, nbad = torch.tensor([2, 1, 3]), torch.tensor([0, 1, 1])
    rb = ReduceBatch(V("sum", "max"), fields, nrec, nbad, torch.zeros(3, dtype=torch.int32), {}, 0, 0, None)
    assert rb.value_bytes(0) == b"\x80\x01" + b"\xff" * 9 + b"\x01"
    assert rb.value_bytes(1) is None
    assert rb.value_bytes(2) == b"\x05\xac\x02"
    import mtblx
    with pytest.raises(mtblx.MergeError, match="2 varints"):
        rb.check()


# ---------------------------------------------------------------- the C ABI, without a device
def _spec(_lib, ops):
    s = _lib.ReduceSpec()
    s.nfields = len(ops)
    for f, op in enumerate(ops):
        s.op[f] = op
    return s


def test_abi_unchanged(mtblx_lib):
    from mtblx import _lib
    assert mtblx_lib.mtblx_abi_version() == 3
    assert C.sizeof(_lib.ReduceSpec) == 12


MIXED = [(0x10, 0x01), (0x00, 0x11, 0x12), (0x10,) * 7 + (0x00,), (0x13,), (0x10, 0x13), (0x30,), (0x90,), (0x14,)]


def test_five_entry_points_refuse_a_mixed_or_unknown_spec(mtblx_lib):
    """MTBLX_E_INVAL before any HIP call: no address handed in is device memory, and no call that got
    as far as the device would return on a machine without one"""
    from mtblx import _lib
    L, E = mtblx_lib, _lib.MTBLX_E_INVAL
    host = np.zeros(1 << 16, np.uint8)
    wp = (host.ctypes.data + 255) & ~255
    wsb = (1 << 16) - 256
    p = C.c_void_p(wp)
    flags = C.c_uint32(0x5A5A)
    out = _lib.Merged(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, C.addressof(flags))
    rec = _lib.Records(0, 0, 0, 0, 0)
    off = (C.c_void_p * 1)(wp)
    ty = np.ascontiguousarray([2], np.int32)
    assert wsb >= L.mtblx_sort_workspace_bytes(0) and wsb >= L.mtblx_merge_workspace_bytes(0, 1)
    assert wsb >= L.mtblx_merge_seg_workspace_bytes(0, 1, 1) and wsb >= L.mtblx_scan_workspace_bytes(1)
    for ops in MIXED:
        s = C.byref(_spec(_lib, ops))
        assert L.mtblx_merge_emit_reduce(C.byref(rec), 1, s, C.byref(out), p, wsb, None) == E, ops
        assert L.mtblx_sort_emit_reduce(C.byref(rec), s, C.byref(out), p, wsb, None) == E, ops
        assert L.mtblx_merge_seg_emit_reduce(C.byref(rec), off, 1, 1, s, C.byref(out), p, wsb, None) == E, ops
        tot = (C.c_uint64 * 4)()
        assert L.mtblx_scan_reduce(p, 1000, 1, 0, 0, 100, None, None, None, None, 0, None, C.c_void_p(ty.ctypes.data),
                                   p, p, p, p, None, 64, 1, p, tot, p, wsb, s, p, p, None) == E, ops
        assert L.mtblx_reduce_segments(C.byref(_lib.Records(0, 0, wp, wp, 4)), p, p, 1, s, p, p, p, None) == E, ops
    assert flags.value == 0x5A5A and not host.any()
    # a well-formed varint spec passes the spec check: with nothing to do the calls that may return do
    good = C.byref(_spec(_lib, (0x10, 0x11, 0x12)))
    tot = (C.c_uint64 * 4)(7, 7, 7, 7)
    assert L.mtblx_scan_reduce(p, 1000, 1, 0, 0, 100, None, None, None, None, 0, None, C.c_void_p(ty.ctypes.data),
                               p, p, p, p, None, 64, 0, p, tot, p, wsb, good, p, p, None) == _lib.MTBLX_OK
    assert list(tot) == [0, 0, 0, 0]
    assert L.mtblx_reduce_segments(C.byref(_lib.Records(0, 0, wp, wp, 4)), None, None, 0, good, p, p, p, None) == _lib.MTBLX_OK
    # and still meets everything else the calls refuse
    assert L.mtblx_sort_emit_reduce(C.byref(rec), good, None, p, wsb, None) == E
    assert L.mtblx_merge_emit_reduce(C.byref(rec), 65, good, C.byref(out), p, wsb, None) == E


def test_workspace_reports_the_per_tile_sums(mtblx_lib):
    """the varint emit scans val_end with one u64 per tile of 1024 records: the three workspace sizes
    count it on top of the edge records"""
    n = 1_000_000
    tiles = (n + 1023) // 1024
    per_record = 16 + 16 + 1 + 4 + 4 + 8 * 4
    for size in (mtblx_lib.mtblx_sort_workspace_bytes(n), mtblx_lib.mtblx_merge_workspace_bytes(n, 3),
                 mtblx_lib.mtblx_merge_seg_workspace_bytes(n, 3, 0)):
        assert size >= per_record * n + (48 + 144 + 8) * tiles
        assert size < per_record * n + (48 + 144 + 8) * tiles + 16 * 256   # and no per-record array came with it

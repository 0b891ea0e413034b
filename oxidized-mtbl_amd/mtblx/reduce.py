"""Device merge functions: u64 sum / min / max over fixed-width or varint-coded fields
(include/mtblx.h "Device merge functions", csrc/reduce_dev.h).

    Reduce("sum")                    one little-endian u64 per value, added mod 2^64
    Reduce("sum", "min", "max")      24-byte values: (count, time_first, time_last)
    Reduce("sum", "min", "max", encoding="varint")
                                     the same record as three LEB128 varints back to back, the
                                     convention of the mtbl ecosystem: decode, reduce, re-encode
    "sum_u64" | "min_u64" | "max_u64"   shorthands for one field

A Reduce is accepted wherever the Merger and the Sorter accept "concat": the groups are then reduced
on the device (mtblx_merge_emit_reduce / mtblx_sort_emit_reduce) and no record returns to the host.
It is not callable on purpose: a callable merge function is the host path.  ``Reduce.host`` is the
same function on the host, for documentation and A/B runs.

Aggregating scans (include/mtblx.h "Aggregating scans") fold the same spec over all the records a
query matches: ``Reduce.fold`` is their definition on the host, ``reduce_segments`` the device
primitive, ``ReduceBatch`` the result of Reader.reduce_batch / Merger.reduce_batch.

As the reference never calls its merge function for a group of one (src/merger.rs:200-201,
src/sorter.rs:166-167), a value alone in its group comes out unchanged whatever its length; in a
group of two or more every value must be exactly 8 * nfields bytes long, else MergeError.

With encoding="varint" a value is well-formed iff it is exactly nfields varints back to back as the
reference's varint_decode64 (src/varint.rs:78-97) reads them: at most 10 bytes looked at per field, a
field without a terminator among them (or before the value's end) is an error, as is an empty rest
or a byte left over; non-canonical encodings are accepted and what a tenth byte holds above 2^64 is
dropped.  The result is the reduced fields encoded canonically (varint_encode64), as long as they
need: longer or shorter than any input.  Every other value is "bad": MergeError in a group of two
or more, counted and left out by the aggregating scans.
"""
from __future__ import annotations

OPS = {"sum": 0, "min": 1, "max": 2}          # MTBLX_REDUCE_SUM / _MIN / _MAX
ENCODINGS = {"u64le": 0, "varint": 0x10}       # OR-ed into every op: MTBLX_REDUCE_VARINT
MAX_FIELDS = 8                                 # MTBLX_REDUCE_MAX_FIELDS
SHORTHANDS = {"sum_u64": "sum", "min_u64": "min", "max_u64": "max"}
_MASK = (1 << 64) - 1


class MergeError(RuntimeError):
    """the merge function failed (the reference's Error::Merge): a group of two or more holds a
    value that is not 8 * nfields bytes long, or with encoding="varint" not nfields varints back to
    back (MTBLX_MERGE_BADVALUE)"""


def varint_encode(x: int) -> bytes:
    """varint_encode64 (src/varint.rs:64-76): the canonical LEB128 bytes of a u64"""
    out = bytearray()
    while x >= 128:
        out.append((x & 127) | 128)
        x >>= 7
    out.append(x)
    return bytes(out)


def varint_decode(data: bytes):
    """varint_decode64 (src/varint.rs:78-97) on a non-empty slice -> (value, consumed); consumed == 0:
    no terminator within the first 10 bytes (or before the slice's end)"""
    x = 0
    for j, b in enumerate(data[:10]):
        x |= (b & 127) << (7 * j)
        if not b & 128:
            return x & _MASK, j + 1
    return 0, 0


def varint_fields(value: bytes, nfields: int):
    """the fields of a well-formed varint-coded value, else None"""
    out, p = [], 0
    for _ in range(nfields):
        if p >= len(value):
            return None          # an empty rest: the reference would panic
        x, k = varint_decode(value[p:])
        if k == 0:
            return None
        out.append(x)
        p += k
    return out if p == len(value) else None


class Reduce:
    """1 to 8 unsigned 64-bit fields, each with one op: "sum" | "min" | "max".  encoding: "u64le" (8
    little-endian bytes per field) or "varint" (one LEB128 varint per field)"""

    def __init__(self, *ops: str, encoding: str = "u64le"):
        if encoding not in ENCODINGS:
            raise ValueError(f"Reduce encoding: {encoding!r} (one of 'u64le', 'varint')")
        self.encoding = encoding
        if not 1 <= len(ops) <= MAX_FIELDS:
            raise ValueError(f"Reduce takes 1 to {MAX_FIELDS} ops, not {len(ops)}")
        for op in ops:
            if op not in OPS:
                raise ValueError(f"Reduce op: {op!r} (one of 'sum', 'min', 'max')")
        self.ops = tuple(ops)

    @property
    def varint(self) -> bool:
        return self.encoding == "varint"

    @property
    def width(self):
        """the bytes of a value: 8 per field; None for varint-coded values, which have no one width"""
        return None if self.varint else 8 * len(self.ops)

    @property
    def shape(self) -> str:
        """what a value must be, for the error texts"""
        if self.varint:
            return f"{len(self.ops)} varints back to back"
        return f"{self.width} bytes long"

    def __repr__(self):
        enc = ", encoding='varint'" if self.varint else ""
        return "Reduce(" + ", ".join(repr(o) for o in self.ops) + enc + ")"

    def __eq__(self, other):
        return isinstance(other, Reduce) and other.ops == self.ops and other.encoding == self.encoding

    def __hash__(self):
        return hash((self.ops, self.encoding))

    def decode(self, value):
        """the fields of one value as unsigned ints, or None if the value is bad"""
        if self.varint:
            return varint_fields(value, len(self.ops))
        if len(value) != self.width:
            return None
        return [int.from_bytes(value[8 * f: 8 * f + 8], "little") for f in range(len(self.ops))]

    def encode(self, fields) -> bytes:
        """the value that holds these fields (varint: canonical)"""
        if self.varint:
            return b"".join(varint_encode(int(x)) for x in fields)
        return b"".join(int(x).to_bytes(8, "little") for x in fields)

    def cstruct(self):
        """the mtblx_reduce of this spec"""
        from . import _lib
        r = _lib.ReduceSpec()
        r.nfields = len(self.ops)
        for f, op in enumerate(self.ops):
            r.op[f] = OPS[op] | ENCODINGS[self.encoding]
        return r

    def host(self, key, values) -> bytes:
        """the same merge function on the host, as a callable(key, values) -> bytes would be given"""
        rows = []
        for v in values:
            row = self.decode(v)
            if row is None:
                raise MergeError(f"merge: a value of {len(v)} bytes in a group of {len(values)} is not "
                                 f"{self.shape}")
            rows.append(row)
        out = []
        for f, op in enumerate(self.ops):
            xs = [row[f] for row in rows]
            out.append(sum(xs) & _MASK if op == "sum" else min(xs) if op == "min" else max(xs))
        return self.encode(out)

    def identities(self):
        """what a field is over nothing: 0 for "sum" and "max", 2^64 - 1 for "min" """
        return tuple(_MASK if op == "min" else 0 for op in self.ops)

    def fold(self, values):
        """The aggregating scans' semantics on the host: -> (fields, nrec, nbad).  nrec = len(values);
        nbad = the values that are not exactly `width` bytes long (varint: not well-formed), left out and
        counted; fields[f] =
        op[f] over field f of the others (unsigned, "sum" mod 2^64), the op's identity over nothing."""
        acc = list(self.identities())
        nrec = nbad = 0
        for v in values:
            nrec += 1
            row = self.decode(v)
            if row is None:
                nbad += 1
                continue
            for f, op in enumerate(self.ops):
                x = row[f]
                acc[f] = (acc[f] + x) & _MASK if op == "sum" else min(acc[f], x) if op == "min" else max(acc[f], x)
        return tuple(acc), nrec, nbad


def as_reduce(merge):
    """a Reduce or one of its shorthand names -> the Reduce; anything else -> None"""
    if isinstance(merge, Reduce):
        return merge
    if isinstance(merge, str) and merge in SHORTHANDS:
        return Reduce(SHORTHANDS[merge])
    return None


def check_merge(merge):
    """what the builders accept: a built-in name, a Reduce (shorthands become one), a callable"""
    r = as_reduce(merge)
    if r is not None:
        return r
    if not callable(merge) and merge not in ("concat", "first", "last"):
        raise ValueError(f"merge: {merge!r}")
    return merge


def reduce_segments(records, seg_lo, seg_hi, reduce, stream=None):
    """mtblx_reduce_segments: `reduce` folded over segments of device records.  `records`: an
    encode.DeviceRecords (only vals / val_end are read); segment s = records [seg_lo[s], seg_hi[s])
    (device int64 [nseg], or anything torch.as_tensor takes), with seg_lo[s] <= seg_hi[s] <=
    seg_lo[s + 1] and seg_hi[-1] <= n; records in no segment bring nothing.  -> device (fields int64
    [nseg, F]: the u64 bit patterns, nbad int64 [nseg]); ValueError for a segment array that breaks
    the rule.  Uploads, kernels and the flags' read-back run on `stream` (default: the current one)."""
    import ctypes as C

    import torch

    from . import _lib, codec
    red = as_reduce(reduce)
    if red is None:
        raise ValueError(f"reduce_segments: {reduce!r} is not a Reduce")
    dev = records.val_end.device
    s = codec._stream_of(stream, dev)
    with torch.cuda.stream(s):
        lo = torch.as_tensor(seg_lo, dtype=torch.int64, device=dev).contiguous()
        hi = torch.as_tensor(seg_hi, dtype=torch.int64, device=dev).contiguous()
        if lo.dim() != 1 or lo.shape != hi.shape:
            raise ValueError("reduce_segments: seg_lo and seg_hi must be two 1-d arrays of one length")
        nseg, nf = int(lo.numel()), len(red.ops)
        fields = torch.tensor(_signed(red.identities()), dtype=torch.int64, device=dev).repeat(nseg, 1)
        nbad = torch.zeros(nseg, dtype=torch.int64, device=dev)
        if nseg == 0:
            return fields, nbad
        flags = torch.zeros(2, dtype=torch.int32, device=dev)
        ve = records.val_end.contiguous()
        rec = _lib.Records(0, 0, codec._u(records.vals), codec._u(ve), int(ve.numel()))
        spec = red.cstruct()
        rc = _lib.lib().mtblx_reduce_segments(C.byref(rec), C.c_void_p(lo.data_ptr()), C.c_void_p(hi.data_ptr()), nseg,
                                              C.byref(spec), C.c_void_p(fields.data_ptr()),
                                              C.c_void_p(nbad.data_ptr()), C.c_void_p(flags.data_ptr()),
                                              C.c_void_p(codec._stream_handle(s)))
        if rc != 0:
            raise RuntimeError(f"mtblx_reduce_segments failed: {rc}")
        fl = int(flags[0].item())   # on s, behind the kernels
    if fl & _lib.REDUCE_BADSEG:
        raise ValueError("reduce_segments: the segments must satisfy seg_lo[s] <= seg_hi[s] <= seg_lo[s + 1] "
                         "and seg_hi[-1] <= n")
    return fields, nbad


def _signed(xs):
    """u64 values as the int64 bit patterns the device tensors hold"""
    return [x - (1 << 64) if x >> 63 else x for x in xs]


class ReduceBatch:
    """Reader.reduce_batch's / Merger.reduce_batch's result.  Device tensors: `fields` int64 [nq, F]
    (the u64 bit patterns), `nrec` / `nbad` int64 [nq] (records yielded; those among them whose value
    is not 8 * F bytes long -- with a varint Reduce: not F varints --, left out and counted), `status` int32 [nq] (SCAN_* of the scan walk).
    A query the walk handed back (SCAN_LARGE, SCAN_FALLBACK, an irregular index) was answered by the
    seek path and its device records reduced by reduce_segments (with a `where`: filtered first, and
    `nmatch` int64 [nq] counts the values the predicate kept): values(q) / value_bytes(q) give every
    query's result, whichever path served it, and end(q) / err(q) how such a query's iteration ended
    (Scan.end / Scan.err; END_NONE for a kernel-served query)."""

    def __init__(self, reduce, fields, nrec, nbad, status, ends, n_large, n_fallback, stream=None, nmatch=None):
        self._stream = stream      # the stream of the batch: every host read goes through it
        self.reduce = reduce
        self.nmatch = nmatch       # reduce_batch(where=): int64 [nq], the values the predicate kept; else None
        self.nq = int(nrec.numel())
        self.fields, self.nrec, self.nbad, self.status = fields, nrec, nbad, status
        self._ends = ends          # q -> (end, err) of the queries the seek path answered
        self.n_large, self.n_fallback = n_large, n_fallback
        self._host = None

    def served_by_kernel(self, q: int) -> bool:
        return q not in self._ends

    def end(self, q: int) -> int:
        return self._ends[q][0] if q in self._ends else 0   # reader.END_NONE

    def err(self, q: int) -> str:
        return self._ends[q][1] if q in self._ends else "None"

    def _h(self):
        if self._host is None:
            import torch
            with torch.cuda.stream(self._stream):   # one read-back, on the batch's stream
                self._host = (self.fields.cpu().numpy().view("uint64"), self.nrec.cpu().numpy(),
                              self.nbad.cpu().numpy())
        return self._host

    def values(self, q: int):
        """query q's fields as a tuple of unsigned ints"""
        return tuple(int(x) for x in self._h()[0][q])

    def counts(self, q: int):
        """(nrec, nbad) of query q"""
        _, nr, nb = self._h()
        return int(nr[q]), int(nb[q])

    def value_bytes(self, q: int):
        """query q's fields as a value of the spec's encoding (8 * F bytes, or F canonical varints), or
        None when nothing was reduced"""
        f, nr, nb = self._h()
        if int(nr[q]) - int(nb[q]) == 0:
            return None
        return self.reduce.encode(f[q])

    def check(self) -> None:
        """MergeError if any query met a bad value (not 8 * F bytes long; varint: not F varints)"""
        nb = self._h()[2]
        if nb.any():
            q = int(nb.nonzero()[0][0])
            raise MergeError(f"reduce_batch: query {q} met {int(nb[q])} values that are not "
                             f"{self.reduce.shape}")

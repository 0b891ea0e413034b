"""Value predicates: device records kept or dropped by the fields of their value
(include/mtblx.h "Value predicates", csrc/where.hip, DESIGN.md §4 "Value predicates").

A Where is a value layout -- exactly a Reduce's: 1 to 8 unsigned 64-bit fields, "u64le" or "varint" --
plus at most one inclusive range per field:

    Where(3, [(1, T, None)])                      time_first >= T        (count, time_first, time_last)
    Where(3, [(0, N, None), (2, T, None)])        count >= N and time_last >= T
    Where(3, [(0, 5, 9, "outside")], mode="any")  count < 5 or count > 9
    Where.like(Reduce("sum", "min", "max", encoding="varint"), [(0, 10, None)])

A value that is not well-formed under the layout is "bad": its record is dropped and counted, never
kept and never an error.  ``Where.keeps`` is the definition on the host, as ``Reduce.fold`` is for
the aggregating scans; ``filter_records`` is the device primitive over any DeviceRecords, with
segments; ``filter_file`` writes the filtered .mtbl file on the device.

HAVING needs no call of its own.  A Rollup's values are encoded in its Reduce's layout, so

    ro = rollup_records(recs, group, red, seg_off)
    f = filter_records(ro.records, Where.like(ro.reduce, [(0, 100, None)]), seg_off=ro.seg_grp)

keeps the groups whose first field is at least 100, segment by segment: ``f.records`` are their keys
and values, ``f.seg_end`` the kept groups of every segment, and ``ro.fields[f.src_idx]`` /
``ro.nrec[f.src_idx]`` their side arrays.
"""
from __future__ import annotations

import ctypes as C

from .reduce import ENCODINGS, MAX_FIELDS, Reduce

_MASK = (1 << 64) - 1
MODES = {"all": 0, "any": 1}   # MTBLX_WHERE_ANY


class Where:
    """`nfields` fields in `encoding`, and `clauses`: (field, lo, hi) keeps lo <= x <= hi (unsigned,
    inclusive; None: 0 / 2^64 - 1), (field, lo, hi, "outside") keeps the others.  lo > hi is an empty
    range.  mode "all": every constrained field passes (no clause: everything well-formed is kept);
    "any": at least one does (no clause: nothing is kept)."""

    def __init__(self, nfields: int, clauses=(), encoding: str = "u64le", mode: str = "all"):
        if not isinstance(nfields, int) or isinstance(nfields, bool) or not 1 <= nfields <= MAX_FIELDS:
            raise ValueError(f"Where: nfields {nfields!r} (1 to {MAX_FIELDS})")
        if encoding not in ENCODINGS:
            raise ValueError(f"Where encoding: {encoding!r} (one of 'u64le', 'varint')")
        if mode not in MODES:
            raise ValueError(f"Where mode: {mode!r} (one of 'all', 'any')")
        self.nfields, self.encoding, self.mode = nfields, encoding, mode
        self.mask = self.outside = 0
        lo, hi = [0] * MAX_FIELDS, [_MASK] * MAX_FIELDS
        for c in clauses:
            if not isinstance(c, (tuple, list)) or len(c) not in (3, 4):
                raise ValueError(f"Where clause: {c!r} ((field, lo, hi) or (field, lo, hi, 'outside'))")
            f = c[0]
            if not isinstance(f, int) or isinstance(f, bool) or not 0 <= f < nfields:
                raise ValueError(f"Where clause: field {f!r} (0 to {nfields - 1})")
            if self.mask >> f & 1:
                raise ValueError(f"Where: a second clause on field {f}")
            if len(c) == 4:
                if c[3] not in ("outside", "inside"):
                    raise ValueError(f"Where clause: {c[3]!r} ('outside' or 'inside')")
                if c[3] == "outside":
                    self.outside |= 1 << f
            for name, b, dflt in (("lo", c[1], 0), ("hi", c[2], _MASK)):
                if b is None:
                    b = dflt
                if not isinstance(b, int) or isinstance(b, bool) or not 0 <= b <= _MASK:
                    raise ValueError(f"Where clause: {name} {b!r} (None or an int in 0 .. 2^64 - 1)")
                (lo if name == "lo" else hi)[f] = b
            self.mask |= 1 << f
        self.lo, self.hi = tuple(lo), tuple(hi)

    @classmethod
    def like(cls, reduce, clauses=(), mode: str = "all") -> "Where":
        """the layout taken from a Reduce"""
        if not isinstance(reduce, Reduce):
            raise ValueError(f"Where.like: {reduce!r} is not a Reduce")
        return cls(len(reduce.ops), clauses, reduce.encoding, mode)

    @property
    def varint(self) -> bool:
        return self.encoding == "varint"

    def layout(self) -> Reduce:
        """a Reduce of this layout (its ops do not matter): decode / encode of the values"""
        return Reduce(*(["sum"] * self.nfields), encoding=self.encoding)

    def same_layout(self, reduce) -> bool:
        return isinstance(reduce, Reduce) and len(reduce.ops) == self.nfields and reduce.encoding == self.encoding

    def keeps(self, value):
        """the contract itself on the host: True (kept), False (well-formed, rejected), None (bad)"""
        x = self.layout().decode(bytes(value))
        if x is None:
            return None
        passed = [(self.lo[f] <= x[f] <= self.hi[f]) != bool(self.outside >> f & 1)
                  for f in range(self.nfields) if self.mask >> f & 1]
        return any(passed) if self.mode == "any" else all(passed)

    def cstruct(self):
        """the mtblx_where of this predicate"""
        from . import _lib
        w = _lib.WhereSpec()
        w.nfields = self.nfields
        w.flags = MODES[self.mode] | ENCODINGS[self.encoding]
        w.mask, w.outside = self.mask, self.outside
        for f in range(MAX_FIELDS):
            w.lo[f], w.hi[f] = self.lo[f], self.hi[f]
        return w

    def _t(self):
        return (self.nfields, self.encoding, self.mode, self.mask, self.outside, self.lo, self.hi)

    def __eq__(self, other):
        return isinstance(other, Where) and self._t() == other._t()

    def __hash__(self):
        return hash(self._t())

    def __repr__(self):
        cl = []
        for f in range(self.nfields):
            if self.mask >> f & 1:
                c = (f, self.lo[f], self.hi[f]) + (("outside",) if self.outside >> f & 1 else ())
                cl.append(repr(c))
        enc = ", encoding='varint'" if self.varint else ""
        mode = ", mode='any'" if self.mode == "any" else ""
        return f"Where({self.nfields}, [{', '.join(cl)}]{enc}{mode})"


def as_where(where):
    """None or a Where"""
    if where is not None and not isinstance(where, Where):
        raise ValueError(f"where: {where!r} is not a Where")
    return where


class Filtered:
    """filter_records' result.  Device tensors: `records` (a DeviceRecords: the kept records in their
    order, its `stream` set), `src_idx` int64 [kept] (the index in the input of every kept record),
    `seg_end` int64 [nseg] (the END index of every segment in the kept order: segment q's kept records
    are [seg_end[q - 1], seg_end[q]), 0 before segment 0), `seg_bad` int64 [nseg] (the bad values of
    every segment).  Host ints: `nbad` (bad values), `nrejected` (well-formed values the predicate
    rejected), `nkept`."""

    def __init__(self, where, records, src_idx, seg_end, seg_bad, nbad, nrejected, stream=None):
        self._stream = stream
        self.where, self.records, self.src_idx = where, records, src_idx
        self.seg_end, self.seg_bad, self.nbad, self.nrejected = seg_end, seg_bad, nbad, nrejected

    @property
    def nkept(self) -> int:
        return int(self.src_idx.numel())

    def seg_off(self):
        """{0, seg_end...}: the kept records as the seg_off of a following segmented call"""
        import torch
        return torch.cat([torch.zeros(1, dtype=torch.int64, device=self.seg_end.device), self.seg_end])


def filter_records(records, where, seg_off=None, stream=None) -> Filtered:
    """The records of `records` (an encode.DeviceRecords) whose value `where` (a Where) keeps, in their
    order.  seg_off: int64 [nseg + 1] (device, or anything torch.as_tensor takes) with
    0 = off[0] <= ... <= off[nseg] = n, else ValueError; None: no segments (seg_end and seg_bad are
    then empty).  mtblx_where_plan, the read-back of its totals, one allocation sized from them,
    mtblx_where_emit: no record returns to the host.  Everything runs on `stream` (default: the
    current stream), which the call synchronises."""
    import torch

    from . import _lib, codec
    from .encode import DeviceRecords
    w = as_where(where)
    if w is None:
        raise ValueError("filter_records: where is a Where")
    dev = records.key_end.device
    s = codec._stream_of(stream, dev)
    with torch.cuda.stream(s):
        L = codec._require_device()
        ke = records.key_end.contiguous()
        ve = records.val_end.contiguous()
        n = int(ke.numel())
        if seg_off is None:
            seg, nseg = None, 0
        else:
            seg = torch.as_tensor(seg_off, dtype=torch.int64, device=dev).contiguous()
            if seg.dim() != 1 or seg.numel() < 1:
                raise ValueError("filter_records: seg_off must be a 1-d array of nseg + 1 offsets")
            nseg = int(seg.numel()) - 1
            if nseg == 0 and n != 0:
                raise ValueError("filter_records: seg_off holds no segment but there are records")
        rec = _lib.Records(codec._u(records.keys), codec._u(ke), codec._u(records.vals), codec._u(ve), n)
        spec = w.cstruct()
        wsb = int(L.mtblx_where_workspace_bytes(n, nseg))
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        segs = torch.zeros(2 * nseg, dtype=torch.int64, device=dev)
        seg_end, seg_bad = segs[:nseg], segs[nseg:]
        totals = (C.c_uint64 * 6)()
        sh = C.c_void_p(codec._stream_handle(s))
        rc = L.mtblx_where_plan(C.byref(rec), C.byref(spec), C.c_void_p(seg.data_ptr()) if nseg else None, nseg,
                                totals, C.c_void_p(seg_end.data_ptr()) if nseg else None,
                                C.c_void_p(seg_bad.data_ptr()) if nseg else None, C.c_void_p(ws.data_ptr()), wsb, sh)
        if rc == _lib.MTBLX_E_FORMAT and totals[5] & _lib.WHERE_BADSEG:
            raise ValueError("filter_records: seg_off must satisfy 0 = off[0] <= ... <= off[nseg] = n")
        if rc != 0:
            raise RuntimeError(f"mtblx_where_plan failed: {rc}")
        K, kb, vb, nbad, nrej = (int(totals[i]) for i in range(5))
        # one buffer: the u64 arrays first (aligned), then the flags' word, then the key and value bytes
        buf = torch.empty(8 * 3 * K + 8 + kb + vb, dtype=torch.uint8, device=dev)
        key_end = buf[: 8 * K].view(torch.int64)
        val_end = buf[8 * K: 16 * K].view(torch.int64)
        src_idx = buf[16 * K: 24 * K].view(torch.int64)
        flags = buf[24 * K: 24 * K + 8].view(torch.int32)
        keys = buf[24 * K + 8: 24 * K + 8 + kb]
        vals = buf[24 * K + 8 + kb:]
        p = buf.data_ptr()
        out = _lib.Filtered(keys=p + 24 * K + 8, keys_cap=kb, vals=p + 24 * K + 8 + kb, vals_cap=vb, key_end=p,
                            val_end=p + 8 * K, src_idx=p + 16 * K, rec_cap=K, flags=p + 24 * K)
        rc = L.mtblx_where_emit(C.byref(rec), C.byref(out), C.c_void_p(ws.data_ptr()), wsb, sh)
        if rc != 0:
            raise RuntimeError(f"mtblx_where_emit failed: {rc}")
        fl = int(flags[0].item())   # on s, behind the emit: the workspace may go back to the allocator
        if fl:
            raise RuntimeError(f"mtblx_where_emit: flags {fl}")
        return Filtered(w, DeviceRecords(keys, key_end, vals, val_end, s), src_idx, seg_end, seg_bad, nbad, nrej, s)


def filter_file(reader, where, **write_file_kwargs):
    """The .mtbl file (device uint8 tensor) of the records of `reader` whose value `where` keeps, on
    the device from the scan of the file to the written blocks; bad values are dropped.  `reader`: a
    reader.Reader, or the bytes / device tensor of a .mtbl file.  Keyword arguments go to
    encode.write_file (block_size, restart_interval, compression); ``stream=`` is the stream of the
    stream contract."""
    import torch

    from . import encode
    from . import reader as rd
    from .merger import _clean_scan
    w = as_where(where)
    if w is None:
        raise ValueError("filter_file: where is a Where")
    r = reader if isinstance(reader, rd.Reader) else rd.Reader(reader)
    stream = r._s(write_file_kwargs.pop("stream", None))
    with torch.cuda.stream(stream):   # a scan that does not end cleanly raises as Merger sources do
        f = filter_records(_clean_scan(r.iter()), w, None, stream)
        return encode.write_file(f.records, stream=stream, **write_file_kwargs)

"""Rollups: device records grouped by a prefix of their key, one aggregate per group
(include/mtblx.h "Rollups", csrc/rollup.hip).

    GroupBy.length(4)                the first 4 bytes of the key (the whole key if it is shorter)
    GroupBy.delimiter(0x2e)          the key up to and including its first "."
    GroupBy.delimiter(0x2f, 2)       ... its second "/": the first two path components

Both rules are monotone in the key order, so over sorted records the records of one group key are
adjacent and the group keys come out strictly increasing: a rollup of a file or of a merged stream
is itself a valid input of the device Writer.  A group is a RUN of adjacent records with one group
key inside one segment, as in uniq: nothing checks the order, and on unsorted input equal group keys
that are not adjacent stay apart.

Per group the result holds its key, nrec, and nbad / fields exactly as Reduce.fold defines them over
the group's values (bad values are left out and counted; nothing passes through, not even in a
group of one), and its value: Reduce.encode of the fields, the identities where no value was good.

rollup_records is the primitive over any DeviceRecords; Reader.rollup / Reader.rollup_batch and
Merger.rollup / Merger.rollup_batch put it behind a file, a batch of queries and a merged view.
"""
from __future__ import annotations

import ctypes as C

from .reduce import MergeError, as_reduce


class GroupBy:
    """how a key is cut to its group key: GroupBy.length(L) or GroupBy.delimiter(byte, count=1)"""

    def __init__(self, kind: str, length: int = 0, delim: int = 0, count: int = 0):
        self.kind, self.length_, self.delim, self.count = kind, length, delim, count

    @staticmethod
    def length(L: int) -> "GroupBy":
        if not isinstance(L, int) or isinstance(L, bool) or not 1 <= L < 1 << 64:
            raise ValueError(f"GroupBy.length: {L!r} (an int >= 1)")
        return GroupBy("length", length=L)

    @staticmethod
    def delimiter(byte, count: int = 1) -> "GroupBy":
        if isinstance(byte, (bytes, bytearray)) and len(byte) == 1:
            byte = byte[0]
        if not isinstance(byte, int) or isinstance(byte, bool) or not 0 <= byte <= 255:
            raise ValueError(f"GroupBy.delimiter: byte {byte!r} (0 .. 255, or one byte)")
        if not isinstance(count, int) or isinstance(count, bool) or not 1 <= count < 1 << 32:
            raise ValueError(f"GroupBy.delimiter: count {count!r} (an int >= 1)")
        return GroupBy("delimiter", delim=byte, count=count)

    def __repr__(self):
        if self.kind == "length":
            return f"GroupBy.length({self.length_})"
        return f"GroupBy.delimiter({self.delim:#04x}, {self.count})"

    def __eq__(self, other):
        return isinstance(other, GroupBy) and (other.kind, other.length_, other.delim, other.count) == \
            (self.kind, self.length_, self.delim, self.count)

    def __hash__(self):
        return hash((self.kind, self.length_, self.delim, self.count))

    def gkey(self, key: bytes) -> bytes:
        """the group key of `key` (the host definition)"""
        if self.kind == "length":
            return key[: self.length_]
        p = -1
        for _ in range(self.count):
            p = key.find(bytes([self.delim]), p + 1)
            if p < 0:
                return key
        return key[: p + 1]

    def cstruct(self):
        """the mtblx_group of this rule"""
        from . import _lib
        if self.kind == "length":
            return _lib.Group(_lib.GROUP_LENGTH, self.length_, 0, 0)
        return _lib.Group(_lib.GROUP_DELIM, 0, self.delim, self.count)


def _as_group(group) -> GroupBy:
    if not isinstance(group, GroupBy):
        raise ValueError(f"rollup: {group!r} is not a GroupBy")
    return group


def reduce_encode(fields, reduce, stream=None):
    """mtblx_reduce_encode: rows of u64 fields (device int64 [n, F], the bit patterns) -> their values
    in `reduce`'s encoding, (vals uint8, val_end int64 [n]) on the device.  u64le: 8 * F bytes per row;
    varint: F canonical varints, vals cut to the bytes used (one word read back on `stream`)."""
    import torch

    from . import _lib, codec
    red = as_reduce(reduce)
    if red is None:
        raise ValueError(f"reduce_encode: {reduce!r} is not a Reduce")
    nf = len(red.ops)
    dev = fields.device
    s = codec._stream_of(stream, dev)
    with torch.cuda.stream(s):
        fields = fields.contiguous()
        if fields.dim() != 2 or fields.shape[1] != nf or fields.dtype != torch.int64:
            raise ValueError(f"reduce_encode: fields must be int64 [n, {nf}]")
        n = int(fields.shape[0])
        cap = (10 if red.varint else 8) * nf * n
        vals = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
        val_end = torch.empty(n, dtype=torch.int64, device=dev)
        if n == 0:
            return vals[:0], val_end
        L = _lib.lib()
        wsb = int(L.mtblx_reduce_encode_workspace_bytes(n))
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        spec = red.cstruct()
        rc = L.mtblx_reduce_encode(C.c_void_p(fields.data_ptr()), n, C.byref(spec), C.c_void_p(vals.data_ptr()),
                                   C.c_void_p(val_end.data_ptr()), cap, C.c_void_p(ws.data_ptr()), wsb,
                                   C.c_void_p(codec._stream_handle(s)))
        if rc != 0:
            raise RuntimeError(f"mtblx_reduce_encode failed: {rc}")
        used = int(val_end[-1].item()) if red.varint else cap   # on s, behind the kernels: ws may go back
        return vals[:used], val_end


class Rollup:
    """rollup_records' result (and that of the Reader's and the Merger's rollup calls).  Device tensors:
    `records` (a DeviceRecords: the group keys and the encoded values, its `stream` set), `fields`
    int64 [G, F] (the u64 bit patterns), `nrec` / `nbad` int64 [G], `grp_rec` int64 [G + 1] (the first
    record of every group, then n), `seg_grp` int64 [nseg + 1] (the groups before every segment:
    segment q's groups are [seg_grp[q], seg_grp[q + 1])).  A query of a batch that the scan handed
    back to the seek path was rolled up from its own device records and is kept beside the kernel
    path's answer: groups(q) serves every query, whichever path answered it."""

    def __init__(self, group, reduce, records, fields, nrec, nbad, grp_rec, seg_grp, stream=None, served=None,
                 ends=None):
        self._stream = stream      # the stream of the rollup: every host read goes through it
        self.group, self.reduce, self.records = group, reduce, records
        self.fields, self.nrec, self.nbad, self.grp_rec, self.seg_grp = fields, nrec, nbad, grp_rec, seg_grp
        self.nseg = int(seg_grp.numel()) - 1
        self._served = served or {}   # q -> Rollup of the queries the seek path answered
        self._ends = ends or {}       # q -> (end, err) of those queries
        self._host = None

    @property
    def ngroups(self) -> int:
        return int(self.nrec.numel())

    def served_by_kernel(self, q: int) -> bool:
        return q not in self._served

    def end(self, q: int) -> int:
        return self._ends[q][0] if q in self._ends else 0   # reader.END_NONE

    def err(self, q: int) -> str:
        return self._ends[q][1] if q in self._ends else "None"

    def _h(self):
        if self._host is None:
            import torch
            with torch.cuda.stream(self._stream):   # one read-back, on the rollup's stream
                r = self.records
                self._host = (r.keys.cpu().numpy().tobytes(), r.key_end.cpu().numpy(),
                              self.fields.cpu().numpy().view("uint64"), self.nrec.cpu().numpy(),
                              self.nbad.cpu().numpy(), self.seg_grp.cpu().numpy())
        return self._host

    def groups(self, q: int = 0):
        """segment (query) q's groups on the host: [(key, fields as unsigned ints, nrec, nbad)]"""
        if q in self._served:
            return self._served[q].groups(0)
        if not 0 <= q < self.nseg:
            raise IndexError(f"groups: segment {q} of {self.nseg}")
        k, ke, f, nr, nb, sg = self._h()
        g0, g1 = int(sg[q]), int(sg[q + 1])
        pk = int(ke[g0 - 1]) if g0 else 0
        out = []
        for g in range(g0, g1):
            out.append((k[pk: ke[g]], tuple(int(x) for x in f[g]), int(nr[g]), int(nb[g])))
            pk = int(ke[g])
        return out

    def check(self) -> None:
        """MergeError if any group met a bad value (not 8 * F bytes long; varint: not F varints)"""
        _, _, _, _, nb, sg = self._h()
        for q in range(self.nseg):
            if q in self._served:   # its slot in the buffers holds what the kernels left of it
                self._served[q].check()
                continue
            part = nb[int(sg[q]): int(sg[q + 1])]
            if part.any():
                g = int(sg[q]) + int(part.nonzero()[0][0])
                raise MergeError(f"rollup: group {g} (segment {q}) met {int(nb[g])} values that are not "
                                 f"{self.reduce.shape}")

    def write_file(self, block_size: int = 8192, restart_interval: int = 16, compression: int = 0):
        """check(), then the .mtbl file of (group key, value) written by the device Writer on the
        rollup's stream (device uint8).  For a rollup of one segment over sorted records: the group
        keys then increase strictly; anything else is refused by the Writer's order check."""
        from . import encode
        self.check()
        return encode.write_file(self.records, block_size, restart_interval, stream=self._stream,
                                 compression=compression)


def rollup_records(records, group, reduce, seg_off=None, stream=None, where=None) -> Rollup:
    """`records` (an encode.DeviceRecords) grouped by `group` (a GroupBy) inside every segment, `reduce`
    (a Reduce or a shorthand name) folded over every group's values.  seg_off: int64 [nseg + 1] (device,
    or anything torch.as_tensor takes) with 0 = off[0] <= ... <= off[nseg] = n, else ValueError; None:
    one segment that holds everything.  mtblx_rollup_plan, a read-back of its two totals, one
    allocation sized from them, mtblx_rollup_emit, mtblx_reduce_segments over the groups and
    mtblx_reduce_encode: no record returns to the host.  Everything runs on `stream` (default: the
    current stream), which the call synchronises.  where (a where.Where): the records are filtered
    first (filter_records) and the kept ones rolled up with the kept segments (seg_off = {0,
    seg_end...}); grp_rec then indexes the KEPT records and a bad value is dropped by the filter, so
    nbad is 0 wherever the Where has the Reduce's layout."""
    import torch

    from . import _lib, codec
    from .encode import DeviceRecords
    from .reduce import reduce_segments
    grp = _as_group(group)
    red = as_reduce(reduce)
    if red is None:
        raise ValueError(f"rollup: {reduce!r} is not a Reduce")
    if where is not None:
        from .where import as_where, filter_records
        kept = filter_records(records, as_where(where), [0, records.n] if seg_off is None else seg_off, stream)
        return rollup_records(kept.records, grp, red, kept.seg_off(), kept._stream, None)
    dev = records.key_end.device
    s = codec._stream_of(stream, dev)
    with torch.cuda.stream(s):
        L = codec._require_device()
        ke = records.key_end.contiguous()
        ve = records.val_end.contiguous()
        n = int(ke.numel())
        if seg_off is None:
            seg = torch.tensor([0, n], dtype=torch.int64, device=dev)
        else:
            seg = torch.as_tensor(seg_off, dtype=torch.int64, device=dev).contiguous()
            if seg.dim() != 1 or seg.numel() < 1:
                raise ValueError("rollup: seg_off must be a 1-d array of nseg + 1 offsets")
        nseg = int(seg.numel()) - 1
        if nseg == 0 and n != 0:
            raise ValueError("rollup: seg_off holds no segment but there are records")
        rec = _lib.Records(codec._u(records.keys), codec._u(ke), codec._u(records.vals), codec._u(ve), n)
        g = grp.cstruct()
        wsb = int(L.mtblx_rollup_workspace_bytes(n, nseg))
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        totals = torch.zeros(2, dtype=torch.int64, device=dev)
        sh = C.c_void_p(codec._stream_handle(s))
        segp = C.c_void_p(seg.data_ptr()) if nseg else None
        rc = L.mtblx_rollup_plan(C.byref(rec), C.byref(g), segp, nseg, C.c_void_p(totals.data_ptr()),
                                 C.c_void_p(ws.data_ptr()), wsb, sh)
        if rc != 0:
            raise RuntimeError(f"mtblx_rollup_plan failed: {rc}")
        G, kb = (int(x) for x in totals.cpu())   # the read-back of two words, on s
        # one buffer: the u64 arrays first (aligned), then the flags' word, then the key bytes
        words = G + (G + 1) + (nseg + 1)
        buf = torch.empty(8 * words + 8 + kb, dtype=torch.uint8, device=dev)
        key_end = buf[: 8 * G].view(torch.int64)
        grp_rec = buf[8 * G: 8 * (2 * G + 1)].view(torch.int64)
        seg_grp = buf[8 * (2 * G + 1): 8 * words].view(torch.int64)
        flags = buf[8 * words: 8 * words + 8].view(torch.int32)
        keys = buf[8 * words + 8:]
        if nseg == 0:
            seg_grp.zero_()
        p = buf.data_ptr()
        out = _lib.Rolled(keys=p + 8 * words + 8, keys_cap=kb, key_end=p, key_end_cap=8 * G, grp_rec=p + 8 * G,
                          grp_rec_cap=8 * (G + 1), seg_grp=p + 8 * (2 * G + 1), seg_grp_cap=8 * (nseg + 1),
                          flags=p + 8 * words)
        rc = L.mtblx_rollup_emit(C.byref(rec), C.byref(g), segp, nseg, C.byref(out), C.c_void_p(ws.data_ptr()), wsb, sh)
        if rc != 0:
            raise RuntimeError(f"mtblx_rollup_emit failed: {rc}")
        fl = int(flags[0].item())   # on s, behind the emit: the workspace may go back to the allocator
        if fl & _lib.ROLLUP_BADSEG:
            raise ValueError("rollup: seg_off must satisfy 0 = off[0] <= ... <= off[nseg] = n")
        if fl:
            raise RuntimeError(f"mtblx_rollup_emit: flags {fl}")
        fields, nbad = reduce_segments(DeviceRecords(records.keys, ke, records.vals, ve), grp_rec[:-1], grp_rec[1:],
                                       red, s)
        nrec = grp_rec[1:] - grp_rec[:-1]
        vals, val_end = reduce_encode(fields, red, s)
        return Rollup(grp, red, DeviceRecords(keys, key_end, vals, val_end, s), fields, nrec, nbad, grp_rec, seg_grp, s)

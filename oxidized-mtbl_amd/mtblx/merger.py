"""Merger / MergerBuilder mirror over the device merge (reference src/merger.rs).

    MergerBuilder::new / add / push / build, Extend   src/merger.rs:66-94
    Merger::builder                                   :101-105
    Merger::into_merge_iter -> MergerIter             :108-125, :159-214
    Merger::into_iter -> MultiIter                    :127-142, :216-260
    Merger::write_into                                :145-157

Every source is scanned on the device (Reader.iter()), and its records never leave it: the
k-way merge, the grouping of duplicate keys and the gather of the merged records are
mtblx_merge_plan / mtblx_merge_emit (include/mtblx.h, csrc/merge.hip).  The built-in merge
functions "concat", "first" and "last" and a reduce.Reduce (u64 sum / min / max per field,
mtblx_merge_emit_reduce) produce an encode.DeviceRecords that feeds
encode.write_file as it is; a callable ``merge(key, values) -> bytes`` is applied on the host to
the groups of two or more values, as the reference never calls it for a group of one (:200-207).

What is promised (include/mtblx.h): keys in order, every source's value per key, the values of a
key in the order the sources were added (the reference leaves that order to its BinaryHeap); the
empty-key quirk of :182-186; an out-of-order source raises UnsortedSource (the reference does not
check).  More than 64 sources are merged in rounds of 64 with the same mode.

Batched reads of the merged view (what the C mtbl library's merger offers as iter_prefix /
iter_range / get on a merger source, for a whole batch): Merger.scan_batch / scan_batch_groups /
get_batch take Reader.scan_batch on every source and join the answers with ONE segmented merge
(merge_segments over mtblx_merge_seg_plan / mtblx_merge_seg_emit, csrc/merge_seg.hip): order
(query, key, source), the empty-key quirk applied inside every query.  -> MergedScanBatch.

Set operations (setops.Select; include/mtblx.h "Set operations"): ``select=`` on merge_records /
merge_all / merge_segments, MergerBuilder.select(sel) and Merger(..., select=sel) keep a key by which
sources hold it (mtblx_merge_plan_select / mtblx_merge_seg_plan_select); every Merger method then
works on the selected groups.  Refused with ValueError before any device work: a selection over
more than 64 sources (a rule over source masks cannot be applied per round), a selection together
with max_records (m + 1 records per source no longer cover the first m items once groups are
dropped), a Select naming a source that is not there.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, codec, encode
from .encode import DeviceRecords
from .reduce import MergeError, Reduce, ReduceBatch, as_reduce, check_merge, reduce_segments  # noqa: F401
from .setops import Select, as_select  # noqa: F401
from .writer import CompressionType

MODES = {"groups": _lib.MERGE_GROUPS, "concat": _lib.MERGE_CONCAT, "first": _lib.MERGE_FIRST,
         "last": _lib.MERGE_LAST}


class UnsortedSource(RuntimeError):
    """a source's key <= its predecessor (mtblx_merge_plan: MTBLX_E_FORMAT, MTBLX_MERGE_UNSORTED)"""

    def __init__(self, flags: int):
        super().__init__(f"merge source out of order (flags={flags})")
        self.flags = flags


@dataclass
class Grouped:
    """MultiIter's items on the device: key g = keys[key_end[g-1]:key_end[g]], its values are
    values grp_end[g-1] .. grp_end[g] of the list cut by val_end (all int64 END offsets)."""
    keys: torch.Tensor
    key_end: torch.Tensor
    vals: torch.Tensor
    val_end: torch.Tensor
    grp_end: torch.Tensor
    stream: object = None   # the stream the tensors were produced on: to_list() reads on it

    def to_list(self):
        with torch.cuda.stream(self.stream):
            ke, ve, ge = (t.cpu().numpy() for t in (self.key_end, self.val_end, self.grp_end))
            k, v = self.keys.cpu().numpy().tobytes(), self.vals.cpu().numpy().tobytes()
        out, pk, pv, pg = [], 0, 0, 0
        for g in range(ke.size):
            vs = []
            for j in range(pg, int(ge[g])):
                vs.append(v[pv: ve[j]])
                pv = int(ve[j])
            out.append((k[pk: ke[g]], vs))
            pk, pg = int(ke[g]), int(ge[g])
        return out


def _records_list(r: DeviceRecords):
    with torch.cuda.stream(r.stream):   # the stream that produced them (None: the current one)
        ke, ve = r.key_end.cpu().numpy(), r.val_end.cpu().numpy()
        k, v = r.keys.cpu().numpy().tobytes(), r.vals.cpu().numpy().tobytes()
    out, pk, pv = [], 0, 0
    for i in range(ke.size):
        out.append((k[pk: ke[i]], v[pv: ve[i]]))
        pk, pv = int(ke[i]), int(ve[i])
    return out


def merge_records(sources, mode, stream=None, device=None, select=None):
    """One mtblx_merge_plan + mtblx_merge_emit over at most 64 sources (DeviceRecords, in source
    order) -> Grouped for "groups", else DeviceRecords.  `mode` is a name of MODES, or a Reduce (or
    its shorthand name): then the emit is mtblx_merge_emit_reduce, with "first"'s layout (a varint
    Reduce: a layout of its own, inside "first"'s capacities), and a group of two or more holding a
    bad value raises MergeError.  `select` (a setops.Select): only the groups it keeps come out
    (mtblx_merge_plan_select).  Workspace and
    outputs are allocated on the stream the kernels run on."""
    L = codec._require_device()
    if len(sources) > _lib.MERGE_MAX_SOURCES:
        raise ValueError("merge_records takes at most 64 sources (Merger merges in rounds)")
    select = as_select(select, len(sources))
    red = as_reduce(mode)
    m = _lib.MERGE_FIRST if red is not None else MODES[mode]
    dev = torch.device(device) if device is not None else (sources[0].key_end.device if sources else
                                                          torch.device("cuda", torch.cuda.current_device()))
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(s):   # the caching allocator ties these blocks to the stream that uses them
        nsrc = len(sources)
        arr = (_lib.Records * max(nsrc, 1))()
        n = 0
        for i, r in enumerate(sources):
            arr[i] = r.cstruct()
            n += r.n
        if n >= _lib.MERGE_MAX_RECORDS:
            raise ValueError("merge: 2^32 - 16 records or more")
        wsb = int(L.mtblx_merge_workspace_bytes(n, nsrc))
        ws = torch.empty(wsb + 256, dtype=torch.uint8, device=dev)
        wp = (ws.data_ptr() + 255) & ~255
        tot = (C.c_uint64 * 8)()
        sh = C.c_void_p(int(s.cuda_stream))
        if select is not None:
            sel = select.cstruct()
            rc = L.mtblx_merge_plan_select(arr, nsrc, C.byref(sel), tot, C.c_void_p(wp), wsb, sh)
        else:
            rc = L.mtblx_merge_plan(arr, nsrc, tot, C.c_void_p(wp), wsb, sh)
        if rc == _lib.MTBLX_E_FORMAT:
            raise UnsortedSource(int(tot[5]))
        if rc != 0:
            raise RuntimeError(f"mtblx_merge_plan failed: {rc}")
        groups, kbytes, nval, vbytes = (int(tot[i]) for i in range(4))
        grouped = m == _lib.MERGE_GROUPS
        keys = torch.empty(kbytes, dtype=torch.uint8, device=dev)
        key_end = torch.empty(groups, dtype=torch.int64, device=dev)
        vals = torch.empty(vbytes, dtype=torch.uint8, device=dev)
        val_end = torch.empty(nval if grouped else groups, dtype=torch.int64, device=dev)
        grp_end = torch.empty(groups if grouped else 0, dtype=torch.int64, device=dev)
        flags = torch.zeros(1, dtype=torch.int32, device=dev)
        u = codec._u
        out = _lib.Merged(u(keys), kbytes, u(key_end), 8 * groups, u(vals), vbytes, u(val_end), 8 * val_end.numel(),
                          u(grp_end), 8 * grp_end.numel(), flags.data_ptr())
        if red is not None:
            spec = red.cstruct()
            rc = L.mtblx_merge_emit_reduce(arr, nsrc, C.byref(spec), C.byref(out), C.c_void_p(wp), wsb, sh)
        else:
            rc = L.mtblx_merge_emit(arr, nsrc, m, C.byref(out), C.c_void_p(wp), wsb, sh)
        if rc != 0:
            raise RuntimeError(f"mtblx_merge_emit failed: {rc}")
        f = int(flags.item())   # synchronizes: the workspace may go back to the allocator after this
        if f & _lib.MERGE_BADVALUE:
            raise MergeError(f"merge: a group of two or more holds a value that is not {red.shape}")
        if f:
            raise RuntimeError(f"mtblx_merge_emit: flags={f}")
        if m in (_lib.MERGE_FIRST, _lib.MERGE_LAST) and groups:   # vals was sized by its upper bound
            vals = vals[: int(val_end[-1].item())]
    if grouped:
        return Grouped(keys, key_end, vals, val_end, grp_end, s)
    return DeviceRecords(keys, key_end, vals, val_end, s)


def _regroup(parts, stream):
    """Grouped results of consecutive source chunks -> the Grouped of all their sources: the value
    bytes of every key joined chunk by chunk (CONCAT over the groups' byte ranges), and the value
    lengths joined the same way (CONCAT over each group's lengths as 8-byte words).  `stream`
    is the stream the parts were produced on; the torch ops between the merges run on it too."""
    a, b = [], []
    with torch.cuda.stream(stream):
        for p in parts:
            nv = int(p.val_end.numel())
            ng = int(p.grp_end.numel())
            gbytes = p.val_end[p.grp_end - 1] if ng else p.grp_end
            a.append(DeviceRecords(p.keys, p.key_end, p.vals, gbytes))
            lens = torch.diff(p.val_end, prepend=p.val_end.new_zeros(1)) if nv else p.val_end
            b.append(DeviceRecords(p.keys, p.key_end, lens.contiguous().view(torch.uint8), p.grp_end * 8))
        va = merge_records(a, "concat", stream)
        vb = merge_records(b, "concat", stream)
        lens = vb.vals.view(torch.int64) if vb.vals.numel() else vb.val_end.new_zeros(0)
        return Grouped(va.keys, va.key_end, va.vals, torch.cumsum(lens, 0), vb.val_end // 8, stream)


def merge_all(sources, mode, stream=None, device=None, select=None):
    """merge_records over any number of sources: rounds of 64 with the same mode, which keeps
    source order (and with it the exact result) for every mode; a Reduce is associative and
    passes a group of one through, so applying it per round gives the same bytes too.  `select`
    needs one round: at most 64 sources."""
    sources = list(sources)
    select = as_select(select, len(sources))
    grouped = mode == "groups"
    first = True
    dev = torch.device(device) if device is not None else (sources[0].key_end.device if sources else None)
    stream = codec._stream_of(stream, dev)   # resolved once: every round runs on the same stream
    while first or len(sources) > 1:
        chunks = [sources[i: i + _lib.MERGE_MAX_SOURCES] for i in range(0, len(sources), _lib.MERGE_MAX_SOURCES)] \
            or [[]]
        if grouped and not first:
            sources = [_regroup(c, stream) for c in chunks]
        else:
            sources = [merge_records(c, mode, stream, device, select) for c in chunks]
        first = False
    return sources[0]


def _merge_segments_64(sources, seg_offs, nseg, mode, s, dev, select=None):
    """one mtblx_merge_seg_plan + emit over at most 64 sources -> (DeviceRecords | Grouped, seg_end)"""
    L = codec._require_device()
    red = as_reduce(mode)
    m = _lib.MERGE_FIRST if red is not None else MODES[mode]
    with torch.cuda.stream(s):
        nsrc = len(sources)
        arr = (_lib.Records * max(nsrc, 1))()
        offs = (C.c_void_p * max(nsrc, 1))()
        n = 0
        for i, (r, o) in enumerate(zip(sources, seg_offs)):
            if o.dtype != torch.int64 or int(o.numel()) != nseg + 1 or not o.is_contiguous():
                raise ValueError("merge_segments: seg_offs are contiguous int64 tensors of nseg + 1 offsets")
            arr[i] = r.cstruct()
            offs[i] = o.data_ptr()
            n += r.n
        if n >= _lib.MERGE_MAX_RECORDS:
            raise ValueError("merge: 2^32 - 16 records or more")
        wsb = int(L.mtblx_merge_seg_workspace_bytes(n, nsrc, nseg))
        ws = torch.empty(wsb + 256, dtype=torch.uint8, device=dev)
        wp = (ws.data_ptr() + 255) & ~255
        seg_end = torch.empty(nseg, dtype=torch.int64, device=dev)
        tot = (C.c_uint64 * 8)()
        sh = C.c_void_p(int(s.cuda_stream))
        if select is not None:
            sel = select.cstruct()
            rc = L.mtblx_merge_seg_plan_select(arr, offs, nsrc, nseg, C.byref(sel), tot, C.c_void_p(seg_end.data_ptr()),
                                               C.c_void_p(wp), wsb, sh)
        else:
            rc = L.mtblx_merge_seg_plan(arr, offs, nsrc, nseg, tot, C.c_void_p(seg_end.data_ptr()), C.c_void_p(wp), wsb,
                                        sh)
        if rc == _lib.MTBLX_E_FORMAT:
            if int(tot[5]) & _lib.MERGE_BADSEG:
                raise ValueError("merge_segments: a seg_off array is not 0 = off[0] <= ... <= off[nseg] = n")
            raise UnsortedSource(int(tot[5]))
        if rc != 0:
            raise RuntimeError(f"mtblx_merge_seg_plan failed: {rc}")
        groups, kbytes, nval, vbytes = (int(tot[i]) for i in range(4))
        grouped = m == _lib.MERGE_GROUPS
        keys = torch.empty(kbytes, dtype=torch.uint8, device=dev)
        key_end = torch.empty(groups, dtype=torch.int64, device=dev)
        vals = torch.empty(vbytes, dtype=torch.uint8, device=dev)
        val_end = torch.empty(nval if grouped else groups, dtype=torch.int64, device=dev)
        grp_end = torch.empty(groups if grouped else 0, dtype=torch.int64, device=dev)
        flags = torch.zeros(1, dtype=torch.int32, device=dev)
        u = codec._u
        out = _lib.Merged(u(keys), kbytes, u(key_end), 8 * groups, u(vals), vbytes, u(val_end), 8 * val_end.numel(),
                          u(grp_end), 8 * grp_end.numel(), flags.data_ptr())
        if red is not None:
            spec = red.cstruct()
            rc = L.mtblx_merge_seg_emit_reduce(arr, offs, nsrc, nseg, C.byref(spec), C.byref(out), C.c_void_p(wp), wsb, sh)
        else:
            rc = L.mtblx_merge_seg_emit(arr, offs, nsrc, nseg, m, C.byref(out), C.c_void_p(wp), wsb, sh)
        if rc != 0:
            raise RuntimeError(f"mtblx_merge_seg_emit failed: {rc}")
        f = int(flags.item())   # synchronizes: the workspace may go back to the allocator after this
        if f & _lib.MERGE_BADVALUE:
            raise MergeError(f"merge: a group of two or more holds a value that is not {red.shape}")
        if f:
            raise RuntimeError(f"mtblx_merge_seg_emit: flags={f}")
        if m in (_lib.MERGE_FIRST, _lib.MERGE_LAST) and groups:   # vals was sized by its upper bound
            vals = vals[: int(val_end[-1].item())]
    if grouped:
        return Grouped(keys, key_end, vals, val_end, grp_end, s), seg_end
    return DeviceRecords(keys, key_end, vals, val_end, s), seg_end


def _seg_off_of(seg_end):
    return torch.cat([seg_end.new_zeros(1), seg_end])


def _regroup_segments(parts, seg_ends, nseg, s, dev):
    """_regroup for segmented results: the two CONCATs are segmented merges over the rounds' groups"""
    a, b, offs = [], [], []
    with torch.cuda.stream(s):
        for p, se in zip(parts, seg_ends):
            nv = int(p.val_end.numel())
            ng = int(p.grp_end.numel())
            gbytes = p.val_end[p.grp_end - 1] if ng else p.grp_end
            a.append(DeviceRecords(p.keys, p.key_end, p.vals, gbytes))
            lens = torch.diff(p.val_end, prepend=p.val_end.new_zeros(1)) if nv else p.val_end
            b.append(DeviceRecords(p.keys, p.key_end, lens.contiguous().view(torch.uint8), p.grp_end * 8))
            offs.append(_seg_off_of(se))
        va, se = _merge_segments_64(a, offs, nseg, "concat", s, dev)
        vb, _ = _merge_segments_64(b, offs, nseg, "concat", s, dev)
        lens = vb.vals.view(torch.int64) if vb.vals.numel() else vb.val_end.new_zeros(0)
        return Grouped(va.keys, va.key_end, va.vals, torch.cumsum(lens, 0), vb.val_end // 8, s), se


def merge_segments(sources, seg_offs, mode, stream=None, device=None, select=None):
    """The merge_records of the segmented calls (mtblx_merge_seg_plan / _emit, csrc/merge_seg.hip).
    Source i (a DeviceRecords) is nseg sorted runs back to back, cut by seg_offs[i] (device int64
    [nseg + 1], 0 = off[0] <= ... <= off[nseg] = n); segment q of the result is the Merger's result
    over segment q of every source, the empty-key quirk applied per segment.  `mode` is a name of
    MODES or a Reduce, as in merge_records.  -> (Grouped for "groups", else DeviceRecords; seg_end:
    device int64 [nseg], the END group index of every segment).  Any number of sources: rounds of 64
    with the same mode, a round's output cut by its seg_end being a source of the next ("groups":
    the two-CONCAT regrouping of _regroup, segmented).  `select` (a setops.Select, at most 64
    sources): every segment holds the groups it keeps, and seg_end counts those
    (mtblx_merge_seg_plan_select)."""
    sources, seg_offs = list(sources), list(seg_offs)
    if len(sources) != len(seg_offs):
        raise ValueError("merge_segments: one seg_off tensor per source")
    select = as_select(select, len(sources))
    if not sources and device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(device) if device is not None else seg_offs[0].device
    nseg = int(seg_offs[0].numel()) - 1 if seg_offs else 0
    if nseg < 0 or nseg > _lib.MERGE_MAX_SEGMENTS:
        raise ValueError("merge_segments: 0 to 2^24 segments")
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    grouped = mode == "groups"
    first = True
    with torch.cuda.stream(s):   # the seg_off joins between the rounds run on s, like the rounds
        while first or len(sources) > 1:
            idx = list(range(0, len(sources), _lib.MERGE_MAX_SOURCES)) or [0]
            outs = []
            for i in idx:
                c, o = sources[i: i + _lib.MERGE_MAX_SOURCES], seg_offs[i: i + _lib.MERGE_MAX_SOURCES]
                if grouped and not first:
                    outs.append(_regroup_segments(c, [x[1:] for x in o], nseg, s, dev))
                else:
                    outs.append(_merge_segments_64(c, o, nseg, mode, s, dev, select))
            sources = [r for r, _ in outs]
            seg_offs = [_seg_off_of(se) for _, se in outs]
            first = False
    return sources[0], seg_offs[0][1:]


def check_queries(queries, max_records):
    """-> (queries as tuples of bytes, per-query limits): what Reader.scan_batch accepts, checked
    before any source is touched"""
    qs = []
    for q in queries:
        if not isinstance(q, (tuple, list)) or not q or q[0] not in ("from", "get", "prefix", "range") or \
                len(q) != (3 if q[0] == "range" else 2):
            raise ValueError(f"scan_batch: bad query {q!r}")
        qs.append((q[0],) + tuple(bytes(k) for k in q[1:]))
    if max_records is None or isinstance(max_records, int):
        limits = [max_records] * len(qs)
    else:
        limits = list(max_records)
        if len(limits) != len(qs):
            raise ValueError("scan_batch: max_records must be one value or one per query")
    if any(m is not None and m < 0 for m in limits):
        raise ValueError("scan_batch: negative max_records")
    return qs, limits


class MergedScanBatch:
    """Merger.scan_batch's result, the counterpart of reader.ScanBatch.  Device tensors over all
    queries in (query, key) order: `keys` / `key_end` / `vals` / `val_end` (int64 END offsets from
    item 0 of the batch; in the grouped form `val_end` has one entry per value and `grp_end` [items]
    cuts the value list); `grp_off` int64 [nq + 1]: query q's items start at grp_off[q]; `count`
    int64 [nq]: how many of them the query reports (min(limit, its items): the items cut by a limit
    stay in the buffers, unreferenced).  A query some source handed back to the seek path was merged
    from the per-source answers by merge_all: its slot in the buffers holds whatever the kernels kept
    of it, count[q] counts the items of merge_all's answer, and records(q) / groups(q) /
    device_records(q) give every query's result, whichever path served it."""

    def __init__(self, nq, merged, seg_end, limits, served, merge, sbs, stream=None):
        self._stream = stream      # the stream the batch was produced on: every host read goes through it
        with torch.cuda.stream(stream):
            self._init(nq, merged, seg_end, limits, served, merge, sbs)

    def _init(self, nq, merged, seg_end, limits, served, merge, sbs):
        self.nq = nq
        self.grouped = isinstance(merged, Grouped)
        self.keys, self.key_end, self.vals, self.val_end = merged.keys, merged.key_end, merged.vals, merged.val_end
        self.grp_end = merged.grp_end if self.grouped else None
        self.grp_off = _seg_off_of(seg_end)
        self._off = self.grp_off.cpu().numpy()          # the one read-back of the kernel path
        n = np.diff(self._off)
        lim = np.array([np.iinfo(np.int64).max if m is None else m for m in limits], dtype=np.int64)
        self._count = np.minimum(n, lim) if nq else np.zeros(0, np.int64)
        for q, r in served.items():   # its slot in the buffers holds what the kernels left of it; the answer is `r`
            self._count[q] = int(r.key_end.numel())
        self.count = torch.from_numpy(self._count).to(seg_end.device)
        self._served = served      # q -> DeviceRecords | Grouped of the queries merge_all answered
        self._merge = merge
        self._host = self._hostb = None
        self.n_large = sum(sb.n_large for sb in sbs)
        self.n_fallback = sum(sb.n_fallback for sb in sbs)

    def served_by_kernel(self, q: int) -> bool:
        return q not in self._served

    def _ends(self):
        if self._host is None:
            with torch.cuda.stream(self._stream):
                self._host = (self.key_end.cpu().numpy(), self.val_end.cpu().numpy(),
                              self.grp_end.cpu().numpy() if self.grouped else None)
        return self._host

    def _view(self, q: int):
        """query q's reported items as a Grouped / DeviceRecords view of the batch's buffers"""
        if q in self._served:
            return self._served[q]
        with torch.cuda.stream(self._stream):   # the offset shifts below are kernels: on the batch's stream
            return self._view_on(q)

    def _view_on(self, q: int):
        ke, ve, ge = self._ends()
        g0 = int(self._off[q])
        g1 = g0 + int(self._count[q])
        k0 = int(ke[g0 - 1]) if g0 else 0
        k1 = int(ke[g1 - 1]) if g1 else 0
        if self.grouped:
            v0 = int(ge[g0 - 1]) if g0 else 0
            v1 = int(ge[g1 - 1]) if g1 else 0
            b0 = int(ve[v0 - 1]) if v0 else 0
            b1 = int(ve[v1 - 1]) if v1 else 0
            return Grouped(self.keys[k0:k1], self.key_end[g0:g1] - k0, self.vals[b0:b1], self.val_end[v0:v1] - b0,
                           self.grp_end[g0:g1] - v0, self._stream)
        b0 = int(ve[g0 - 1]) if g0 else 0
        b1 = int(ve[g1 - 1]) if g1 else 0
        return DeviceRecords(self.keys[k0:k1], self.key_end[g0:g1] - k0, self.vals[b0:b1], self.val_end[g0:g1] - b0,
                             self._stream)

    def _bytes(self):
        if self._hostb is None:
            with torch.cuda.stream(self._stream):
                self._hostb = (self.keys.cpu().numpy().tobytes(), self.vals.cpu().numpy().tobytes())
        return self._hostb

    def groups(self, q: int):
        """MultiIter's items of query q on the host (the grouped form: scan_batch_groups, or a
        callable merge function); the batch is copied once"""
        if not self.grouped:
            raise ValueError("groups(q): the batch holds merged values (scan_batch_groups keeps the groups)")
        if q in self._served:
            return self._served[q].to_list()
        ke, ve, ge = self._ends()
        k, v = self._bytes()
        g0 = int(self._off[q])
        pk = int(ke[g0 - 1]) if g0 else 0
        pg = int(ge[g0 - 1]) if g0 else 0
        pv = int(ve[pg - 1]) if pg else 0
        out = []
        for g in range(g0, g0 + int(self._count[q])):
            vs = []
            for j in range(pg, int(ge[g])):
                vs.append(v[pv: ve[j]])
                pv = int(ve[j])
            out.append((k[pk: ke[g]], vs))
            pk, pg = int(ke[g]), int(ge[g])
        return out

    def records(self, q: int):
        """MergerIter's items of query q on the host: [(key, merged value)]; the batch is copied once"""
        if self.grouped:
            if not callable(self._merge):
                raise ValueError("records(q): the batch holds groups (groups(q) returns them)")
            return [(k, vs[0] if len(vs) == 1 else bytes(self._merge(k, vs))) for k, vs in self.groups(q)]
        if q in self._served:
            return _records_list(self._served[q])
        ke, ve, _ = self._ends()
        k, v = self._bytes()
        g0 = int(self._off[q])
        pk = int(ke[g0 - 1]) if g0 else 0
        pv = int(ve[g0 - 1]) if g0 else 0
        out = []
        for g in range(g0, g0 + int(self._count[q])):
            out.append((k[pk: ke[g]], v[pv: ve[g]]))
            pk, pv = int(ke[g]), int(ve[g])
        return out

    def device_records(self, q: int) -> DeviceRecords:
        """query q's merged records on the device (what encode.write_file takes)"""
        with torch.cuda.stream(self._stream):
            if self.grouped:
                return DeviceRecords.from_list(self.records(q), device=self.keys.device, stream=self._stream)
            v = self._view(q)
            return DeviceRecords(v.keys, v.key_end.contiguous(), v.vals, v.val_end.contiguous(), self._stream)


def _cut_groups(r, m):
    """the first m items of a merge_all result"""
    if m is None or int(r.key_end.numel()) <= m:
        return r
    if m == 0:
        z = r.key_end[:0]
        return Grouped(r.keys[:0], z, r.vals[:0], z, z, r.stream) if isinstance(r, Grouped) else \
            DeviceRecords(r.keys[:0], z, r.vals[:0], z, r.stream)
    with torch.cuda.stream(r.stream):
        kb = int(r.key_end[m - 1].item())
        if isinstance(r, Grouped):
            nv = int(r.grp_end[m - 1].item())
            return Grouped(r.keys[:kb], r.key_end[:m], r.vals[: int(r.val_end[nv - 1].item())], r.val_end[:nv],
                           r.grp_end[:m], r.stream)
        return DeviceRecords(r.keys[:kb], r.key_end[:m], r.vals[: int(r.val_end[m - 1].item())], r.val_end[:m], r.stream)


def _scan_records(reader) -> DeviceRecords:
    """Reader.iter() of a source; a scan that does not end cleanly raises what the Reader surface
    raises (where the reference returns Err from into_merge_iter / fill, src/merger.rs:111-112, :190-193)"""
    return _clean_scan(reader.iter())


def _clean_scan(sc) -> DeviceRecords:
    from . import reader as R
    if sc.end in (R.END_ERR_OPEN, R.END_ERR_NEXT):
        raise R.MtblError(R.ERR_NAMES.index(sc.err) if sc.err in R.ERR_NAMES else 6)
    if sc.end == R.END_PANIC:
        raise R.ReferencePanic("merge source: the scan panics")
    if sc.end == R.END_LOOP:
        raise R.ReferenceLoop("merge source: the scan never ends")
    n = sc.nrec
    return DeviceRecords(sc.keys, sc.key_end[:n], sc.vals, sc.val_end[:n])


class MergerBuilder:
    """src/merger.rs:66-94.  merge: "concat" | "first" | "last" | Reduce (or "sum_u64" | "min_u64" |
    "max_u64") | callable(key, values) -> bytes"""

    def __init__(self, merge):
        self._merge = check_merge(merge)
        self._sources = []
        self._select = None

    def add(self, source) -> "MergerBuilder":
        self.push(source)
        return self

    def push(self, source) -> None:
        self._sources.append(source)

    def extend(self, sources) -> "MergerBuilder":
        self._sources.extend(sources)
        return self

    def select(self, sel) -> "MergerBuilder":
        """keep a key by which sources hold it (a setops.Select over the sources in the order added)"""
        self._select = sel
        return self

    def build(self) -> "Merger":
        return Merger(list(self._sources), self._merge, select=self._select)


class Merger:
    def __init__(self, sources, merge, stream=None, select=None):
        self.sources = sources
        self.merge = check_merge(merge)
        self.stream = stream
        self.select = as_select(select, len(sources))   # every method below works on the groups it keeps

    @staticmethod
    def builder(merge) -> MergerBuilder:
        return MergerBuilder(merge)

    def _device(self):
        return self.sources[0].file.device if self.sources else None

    def _s(self, stream=None):
        """S of the stream contract for this Merger: `stream`, else Merger(stream=), else the current stream"""
        return codec._stream_of(stream if stream is not None else self.stream, self._device())

    def _run(self, mode: str):
        s = self._s()
        with torch.cuda.stream(s):   # the sources are scanned on the stream that merges them
            return merge_all([_scan_records(r) for r in self.sources], mode, s, self._device(), self.select)

    def groups(self) -> Grouped:
        """MultiIter's items, on the device"""
        return self._run("groups")

    def into_iter(self):
        """MultiIter: (key, [values]) per distinct key, the values in source order"""
        return iter(self.groups().to_list())

    def _merged_list(self):
        out = []
        for k, vs in self.groups().to_list():
            out.append((k, vs[0] if len(vs) == 1 else bytes(self.merge(k, vs))))   # src/merger.rs:200-207
        return out

    def into_merge_iter(self):
        """MergerIter: (key, merged value) per distinct key"""
        if callable(self.merge):
            return iter(self._merged_list())
        return iter(_records_list(self.records()))

    def records(self, where=None) -> DeviceRecords:
        """the merged stream on the device (what encode.write_file takes).  where (a where.Where): only
        the records whose MERGED value it keeps -- the predicate sees the value after the merge function,
        the empty-key quirk and any Select (filter_records over the merged records)"""
        from .where import as_where, filter_records
        where = as_where(where)                             # refused before any device work
        s = self._s()
        if callable(self.merge):
            r = DeviceRecords.from_list(self._merged_list(), device=self._device() or "cuda", stream=s)
        else:
            r = self._run(self.merge)
        return r if where is None else filter_records(r, where, None, s).records

    def write_file(self, block_size: int = 8192, restart_interval: int = 16,
                   compression: int = CompressionType.None_, where=None) -> torch.Tensor:
        """the merged .mtbl file (device uint8), written by the device Writer; where: as records(where=)"""
        s = self._s()
        with torch.cuda.stream(s):   # records() and the Writer on one stream, also when self.stream is None
            return encode.write_file(self.records(where), block_size, restart_interval, stream=s, compression=compression)

    def write_into(self, writer) -> None:
        """Merger::write_into (src/merger.rs:149-156) for the host Writer"""
        r = self.records()
        if r.n == 0:
            return
        with torch.cuda.stream(r.stream):
            writer.insert_batch(r.keys.cpu().numpy(), r.key_end.cpu().numpy().astype(np.uint64),
                                r.vals.cpu().numpy(), r.val_end.cpu().numpy().astype(np.uint64))

    # ---- batched reads of the merged view ----
    def _scan_merge(self, queries, max_blocks, max_records, stream, mode) -> MergedScanBatch:
        qs, limits = check_queries(queries, max_records)
        if self.select is not None:
            as_select(self.select, len(self.sources))
            if any(m is not None for m in limits):
                raise ValueError("scan_batch: max_records cannot be combined with a selection (m + 1 records per "
                                 "source do not cover the first m items once groups are dropped)")
        s = self._s(stream)
        with torch.cuda.stream(s):   # the sources' scans, the seek-path answers, the merges and the read-back: all on s
            return self._scan_merge_on(qs, limits, max_blocks, s, mode)

    def _scan_merge_on(self, qs, limits, max_blocks, s, mode) -> MergedScanBatch:
        nq = len(qs)
        # m + 1 records per source are enough for the first m items: a source's record at position
        # p >= m + 1 has at least p - 1 >= m distinct kept keys before it (the - 1: the empty key)
        per_src = None if all(m is None for m in limits) else [None if m is None else m + 1 for m in limits]
        sbs = [r.scan_batch(qs, max_blocks, per_src, s) for r in self.sources]
        back = sorted({q for sb in sbs for q in sb._served})
        parts = {q: [_clean_scan(sb.scan(q)) for sb in sbs] for q in back}   # raises for the lowest (q, source)
        dev = self._device() or torch.device("cuda", torch.cuda.current_device())
        recs = [DeviceRecords(sb.keys, sb.key_end, sb.vals, sb.val_end) for sb in sbs]
        offs = [sb.rec_off.contiguous() for sb in sbs]
        if not sbs:   # no sources: nq empty segments of one empty source
            recs, offs = [DeviceRecords.from_list([], device=dev)], [torch.zeros(nq + 1, dtype=torch.int64, device=dev)]
        merged, seg_end = merge_segments(recs, offs, mode, s, dev, self.select if sbs else None)
        served = {q: _cut_groups(merge_all(parts[q], mode, s, dev, self.select), limits[q]) for q in back}
        return MergedScanBatch(nq, merged, seg_end, limits, served, self.merge, sbs, s)

    def scan_batch(self, queries, max_blocks: int = 64, max_records=None, stream=None) -> MergedScanBatch:
        """MergerIter over iter_from / get / iter_prefix / iter_range of every source, for a batch of
        queries (Reader.scan_batch's: ("from", k), ("get", k), ("prefix", p), ("range", a, b)): query
        q's result is what into_merge_iter would yield if each source were opened with that query,
        the empty-key quirk applied inside the query.  Every source answers the batch with
        Reader.scan_batch; one segmented merge (mtblx_merge_seg_plan / _emit) joins the answers on
        the device.  `max_records`: None, one limit or one per query: query q reports the first m
        items of its unlimited result (every source is asked for m + 1 records, the merged result is
        cut as a view).  With a Reduce, MergeError is raised iff a bad group lies among the reported
        items or among the at most S * (m + 1) records fetched for that query.  A query any source
        handed back to the seek path (max_blocks, a reference panic / error, an irregular index) is
        merged by merge_all from the per-source answers; a source's error raises as in records()."""
        return self._scan_merge(queries, max_blocks, max_records, stream,
                                "groups" if callable(self.merge) else self.merge)

    def scan_batch_groups(self, queries, max_blocks: int = 64, max_records=None, stream=None) -> MergedScanBatch:
        """scan_batch with MultiIter's items: groups(q) -> [(key, [values in source order])]"""
        return self._scan_merge(queries, max_blocks, max_records, stream, "groups")

    def get_batch(self, keys, max_blocks: int = 64, stream=None) -> MergedScanBatch:
        """the merged value of every key: scan_batch of ("get", k); count[q] is 0 or 1"""
        return self.scan_batch([("get", bytes(k)) for k in keys], max_blocks, None, stream)

    def reduce_batch(self, queries, reduce=None, max_blocks: int = 64, max_records=None, stream=None) -> ReduceBatch:
        """Reader.reduce_batch over the merged view: per query, `reduce` folded (Reduce.fold) over the
        merged values scan_batch reports for it.  scan_batch runs as it stands -- the Merger's own merge
        function (a built-in name or a Reduce) joins each key's values -- and one reduce_segments over
        the segments [grp_off[q], grp_off[q] + count[q]) of the merged buffers folds them; a query some
        source handed back is reduced from its own device records.  `reduce=None` takes the Merger's
        merge function when it is a Reduce.  A callable merge function is refused: the batch then holds
        groups, not values.  Everything runs on `stream` (default: Merger(stream=), else the current
        stream)."""
        if callable(self.merge):
            raise ValueError("reduce_batch: a callable merge function leaves groups, not merged values")
        red = as_reduce(reduce if reduce is not None else self.merge)
        if red is None:
            raise ValueError("reduce_batch: pass a Reduce (the Merger's merge function is not one)" if reduce is None
                             else f"reduce_batch: {reduce!r} is not a Reduce")
        mb = self.scan_batch(queries, max_blocks, max_records, stream)   # checks the queries before any source is touched
        s = mb._stream
        with torch.cuda.stream(s):
            lo = mb.grp_off[:-1].contiguous()
            cnt = mb._count.copy()
            cnt[sorted(mb._served)] = 0   # count[q] of a handed-back query counts merge_all's answer, not its slot
            fields, nbad = reduce_segments(DeviceRecords(mb.keys, mb.key_end, mb.vals, mb.val_end), lo,
                                           lo + torch.from_numpy(cnt).to(lo.device), red, s)
            nrec = mb.count.clone()
            for q, r in mb._served.items():   # its slot in the buffers holds what the kernels left of it
                n = int(r.key_end.numel())
                f, nb = reduce_segments(r, [0], [n], red, s)
                fields[q] = f[0]
                nbad[q] = nb[0]
            status = torch.zeros(mb.nq, dtype=torch.int32, device=nrec.device)
            if mb._served:
                status[torch.tensor(sorted(mb._served), dtype=torch.int64, device=nrec.device)] = _lib.SCAN_FALLBACK
            ends = {q: (0, "None") for q in mb._served}   # a source's error has raised in scan_batch
            return ReduceBatch(red, fields, nrec, nbad, status, ends, mb.n_large, mb.n_fallback, s)

    def rollup(self, group, reduce=None, stream=None):
        """The merged stream rolled up: records() -- the Merger's own merge function joins each key's
        values first, the empty-key quirk applied -- grouped by `group` (a rollup.GroupBy) with `reduce`
        folded over every group's merged values -> rollup.Rollup with one segment, whose write_file()
        gives the rolled-up .mtbl.  `reduce=None` takes the Merger's merge function when it is a
        Reduce.  A callable merge function is refused.  Everything runs on `stream` (default:
        Merger(stream=), else the current stream)."""
        from .rollup import _as_group, rollup_records
        grp, red = _as_group(group), self._rollup_reduce(reduce, "rollup")
        s = self._s(stream)
        with torch.cuda.stream(s):
            recs = merge_all([_scan_records(r) for r in self.sources], self.merge, s, self._device(), self.select)
            return rollup_records(recs, grp, red, None, s)

    def _rollup_reduce(self, reduce, what):
        if callable(self.merge):
            raise ValueError(f"{what}: a callable merge function leaves groups, not merged values")
        red = as_reduce(reduce if reduce is not None else self.merge)
        if red is None:
            raise ValueError(f"{what}: pass a Reduce (the Merger's merge function is not one)" if reduce is None
                             else f"{what}: {reduce!r} is not a Reduce")
        return red

    def rollup_batch(self, queries, group, reduce=None, max_blocks: int = 64, stream=None):
        """Reader.rollup_batch over the merged view: scan_batch runs as it stands -- the Merger's own
        merge function joins each key's values inside every query -- and one rollup over the merged
        buffers with the queries as segments (seg_off = grp_off) groups the merged records of every
        query; a query some source handed back is rolled up from its own merged device records.
        `reduce=None` and a callable merge function as in rollup().  -> rollup.Rollup, groups(q) per
        query.  Everything runs on `stream` (default: Merger(stream=), else the current stream)."""
        from .rollup import _as_group, rollup_records
        grp, red = _as_group(group), self._rollup_reduce(reduce, "rollup_batch")
        mb = self.scan_batch(queries, max_blocks, None, stream)   # checks the queries before any source is touched
        s = mb._stream
        with torch.cuda.stream(s):
            out = rollup_records(DeviceRecords(mb.keys, mb.key_end, mb.vals, mb.val_end), grp, red, mb.grp_off, s)
            for q, r in mb._served.items():   # its slot in the buffers holds what the kernels left of it
                out._served[q] = rollup_records(r, grp, red, None, s)
                out._ends[q] = (0, "None")    # a source's error has raised in scan_batch
            return out

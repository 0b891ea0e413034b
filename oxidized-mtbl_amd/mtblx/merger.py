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
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, codec, encode
from .encode import DeviceRecords
from .reduce import MergeError, Reduce, as_reduce, check_merge  # noqa: F401
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

    def to_list(self):
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
    ke, ve = r.key_end.cpu().numpy(), r.val_end.cpu().numpy()
    k, v = r.keys.cpu().numpy().tobytes(), r.vals.cpu().numpy().tobytes()
    out, pk, pv = [], 0, 0
    for i in range(ke.size):
        out.append((k[pk: ke[i]], v[pv: ve[i]]))
        pk, pv = int(ke[i]), int(ve[i])
    return out


def merge_records(sources, mode, stream=None, device=None):
    """One mtblx_merge_plan + mtblx_merge_emit over at most 64 sources (DeviceRecords, in source
    order) -> Grouped for "groups", else DeviceRecords.  `mode` is a name of MODES, or a Reduce (or
    its shorthand name): then the emit is mtblx_merge_emit_reduce, with "first"'s layout, and a
    group of two or more holding a value of another length raises MergeError.  Workspace and
    outputs are allocated on the stream the kernels run on."""
    L = codec._require_device()
    if len(sources) > _lib.MERGE_MAX_SOURCES:
        raise ValueError("merge_records takes at most 64 sources (Merger merges in rounds)")
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
        tot = (C.c_uint64 * 6)()
        sh = C.c_void_p(int(s.cuda_stream))
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
            raise MergeError(f"merge: a group of two or more holds a value that is not {red.width} bytes long")
        if f:
            raise RuntimeError(f"mtblx_merge_emit: flags={f}")
        if m in (_lib.MERGE_FIRST, _lib.MERGE_LAST) and groups:   # vals was sized by its upper bound
            vals = vals[: int(val_end[-1].item())]
    if grouped:
        return Grouped(keys, key_end, vals, val_end, grp_end)
    return DeviceRecords(keys, key_end, vals, val_end)


def _regroup(parts, stream):
    """Grouped results of consecutive source chunks -> the Grouped of all their sources: the value
    bytes of every key joined chunk by chunk (CONCAT over the groups' byte ranges), and the value
    lengths joined the same way (CONCAT over each group's lengths as 8-byte words)."""
    a, b = [], []
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
    return Grouped(va.keys, va.key_end, va.vals, torch.cumsum(lens, 0), vb.val_end // 8)


def merge_all(sources, mode, stream=None, device=None):
    """merge_records over any number of sources: rounds of 64 with the same mode, which keeps
    source order (and with it the exact result) for every mode; a Reduce is associative and
    passes a group of one through, so applying it per round gives the same bytes too."""
    sources = list(sources)
    grouped = mode == "groups"
    first = True
    while first or len(sources) > 1:
        chunks = [sources[i: i + _lib.MERGE_MAX_SOURCES] for i in range(0, len(sources), _lib.MERGE_MAX_SOURCES)] \
            or [[]]
        if grouped and not first:
            sources = [_regroup(c, stream) for c in chunks]
        else:
            sources = [merge_records(c, mode, stream, device) for c in chunks]
        first = False
    return sources[0]


def _scan_records(reader) -> DeviceRecords:
    """Reader.iter() of a source; a scan that does not end cleanly raises what the Reader surface
    raises (where the reference returns Err from into_merge_iter / fill, src/merger.rs:111-112, :190-193)"""
    from . import reader as R
    sc = reader.iter()
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

    def add(self, source) -> "MergerBuilder":
        self.push(source)
        return self

    def push(self, source) -> None:
        self._sources.append(source)

    def extend(self, sources) -> "MergerBuilder":
        self._sources.extend(sources)
        return self

    def build(self) -> "Merger":
        return Merger(list(self._sources), self._merge)


class Merger:
    def __init__(self, sources, merge, stream=None):
        self.sources = sources
        self.merge = check_merge(merge)
        self.stream = stream

    @staticmethod
    def builder(merge) -> MergerBuilder:
        return MergerBuilder(merge)

    def _device(self):
        return self.sources[0].file.device if self.sources else None

    def _run(self, mode: str):
        return merge_all([_scan_records(r) for r in self.sources], mode, self.stream, self._device())

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

    def records(self) -> DeviceRecords:
        """the merged stream on the device (what encode.write_file takes)"""
        if callable(self.merge):
            return DeviceRecords.from_list(self._merged_list(), device=self._device() or "cuda")
        return self._run(self.merge)

    def write_file(self, block_size: int = 8192, restart_interval: int = 16,
                   compression: int = CompressionType.None_) -> torch.Tensor:
        """the merged .mtbl file (device uint8), written by the device Writer"""
        return encode.write_file(self.records(), block_size, restart_interval, stream=self.stream,
                                 compression=compression)

    def write_into(self, writer) -> None:
        """Merger::write_into (src/merger.rs:149-156) for the host Writer"""
        r = self.records()
        if r.n == 0:
            return
        writer.insert_batch(r.keys.cpu().numpy(), r.key_end.cpu().numpy().astype(np.uint64),
                            r.vals.cpu().numpy(), r.val_end.cpu().numpy().astype(np.uint64))

"""Sorter / SorterBuilder mirror over the device sort (reference src/sorter.rs).

    SorterBuilder::new / max_memory / max_nb_chunks / chunk_compression_* / build   src/sorter.rs:25-70
    Sorter::builder / Sorter::new                                                   :107-115
    Sorter::insert: the memory rule                                                 :120-140
    Sorter::write_chunk                                                             :142-197
    Sorter::merge_chunks                                                            :199-233
    Sorter::write_into                                                              :235-242
    Sorter::into_iter                                                               :244-257
    defaults                                                                        src/lib.rs:11-15

Records go in in any order; ``write_chunk`` is one mtblx_sort_plan + mtblx_sort_emit
(``sort_records``: include/mtblx.h, csrc/sort.hip) and the chunks are merged by the device Merger
(``merger.merge_all``), whose empty-key quirk therefore applies exactly where the reference has it.

What differs from the reference, on purpose:
  * a chunk is a DeviceRecords kept in device memory, not a compressed temp file.  So
    ``chunk_compression_type`` / ``chunk_compression_level`` are accepted and stored and have no
    effect, and ``max_memory`` bounds the pending (unsorted) records only, as in the reference;
  * the values of a key come out in insertion order (the reference sorts with sort_unstable_by and
    drains a BinaryHeap: it promises only the multiset).  A merged chunk counts as the oldest
    source of every later merge, which keeps that order across ``merge_chunks``.
For the built-in merge functions and for a reduce.Reduce (u64 sum / min / max per field, reduced on
the device per chunk and again over the chunks) no record returns to the host between ``insert`` and the file; a
callable ``merge(key, values) -> bytes`` is applied on the host to the groups of two or more
values, never to a group of one (:166-170).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, codec, encode
from .encode import DeviceRecords
from .merger import MODES, Grouped, _records_list, merge_all  # noqa: F401  (merge_all: looked up here at call time)
from .reduce import MergeError, Reduce, as_reduce, check_merge  # noqa: F401
from .writer import CompressionType

DEFAULT_NB_CHUNKS, MIN_NB_CHUNKS = 25, 1                              # src/lib.rs:11-12
DEFAULT_SORTER_MEMORY, MIN_SORTER_MEMORY = 1_073_741_824, 10_485_760  # :13-14
INITIAL_SORTER_VEC_SIZE = 131_072                                     # :15
DEFAULT_COMPRESSION_LEVEL = 0                                         # :8
ENTRY_SIZE = 32   # size_of::<Entry>() on 64-bit: a Vec<u8> (24) + key_len (8), src/sorter.rs:72-75


def sort_records(recs: DeviceRecords, mode, stream=None):
    """One mtblx_sort_plan + mtblx_sort_emit over one batch of records in any order -> Grouped for
    "groups", else DeviceRecords: keys ascending, one item per distinct key, the values of a key in
    input order, the empty-key group kept (no quirk here).  `mode` is a name of MODES, or a Reduce
    (or its shorthand name): then the emit is mtblx_sort_emit_reduce, with "first"'s layout, and a
    group of two or more holding a value of another length raises MergeError.  Workspace and
    outputs are allocated on the stream the kernels run on."""
    L = codec._require_device()
    red = as_reduce(mode)
    m = _lib.MERGE_FIRST if red is not None else MODES[mode]
    dev = recs.key_end.device
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(s):   # the caching allocator ties these blocks to the stream that uses them
        n = recs.n
        if n >= _lib.MERGE_MAX_RECORDS:
            raise ValueError("sort: 2^32 - 16 records or more")
        rec = recs.cstruct()
        wsb = int(L.mtblx_sort_workspace_bytes(n))
        ws = torch.empty(wsb + 256, dtype=torch.uint8, device=dev)
        wp = (ws.data_ptr() + 255) & ~255
        tot = (C.c_uint64 * 6)()
        sh = C.c_void_p(int(s.cuda_stream))
        rc = L.mtblx_sort_plan(C.byref(rec), tot, C.c_void_p(wp), wsb, sh)
        if rc != 0:
            raise RuntimeError(f"mtblx_sort_plan failed: {rc} (flags={int(tot[5])})")
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
            rc = L.mtblx_sort_emit_reduce(C.byref(rec), C.byref(spec), C.byref(out), C.c_void_p(wp), wsb, sh)
        else:
            rc = L.mtblx_sort_emit(C.byref(rec), m, C.byref(out), C.c_void_p(wp), wsb, sh)
        if rc != 0:
            raise RuntimeError(f"mtblx_sort_emit failed: {rc}")
        f = int(flags.item())   # synchronizes: the workspace may go back to the allocator after this
        if f & _lib.MERGE_BADVALUE:
            raise MergeError(f"merge: a group of two or more holds a value that is not {red.shape}")
        if f:
            raise RuntimeError(f"mtblx_sort_emit: flags={f}")
        if m in (_lib.MERGE_FIRST, _lib.MERGE_LAST) and groups:   # vals was sized by its upper bound
            vals = vals[: int(val_end[-1].item())]
    if grouped:
        return Grouped(keys, key_end, vals, val_end, grp_end, s)
    return DeviceRecords(keys, key_end, vals, val_end, s)


def _apply(merge, grouped: Grouped, device) -> DeviceRecords:
    """a callable merge function over MultiIter-shaped groups: groups of one pass through (:166-170);
    read back and uploaded again on the stream the groups were produced on"""
    return DeviceRecords.from_list([(k, vs[0] if len(vs) == 1 else bytes(merge(k, vs))) for k, vs in grouped.to_list()],
                                   device=device, stream=grouped.stream)


class SorterBuilder:
    """src/sorter.rs:25-70.  merge: "concat" | "first" | "last" | Reduce (or "sum_u64" | "min_u64" |
    "max_u64") | callable(key, values) -> bytes.
    Chunks stay in device memory, so the two chunk_compression settings are stored and unused."""

    def __init__(self, merge, device="cuda", stream=None):
        self._merge = check_merge(merge)
        self._device, self._stream = device, stream
        self._max_memory = DEFAULT_SORTER_MEMORY                  # :28
        self._max_nb_chunks = DEFAULT_NB_CHUNKS                   # :29
        self._chunk_compression_type = CompressionType.Snappy     # :30
        self._chunk_compression_level = DEFAULT_COMPRESSION_LEVEL  # :31

    def max_memory(self, memory: int) -> "SorterBuilder":
        self._max_memory = max(int(memory), MIN_SORTER_MEMORY)    # :37
        return self

    def max_nb_chunks(self, nb_chunks: int) -> "SorterBuilder":
        self._max_nb_chunks = max(int(nb_chunks), MIN_NB_CHUNKS)  # :44
        return self

    def chunk_compression_type(self, compression) -> "SorterBuilder":
        self._chunk_compression_type = compression                # :49 (no effect: no chunk files)
        return self

    def chunk_compression_level(self, level: int) -> "SorterBuilder":
        self._chunk_compression_level = int(level)                # :54 (no effect: no chunk files)
        return self

    def build(self) -> "Sorter":
        s = Sorter(self._merge, device=self._device, stream=self._stream)
        s.max_memory, s.max_nb_chunks = self._max_memory, self._max_nb_chunks
        s.chunk_compression_type, s.chunk_compression_level = self._chunk_compression_type, self._chunk_compression_level
        return s


class Sorter:
    """src/sorter.rs:95-258.  chunk_sizes: the records that went into each write_chunk, in order;
    merges: how often merge_chunks ran."""

    def __init__(self, merge, device="cuda", stream=None):   # Sorter::new (:112-114)
        self.merge = check_merge(merge)
        self.device, self.stream = torch.device(device), stream
        self.max_memory, self.max_nb_chunks = DEFAULT_SORTER_MEMORY, DEFAULT_NB_CHUNKS
        self.chunk_compression_type, self.chunk_compression_level = CompressionType.Snappy, DEFAULT_COMPRESSION_LEVEL
        self.chunks = []            # DeviceRecords, oldest first (:96)
        self.entry_bytes = 0        # :99
        # entries: Vec::with_capacity(INITIAL_SORTER_VEC_SIZE) (:61).  Only its len and capacity
        # enter the memory rule.  The capacity doubles when a push finds the Vec full and survives
        # drain(..): that is std's current amortised growth, an implementation detail of the
        # standard library and not a documented guarantee, emulated here because :131 reads it
        self._len, self._capacity = 0, INITIAL_SORTER_VEC_SIZE
        self._single = []           # (key, val) of insert() not yet packed into a piece
        self._pieces = []           # pending records in insertion order: (keys, key_end, vals, val_end), ENDs from 0
        self.chunk_sizes, self.merges = [], 0
        self._done = False

    def _s(self):
        """S of the stream contract: Sorter(stream=), else the stream current at the call.  Device
        batches handed to insert_batch must be ready on it; staging, sorts and merges all run on it."""
        return codec._stream_of(self.stream, self.device)

    @staticmethod
    def builder(merge, device="cuda", stream=None) -> SorterBuilder:   # :108-110
        return SorterBuilder(merge, device, stream)

    # ---- insert (:120-140)
    def _cut(self) -> None:
        self.write_chunk()                                  # :133
        if len(self.chunks) > self.max_nb_chunks:           # :134
            self.merge_chunks()                             # :135

    def insert(self, key, val) -> None:
        key, val = bytes(key), bytes(val)
        self.entry_bytes += len(key) + len(val)             # :128
        if self._len == self._capacity:                     # :129 push: amortised growth (see __init__)
            self._capacity *= 2
        self._len += 1
        self._single.append((key, val))
        if self.entry_bytes + self._capacity * ENTRY_SIZE >= self.max_memory:   # :131-132
            self._cut()

    def insert_batch(self, keys, key_end, vals, val_end) -> None:
        """n records as concatenated bytes + END offsets: host arrays as Writer.insert_batch takes
        them, or device tensors (uint8 / int64).  Same effect as insert() record by record; the
        cut positions come from the cumulative lengths, one step per cut or capacity doubling."""
        dev = isinstance(key_end, torch.Tensor)
        with torch.cuda.stream(self._s() if dev else None):   # the offset sums, searches and reads of a device batch
            self._insert_batch(keys, key_end, vals, val_end, dev)

    def _insert_batch(self, keys, key_end, vals, val_end, dev) -> None:
        if dev:
            ke, ve = key_end.to(torch.int64), val_end.to(torch.int64)
            cs = ke + ve
        else:
            keys, vals = np.ascontiguousarray(keys, np.uint8), np.ascontiguousarray(vals, np.uint8)
            ke, ve = np.asarray(key_end).astype(np.int64), np.asarray(val_end).astype(np.int64)
            cs = ke + ve
        n = int(ke.shape[0])

        def first_reaching(target: int, lo: int) -> int:
            """the first record index i >= lo whose END sum cs[i] >= target (n if none)"""
            if dev:
                i = int(torch.searchsorted(cs, torch.tensor([target], dtype=torch.int64, device=cs.device)).item())
            else:
                i = int(np.searchsorted(cs, target, side="left"))
            return max(i, lo)

        p = 0   # records of the batch consumed so far
        while p < n:
            if self._len == self._capacity:
                self._capacity *= 2
            room = self._capacity - self._len               # pushes that leave the capacity as it is
            before = int(cs[p - 1]) if p else 0
            need = self.max_memory - self._capacity * ENTRY_SIZE - self.entry_bytes   # bytes still to come before a cut
            i = first_reaching(before + need, p)            # record i is the one whose insert cuts
            last = min(p + room, n)                         # the segment [p, last) keeps this capacity
            if i < last:
                self._take(keys, ke, vals, ve, p, i + 1)
                self.entry_bytes += int(cs[i]) - before
                self._len += i + 1 - p
                p = i + 1
                self._cut()
            else:
                self._take(keys, ke, vals, ve, p, last)
                self.entry_bytes += int(cs[last - 1]) - before
                self._len += last - p
                p = last

    def _take(self, keys, ke, vals, ve, a: int, b: int) -> None:
        """records [a, b) of a batch become a pending piece"""
        if b <= a:
            return
        self._flush_single()
        k0, v0 = (int(ke[a - 1]), int(ve[a - 1])) if a else (0, 0)
        self._pieces.append((keys[k0: int(ke[b - 1])], ke[a:b] - k0, vals[v0: int(ve[b - 1])], ve[a:b] - v0))

    def _flush_single(self) -> None:
        if self._single:
            recs, self._single = self._single, []
            self._pieces.append((np.frombuffer(b"".join(k for k, _ in recs), np.uint8),
                                 np.cumsum([len(k) for k, _ in recs], dtype=np.int64),
                                 np.frombuffer(b"".join(v for _, v in recs), np.uint8),
                                 np.cumsum([len(v) for _, v in recs], dtype=np.int64)))

    def _pending(self) -> DeviceRecords:
        """the pending pieces joined, in insertion order, on the device"""
        self._flush_single()
        pieces, self._pieces = self._pieces, []

        def t(x, dtype):
            x = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x, copy=True))
            return x.to(device=self.device, dtype=dtype)

        ks, kes, vs, ves, kb, vb = [], [], [], [], 0, 0
        for k, ke, v, ve in pieces:
            ks.append(t(k, torch.uint8))
            vs.append(t(v, torch.uint8))
            kes.append(t(ke, torch.int64) + kb)
            ves.append(t(ve, torch.int64) + vb)
            kb += int(k.shape[0])
            vb += int(v.shape[0])
        z8, z64 = torch.zeros(0, dtype=torch.uint8, device=self.device), torch.zeros(0, dtype=torch.int64, device=self.device)
        return DeviceRecords(torch.cat(ks + [z8]), torch.cat(kes + [z64]), torch.cat(vs + [z8]), torch.cat(ves + [z64]))

    # ---- write_chunk (:142-197)
    def write_chunk(self) -> None:
        with torch.cuda.stream(self._s()):   # the pieces are joined on the stream that sorts them
            self._write_chunk(self._s())

    def _write_chunk(self, s) -> None:
        recs = self._pending()
        self.chunk_sizes.append(recs.n)
        if callable(self.merge):
            chunk = _apply(self.merge, sort_records(recs, "groups", s), self.device)   # :152-188
        else:
            chunk = sort_records(recs, self.merge, s)
        self.chunks.append(chunk)                           # :191
        self.entry_bytes = 0                                # :192
        self._len = 0                                       # :155 drain(..): the capacity stays

    def _merge_all(self) -> DeviceRecords:
        """a Merger over the chunks, oldest first (MergerIter with its empty-key quirk)"""
        s = self._s()
        if callable(self.merge):
            return _apply(self.merge, merge_all(self.chunks, "groups", s, self.device), self.device)
        return merge_all(self.chunks, self.merge, s, self.device)

    # ---- merge_chunks (:199-233)
    def merge_chunks(self) -> None:
        self.chunks = [self._merge_all()]                   # :211-228: the result is the only, hence the oldest, chunk
        self.merges += 1

    # ---- into_iter (:244-257)
    def records(self, where=None) -> DeviceRecords:
        """the sorted, merged stream on the device (what encode.write_file takes).  Consumes the Sorter.
        where (a where.Where): only the records whose MERGED value it keeps (filter_records)."""
        if self._done:
            raise RuntimeError("Sorter already consumed")
        if where is not None:
            from .where import as_where, filter_records
            as_where(where)                                 # refused before the Sorter is consumed
        self._done = True
        self.write_chunk()                                  # :246, also when nothing is pending
        r = self._merge_all()                               # :253-256; no merge_chunks here
        return r if where is None else filter_records(r, where, None, self._s()).records

    def into_iter(self):
        """MergerIter over the chunks: (key, merged value) per distinct key"""
        return iter(_records_list(self.records()))

    def write_file(self, block_size: int = 8192, restart_interval: int = 16,
                   compression: int = CompressionType.None_, where=None) -> torch.Tensor:
        """the .mtbl file (device uint8), written by the device Writer; where: as records(where=)"""
        s = self._s()
        with torch.cuda.stream(s):   # the last chunk, the merge and the Writer on one stream
            return encode.write_file(self.records(where), block_size, restart_interval, stream=s, compression=compression)

    def write_into(self, writer) -> None:
        """Sorter::write_into (:235-242) for the host Writer"""
        r = self.records()
        if r.n == 0:
            return
        with torch.cuda.stream(r.stream):
            writer.insert_batch(r.keys.cpu().numpy(), r.key_end.cpu().numpy().astype(np.uint64),
                                r.vals.cpu().numpy(), r.val_end.cpu().numpy().astype(np.uint64))

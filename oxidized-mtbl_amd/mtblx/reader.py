"""Reader / ReaderBuilder mirror over the device codec (reference src/reader.rs).

A whole .mtbl file is scanned on the GPU:

    ReaderBuilder::read   src/reader.rs:31-81   footer + index framing (host, a few bytes)
    index block           decoded on the device like any block (mtblx_decode_blocks)
    block_at_index        src/reader.rs:177-186 \\ all entries at once: mtblx_block_dir
    Reader::block framing src/reader.rs:139-157 /
    crc32c verify         src/reader.rs:159-164  mtblx_crc32c_blocks (framed), if verifying
    Block::init + scan    src/block.rs           mtblx_decode_blocks over the directory
    ReaderIntoIter::next  src/reader.rs:337-405  how the iteration ENDS is decided on the host
                                                 from the per-block statuses (below); the
                                                 records stay on the device

`Reader.iter()` returns a `Scan`: the records the reference iterator yields, in order, as a
prefix of the device output arrays, plus how the iteration ends (`end`: NONE / ERR_OPEN /
ERR_NEXT / PANIC / LOOP, the oracle's codes).  Errors the reference returns from
ReaderBuilder::read raise `MtblError` here.

Seek-based iteration -- iter_from / iter_prefix / iter_range (src/reader.rs:128-138) and the
stateful ReaderIntoIter with next() / seek() (:219-405) -- goes through the device index seek,
block_at_index and block seek, decoding only the blocks the iteration reaches (iterator.py).
get() is the device Reader::get (mtblx_get).

Compressed files: Reader::block's decompress step (src/reader.rs:166-170) runs on the device for
Snappy (mtblx_stage_plan / mtblx_stage_emit: the stored bytes stay where they are) and on the host
for Zlib / Zstd (mtblx_decompress_blocks).  get_batch / scan_batch / count_batch on a Snappy file
decompress only the blocks a batch touches when the index is regular and the directory ascends
(mtblx_scan_touch -> mtblx_bitmap_compact -> stage -> mtblx_table_gather: the on-demand table, its
bytes in an arena that grows by doubling), else every block once.  Reader.stage_stats counts both
sides; ReaderBuilder(snappy_stage="host") keeps the host path (DESIGN.md §4 "Snappy files in the
Reader").
"""
from __future__ import annotations

import contextlib
import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, codec

END_NONE, END_ERR_OPEN, END_ERR_NEXT, END_PANIC, END_LOOP = range(5)
ERR_NAMES = ["None", "InvalidMetadataSize", "InvalidIndexBlockOffset", "InvalidIndexLength",
             "InvalidFormatVersion", "InvalidCompressionAlgorithm", "InvalidBlock", "Io"]
METADATA_SIZE = 512


class MtblError(RuntimeError):
    """Err(Error::Mtbl(..)) of the reference (src/error.rs:44-52)."""

    def __init__(self, code: int):
        super().__init__(ERR_NAMES[code] if 0 <= code < len(ERR_NAMES) else str(code))
        self.code = code


class ReferencePanic(RuntimeError):
    """Where the reference panics (assert / unwrap / slice out of range)."""


class ReferenceLoop(RuntimeError):
    """Where the reference never returns (an entry that does not advance)."""


@dataclass
class Scan:
    end: int                 # END_*
    err: str                 # error name for END_ERR_*
    nrec: int                # records yielded
    keys: torch.Tensor       # device, key bytes of the yielded records (concatenated)
    vals: torch.Tensor
    key_end: torch.Tensor    # device int64 [nrec], global END offsets into keys
    val_end: torch.Tensor
    stream: object = None    # the stream the tensors were produced on (None: whatever is current at the read)

    def records(self):
        with torch.cuda.stream(self.stream):
            ke = self.key_end.cpu().numpy()
            ve = self.val_end.cpu().numpy()
            k = self.keys.cpu().numpy().tobytes()
            v = self.vals.cpu().numpy().tobytes()
        out, pk, pv = [], 0, 0
        for i in range(self.nrec):
            out.append((k[pk: ke[i]], v[pv: ve[i]]))
            pk, pv = int(ke[i]), int(ve[i])
        return out


class ScanBatch:
    """Reader.scan_batch's result.  Device tensors: `keys` / `vals` (the records of the queries the
    kernels served, in query order), `key_end` / `val_end` (int64 END offsets from record 0 of the
    batch: with keys / vals an mtblx_records), `rec_off` (int64 [nq + 1]: query q's records are
    [rec_off[q], rec_off[q + 1])), `status` (int32 [nq], SCAN_*).  Queries that are not SCAN_OK were
    answered by iterator.bulk(); scan(q) / records(q) give every query's result, whichever path
    served it."""

    def __init__(self, nq, keys, vals, key_end, val_end, rec_off, status, host, served, stream=None):
        self._stream = stream      # the stream of the scan: scan(q) / records(q) work and read on it
        self.nq, self.keys, self.vals, self.key_end, self.val_end = nq, keys, vals, key_end, val_end
        self.rec_off, self.status = rec_off, status
        self._res = host           # mtblx_scan_result per query (host)
        self._served = served      # q -> Scan of the queries bulk() answered
        self._host = None
        self.n_large = int((host["status"] == _lib.SCAN_LARGE).sum())
        self.n_fallback = int((host["status"] == _lib.SCAN_FALLBACK).sum())

    def served_by_kernel(self, q: int) -> bool:
        return q not in self._served

    def scan(self, q: int) -> Scan:
        """query q as iter_from / iter_prefix / iter_range would return it"""
        if q in self._served:
            return self._served[q]
        r = self._res[q]
        r0, n = int(r["rec_base"]), int(r["nrec"])
        k0, v0 = int(r["key_base"]), int(r["val_base"])
        with torch.cuda.stream(self._stream):   # the offset shifts are kernels
            return Scan(END_NONE, "None", n, self.keys[k0: k0 + int(r["key_bytes"])],
                        self.vals[v0: v0 + int(r["val_bytes"])], self.key_end[r0: r0 + n] - k0,
                        self.val_end[r0: r0 + n] - v0, self._stream)

    def records(self, q: int):
        """query q's (key, value) pairs on the host (the batch is copied once)"""
        if q in self._served:
            return self._served[q].records()
        if self._host is None:
            with torch.cuda.stream(self._stream):
                self._host = (self.keys.cpu().numpy().tobytes(), self.vals.cpu().numpy().tobytes(),
                              self.key_end.cpu().numpy(), self.val_end.cpu().numpy())
        k, v, ke, ve = self._host
        r = self._res[q]
        r0, pk, pv = int(r["rec_base"]), int(r["key_base"]), int(r["val_base"])
        out = []
        for i in range(r0, r0 + int(r["nrec"])):
            out.append((k[pk: ke[i]], v[pv: ve[i]]))
            pk, pv = int(ke[i]), int(ve[i])
        return out


def prefix_bound(prefix: bytes):
    """the smallest key above every key that starts with `prefix` (its last non-0xff byte
    incremented, the tail dropped), or None when there is none (empty or all 0xff): the bound
    mtblx_scan_touch takes for an iter_prefix query"""
    p = bytes(prefix).rstrip(b"\xff")
    if not p:
        return None
    return p[:-1] + bytes([p[-1] + 1])


class ReaderBuilder:
    """src/reader.rs:15-30: verify_checksums defaults to true.  snappy_stage: where the blocks of a
    Snappy file are decompressed: "device" (mtblx_stage_*, the stored bytes never leave the GPU) or
    "host" (mtblx_decompress_blocks on CPU threads: the A/B baseline)."""

    def __init__(self, snappy_stage: str = "device"):
        self._verify = True
        self.snappy_stage(snappy_stage)

    def verify_checksums(self, verify: bool) -> "ReaderBuilder":
        self._verify = bool(verify)
        return self

    def snappy_stage(self, where: str) -> "ReaderBuilder":
        if where not in ("device", "host"):
            raise ValueError(f"snappy_stage: {where!r} (\"device\" or \"host\")")
        self._snappy_stage = where
        return self

    def read(self, data, device="cuda") -> "Reader":
        return Reader(data, self._verify, device, snappy_stage=self._snappy_stage)


class _OnDemand:
    """the on-demand table of a Snappy file: which directory entries are resident (bitmap), their
    per-ordinal rows, the arena their decompressed bytes live in and the compact table built from
    them"""

    def __init__(self, nent: int, eoffs: torch.Tensor, dev):
        self.nwords = (nent + 31) // 32
        self.eoffs = eoffs
        self.resident = torch.zeros(self.nwords, dtype=torch.int32, device=dev)
        self.row_start = torch.zeros(nent, dtype=torch.int64, device=dev)
        self.row_doff = torch.zeros(nent, dtype=torch.int64, device=dev)
        self.row_dlen = torch.zeros(nent, dtype=torch.int64, device=dev)
        self.row_st = torch.zeros(nent, dtype=torch.int32, device=dev)
        self.arena = torch.empty(16, dtype=torch.uint8, device=dev)
        self.used = 0
        self.nres = 0
        z64 = torch.zeros(0, dtype=torch.int64, device=dev)
        self.table = (z64, z64, z64, torch.zeros(0, dtype=torch.int32, device=dev), 0, self.arena)


class Reader:
    def __init__(self, data, verify_checksums: bool = True, device="cuda", snappy_stage: str = "device"):
        codec._require_device()
        if snappy_stage not in ("device", "host"):
            raise ValueError(f"snappy_stage: {snappy_stage!r} (\"device\" or \"host\")")
        if isinstance(data, torch.Tensor):
            self.file = data.to(device=device, dtype=torch.uint8).contiguous()
            host = None
        else:
            host = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else \
                np.ascontiguousarray(data, np.uint8)
            self.file = torch.from_numpy(host.copy()).to(device) if host.size else \
                torch.zeros(1, dtype=torch.uint8, device=device)
        self.len = int(host.size) if host is not None else int(self.file.numel())
        self.verify = verify_checksums
        L = _lib.lib()
        # ReaderBuilder::read (src/reader.rs:31-81): footer, index framing + checksum (host)
        if self.len < METADATA_SIZE:
            raise MtblError(1)
        tail = host[self.len - METADATA_SIZE:] if host is not None else \
            self.file[self.len - METADATA_SIZE:].cpu().numpy()
        f = _lib.Footer()
        # mtblx_read_footer wants the whole file for its offset check; a 512-byte view plus
        # the length is enough: pass a buffer whose last 512 bytes are the footer
        buf = np.zeros(self.len, np.uint8) if host is None else host
        if host is None:
            buf[self.len - METADATA_SIZE:] = tail
        rc = L.mtblx_read_footer(buf.ctypes.data_as(_lib.u8p), self.len, C.byref(f))
        if rc != 0:
            raise MtblError(int(f.err))
        self.meta = list(f.meta)
        self.version = int(f.version)
        self.compression = int(self.meta[2])   # 0..5 (read_footer rejects others: InvalidCompressionAlgorithm)
        self._snappy_dev = self.compression == 1 and snappy_stage == "device"
        self._nhost = 0        # blocks decompressed on the host
        self._ndev = 0         # blocks decompressed on the device
        self._od = None        # _OnDemand, False = not applicable (full table), None = not decided
        self._dtab = None
        idx_off = int(self.meta[0])
        if host is None:   # index block bytes to the host (framing + checksum)
            hi = self.len - METADATA_SIZE
            buf[idx_off:hi] = self.file[idx_off:hi].cpu().numpy()
        coff, clen, panic = C.c_uint64(0), C.c_uint64(0), C.c_int(0)
        rc = L.mtblx_frame_block(buf.ctypes.data_as(_lib.u8p), self.len, self.version, idx_off,
                                 1 if verify_checksums else 0, C.byref(coff), C.byref(clen), C.byref(panic))
        if panic.value:
            raise ReferencePanic("index block framing / checksum (src/reader.rs:52-74)")
        if rc != 0:
            raise MtblError(3)
        self.index_off, self.index_len = int(coff.value), int(clen.value)
        # index block on the device
        self._ibatch = codec.DeviceBatch(self.file, torch.tensor([coff.value], dtype=torch.int64, device=device),
                                         torch.tensor([clen.value], dtype=torch.int32, device=device),
                                         int(clen.value))
        self.index = codec.decode_blocks(self._ibatch)
        ist = int(self.index.status[0].item())   # synchronises the current stream, which ran the decode
        # the decoded index is complete from here on and is read by calls on any stream: its host
        # reads use the stream current at the read, not the constructor's (a call must not wait for that one)
        self.index._stream = None
        if ist == _lib.ST_INVALID_BLOCK:
            raise MtblError(6)   # Block::init(index) -> InvalidBlock (src/reader.rs:76)
        self.index_status = ist
        self.nent = int(self.index.totals_host()[0])
        self._dir = None
        self._dir3 = None
        self._scan = None
        self._eoffs = None
        self._regular = None
        self._ikeys = None
        self._irecs = None

    # ------------------------------------------------------------------ streams ("Streams")
    def _s(self, stream):
        """S of the stream contract: `stream`, or the stream current on the file's device"""
        return codec._stream_of(stream, self.file.device)

    def _settle(self) -> None:
        """Device state the Reader keeps across calls (the directory, the cached scan, the
        decompressed-block tables and the on-demand arena) is built on the stream of the call that
        first needs it and read by later calls on any stream: whoever builds or changes it drains
        that stream once, so the state is complete before another stream can see it.  It drains
        the CURRENT stream: correct only where the builder already runs under torch.cuda.stream(S),
        as every public entry point arranges; a builder called outside that context would drain
        the wrong stream."""
        torch.cuda.current_stream(self.file.device).synchronize()

    # ------------------------------------------------------------------ directory
    def directory(self):
        """(blk_off int64, blk_len int32, dir_status int32, crc_bad uint8|None) on the device,
        one entry per index record."""
        if self._dir is None:
            off, ln, st = self._framing()
            self._dir = (off, ln, st, self._bad_range(0, self.nent))
        return self._dir

    def _bad_range(self, i0: int, i1: int):
        """Reader::block's checksum assert for directory entries [i0, i1) (device uint8), or
        None when not verifying"""
        if not self.verify or i1 <= i0:
            return None
        off, ln, _ = self._framing()
        batch = codec.DeviceBatch(self.file, off[i0:i1], ln[i0:i1], codec.u32_max(ln[i0:i1]))
        return codec.crc32c_blocks(batch, framed=True)[1]

    def _framing(self):
        """block_at_index + Reader::block framing of every index entry: (off, len, status)"""
        if self._dir3 is None:
            n = max(self.nent, 1)
            dev = self.file.device
            off = torch.zeros(n, dtype=torch.int64, device=dev)
            ln = torch.zeros(n, dtype=torch.int32, device=dev)
            st = torch.zeros(n, dtype=torch.int32, device=dev)
            L = _lib.lib()
            if self.nent:
                rc = L.mtblx_block_dir(C.c_void_p(self.file.data_ptr()), self.len, self.version,
                                       C.c_void_p(self.index.vals.data_ptr()), C.c_void_p(self.index.val_end.data_ptr()),
                                       0, self.nent, C.c_void_p(off.data_ptr()), C.c_void_p(ln.data_ptr()),
                                       C.c_void_p(st.data_ptr()), C.c_void_p(codec._stream_handle(None)))
                if rc != 0:
                    raise RuntimeError(f"mtblx_block_dir failed: {rc}")
            self._dir3 = (off[: self.nent], ln[: self.nent], st[: self.nent])
            self._settle()
        return self._dir3

    # ------------------------------------------------------------------ iteration
    def _host_stage(self, off, ln, st):
        """Reader::block's decompression step (src/reader.rs:166-170 -> src/compression.rs:57-68)
        on the host for every block the directory frames, any CompressionType:
        mtblx_decompress_blocks (16 threads; codecs_host.cpp).  A decoder error is the crate's
        Err(Error::Io); Lz4 / Lz4hc are its Err "unsupported" (also Error::Io)."""
        L = _lib.lib()
        host = self.file.cpu().numpy()
        o = off.cpu().numpy().view(np.uint64).copy()
        n = ln.cpu().numpy().view(np.uint32).copy()
        ok = st.cpu().numpy() == _lib.DIR_OK
        n[~ok] = 0
        o[~ok] = 0
        nb = o.size
        self._nhost += int(ok.sum())
        dst = _lib.u8p()
        doff = np.zeros(max(nb, 1), np.uint64)
        dlen = np.zeros(max(nb, 1), np.uint64)
        zst = np.zeros(max(nb, 1), np.int32)
        L.mtblx_decompress_blocks(self.compression, host.ctypes.data, o.ctypes.data, n.ctypes.data, nb, 16,
                                  C.byref(dst), doff.ctypes.data, dlen.ctypes.data, zst.ctypes.data)
        total = int(doff[nb - 1]) + ((int(dlen[nb - 1]) + 15) & ~15) if nb else 0
        buf = np.empty(max(total, 16), np.uint8)
        C.memmove(buf.ctypes.data, dst, total)
        L.mtblx_free(dst)
        zerr = zst[:nb].copy()
        zerr[~ok] = 0
        # u64 lengths: a content >= 4 GiB is not decoded by the batched call (u32 lengths) but by
        # the emitting block seek on its bytes in the uploaded buffer (_big_content)
        return buf, doff[:nb].copy(), dlen[:nb].copy(), zerr

    def iter(self) -> Scan:
        """ReaderIntoIter (mode Iter) to the end: the records yielded and how it ends."""
        if self._scan is not None:
            return self._scan
        from . import iterator
        n = self.nent
        end, err = END_NONE, "None"
        if n == 0:   # ReaderIntoIter::new with no index entry; a corrupt index panics at its first
            end = END_PANIC if self.index_status == _lib.ST_CORRUPT else END_NONE
            self._scan = iterator._assemble([], end, err, self.file.device)
            self._settle()
            return self._scan
        parts, end, err, stopped = self._walk_blocks(0, n, first_exempt=True)
        if not stopped:
            if self.index_status == _lib.ST_CORRUPT:
                end = END_PANIC          # the index iterator panics advancing past its last entry
            elif self.index_status == _lib.ST_LOOP:
                end = END_LOOP
        self._scan = iterator._assemble(parts, end, err, self.file.device)
        self._settle()
        return self._scan

    def _walk_blocks(self, i0: int, i1: int, first_exempt: bool):
        """ReaderIntoIter::next over directory entries [i0, i1) (src/reader.rs:337-405):
        Reader::block's framing / checksum / decompression, Block::init, the scan; an empty
        block loaded by next() ends the iteration (first_exempt: block i0 came from
        ReaderIntoIter::new, whose Err is an Err at open and whose emptiness does not end it).
        Blocks >= 4 GiB are decoded one by one (_big_block) and spliced in.
        -> (parts [(keys, vals, key_end, val_end, nrec)], end, err, stopped)"""
        dst, bad, zerr, data, (base, boff, blen) = self._decode_range(i0, i1)
        n = i1 - i0
        bst = data.status[:n].cpu().numpy()
        bnr = data.nrec[:n].cpu().numpy().astype(np.int64)
        parts, seg, take_last = [], 0, 0
        end, err, stopped = END_NONE, "None", False

        def errend(i):
            return END_ERR_OPEN if (first_exempt and i == 0) else END_ERR_NEXT

        i = 0
        while i < n:
            # content >= 4 GiB (u64 restart array): stored that big (DIR_UNSUPPORTED: framed,
            # checked and decompressed by _big_block), or decompressed that big (_big_content)
            big_dec = dst[i] == _lib.DIR_OK and not bad[i] and not zerr[i] and int(blen[i]) > 0xFFFFFFFF
            if dst[i] == _lib.DIR_UNSUPPORTED or big_dec:
                parts.append(self._slice(data, seg, i, 0))
                seg = i + 1
                kind, em = (self._big_content((base, int(boff[i]), int(blen[i]))) if big_dec
                            else self._big_block(i0 + i))
                if kind == "panic":
                    end, stopped = END_PANIC, True
                    break
                if kind == "loop":
                    end, stopped = END_LOOP, True
                    break
                if kind != "ok":
                    end, err, stopped = errend(i), kind, True
                    break
                if em.nrec == 0 and em.end == _lib.EMIT_END and not (first_exempt and i == 0):
                    stopped = True
                    break
                parts.append((em.keys, em.vals, em.key_end, em.val_end, em.nrec))
                if em.end in (_lib.EMIT_PANIC, _lib.EMIT_LOOP):
                    end, stopped = (END_PANIC if em.end == _lib.EMIT_PANIC else END_LOOP), True
                    break
                i += 1
                continue
            if dst[i] != _lib.DIR_OK or bad[i]:        # Reader::block panics (framing / checksum)
                end, stopped = END_PANIC, True
                break
            if zerr[i]:                                # decompress -> Err(Error::Io) (src/reader.rs:166)
                end, err, stopped = errend(i), "Io", True
                break
            st = int(bst[i])
            if st == _lib.ST_INVALID_BLOCK:
                end, err, stopped = errend(i), "InvalidBlock", True
                break
            if st == _lib.ST_UNSUPPORTED:     # the batch carries u32 lengths: cannot happen
                raise RuntimeError("batched decode: block >= 4 GiB")
            if st == _lib.ST_OK and bnr[i] == 0 and not (first_exempt and i == 0):
                stopped = True                         # an empty block ends the iteration (:362-371)
                break
            if st in (_lib.ST_CORRUPT, _lib.ST_LOOP):  # the records before the panic / loop, then stop
                take_last = int(bnr[i])
                end, stopped = (END_PANIC if st == _lib.ST_CORRUPT else END_LOOP), True
                break
            i += 1
        parts.append(self._slice(data, seg, i, take_last))
        return parts, end, err, stopped

    def _slice(self, d, i0: int, i1: int, take_last: int):
        """records of decoded blocks [i0, i1) plus the first take_last records of block i1
        -> (keys, vals, key_end, val_end, nrec) on the device, END offsets from the slice start"""
        dev = self.file.device
        nb_used = i1 - i0 + (1 if take_last else 0)
        z = torch.zeros(0, dtype=torch.uint8, device=dev)
        e = torch.zeros(0, dtype=torch.int64, device=dev)
        if d is None or nb_used <= 0:
            return z, z, e, e, 0
        counts = d.nrec[i0: i0 + nb_used].to(torch.int64).clone()
        if take_last:
            counts[-1] = take_last
        nrec = int(counts.sum().item())
        if nrec == 0:
            return z, z, e, e, 0
        r0 = int(d.rec_base[i0].item())
        kb = d.key_base[i0: i0 + nb_used]
        vb = d.val_base[i0: i0 + nb_used]
        k0, v0 = int(kb[0].item()), int(vb[0].item())
        blk_of = torch.repeat_interleave(torch.arange(nb_used, device=dev), counts)
        m32 = 0xFFFFFFFF
        key_end = kb[blk_of] - k0 + (d.key_end[r0: r0 + nrec].to(torch.int64) & m32)
        val_end = vb[blk_of] - v0 + (d.val_end[r0: r0 + nrec].to(torch.int64) & m32)
        klen = int(key_end[-1].item())
        vlen = int(val_end[-1].item())
        return d.keys[k0: k0 + klen], d.vals[v0: v0 + vlen], key_end, val_end, nrec

    def _big_frame(self, i: int):
        """Reader::block framing of directory entry i from its index value (host, a few bytes)
        -> (block offset, content start, content length, stored crc)"""
        return self._big_frame_value(self._index_records()[i][1])

    def _big_frame_value(self, v: bytes):
        L = _lib.lib()
        off = C.c_uint64(0)
        vb = np.frombuffer(v or b"\0", np.uint8)
        L.mtblx_varint_decode64(vb.ctypes.data_as(_lib.u8p), len(v), C.byref(off))
        off = int(off.value)
        head = self.file[off: off + 14].cpu().numpy()
        if self.version == 0:
            ll, size = 4, int.from_bytes(head[:4].tobytes(), "little")
        else:
            sz = C.c_uint64(0)
            ll = int(L.mtblx_varint_decode64(head.ctypes.data_as(_lib.u8p), head.size, C.byref(sz)))
            size = int(sz.value)
        stored = int.from_bytes(head[ll: ll + 4].tobytes(), "little")
        return off, off + ll + 4, size, stored

    def _crc_big(self, start: int, size: int) -> int:
        """CRC-32C of file[start, start + size) for size >= 4 GiB: the device CRC of <= 1 GiB
        pieces, joined on the host with crc(A || B) = x^(8|B|) * crc(A) ^ crc(B) (mod P)"""
        piece = 1 << 30
        offs = list(range(start, start + size, piece))
        lens = [min(piece, start + size - o) for o in offs]
        dev = self.file.device
        batch = codec.DeviceBatch(self.file, torch.tensor(offs, dtype=torch.int64, device=dev),
                                  torch.tensor(lens, dtype=torch.int32, device=dev), max(lens))
        crcs = codec.crc32c_blocks(batch)[0].cpu().numpy().view(np.uint32)
        c = int(crcs[0])
        for k in range(1, len(lens)):
            c = _gf2_mul(_x8n(lens[k]), c) ^ int(crcs[k])
        return c

    def _big_block(self, i: int):
        """Reader::block + Block::init + the scan for a block >= 4 GiB (u64 restart array,
        src/block.rs:25-42): decoded on the device by the emitting block seek (seek_to_first).
        -> ("ok", Emitted) | ("panic", None) | ("loop", None) | (error name, None)"""
        return self._big_block_value(self._index_records()[i][1])[:2]

    def _big_block_value(self, value: bytes):
        off, start, size, stored = self._big_frame_value(value)
        if start > self.len or size > self.len - start:
            return "panic", None, None
        if self.verify and self._crc_big(start, size) != stored:
            return "panic", None, None                 # assert_eq of the checksum (src/reader.rs:163)
        if self.compression == 0:
            content = (self.file, start, size)
        else:
            try:                                       # src/reader.rs:166-170 (host, any size)
                content = self._decompressed(start, size)
            except MtblError:
                return "Io", None, None
        return self._big_content(content) + (content,)

    def _big_content(self, content):
        """Block::init + the scan of a content >= 4 GiB (tensor, off, len) on the device"""
        from . import iterator
        em = iterator.block_seek(content, None, 0, small_caps=True)
        if em.status == _lib.SEEK_ERR:
            return "InvalidBlock", None
        if em.status == _lib.SEEK_PANIC:
            return "panic", None
        if em.status == _lib.SEEK_LOOP:
            return "loop", None
        if em.status == _lib.SEEK_UNSUPPORTED:
            raise RuntimeError("emitting seek: key buffer too small")
        return "ok", em

    # ------------------------------------------------------------------ point queries
    def _dec_table(self):
        """Every data block the directory frames, decompressed on the host (Reader::block's
        decompress step, src/reader.rs:166-170), on the device, with the table
        mtblx_get_decompressed takes: sorted by stored content start."""
        if self._snappy_dev:
            od = self._on_demand()
            if od:
                return od.table
            if self._dtab is None:   # the full table, staged on the device
                off, ln, st = self._framing()
                buf, _, _, (ts, tdo, tdl, tst), _ = self._stage_all(off, ln, st, None)
                ok = st == _lib.DIR_OK
                ts, tdo, tdl, tst = ts[ok], tdo[ok], tdl[ok], tst[ok]
                order = torch.argsort(ts, stable=True)
                self._dtab = (ts[order], tdo[order], tdl[order], tst[order], int(order.numel()), buf)
                self._settle()
            return self._dtab
        if self._dtab is None:
            off, ln, st = self._framing()
            buf, doff, dlen, zerr = self._host_stage(off, ln, st)
            start = off.cpu().numpy().view(np.uint64)
            ok = st.cpu().numpy() == _lib.DIR_OK
            start, doff, dlen = start[ok], doff[ok], dlen[ok]
            zst = zerr[ok].astype(np.int32)
            order = np.argsort(start, kind="stable")
            dev = self.file.device
            t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)
            self._dtab = (t(start[order], np.int64), t(doff[order], np.int64), t(dlen[order], np.int64),
                          t(zst[order], np.int32), int(order.size), torch.from_numpy(buf).to(dev))
            self._settle()
        return self._dtab

    def _dtab_add(self, starts, sizes):
        """decompress stored blocks [start, + size) the table lacks (a get_batch seek landed on
        them: MTBLX_GET_MISSING) and add them to the table"""
        ts, tdo, tdl, tst, n, dec = self._dec_table()
        L = _lib.lib()
        self._nhost += len(starts)
        parts, base = [], int(dec.numel())
        s0, o0, l0, z0 = [], [], [], []
        for a, n_ in zip(starts, sizes):
            raw = self.file[int(a): int(a) + int(n_)].cpu().numpy()
            out = _lib.u8p()
            un = C.c_uint64(0)
            src = raw if raw.size else np.zeros(1, np.uint8)
            ok = L.mtblx_decompress(self.compression, src.ctypes.data, raw.size, C.byref(out), C.byref(un)) == 0
            b = np.empty(int(un.value) if ok else 0, np.uint8)
            if ok:
                C.memmove(b.ctypes.data, out, int(un.value))
                L.mtblx_free(out)
            s0.append(int(a)); o0.append(base); l0.append(b.size); z0.append(0 if ok else 1)
            parts.append(b)
            base += b.size
        dev = self.file.device
        start = np.concatenate([ts.cpu().numpy(), np.array(s0, np.int64)])
        doff = np.concatenate([tdo.cpu().numpy(), np.array(o0, np.int64)])
        dlen = np.concatenate([tdl.cpu().numpy(), np.array(l0, np.int64)])
        zst = np.concatenate([tst.cpu().numpy(), np.array(z0, np.int32)])
        order = np.argsort(start, kind="stable")
        t = lambda a_: torch.from_numpy(np.ascontiguousarray(a_)).to(dev)
        extra = torch.from_numpy(np.concatenate(parts) if parts else np.zeros(0, np.uint8)).to(dev)
        self._dtab = (t(start[order]), t(doff[order]), t(dlen[order]), t(zst[order]), int(order.size),
                      torch.cat([dec, extra]))
        self._settle()

    # ------------------------------------------------------------------ device staging (Snappy)
    def _stage_plan(self, off, ln, st, bad, sel, stream=None):
        """mtblx_stage_plan over a directory (device tensors; sel: int32 ordinals or None)
        -> (workspace, its size, (layout bytes, largest decompressed length, corrupt preambles))"""
        L = _lib.lib()
        ndir = int(off.numel())
        n = int(sel.numel()) if sel is not None else ndir
        wsb = int(L.mtblx_stage_workspace_bytes(n))
        ws = torch.empty(wsb, dtype=torch.uint8, device=self.file.device)   # the caching allocator aligns to 512 bytes
        totals = (C.c_uint64 * 3)()
        rc = L.mtblx_stage_plan(C.c_void_p(self.file.data_ptr()), self.len, C.c_void_p(codec._u(off)),
                                C.c_void_p(codec._u(ln)), C.c_void_p(codec._u(st)),
                                C.c_void_p(codec._u(bad)) if bad is not None else None, ndir,
                                C.c_void_p(codec._u(sel)) if sel is not None else None, n if sel is not None else 0,
                                totals, C.c_void_p(ws.data_ptr()), wsb, C.c_void_p(codec._stream_handle(stream)))
        if rc != 0:
            raise RuntimeError(f"mtblx_stage_plan failed: {rc}")
        return ws, wsb, [int(x) for x in totals]

    def _stage_emit(self, off, sel, ws, wsb, totals, dst, base, doff, dlen, tab, by_ordinal, stream=None):
        ndir = int(off.numel())
        n = int(sel.numel()) if sel is not None else ndir
        p = lambda t: C.c_void_p(codec._u(t)) if t is not None else None   # noqa: E731
        tab = tab if tab is not None else (None, None, None, None)
        rc = _lib.lib().mtblx_stage_emit(C.c_void_p(self.file.data_ptr()), self.len, p(off), ndir, p(sel),
                                         n if sel is not None else 0, C.c_void_p(dst.data_ptr()), int(dst.numel()),
                                         base, totals[0], min(totals[1], 0xFFFFFFFF), p(doff), p(dlen), p(tab[0]),
                                         p(tab[1]), p(tab[2]), p(tab[3]), 1 if by_ordinal else 0,
                                         C.c_void_p(ws.data_ptr()), wsb, C.c_void_p(codec._stream_handle(stream)))
        if rc != 0:
            raise RuntimeError(f"mtblx_stage_emit failed: {rc}")

    def _stage_all(self, off, ln, st, bad, stream=None):
        """Reader::block's decompression step for every entry of a directory, on the device
        -> (decompressed bytes, offsets int64 [n], lengths int32 [n] (0: failed or skipped),
        table rows (start, offset, length, Err(Io)) [n], largest length); nothing is read back"""
        dev = self.file.device
        n = int(off.numel())
        ws, wsb, totals = self._stage_plan(off, ln, st, bad, None, stream)
        buf = torch.empty(max(totals[0], 16), dtype=torch.uint8, device=dev)
        doff = torch.zeros(n, dtype=torch.int64, device=dev)
        dlen = torch.zeros(n, dtype=torch.int32, device=dev)
        tab = (torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev),
               torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))
        self._stage_emit(off, None, ws, wsb, totals, buf, 0, doff, dlen, tab, False, stream)
        self._ndev += n
        return buf, doff, dlen, tab, totals[1]

    def _on_demand(self):
        """the on-demand table's state, or False where it does not apply: the index must be
        regular (a seek lands on the scan chain: entry i <-> directory ordinal i) and the stored
        content starts must ascend with the ordinal (mtblx_dir_ascends, once per Reader)"""
        if self._od is None:
            self._od = False
            eoffs, regular = self._index_chain()
            if self._snappy_dev and regular and self.nent and eoffs.size == self.nent:
                dev = self.file.device
                off, ln, st = self._framing()
                viol = torch.zeros(1, dtype=torch.int32, device=dev)
                rc = _lib.lib().mtblx_dir_ascends(C.c_void_p(off.data_ptr()), C.c_void_p(st.data_ptr()), self.nent,
                                                  C.c_void_p(viol.data_ptr()), C.c_void_p(codec._stream_handle(None)))
                if rc != 0:
                    raise RuntimeError(f"mtblx_dir_ascends failed: {rc}")
                if int(viol.item()) == 0:
                    self._od = _OnDemand(self.nent, torch.from_numpy(np.ascontiguousarray(eoffs, np.int64)).to(dev), dev)
                    self._settle()
        return self._od

    @property
    def table_mode(self):
        """how point queries on this compressed file find their blocks: "on-demand" (only the
        blocks queries touched are decompressed), "full" (every block), None (not compressed)"""
        if self.compression == 0:
            return None
        return "on-demand" if self._snappy_dev and self._on_demand() else "full"

    @property
    def stage_stats(self):
        """counters of the decompression step: blocks decompressed on the host and entries handed
        to the device stage so far (the ones it skips included), blocks resident in the point-query
        table, and the bytes of its arena (allocated / used)"""
        od = self._od if self._snappy_dev else None
        if od:
            res, arena, used = od.nres, int(od.arena.numel()), od.used
        elif self._dtab is not None:
            res, arena = self._dtab[4], int(self._dtab[5].numel())
            used = arena
        else:
            res = arena = used = 0
        return {"host_blocks": self._nhost, "device_blocks": self._ndev, "resident_blocks": res,
                "arena_bytes": arena, "arena_used": used}

    def _od_touch(self, kb, ke, k2b, k2e, caps, cap_all, nq, stream=None):
        """touch -> compact -> stage what is not resident -> rebuild the compact table"""
        od = self._od
        if nq == 0:
            return
        ctx = torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
        with ctx:
            want = torch.zeros(od.nwords, dtype=torch.int32, device=self.file.device)
            p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
            rc = _lib.lib().mtblx_scan_touch(C.c_void_p(self.file.data_ptr()), self.len, self.index_off, self.index_len,
                                             p(od.eoffs), self.nent, p(kb), p(ke), p(k2b), p(k2e), p(caps), cap_all, nq,
                                             p(want), od.nwords, C.c_void_p(codec._stream_handle(stream)))
            if rc != 0:
                raise RuntimeError(f"mtblx_scan_touch failed: {rc}")
            self._od_stage(want, stream)

    def _od_stage(self, want, stream=None):
        """stage the entries of the bitmap `want` that are not resident into the arena"""
        od, dev, L = self._od, self.file.device, _lib.lib()
        sh = C.c_void_p(codec._stream_handle(stream))
        lst = torch.empty(self.nent, dtype=torch.int32, device=dev)
        cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        rc = L.mtblx_bitmap_compact(C.c_void_p(want.data_ptr()), C.c_void_p(od.resident.data_ptr()), self.nent,
                                    C.c_void_p(lst.data_ptr()), self.nent, C.c_void_p(cnt.data_ptr()), sh)
        if rc != 0:
            raise RuntimeError(f"mtblx_bitmap_compact failed: {rc}")
        n = int(cnt.item())
        if n == 0:
            return
        sel = lst[:n]
        off, ln, st = self._framing()
        ws, wsb, totals = self._stage_plan(off, ln, st, None, sel, stream)
        need = od.used + totals[0]
        if need > od.arena.numel():       # grows by doubling; offsets are relative to the base
            grown = torch.empty(max(2 * int(od.arena.numel()), need), dtype=torch.uint8, device=dev)
            grown[: od.used] = od.arena[: od.used]
            od.arena = grown
        self._stage_emit(off, sel, ws, wsb, totals, od.arena, od.used, None, None,
                         (od.row_start, od.row_doff, od.row_dlen, od.row_st), True, stream)
        od.used = need
        od.resident |= want
        self._ndev += n
        rc = L.mtblx_bitmap_compact(C.c_void_p(od.resident.data_ptr()), None, self.nent, C.c_void_p(lst.data_ptr()),
                                    self.nent, C.c_void_p(cnt.data_ptr()), sh)
        if rc != 0:
            raise RuntimeError(f"mtblx_bitmap_compact failed: {rc}")
        od.nres = m = int(cnt.item())
        ts = torch.empty(m, dtype=torch.int64, device=dev)
        tdo = torch.empty(m, dtype=torch.int64, device=dev)
        tdl = torch.empty(m, dtype=torch.int64, device=dev)
        tst = torch.empty(m, dtype=torch.int32, device=dev)
        rc = L.mtblx_table_gather(C.c_void_p(lst.data_ptr()), m, self.nent, C.c_void_p(off.data_ptr()),
                                  C.c_void_p(od.row_doff.data_ptr()), C.c_void_p(od.row_dlen.data_ptr()),
                                  C.c_void_p(od.row_st.data_ptr()), C.c_void_p(ts.data_ptr()),
                                  C.c_void_p(tdo.data_ptr()), C.c_void_p(tdl.data_ptr()), C.c_void_p(tst.data_ptr()), sh)
        if rc != 0:
            raise RuntimeError(f"mtblx_table_gather failed: {rc}")
        od.table = (ts, tdo, tdl, tst, m, od.arena)
        self._settle()   # the arena and the table changed: complete before a call on another stream reads them

    def _od_missing(self, starts, stream=None) -> bool:
        """a lookup reached stored blocks the on-demand table lacks (the touch is a hint): stage
        those that are directory entries; False when one is not (the caller builds the full table)"""
        od = self._od
        if getattr(self, "_starts_host", None) is None:
            self._starts_host = self._framing()[0].cpu().numpy()
        pos = np.searchsorted(self._starts_host, np.asarray(starts, np.int64))
        if (pos >= self.nent).any() or (self._starts_host[np.minimum(pos, self.nent - 1)] != starts).any():
            return False
        bits = np.zeros(od.nwords, np.uint32)
        np.bitwise_or.at(bits, pos >> 5, (np.uint32(1) << (pos & 31).astype(np.uint32)))
        ctx = torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
        with ctx:
            self._od_stage(torch.from_numpy(bits.view(np.int32)).to(self.file.device), stream)
        return True

    @property
    def value_source(self):
        """the device bytes get_batch's val_off / val_len point into: the file, or for a
        compressed file its decompressed blocks"""
        return self.file if self.compression == 0 else self._dec_table()[5]

    def get_batch(self, keys, stream=None):
        """Reader::get for every key at once on the device (mtblx_get / mtblx_get_decompressed,
        f2).  -> (status int32 [nq] (GET_*), val_off int64 [nq], val_len int64 [nq]) device
        tensors; the value of a FOUND query q is value_source[val_off[q] : val_off[q] +
        val_len[q]] (the file itself unless it is compressed).  Asynchronous on `stream` for an
        uncompressed file; a compressed one synchronises `stream` for the on-demand table."""
        stream = self._s(stream)
        with torch.cuda.stream(stream):   # queries, outputs, table work and the MISSING read-backs: all on `stream`
            return self._get_batch(keys, stream)

    def _get_batch(self, keys, stream):
        dev = self.file.device
        ks = [bytes(k) for k in keys]
        nq = len(ks)
        blob = b"".join(ks) or b"\0"
        # through pinned memory, without blocking: a copy from pageable memory would make the host wait
        # for everything queued on `stream` before it, and the uncompressed lookup only enqueues
        up = lambda a: torch.from_numpy(a).pin_memory().to(dev, non_blocking=True)   # noqa: E731
        kb = up(np.frombuffer(blob, np.uint8).copy())
        ke = up(np.cumsum([len(k) for k in ks], dtype=np.int64) if nq else np.zeros(1, np.int64))
        n = max(nq, 1)
        st = torch.zeros(n, dtype=torch.int32, device=dev)
        vo = torch.zeros(n, dtype=torch.int64, device=dev)
        vl = torch.zeros(n, dtype=torch.int64, device=dev)
        if self.compression == 0:
            rc = _lib.lib().mtblx_get(C.c_void_p(self.file.data_ptr()), self.len, self.version, 1 if self.verify else 0,
                                      self.index_off, self.index_len, C.c_void_p(kb.data_ptr()),
                                      C.c_void_p(ke.data_ptr()), nq, C.c_void_p(st.data_ptr()),
                                      C.c_void_p(vo.data_ptr()), C.c_void_p(vl.data_ptr()),
                                      C.c_void_p(codec._stream_handle(stream)))
        else:
            # a lookup that reaches a stored block the table lacks (MTBLX_GET_MISSING: only a
            # corrupt index read with verification off leads there) gets that block decompressed
            # and added, and the batch runs again; every round adds a block, so this ends
            if self._snappy_dev and self._on_demand():
                # Reader::get opens the block its key lands in and, when the seek runs past it, the next
                self._od_touch(kb, ke, kb, ke, None, 2, nq, stream)
            for _ in range(1 + 4096):
                ts, tdo, tdl, tst, ntab, dec = self._dec_table()
                rc = _lib.lib().mtblx_get_decompressed(
                    C.c_void_p(self.file.data_ptr()), self.len, self.version, 1 if self.verify else 0,
                    self.index_off, self.index_len, C.c_void_p(ts.data_ptr()), C.c_void_p(tdo.data_ptr()),
                    C.c_void_p(tdl.data_ptr()), C.c_void_p(tst.data_ptr()), ntab, C.c_void_p(dec.data_ptr()),
                    C.c_void_p(kb.data_ptr()), C.c_void_p(ke.data_ptr()), nq, C.c_void_p(st.data_ptr()),
                    C.c_void_p(vo.data_ptr()), C.c_void_p(vl.data_ptr()), C.c_void_p(codec._stream_handle(stream)))
                if rc != 0 or nq == 0:
                    break
                miss = (st[:nq] == _lib.GET_MISSING).cpu().numpy()
                if not miss.any():
                    break
                pairs = sorted(set(zip(vo[:nq].cpu().numpy()[miss].tolist(), vl[:nq].cpu().numpy()[miss].tolist())))
                if self._snappy_dev and self._od:
                    if not self._od_missing([a for a, _ in pairs], stream):
                        self._od = False   # a block outside the directory: the full table, then the host path
                    continue
                self._dtab_add([a for a, _ in pairs], [b for _, b in pairs])
            else:
                raise RuntimeError("get_batch: missing blocks did not converge")
        if rc != 0:
            raise RuntimeError(f"mtblx_get failed: {rc}")
        return st[:nq], vo[:nq], vl[:nq]

    def get(self, key: bytes):
        """Reader::get (src/reader.rs:111-122): the value of `key`, or None; raises where the
        reference panics / returns Err."""
        if self.compression != 0:   # values live in decompressed blocks: the seek-based iterator
            from . import iterator
            it = iterator.ReaderIntoIter(self, "get", bytes(key))
            held = it.bi
            try:
                rec = it.next()
            except MtblError:
                # next() returned Some(Err): Reader::get matches Some(_) and returns the OLD
                # block iterator's `val` (src/reader.rs:111-122, :376-379), or None
                return held.last_val if held is not None else None
            if rec is None:
                return None
            # Some((k, v)) with k != key is still Some(_): ReaderIntoGet over bi's val
            return rec[1] if rec[0] == bytes(key) else it.bi.recs[it.bi.pos][1]
        st, vo, vl = self.get_batch([key])
        s = int(st[0].item())
        if s == _lib.GET_FOUND:
            o, n = int(vo[0].item()), int(vl[0].item())
            return self.file[o: o + n].cpu().numpy().tobytes()
        if s == _lib.GET_NONE:
            return None
        if s == _lib.GET_ERR:
            raise MtblError(6)
        raise ReferencePanic("Reader::get" + (" never returns" if s == _lib.GET_LOOP else ""))

    def _sorted_keys(self):
        s = self.iter()
        return s, s.records()

    def get_prefix(self, prefix: bytes):
        """iter_prefix's records on the host"""
        return self.iter_prefix(prefix).records()

    def get_range(self, start: bytes, end: bytes):
        """iter_range's records on the host"""
        return self.iter_range(start, end).records()

    # ------------------------------------------------------------------ seek-based iteration
    def iter_from(self, key: bytes) -> Scan:
        """Reader::iter_from (src/reader.rs:128-130) run to the end, touching only the blocks
        from the sought one on."""
        from . import iterator
        return iterator.bulk(self, "from", bytes(key))

    def iter_prefix(self, prefix: bytes) -> Scan:
        """Reader::iter_prefix (src/reader.rs:132-134)"""
        from . import iterator
        return iterator.bulk(self, "prefix", bytes(prefix))

    def iter_range(self, start: bytes, end: bytes) -> Scan:
        """Reader::iter_range (src/reader.rs:136-138): start <= key <= end"""
        from . import iterator
        return iterator.bulk(self, "range", bytes(start), bytes(end))

    # ------------------------------------------------------------------ batched scans
    def _scan_plan(self, queries, max_blocks, max_records, stream, reduce=None, where=None):
        """mtblx_scan_plan over `queries` -> (res uint8 [nq * 64] device, totals, workspace, per-query
        limits, table arguments).  With a Reduce the call is mtblx_scan_reduce and the tuple ends with
        (fields int64 [nq, F], nbad int64 [nq]); with a Where too it is mtblx_scan_reduce_where and the
        last tuple is (fields, nbad, nmatch int64 [nq])."""
        from . import iterator
        dev = self.file.device
        nq = len(queries)
        qs = []
        for q in queries:
            kind = q[0]
            if kind not in ("from", "get", "prefix", "range") or len(q) != (3 if kind == "range" else 2):
                raise ValueError(f"scan_batch: bad query {q!r}")
            qs.append((iterator.KINDS[kind], bytes(q[1]), bytes(q[2]) if kind == "range" else b""))
        if max_records is None or isinstance(max_records, int):
            limits = [max_records] * nq
        else:
            limits = list(max_records)
            if len(limits) != nq:
                raise ValueError("scan_batch: max_records must be one value or one per query")
        if any(m is not None and m < 0 for m in limits):
            raise ValueError("scan_batch: negative max_records")

        def blob(ks):
            b = torch.frombuffer(bytearray(b"".join(ks) or b"\0"), dtype=torch.uint8).to(dev)
            e = torch.from_numpy(np.cumsum([len(k) for k in ks] or [0], dtype=np.int64)).to(dev)
            return b, e

        kb, ke = blob([k for _, k, _ in qs])
        k2b, k2e = blob([k2 for _, _, k2 in qs])
        types = np.ascontiguousarray([t for t, _, _ in qs] or [0], dtype=np.int32)
        mr = None
        if any(m is not None for m in limits):
            mr = torch.from_numpy(np.array([(1 << 63) - 1 if m is None else min(m, (1 << 63) - 1) for m in limits],
                                           dtype=np.int64)).to(dev)
        L = _lib.lib()
        wsb = int(L.mtblx_scan_workspace_bytes(nq))
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)       # the caching allocator aligns to 512 bytes
        res = torch.zeros(max(nq, 1) * C.sizeof(_lib.ScanResult), dtype=torch.uint8, device=dev)
        if self.compression == 0:
            tab = (None, None, None, None, 0, None)
            keep = None
        else:
            if self._snappy_dev and nq and self._on_demand():
                # the bound of each query (mtblx.h, mtblx_scan_touch); Reader::get opens at most two blocks
                bounds = [k if t == _lib.SCAN_GET else k2 if t == _lib.SCAN_RANGE else
                          (prefix_bound(k) or b"") if t == _lib.SCAN_PREFIX else b"" for t, k, k2 in qs]
                bb, be = blob(bounds)
                caps = torch.from_numpy(np.array([min(max_blocks, 2) if t == _lib.SCAN_GET else max_blocks
                                                  for t, _, _ in qs], dtype=np.uint32).view(np.int32)).to(dev)
                self._od_touch(kb, ke, bb, be, caps, 0, nq, stream)
            keep = self._dec_table()
            ts, tdo, tdl, tst, ntab, dec = keep
            tab = (C.c_void_p(ts.data_ptr()), C.c_void_p(tdo.data_ptr()), C.c_void_p(tdl.data_ptr()),
                   C.c_void_p(tst.data_ptr()), ntab, C.c_void_p(dec.data_ptr()))
        totals = (C.c_uint64 * 4)()
        args = (C.c_void_p(self.file.data_ptr()), self.len, self.version, 1 if self.verify else 0,
                self.index_off, self.index_len, *tab, C.c_void_p(types.ctypes.data),
                C.c_void_p(kb.data_ptr()), C.c_void_p(ke.data_ptr()), C.c_void_p(k2b.data_ptr()),
                C.c_void_p(k2e.data_ptr()), C.c_void_p(mr.data_ptr()) if mr is not None else None,
                max_blocks, nq, C.c_void_p(res.data_ptr()), totals, C.c_void_p(ws.data_ptr()), wsb)
        if reduce is None:
            rc = L.mtblx_scan_plan(*args, C.c_void_p(codec._stream_handle(stream)))
            if rc != 0:
                raise RuntimeError(f"mtblx_scan_plan failed: {rc}")
            return res, [int(x) for x in totals], ws, wsb, limits, tab, keep
        spec = reduce.cstruct()
        fields = torch.zeros((max(nq, 1), len(reduce.ops)), dtype=torch.int64, device=dev)
        nbad = torch.zeros(max(nq, 1), dtype=torch.int64, device=dev)
        if where is not None:
            wspec = where.cstruct()
            nmatch = torch.zeros(max(nq, 1), dtype=torch.int64, device=dev)
            rc = L.mtblx_scan_reduce_where(*args, C.byref(spec), C.c_void_p(fields.data_ptr()),
                                           C.c_void_p(nbad.data_ptr()), C.byref(wspec), C.c_void_p(nmatch.data_ptr()),
                                           C.c_void_p(codec._stream_handle(stream)))
            if rc != 0:
                raise RuntimeError(f"mtblx_scan_reduce_where failed: {rc}")
            return res, [int(x) for x in totals], ws, wsb, limits, tab, keep, (fields[:nq], nbad[:nq], nmatch[:nq])
        rc = L.mtblx_scan_reduce(*args, C.byref(spec), C.c_void_p(fields.data_ptr()), C.c_void_p(nbad.data_ptr()),
                                 C.c_void_p(codec._stream_handle(stream)))
        if rc != 0:
            raise RuntimeError(f"mtblx_scan_reduce failed: {rc}")
        return res, [int(x) for x in totals], ws, wsb, limits, tab, keep, (fields[:nq], nbad[:nq])

    def count_batch(self, queries, max_blocks: int = 64, stream=None):
        """The plan of scan_batch alone: (status int32, nrec, key_bytes, val_bytes int64) [nq] on the
        device.  Queries that are not SCAN_OK count 0: scan_batch answers them through bulk()."""
        nq = len(queries)
        stream = self._s(stream)
        with torch.cuda.stream(stream):   # mtblx_scan_plan returns its totals: it synchronises `stream`, so the
            res = self._scan_plan(queries, max_blocks, None, stream)[0]   # workspace may go back to the allocator
        w = res.view(torch.int64).view(-1, 8)[:nq]
        return res.view(torch.int32).view(-1, 16)[:nq, 0], w[:, 1], w[:, 2], w[:, 3]

    def scan_batch(self, queries, max_blocks: int = 64, max_records=None, stream=None, where=None) -> "ScanBatch":
        """iter_from / get / iter_prefix / iter_range for a batch of queries: one plan, one allocation
        sized from its totals, one emit (mtblx_scan_plan / mtblx_scan_emit).  `queries`: ("from", k),
        ("get", k), ("prefix", p) or ("range", a, b); `max_records`: None, one limit, or one per query
        (None = no limit).  A query the kernels hand back -- SCAN_LARGE: more than `max_blocks` data
        blocks; SCAN_FALLBACK: somewhere the reference panics, errs or loops -- is answered by
        iterator.bulk() with the limit applied; so is every query when the index block is not
        regular.  ("get", k) is Reader::get: at most one record.  Everything -- the uploads, the
        on-demand staging, plan and emit, the read-backs and the seek-path answers -- runs on
        `stream` (default: the current stream), which the call synchronises.  where (a where.Where):
        the ScanBatch then reports, per query, the records whose value it keeps -- emit plus
        filter_records over the emitted buffers with the queries as segments, before anything is read
        back; `max_records` cuts before the filter; the bad values it dropped are `nbad` (int64 [nq])."""
        from .where import as_where
        where = as_where(where)
        stream = self._s(stream)
        with torch.cuda.stream(stream):
            sb = self._scan_batch(list(queries), max_blocks, max_records, stream)
            return sb if where is None else self._filter_scan(sb, where, stream)

    def _filter_scan(self, sb: "ScanBatch", where, stream) -> "ScanBatch":
        """`sb` with every query's records filtered on the device: the kernel path's buffers in one
        filter_records whose segments are the queries, a seek-path answer from its own device records"""
        from .encode import DeviceRecords
        from .where import filter_records
        f = filter_records(DeviceRecords(sb.keys, sb.key_end, sb.vals, sb.val_end), where, sb.rec_off, stream)
        r, nq = f.records, sb.nq
        rec_off = f.seg_off()
        kb = torch.cat([r.key_end.new_zeros(1), r.key_end])[rec_off]   # the bytes before every query's kept records
        vb = torch.cat([r.val_end.new_zeros(1), r.val_end])[rec_off]
        host = sb._res.copy()
        ro, kh, vh = (t.cpu().numpy() for t in (rec_off, kb, vb))       # three words per query, on `stream`
        host["nrec"], host["rec_base"] = np.diff(ro), ro[:-1]
        host["key_bytes"], host["key_base"] = np.diff(kh), kh[:-1]
        host["val_bytes"], host["val_base"] = np.diff(vh), vh[:-1]
        nbad = f.seg_bad.clone()
        served = {}
        for q, sc in sb._served.items():
            n = sc.nrec
            g = filter_records(DeviceRecords(sc.keys, sc.key_end[:n], sc.vals, sc.val_end[:n]), where, None, stream)
            served[q] = Scan(sc.end, sc.err, g.nkept, g.records.keys, g.records.vals, g.records.key_end,
                             g.records.val_end, stream)
            nbad[q] = g.nbad
        out = ScanBatch(nq, r.keys, r.vals, r.key_end, r.val_end, rec_off, sb.status, host, served, stream)
        out.nbad = nbad
        return out

    def _scan_limited(self, query, m, stream) -> Scan:
        """one query of a batch through the seek path (iterator.bulk), cut at its limit `m`"""
        from . import iterator
        kind = query[0]
        s = iterator.bulk(self, kind, bytes(query[1]), bytes(query[2]) if kind == "range" else b"")
        if kind == "get":
            m = 1 if m is None else min(m, 1)
        if m is None or s.nrec < m or (m == 0 and s.end != END_NONE):
            s.stream = stream
            return s
        p = iterator._cut_part((s.keys, s.vals, s.key_end, s.val_end, s.nrec), m)
        return Scan(END_NONE, "None", m, p[0], p[1], p[2], p[3], stream)

    def _scan_batch(self, queries, max_blocks, max_records, stream) -> "ScanBatch":
        dev = self.file.device
        queries = list(queries)
        nq = len(queries)

        def limited(q, m):
            return self._scan_limited(queries[q], m, stream)

        z8 = torch.zeros(0, dtype=torch.uint8, device=dev)
        z64 = torch.zeros(0, dtype=torch.int64, device=dev)
        if nq == 0 or not self.index_regular():
            limits = [max_records] * nq if max_records is None or isinstance(max_records, int) else list(max_records)
            served = {q: limited(q, limits[q]) for q in range(nq)}
            host = np.zeros(nq, np.dtype(_lib.ScanResult))
            host["status"] = _lib.SCAN_FALLBACK
            return ScanBatch(nq, z8, z8, z64, z64, torch.zeros(nq + 1, dtype=torch.int64, device=dev),
                             torch.full((nq,), _lib.SCAN_FALLBACK, dtype=torch.int32, device=dev), host, served,
                             stream)
        res, totals, ws, wsb, limits, tab, keep = self._scan_plan(queries, max_blocks, max_records, stream)
        nrec, kbytes, vbytes = totals[0], totals[1], totals[2]
        buf = torch.empty(kbytes + vbytes + 16 * nrec + 8, dtype=torch.uint8, device=dev)   # ends first: aligned
        key_end = buf[: 8 * nrec].view(torch.int64)
        val_end = buf[8 * nrec: 16 * nrec].view(torch.int64)
        flags = buf[16 * nrec: 16 * nrec + 8].view(torch.int32)
        keys = buf[16 * nrec + 8: 16 * nrec + 8 + kbytes]
        vals = buf[16 * nrec + 8 + kbytes:]
        out = _lib.Scanned(keys=buf.data_ptr() + 16 * nrec + 8, keys_cap=kbytes,
                           vals=buf.data_ptr() + 16 * nrec + 8 + kbytes, vals_cap=vbytes,
                           key_end=buf.data_ptr(), val_end=buf.data_ptr() + 8 * nrec, rec_cap=nrec,
                           flags=buf.data_ptr() + 16 * nrec)
        rc = _lib.lib().mtblx_scan_emit(C.c_void_p(self.file.data_ptr()), self.len, self.version, self.index_off,
                                        self.index_len, *tab, nq, C.byref(out), C.c_void_p(ws.data_ptr()), wsb,
                                        C.c_void_p(codec._stream_handle(stream)))
        if rc != 0:
            raise RuntimeError(f"mtblx_scan_emit failed: {rc}")
        # the one read-back: on `stream`, behind the emit, so it synchronises the emit too -- the flags
        # word is complete, and the workspace may go back to the allocator when this call returns
        host = np.frombuffer(res.cpu().numpy().tobytes(), np.dtype(_lib.ScanResult))[:nq]
        fl = int(flags[0].item())
        if fl:
            raise RuntimeError(f"mtblx_scan_emit: flags {fl}")
        w = res.view(torch.int64).view(-1, 8)[:nq]
        rec_off = torch.cat([w[:, 4], torch.tensor([nrec], dtype=torch.int64, device=dev)])
        status = res.view(torch.int32).view(-1, 16)[:nq, 0]
        served = {int(q): limited(int(q), limits[int(q)]) for q in np.nonzero(host["status"] != _lib.SCAN_OK)[0]}
        return ScanBatch(nq, keys, vals, key_end, val_end, rec_off, status, host, served, stream)

    def reduce_batch(self, queries, reduce, max_blocks: int = 64, max_records=None, stream=None,
                     where=None) -> "ReduceBatch":
        """scan_batch that aggregates instead of returning records: per query, `reduce` (a Reduce or a
        shorthand name) folded over the values of the records scan_batch would report (same stop rules,
        same `max_records`, ("get", k) at most one record), as Reduce.fold defines it.  One
        mtblx_scan_reduce -- the plan walk reads each value where it lies, no key or value is
        materialised -- and one read-back; the answer is 8 * F + 16 bytes per query.  A query the walk
        hands back (SCAN_LARGE, SCAN_FALLBACK) and every query of a reader with an irregular index is
        answered by iterator.bulk() with the limit applied and its device records are reduced by
        reduce_segments: no record is copied to the host.  Everything runs on `stream` (default: the
        current stream), which the call synchronises.  where (a where.Where of the Reduce's layout,
        else ValueError): the fused walk mtblx_scan_reduce_where -- `nrec` and the status stay what
        scan_batch reports (the predicate sits after the iterator and after `max_records`), `nbad`
        counts the bad values, `nmatch` the kept ones, and `fields` folds the kept values alone; a
        handed-back query goes through filter_records, then reduce_segments."""
        from .reduce import as_reduce
        from .where import as_where
        red = as_reduce(reduce)
        if red is None:
            raise ValueError(f"reduce_batch: {reduce!r} is not a Reduce")
        where = as_where(where)
        if where is not None and not where.same_layout(red):
            raise ValueError(f"reduce_batch: {where!r} has not the layout of {red!r}")
        stream = self._s(stream)
        with torch.cuda.stream(stream):
            return self._reduce_batch(list(queries), red, max_blocks, max_records, stream, where)

    def _reduce_batch(self, queries, red, max_blocks, max_records, stream, where=None) -> "ReduceBatch":
        from .encode import DeviceRecords
        from .reduce import ReduceBatch, _signed, reduce_segments
        dev = self.file.device
        nq = len(queries)
        if nq == 0 or not self.index_regular():
            from .merger import check_queries
            queries, limits = check_queries(queries, max_records)   # the kernel path: _scan_plan checks them
            fields = torch.tensor(_signed(red.identities()), dtype=torch.int64, device=dev).repeat(nq, 1)
            nbad = torch.zeros(nq, dtype=torch.int64, device=dev)
            nrec = torch.zeros(nq, dtype=torch.int64, device=dev)
            status = torch.full((nq,), _lib.SCAN_FALLBACK, dtype=torch.int32, device=dev)
            nmatch = torch.zeros(nq, dtype=torch.int64, device=dev) if where is not None else None
            back, n_large, n_fallback = range(nq), 0, nq
        else:
            res, _, _, _, limits, _, _, outs = self._scan_plan(queries, max_blocks, max_records, stream, red, where)
            fields, nbad, nmatch = outs if where is not None else (*outs, None)
            # the one read-back: mtblx_scan_reduce has synchronised `stream`
            host = np.frombuffer(res.cpu().numpy().tobytes(), np.dtype(_lib.ScanResult))[:nq]
            nrec = res.view(torch.int64).view(-1, 8)[:nq, 1].clone()
            status = res.view(torch.int32).view(-1, 16)[:nq, 0].clone()
            back = [int(q) for q in np.nonzero(host["status"] != _lib.SCAN_OK)[0]]
            n_large = int((host["status"] == _lib.SCAN_LARGE).sum())
            n_fallback = int((host["status"] == _lib.SCAN_FALLBACK).sum())
        ends = {}
        for q in back:   # the seek path's answer stays on the device: one segment over its records
            sc = self._scan_limited(queries[q], limits[q], stream)
            n = sc.nrec
            recs = DeviceRecords(sc.keys, sc.key_end[:n], sc.vals, sc.val_end[:n])
            if where is None:
                f, nb = reduce_segments(recs, [0], [n], red, stream)
                nbad[q] = nb[0]
            else:   # the kept records are well-formed: the fold over them meets no bad value
                from .where import filter_records
                kept = filter_records(recs, where, None, stream)
                f, _ = reduce_segments(kept.records, [0], [kept.nkept], red, stream)
                nbad[q] = kept.nbad
                nmatch[q] = kept.nkept
            fields[q] = f[0]
            nrec[q] = n
            ends[q] = (sc.end, sc.err)
        return ReduceBatch(red, fields, nrec, nbad, status, ends, n_large, n_fallback, stream, nmatch)

    def rollup(self, group, reduce, stream=None, where=None):
        """The whole file rolled up: its records (iter()) grouped by `group` (a rollup.GroupBy), `reduce`
        folded over every group's values -> rollup.Rollup with one segment.  A file sorts its keys, so
        the group keys increase strictly and Rollup.write_file() gives the rolled-up .mtbl.  A scan
        that does not end cleanly raises as Merger sources do.  Everything runs on `stream` (default:
        the current stream), which the call synchronises.  where (a where.Where): only the records
        whose value it keeps are rolled up (rollup_records)."""
        from .merger import _clean_scan
        from .rollup import rollup_records
        stream = self._s(stream)
        with torch.cuda.stream(stream):
            return rollup_records(_clean_scan(self.iter()), group, reduce, None, stream, where)

    def rollup_batch(self, queries, group, reduce, max_blocks: int = 64, stream=None, where=None):
        """scan_batch, then one rollup over its records with the queries as segments (seg_off =
        rec_off): per query, the records scan_batch reports for it grouped by `group` with `reduce`
        folded over every group -> rollup.Rollup, groups(q) per query.  A query the walk hands back
        (SCAN_LARGE, SCAN_FALLBACK) and every query of a reader with an irregular index is answered
        by the seek path and rolled up from its own device records, kept beside the kernel path's
        answer; end(q) / err(q) tell how such a query's iteration ended.  Everything runs on `stream`
        (default: the current stream), which the call synchronises.  where (a where.Where): every
        query's records are filtered first and the kept ones rolled up (rollup_records)."""
        from .encode import DeviceRecords
        from .reduce import as_reduce
        from .rollup import _as_group, rollup_records
        from .where import as_where
        grp = _as_group(group)
        red = as_reduce(reduce)
        if red is None:
            raise ValueError(f"rollup_batch: {reduce!r} is not a Reduce")
        where = as_where(where)
        stream = self._s(stream)
        with torch.cuda.stream(stream):
            sb = self._scan_batch(list(queries), max_blocks, None, stream)
            out = rollup_records(DeviceRecords(sb.keys, sb.key_end, sb.vals, sb.val_end), grp, red, sb.rec_off, stream,
                                 where)
            for q, sc in sb._served.items():
                n = sc.nrec
                out._served[q] = rollup_records(DeviceRecords(sc.keys, sc.key_end[:n], sc.vals, sc.val_end[:n]), grp,
                                                red, None, stream, where)
                out._ends[q] = (sc.end, sc.err)
            return out

    def into_iter(self, kind: str = "iter", key: bytes = b"", key2: bytes = b""):
        """the stateful ReaderIntoIter (next() / seek()), see iterator.ReaderIntoIter"""
        from . import iterator
        return iterator.ReaderIntoIter(self, kind, key, key2)

    def _index_records(self):
        """the index block's records (separator key, value) on the host, cached"""
        if self._irecs is None:
            self._irecs = self.index.to_host().records(0) if self.nent else []
        return self._irecs

    def _index_keys(self):
        if self._ikeys is None:
            self._ikeys = [k for k, _ in self._index_records()]
        return self._ikeys

    def _index_chain(self):
        """(entry offsets of the index scan chain, regular) from mtblx_entry_offsets: regular =
        a seek from any index iterator state lands on the chain and continues along the
        directory (include/mtblx.h); otherwise the iterators drive the live index iterator on
        the device (iterator._IxList)"""
        if self._eoffs is None:
            dev = self.file.device
            cap = max(self.index_len // 3 + 1, 1)          # an entry takes >= 3 bytes
            offs = torch.zeros(cap, dtype=torch.int64, device=dev)
            cnt = torch.zeros(1, dtype=torch.int64, device=dev)
            reg = torch.zeros(1, dtype=torch.int32, device=dev)
            rc = _lib.lib().mtblx_entry_offsets(C.c_void_p(self.file.data_ptr() + self.index_off), self.index_len,
                                                C.c_void_p(offs.data_ptr()), cap, C.c_void_p(cnt.data_ptr()),
                                                C.c_void_p(reg.data_ptr()), C.c_void_p(codec._stream_handle(None)))
            if rc != 0:
                raise RuntimeError(f"mtblx_entry_offsets failed: {rc}")
            n = min(int(cnt.item()), cap)
            self._eoffs = offs[:n].cpu().numpy()
            self._regular = bool(reg.item()) and self.index_status == _lib.ST_OK
        return self._eoffs, self._regular

    def index_regular(self) -> bool:
        return self._index_chain()[1]

    def _chain_ordinal(self, entry: int):
        """position on the index scan chain of the entry at `entry` (the index seek's landing),
        or None when it lies off the chain (a corrupt index)"""
        eoffs = self._index_chain()[0]
        i = int(np.searchsorted(eoffs, entry))
        if i < eoffs.size and int(eoffs[i]) == entry:
            return i
        return None

    def _ordinal(self, entry: int) -> int:
        """directory entry of a regular index's seek landing (always on the chain)"""
        i = self._chain_ordinal(entry)
        if i is None or i >= self.nent:
            raise RuntimeError("index seek landed off the directory of a regular index")
        return i

    def index_content(self):
        """the index block content on the device as (tensor, off, len)"""
        return self.file, self.index_off, self.index_len

    def _frame_values(self, values):
        """block_at_index + Reader::block framing (src/reader.rs:177-186, :139-157) of arbitrary
        index values (the live index iterator's records) on the device: (off, len, status)"""
        dev = self.file.device
        n = len(values)
        blob = b"".join(values) or b"\0"
        vals = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev)
        vend = torch.tensor(np.cumsum([len(v) for v in values], dtype=np.int64).astype(np.uint32).view(np.int32),
                            dtype=torch.int32, device=dev)
        off = torch.zeros(n, dtype=torch.int64, device=dev)
        ln = torch.zeros(n, dtype=torch.int32, device=dev)
        st = torch.zeros(n, dtype=torch.int32, device=dev)
        rc = _lib.lib().mtblx_block_dir(C.c_void_p(self.file.data_ptr()), self.len, self.version,
                                        C.c_void_p(vals.data_ptr()), C.c_void_p(vend.data_ptr()), 0, n,
                                        C.c_void_p(off.data_ptr()), C.c_void_p(ln.data_ptr()),
                                        C.c_void_p(st.data_ptr()), C.c_void_p(codec._stream_handle(None)))
        if rc != 0:
            raise RuntimeError(f"mtblx_block_dir failed: {rc}")
        return off, ln, st

    def _value_blocks(self, values):
        """the blocks of index values as next() loads them (see _host_blocks)"""
        off, ln, st = self._frame_values(values)
        return self._host_blocks_framed(off, ln, st, values)

    def _value_content(self, value: bytes):
        """Reader::block (src/reader.rs:139-175) at the offset an index value names -> the
        content (tensor, off, len) BlockIter reads; raises the reference's panics / Err"""
        off, ln, st = self._frame_values([value])
        s = int(st[0].item())
        if s == _lib.DIR_UNSUPPORTED:                   # stored content >= 4 GiB
            _, start, size, stored = self._big_frame_value(value)
            if self.verify and self._crc_big(start, size) != stored:
                raise ReferencePanic("Reader::block: checksum")
            if self.compression != 0:
                return self._decompressed(start, size)
            return self.file, start, size
        if s != _lib.DIR_OK:
            raise ReferencePanic("Reader::block: framing")
        if self.verify:
            batch = codec.DeviceBatch(self.file, off, ln, int(ln[0].item()))
            if int(codec.crc32c_blocks(batch, framed=True)[1][0].item()):
                raise ReferencePanic("Reader::block: checksum")
        o, n = int(off[0].item()), int(ln[0].item()) & 0xFFFFFFFF
        if self.compression == 0:
            return self.file, o, n
        return self._decompressed(o, n)

    def _seek_content(self, s):
        """Reader::block of an index seek's landed entry -> (tensor, off, len) of the content
        BlockIter reads (host-decompressed for compressed files); raises Err / panic."""
        if s.block_status == _lib.SEEK_PANIC:
            raise ReferencePanic("Reader::block")
        if self.compression == 0:
            if s.block_status == _lib.SEEK_ERR:
                raise MtblError(6)
            if s.block_status == _lib.SEEK_UNSUPPORTED:   # frame_block handles any size
                raise RuntimeError("index seek: unexpected block status")
            return self.file, int(s.data_off), int(s.data_len)
        # compressed: Block::init runs on the decompressed content (mtblx_block_seek_batch);
        # block_status's ERR / UNSUPPORTED judged the compressed bytes and do not apply
        return self._decompressed(int(s.data_off), int(s.data_len))

    def _decompressed(self, off: int, n: int):
        """src/compression.rs:57-68 for one stored block -> content on the device (Snappy: on the
        device; the other codecs and a stored content >= 4 GiB: on the host)"""
        if self._snappy_dev and n <= 0xFFFFFFFF:
            dev = self.file.device
            o = torch.tensor([off], dtype=torch.int64, device=dev)
            ln = torch.from_numpy(np.array([n], np.uint32).view(np.int32)).to(dev)
            buf, doff, dlen, tab, _ = self._stage_all(o, ln, torch.zeros(1, dtype=torch.int32, device=dev), None)
            if int(tab[3][0].item()):
                raise MtblError(7)
            return buf, int(doff[0].item()), int(dlen[0].item()) & 0xFFFFFFFF
        self._nhost += 1
        raw = self.file[off: off + n].cpu().numpy()
        L = _lib.lib()
        out = _lib.u8p()
        un = C.c_uint64(0)
        src = raw if raw.size else np.zeros(1, np.uint8)
        if L.mtblx_decompress(self.compression, src.ctypes.data, raw.size, C.byref(out), C.byref(un)) != 0:
            raise MtblError(7)
        buf = np.empty(max(int(un.value), 1), np.uint8)   # no bytes object: blocks of GiBs
        C.memmove(buf.ctypes.data, out, int(un.value))
        L.mtblx_free(out)
        t = torch.from_numpy(buf).to(self.file.device)
        return t, 0, int(un.value)

    def _decode_range(self, i0: int, i1: int):
        """decode directory entries [i0, i1) -> (dir status, crc bad, decompress errors, decoded,
        (base tensor, content offsets, content lengths)) with host arrays"""
        off, ln, st = self._framing()
        bad = self._bad_range(i0, i1)
        return self._decode_framed(off[i0:i1], ln[i0:i1], st[i0:i1], bad)

    def _decode_framed(self, off, ln, st, bad="verify"):
        """decode framed blocks (off, len, dir status: device tensors); bad: the checksum
        assert per block (device uint8), None when not verifying, "verify" to compute it"""
        n = int(off.numel())
        dst = st.cpu().numpy()
        if isinstance(bad, str):
            bad = None
            if self.verify and n:
                okl = torch.where(st == _lib.DIR_OK, ln, torch.zeros_like(ln))
                batch = codec.DeviceBatch(self.file, off, okl, codec.u32_max(okl))
                bad = codec.crc32c_blocks(batch, framed=True)[1]
        bad_dev = bad
        bad = bad.cpu().numpy() if bad is not None else np.zeros(n, np.uint8)
        if self._snappy_dev:
            # the stored bytes stay where they are; a preamble is a u32, so no content here is >= 4 GiB
            buf, doff, dlen, tab, mx = self._stage_all(off, ln, st, bad_dev)
            zerr = tab[3].cpu().numpy()
            uoff = doff.cpu().numpy()
            uln = dlen.cpu().numpy().view(np.uint32).astype(np.int64)
            batch = codec.DeviceBatch(buf, doff, dlen, int(uln.max()) if n else 0)
            where = (buf, uoff, uln)
        elif self.compression != 0:
            buf, uoff, uln, zerr = self._host_stage(off, ln, st)
            small = np.where(uln > 0xFFFFFFFF, 0, uln).astype(np.uint32)   # >= 4 GiB: _big_content
            batch = codec.DeviceBatch.from_host(buf, uoff, small, device=self.file.device)
            where = (batch.data, uoff.astype(np.int64), uln.astype(np.int64))
        else:
            zerr = np.zeros(n, np.int32)
            batch = codec.DeviceBatch(self.file, off, ln, codec.u32_max(ln))
            where = (self.file, off.cpu().numpy(), ln.cpu().numpy().view(np.uint32).astype(np.int64))
        data = codec.decode_blocks(batch)
        return dst, bad, zerr, data, where

    def _walk_range(self, i0: int, i1: int):
        """ReaderIntoIter::next over directory entries [i0, i1), each block loaded by next()
        -> ((keys, vals, key_end, val_end, nrec) on the device, end, err, stopped)"""
        from . import iterator
        parts, end, err, stopped = self._walk_blocks(i0, i1, first_exempt=False)
        sc = iterator._assemble(parts, end, err, self.file.device)
        return (sc.keys, sc.vals, sc.key_end, sc.val_end, sc.nrec), end, err, stopped

    def _host_blocks(self, i0: int, i1: int):
        """blocks [i0, i1) as next() loads them, for the stateful iterator: per block an
        exception to raise (Err / panic) or ((tensor, off, len), records, emit end)"""
        off, ln, st = self._framing()
        recs = self._index_records()
        return self._host_blocks_framed(off[i0:i1], ln[i0:i1], st[i0:i1], [recs[i][1] for i in range(i0, i1)],
                                        self._bad_range(i0, i1))

    def _host_blocks_framed(self, off, ln, st, values, bad="verify"):
        dst, bad, zerr, data, (base, boff, blen) = self._decode_framed(off, ln, st, bad)
        h = data.to_host()
        out = []
        for i in range(len(values)):
            content = (base, int(boff[i]), int(blen[i]))
            big_dec = dst[i] == _lib.DIR_OK and not bad[i] and not zerr[i] and int(blen[i]) > 0xFFFFFFFF
            if dst[i] == _lib.DIR_UNSUPPORTED or big_dec:   # content >= 4 GiB
                if big_dec:
                    kind, em = self._big_content(content)
                else:
                    kind, em, content = self._big_block_value(values[i])
                if kind == "ok":
                    out.append((content, em.host_records(), em.end))
                elif kind in ("panic", "loop"):
                    out.append(ReferencePanic("Reader::block / BlockIter") if kind == "panic"
                               else ReferenceLoop("BlockIter::next"))
                else:
                    out.append(MtblError(7 if kind == "Io" else 6))
                continue
            if dst[i] != _lib.DIR_OK or bad[i]:
                out.append(ReferencePanic("Reader::block"))
                continue
            if zerr[i]:
                out.append(MtblError(7))
                continue
            s = int(h.status[i])
            if s == _lib.ST_INVALID_BLOCK:
                out.append(MtblError(6))
            elif s == _lib.ST_UNSUPPORTED:   # the batch carries u32 lengths: cannot happen
                out.append(RuntimeError("batched decode: block >= 4 GiB"))
            else:
                end = {_lib.ST_CORRUPT: _lib.EMIT_PANIC, _lib.ST_LOOP: _lib.EMIT_LOOP}.get(s, _lib.EMIT_END)
                out.append((content, h.records(i), end))
        return out


# GF(2) arithmetic of CRC-32C (reflected, x^0 = bit 31) for joining piece checksums
_POLY = 0x82F63B78


def _gf2_mul(a: int, b: int) -> int:
    p = 0
    for i in range(32):
        if a & (0x80000000 >> i):
            p ^= b
        b = (b >> 1) ^ _POLY if b & 1 else b >> 1
    return p


def _x8n(n: int) -> int:
    """x^(8 n) mod P"""
    r, sq, e = 0x80000000, 0x80000000 >> 8, n   # sq = x^8
    while e:
        if e & 1:
            r = _gf2_mul(sq, r)
        sq = _gf2_mul(sq, sq)
        e >>= 1
    return r

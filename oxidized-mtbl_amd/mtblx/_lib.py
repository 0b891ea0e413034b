"""ctypes binding of libmtblx.so (include/mtblx.h, include/mtblx_host.h).

The library is built in-tree (``make -C oxidized-mtbl_amd``).  There is no fallback:
if the shared object is missing, importing the codec raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# MTBLX_LIB selects the diagnostic stamps build (bench.py --stamps); default is the product build
LIB_PATH = os.environ.get("MTBLX_LIB") or os.path.join(_HERE, "libmtblx.so")

u8p = C.POINTER(C.c_uint8)
u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)
i32p = C.POINTER(C.c_int32)

MTBLX_OK, MTBLX_E_INVAL, MTBLX_E_HIP, MTBLX_E_NODEV, MTBLX_E_FORMAT, MTBLX_E_TIMEOUT, MTBLX_E_IO = 0, -1, -2, -3, -4, -5, -6
ST_OK, ST_INVALID_BLOCK, ST_CORRUPT, ST_LOOP, ST_UNSUPPORTED, ST_OVERFLOW, ST_DECOMPRESS = range(7)
SNAPPY_OK, SNAPPY_CORRUPT, SNAPPY_TOO_SMALL, SNAPPY_TIMEOUT = range(4)
CODEC_OK, CODEC_CORRUPT, CODEC_UNSUPPORTED = range(3)
DIR_OK, DIR_PANIC, DIR_UNSUPPORTED = range(3)
GET_FOUND, GET_NONE, GET_PANIC, GET_ERR, GET_LOOP, GET_MISSING = range(6)
SEEK_OK, SEEK_ERR, SEEK_PANIC, SEEK_LOOP, SEEK_UNSUPPORTED = range(5)
EMIT_END, EMIT_PANIC, EMIT_LOOP, EMIT_MAX, EMIT_OVERFLOW = range(5)

# every symbol the public headers declare (checked by tests/test_abi.py)
EXPORTS = [
    "mtblx_abi_version", "mtblx_device_ok", "mtblx_decode_workspace_bytes", "mtblx_decode_blocks",
    "mtblx_count_blocks", "mtblx_decode_counted", "mtblx_decode_blocks_valpos", "mtblx_decode_blocks_verify", "mtblx_crc32c_blocks", "mtblx_block_dir", "mtblx_get", "mtblx_get_decompressed", "mtblx_crc32c", "mtblx_varint_decode64", "mtblx_read_footer", "mtblx_frame_block",
    "mtblx_writer_new", "mtblx_writer_insert", "mtblx_writer_insert_batch", "mtblx_writer_finish",
    "mtblx_writer_block_count", "mtblx_writer_block_dir", "mtblx_writer_free", "mtblx_free",
    "mtblx_snappy_max_compressed_len", "mtblx_snappy_uncompressed_len", "mtblx_snappy_decompress",
    "mtblx_snappy_compress", "mtblx_snappy_decompress_blocks", "mtblx_pipe_new", "mtblx_pipe_free",
    "mtblx_pipe_decode", "mtblx_pipe_decode_valpos", "mtblx_pipe_set", "mtblx_host_alloc", "mtblx_host_free", "mtblx_host_register", "mtblx_host_unregister",
    "mtblx_encode_plan", "mtblx_encode_workspace_bytes", "mtblx_encode_blocks", "mtblx_plan_keep_bytes",
    "mtblx_encode_plan_keep", "mtblx_encode_blocks_planned", "mtblx_plan_release", "mtblx_plan_workspace_bytes",
    "mtblx_plan_serial_workspace_bytes",
    "mtblx_snappy_workspace_bytes", "mtblx_snappy_dir", "mtblx_snappy_decompress_dev", "mtblx_stream_copy", "mtblx_encode_index",
    "mtblx_codec_available", "mtblx_decompress", "mtblx_compress", "mtblx_decompress_blocks", "mtblx_writer_set_level",
    "mtblx_index_seek_batch", "mtblx_block_seek_batch", "mtblx_block_seek_batch_kbuf", "mtblx_block_seek_batch_ex", "mtblx_copy_ranges", "mtblx_entry_offsets",
    "mtblx_key_filter",
    "mtblx_merge_workspace_bytes", "mtblx_merge_plan", "mtblx_merge_emit", "mtblx_merge_plan_timed",
    "mtblx_sort_workspace_bytes", "mtblx_sort_plan", "mtblx_sort_emit", "mtblx_sort_plan_timed",
    "mtblx_merge_emit_reduce", "mtblx_sort_emit_reduce",
    "mtblx_merge_seg_workspace_bytes", "mtblx_merge_seg_plan", "mtblx_merge_seg_emit", "mtblx_merge_seg_emit_reduce",
    "mtblx_merge_seg_plan_timed",
    "mtblx_merge_plan_select", "mtblx_merge_seg_plan_select",
    "mtblx_snappy_compress_workspace_bytes", "mtblx_snappy_slots", "mtblx_snappy_compress_dev", "mtblx_frame_blocks",
    "mtblx_encode_index_c",
    "mtblx_scan_workspace_bytes", "mtblx_scan_plan", "mtblx_scan_emit",
    "mtblx_scan_reduce", "mtblx_reduce_segments", "mtblx_reduce_seg_tile",
    "mtblx_rollup_workspace_bytes", "mtblx_rollup_plan", "mtblx_rollup_emit", "mtblx_rollup_tile",
    "mtblx_reduce_encode_workspace_bytes", "mtblx_reduce_encode",
    "mtblx_where_workspace_bytes", "mtblx_where_plan", "mtblx_where_emit", "mtblx_where_tile",
    "mtblx_scan_reduce_where",
    "mtblx_stage_workspace_bytes", "mtblx_stage_plan", "mtblx_stage_emit", "mtblx_scan_touch", "mtblx_bitmap_compact",
    "mtblx_table_gather", "mtblx_dir_ascends",
    "mtblx_debug_cu_limit", "mtblx_debug_grid_items", "mtblx_debug_decode_tiles",
]
MERGE_MAX_SOURCES, MERGE_MAX_RECORDS = 64, (1 << 32) - 16
MERGE_GROUPS, MERGE_CONCAT, MERGE_FIRST, MERGE_LAST = range(4)
MERGE_UNSORTED, MERGE_INTERNAL = 1, 2          # totals[5] of mtblx_merge_plan
MERGE_OVERFLOW, MERGE_NOT_PLANNED = 1, 2       # *flags of mtblx_merge_emit
MERGE_BADVALUE = 4                             # *flags of mtblx_merge_emit_reduce / mtblx_sort_emit_reduce
MERGE_MAX_SEGMENTS = 1 << 24                   # MTBLX_MERGE_MAX_SEGMENTS: segments per mtblx_merge_seg_plan
MERGE_BADSEG = 4                               # totals[5] of mtblx_merge_seg_plan: a bad seg_off array
REDUCE_SUM, REDUCE_MIN, REDUCE_MAX = range(3)  # mtblx_reduce.op
REDUCE_MAX_FIELDS = 8
REDUCE_VARINT = 0x10                           # MTBLX_REDUCE_VARINT: OR-ed into every op, the fields are varints
REDUCE_BADSEG = 8                              # *flags of mtblx_reduce_segments: a bad segment array
REDUCE_MAX_SEGMENTS = 0xFFFFFF00               # MTBLX_REDUCE_MAX_SEGMENTS: nseg of mtblx_reduce_segments
REDUCE_SEG_TILE = 1024                         # MTBLX_REDUCE_SEG_TILE: records per workgroup of mtblx_reduce_segments
GROUP_LENGTH, GROUP_DELIM = 0, 1                # mtblx_group.kind
ROLLUP_OVERFLOW, ROLLUP_NOT_PLANNED, ROLLUP_BADSEG = 1, 2, 8   # *flags of mtblx_rollup_emit
WHERE_ANY, WHERE_VARINT = 1, 0x10                # mtblx_where.flags
WHERE_OVERFLOW, WHERE_NOT_PLANNED, WHERE_BADSEG = 1, 2, 8      # *flags of mtblx_where_emit; BADSEG also totals[5]
SORT_TILE = 1024                               # MTBLX_SORT_TILE: handles per tile-sorted run of mtblx_sort_plan
PLAN_OUT_OF_ORDER, PLAN_PANIC, PLAN_TOO_LONG = 1, 2, 4
SCAN_OK, SCAN_LARGE, SCAN_FALLBACK = range(3)  # mtblx_scan_result.status
SCAN_MAX_KEY = 1024                            # MTBLX_SCAN_MAX_KEY: the emit kernel's key buffer
SCAN_OVERFLOW, SCAN_NOT_PLANNED, SCAN_INTERNAL = 1, 2, 4   # *flags of mtblx_scan_emit
SCAN_FROM, SCAN_GET, SCAN_PREFIX, SCAN_RANGE = range(4)    # query types (mtblx_key_filter's numbering)
# MTBLX_GRID_*: the families of mtblx_debug_grid_items
(GRID_SCAN_PLAN, GRID_SCAN_EMIT, GRID_GET, GRID_MERGE_BUILD, GRID_SEG_BUILD, GRID_SORT_SKIP, GRID_CRC,
 GRID_SNAPPY_SMALL, GRID_SNAPPY_LARGE, GRID_SNAPPY_COMP, GRID_COPY_RANGES, GRID_STREAM_COPY, GRID_DECODE_PIPE,
 GRID_DECODE_TILES) = range(14)


class BlockBatch(C.Structure):
    _fields_ = [("data", C.c_void_p), ("data_len", C.c_uint64), ("blk_off", C.c_void_p), ("blk_len", C.c_void_p),
                ("nblk", C.c_uint32), ("max_blk_len", C.c_uint32)]


class Decoded(C.Structure):
    _fields_ = [("nrec", C.c_void_p), ("rec_base", C.c_void_p), ("key_base", C.c_void_p), ("val_base", C.c_void_p),
                ("status", C.c_void_p), ("key_end", C.c_void_p), ("val_end", C.c_void_p), ("rec_cap", C.c_uint64),
                ("keys", C.c_void_p), ("keys_cap", C.c_uint64), ("vals", C.c_void_p), ("vals_cap", C.c_uint64),
                ("totals", C.c_void_p)]


class Records(C.Structure):
    _fields_ = [("keys", C.c_void_p), ("key_end", C.c_void_p), ("vals", C.c_void_p), ("val_end", C.c_void_p),
                ("n", C.c_uint64)]


class Merged(C.Structure):   # mtblx_merged (capacities in bytes)
    _fields_ = [("keys", C.c_void_p), ("keys_cap", C.c_uint64), ("key_end", C.c_void_p), ("key_end_cap", C.c_uint64),
                ("vals", C.c_void_p), ("vals_cap", C.c_uint64), ("val_end", C.c_void_p), ("val_end_cap", C.c_uint64),
                ("grp_end", C.c_void_p), ("grp_end_cap", C.c_uint64), ("flags", C.c_void_p)]


class SelectSpec(C.Structure):   # mtblx_select
    _fields_ = [("require", C.c_uint64), ("exclude", C.c_uint64), ("min_count", C.c_uint32),
                ("max_count", C.c_uint32)]


class ReduceSpec(C.Structure):   # mtblx_reduce
    _fields_ = [("nfields", C.c_uint32), ("op", C.c_uint8 * 8)]


class Group(C.Structure):   # mtblx_group
    _fields_ = [("kind", C.c_uint32), ("length", C.c_uint64), ("delim", C.c_uint32), ("count", C.c_uint32)]


class Rolled(C.Structure):   # mtblx_rolled (capacities in bytes)
    _fields_ = [("keys", C.c_void_p), ("keys_cap", C.c_uint64), ("key_end", C.c_void_p), ("key_end_cap", C.c_uint64),
                ("grp_rec", C.c_void_p), ("grp_rec_cap", C.c_uint64), ("seg_grp", C.c_void_p),
                ("seg_grp_cap", C.c_uint64), ("flags", C.c_void_p)]


class WhereSpec(C.Structure):   # mtblx_where
    _fields_ = [("nfields", C.c_uint32), ("flags", C.c_uint32), ("mask", C.c_uint8), ("outside", C.c_uint8),
                ("lo", C.c_uint64 * 8), ("hi", C.c_uint64 * 8)]


class Filtered(C.Structure):   # mtblx_filtered (keys_cap / vals_cap in bytes, rec_cap in records)
    _fields_ = [("keys", C.c_void_p), ("keys_cap", C.c_uint64), ("vals", C.c_void_p), ("vals_cap", C.c_uint64),
                ("key_end", C.c_void_p), ("val_end", C.c_void_p), ("src_idx", C.c_void_p), ("rec_cap", C.c_uint64),
                ("flags", C.c_void_p)]


class ScanResult(C.Structure):   # mtblx_scan_result
    _fields_ = [("status", C.c_int32), ("end", C.c_int32), ("nrec", C.c_uint64), ("key_bytes", C.c_uint64),
                ("val_bytes", C.c_uint64), ("rec_base", C.c_uint64), ("key_base", C.c_uint64),
                ("val_base", C.c_uint64), ("blocks", C.c_uint32), ("pad", C.c_uint32)]


class Scanned(C.Structure):   # mtblx_scanned (keys_cap / vals_cap in bytes, rec_cap in records)
    _fields_ = [("keys", C.c_void_p), ("keys_cap", C.c_uint64), ("vals", C.c_void_p), ("vals_cap", C.c_uint64),
                ("key_end", C.c_void_p), ("val_end", C.c_void_p), ("rec_cap", C.c_uint64), ("flags", C.c_void_p)]


class PipeStats(C.Structure):
    _fields_ = [("seconds", C.c_double), ("stage_seconds", C.c_double), ("decode_ms", C.c_double),
                ("block_bytes", C.c_uint64), ("h2d_bytes", C.c_uint64), ("d2h_bytes", C.c_uint64),
                ("chunks", C.c_uint32), ("decompress_errors", C.c_uint32)]


class IndexSeek(C.Structure):   # mtblx_index_seek
    _fields_ = [("status", C.c_int32), ("valid", C.c_int32), ("entry", C.c_uint64), ("block_off", C.c_uint64),
                ("block_status", C.c_int32), ("pad", C.c_int32), ("data_off", C.c_uint64), ("data_len", C.c_uint64)]


class BlockSeek(C.Structure):   # mtblx_block_seek
    _fields_ = [("data_off", C.c_uint64), ("data_len", C.c_uint64), ("kcap", C.c_uint64), ("max_records", C.c_uint64),
                ("first", C.c_int32), ("status", C.c_int32), ("end", C.c_int32), ("has_val", C.c_int32),
                ("entry", C.c_uint64), ("nrec", C.c_uint64), ("key_bytes", C.c_uint64), ("val_bytes", C.c_uint64),
                ("last_voff", C.c_uint64), ("last_vlen", C.c_uint64), ("resume_off", C.c_uint64),
                ("stop_off", C.c_uint64), ("early", C.c_int32), ("pad", C.c_int32)]


class Footer(C.Structure):
    _fields_ = [("meta", C.c_uint64 * 9), ("version", C.c_uint32), ("err", C.c_int32)]


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"libmtblx.so not built ({LIB_PATH}); run `make -C oxidized-mtbl_amd` "
                              "(no CPU fallback exists for the device codec)")
        # torch bundles its own libamdhip64.so.7 (same soname as /opt/rocm's): whichever loads
        # first serves the whole process.  Load torch first, so the device pointers and streams
        # torch hands us and libmtblx's kernels live in one HIP runtime (the order every
        # product path takes); without torch, libmtblx uses the system runtime.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        L.mtblx_abi_version.restype = C.c_int
        L.mtblx_device_ok.restype = C.c_int
        L.mtblx_decode_workspace_bytes.argtypes = [C.c_uint32]
        L.mtblx_decode_workspace_bytes.restype = C.c_size_t
        for f in (L.mtblx_decode_blocks, L.mtblx_count_blocks, L.mtblx_decode_counted):
            f.argtypes = [C.POINTER(BlockBatch), C.POINTER(Decoded), C.c_void_p, C.c_size_t, C.c_void_p]
            f.restype = C.c_int
        L.mtblx_decode_blocks_valpos.argtypes = [C.POINTER(BlockBatch), C.POINTER(Decoded), C.c_void_p, C.c_void_p,
                                                 C.c_size_t, C.c_void_p]
        L.mtblx_decode_blocks_valpos.restype = C.c_int
        L.mtblx_decode_blocks_verify.argtypes = [C.POINTER(BlockBatch), C.POINTER(Decoded), C.c_void_p, C.c_void_p,
                                                 C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
        L.mtblx_decode_blocks_verify.restype = C.c_int
        L.mtblx_crc32c_blocks.argtypes = [C.POINTER(BlockBatch), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.mtblx_crc32c_blocks.restype = C.c_int
        L.mtblx_block_dir.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64,
                                      C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mtblx_block_dir.restype = C.c_int
        L.mtblx_get.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p,
                                C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mtblx_get.restype = C.c_int
        L.mtblx_get_decompressed.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_uint64, C.c_uint64,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p]
        L.mtblx_get_decompressed.restype = C.c_int
        L.mtblx_crc32c.argtypes = [u8p, C.c_uint64]
        L.mtblx_crc32c.restype = C.c_uint32
        L.mtblx_varint_decode64.argtypes = [u8p, C.c_uint64, u64p]
        L.mtblx_varint_decode64.restype = C.c_int
        L.mtblx_read_footer.argtypes = [u8p, C.c_uint64, C.POINTER(Footer)]
        L.mtblx_read_footer.restype = C.c_int
        L.mtblx_frame_block.argtypes = [u8p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, u64p, u64p,
                                        C.POINTER(C.c_int)]
        L.mtblx_frame_block.restype = C.c_int
        L.mtblx_writer_new.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32]
        L.mtblx_writer_new.restype = C.c_void_p
        L.mtblx_writer_insert.argtypes = [C.c_void_p, u8p, C.c_uint64, u8p, C.c_uint64]
        L.mtblx_writer_insert.restype = C.c_int
        L.mtblx_writer_insert_batch.argtypes = [C.c_void_p, u8p, u64p, u8p, u64p, C.c_uint64]
        L.mtblx_writer_insert_batch.restype = C.c_int
        L.mtblx_writer_finish.argtypes = [C.c_void_p, C.POINTER(u8p), u64p]
        L.mtblx_writer_finish.restype = C.c_int
        L.mtblx_writer_block_count.argtypes = [C.c_void_p]
        L.mtblx_writer_block_count.restype = C.c_uint64
        L.mtblx_writer_block_dir.argtypes = [C.c_void_p, u64p, u32p, u32p]
        L.mtblx_writer_block_dir.restype = C.c_int
        L.mtblx_writer_free.argtypes = [C.c_void_p]
        L.mtblx_free.argtypes = [C.c_void_p]
        L.mtblx_snappy_max_compressed_len.argtypes = [C.c_uint64]
        L.mtblx_snappy_max_compressed_len.restype = C.c_uint64
        L.mtblx_snappy_uncompressed_len.argtypes = [C.c_void_p, C.c_uint64, u64p]
        L.mtblx_snappy_uncompressed_len.restype = C.c_int
        L.mtblx_snappy_decompress.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, u64p]
        L.mtblx_snappy_decompress.restype = C.c_int
        L.mtblx_snappy_compress.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, u64p]
        L.mtblx_snappy_compress.restype = C.c_int
        L.mtblx_snappy_decompress_blocks.argtypes = [C.c_void_p] * 7 + [C.c_uint64, C.c_uint32]
        L.mtblx_snappy_decompress_blocks.restype = C.c_uint64
        L.mtblx_pipe_new.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
        L.mtblx_pipe_new.restype = C.c_void_p
        L.mtblx_pipe_free.argtypes = [C.c_void_p]
        L.mtblx_pipe_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                        C.c_uint32, C.POINTER(Decoded), C.POINTER(PipeStats)]
        L.mtblx_pipe_decode.restype = C.c_int
        L.mtblx_pipe_decode_valpos.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32,
                                               C.POINTER(Decoded), C.c_void_p, C.POINTER(PipeStats)]
        L.mtblx_pipe_decode_valpos.restype = C.c_int
        L.mtblx_pipe_set.argtypes = [C.c_void_p, C.c_int, C.c_int64]
        L.mtblx_pipe_set.restype = C.c_int
        L.mtblx_encode_plan.argtypes = [C.POINTER(Records), C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32,
                                        C.c_void_p, C.c_uint64, u64p, u32p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.mtblx_encode_plan.restype = C.c_int
        L.mtblx_encode_workspace_bytes.argtypes = [C.c_uint32]
        L.mtblx_encode_workspace_bytes.restype = C.c_size_t
        L.mtblx_encode_blocks.argtypes = [C.POINTER(Records), C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p,
                                          C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_size_t, C.c_void_p]
        L.mtblx_encode_blocks.restype = C.c_int
        L.mtblx_plan_keep_bytes.argtypes = [C.c_uint64]
        L.mtblx_plan_keep_bytes.restype = C.c_size_t
        L.mtblx_encode_plan_keep.argtypes = L.mtblx_encode_plan.argtypes[:-3] + [C.c_void_p, C.c_size_t, C.c_void_p,
                                                                                 C.c_size_t, C.c_void_p]
        L.mtblx_plan_workspace_bytes.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_int]
        L.mtblx_plan_workspace_bytes.restype = C.c_size_t
        L.mtblx_plan_serial_workspace_bytes.argtypes = [C.c_uint32]
        L.mtblx_plan_serial_workspace_bytes.restype = C.c_size_t
        L.mtblx_encode_plan_keep.restype = C.c_int
        L.mtblx_encode_blocks_planned.argtypes = L.mtblx_encode_blocks.argtypes[:-1] + [C.c_void_p, C.c_void_p]
        L.mtblx_encode_blocks_planned.restype = C.c_int
        L.mtblx_snappy_workspace_bytes.argtypes = [C.c_uint32]
        L.mtblx_snappy_workspace_bytes.restype = C.c_size_t
        L.mtblx_snappy_dir.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.mtblx_snappy_dir.restype = C.c_int
        L.mtblx_snappy_decompress_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                                  C.c_void_p]
        L.mtblx_snappy_decompress_dev.restype = C.c_int
        L.mtblx_encode_index.argtypes = [C.POINTER(Records), C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p,
                                         C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, u64p,
                                         C.c_void_p]
        L.mtblx_encode_index.restype = C.c_int
        L.mtblx_encode_index_c.argtypes = L.mtblx_encode_index.argtypes[:-2] + [C.c_uint32, u64p, C.c_void_p]
        L.mtblx_encode_index_c.restype = C.c_int
        L.mtblx_snappy_compress_workspace_bytes.argtypes = [C.c_uint32]
        L.mtblx_snappy_compress_workspace_bytes.restype = C.c_size_t
        L.mtblx_snappy_slots.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                         C.c_void_p]
        L.mtblx_snappy_slots.restype = C.c_int
        L.mtblx_snappy_compress_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.mtblx_snappy_compress_dev.restype = C.c_int
        L.mtblx_frame_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.mtblx_frame_blocks.restype = C.c_int
        L.mtblx_codec_available.argtypes = [C.c_uint32]
        L.mtblx_codec_available.restype = C.c_int
        L.mtblx_decompress.argtypes = [C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(u8p), u64p]
        L.mtblx_decompress.restype = C.c_int
        L.mtblx_compress.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(u8p), u64p]
        L.mtblx_compress.restype = C.c_int
        L.mtblx_decompress_blocks.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                              C.POINTER(u8p), C.c_void_p, C.c_void_p, C.c_void_p]
        L.mtblx_decompress_blocks.restype = C.c_uint64
        L.mtblx_writer_set_level.argtypes = [C.c_void_p, C.c_uint32]
        L.mtblx_writer_set_level.restype = C.c_int
        L.mtblx_stream_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]
        L.mtblx_stream_copy.restype = C.c_int
        L.mtblx_index_seek_batch.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_uint64, C.c_uint64,
                                             C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.mtblx_index_seek_batch.restype = C.c_int
        L.mtblx_block_seek_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                             C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_uint64, C.c_void_p]
        L.mtblx_block_seek_batch.restype = C.c_int
        L.mtblx_block_seek_batch_kbuf.argtypes = L.mtblx_block_seek_batch.argtypes[:-1] + [C.c_void_p, C.c_uint64,
                                                                                          C.c_void_p]
        L.mtblx_block_seek_batch_kbuf.restype = C.c_int
        L.mtblx_block_seek_batch_ex.argtypes = L.mtblx_block_seek_batch_kbuf.argtypes[:-1] + [C.c_void_p, C.c_void_p]
        L.mtblx_block_seek_batch_ex.restype = C.c_int
        L.mtblx_copy_ranges.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_uint32, C.c_uint64, C.c_void_p]
        L.mtblx_copy_ranges.restype = C.c_int
        L.mtblx_entry_offsets.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                           C.c_void_p]
        L.mtblx_entry_offsets.restype = C.c_int
        L.mtblx_key_filter.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p, C.c_uint64,
                                       C.c_void_p, C.c_void_p]
        L.mtblx_key_filter.restype = C.c_int
        L.mtblx_merge_workspace_bytes.argtypes = [C.c_uint64, C.c_uint32]
        L.mtblx_merge_workspace_bytes.restype = C.c_size_t
        L.mtblx_merge_plan.argtypes = [C.POINTER(Records), C.c_uint32, u64p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.mtblx_merge_plan.restype = C.c_int
        L.mtblx_merge_plan_timed.argtypes = L.mtblx_merge_plan.argtypes + [C.POINTER(C.c_float), C.c_uint32]
        L.mtblx_merge_plan_timed.restype = C.c_int
        L.mtblx_merge_emit.argtypes = [C.POINTER(Records), C.c_uint32, C.c_int, C.POINTER(Merged), C.c_void_p,
                                       C.c_size_t, C.c_void_p]
        L.mtblx_merge_emit.restype = C.c_int
        L.mtblx_sort_workspace_bytes.argtypes = [C.c_uint64]
        L.mtblx_sort_workspace_bytes.restype = C.c_size_t
        L.mtblx_sort_plan.argtypes = [C.POINTER(Records), u64p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.mtblx_sort_plan.restype = C.c_int
        L.mtblx_sort_plan_timed.argtypes = L.mtblx_sort_plan.argtypes + [C.POINTER(C.c_float), C.c_uint32]
        L.mtblx_sort_plan_timed.restype = C.c_int
        L.mtblx_sort_emit.argtypes = [C.POINTER(Records), C.c_int, C.POINTER(Merged), C.c_void_p, C.c_size_t,
                                      C.c_void_p]
        L.mtblx_sort_emit.restype = C.c_int
        L.mtblx_merge_emit_reduce.argtypes = [C.POINTER(Records), C.c_uint32, C.POINTER(ReduceSpec), C.POINTER(Merged),
                                              C.c_void_p, C.c_size_t, C.c_void_p]
        L.mtblx_merge_emit_reduce.restype = C.c_int
        L.mtblx_sort_emit_reduce.argtypes = [C.POINTER(Records), C.POINTER(ReduceSpec), C.POINTER(Merged), C.c_void_p,
                                             C.c_size_t, C.c_void_p]
        L.mtblx_sort_emit_reduce.restype = C.c_int
        _seg = [C.POINTER(Records), C.POINTER(C.c_void_p), C.c_uint32, C.c_uint32]   # src, seg_off, nsrc, nseg
        L.mtblx_merge_seg_workspace_bytes.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
        L.mtblx_merge_seg_workspace_bytes.restype = C.c_size_t
        L.mtblx_merge_seg_plan.argtypes = _seg + [u64p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.mtblx_merge_seg_plan.restype = C.c_int
        L.mtblx_merge_seg_plan_timed.argtypes = L.mtblx_merge_seg_plan.argtypes + [C.POINTER(C.c_float), C.c_uint32]
        L.mtblx_merge_seg_plan_timed.restype = C.c_int
        L.mtblx_merge_seg_emit.argtypes = _seg + [C.c_int, C.POINTER(Merged), C.c_void_p, C.c_size_t, C.c_void_p]
        L.mtblx_merge_seg_emit.restype = C.c_int
        L.mtblx_merge_seg_emit_reduce.argtypes = _seg + [C.POINTER(ReduceSpec), C.POINTER(Merged), C.c_void_p,
                                                         C.c_size_t, C.c_void_p]
        L.mtblx_merge_seg_emit_reduce.restype = C.c_int
        L.mtblx_merge_plan_select.argtypes = [C.POINTER(Records), C.c_uint32, C.POINTER(SelectSpec), u64p, C.c_void_p,
                                              C.c_size_t, C.c_void_p]
        L.mtblx_merge_plan_select.restype = C.c_int
        L.mtblx_merge_seg_plan_select.argtypes = _seg + [C.POINTER(SelectSpec), u64p, C.c_void_p, C.c_void_p,
                                                         C.c_size_t, C.c_void_p]
        L.mtblx_merge_seg_plan_select.restype = C.c_int
        L.mtblx_scan_workspace_bytes.argtypes = [C.c_uint32]
        L.mtblx_scan_workspace_bytes.restype = C.c_size_t
        _file = [C.c_void_p, C.c_uint64, C.c_uint32]                                    # file, file_len, version
        _tab = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]  # tab_*, ntab, dec
        L.mtblx_scan_plan.argtypes = _file + [C.c_int, C.c_uint64, C.c_uint64] + _tab + [
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
            C.c_void_p, u64p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.mtblx_scan_plan.restype = C.c_int
        L.mtblx_scan_reduce.argtypes = L.mtblx_scan_plan.argtypes[:-1] + [C.POINTER(ReduceSpec), C.c_void_p,
                                                                          C.c_void_p, C.c_void_p]
        L.mtblx_scan_reduce.restype = C.c_int
        L.mtblx_reduce_segments.argtypes = [C.POINTER(Records), C.c_void_p, C.c_void_p, C.c_uint32,
                                            C.POINTER(ReduceSpec), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mtblx_reduce_segments.restype = C.c_int
        L.mtblx_reduce_seg_tile.restype = C.c_uint32
        _roll = [C.POINTER(Records), C.POINTER(Group), C.c_void_p, C.c_uint32]   # recs, group, seg_off, nseg
        L.mtblx_rollup_workspace_bytes.argtypes = [C.c_uint64, C.c_uint32]
        L.mtblx_rollup_workspace_bytes.restype = C.c_size_t
        L.mtblx_rollup_plan.argtypes = _roll + [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.mtblx_rollup_plan.restype = C.c_int
        L.mtblx_rollup_emit.argtypes = _roll + [C.POINTER(Rolled), C.c_void_p, C.c_size_t, C.c_void_p]
        L.mtblx_rollup_emit.restype = C.c_int
        L.mtblx_rollup_tile.restype = C.c_uint32
        L.mtblx_reduce_encode_workspace_bytes.argtypes = [C.c_uint64]
        L.mtblx_reduce_encode_workspace_bytes.restype = C.c_size_t
        L.mtblx_reduce_encode.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(ReduceSpec), C.c_void_p, C.c_void_p,
                                          C.c_uint64, C.c_void_p, C.c_size_t, C.c_void_p]
        L.mtblx_reduce_encode.restype = C.c_int
        L.mtblx_where_workspace_bytes.argtypes = [C.c_uint64, C.c_uint32]
        L.mtblx_where_workspace_bytes.restype = C.c_size_t
        L.mtblx_where_plan.argtypes = [C.POINTER(Records), C.POINTER(WhereSpec), C.c_void_p, C.c_uint32, u64p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.mtblx_where_plan.restype = C.c_int
        L.mtblx_where_emit.argtypes = [C.POINTER(Records), C.POINTER(Filtered), C.c_void_p, C.c_size_t, C.c_void_p]
        L.mtblx_where_emit.restype = C.c_int
        L.mtblx_where_tile.restype = C.c_uint32
        L.mtblx_scan_reduce_where.argtypes = L.mtblx_scan_reduce.argtypes[:-1] + [C.POINTER(WhereSpec), C.c_void_p,
                                                                                  C.c_void_p]
        L.mtblx_scan_reduce_where.restype = C.c_int
        L.mtblx_scan_emit.argtypes = _file + [C.c_uint64, C.c_uint64] + _tab + [
            C.c_uint32, C.POINTER(Scanned), C.c_void_p, C.c_size_t, C.c_void_p]
        L.mtblx_scan_emit.restype = C.c_int
        L.mtblx_stage_workspace_bytes.argtypes = [C.c_uint32]
        L.mtblx_stage_workspace_bytes.restype = C.c_size_t
        L.mtblx_stage_plan.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                       C.c_void_p, C.c_uint32, u64p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.mtblx_stage_plan.restype = C.c_int
        L.mtblx_stage_emit.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                       C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                       C.c_size_t, C.c_void_p]
        L.mtblx_stage_emit.restype = C.c_int
        L.mtblx_scan_touch.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                       C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
        L.mtblx_scan_touch.restype = C.c_int
        L.mtblx_bitmap_compact.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                           C.c_void_p]
        L.mtblx_bitmap_compact.restype = C.c_int
        L.mtblx_table_gather.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 9
        L.mtblx_table_gather.restype = C.c_int
        L.mtblx_dir_ascends.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.mtblx_dir_ascends.restype = C.c_int
        L.mtblx_debug_cu_limit.argtypes = [C.c_int]
        L.mtblx_debug_cu_limit.restype = C.c_int
        L.mtblx_debug_grid_items.argtypes = [C.c_int, C.c_int]
        L.mtblx_debug_grid_items.restype = C.c_uint64
        L.mtblx_debug_decode_tiles.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_int)]
        L.mtblx_debug_decode_tiles.restype = C.c_uint32
        L.mtblx_host_alloc.argtypes = [C.POINTER(C.c_void_p), C.c_uint64]
        L.mtblx_host_alloc.restype = C.c_int
        L.mtblx_host_free.argtypes = [C.c_void_p]
        L.mtblx_host_free.restype = C.c_int
        L.mtblx_host_register.argtypes = [C.c_void_p, C.c_uint64]
        L.mtblx_host_register.restype = C.c_int
        L.mtblx_host_unregister.argtypes = [C.c_void_p]
        L.mtblx_host_unregister.restype = C.c_int
        _lib = L
    return _lib

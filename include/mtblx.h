/*
 * mtblx.h — C ABI of the MI355X-native mtbl block codec (libmtblx.so).
 *
 * Drop-in boundary for Kerollmops/oxidized-mtbl's block decode seam:
 *   Reader::block -> Block::init -> BlockIter::{init, seek_to_first, next, get}
 *   (reference src/reader.rs:140-186, src/block.rs:16-49, :75-93, :119-143, :145-213,
 *    driven per record by ReaderIntoIter::next src/reader.rs:337-405).
 * The reference exposes no FFI of its own (Block/BlockIter are crate-private,
 * src/lib.rs:32-33); these entry points are what a Rust `extern "C"` shim would bind
 * to replace that seam with one batched device call (INTEGRATION.md shows the binding).
 *
 * Conventions
 *  - plain pointers + sizes only; no HIP or torch types (streams are `void*`,
 *    i.e. a hipStream_t, NULL = the null stream).
 *  - "device" = memory the kernels read/write (hipMalloc'd or host-pinned mapped).
 *  - the library never allocates on a hot call: the caller passes every buffer,
 *    including the workspace sized by mtblx_decode_workspace_bytes().
 *  - the workspace carries state from call to call (a launch counter and the per-tile
 *    look-back words of both launch parities), so a call needs no fill: ZERO-FILL IT ONCE
 *    after allocating it, then reuse it for any sequence of batches of at most the
 *    nblk it was sized for.  One workspace serves one call at a time (per stream).
 *  - calls are asynchronous on `stream` and re-entrant: the library keeps no mutable state
 *    between calls -- every scratch buffer is the caller's (the block cut's too, since ABI v3);
 *    the one process-wide datum is a per-device cache of what the hardware is (compute-unit
 *    counts, kernel occupancy: csrc/devinfo.h), filled on first use with relaxed atomics.
 *  - streams: every launch, memset and copy of a call goes to `stream`, never to the null stream
 *    unless `stream` is it; inputs must be ready in stream order on `stream`, outputs are valid in
 *    stream order on it, and a call that returns a size or a flag to the host synchronises
 *    `stream` alone.  Exceptions: mtblx_entry_offsets and mtblx_encode_index(_c) allocate and free
 *    device memory themselves, which waits for the whole device ("Streams").
 *  - return value: MTBLX_OK or a negative MTBLX_E_* (argument / HIP launch errors).
 *    Per-block outcomes are reported in `status[]` (MTBLX_ST_*), never by aborting.
 */
#ifndef MTBLX_H
#define MTBLX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTBLX_ABI_VERSION 3   /* 3: the block cut takes a caller-owned workspace (round 6).  Still 3 with
                                 mtblx_decode_blocks_valpos / mtblx_pipe_decode_valpos and with the
                                 mtblx_merge_*, mtblx_sort_*, mtblx_scan_* and mtblx_stage_* calls (the two
                                 mtblx_*_emit_reduce, mtblx_scan_reduce and mtblx_reduce_segments among
                                 them), with mtblx_rollup_* and mtblx_reduce_encode and with mtblx_where_*:
                                 added symbols, no existing one changed */

/* ---- API return codes ---- */
#define MTBLX_OK 0
#define MTBLX_E_INVAL (-1)    /* bad argument (NULL pointer, workspace too small, ...) */
#define MTBLX_E_HIP (-2)      /* a HIP runtime call failed                              */
#define MTBLX_E_NODEV (-3)    /* no gfx950 device visible                               */
#define MTBLX_E_FORMAT (-4)   /* host-side file/format error (reader API)               */
#define MTBLX_E_TIMEOUT (-5)  /* a decode launch reported a look-back timeout (totals[3] bit 1) twice:
                                 its outputs were discarded (synchronous entry points only).
                                 Worst case: a waiting wave gives up after 20 s (look-back) or
                                 21 s (hand-off inside a workgroup); with the one retry a stuck
                                 launch returns this after about 42-45 s                      */
#define MTBLX_E_IO (-6)       /* the writer's compressor returned Err (Writer::insert / into_inner's
                                 io::Error: Lz4 / Lz4hc "unsupported", src/compression.rs:70-81;
                                 a codec failure); nothing was written, but the records of the
                                 block being flushed are lost and the next insert fails (the
                                 reference's BlockBuilder::finish already ran, :85-104)       */

/* ---- per-block status (status[b]) ----
 * Exact correspondence with the reference's behaviour on the same bytes:         */
#define MTBLX_ST_OK 0            /* decoded; identical records to src/block.rs    */
#define MTBLX_ST_INVALID_BLOCK 1 /* Block::init returns None -> MtblError::InvalidBlock (src/block.rs:16-49) */
#define MTBLX_ST_CORRUPT 2       /* the reference panics (assert/unwrap/slice, src/block.rs:59,79,131-135,217-235);
                                    nrec[b] = records the reference yielded before the panic          */
#define MTBLX_ST_LOOP 3          /* zero-progress entry: the reference yields it forever; emitted once */
#define MTBLX_ST_UNSUPPORTED 4   /* block >= 4 GiB (u64 restart arrays): not decoded by this batched
                                    call (u32 lengths); mtblx_block_seek_batch decodes such blocks    */
#define MTBLX_ST_OVERFLOW 5      /* caller's key/value/record capacity exceeded; block not written    */
#define MTBLX_ST_DECOMPRESS 6    /* (mtblx_pipe_decode) host decompression failed: Reader::block returns
                                    Err(Error::Io) (src/reader.rs:166, src/compression.rs:57-68)      */

/* A batch of uncompressed block contents already resident on the device.
 * Block b occupies data[blk_off[b] .. blk_off[b] + blk_len[b]). */
typedef struct mtblx_block_batch {
  const uint8_t* data;      /* device */
  uint64_t data_len;        /* bytes readable at `data` (bounds for staging loads) */
  const uint64_t* blk_off;  /* device [nblk] */
  const uint32_t* blk_len;  /* device [nblk] */
  uint32_t nblk;
  uint32_t max_blk_len;     /* host hint: max of blk_len (selects the kernel variant); 0 = unknown */
} mtblx_block_batch;

/* Output layout (the north star's "keys and values laid out contiguously"):
 *   records of block b are global records rec_base[b] .. rec_base[b] + nrec[b]
 *   key of record i of block b  = keys[key_base[b] + (i ? key_end[r-1] : 0) .. key_base[b] + key_end[r]]
 *   value                        = vals[val_base[b] + (i ? val_end[r-1] : 0) .. val_base[b] + val_end[r]]
 *   with r = rec_base[b] + i; key_end/val_end are u32 END offsets relative to the block's base.
 * Records keep the reference's order within and across blocks. */
typedef struct mtblx_decoded {
  uint32_t* nrec;       /* device [nblk] */
  uint64_t* rec_base;   /* device [nblk] exclusive prefix of nrec            */
  uint64_t* key_base;   /* device [nblk] exclusive prefix of key bytes       */
  uint64_t* val_base;   /* device [nblk] exclusive prefix of value bytes     */
  int32_t* status;      /* device [nblk] MTBLX_ST_*                          */
  uint32_t* key_end;    /* device [rec_cap] */
  uint32_t* val_end;    /* device [rec_cap] */
  uint64_t rec_cap;
  uint8_t* keys;        /* device [keys_cap] */
  uint64_t keys_cap;
  uint8_t* vals;        /* device [vals_cap] */
  uint64_t vals_cap;
  uint64_t* totals;     /* device [4]: records, key bytes, value bytes, flags:
                             bit0 = some block's outputs overflowed the caller's capacity (its
                                    status is MTBLX_ST_OVERFLOW; totals[0..2] are still exact)
                             bit1 = LOOK-BACK TIMEOUT: NOTHING this launch wrote may be used.
                           The decode is one persistent launch whose workgroups (one per CU) hand
                           their tiles' output sizes to each other; it relies on all of them being
                           resident at once.  If another kernel holds CUs for long enough, a bounded
                           wait gives up and sets bit1.  Every reader surface of this library
                           (mtblx/codec.py, reader.py, include/mtbl.hpp, mtblx_pipe_decode) checks
                           it and raises / re-runs; a direct caller must check it too and re-run.
                           Env MTBLX_DEBUG_FLAGS (test knob): bits ORed into every launch's totals[3]. */
} mtblx_decoded;

/* Library identity / device check. */
int mtblx_abi_version(void);
int mtblx_device_ok(void); /* 1 if the current HIP device is gfx950, else 0 */

/* Workspace bytes needed by mtblx_decode_blocks for a batch of up to nblk blocks
 * (zero-fill once before first use, see above). */
size_t mtblx_decode_workspace_bytes(uint32_t nblk);

/* Decode every block of `in` into `out` (replaces Block::init + the BlockIter scan
 * seek_to_first/next/get of src/block.rs for each block; see header comment). */
int mtblx_decode_blocks(const mtblx_block_batch* in, const mtblx_decoded* out, void* workspace,
                        size_t workspace_bytes, void* stream);

/* mtblx_decode_blocks without the value bytes: val_pos[r] (device [out->rec_cap]) = offset of
 * record r's value from the start of its block's content, so the value is
 *   in->data[blk_off[b] + val_pos[r] .. + len),  len = val_end[r] - (i ? val_end[r-1] : 0)
 * -- the (val_offset, val_len) BlockIter::get slices with (src/block.rs:204-213), i.e.
 * decode_entry's p + non_shared (src/block.rs:216-238).  Defined for empty values (the byte
 * after the key suffix) and for the records a MTBLX_ST_CORRUPT / MTBLX_ST_LOOP block yields
 * before it stops; val_pos[r] + len <= blk_len[b] - 4 for every record written.
 * out->vals / out->vals_cap are ignored (may be NULL / 0), never written, never a cause of
 * MTBLX_ST_OVERFLOW (rec_cap and keys_cap still are; an overflowing block writes no val_pos).
 * Every other output, totals[2] (value bytes) and val_base included, is exactly what
 * mtblx_decode_blocks writes.  val_pos == NULL with rec_cap != 0 is MTBLX_E_INVAL.  Same
 * workspace as mtblx_decode_blocks (the two may alternate on one).  No fused-verify form: run
 * mtblx_crc32c_blocks on the same stream. */
int mtblx_decode_blocks_valpos(const mtblx_block_batch* in, const mtblx_decoded* out, uint32_t* val_pos,
                               void* workspace, size_t workspace_bytes, void* stream);

/* Sizes only (nrec, status, bases, totals); no key/value bytes are written.
 * Lets a caller size `out` exactly before mtblx_decode_blocks. */
int mtblx_count_blocks(const mtblx_block_batch* in, const mtblx_decoded* out, void* workspace,
                       size_t workspace_bytes, void* stream);

/* Second half of a count/decode split (count to size the outputs, then write).  The
 * kernel is single-pass (counting fused into the decode), so this is the same work as
 * mtblx_decode_blocks; kept so callers written against the split stay valid. */
int mtblx_decode_counted(const mtblx_block_batch* in, const mtblx_decoded* out, void* workspace,
                         size_t workspace_bytes, void* stream);

/* CRC-32C (Castagnoli, crate crc32c 0.4) of every block's content bytes: crc[b] (device
 * [nblk]).  This is the checksum Reader::block verifies before decoding a block
 * (src/reader.rs:159-164, on by default, ReaderBuilder::verify_checksums src/reader.rs:22).
 * With framed != 0 the batch addresses contents inside an mtbl file, whose framing stores
 * the checksum as the u32 LE right before each content (varint len | crc32c | content,
 * src/writer.rs:213-225): bad[b] = 1 where it differs from crc[b] -- exactly where the
 * reference's assert_eq panics -- else 0.  crc or bad may be NULL (not both).
 * Kernel: k_crc32c_mfma (CRC-32C as fp4 / f16 matrix-core GEMMs over 1 KiB steps, one
 * persistent 16-wave workgroup per CU); MTBLX_CRC_KERNEL=lanes in the environment selects the
 * VALU table kernel k_crc32c_blocks (A/B only).  Same checksums either way. */
int mtblx_crc32c_blocks(const mtblx_block_batch* in, uint32_t* crc, uint8_t* bad, int framed, void* stream);

/* mtblx_decode_blocks + the checksum of every block (f1): crc / crc_bad as
 * mtblx_crc32c_blocks (either may be NULL, not both; `framed` bit 0 as there).  The records
 * are decoded regardless -- the caller applies Reader::block's order (checksum assert before
 * Block::init, src/reader.rs:159-172).
 * Default: the decode launch, then the matrix-core CRC kernel (k_crc32c_mfma, as
 * mtblx_crc32c_blocks) on the same stream.  With
 * MTBLX_VERIFY_FUSED in `framed` the checksum is computed inside the decode launch from the
 * tiles already staged in LDS (by the look-back and loader waves); blocks above ~64 KiB
 * still take a second launch.  On gfx950 the fused form measures slower (DESIGN.md §4:
 * table-driven CRC-32C needs one LDS lookup per byte, more than the decode leaves spare). */
#define MTBLX_VERIFY_FUSED 2
int mtblx_decode_blocks_verify(const mtblx_block_batch* in, const mtblx_decoded* out, uint32_t* crc, uint8_t* crc_bad,
                               int framed, void* workspace, size_t workspace_bytes, void* stream);

/* ---- index block -> data-block directory (f3) ----
 * The index block is decoded with mtblx_decode_blocks like any block; its values are the
 * varint64 file offsets of the data blocks.  For every index entry i this does what
 * block_at_index + the framing part of Reader::block do (src/reader.rs:177-186, :139-157):
 * varint_decode64 of the value, then (FormatV1 u32 | FormatV2 varint64) content length,
 * and the content window [blk_off[i], blk_off[i] + blk_len[i]) of the file.
 * vals/val_end/val_base: the decoded index block (values blob, its block-relative value end
 * offsets, and its val_base); file: the whole mtbl file on the device.  version: 0 = V1,
 * 1 = V2 (mtblx_footer.version).  dir_st[i]: */
#define MTBLX_DIR_OK 0          /* framed; checksum and Block::init are checked by
                                   mtblx_crc32c_blocks (framed) and mtblx_decode_blocks */
#define MTBLX_DIR_PANIC 1       /* the reference panics: offset >= file length, varint on an
                                   empty value, content slice past the end of the file   */
#define MTBLX_DIR_UNSUPPORTED 2 /* content >= 4 GiB: blk_off = the content start, blk_len 0 (a batch
                                   cannot carry it); decode it with mtblx_block_seek_batch, first=1 */
int mtblx_block_dir(const uint8_t* file, uint64_t file_len, uint32_t version, const uint8_t* vals,
                    const uint32_t* val_end, uint64_t val_base, uint32_t nent, uint64_t* blk_off,
                    uint32_t* blk_len, int32_t* dir_st, void* stream);

/* ---- batched point lookups (f2) ----
 * Reader::get (src/reader.rs:111-122) for nq keys at once: index_iter.seek(key) ->
 * block_at_index -> BlockIter::seek(key) -> the first record if its key equals `key`
 * (the next index entry's first record when the seek runs past the block), with the
 * reference's exact BlockIter::seek (src/block.rs:154-194) on the raw index and data blocks.
 * Quirk kept: when the seek runs past the block and the NEXT block fails Block::init
 * (InvalidBlock), Reader::get returns the value of the last entry the seek parsed in the old
 * block (FOUND with that value), or None if it parsed none -- not an error.
 * file: the whole mtbl file on the device; index_off/index_len: the index block content
 * (host-side framing, mtblx_frame_block); verify: check each data block's crc32c as
 * Reader::block does.  keys[key_end[q-1] .. key_end[q]) = query q (device).
 * Per query: status[q], and for FOUND the value at file[val_off[q] .. + val_len[q]). */
#define MTBLX_GET_FOUND 0
#define MTBLX_GET_NONE 1    /* Ok(None)                                      */
#define MTBLX_GET_PANIC 2   /* the reference panics                          */
#define MTBLX_GET_ERR 3     /* Err(InvalidBlock)                             */
#define MTBLX_GET_LOOP 4    /* the reference never returns (zero-progress entry) */
#define MTBLX_GET_MISSING 5 /* mtblx_get_decompressed only: the lookup reached a stored block the
                               caller's table does not hold; val_off / val_len = its stored content
                               (framing valid, checksum verified when verify).  Decompress it, add
                               it to the table and run the query again. */
int mtblx_get(const uint8_t* file, uint64_t file_len, uint32_t version, int verify, uint64_t index_off,
              uint64_t index_len, const uint8_t* keys, const uint64_t* key_end, uint32_t nq, int32_t* status,
              uint64_t* val_off, uint64_t* val_len, void* stream);

/* The same for a compressed file (Snappy / Zlib / Zstd: the crate's decompress step of
 * Reader::block, src/reader.rs:166-170).  Framing and the checksum stay on the stored bytes in
 * `file`; the blocks are scanned in their decompressed form, which the caller provides (the
 * host codecs, mtblx_decompress_blocks, or the device snappy): a table of ntab blocks sorted by
 * tab_start = the file offset of the stored content (Reader::block's raw_start), whose content
 * is dec[tab_doff[i] .. + tab_dlen[i]) when tab_st[i] == 0, and Err(Io) otherwise (the
 * crate's decompress error; reported like Err(InvalidBlock)).  A stored block missing from the
 * table is reported as MTBLX_GET_MISSING with its stored extent: a corrupt index read with
 * verification off can land a seek on a block the caller's linear walk of the index never
 * reached (the reference reads, decompresses and scans it like any other).  val_off of FOUND is
 * an offset into `dec`. */
int mtblx_get_decompressed(const uint8_t* file, uint64_t file_len, uint32_t version, int verify,
                           uint64_t index_off, uint64_t index_len, const uint64_t* tab_start,
                           const uint64_t* tab_doff, const uint64_t* tab_dlen, const int32_t* tab_st, uint32_t ntab,
                           const uint8_t* dec, const uint8_t* keys, const uint64_t* key_end, uint32_t nq,
                           int32_t* status, uint64_t* val_off, uint64_t* val_len, void* stream);

/* ---- seek-based iteration (ReaderIntoIter::new_from / seek, src/reader.rs:256-335) ----
 * Three device primitives; the host drives the iterator state (block_offset quirk, first /
 * valid, index position) exactly as src/reader.rs:219-405 does, and decodes the blocks after
 * the sought one with mtblx_decode_blocks -- only the blocks the iteration touches.
 *
 * (1) index_iter.seek(key) + the landed entry's block_at_index / Reader::block
 *     (src/block.rs:154-194, src/reader.rs:139-186), one wave per query, starting from a fresh
 *     index iterator.  ReaderIntoIter::seek re-seeks its LIVE index iterator (:303); from a
 *     regular index block (mtblx_entry_offsets) every start lands on the same entry, so the
 *     drivers use this primitive there, and otherwise seek the index block itself with
 *     mtblx_block_seek_batch from the live iterator's state and key capacity
 *     (mtblx/iterator.py, include/mtbl.hpp ReaderIntoIter).  All fields are outputs. */
#define MTBLX_SEEK_OK 0
#define MTBLX_SEEK_ERR 1          /* Err(InvalidBlock) from Block::init                       */
#define MTBLX_SEEK_PANIC 2        /* the reference panics                                     */
#define MTBLX_SEEK_LOOP 3         /* the reference never returns (zero-progress entry)        */
#define MTBLX_SEEK_UNSUPPORTED 4  /* a key > 64 KiB in mtblx_block_seek_batch's LDS key (retry with
                                     mtblx_block_seek_batch_kbuf); blocks >= 4 GiB with u64
                                     restart arrays are handled: src/block.rs:25-42, :95-104    */
typedef struct mtblx_index_seek {
  int32_t status;          /* of the index seek: OK / PANIC / LOOP                               */
  int32_t valid;           /* index_iter.get() is Some after the seek                             */
  uint64_t entry;          /* the index iterator's current entry offset in the index block        */
  uint64_t block_off;      /* varint_decode64(entry value): the file offset ReaderIntoIter keeps  */
  int32_t block_status;    /* Reader::block(block_off): OK / ERR / PANIC (UNSUPPORTED >= 4 GiB);
                              ERR / UNSUPPORTED come from Block::init on the stored bytes, which
                              is only meaningful for uncompressed files                        */
  int32_t pad;
  uint64_t data_off, data_len;   /* the block content (framed; crc32c checked when verify)       */
} mtblx_index_seek;
int mtblx_index_seek_batch(const uint8_t* file, uint64_t file_len, uint32_t version, int verify,
                           uint64_t index_off, uint64_t index_len, const uint8_t* keys, const uint64_t* key_end,
                           uint32_t nq, mtblx_index_seek* out, void* stream);

/* (2) BlockIter::seek(key) (or seek_to_first) on one block content, then the records the
 *     iterator yields from there (get / next until get() is None), keys materialised.  One
 *     workgroup per query.  kcap = the iterator's key Vec capacity (src/block.rs:132 asserts
 *     on it): 0 for a fresh BlockIter::init, or a re-seeked iterator's.  Query q writes its
 *     records to out_keys + q*keys_cap, out_vals + q*vals_cap, and END offsets (relative to
 *     the query's base) to key_end_out/val_end_out + q*rec_cap, plus the iterator's key
 *     capacity at each record to kcap_out + q*rec_cap (may be NULL).  On OVERFLOW the counts
 *     are what is needed.  keys: the seek targets (ignored for first). */
#define MTBLX_EMIT_END 0        /* get() returned None: the block is exhausted                 */
#define MTBLX_EMIT_PANIC 1      /* next() / get() panics after the emitted records             */
#define MTBLX_EMIT_LOOP 2       /* next() never returns after the emitted records              */
#define MTBLX_EMIT_MAX 3        /* max_records emitted                                         */
#define MTBLX_EMIT_OVERFLOW 4   /* a capacity was too small (counts = needed)                  */
typedef struct mtblx_block_seek {
  uint64_t data_off, data_len;   /* in: block content in `data`                                  */
  uint64_t kcap;                 /* in: key capacity (0 = fresh); out: after the emitted records  */
  uint64_t max_records;          /* in                                                            */
  int32_t first;                 /* in: 0 = seek(key); 1 = seek_to_first; 2 = resume: the iterator
                                    holds key = keys[q] (its current key bytes) and kcap, and its
                                    next() parses the entry at resume_off (BlockIter::next,
                                    src/block.rs:196-202) -- the records from there are emitted  */
  int32_t status;                /* out: MTBLX_SEEK_* of Block::init / BlockIter::init / the seek */
  int32_t end;                   /* out: MTBLX_EMIT_*                                             */
  int32_t has_val;               /* out: an entry was parsed (BlockIter::val is Some)             */
  uint64_t entry;                /* out: the iterator's current entry offset after the seek       */
  uint64_t nrec, key_bytes, val_bytes;   /* out                                                   */
  uint64_t last_voff, last_vlen; /* out: `val` of the last parsed entry (content offsets) -- what
                                    Reader::get returns when next() hits Err (src/reader.rs:111-122) */
  uint64_t resume_off;           /* in (first == 2): offset of the entry next() parses            */
  uint64_t stop_off;             /* out: the iterator's current entry offset when the emission
                                    stopped; after MTBLX_EMIT_MAX: the entry after the last
                                    emitted record (resume there with that record's key / kcap) */
  int32_t early;                 /* out (first == 0): the binary search returned early on a restart
                                    entry with shared != 0 (src/block.rs:167-170): a live iterator
                                    keeps its previous position; nothing after it applies       */
  int32_t pad;
} mtblx_block_seek;
int mtblx_block_seek_batch(const uint8_t* data, const uint8_t* keys, const uint64_t* key_end, uint32_t nq,
                           mtblx_block_seek* q, uint8_t* out_keys, uint64_t keys_cap, uint8_t* out_vals,
                           uint64_t vals_cap, uint64_t* key_end_out, uint64_t* val_end_out, uint64_t* kcap_out,
                           uint64_t rec_cap, void* stream);
/* (2') the same with the iterator's key kept in a caller buffer, key_buf + q * key_buf_cap
 *      (device), instead of 64 KiB of LDS: keys of any length.  mtblx_block_seek_batch reports a
 *      key past 64 KiB as status MTBLX_SEEK_UNSUPPORTED; here that means past key_buf_cap.  A
 *      key never exceeds len(keys[q]) + data_len bytes (every byte after the target's comes from
 *      a distinct suffix in the block), so that capacity always suffices. */
int mtblx_block_seek_batch_kbuf(const uint8_t* data, const uint8_t* keys, const uint64_t* key_end, uint32_t nq,
                                mtblx_block_seek* q, uint8_t* out_keys, uint64_t keys_cap, uint8_t* out_vals,
                                uint64_t vals_cap, uint64_t* key_end_out, uint64_t* val_end_out, uint64_t* kcap_out,
                                uint64_t rec_cap, uint8_t* key_buf, uint64_t key_buf_cap, void* stream);
/* (2'') the same with the value bytes left to the caller (blocks >= 4 GiB hold values of GiBs):
 *      record r of query q gets val_end_out as above and val_src_out[q * rec_cap + r] = its value's
 *      offset in the block content; out_vals is not written (may be NULL) and vals_cap only sizes
 *      the emission.  The caller then moves the bytes with mtblx_copy_ranges (the whole grid).
 *      key_buf == NULL: the key in LDS as mtblx_block_seek_batch; else as _kbuf. */
int mtblx_block_seek_batch_ex(const uint8_t* data, const uint8_t* keys, const uint64_t* key_end, uint32_t nq,
                              mtblx_block_seek* q, uint8_t* out_keys, uint64_t keys_cap, uint8_t* out_vals,
                              uint64_t vals_cap, uint64_t* key_end_out, uint64_t* val_end_out, uint64_t* kcap_out,
                              uint64_t rec_cap, uint8_t* key_buf, uint64_t key_buf_cap, uint64_t* val_src_out,
                              void* stream);

/* (3) the offsets of the entries seek_to_first + next visit in a block (the index block: entry
 *     i <-> index record i <-> directory entry i), so a seek's landed entry maps to its index
 *     position.  Parallel over restart intervals when every interval's chain lands on the next
 *     restart point; otherwise one serial walk.  Writes min(count, cap) offsets; *count (device)
 *     = entries up to the end of the block or the first entry the scan cannot decode.
 *     *regular (device u32, may be NULL) = 1 when every interval's chain lands on the next
 *     restart point, every restart entry has shared == 0 and every other entry shared <= the
 *     previous key's length.  For such an index block a seek from ANY iterator state (fresh or
 *     live, any key capacity) never returns early, lands on the scan chain, rebuilds the scan's
 *     keys and cannot hit the key-capacity assert: the host may then follow the directory
 *     (entries i+1, i+2, ...) after a seek.  Otherwise the host drives the live index iterator
 *     with mtblx_block_seek_batch (seek / resume) over the index block.  Synchronous: returns
 *     after the launch completed (its scratch is freed then). */
int mtblx_entry_offsets(const uint8_t* block, uint64_t len, uint64_t* offs, uint64_t cap, uint64_t* count,
                        uint32_t* regular, void* stream);

/* (4) ReaderIntoIter's stop rules (src/reader.rs:385-402) over decoded records: the index of
 *     the first record whose key fails (type 1 Get: != k, 2 GetPrefix: !starts_with(k), 3
 *     GetRange: > k), or n.  key_end: absolute END offsets (int64).  *first_fail (device) is
 *     min-reduced: set it to n before the call. */
int mtblx_key_filter(const uint8_t* keys, const uint64_t* key_end, uint64_t n, int32_t type, const uint8_t* k,
                     uint64_t klen, uint64_t* first_fail, void* stream);

/* ---- batched scans: iter_from / get / iter_prefix / iter_range for nq queries at once ----
 * Per query the whole ReaderIntoIter loop (new_from + next(), src/reader.rs:256-405) runs on the
 * device: the index seek on a fresh iterator, Reader::block (framing, checksum when verify, the
 * caller's decompressed-block table as mtblx_get_decompressed), BlockIter::seek(start), records
 * while the stop rule holds (Get: == k, GetPrefix: starts_with(k), GetRange: <= k2), and at a
 * block's end the next index entry's block from its first record.
 *
 * Two calls, as the Merger.  mtblx_scan_plan (synchronous) walks every query once without writing
 * a record, counts it, scans the counts of the OK queries in query order into per-query output
 * offsets and returns the totals.  mtblx_scan_emit (asynchronous) walks the OK queries again from
 * the landing the plan saved and writes their records.  The caller owns the workspace (device,
 * 256-byte aligned, mtblx_scan_workspace_bytes; no fill needed; one call at a time).
 *
 * Per query, res[q].status:
 *   MTBLX_SCAN_OK        the records are in the output; the iteration ended with None (end = 0) or
 *                        at max_records[q] (end = 1).
 *   MTBLX_SCAN_LARGE     the iteration would open more than max_blocks data blocks (every
 *                        Reader::block call counts, the sought block included).  Counts 0, nothing
 *                        emitted: a scan of many blocks belongs to the full-rate decoder.
 *   MTBLX_SCAN_FALLBACK  anything else: the reference would panic, return Err or never return
 *                        somewhere on this query's path (a checksum mismatch with verify included),
 *                        a block content >= 4 GiB, a compressed block missing from the table, or a
 *                        key longer than MTBLX_SCAN_MAX_KEY bytes among the entries the walk parses.
 *                        Counts 0, nothing emitted: the caller runs the query through the exact
 *                        seek primitives above, which keep every such quirk.
 * Corrupt files read with verify = 0 are supported input: every such condition is detected and no
 * access leaves the file, the table's blocks, the workspace or the outputs.
 *
 * type (HOST array [nq]): 0 from, 1 get, 2 prefix, 3 range -- mtblx_key_filter's numbering; get is
 * Reader::get (src/reader.rs:111-122), which takes the iterator's first record only.  keys /
 * key_end (device, u64 END offsets): the start key / prefix of query q.  keys2 / key2_end (device):
 * the inclusive range end, read only for type 3; both may be NULL when no query is a range.
 * max_records (device [nq], may be NULL = no limit).  res: device [nq].  totals: host [4] = records,
 * key bytes, value bytes of the OK queries, and the number of queries not OK.
 *
 * MTBLX_E_INVAL before any device call: NULL or misaligned workspace, ws_bytes too small, a type
 * outside 0..3, version > 1, a NULL required pointer.  nq == 0: MTBLX_OK with zero totals. */
#define MTBLX_SCAN_OK 0
#define MTBLX_SCAN_LARGE 1
#define MTBLX_SCAN_FALLBACK 2
#define MTBLX_SCAN_MAX_KEY 1024          /* bytes of the emit kernel's per-wave key buffer (LDS)      */
#define MTBLX_SCAN_OVERFLOW 1u           /* *flags of mtblx_scan_emit: a capacity was too small; no
                                            record that does not fit whole is written               */
#define MTBLX_SCAN_NOT_PLANNED 2u        /* *flags: the workspace is not that of a mtblx_scan_plan of
                                            nq queries; nothing was written                         */
#define MTBLX_SCAN_INTERNAL 4u           /* *flags: the emit walk met a count that differs from the
                                            plan's (a bug); it never writes outside the query's slot */
typedef struct mtblx_scan_result {
  int32_t status;                          /* MTBLX_SCAN_*                                          */
  int32_t end;                             /* OK: 0 = the iterator returned None, 1 = max_records   */
  uint64_t nrec, key_bytes, val_bytes;     /* of this query (0 unless OK)                           */
  uint64_t rec_base, key_base, val_base;   /* exclusive offsets of this query into the outputs: the
                                              scan of the three counts over the OK queries before it */
  uint32_t blocks;                         /* data blocks opened                                    */
  uint32_t pad;
} mtblx_scan_result;
/* Output of mtblx_scan_emit (device buffers; keys_cap / vals_cap in bytes, rec_cap in records).
 * key_end / val_end are u64 END offsets counted from record 0 of the whole batch: keys, key_end,
 * vals, val_end and n = totals[0] are an mtblx_records as they stand; query q's records are
 * [rec_base, rec_base + nrec). */
typedef struct mtblx_scanned {
  uint8_t* keys;
  uint64_t keys_cap;
  uint8_t* vals;
  uint64_t vals_cap;
  uint64_t* key_end;
  uint64_t* val_end;
  uint64_t rec_cap;
  uint32_t* flags;                         /* device u32, written by the emit: MTBLX_SCAN_* bits   */
} mtblx_scanned;
size_t mtblx_scan_workspace_bytes(uint32_t nq);
int mtblx_scan_plan(const uint8_t* file, uint64_t file_len, uint32_t version, int verify, uint64_t index_off,
                    uint64_t index_len, const uint64_t* tab_start, const uint64_t* tab_doff, const uint64_t* tab_dlen,
                    const int32_t* tab_st, uint32_t ntab, const uint8_t* dec, const int32_t* type,
                    const uint8_t* keys, const uint64_t* key_end, const uint8_t* keys2, const uint64_t* key2_end,
                    const uint64_t* max_records, uint32_t max_blocks, uint32_t nq, mtblx_scan_result* res,
                    uint64_t* totals, void* workspace, size_t ws_bytes, void* stream);
/* dec == NULL: the file is not compressed (the table arguments are ignored). */
int mtblx_scan_emit(const uint8_t* file, uint64_t file_len, uint32_t version, uint64_t index_off, uint64_t index_len,
                    const uint64_t* tab_start, const uint64_t* tab_doff, const uint64_t* tab_dlen,
                    const int32_t* tab_st, uint32_t ntab, const uint8_t* dec, uint32_t nq, const mtblx_scanned* out,
                    const void* workspace, size_t ws_bytes, void* stream);

/* ---- encode side on the device: Writer's block cut + BlockBuilder + write_block framing ----
 * Records (device): key r = keys[r ? key_end[r-1] : 0 .. key_end[r]), value likewise (u64 END
 * offsets from record 0), in Writer::insert order (strictly increasing keys). */
typedef struct mtblx_records {
  const uint8_t* keys;
  const uint64_t* key_end;
  const uint8_t* vals;
  const uint64_t* val_end;
  uint64_t n;
} mtblx_records;

/* Writer::insert's flush rule (src/writer.rs:125-130 with BlockBuilder::current_size_estimate,
 * src/block_builder.rs:40-47): where the Writer would cut blocks.  Each shard s = records
 * [shard_rec[s], shard_rec[s+1]) (device) is an independent Writer (one file each; one shard
 * = one file); blocks of all shards are numbered consecutively: block b = records
 * [blk_rec[b], blk_rec[b+1]) (device, capacity blk_cap >= nblk + 1; blk_rec may be NULL to
 * count only).  block_size is clamped to >= 1024 like WriterBuilder::block_size.
 * Synchronous; *nblk_out = number of blocks.  Returns MTBLX_E_FORMAT where the Writer
 * panics; *flags_out tells why: */
#define MTBLX_PLAN_OUT_OF_ORDER 1u /* a key <= its predecessor: panic!("out-of-order key") (:119-123) */
#define MTBLX_PLAN_PANIC 2u        /* restart_interval 0 and a second entry: assert (src/block_builder.rs:50) */
#define MTBLX_PLAN_TOO_LONG 4u     /* a key or value >= 4 GiB (u32 varint lengths)                    */
/* Scratch (device, 256-byte aligned, no fill needed) of the parallel cut for up to `nrec` records in
 * `nshard` shards at this interval; keep != 0 for mtblx_encode_plan_keep (whose entry sizes live in
 * the plan buffer).  A bound that holds for any record sizes, ~50 B per record.  The library keeps
 * no scratch between calls: one workspace serves one call at a time. */
size_t mtblx_plan_workspace_bytes(uint64_t nrec, uint32_t nshard, uint32_t restart_interval, int keep);
/* The serial walk's scratch (one wave per shard, the round-1..4 cut): 16 B per shard. */
size_t mtblx_plan_serial_workspace_bytes(uint32_t nshard);
/* workspace: at least mtblx_plan_workspace_bytes(records of the shards, nshard, restart_interval, 0)
 * runs the parallel cut (every record's next block start at once + pointer doubling); a smaller one,
 * of at least mtblx_plan_serial_workspace_bytes(nshard), the serial walk (same cut; also taken for
 * record ranges of 2^32 - 16 or more and under MTBLX_PLAN=serial).  NULL or misaligned: MTBLX_E_INVAL. */
int mtblx_encode_plan(const mtblx_records* rec, const uint64_t* shard_rec, uint32_t nshard, uint64_t block_size,
                      uint32_t restart_interval, uint64_t* blk_rec, uint64_t blk_cap, uint64_t* nblk_out,
                      uint32_t* flags_out, void* workspace, size_t ws_bytes, void* stream);

/* The same block cut, keeping what the encode needs (round 5): `plan` (device, 256-byte aligned,
 * mtblx_plan_keep_bytes(number of records in the shards) bytes) receives every record's entry size
 * summed in order, the bytes a restart entry loses by not sharing summed along residue classes
 * mod restart_interval, and every record's shared-prefix length with its predecessor (across shard
 * starts too).  restart_interval must be >= 1, the shards must hold fewer than 2^32 - 16 records and
 * the workspace at least mtblx_plan_workspace_bytes(..., keep = 1): otherwise MTBLX_E_INVAL (no
 * serial fallback: cut with mtblx_encode_plan and encode with mtblx_encode_blocks instead).
 * Returns like mtblx_encode_plan. */
size_t mtblx_plan_keep_bytes(uint64_t nrec);
/* ABI v2 compatibility: a no-op (the cut used to cache its scratch; it keeps none now). */
void mtblx_plan_release(void);
int mtblx_encode_plan_keep(const mtblx_records* rec, const uint64_t* shard_rec, uint32_t nshard, uint64_t block_size,
                           uint32_t restart_interval, uint64_t* blk_rec, uint64_t blk_cap, uint64_t* nblk_out,
                           uint32_t* flags_out, void* plan, size_t plan_bytes, void* workspace, size_t ws_bytes,
                           void* stream);

/* BlockBuilder::add for every record of a block, then finish (src/block_builder.rs:49-104),
 * for every block b of blk_rec at once.  framed != 0 adds write_block's framing before each
 * content (varint64 len | crc32c | content, src/writer.rs:203-237, CompressionType::None):
 * the blocks then sit back to back from out[0], byte-identical to the data-block region of
 * the file Writer produces.  blk_off[b]/blk_len[b] = content window in `out` (the decode
 * batch directory); status[b] = MTBLX_ST_OK, _CORRUPT (BlockBuilder assert), _UNSUPPORTED
 * (>= 4 GiB), _OVERFLOW (out_cap); totals (device [2]) = bytes written, flags (bit 0: a
 * block not OK, bit 1: look-back timeout).  Asynchronous on `stream`; the workspace
 * (mtblx_encode_workspace_bytes) is cleared by the call. */
size_t mtblx_encode_workspace_bytes(uint32_t nblk);
int mtblx_encode_blocks(const mtblx_records* rec, const uint64_t* blk_rec, uint32_t nblk, uint32_t restart_interval,
                        int framed, uint8_t* out, uint64_t out_cap, uint64_t* blk_off, uint32_t* blk_len,
                        int32_t* status, uint64_t* totals, void* workspace, size_t ws_bytes, void* stream);
/* mtblx_encode_blocks reading a kept plan (mtblx_encode_plan_keep over the same records and
 * restart_interval; blk_rec may be any cut of records inside it): every block's length and file
 * offset come from the kept sums and one scan, so no block waits on its predecessors, and no
 * entry's shared prefix is recomputed.  Output identical to mtblx_encode_blocks.  Asynchronous
 * after one small synchronous read of the plan's header. */
int mtblx_encode_blocks_planned(const mtblx_records* rec, const uint64_t* blk_rec, uint32_t nblk,
                                uint32_t restart_interval, int framed, uint8_t* out, uint64_t out_cap,
                                uint64_t* blk_off, uint32_t* blk_len, int32_t* status, uint64_t* totals,
                                void* workspace, size_t ws_bytes, const void* plan, void* stream);

/* Writer::into_inner's tail on the device (src/writer.rs:132-138, :155-181, :239-265;
 * src/metadata.rs:61-79) for ONE file whose data blocks mtblx_encode_blocks wrote framed:
 * data[region_off .. region_off + data_bytes) holds them back to back; blk_off/blk_len (device
 * [nblk], offsets relative to `data`) and blk_rec (device [nblk + 1], absolute record indices
 * into rec) are that call's directory and plan for this file.  Writes the whole file to
 * `file` (device; the data region is copied unless file == data + region_off): the data
 * blocks, then the index block -- one entry per data block, key = bytes_shortest_separator(
 * its last key, the next block's first key) with the crate's write_u16 APPEND quirk (the
 * last block's entry keeps the file's last key), value = varint64(the block's file offset)
 * -- built by BlockBuilder with `restart_interval` and framed with CompressionType::None,
 * then the 512-byte footer (block_size clamped to >= 1024 as WriterBuilder::block_size).
 * nblk == 0 writes the empty file.  Synchronous (allocates its temporaries: once per file);
 * every copy it makes, the footer's read-backs of blk_rec and the END offsets included, is
 * queued on `stream`.  The two ends of the cut are checked before anything is launched:
 * blk_rec[0] <= blk_rec[nblk] <= rec->n, else MTBLX_E_INVAL and nothing is written.  Only the
 * ends: the entries in between must ascend, which the kernels trust as mtblx_encode_blocks does.
 * *file_len = bytes written.  Byte-identical to the crate's Writer for the same records. */
int mtblx_encode_index(const mtblx_records* rec, const uint64_t* blk_rec, uint32_t nblk, uint64_t block_size,
                       uint32_t restart_interval, const uint8_t* data, uint64_t region_off, uint64_t data_bytes,
                       const uint64_t* blk_off, const uint32_t* blk_len, uint8_t* file, uint64_t file_cap,
                       uint64_t* file_len, void* stream);
/* mtblx_encode_index for data blocks stored with `compression` (the footer's
 * compression_algorithm, src/metadata.rs:69: 0 None, 1 Snappy): the region holds the blocks
 * framed as stored (mtblx_frame_blocks), blk_off/blk_len address the STORED contents, and
 * data_bytes (bytes_data_blocks, the index block's offset) is the stored region's size.  The
 * index block itself stays CompressionType::None (src/writer.rs:165-173).  mtblx_encode_index
 * is this call with compression = 0. */
int mtblx_encode_index_c(const mtblx_records* rec, const uint64_t* blk_rec, uint32_t nblk, uint64_t block_size,
                         uint32_t restart_interval, const uint8_t* data, uint64_t region_off, uint64_t data_bytes,
                         const uint64_t* blk_off, const uint32_t* blk_len, uint8_t* file, uint64_t file_cap,
                         uint32_t compression, uint64_t* file_len, void* stream);

/* ---- snappy raw compression on the device: the device Writer's CompressionType::Snappy ----
 * write_block's compression step (src/writer.rs:213-214 -> src/compression.rs:126-130,
 * snap::raw::Encoder::compress_vec) for a batch of blocks, and its framing of the stored bytes.
 * Block b's uncompressed content is src[src_off[b] .. + src_len[b]) (device, any alignment);
 * each is compressed on its own into a Snappy raw stream: varint32 length, literal, copy-1 and
 * copy-2 elements (no copy-4), no match across a 64 KiB fragment boundary; src_len 0 gives the
 * single byte 0x00.  The compressed bytes are valid Snappy that decodes to the block; they are
 * not the host compressor's bytes (neither is pinned to the reference's).  Equal inputs give
 * equal bytes, run after run.
 *
 * mtblx_snappy_slots: the output layout: dst_off[b] = the exclusive prefix of
 * mtblx_snappy_max_compressed_len(src_len[b]) rounded up to 16 bytes; totals (device [1]) =
 * the bytes the slots need.
 *
 * mtblx_snappy_compress_dev: block b's stream goes to dst[dst_off[b] .. + dst_len[b]).  Its
 * slot ends at dst_off[b + 1] (dst_off non-decreasing; the last slot ends at dst_cap).
 * status[b] = MTBLX_ST_OK, or MTBLX_ST_OVERFLOW when the slot is smaller than
 * mtblx_snappy_max_compressed_len(src_len[b]) or runs past dst_cap: nothing is written for
 * that block and dst_len[b] = 0.  {dst, dst_off, dst_len} is directly the input of
 * mtblx_snappy_dir / mtblx_snappy_decompress_dev and of mtblx_frame_blocks.
 *
 * mtblx_frame_blocks: write_block's framing (src/writer.rs:203-237) over nblk stored contents:
 * out = varint64(len) | crc32c(content) LE | content, back to back from out[0];
 * blk_off[b] (device [nblk]) = the content's start in out; totals (device [2]) = bytes
 * written, flags (bit 0: out_cap too small, the blocks that do not fit are not written).
 * The checksums come from mtblx_crc32c_blocks' kernel, which reads whole aligned 16-byte
 * chunks: up to 15 bytes around a range inside the aligned 16 bytes holding its ends.
 * workspace: mtblx_snappy_compress_workspace_bytes(nblk) bytes (device, 4-byte aligned, no fill);
 * nblk == 0 writes totals = {0, 0} and takes none (NULL allowed, as for the other two calls).
 *
 * All three are asynchronous on `stream`, keep no library-owned scratch and never synchronise
 * with the host.  workspace may be NULL for the first two (they use none today). */
size_t mtblx_snappy_compress_workspace_bytes(uint32_t nblk);
int mtblx_snappy_slots(const uint32_t* src_len, uint32_t nblk, uint64_t* dst_off, uint64_t* totals, void* workspace,
                       size_t ws_bytes, void* stream);
int mtblx_snappy_compress_dev(const uint8_t* src, const uint64_t* src_off, const uint32_t* src_len, uint32_t nblk,
                              uint8_t* dst, uint64_t dst_cap, const uint64_t* dst_off, uint32_t* dst_len,
                              int32_t* status, void* workspace, size_t ws_bytes, void* stream);
int mtblx_frame_blocks(const uint8_t* src, const uint64_t* src_off, const uint32_t* src_len, uint32_t nblk,
                       uint8_t* out, uint64_t out_cap, uint64_t* blk_off, uint64_t* totals, void* workspace,
                       size_t ws_bytes, void* stream);

/* ---- Merger on the device: k-way merge of sorted sources, duplicate keys grouped (src/merger.rs) ----
 * nsrc sources (host array of mtblx_records with device pointers, keys strictly increasing within a
 * source; keys / vals may be NULL where every key / value of the source is empty) are merged into
 * what MergerIter / MultiIter yield (src/merger.rs:172-260): one item per distinct key, in key
 * order (unsigned bytes, then length: Vec<u8>::cmp), carrying every source's value for that key.
 *  - Order inside a group.  The reference drains a BinaryHeap whose Ord looks at the key only
 *    (:45-49), so its order of equal keys is unspecified; what is taken from it is the order of
 *    keys and the multiset of values per key.  This library promises more: the values of a group
 *    are in source order (the order of `src`).
 *  - The empty-key quirk (:182-186, :236-240: cur_key.is_empty() doubles as "no current key").  The
 *    records with the empty key (at most one per source, its first) vanish -- key and values --
 *    when any other record exists; when none does, one item ("", [v]) comes out, v being the value
 *    taken last and the merge function not called.  Where the reference's v depends on heap order
 *    (two or more sources, each holding only the empty key), v here is the highest-numbered
 *    source's.  totals[4] counts the records dropped this way.
 *  - An out-of-order source (a key <= its predecessor) is refused: mtblx_merge_plan returns
 *    MTBLX_E_FORMAT with MTBLX_MERGE_UNSORTED in totals[5] (other totals 0).  The reference does
 *    not check; its output for such input is an accident of the heap and is not reproduced.
 *  - Limits: at most MTBLX_MERGE_MAX_SOURCES sources per call (more: MTBLX_E_INVAL; merge in rounds
 *    with the same mode, exact because source order is kept -- mtblx/merger.py and mtbl.hpp do),
 *    fewer than MTBLX_MERGE_MAX_RECORDS records in all sources together (u32 handles).
 * Two calls: mtblx_merge_plan (synchronous) builds one 16-byte handle per record, merges the handles
 * in ceil(log2 nsrc) passes, finds the groups and returns the output sizes in totals (host, 6 words):
 *   [0] groups  [1] key bytes of the groups  [2] values in all groups  [3] value bytes in all groups
 *   [4] records dropped by the empty-key quirk  [5] flags (MTBLX_MERGE_UNSORTED / _INTERNAL)
 * which size every mode's output exactly: keys [1] bytes, key_end [0] entries; GROUPS: vals [3]
 * bytes, val_end [2] entries, grp_end [0] entries; CONCAT: vals [3] bytes, val_end [0] entries;
 * FIRST / LAST: val_end [0] entries and vals at most [3] bytes (an upper bound: the bytes written
 * are val_end[groups - 1]).  mtblx_merge_emit (asynchronous) then reads the planned workspace with
 * the same sources and writes the outputs.  The workspace (device, 256-byte aligned,
 * mtblx_merge_workspace_bytes; no fill needed; one call at a time) holds the two handle arrays and
 * the grouping arrays, ~90 B per record.  nsrc == 0 and sources with n == 0 are legal. */
#define MTBLX_MERGE_MAX_SOURCES 64
#define MTBLX_MERGE_MAX_RECORDS 0xFFFFFFF0ull   /* 2^32 - 16 */
#define MTBLX_MERGE_GROUPS 0   /* MultiIter: key g has values grp_end[g-1] .. grp_end[g], one val_end per value */
#define MTBLX_MERGE_CONCAT 1   /* one value per key: the group's values joined in source order (the merge
                                  function of the reference's own tests, src/merger.rs:269-275)            */
#define MTBLX_MERGE_FIRST 2    /* the lowest-numbered source's value (oldest wins)                        */
#define MTBLX_MERGE_LAST 3     /* the highest-numbered source's value (newest wins)                       */
#define MTBLX_MERGE_UNSORTED 1u     /* totals[5]: a source's key <= its predecessor                      */
#define MTBLX_MERGE_INTERNAL 2u     /* totals[5]: a merge pass met a split it could not use (a bug)      */
#define MTBLX_MERGE_OVERFLOW 1u     /* *flags of mtblx_merge_emit: a capacity was too small              */
#define MTBLX_MERGE_NOT_PLANNED 2u  /* *flags: the workspace is not that of a successful mtblx_merge_plan
                                       over sources of these record counts; nothing was written          */
/* Output of mtblx_merge_emit.  Every capacity is in BYTES; an entry or a key / value that does not
 * fit entirely is not written at all (MTBLX_MERGE_OVERFLOW in *flags), nothing past a capacity is.
 * In the three single-value modes keys / key_end / vals / val_end are exactly an mtblx_records of
 * totals[0] records: they feed mtblx_encode_plan / mtblx_encode_blocks with no reshaping. */
typedef struct mtblx_merged {
  uint8_t* keys;       /* device: key of group g = keys[key_end[g-1] .. key_end[g])                       */
  uint64_t keys_cap;
  uint64_t* key_end;   /* device [groups], u64 END offsets                                               */
  uint64_t key_end_cap;
  uint8_t* vals;
  uint64_t vals_cap;
  uint64_t* val_end;   /* device, u64 END offsets: [values] in MTBLX_MERGE_GROUPS, else [groups]         */
  uint64_t val_end_cap;
  uint64_t* grp_end;   /* device [groups], u64 END index into the value list; MTBLX_MERGE_GROUPS only
                          (else never written, may be NULL)                                            */
  uint64_t grp_end_cap;
  uint32_t* flags;     /* device word, cleared by the call: MTBLX_MERGE_OVERFLOW / _NOT_PLANNED           */
} mtblx_merged;
size_t mtblx_merge_workspace_bytes(uint64_t nrec, uint32_t nsrc);
int mtblx_merge_plan(const mtblx_records* src, uint32_t nsrc, uint64_t* totals, void* workspace, size_t ws_bytes,
                     void* stream);
int mtblx_merge_emit(const mtblx_records* src, uint32_t nsrc, int mode, const mtblx_merged* out,
                     const void* workspace, size_t ws_bytes, void* stream);
/* diagnostic (scripts/merge_bench.py): mtblx_merge_plan, plus the HIP-event time in ms of each of
 * its phases: phase_ms[0] the handle build (shared prefix, handles, order check), [1 .. passes] the
 * merge passes (passes = ceil(log2 nsrc)), [passes + 1] the grouping.  phase_cap >= passes + 2. */
int mtblx_merge_plan_timed(const mtblx_records* src, uint32_t nsrc, uint64_t* totals, void* workspace,
                           size_t ws_bytes, void* stream, float* phase_ms, uint32_t phase_cap);

/* ---- Sorter on the device: one batch of unsorted records, duplicate keys grouped (src/sorter.rs) ----
 * `in` is ONE mtblx_records batch on the device: keys in any order, duplicate keys and empty keys
 * allowed, keys / vals NULL where every key / value is empty, n < MTBLX_MERGE_MAX_RECORDS.  The
 * result is what Sorter::write_chunk (src/sorter.rs:142-197) writes for these records: keys
 * ascending by Vec<u8>::cmp, one item per distinct key.  totals[0..5], mtblx_merged, the four
 * MTBLX_MERGE_* modes, MTBLX_MERGE_OVERFLOW / _NOT_PLANNED and the two-call shape (plan synchronous,
 * emit asynchronous, every capacity in bytes) are those of mtblx_merge_*, with two differences:
 *  - The values of a key come out in INPUT order (record index), so FIRST / LAST are the first /
 *    last inserted and CONCAT joins in insertion order.  The reference promises nothing here
 *    (sort_unstable_by, :152); this library promises stability, as the merge promises source order.
 *  - No empty-key quirk in this call: write_chunk keeps its current key in an Option (:154-188),
 *    not behind cur_key.is_empty(), so the empty-key group is kept like any other and totals[4] is
 *    always 0.  The quirk enters where the reference has it: in the Merger that the Sorter runs
 *    over its chunks (mtblx/sorter.py, mtbl::Sorter).  There is no order to check either:
 *    totals[5] can only carry MTBLX_MERGE_INTERNAL.
 * How: the bytes every key shares are found by one pass over all keys (the minimum common prefix
 * with record 0's key); workgroups sort tiles of MTBLX_SORT_TILE handles in LDS into sorted runs;
 * ceil(log2 ceil(n / MTBLX_SORT_TILE)) passes of the Merger's merge pass join the runs; grouping
 * and gather are the Merger's.  The workspace (device, 256-byte aligned,
 * mtblx_sort_workspace_bytes; no fill needed; one call at a time) has the Merger's layout, ~90 B
 * per record; its planned mark differs from the Merger's, so an emit of one kind over a workspace
 * planned by the other reports MTBLX_MERGE_NOT_PLANNED and writes nothing.  n == 0 is legal.
 * MTBLX_E_INVAL, before any device work: NULL or misaligned workspace, workspace too small, bad
 * mode, n >= MTBLX_MERGE_MAX_RECORDS, n != 0 with a NULL END array. */
#define MTBLX_SORT_TILE 1024   /* handles per tile-sorted run (csrc/merge_dev.h kSortTile) */
size_t mtblx_sort_workspace_bytes(uint64_t nrec);
int mtblx_sort_plan(const mtblx_records* in, uint64_t* totals, void* workspace, size_t ws_bytes, void* stream);
int mtblx_sort_emit(const mtblx_records* in, int mode, const mtblx_merged* out, const void* workspace,
                    size_t ws_bytes, void* stream);
/* diagnostic (scripts/sort_bench.py): mtblx_sort_plan, plus the HIP-event time in ms of each of its
 * phases: phase_ms[0] the shared-prefix scan, [1] the tile sort (handles built and sorted in LDS),
 * [2 .. passes + 1] the merge passes, [passes + 2] the grouping.  phase_cap >= passes + 3. */
int mtblx_sort_plan_timed(const mtblx_records* in, uint64_t* totals, void* workspace, size_t ws_bytes, void* stream,
                          float* phase_ms, uint32_t phase_cap);

/* ---- Device merge functions: u64 sum / min / max for the Merger and the Sorter ----
 * The reference's merge function is Fn(&[u8], &[Vec<u8>]) -> Result<Vec<u8>, U> (src/merger.rs:145-147,
 * src/sorter.rs:117-118); the three single-value modes above only join or pick values.  A reduce
 * spec is a merge function that adds, evaluated on the device: 1 to MTBLX_REDUCE_MAX_FIELDS fields,
 * each an unsigned 64-bit little-endian integer with one op, MTBLX_REDUCE_SUM (wrapping, mod 2^64),
 * _MIN or _MAX (unsigned).  W = 8 * nfields is the value width.  Per group, after the empty-key
 * quirk has dropped what it drops (the merge only, as in every mode):
 *  - a group of one value comes out unchanged, whatever its length: the reference never calls the
 *    merge function for it (src/merger.rs:200-201, src/sorter.rs:166-167);
 *  - a group of two or more whose values are all exactly W bytes long gives one W-byte value,
 *    field f reduced with op[f] over the group;
 *  - a group of two or more with a value of any other length is the reference's Err from the merge
 *    function (Error::Merge): MTBLX_MERGE_BADVALUE is set in *flags, that group's value bytes are
 *    unspecified but inside its slot, and nothing is written outside the layout.
 * The three ops are associative and commutative and a group of one passes through, so applying the
 * spec per round of MTBLX_MERGE_MAX_SOURCES sources, per Sorter chunk and again when the chunks are
 * merged gives the same bytes as one application over all values of a key (the reference's Sorter
 * applies its merge function that way too), and an erroneous input stays erroneous: a value of
 * another length survives every round unchanged until it meets a partner.
 * The output layout is exactly MTBLX_MERGE_FIRST's: in every valid group the output is as long as
 * the group's first value (its own length for a group of one, W otherwise), so totals[] of the
 * plan, the capacities (totals[3] bounds vals; the bytes used are val_end[groups - 1]) and the
 * workspace are those of an emit in MTBLX_MERGE_FIRST mode, and out->grp_end is unused.  Both calls
 * are asynchronous like the emits they sit beside and take the workspace of a successful
 * mtblx_merge_plan / mtblx_sort_plan over the same records; it is written (a per-tile array for
 * the groups that cross a tile of 1024 merged records), hence not const.  MTBLX_MERGE_OVERFLOW and
 * MTBLX_MERGE_NOT_PLANNED as in the plain emits.  MTBLX_E_INVAL, before any device work: a NULL spec,
 * nfields 0 or above MTBLX_REDUCE_MAX_FIELDS, an op above MTBLX_REDUCE_MAX, and everything the plain
 * emits refuse.
 *
 * Varint-coded values: MTBLX_REDUCE_VARINT OR-ed into every op[f] (all nfields of them or none: a mix
 * is MTBLX_E_INVAL before any device work, as is an op whose other bits exceed MTBLX_REDUCE_MAX).  It
 * is accepted by mtblx_merge_emit_reduce, mtblx_sort_emit_reduce, mtblx_merge_seg_emit_reduce,
 * mtblx_scan_reduce and mtblx_reduce_segments.  This is the convention of the mtbl ecosystem: a value
 * is a sequence of LEB128 varints, merged by decode -> min / max / sum -> re-encode.
 *  - A value is well-formed iff it is exactly F = nfields varints back to back as varint_decode64
 *    (src/varint.rs:78-97) reads them: for each field the decoder is applied to the rest of the value
 *    and must consume at least one byte, and after the F-th field nothing is left.  The decoder's own
 *    behaviour is kept: it looks at no more than 10 bytes per field; a field with no terminator
 *    among them is an error (consumed 0); an empty rest is an error (the reference would panic);
 *    non-canonical encodings (0x80 0x00) are accepted; bits above 2^64 in a tenth byte are dropped,
 *    as the reference's shifts drop them.  Any other value is "bad".
 *  - A group of one value comes out unchanged, whatever its bytes (not re-encoded, bad or not).
 *  - A group of two or more well-formed values gives field f = op[f] over the decoded u64s (SUM mod
 *    2^64, unsigned MIN / MAX), the F results encoded canonically by varint_encode64
 *    (src/varint.rs:64-76) back to back.
 *  - A group of two or more with a bad value sets MTBLX_MERGE_BADVALUE; its slot is as long as its
 *    first value and holds that value, so the layout stays defined.
 *  - In the aggregating calls fields[] stay u64 words, a bad value is counted in nbad and left out.
 * The outputs are canonical and a group of one passes through, so applying the spec per round of
 * sources, per Sorter chunk and again over the chunks gives the bytes of one application: decoding
 * a canonical partial result gives back the number it encodes, the ops are associative and
 * commutative, and the final encoding depends on the final numbers alone.  A bad value survives
 * every round unchanged (alone in its group it passes through; with a partner it is the error).
 * With VARINT the output layout is NOT MTBLX_MERGE_FIRST's: a result is as long as its result needs,
 * longer than the group's first value (0x7f + 0x01 -> 0x80 0x01) or shorter (a sum that wraps).  vals
 * must hold up to totals[3] bytes (all kept value bytes); the bytes used are val_end[groups - 1];
 * keys, key_end and val_end as in MTBLX_MERGE_FIRST mode.  totals[3] is enough because a group's
 * encoded result never exceeds the sum of its inputs' lengths, field by field: len(a + b) <=
 * max(la, lb) + 1 <= la + lb (la, lb >= 1), min / max give <= max(la, lb), and a sum that wraps had
 * a 10-byte operand; non-canonical inputs only widen the margin.  The workspace is the same (its
 * size counts one more per-tile array); val_end is written, scanned in place and read by the call. */
#define MTBLX_REDUCE_SUM 0
#define MTBLX_REDUCE_MIN 1
#define MTBLX_REDUCE_MAX 2
#define MTBLX_REDUCE_MAX_FIELDS 8
#define MTBLX_REDUCE_VARINT 0x10u   /* OR-ed into every op[f]: the fields are LEB128 varints back to back */
#define MTBLX_MERGE_BADVALUE 4u     /* *flags of the two calls below: a group of two or more holds a
                                       value that is not 8 * nfields bytes long (VARINT: not nfields
                                       varints back to back)                                            */
typedef struct mtblx_reduce {
  uint32_t nfields;
  uint8_t op[MTBLX_REDUCE_MAX_FIELDS];
} mtblx_reduce;
int mtblx_merge_emit_reduce(const mtblx_records* src, uint32_t nsrc, const mtblx_reduce* spec,
                            const mtblx_merged* out, void* workspace, size_t ws_bytes, void* stream);
int mtblx_sort_emit_reduce(const mtblx_records* in, const mtblx_reduce* spec, const mtblx_merged* out,
                           void* workspace, size_t ws_bytes, void* stream);

/* ---- Segmented merge: the Merger over a batch of scan results (csrc/merge_seg.hip) ----
 * Every source is nseg sorted runs back to back: source s's records [seg_off[s][q], seg_off[s][q+1])
 * belong to segment q (seg_off: host array [nsrc] of device arrays [nseg + 1], u64, with
 * 0 = off[0] <= ... <= off[nseg] = src[s].n).  That is the shape of nsrc results of mtblx_scan_emit
 * over the same nq = nseg queries (the records plus rec_off): the segments come in any order and may
 * overlap; keys are strictly increasing INSIDE a segment only.  Segment q of the output is what
 * mtblx_merge_plan / _emit give over segment q of every source: one item per distinct key of the
 * segment, the values of a group in source order, and the empty-key quirk applied per segment (an
 * empty-key record is kept iff it is the last record of its segment's merged order; when only
 * empty keys match, one item ("", [v]) with the highest-numbered source's v).  This is the read
 * path of a merged view: MergerIter / MultiIter (src/merger.rs:159-260) as they would run if
 * into_merge_iter built each Entry from iter_from / iter_prefix / iter_range / get of the source.
 *  - Output: one mtblx_merged in (segment, key) order; the groups of segment q are
 *    [seg_end[q-1], seg_end[q]) (seg_end: device [nseg], END group indices; 0 before segment 0).
 *    Modes, capacities, *flags, MTBLX_MERGE_NOT_PLANNED and totals[0..5] are exactly
 *    mtblx_merge_emit's and mtblx_merge_plan's (totals[4] counts the quirk's drops over all
 *    segments); in the three single-value modes the output is an mtblx_records as it stands.
 *    mtblx_merge_seg_emit_reduce is mtblx_merge_emit_reduce over the same plan.
 *  - seg_off is validated on the device before anything is indexed with it: a bad array gives
 *    MTBLX_E_FORMAT with MTBLX_MERGE_BADSEG in totals[5]; an out-of-order pair inside a segment gives
 *    MTBLX_E_FORMAT with MTBLX_MERGE_UNSORTED.  Both are read back before any merge pass (other
 *    totals 0).  The same two keys out of order in DIFFERENT segments are fine.
 *  - Limits: nsrc <= MTBLX_MERGE_MAX_SOURCES (more: merge in rounds with the same mode; a round's
 *    output with {0, seg_end...} as its seg_off is a source of the next), nseg <=
 *    MTBLX_MERGE_MAX_SEGMENTS, fewer than MTBLX_MERGE_MAX_RECORDS records in all sources together.
 *    nseg == 0, nsrc == 0 and empty sources are legal and give zero totals (seg_off may be NULL
 *    when nsrc == 0).
 *  - MTBLX_E_INVAL before any device call: NULL or misaligned workspace, ws_bytes below
 *    mtblx_merge_seg_workspace_bytes, nsrc or nseg above the limits, too many records, NULL src /
 *    seg_off / seg_off[s] (nsrc != 0), NULL totals, NULL seg_end (nseg != 0), and everything
 *    mtblx_merge_emit / mtblx_merge_emit_reduce refuse.
 * How: the Merger's 16-byte handle with the segment in the upper 26 bits of its source word,
 * ordered by (segment, key, source), so each source's handles are one sorted run and the Merger's
 * merge passes run unchanged; the bytes every key shares are found PER SEGMENT on the device (one
 * thread per segment) and the 8-byte prefix of a handle is taken after them.  The workspace
 * (device, 256-byte aligned, no fill needed, one call at a time) is the Merger's plus 12 B per
 * segment; its planned mark is derived from the record, source and segment counts and differs from
 * the Merger's and the Sorter's.  The plan is synchronous, the emits asynchronous. */
#define MTBLX_MERGE_MAX_SEGMENTS (1u << 24)
#define MTBLX_MERGE_BADSEG 4u     /* totals[5]: a seg_off array is not 0 = off[0] <= ... <= off[nseg] = n */
size_t mtblx_merge_seg_workspace_bytes(uint64_t nrec, uint32_t nsrc, uint32_t nseg);
int mtblx_merge_seg_plan(const mtblx_records* src, const uint64_t* const* seg_off, uint32_t nsrc, uint32_t nseg,
                         uint64_t* totals, uint64_t* seg_end, void* workspace, size_t ws_bytes, void* stream);
int mtblx_merge_seg_emit(const mtblx_records* src, const uint64_t* const* seg_off, uint32_t nsrc, uint32_t nseg,
                         int mode, const mtblx_merged* out, const void* workspace, size_t ws_bytes, void* stream);
int mtblx_merge_seg_emit_reduce(const mtblx_records* src, const uint64_t* const* seg_off, uint32_t nsrc,
                                uint32_t nseg, const mtblx_reduce* spec, const mtblx_merged* out, void* workspace,
                                size_t ws_bytes, void* stream);
/* diagnostic (scripts/merger_scan_bench.py): mtblx_merge_seg_plan, plus the HIP-event time in ms of
 * its phases: phase_ms[0] the offsets' check, the per-segment skips and the handles, [1 .. passes]
 * the merge passes (passes = ceil(log2 nsrc)), [passes + 1] the grouping and the segment ends.
 * phase_cap >= passes + 2. */
int mtblx_merge_seg_plan_timed(const mtblx_records* src, const uint64_t* const* seg_off, uint32_t nsrc,
                               uint32_t nseg, uint64_t* totals, uint64_t* seg_end, void* workspace, size_t ws_bytes,
                               void* stream, float* phase_ms, uint32_t phase_cap);

/* ---- Set operations: keep a key by which sources hold it (csrc/merge_dev.h k_group_select) ----
 * A group of the Merger holds at most one record per source, so which sources hold its key is one
 * 64-bit mask m: the OR of 1 << source over the group's records.  A selection keeps the group iff
 *    (m & require) == require,  (m & exclude) == 0,  max(min_count, 1) <= popcount(m) <= max_count.
 *    union                {0, 0, 1, 64}: the Merger as it is
 *    intersection         require = all sources
 *    difference A \ B...  require = 1 (A is source 0), exclude = the rest
 *    in exactly one       max_count = 1 (two sources: the symmetric difference)
 *    in at least k        min_count = k
 *    semi-join            require = 0b11 with MTBLX_MERGE_FIRST: A's records whose key is in B
 * The selection sees the groups the Merger yields: the empty-key quirk runs first, the records it
 * drops contribute to no mask, and the item ("", [v]) that survives when only empty keys exist has
 * the mask of the one source whose v it carries (the highest-numbered) and is selected like any
 * other group.  The reference has no set operations; the definition above is the contract.
 * mtblx_merge_plan_select / mtblx_merge_seg_plan_select are mtblx_merge_plan / mtblx_merge_seg_plan
 * with `sel` applied between the grouping and the sums (sel == NULL: the plain plan).  totals is
 * 8 words: [0..3] and [5] as in the plan, counting the kept groups and their records only, so they
 * still size every emit mode exactly; [4] the records dropped by the empty-key quirk alone; [6] the
 * groups the selection left out; [7] the records in those groups.  seg_end[q] counts kept groups.
 * Workspace sizes and the planned mark are the plain plans': mtblx_merge_emit,
 * mtblx_merge_emit_reduce, mtblx_merge_seg_emit and mtblx_merge_seg_emit_reduce take a
 * select-planned workspace as they are.  MTBLX_E_INVAL before any device work: a bit at or above
 * nsrc in require or exclude, require & exclude != 0, max_count == 0 or > 64,
 * max(min_count, 1) > max_count, and everything the plain plans refuse. */
typedef struct mtblx_select {
  uint64_t require;    /* bit s: source s must hold the key                     */
  uint64_t exclude;    /* bit s: source s must not hold the key                 */
  uint32_t min_count;  /* sources holding the key: at least ... (0 reads as 1)  */
  uint32_t max_count;  /* ... and at most (1..64)                               */
} mtblx_select;
int mtblx_merge_plan_select(const mtblx_records* src, uint32_t nsrc, const mtblx_select* sel, uint64_t* totals,
                            void* workspace, size_t ws_bytes, void* stream);
int mtblx_merge_seg_plan_select(const mtblx_records* src, const uint64_t* const* seg_off, uint32_t nsrc,
                                uint32_t nseg, const mtblx_select* sel, uint64_t* totals, uint64_t* seg_end,
                                void* workspace, size_t ws_bytes, void* stream);

/* ---- Aggregating scans: a reduce spec folded over all the records a query matches ----
 * (csrc/scan.hip, csrc/reduce_seg.hip, DESIGN.md §4 "Aggregating scans").  The spec is the
 * mtblx_reduce of the device merge functions: F = nfields little-endian u64 fields, W = 8 * F (with
 * MTBLX_REDUCE_VARINT: F varints back to back; "not exactly W bytes long" below then reads "not
 * well-formed", see "Varint-coded values" above; fields[] are u64 words either way).  For
 * one query (or one segment), over the records it yields:
 *    nrec       the records yielded (mtblx_scan_result.nrec; the segment's length);
 *    nbad       those among them whose value is not exactly W bytes long: left out of the reduction
 *               and counted.  "A group of one passes through" does not apply: nothing passes through;
 *    fields[f]  op[f] over field f of the nrec - nbad other values; over nothing, the op's identity
 *               (0 for SUM and MAX, 2^64 - 1 for MIN).
 * The results are exact and the ops associative and commutative: no result depends on evaluation
 * order, tile size or which of the two calls served the query.
 *
 * mtblx_scan_reduce is mtblx_scan_plan (same arguments, same res[], same totals, synchronous) whose
 * walk also reduces: where it counts a record it folds the record's value, read where it lies in the
 * block, into fields[q * F + f] and nbad[q] (device, [nq * F] and [nq]).  No key is materialised and
 * there is no second walk and no output buffer.  A query that ends LARGE or FALLBACK has zero fields
 * and zero nbad, as it has zero counts.  The workspace is left planned exactly as mtblx_scan_plan
 * leaves it: a caller who also wants the records follows with mtblx_scan_emit over it.
 * MTBLX_E_INVAL before any device call: everything mtblx_scan_plan refuses, nfields 0 or above
 * MTBLX_REDUCE_MAX_FIELDS, an op above MTBLX_REDUCE_MAX, NULL spec / fields / nbad, fields or nbad not
 * 8-byte aligned.
 *
 * mtblx_reduce_segments (asynchronous, no workspace) reduces segments of any mtblx_records on the
 * device: segment s = records [seg_lo[s], seg_hi[s]) (device u64 [nseg]), with seg_lo[s] <= seg_hi[s]
 * <= seg_lo[s + 1] and seg_hi[nseg - 1] <= n; records in no segment bring nothing.  fields (device
 * [nseg * F]) and nbad (device [nseg]) are 8-byte aligned arrays the call initialises itself.  A
 * segment array that breaks the rule sets MTBLX_REDUCE_BADSEG in *flags (device u32, zeroed by the
 * call) and fields / nbad are left as they were.  A workgroup owns MTBLX_REDUCE_SEG_TILE consecutive
 * records, so one segment of a million records costs what a million segments cost.
 * n < MTBLX_MERGE_MAX_RECORDS.  nseg == 0: MTBLX_OK, nothing written; n == 0: the identities.
 * MTBLX_E_INVAL before any device call: a bad spec, NULL recs / fields / nbad / flags, NULL seg_lo or
 * seg_hi with nseg != 0, n too large, nseg above MTBLX_REDUCE_MAX_SEGMENTS, n != 0 with a NULL val_end
 * (vals may be NULL where every value is empty; keys and key_end are not read), and fields, nbad,
 * seg_lo, seg_hi or val_end not 8-byte aligned (flags: 4-byte). */
#define MTBLX_REDUCE_BADSEG 8u           /* *flags of mtblx_reduce_segments: a bad segment array     */
#define MTBLX_REDUCE_SEG_TILE 1024       /* records per workgroup of mtblx_reduce_segments           */
#define MTBLX_REDUCE_MAX_SEGMENTS 0xFFFFFF00u   /* nseg of mtblx_reduce_segments: 2^32 - 256 at most   */
int mtblx_scan_reduce(const uint8_t* file, uint64_t file_len, uint32_t version, int verify, uint64_t index_off,
                      uint64_t index_len, const uint64_t* tab_start, const uint64_t* tab_doff, const uint64_t* tab_dlen,
                      const int32_t* tab_st, uint32_t ntab, const uint8_t* dec, const int32_t* type,
                      const uint8_t* keys, const uint64_t* key_end, const uint8_t* keys2, const uint64_t* key2_end,
                      const uint64_t* max_records, uint32_t max_blocks, uint32_t nq, mtblx_scan_result* res,
                      uint64_t* totals, void* workspace, size_t ws_bytes, const mtblx_reduce* spec, uint64_t* fields,
                      uint64_t* nbad, void* stream);
int mtblx_reduce_segments(const mtblx_records* recs, const uint64_t* seg_lo, const uint64_t* seg_hi, uint32_t nseg,
                          const mtblx_reduce* spec, uint64_t* fields, uint64_t* nbad, uint32_t* flags, void* stream);
uint32_t mtblx_reduce_seg_tile(void);    /* MTBLX_REDUCE_SEG_TILE of the library that is loaded      */

/* ---- Rollups: records grouped by a prefix of their key, one aggregate per group ----
 * (csrc/rollup.hip, DESIGN.md §4 "Rollups").  The group key gkey(k) of a key k is given by an
 * mtblx_group:
 *    MTBLX_GROUP_LENGTH  k's first `length` bytes, or all of k if it is shorter (length >= 1);
 *    MTBLX_GROUP_DELIM   k up to and including the `count`-th occurrence of the byte `delim`, or all
 *                        of k if it holds fewer (delim <= 255, count >= 1).
 * Both rules are monotone -- a <= b (unsigned bytes, then length) implies gkey(a) <= gkey(b) -- so over
 * sorted keys the records of one group key are adjacent and the group keys come out strictly
 * increasing.  Over one mtblx_records of n records with segments seg_off[0 .. nseg] (device u64,
 * 0 = off[0] <= ... <= off[nseg] = n; nseg == 0: one segment that holds everything, seg_off is not
 * read and seg_grp not written), record r is a HEAD iff r == 0, or r == seg_off[q] for some q, or
 * gkey(r) differs from gkey(r - 1) in length or bytes.  A group is a head and the records up to the
 * next head: groups are runs, as in uniq.  Nothing checks the order of the keys; on unsorted input
 * equal group keys that are not adjacent stay apart.
 *
 * mtblx_rollup_plan (asynchronous) finds the heads and writes totals (DEVICE, 2 words, 8-byte aligned):
 *    [0] groups   [1] the bytes of their keys
 * which size the emit's outputs exactly.  mtblx_rollup_emit (asynchronous, same records, rule and
 * segments) reads the planned workspace and writes, per group g in record order:
 *    keys / key_end   gkey of the group (u64 END offsets: with a value per group an mtblx_records);
 *    grp_rec[g]       its first record, and grp_rec[groups] = n: group g is the records
 *                     [grp_rec[g], grp_rec[g + 1]), which is what mtblx_reduce_segments takes as
 *                     seg_lo / seg_hi, and nrec[g] the difference;
 *    seg_grp[q]       q = 0 .. nseg: the groups that begin before segment q; segment q's groups are
 *                     [seg_grp[q], seg_grp[q + 1]), none for an empty segment.
 * Every capacity is in BYTES.  *flags (device u32, cleared by the emit):
 *    MTBLX_ROLLUP_OVERFLOW     a capacity is below what the totals ask for (keys: [1]; key_end: 8 * [0];
 *                              grp_rec: 8 * ([0] + 1); seg_grp: 8 * (nseg + 1));
 *    MTBLX_ROLLUP_NOT_PLANNED  the workspace is not that of a plan over this record count, segment
 *                              count and rule;
 *    MTBLX_ROLLUP_BADSEG       the plan met a seg_off that breaks its rule (its totals are then zero).
 * With any of them set NOTHING else is written: the outputs are as they were.
 * The workspace (device, 256-byte aligned, mtblx_rollup_workspace_bytes; no fill needed; one call at a
 * time) holds a header, 9 B per record and 16 B per tile of mtblx_rollup_tile() records.
 * n < MTBLX_MERGE_MAX_RECORDS; n == 0 is legal (no groups; grp_rec[0] = 0, seg_grp all 0).
 * MTBLX_E_INVAL before any device call: NULL recs or group, an unknown kind, length == 0 (LENGTH),
 * count == 0 or delim > 255 (DELIM), NULL or misaligned (256) workspace, ws_bytes too small, n too
 * large, nseg above MTBLX_REDUCE_MAX_SEGMENTS, nseg != 0 with a NULL seg_off, n != 0 with a NULL
 * key_end (keys may be NULL where every key is empty; vals and val_end are not read), key_end or
 * seg_off not 8-byte aligned; the plan: NULL or misaligned totals; the emit: NULL out or flags
 * (4-byte aligned), a NULL key_end or grp_rec, a NULL keys with a non-zero keys_cap, a NULL seg_grp
 * with nseg != 0, and key_end, grp_rec or seg_grp not 8-byte aligned.
 *
 * The aggregate of a group is mtblx_reduce_segments over (grp_rec, grp_rec + 1): fields and nbad as
 * the aggregating scans define them -- bad values left out and counted, nothing passes through, not
 * even in a group of one.  mtblx_reduce_encode (asynchronous) then turns n rows of F = nfields u64
 * words (device, 8-byte aligned: the fields of mtblx_reduce_segments) into n values and their u64 END
 * offsets: row i's F words as little-endian bytes (val_end[i] = 8 * F * (i + 1)), or with
 * MTBLX_REDUCE_VARINT as F canonical varints back to back (varint_encode64, src/varint.rs:64-76).
 * cap (bytes of vals) must be at least 8 * F * n, with VARINT 10 * F * n: what n rows can take; the
 * bytes used are val_end[n - 1].  The workspace (device, 8-byte aligned,
 * mtblx_reduce_encode_workspace_bytes) holds one word per tile; the u64le form does not touch it.
 * n == 0: MTBLX_OK, nothing written.  MTBLX_E_INVAL before any device call: a bad spec, n >=
 * MTBLX_MERGE_MAX_RECORDS, and with n != 0 a NULL or misaligned fields / val_end / workspace, a NULL
 * vals, a cap or ws_bytes too small. */
#define MTBLX_GROUP_LENGTH 0
#define MTBLX_GROUP_DELIM 1
#define MTBLX_ROLLUP_OVERFLOW 1u
#define MTBLX_ROLLUP_NOT_PLANNED 2u
#define MTBLX_ROLLUP_BADSEG 8u
typedef struct mtblx_group {
  uint32_t kind;     /* MTBLX_GROUP_LENGTH / MTBLX_GROUP_DELIM                                          */
  uint64_t length;   /* LENGTH: the bytes of a group key, >= 1                                          */
  uint32_t delim;    /* DELIM: the delimiter byte, <= 255                                               */
  uint32_t count;    /* DELIM: the group key ends with the count-th delimiter, >= 1                     */
} mtblx_group;
typedef struct mtblx_rolled {
  uint8_t* keys;       /* device: key of group g = keys[key_end[g-1] .. key_end[g])                       */
  uint64_t keys_cap;
  uint64_t* key_end;   /* device [groups], u64 END offsets                                               */
  uint64_t key_end_cap;
  uint64_t* grp_rec;   /* device [groups + 1]: the first record of every group, then n                   */
  uint64_t grp_rec_cap;
  uint64_t* seg_grp;   /* device [nseg + 1]: the groups before every segment (nseg == 0: not written)    */
  uint64_t seg_grp_cap;
  uint32_t* flags;     /* device word, cleared by the call: MTBLX_ROLLUP_*                                */
} mtblx_rolled;
size_t mtblx_rollup_workspace_bytes(uint64_t nrec, uint32_t nseg);
int mtblx_rollup_plan(const mtblx_records* recs, const mtblx_group* group, const uint64_t* seg_off, uint32_t nseg,
                      uint64_t* totals, void* workspace, size_t ws_bytes, void* stream);
int mtblx_rollup_emit(const mtblx_records* recs, const mtblx_group* group, const uint64_t* seg_off, uint32_t nseg,
                      const mtblx_rolled* out, const void* workspace, size_t ws_bytes, void* stream);
uint32_t mtblx_rollup_tile(void);        /* records per workgroup of the rollup's scans               */
size_t mtblx_reduce_encode_workspace_bytes(uint64_t n);
int mtblx_reduce_encode(const uint64_t* fields, uint64_t n, const mtblx_reduce* spec, uint8_t* vals,
                        uint64_t* val_end, uint64_t cap, void* workspace, size_t ws_bytes, void* stream);

/* ---- Value predicates: records kept or dropped by the fields of their value ----
 * (csrc/where.hip, DESIGN.md §4 "Value predicates").  An mtblx_where is a value layout -- exactly that
 * of an mtblx_reduce: F = nfields little-endian u64 fields (the value is exactly 8 * F bytes), or with
 * MTBLX_WHERE_VARINT F varints back to back, read with every quirk listed under "Varint-coded values"
 * above -- plus at most one inclusive, unsigned range per field.  For one value:
 *    a value that is not well-formed under the layout is BAD: its record is dropped and counted,
 *      never kept and never an error;
 *    otherwise field f PASSES iff (lo[f] <= x_f && x_f <= hi[f]) != (bit f of outside);
 *    flags without MTBLX_WHERE_ANY: kept iff every field of `mask` passes (mask == 0: always kept);
 *    with MTBLX_WHERE_ANY:          kept iff some field of `mask` passes (mask == 0: never kept).
 * lo > hi is legal and is an empty range (with its outside bit: every value).  The reference has no
 * predicates; the definition above is the contract.  MTBLX_E_INVAL before any device work: nfields 0
 * or above MTBLX_REDUCE_MAX_FIELDS, unknown flag bits, a mask or outside bit at or above nfields,
 * outside & ~mask.
 *
 * mtblx_where_plan (SYNCHRONOUS) evaluates the predicate once per record of `recs`, leaves the
 * keep / bad bits in the workspace and writes
 *    totals (HOST, 6 words)  [0] kept records  [1] their key bytes  [2] their value bytes
 *                            [3] bad values    [4] well-formed values rejected    [5] flags
 *    seg_end[q]  (device [nseg]) the END index of segment q in the kept order: segment q's kept
 *                records are [seg_end[q - 1], seg_end[q]) (0 before segment 0);
 *    seg_bad[q]  (device [nseg], may be NULL) the bad values in segment q.
 * seg_off (device u64 [nseg + 1], 0 = off[0] <= ... <= off[nseg] = n) is checked on the device before
 * it indexes anything: a bad array gives MTBLX_E_FORMAT with MTBLX_WHERE_BADSEG in totals[5] (the
 * other totals 0; seg_end / seg_bad as they were).  nseg == 0: the whole of recs, no segments;
 * seg_off, seg_end and seg_bad are not read or written.
 * mtblx_where_emit (asynchronous, same records) reads the planned workspace and writes the kept
 * records in their order: keys / key_end / vals / val_end (u64 END offsets: an mtblx_records as it
 * stands, which feeds the device Writer) and, where src_idx is not NULL, src_idx[e] = the index in
 * recs of kept record e, for gathering side arrays.  keys_cap / vals_cap are in BYTES, rec_cap in
 * RECORDS (of key_end, val_end and src_idx alike).  *flags (device u32, cleared by the emit):
 *    MTBLX_WHERE_OVERFLOW     a capacity is below what the totals ask for (keys: [1]; vals: [2];
 *                             rec_cap: [0]);
 *    MTBLX_WHERE_NOT_PLANNED  the workspace is not that of an mtblx_where_plan over this record count
 *                             (the mark differs from every other workspace's);
 *    MTBLX_WHERE_BADSEG       the plan met a bad seg_off.
 * With any of them set NOTHING else is written: the outputs are as they were.
 * The workspace (device, 256-byte aligned, mtblx_where_workspace_bytes; no fill needed; one call at a
 * time) holds a header, 1 B per record and 32 B per tile of mtblx_where_tile() records: a workgroup
 * owns a tile of consecutive records, so one segment of a million records costs what a million
 * segments cost.  n < MTBLX_MERGE_MAX_RECORDS; n == 0 is legal.  Values are read at any alignment.
 * MTBLX_E_INVAL before any device call: a bad mtblx_where, NULL recs, NULL or misaligned (256)
 * workspace, ws_bytes too small, n too large, nseg above MTBLX_REDUCE_MAX_SEGMENTS, nseg != 0 with a
 * NULL seg_off or seg_end, n != 0 with a NULL key_end or val_end (keys / vals may be NULL where every
 * key / value is empty), key_end, val_end, seg_off, seg_end or seg_bad not 8-byte aligned; the plan:
 * NULL totals; the emit: NULL out or flags (4-byte aligned), a NULL keys / vals with a non-zero
 * capacity, a NULL key_end or val_end with a non-zero rec_cap, and key_end, val_end or src_idx not
 * 8-byte aligned. */
#define MTBLX_WHERE_ANY 1u        /* flags: at least one constrained field passes (default: all of them) */
#define MTBLX_WHERE_VARINT 0x10u  /* flags: the fields are varints; the same bit as MTBLX_REDUCE_VARINT  */
#define MTBLX_WHERE_OVERFLOW 1u
#define MTBLX_WHERE_NOT_PLANNED 2u
#define MTBLX_WHERE_BADSEG 8u
typedef struct mtblx_where {
  uint32_t nfields;   /* 1..MTBLX_REDUCE_MAX_FIELDS */
  uint32_t flags;     /* MTBLX_WHERE_ANY | MTBLX_WHERE_VARINT */
  uint8_t mask;       /* bit f: field f is constrained */
  uint8_t outside;    /* bit f: field f must lie OUTSIDE [lo[f], hi[f]] (a subset of mask) */
  uint64_t lo[8], hi[8];   /* inclusive, unsigned */
} mtblx_where;
typedef struct mtblx_filtered {
  uint8_t* keys;       /* device: key of kept record e = keys[key_end[e-1] .. key_end[e])               */
  uint64_t keys_cap;   /* bytes                                                                         */
  uint8_t* vals;
  uint64_t vals_cap;   /* bytes                                                                         */
  uint64_t* key_end;   /* device [kept], u64 END offsets                                                */
  uint64_t* val_end;
  uint64_t* src_idx;   /* device [kept], may be NULL: the index in recs of every kept record            */
  uint64_t rec_cap;    /* records: the capacity of key_end, val_end and src_idx                         */
  uint32_t* flags;     /* device word, cleared by the call: MTBLX_WHERE_*                               */
} mtblx_filtered;
size_t mtblx_where_workspace_bytes(uint64_t nrec, uint32_t nseg);
int mtblx_where_plan(const mtblx_records* recs, const mtblx_where* w, const uint64_t* seg_off, uint32_t nseg,
                     uint64_t* totals, uint64_t* seg_end, uint64_t* seg_bad, void* workspace, size_t ws_bytes,
                     void* stream);
int mtblx_where_emit(const mtblx_records* recs, const mtblx_filtered* out, const void* workspace, size_t ws_bytes,
                     void* stream);
uint32_t mtblx_where_tile(void);         /* records per workgroup of the filter's kernels             */
/* The fused aggregating walk: mtblx_scan_reduce (same arguments, same res[], same totals, same
 * workspace, synchronous) with a predicate between the iterator and the fold.  Where the walk folds a
 * record's value it first evaluates `where` on the same decoded fields -- lane f holds field f's
 * bounds; one compare per lane and one ballot decide.  Per query: res[q].nrec, key_bytes, val_bytes
 * and the status are exactly mtblx_scan_plan's (the predicate sits AFTER the iterator and after
 * max_records); nbad[q] the bad values; nmatch[q] (device [nq], 8-byte aligned) the kept values;
 * fields the ops over the kept values only, over nothing the identities.  Queries that are not
 * MTBLX_SCAN_OK give zeros.  MTBLX_E_INVAL before any device call: everything mtblx_scan_reduce
 * refuses, a bad mtblx_where, a layout of `where` (nfields and the varint bit) that is not the
 * spec's, a NULL or misaligned nmatch. */
int mtblx_scan_reduce_where(const uint8_t* file, uint64_t file_len, uint32_t version, int verify, uint64_t index_off,
                            uint64_t index_len, const uint64_t* tab_start, const uint64_t* tab_doff,
                            const uint64_t* tab_dlen, const int32_t* tab_st, uint32_t ntab, const uint8_t* dec,
                            const int32_t* type, const uint8_t* keys, const uint64_t* key_end, const uint8_t* keys2,
                            const uint64_t* key2_end, const uint64_t* max_records, uint32_t max_blocks, uint32_t nq,
                            mtblx_scan_result* res, uint64_t* totals, void* workspace, size_t ws_bytes,
                            const mtblx_reduce* spec, uint64_t* fields, uint64_t* nbad, const mtblx_where* where,
                            uint64_t* nmatch, void* stream);

/* ---- snappy raw decompression on the device (f4) ----
 * Reader::block's decompression step for CompressionType::Snappy (src/reader.rs:166-170 ->
 * src/compression.rs:57-68, :116-119, snap::raw::Decoder::decompress_vec), for a batch of
 * blocks at once.  Block b's STORED bytes are src[src_off[b] .. + src_len[b]) (device).
 * Status codes are mtblx_host.h's MTBLX_SNAPPY_*: OK, CORRUPT (snap errors -> Err(Error::Io)),
 * TOO_SMALL (the preamble length exceeds dst_len[b]).
 *
 * mtblx_snappy_dir: the output layout from the preambles: dst_len[b] = the stored
 * uncompressed length (0 if the preamble is corrupt, status[b] = CORRUPT), dst_off[b] = the
 * exclusive prefix of dst_len rounded up to 16 bytes; totals (device [3]) = bytes of the
 * layout, max dst_len, corrupt preambles.  workspace: mtblx_snappy_workspace_bytes(nblk)
 * bytes of device memory (no fill needed).
 *
 * mtblx_snappy_decompress_dev: decompresses block b into dst[dst_off[b] .. + its length)
 * (dst_len[b] = capacity); status[b]; dec_len[b] (device [nblk], may be NULL) = the
 * decompressed length, or 0 if the block failed -- i.e. {dst, dst_off, dec_len} is directly
 * the mtblx_block_batch directory of the decompressed blocks.  max_dst_len: host hint (max
 * of dst_len; 0 = unknown) selecting the kernel variant; the environment variable
 * MTBLX_SNAPPY_KERNEL (read per call: auto | quads | lanes | two) forces one for A/B runs and
 * tests, with identical outputs and statuses.  Both calls are asynchronous on `stream`. */
size_t mtblx_snappy_workspace_bytes(uint32_t nblk);
int mtblx_snappy_dir(const uint8_t* src, const uint64_t* src_off, const uint32_t* src_len, uint32_t nblk,
                     uint64_t* dst_off, uint32_t* dst_len, int32_t* status, uint64_t* totals, void* workspace,
                     size_t workspace_bytes, void* stream);
int mtblx_snappy_decompress_dev(const uint8_t* src, const uint64_t* src_off, const uint32_t* src_len, uint32_t nblk,
                                uint8_t* dst, const uint64_t* dst_off, const uint32_t* dst_len, uint32_t max_dst_len,
                                int32_t* status, uint32_t* dec_len, void* stream);

/* ---- device staging of Snappy blocks: a block directory -> a staged batch and a lookup table ----
 * Reader::block's decompress step (src/reader.rs:166-170) for the entries of a directory as
 * mtblx_block_dir writes it (blk_off / blk_len / dir_st, device [ndir]), with the stored bytes left
 * where they are in `file` (device).  bad (device [ndir], may be NULL): the checksum assert of
 * mtblx_crc32c_blocks (framed).  sel (device [nsel], may be NULL = every entry, n = ndir): ascending
 * directory ordinals; n = nsel entries are staged.  Two calls, as the Merger and the scans:
 *
 * mtblx_stage_plan (synchronous): an entry that is not MTBLX_DIR_OK, is `bad`, names an ordinal
 * >= ndir or an extent outside the file is SKIPPED -- the reference panics before it decompresses
 * it -- and gets length 0 and no error.  The other entries' preambles give 16-byte aligned
 * destinations (mtblx_snappy_dir).  totals (host [3]) = bytes of the layout, the largest
 * decompressed length, corrupt preambles among the entries not skipped.  A stored length of 0 is a
 * corrupt preamble (the host stage's Err(Io), mtblx_decompress_blocks).
 *
 * mtblx_stage_emit (asynchronous, no allocation, no synchronisation): decompresses entry j into
 * dst[base + its offset ..) with mtblx_snappy_decompress_dev's kernels and variant choice
 * (max_dec_len = totals[1]); base % 16 == 0 and base + total <= dst_cap (total = totals[0]), else
 * MTBLX_E_INVAL.  Writes
 *   dst_off / dec_len (device [n], either may be NULL): with dst, an mtblx_block_batch directory of
 *     the decompressed blocks; dec_len 0 for a failed or skipped entry;
 *   tab_start / tab_doff / tab_dlen / tab_st (device, all NULL or none): the rows
 *     mtblx_get_decompressed takes -- the stored content start, the offset in dst, the length, and
 *     nonzero where the crate's decompress step returns Err(Io) -- at row j (by_ordinal == 0,
 *     [n] rows: with sel == NULL on an ascending directory the table as it stands), or at row
 *     sel[j] (by_ordinal != 0, [ndir] rows: per-ordinal rows for mtblx_table_gather).
 * The workspace (device, 256-byte aligned, mtblx_stage_workspace_bytes(n); no fill needed) is the
 * caller's and carries the plan to the emit: same file, directory and selection in both. */
size_t mtblx_stage_workspace_bytes(uint32_t n);
int mtblx_stage_plan(const uint8_t* file, uint64_t file_len, const uint64_t* blk_off, const uint32_t* blk_len,
                     const int32_t* dir_st, const uint8_t* bad, uint32_t ndir, const uint32_t* sel, uint32_t nsel,
                     uint64_t* totals, void* workspace, size_t ws_bytes, void* stream);
int mtblx_stage_emit(const uint8_t* file, uint64_t file_len, const uint64_t* blk_off, uint32_t ndir,
                     const uint32_t* sel, uint32_t nsel, uint8_t* dst, uint64_t dst_cap, uint64_t base, uint64_t total,
                     uint32_t max_dec_len, uint64_t* dst_off, uint32_t* dec_len, uint64_t* tab_start,
                     uint64_t* tab_doff, uint64_t* tab_dlen, int32_t* tab_st, int by_ordinal, const void* workspace,
                     size_t ws_bytes, void* stream);

/* ---- which blocks a batch of queries needs: touch, compaction, the on-demand table ----
 * mtblx_scan_touch: per query the fresh index seek of Reader::get / ReaderIntoIter::new_from
 * (src/reader.rs:256-275) on the index block file[index_off .. + index_len), for the start key
 * keys[key_end[q-1] .. key_end[q]) and the bound keys2[key2_end[q-1] .. key2_end[q]) (empty, or
 * key2_end == NULL: open ended).  entry_off (device [nent], ascending): the entry offsets of the
 * index scan chain (mtblx_entry_offsets), entry i <-> directory ordinal i.  lo = the ordinal where
 * the start key lands, hi = the ordinal where the bound lands plus one (the iterator opens the next
 * block when a block runs out before the stop rule fires); the bits [lo, min(hi, lo + cap - 1)] are
 * ORed into want (device u32 [nwords] over the directory, nwords * 32 >= nent; not cleared).  cap:
 * device [nq], or NULL = cap_all for every query.  Host glue: get k -> (k, k); from k -> (k, none);
 * range a b -> (a, b); prefix p -> (p, p with its last non-0xff byte incremented and the tail
 * dropped; none if p is empty or all 0xff).  The result is a HINT: correctness rests on the lookup
 * kernels, which report a block the table lacks (MTBLX_GET_MISSING / MTBLX_SCAN_FALLBACK).  On a
 * corrupt index every access stays inside the index block, entry_off and want; a seek that panics,
 * loops or lands off the chain marks nothing.
 *
 * mtblx_bitmap_compact: the set bits of bits & ~exclude (exclude may be NULL) below nbits, ascending,
 * to list (device [list_cap]; ordinals past list_cap are counted, not written); *count (device).
 *
 * mtblx_table_gather: row j of the compact table = (blk_off[o], row_doff[o], row_dlen[o], row_st[o])
 * for o = list[j] (n rows from per-ordinal arrays of nrow entries).  On a directory whose content
 * starts ascend with the ordinal (mtblx_dir_ascends: *violations (device) = entries that are not
 * MTBLX_DIR_OK or whose start is not below the next one's) an ascending list gives the table sorted
 * by stored start that the lookup kernels binary-search.  All four are asynchronous on `stream`. */
int mtblx_scan_touch(const uint8_t* file, uint64_t file_len, uint64_t index_off, uint64_t index_len,
                     const uint64_t* entry_off, uint32_t nent, const uint8_t* keys, const uint64_t* key_end,
                     const uint8_t* keys2, const uint64_t* key2_end, const uint32_t* cap, uint32_t cap_all, uint32_t nq,
                     uint32_t* want, uint32_t nwords, void* stream);
int mtblx_bitmap_compact(const uint32_t* bits, const uint32_t* exclude, uint32_t nbits, uint32_t* list,
                         uint32_t list_cap, uint32_t* count, void* stream);
int mtblx_table_gather(const uint32_t* list, uint32_t n, uint32_t nrow, const uint64_t* blk_off,
                       const uint64_t* row_doff, const uint64_t* row_dlen, const int32_t* row_st, uint64_t* tab_start,
                       uint64_t* tab_doff, uint64_t* tab_dlen, int32_t* tab_st, void* stream);
int mtblx_dir_ascends(const uint64_t* blk_off, const int32_t* dir_st, uint32_t ndir, uint32_t* violations,
                      void* stream);

/* ---- end-to-end decode from host memory (the PCIe-inclusive path of the north star) ----
 * An mtbl file in host memory in (mmap'd or read), the caller's host byte slices out:
 * for every data block, Reader::block's decompression (src/reader.rs:166-170, host: the
 * north star keeps src/compression.rs on the host) + Block::init + the BlockIter scan
 * (device).  Consecutive blocks are cut into chunks that flow through three stages with
 * three chunks in flight: host staging (nothing for a pinned uncompressed file; a parallel
 * copy into pinned memory for a pageable one; parallel snappy decompression), H2D +
 * mtblx_decode_blocks on the device, D2H of the chunk's outputs into `out`.
 *   file/blk_off/blk_len: host; block b's STORED content is file[blk_off[b] .. + blk_len[b])
 *   (the directory mtblx_writer_block_dir / mtblx_block_dir produce).  compression: the
 *   footer's compression_algorithm: 0 None, 1 Snappy (others: MTBLX_E_INVAL).
 *   out: mtblx_decoded whose pointers are HOST memory (pin it -- mtblx_host_alloc or
 *   mtblx_host_register -- for full PCIe rate), same layout and status codes as
 *   mtblx_decode_blocks plus MTBLX_ST_DECOMPRESS.  If a capacity is too small the outputs of
 *   the chunks that do not fit are skipped (their blocks: MTBLX_ST_OVERFLOW, totals[3] bit 0)
 *   and totals[0..2] still report the exact sizes, so a caller can size and call again.
 * Synchronous: returns when `out` is complete.  One call at a time per pipe. */
typedef struct mtblx_pipe mtblx_pipe;
typedef struct mtblx_pipe_stats {
  double seconds;          /* wall time of the call                                */
  double stage_seconds;    /* host staging (copies / decompression) on the calling path */
  double decode_ms;        /* device time of the decode launches (HIP events)     */
  uint64_t block_bytes;    /* uncompressed block content bytes decoded            */
  uint64_t h2d_bytes, d2h_bytes;
  uint32_t chunks;
  uint32_t decompress_errors;
} mtblx_pipe_stats;
/* chunk_bytes: uncompressed bytes per chunk (0 = 64 MiB); max_blocks: blocks per chunk
 * (0 = 65536); threads: host staging threads (0 = 16).  Binds to the current HIP device. */
mtblx_pipe* mtblx_pipe_new(uint64_t chunk_bytes, uint32_t max_blocks, uint32_t threads);
void mtblx_pipe_free(mtblx_pipe* p);
int mtblx_pipe_decode(mtblx_pipe* p, const uint8_t* file, uint64_t file_len, uint32_t compression,
                      const uint64_t* blk_off, const uint32_t* blk_len, uint32_t nblk, const mtblx_decoded* out,
                      mtblx_pipe_stats* stats);
/* mtblx_pipe_decode for CompressionType::None with the values left where they are: same
 * outputs into host `out` except out->vals (ignored, as out->vals_cap), plus val_pos (host
 * [out->rec_cap], pin it) as mtblx_decode_blocks_valpos defines it.  Positions are
 * block-relative, so they do not depend on how the file is cut into chunks; value r of block b
 * is file[blk_off[b] + val_pos[r] ..].  No value byte crosses PCIe back: per record the D2H is
 * key_end, val_end and val_pos (12 B) plus the key bytes.  One pipe may serve this and
 * mtblx_pipe_decode alternately.  val_pos == NULL with rec_cap != 0 is MTBLX_E_INVAL. */
int mtblx_pipe_decode_valpos(mtblx_pipe* p, const uint8_t* file, uint64_t file_len, const uint64_t* blk_off,
                             const uint32_t* blk_len, uint32_t nblk, const mtblx_decoded* out,
                             uint32_t* val_pos, mtblx_pipe_stats* stats);
/* pipe options.  MTBLX_PIPE_DEVICE_SNAPPY (value 1 = on, 0 = off, 2 = auto, the default):
 * snappy files cross PCIe as stored and are decompressed on the device
 * (mtblx_snappy_decompress_dev) right before the decode; off = host decompression in the
 * staging stage; auto = the device (measured faster end to end on poorly compressed and on
 * compressible streams alike).  Same outputs either way. */
#define MTBLX_PIPE_DEVICE_SNAPPY 1
int mtblx_pipe_set(mtblx_pipe* p, int option, int64_t value);
/* pinned host memory for the pipe's inputs / outputs */
int mtblx_host_alloc(void** p, uint64_t bytes);
int mtblx_host_free(void* p);
int mtblx_host_register(void* p, uint64_t bytes);   /* pin an existing range, e.g. an mmap'd file */
int mtblx_host_unregister(void* p);

/* ---- diagnostic: device copy at the HBM ceiling ----
 * dst[0 .. bytes) = src[0 .. bytes) (16-byte aligned, bytes % 16 == 0) by a plain gfx950
 * streaming kernel: 16 B per lane per access, 2^(variant & 3) accesses in flight per lane,
 * 8 workgroups per CU.  bench.py takes the best of a sweep as this box's copy ceiling, the
 * reference its roofline fraction is read against besides the 8 TB/s spec.  Asynchronous. */
#define MTBLX_COPY_NT_STORES 4
#define MTBLX_COPY_NT_LOADS 8
int mtblx_stream_copy(void* dst, const void* src, uint64_t bytes, int variant, void* stream);

/* n byte ranges src + src_off[i] -> dst + dst_off[i] (len[i] bytes each, device arrays) by the
 * whole grid: chunk_base[i] = the exclusive prefix of ceil(len / 16) over the ranges, nchunks its
 * total.  Asynchronous on `stream`.  Used with mtblx_block_seek_batch_ex for the values of blocks
 * >= 4 GiB (one wave would copy their GiBs at a few GB/s). */
int mtblx_copy_ranges(const uint8_t* src, const uint64_t* src_off, uint8_t* dst, const uint64_t* dst_off,
                      const uint64_t* len, const uint64_t* chunk_base, uint32_t n, uint64_t nchunks, void* stream);

/* ---- Diagnostics: a process-wide compute-unit limit for launch sizing ----
 * Most launches cap their grid at a multiple of the device's compute units and let every
 * workgroup, wave or lane loop over the rest of the work.  The second trip of such a loop needs,
 * on a whole MI355X, inputs far above what a test can afford; this seam lowers the cap instead.
 *
 * mtblx_debug_cu_limit(n) stores n (one relaxed atomic; 0 = no limit, the default) and returns
 * the previous value.  While a limit is set every launch is sized as if the device had
 * min(real compute units, max(1, n)) of them, from the next launch of every kernel on (grids that
 * are cached per device are recomputed, and nothing computed under a limit is cached).  The limit
 * can only LOWER the count, never raise it: the decode kernels' look-back between workgroups needs
 * every workgroup of a launch resident, and a grid above the device's real capacity could spin
 * forever.  MTBLX_PIPE_CUS still applies; the limit applies on top of it.  No workspace size and no
 * result depends on the limit: a plan made under one limit and its emit under another are valid.
 * Not thread-safe against launches in flight on other host threads (they see either value).
 *
 * mtblx_debug_grid_items(family, arg) = the work items one launch of that family starts, at the
 * current limit and the current routing variables, before a worker of its loop takes a second
 * trip: n items with n > 2 * this make every worker wrap at least twice.  Computed by the same
 * functions the launches use.  0 for an unknown family.
 *
 * mtblx_debug_decode_tiles = the tiles the block decode cuts a batch of nblk blocks, the longest
 * max_blk_len bytes, into (verify: mtblx_decode_blocks_verify's plan), and in *kind (may be NULL)
 * the kernel family that takes it: 0 the small pipeline, 1 the large one (MTBLX_GRID_DECODE_PIPE
 * both), 2 k_decode_tiles (MTBLX_GRID_DECODE_TILES). */
#define MTBLX_GRID_SCAN_PLAN 0     /* queries: k_scan_plan<...> of scan_plan / scan_reduce / scan_reduce_where */
#define MTBLX_GRID_SCAN_EMIT 1     /* queries: k_scan_emit                                                      */
#define MTBLX_GRID_GET 2           /* keys: k_get_lanes, or k_get with MTBLX_GET_KERNEL=wave                    */
#define MTBLX_GRID_MERGE_BUILD 3   /* records: k_merge_build                                                    */
#define MTBLX_GRID_SEG_BUILD 4     /* records: k_seg_build                                                      */
#define MTBLX_GRID_SORT_SKIP 5     /* records: k_sort_skip                                                      */
#define MTBLX_GRID_CRC 6           /* blocks: k_crc32c_mfma (64 per wave and trip), or k_crc32c_blocks with
                                      MTBLX_CRC_KERNEL=lanes                                                    */
#define MTBLX_GRID_SNAPPY_SMALL 7  /* blocks: the widest of k_snappy_quads / _exec / _waves / _deferred         */
#define MTBLX_GRID_SNAPPY_LARGE 8  /* blocks: k_snappy_blocks<Large> (blocks above 4608 bytes)                  */
#define MTBLX_GRID_SNAPPY_COMP 9   /* blocks: k_snappy_compress, k_frame_write                                  */
#define MTBLX_GRID_COPY_RANGES 10  /* 16-byte chunks: k_copy_ranges                                             */
#define MTBLX_GRID_STREAM_COPY 11  /* 16-byte chunks: k_stream_copy; arg = mtblx_stream_copy's variant          */
#define MTBLX_GRID_DECODE_PIPE 12  /* tiles: k_decode_pipe<...>                                                 */
#define MTBLX_GRID_DECODE_TILES 13 /* tiles: k_decode_tiles<CfgLarge>, or <CfgLargeP> with arg = 1 (positions)  */
int mtblx_debug_cu_limit(int n);
uint64_t mtblx_debug_grid_items(int family, int arg);
uint32_t mtblx_debug_decode_tiles(uint32_t nblk, uint32_t max_blk_len, int verify, int* kind);

#ifdef __cplusplus
}
#endif
#endif /* MTBLX_H */

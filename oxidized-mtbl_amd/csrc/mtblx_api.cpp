// mtblx_api.cpp — C ABI entry points of libmtblx.so (declared in include/mtblx.h).
//
// Thin, allocation-free glue: argument checks, then the kernel pipeline in decode.hip
// on the caller's stream.  See include/mtblx.h for the contract and the reference
// interfaces each entry point replaces.
#include <hip/hip_runtime.h>
#include <string.h>

#include "mtblx.h"
#include "devinfo.h"

extern "C" size_t mtblx_impl_ws_bytes(uint32_t nblk);
extern "C" int mtblx_impl_run(const mtblx_block_batch* in, const mtblx_decoded* out, void* ws, size_t ws_bytes,
                              int write, hipStream_t s, int verify, uint32_t* crc, uint8_t* crc_bad, int framed);

extern "C" int mtblx_crc32c_blocks(const mtblx_block_batch* in, uint32_t* crc, uint8_t* bad, int framed,
                                   void* stream);
extern "C" int mtblx_impl_run_valpos(const mtblx_block_batch* in, const mtblx_decoded* out, uint32_t* val_pos, void* ws,
                                     size_t ws_bytes, hipStream_t s);

extern "C" int mtblx_abi_version(void) { return MTBLX_ABI_VERSION; }

// ---- diagnostics: the CU limit of devinfo.h and what each capped launch starts under it ----
extern "C" uint64_t mtblx_grid_items_scan_plan(void);
extern "C" uint64_t mtblx_grid_items_scan_emit(void);
extern "C" uint64_t mtblx_grid_items_get(void);
extern "C" uint64_t mtblx_grid_items_merge_build(void);
extern "C" uint64_t mtblx_grid_items_seg_build(void);
extern "C" uint64_t mtblx_grid_items_sort_skip(void);
extern "C" uint64_t mtblx_grid_items_crc(void);
extern "C" uint64_t mtblx_grid_items_snappy_small(void);
extern "C" uint64_t mtblx_grid_items_snappy_large(void);
extern "C" uint64_t mtblx_grid_items_snappy_comp(void);
extern "C" uint64_t mtblx_grid_items_copy_ranges(void);
extern "C" uint64_t mtblx_grid_items_stream_copy(int variant);
extern "C" uint64_t mtblx_grid_items_decode_pipe(void);
extern "C" uint64_t mtblx_grid_items_decode_tiles(int positions);
extern "C" uint32_t mtblx_impl_decode_tiles(uint32_t nblk, uint32_t max_blk_len, int verify, int* kind);

extern "C" int mtblx_debug_cu_limit(int n) {
  return mtblx_dev::cu_limit_word().exchange(n, std::memory_order_relaxed);
}

extern "C" uint64_t mtblx_debug_grid_items(int family, int arg) {
  switch (family) {
    case MTBLX_GRID_SCAN_PLAN: return mtblx_grid_items_scan_plan();
    case MTBLX_GRID_SCAN_EMIT: return mtblx_grid_items_scan_emit();
    case MTBLX_GRID_GET: return mtblx_grid_items_get();
    case MTBLX_GRID_MERGE_BUILD: return mtblx_grid_items_merge_build();
    case MTBLX_GRID_SEG_BUILD: return mtblx_grid_items_seg_build();
    case MTBLX_GRID_SORT_SKIP: return mtblx_grid_items_sort_skip();
    case MTBLX_GRID_CRC: return mtblx_grid_items_crc();
    case MTBLX_GRID_SNAPPY_SMALL: return mtblx_grid_items_snappy_small();
    case MTBLX_GRID_SNAPPY_LARGE: return mtblx_grid_items_snappy_large();
    case MTBLX_GRID_SNAPPY_COMP: return mtblx_grid_items_snappy_comp();
    case MTBLX_GRID_COPY_RANGES: return mtblx_grid_items_copy_ranges();
    case MTBLX_GRID_STREAM_COPY: return mtblx_grid_items_stream_copy(arg);
    case MTBLX_GRID_DECODE_PIPE: return mtblx_grid_items_decode_pipe();
    case MTBLX_GRID_DECODE_TILES: return mtblx_grid_items_decode_tiles(arg);
    default: return 0;
  }
}

extern "C" uint32_t mtblx_debug_decode_tiles(uint32_t nblk, uint32_t max_blk_len, int verify, int* kind) {
  return mtblx_impl_decode_tiles(nblk, max_blk_len, verify, kind);
}

extern "C" int mtblx_device_ok(void) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, dev) != hipSuccess) return 0;
  return strncmp(p.gcnArchName, "gfx950", 6) == 0 ? 1 : 0;
}

extern "C" size_t mtblx_decode_workspace_bytes(uint32_t nblk) {
  return mtblx_impl_ws_bytes(nblk) + 256u;
}

static int check_common(const mtblx_block_batch* in, const mtblx_decoded* out, void* ws, size_t wsb, void* stream) {
  if (!in || !out) return MTBLX_E_INVAL;
  if (in->nblk == 0) {  // empty batch: zero totals, nothing else to do
    if (out->totals && hipMemsetAsync(out->totals, 0, 32, reinterpret_cast<hipStream_t>(stream)) != hipSuccess)
      return MTBLX_E_HIP;
    return MTBLX_OK;
  }
  if (!in->data || !in->blk_off || !in->blk_len) return MTBLX_E_INVAL;
  if (!out->nrec || !out->rec_base || !out->key_base || !out->val_base || !out->status || !out->totals)
    return MTBLX_E_INVAL;
  if (!ws || wsb < mtblx_decode_workspace_bytes(in->nblk)) return MTBLX_E_INVAL;
  if ((reinterpret_cast<uintptr_t>(ws) & 7u) != 0) return MTBLX_E_INVAL;
  return 1;
}

extern "C" int mtblx_count_blocks(const mtblx_block_batch* in, const mtblx_decoded* out, void* ws, size_t wsb,
                                  void* stream) {
  int c = check_common(in, out, ws, wsb, stream);
  if (c != 1) return c;
  return mtblx_impl_run(in, out, ws, wsb, 0, reinterpret_cast<hipStream_t>(stream), 0, nullptr, nullptr, 0);
}

extern "C" int mtblx_decode_counted(const mtblx_block_batch* in, const mtblx_decoded* out, void* ws, size_t wsb,
                                    void* stream) {
  int c = check_common(in, out, ws, wsb, stream);
  if (c != 1) return c;
  if ((!out->keys && out->keys_cap) || (!out->vals && out->vals_cap) || (!out->key_end && out->rec_cap) ||
      (!out->val_end && out->rec_cap))
    return MTBLX_E_INVAL;
  // single-pass kernel: counting is fused into the decode, so this is a full decode
  return mtblx_impl_run(in, out, ws, wsb, 1, reinterpret_cast<hipStream_t>(stream), 0, nullptr, nullptr, 0);
}

extern "C" int mtblx_decode_blocks(const mtblx_block_batch* in, const mtblx_decoded* out, void* ws, size_t wsb,
                                   void* stream) {
  int c = check_common(in, out, ws, wsb, stream);
  if (c != 1) return c;
  if ((!out->keys && out->keys_cap) || (!out->vals && out->vals_cap) || (!out->key_end && out->rec_cap) ||
      (!out->val_end && out->rec_cap))
    return MTBLX_E_INVAL;
  return mtblx_impl_run(in, out, ws, wsb, 1, reinterpret_cast<hipStream_t>(stream), 0, nullptr, nullptr, 0);
}

extern "C" int mtblx_decode_blocks_valpos(const mtblx_block_batch* in, const mtblx_decoded* out, uint32_t* val_pos,
                                          void* ws, size_t wsb, void* stream) {
  if (out && !val_pos && out->rec_cap) return MTBLX_E_INVAL;   // before any HIP call
  int c = check_common(in, out, ws, wsb, stream);
  if (c != 1) return c;
  // out->vals / out->vals_cap are not looked at: no value byte is written
  if ((!out->keys && out->keys_cap) || (!out->key_end && out->rec_cap) || (!out->val_end && out->rec_cap))
    return MTBLX_E_INVAL;
  return mtblx_impl_run_valpos(in, out, val_pos, ws, wsb, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int mtblx_decode_blocks_verify(const mtblx_block_batch* in, const mtblx_decoded* out, uint32_t* crc,
                                          uint8_t* crc_bad, int framed, void* ws, size_t wsb, void* stream) {
  int c = check_common(in, out, ws, wsb, stream);
  if (c != 1) return c;
  if ((!out->keys && out->keys_cap) || (!out->vals && out->vals_cap) || (!out->key_end && out->rec_cap) ||
      (!out->val_end && out->rec_cap) || (!crc && !crc_bad))
    return MTBLX_E_INVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (framed & MTBLX_VERIFY_FUSED)   // one launch: the CRC from the LDS-staged tiles
    return mtblx_impl_run(in, out, ws, wsb, 1, s, 1, crc, crc_bad, framed & 1);
  // default: the decode, then the CRC-32C kernel (k_crc32c_mfma) on the same stream
  const int rc = mtblx_impl_run(in, out, ws, wsb, 1, s, 0, nullptr, nullptr, 0);
  if (rc != MTBLX_OK) return rc;
  return mtblx_crc32c_blocks(in, crc, crc_bad, framed & 1, stream);
}

// ---- Merger (csrc/merge.hip): the argument checks need no device ----
extern "C" size_t mtblx_merge_impl_ws_bytes(uint64_t nrec);
extern "C" int mtblx_merge_impl_plan(const mtblx_records* src, uint32_t nsrc, const mtblx_select* sel,
                                     uint64_t* totals, void* ws, hipStream_t s, float* phase_ms,
                                     uint32_t phase_cap);
extern "C" int mtblx_merge_impl_select_ok(const mtblx_select* sel, uint32_t nsrc);
extern "C" int mtblx_merge_impl_emit(const mtblx_records* src, uint32_t nsrc, int mode, const mtblx_merged* out,
                                     const void* ws, hipStream_t s);

extern "C" size_t mtblx_merge_workspace_bytes(uint64_t nrec, uint32_t nsrc) {
  (void)nsrc;   // the source table travels in the kernel arguments
  if (nrec >= MTBLX_MERGE_MAX_RECORDS) return 0;
  return mtblx_merge_impl_ws_bytes(nrec);
}

static int merge_check(const mtblx_records* src, uint32_t nsrc, const void* ws, size_t wsb) {
  if (nsrc > MTBLX_MERGE_MAX_SOURCES || (nsrc && !src)) return MTBLX_E_INVAL;
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255u) != 0) return MTBLX_E_INVAL;
  uint64_t n = 0;
  for (uint32_t i = 0; i < nsrc; ++i) {
    if (src[i].n >= MTBLX_MERGE_MAX_RECORDS) return MTBLX_E_INVAL;
    n += src[i].n;
  }
  if (n >= MTBLX_MERGE_MAX_RECORDS || wsb < mtblx_merge_impl_ws_bytes(n)) return MTBLX_E_INVAL;
  return MTBLX_OK;
}

// sel == NULL: mtblx_merge_plan itself (totals[6] and [7] are 0: nothing was left out)
extern "C" int mtblx_merge_plan_select(const mtblx_records* src, uint32_t nsrc, const mtblx_select* sel,
                                       uint64_t* totals, void* ws, size_t wsb, void* stream) {
  if (!totals) return MTBLX_E_INVAL;
  if (sel && (nsrc > MTBLX_MERGE_MAX_SOURCES || !mtblx_merge_impl_select_ok(sel, nsrc))) return MTBLX_E_INVAL;
  const int c = merge_check(src, nsrc, ws, wsb);
  if (c != MTBLX_OK) return c;
  totals[6] = totals[7] = 0;
  return mtblx_merge_impl_plan(src, nsrc, sel, totals, ws, reinterpret_cast<hipStream_t>(stream), nullptr, 0);
}

extern "C" int mtblx_merge_plan(const mtblx_records* src, uint32_t nsrc, uint64_t* totals, void* ws, size_t wsb,
                                void* stream) {
  if (!totals) return MTBLX_E_INVAL;
  const int c = merge_check(src, nsrc, ws, wsb);
  if (c != MTBLX_OK) return c;
  return mtblx_merge_impl_plan(src, nsrc, nullptr, totals, ws, reinterpret_cast<hipStream_t>(stream), nullptr, 0);
}

extern "C" int mtblx_merge_plan_timed(const mtblx_records* src, uint32_t nsrc, uint64_t* totals, void* ws, size_t wsb,
                                      void* stream, float* phase_ms, uint32_t phase_cap) {
  if (!totals || !phase_ms) return MTBLX_E_INVAL;
  const int c = merge_check(src, nsrc, ws, wsb);
  if (c != MTBLX_OK) return c;
  return mtblx_merge_impl_plan(src, nsrc, nullptr, totals, ws, reinterpret_cast<hipStream_t>(stream), phase_ms,
                               phase_cap);
}

extern "C" int mtblx_merge_emit(const mtblx_records* src, uint32_t nsrc, int mode, const mtblx_merged* out,
                                const void* ws, size_t wsb, void* stream) {
  if (!out || !out->flags || mode < MTBLX_MERGE_GROUPS || mode > MTBLX_MERGE_LAST) return MTBLX_E_INVAL;
  if ((!out->keys && out->keys_cap) || (!out->key_end && out->key_end_cap) || (!out->vals && out->vals_cap) ||
      (!out->val_end && out->val_end_cap) || (!out->grp_end && out->grp_end_cap))
    return MTBLX_E_INVAL;
  const int c = merge_check(src, nsrc, ws, wsb);
  if (c != MTBLX_OK) return c;
  return mtblx_merge_impl_emit(src, nsrc, mode, out, ws, reinterpret_cast<hipStream_t>(stream));
}

// ---- Sorter (csrc/sort.hip): one batch of unsorted records; the argument checks need no device ----
extern "C" size_t mtblx_sort_impl_ws_bytes(uint64_t nrec);
extern "C" int mtblx_sort_impl_plan(const mtblx_records* in, uint64_t* totals, void* ws, hipStream_t s,
                                    float* phase_ms, uint32_t phase_cap);
extern "C" int mtblx_sort_impl_emit(const mtblx_records* in, int mode, const mtblx_merged* out, const void* ws,
                                    hipStream_t s);

extern "C" size_t mtblx_sort_workspace_bytes(uint64_t nrec) {
  if (nrec >= MTBLX_MERGE_MAX_RECORDS) return 0;
  return mtblx_sort_impl_ws_bytes(nrec);
}

static int sort_check(const mtblx_records* in, const void* ws, size_t wsb) {
  if (!in || in->n >= MTBLX_MERGE_MAX_RECORDS) return MTBLX_E_INVAL;
  if (in->n && (!in->key_end || !in->val_end)) return MTBLX_E_INVAL;
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255u) != 0) return MTBLX_E_INVAL;
  if (wsb < mtblx_sort_impl_ws_bytes(in->n)) return MTBLX_E_INVAL;
  return MTBLX_OK;
}

extern "C" int mtblx_sort_plan(const mtblx_records* in, uint64_t* totals, void* ws, size_t wsb, void* stream) {
  if (!totals) return MTBLX_E_INVAL;
  const int c = sort_check(in, ws, wsb);
  if (c != MTBLX_OK) return c;
  return mtblx_sort_impl_plan(in, totals, ws, reinterpret_cast<hipStream_t>(stream), nullptr, 0);
}

extern "C" int mtblx_sort_plan_timed(const mtblx_records* in, uint64_t* totals, void* ws, size_t wsb, void* stream,
                                     float* phase_ms, uint32_t phase_cap) {
  if (!totals || !phase_ms) return MTBLX_E_INVAL;
  const int c = sort_check(in, ws, wsb);
  if (c != MTBLX_OK) return c;
  return mtblx_sort_impl_plan(in, totals, ws, reinterpret_cast<hipStream_t>(stream), phase_ms, phase_cap);
}

extern "C" int mtblx_sort_emit(const mtblx_records* in, int mode, const mtblx_merged* out, const void* ws, size_t wsb,
                               void* stream) {
  if (!out || !out->flags || mode < MTBLX_MERGE_GROUPS || mode > MTBLX_MERGE_LAST) return MTBLX_E_INVAL;
  if ((!out->keys && out->keys_cap) || (!out->key_end && out->key_end_cap) || (!out->vals && out->vals_cap) ||
      (!out->val_end && out->val_end_cap) || (!out->grp_end && out->grp_end_cap))
    return MTBLX_E_INVAL;
  const int c = sort_check(in, ws, wsb);
  if (c != MTBLX_OK) return c;
  return mtblx_sort_impl_emit(in, mode, out, ws, reinterpret_cast<hipStream_t>(stream));
}

// ---- device merge functions (csrc/reduce_dev.h): the spec is checked before any HIP call ----
extern "C" int mtblx_merge_impl_emit_reduce(const mtblx_records* src, uint32_t nsrc, const mtblx_reduce* spec,
                                            const mtblx_merged* out, void* ws, hipStream_t s);
extern "C" int mtblx_sort_impl_emit_reduce(const mtblx_records* in, const mtblx_reduce* spec, const mtblx_merged* out,
                                           void* ws, hipStream_t s);

// a reduce spec: 1 to 8 ops, each SUM / MIN / MAX, with MTBLX_REDUCE_VARINT on all of them or on none
static int spec_check(const mtblx_reduce* spec) {
  if (!spec || spec->nfields < 1 || spec->nfields > MTBLX_REDUCE_MAX_FIELDS) return MTBLX_E_INVAL;
  uint32_t nv = 0;
  for (uint32_t f = 0; f < spec->nfields; ++f) {
    if ((spec->op[f] & ~MTBLX_REDUCE_VARINT) > MTBLX_REDUCE_MAX) return MTBLX_E_INVAL;
    if (spec->op[f] & MTBLX_REDUCE_VARINT) ++nv;
  }
  return nv == 0 || nv == spec->nfields ? MTBLX_OK : MTBLX_E_INVAL;
}

static int reduce_check(const mtblx_reduce* spec, const mtblx_merged* out) {
  if (spec_check(spec) != MTBLX_OK) return MTBLX_E_INVAL;
  if (!out || !out->flags) return MTBLX_E_INVAL;
  if ((!out->keys && out->keys_cap) || (!out->key_end && out->key_end_cap) || (!out->vals && out->vals_cap) ||
      (!out->val_end && out->val_end_cap))
    return MTBLX_E_INVAL;
  return MTBLX_OK;
}

extern "C" int mtblx_merge_emit_reduce(const mtblx_records* src, uint32_t nsrc, const mtblx_reduce* spec,
                                       const mtblx_merged* out, void* ws, size_t wsb, void* stream) {
  int c = reduce_check(spec, out);
  if (c != MTBLX_OK) return c;
  c = merge_check(src, nsrc, ws, wsb);
  if (c != MTBLX_OK) return c;
  return mtblx_merge_impl_emit_reduce(src, nsrc, spec, out, ws, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int mtblx_sort_emit_reduce(const mtblx_records* in, const mtblx_reduce* spec, const mtblx_merged* out,
                                      void* ws, size_t wsb, void* stream) {
  int c = reduce_check(spec, out);
  if (c != MTBLX_OK) return c;
  c = sort_check(in, ws, wsb);
  if (c != MTBLX_OK) return c;
  return mtblx_sort_impl_emit_reduce(in, spec, out, ws, reinterpret_cast<hipStream_t>(stream));
}

// ---- segmented merge (csrc/merge_seg.hip): the argument checks need no device ----
extern "C" size_t mtblx_merge_seg_impl_ws_bytes(uint64_t nrec, uint32_t nseg);
extern "C" int mtblx_merge_seg_impl_plan(const mtblx_records* src, const uint64_t* const* seg_off, uint32_t nsrc,
                                         uint32_t nseg, const mtblx_select* sel, uint64_t* totals, uint64_t* seg_end,
                                         void* ws, hipStream_t s, float* phase_ms, uint32_t phase_cap);
extern "C" int mtblx_merge_seg_impl_emit(const mtblx_records* src, uint32_t nsrc, uint32_t nseg, int mode,
                                         const mtblx_reduce* spec, const mtblx_merged* out, void* ws, hipStream_t s);

extern "C" size_t mtblx_merge_seg_workspace_bytes(uint64_t nrec, uint32_t nsrc, uint32_t nseg) {
  (void)nsrc;   // the source and offset tables travel in the kernel arguments
  if (nrec >= MTBLX_MERGE_MAX_RECORDS || nseg > MTBLX_MERGE_MAX_SEGMENTS) return 0;
  return mtblx_merge_seg_impl_ws_bytes(nrec, nseg);
}

static int merge_seg_check(const mtblx_records* src, const uint64_t* const* seg_off, uint32_t nsrc, uint32_t nseg,
                           const void* ws, size_t wsb) {
  if (nsrc > MTBLX_MERGE_MAX_SOURCES || nseg > MTBLX_MERGE_MAX_SEGMENTS) return MTBLX_E_INVAL;
  if (nsrc && (!src || !seg_off)) return MTBLX_E_INVAL;
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255u) != 0) return MTBLX_E_INVAL;
  uint64_t n = 0;
  for (uint32_t i = 0; i < nsrc; ++i) {
    if (!seg_off[i] || src[i].n >= MTBLX_MERGE_MAX_RECORDS) return MTBLX_E_INVAL;
    if (src[i].n && (!src[i].key_end || !src[i].val_end)) return MTBLX_E_INVAL;
    n += src[i].n;
  }
  if (n >= MTBLX_MERGE_MAX_RECORDS || wsb < mtblx_merge_seg_impl_ws_bytes(n, nseg)) return MTBLX_E_INVAL;
  return MTBLX_OK;
}

extern "C" int mtblx_merge_seg_plan_timed(const mtblx_records* src, const uint64_t* const* seg_off, uint32_t nsrc,
                                          uint32_t nseg, uint64_t* totals, uint64_t* seg_end, void* ws, size_t wsb,
                                          void* stream, float* phase_ms, uint32_t phase_cap) {
  if (!totals || !phase_ms || (nseg && !seg_end)) return MTBLX_E_INVAL;
  const int c = merge_seg_check(src, seg_off, nsrc, nseg, ws, wsb);
  if (c != MTBLX_OK) return c;
  return mtblx_merge_seg_impl_plan(src, seg_off, nsrc, nseg, nullptr, totals, seg_end, ws,
                                   reinterpret_cast<hipStream_t>(stream), phase_ms, phase_cap);
}

extern "C" int mtblx_merge_seg_plan(const mtblx_records* src, const uint64_t* const* seg_off, uint32_t nsrc,
                                    uint32_t nseg, uint64_t* totals, uint64_t* seg_end, void* ws, size_t wsb,
                                    void* stream) {
  if (!totals || (nseg && !seg_end)) return MTBLX_E_INVAL;
  const int c = merge_seg_check(src, seg_off, nsrc, nseg, ws, wsb);
  if (c != MTBLX_OK) return c;
  return mtblx_merge_seg_impl_plan(src, seg_off, nsrc, nseg, nullptr, totals, seg_end, ws,
                                   reinterpret_cast<hipStream_t>(stream), nullptr, 0);
}

// sel == NULL: mtblx_merge_seg_plan itself (totals[6] and [7] are 0: nothing was left out)
extern "C" int mtblx_merge_seg_plan_select(const mtblx_records* src, const uint64_t* const* seg_off, uint32_t nsrc,
                                           uint32_t nseg, const mtblx_select* sel, uint64_t* totals,
                                           uint64_t* seg_end, void* ws, size_t wsb, void* stream) {
  if (!totals || (nseg && !seg_end)) return MTBLX_E_INVAL;
  if (sel && (nsrc > MTBLX_MERGE_MAX_SOURCES || !mtblx_merge_impl_select_ok(sel, nsrc))) return MTBLX_E_INVAL;
  const int c = merge_seg_check(src, seg_off, nsrc, nseg, ws, wsb);
  if (c != MTBLX_OK) return c;
  totals[6] = totals[7] = 0;
  return mtblx_merge_seg_impl_plan(src, seg_off, nsrc, nseg, sel, totals, seg_end, ws,
                                   reinterpret_cast<hipStream_t>(stream), nullptr, 0);
}

extern "C" int mtblx_merge_seg_emit(const mtblx_records* src, const uint64_t* const* seg_off, uint32_t nsrc,
                                    uint32_t nseg, int mode, const mtblx_merged* out, const void* ws, size_t wsb,
                                    void* stream) {
  if (!out || !out->flags || mode < MTBLX_MERGE_GROUPS || mode > MTBLX_MERGE_LAST) return MTBLX_E_INVAL;
  if ((!out->keys && out->keys_cap) || (!out->key_end && out->key_end_cap) || (!out->vals && out->vals_cap) ||
      (!out->val_end && out->val_end_cap) || (!out->grp_end && out->grp_end_cap))
    return MTBLX_E_INVAL;
  const int c = merge_seg_check(src, seg_off, nsrc, nseg, ws, wsb);
  if (c != MTBLX_OK) return c;
  // the plain emit only reads the workspace
  return mtblx_merge_seg_impl_emit(src, nsrc, nseg, mode, nullptr, out, const_cast<void*>(ws),
                                   reinterpret_cast<hipStream_t>(stream));
}

extern "C" int mtblx_merge_seg_emit_reduce(const mtblx_records* src, const uint64_t* const* seg_off, uint32_t nsrc,
                                           uint32_t nseg, const mtblx_reduce* spec, const mtblx_merged* out, void* ws,
                                           size_t wsb, void* stream) {
  int c = reduce_check(spec, out);
  if (c != MTBLX_OK) return c;
  c = merge_seg_check(src, seg_off, nsrc, nseg, ws, wsb);
  if (c != MTBLX_OK) return c;
  return mtblx_merge_seg_impl_emit(src, nsrc, nseg, MTBLX_MERGE_FIRST, spec, out, ws,
                                   reinterpret_cast<hipStream_t>(stream));
}

// ---- batched scans (csrc/scan.hip): the argument checks need no device ----
extern "C" size_t mtblx_scan_impl_ws_bytes(uint32_t nq);
extern "C" int mtblx_scan_impl_plan(const uint8_t* file, uint64_t file_len, uint32_t version, int verify,
                                    uint64_t index_off, uint64_t index_len, const uint64_t* tab_start,
                                    const uint64_t* tab_doff, const uint64_t* tab_dlen, const int32_t* tab_st,
                                    uint32_t ntab, const uint8_t* dec, const int32_t* type, const uint8_t* keys,
                                    const uint64_t* key_end, const uint8_t* keys2, const uint64_t* key2_end,
                                    const uint64_t* max_records, uint32_t max_blocks, uint32_t nq,
                                    mtblx_scan_result* res, uint64_t* totals, void* ws, hipStream_t s);
extern "C" int mtblx_scan_impl_emit(const uint8_t* file, uint64_t file_len, uint32_t version, uint64_t index_off,
                                    uint64_t index_len, const uint64_t* tab_start, const uint64_t* tab_doff,
                                    const uint64_t* tab_dlen, const int32_t* tab_st, uint32_t ntab,
                                    const uint8_t* dec, uint32_t nq, const mtblx_scanned* out, const void* ws,
                                    hipStream_t s);

extern "C" size_t mtblx_scan_workspace_bytes(uint32_t nq) { return mtblx_scan_impl_ws_bytes(nq); }

static int scan_check(const uint8_t* file, uint32_t version, const uint64_t* tab_start, const uint64_t* tab_doff,
                      const uint64_t* tab_dlen, const int32_t* tab_st, uint32_t ntab, const uint8_t* dec, uint32_t nq,
                      const void* ws, size_t wsb) {
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255u) != 0 || wsb < mtblx_scan_impl_ws_bytes(nq)) return MTBLX_E_INVAL;
  if (version > 1) return MTBLX_E_INVAL;
  if (nq && !file) return MTBLX_E_INVAL;
  if (dec && ntab && (!tab_start || !tab_doff || !tab_dlen || !tab_st)) return MTBLX_E_INVAL;
  return MTBLX_OK;
}

// what mtblx_scan_plan and mtblx_scan_reduce check alike; MTBLX_OK: the totals are zeroed
static int scan_plan_check(const uint8_t* file, uint32_t version, const uint64_t* tab_start, const uint64_t* tab_doff,
                           const uint64_t* tab_dlen, const int32_t* tab_st, uint32_t ntab, const uint8_t* dec,
                           const int32_t* type, const uint8_t* keys, const uint64_t* key_end, const uint8_t* keys2,
                           const uint64_t* key2_end, uint32_t nq, const mtblx_scan_result* res, uint64_t* totals,
                           const void* ws, size_t wsb) {
  if (!totals) return MTBLX_E_INVAL;
  const int c = scan_check(file, version, tab_start, tab_doff, tab_dlen, tab_st, ntab, dec, nq, ws, wsb);
  if (c != MTBLX_OK) return c;
  if (nq && (!type || !keys || !key_end || !res)) return MTBLX_E_INVAL;
  for (uint32_t q = 0; q < nq; ++q) {
    if (type[q] < 0 || type[q] > 3) return MTBLX_E_INVAL;
    if (type[q] == 3 && (!keys2 || !key2_end)) return MTBLX_E_INVAL;
  }
  memset(totals, 0, 4 * sizeof(uint64_t));
  return MTBLX_OK;
}

extern "C" int mtblx_scan_plan(const uint8_t* file, uint64_t file_len, uint32_t version, int verify, uint64_t index_off,
                               uint64_t index_len, const uint64_t* tab_start, const uint64_t* tab_doff,
                               const uint64_t* tab_dlen, const int32_t* tab_st, uint32_t ntab, const uint8_t* dec,
                               const int32_t* type, const uint8_t* keys, const uint64_t* key_end, const uint8_t* keys2,
                               const uint64_t* key2_end, const uint64_t* max_records, uint32_t max_blocks, uint32_t nq,
                               mtblx_scan_result* res, uint64_t* totals, void* ws, size_t wsb, void* stream) {
  const int c = scan_plan_check(file, version, tab_start, tab_doff, tab_dlen, tab_st, ntab, dec, type, keys, key_end,
                                keys2, key2_end, nq, res, totals, ws, wsb);
  if (c != MTBLX_OK) return c;
  if (nq == 0) return MTBLX_OK;
  return mtblx_scan_impl_plan(file, file_len, version, verify, index_off, index_len, tab_start, tab_doff, tab_dlen,
                              tab_st, ntab, dec, type, keys, key_end, keys2, key2_end, max_records, max_blocks, nq, res,
                              totals, ws, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int mtblx_scan_emit(const uint8_t* file, uint64_t file_len, uint32_t version, uint64_t index_off,
                               uint64_t index_len, const uint64_t* tab_start, const uint64_t* tab_doff,
                               const uint64_t* tab_dlen, const int32_t* tab_st, uint32_t ntab, const uint8_t* dec,
                               uint32_t nq, const mtblx_scanned* out, const void* ws, size_t wsb, void* stream) {
  if (!out || !out->flags) return MTBLX_E_INVAL;
  if ((!out->keys && out->keys_cap) || (!out->vals && out->vals_cap) ||
      ((!out->key_end || !out->val_end) && out->rec_cap))
    return MTBLX_E_INVAL;
  const int c = scan_check(file, version, tab_start, tab_doff, tab_dlen, tab_st, ntab, dec, nq, ws, wsb);
  if (c != MTBLX_OK) return c;
  if (nq == 0) return MTBLX_OK;
  return mtblx_scan_impl_emit(file, file_len, version, index_off, index_len, tab_start, tab_doff, tab_dlen, tab_st,
                              ntab, dec, nq, out, ws, reinterpret_cast<hipStream_t>(stream));
}

// ---- aggregating scans (csrc/scan.hip, csrc/reduce_seg.hip): the spec and the outputs are checked
// before any HIP call ----
extern "C" int mtblx_scan_impl_reduce(const uint8_t* file, uint64_t file_len, uint32_t version, int verify,
                                      uint64_t index_off, uint64_t index_len, const uint64_t* tab_start,
                                      const uint64_t* tab_doff, const uint64_t* tab_dlen, const int32_t* tab_st,
                                      uint32_t ntab, const uint8_t* dec, const int32_t* type, const uint8_t* keys,
                                      const uint64_t* key_end, const uint8_t* keys2, const uint64_t* key2_end,
                                      const uint64_t* max_records, uint32_t max_blocks, uint32_t nq,
                                      mtblx_scan_result* res, uint64_t* totals, void* ws, const mtblx_reduce* spec,
                                      uint64_t* fields, uint64_t* nbad, const mtblx_where* where, uint64_t* nmatch,
                                      hipStream_t s);
extern "C" int mtblx_reduce_seg_impl(const mtblx_records* recs, const uint64_t* seg_lo, const uint64_t* seg_hi,
                                     uint32_t nseg, const mtblx_reduce* spec, uint64_t* fields, uint64_t* nbad,
                                     uint32_t* flags, hipStream_t s);

extern "C" int mtblx_scan_reduce(const uint8_t* file, uint64_t file_len, uint32_t version, int verify,
                                 uint64_t index_off, uint64_t index_len, const uint64_t* tab_start,
                                 const uint64_t* tab_doff, const uint64_t* tab_dlen, const int32_t* tab_st,
                                 uint32_t ntab, const uint8_t* dec, const int32_t* type, const uint8_t* keys,
                                 const uint64_t* key_end, const uint8_t* keys2, const uint64_t* key2_end,
                                 const uint64_t* max_records, uint32_t max_blocks, uint32_t nq, mtblx_scan_result* res,
                                 uint64_t* totals, void* ws, size_t wsb, const mtblx_reduce* spec, uint64_t* fields,
                                 uint64_t* nbad, void* stream) {
  if (!fields || !nbad || ((reinterpret_cast<uintptr_t>(fields) | reinterpret_cast<uintptr_t>(nbad)) & 7u))
    return MTBLX_E_INVAL;
  int c = spec_check(spec);
  if (c != MTBLX_OK) return c;
  c = scan_plan_check(file, version, tab_start, tab_doff, tab_dlen, tab_st, ntab, dec, type, keys, key_end, keys2,
                      key2_end, nq, res, totals, ws, wsb);
  if (c != MTBLX_OK) return c;
  if (nq == 0) return MTBLX_OK;
  return mtblx_scan_impl_reduce(file, file_len, version, verify, index_off, index_len, tab_start, tab_doff, tab_dlen,
                                tab_st, ntab, dec, type, keys, key_end, keys2, key2_end, max_records, max_blocks, nq,
                                res, totals, ws, spec, fields, nbad, nullptr, nullptr,
                                reinterpret_cast<hipStream_t>(stream));
}

extern "C" int mtblx_reduce_segments(const mtblx_records* recs, const uint64_t* seg_lo, const uint64_t* seg_hi,
                                     uint32_t nseg, const mtblx_reduce* spec, uint64_t* fields, uint64_t* nbad,
                                     uint32_t* flags, void* stream) {
  if (!fields || !nbad || !flags) return MTBLX_E_INVAL;
  // the kernels load and update these as aligned words
  if (((reinterpret_cast<uintptr_t>(fields) | reinterpret_cast<uintptr_t>(nbad) | reinterpret_cast<uintptr_t>(seg_lo) |
        reinterpret_cast<uintptr_t>(seg_hi)) & 7u) || (reinterpret_cast<uintptr_t>(flags) & 3u))
    return MTBLX_E_INVAL;
  if (nseg > MTBLX_REDUCE_MAX_SEGMENTS) return MTBLX_E_INVAL;
  const int c = spec_check(spec);
  if (c != MTBLX_OK) return c;
  if (!recs || recs->n >= MTBLX_MERGE_MAX_RECORDS) return MTBLX_E_INVAL;
  if (recs->n && (!recs->val_end || (reinterpret_cast<uintptr_t>(recs->val_end) & 7u)))
    return MTBLX_E_INVAL;   // vals may be NULL where every value is empty
  if (nseg && (!seg_lo || !seg_hi)) return MTBLX_E_INVAL;
  if (nseg == 0) return MTBLX_OK;
  return mtblx_reduce_seg_impl(recs, seg_lo, seg_hi, nseg, spec, fields, nbad, flags,
                               reinterpret_cast<hipStream_t>(stream));
}

// ---- rollups (csrc/rollup.hip): every argument is checked before any HIP call ----
extern "C" size_t mtblx_rollup_impl_ws_bytes(uint64_t n);
extern "C" int mtblx_rollup_impl_plan(const mtblx_records* recs, const mtblx_group* group, const uint64_t* seg_off,
                                      uint32_t nseg, uint64_t* totals, void* ws, hipStream_t s);
extern "C" int mtblx_rollup_impl_emit(const mtblx_records* recs, const mtblx_group* group, const uint64_t* seg_off,
                                      uint32_t nseg, const mtblx_rolled* out, const void* ws, hipStream_t s);
extern "C" size_t mtblx_reduce_encode_impl_ws_bytes(uint64_t n);
extern "C" int mtblx_reduce_encode_impl(const uint64_t* fields, uint64_t n, const mtblx_reduce* spec, uint8_t* vals,
                                        uint64_t* val_end, uint64_t cap, void* ws, hipStream_t s);

extern "C" size_t mtblx_rollup_workspace_bytes(uint64_t nrec, uint32_t nseg) {
  (void)nseg;   // the segments are read where the caller keeps them
  return mtblx_rollup_impl_ws_bytes(nrec);
}

// what mtblx_rollup_plan and mtblx_rollup_emit check alike
static int rollup_check(const mtblx_records* recs, const mtblx_group* g, const uint64_t* seg_off, uint32_t nseg,
                        const void* ws, size_t wsb) {
  if (!recs || !g) return MTBLX_E_INVAL;
  if (g->kind == MTBLX_GROUP_LENGTH) {
    if (g->length == 0) return MTBLX_E_INVAL;
  } else if (g->kind == MTBLX_GROUP_DELIM) {
    if (g->count == 0 || g->delim > 255u) return MTBLX_E_INVAL;
  } else {
    return MTBLX_E_INVAL;
  }
  if (recs->n >= MTBLX_MERGE_MAX_RECORDS || nseg > MTBLX_REDUCE_MAX_SEGMENTS) return MTBLX_E_INVAL;
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255u) != 0 || wsb < mtblx_rollup_impl_ws_bytes(recs->n))
    return MTBLX_E_INVAL;
  if (nseg && !seg_off) return MTBLX_E_INVAL;
  if (recs->n && !recs->key_end) return MTBLX_E_INVAL;   // keys may be NULL where every key is empty
  if ((reinterpret_cast<uintptr_t>(recs->key_end) | reinterpret_cast<uintptr_t>(seg_off)) & 7u) return MTBLX_E_INVAL;
  return MTBLX_OK;
}

extern "C" int mtblx_rollup_plan(const mtblx_records* recs, const mtblx_group* group, const uint64_t* seg_off,
                                 uint32_t nseg, uint64_t* totals, void* ws, size_t wsb, void* stream) {
  if (!totals || (reinterpret_cast<uintptr_t>(totals) & 7u)) return MTBLX_E_INVAL;
  const int c = rollup_check(recs, group, seg_off, nseg, ws, wsb);
  if (c != MTBLX_OK) return c;
  return mtblx_rollup_impl_plan(recs, group, seg_off, nseg, totals, ws, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int mtblx_rollup_emit(const mtblx_records* recs, const mtblx_group* group, const uint64_t* seg_off,
                                 uint32_t nseg, const mtblx_rolled* out, const void* ws, size_t wsb, void* stream) {
  if (!out || !out->flags || (reinterpret_cast<uintptr_t>(out->flags) & 3u)) return MTBLX_E_INVAL;
  if (!out->key_end || !out->grp_rec || (!out->keys && out->keys_cap) || (nseg && !out->seg_grp)) return MTBLX_E_INVAL;
  if ((reinterpret_cast<uintptr_t>(out->key_end) | reinterpret_cast<uintptr_t>(out->grp_rec) |
       reinterpret_cast<uintptr_t>(out->seg_grp)) & 7u)
    return MTBLX_E_INVAL;
  const int c = rollup_check(recs, group, seg_off, nseg, ws, wsb);
  if (c != MTBLX_OK) return c;
  return mtblx_rollup_impl_emit(recs, group, seg_off, nseg, out, ws, reinterpret_cast<hipStream_t>(stream));
}

extern "C" size_t mtblx_reduce_encode_workspace_bytes(uint64_t n) { return mtblx_reduce_encode_impl_ws_bytes(n); }

extern "C" int mtblx_reduce_encode(const uint64_t* fields, uint64_t n, const mtblx_reduce* spec, uint8_t* vals,
                                   uint64_t* val_end, uint64_t cap, void* ws, size_t wsb, void* stream) {
  const int c = spec_check(spec);
  if (c != MTBLX_OK) return c;
  if (n >= MTBLX_MERGE_MAX_RECORDS) return MTBLX_E_INVAL;
  if (n == 0) return MTBLX_OK;
  const bool varint = spec->op[0] & MTBLX_REDUCE_VARINT;
  if (!fields || !val_end || !vals || !ws) return MTBLX_E_INVAL;
  if ((reinterpret_cast<uintptr_t>(fields) | reinterpret_cast<uintptr_t>(val_end) | reinterpret_cast<uintptr_t>(ws)) & 7u)
    return MTBLX_E_INVAL;
  if (cap < (varint ? 10ull : 8ull) * spec->nfields * n || wsb < mtblx_reduce_encode_impl_ws_bytes(n))
    return MTBLX_E_INVAL;
  return mtblx_reduce_encode_impl(fields, n, spec, vals, val_end, cap, ws, reinterpret_cast<hipStream_t>(stream));
}

// ---- value predicates (csrc/where.hip): every argument is checked before any HIP call ----
extern "C" size_t mtblx_where_impl_ws_bytes(uint64_t n);
extern "C" int mtblx_where_impl_plan(const mtblx_records* recs, const mtblx_where* where, const uint64_t* seg_off,
                                     uint32_t nseg, uint64_t* totals, uint64_t* seg_end, uint64_t* seg_bad, void* ws,
                                     hipStream_t s);
extern "C" int mtblx_where_impl_emit(const mtblx_records* recs, const mtblx_filtered* out, const void* ws,
                                     hipStream_t s);

extern "C" size_t mtblx_where_workspace_bytes(uint64_t nrec, uint32_t nseg) {
  (void)nseg;   // the segments are read where the caller keeps them
  return mtblx_where_impl_ws_bytes(nrec);
}

static int where_spec_check(const mtblx_where* w) {
  if (!w || w->nfields < 1 || w->nfields > MTBLX_REDUCE_MAX_FIELDS) return MTBLX_E_INVAL;
  if (w->flags & ~(MTBLX_WHERE_ANY | MTBLX_WHERE_VARINT)) return MTBLX_E_INVAL;
  const uint32_t all = (1u << w->nfields) - 1u;
  if ((w->mask & ~all) || (w->outside & ~all) || (w->outside & ~w->mask)) return MTBLX_E_INVAL;
  return MTBLX_OK;
}

// what mtblx_where_plan and mtblx_where_emit check alike
static int where_check(const mtblx_records* recs, const void* ws, size_t wsb) {
  if (!recs || recs->n >= MTBLX_MERGE_MAX_RECORDS) return MTBLX_E_INVAL;
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255u) != 0 || wsb < mtblx_where_impl_ws_bytes(recs->n))
    return MTBLX_E_INVAL;
  if (recs->n && (!recs->key_end || !recs->val_end)) return MTBLX_E_INVAL;   // keys / vals may be NULL
  if ((reinterpret_cast<uintptr_t>(recs->key_end) | reinterpret_cast<uintptr_t>(recs->val_end)) & 7u)
    return MTBLX_E_INVAL;
  return MTBLX_OK;
}

extern "C" int mtblx_where_plan(const mtblx_records* recs, const mtblx_where* where, const uint64_t* seg_off,
                                uint32_t nseg, uint64_t* totals, uint64_t* seg_end, uint64_t* seg_bad, void* ws,
                                size_t wsb, void* stream) {
  if (!totals) return MTBLX_E_INVAL;
  int c = where_spec_check(where);
  if (c != MTBLX_OK) return c;
  c = where_check(recs, ws, wsb);
  if (c != MTBLX_OK) return c;
  if (nseg > MTBLX_REDUCE_MAX_SEGMENTS || (nseg && (!seg_off || !seg_end))) return MTBLX_E_INVAL;
  if ((reinterpret_cast<uintptr_t>(seg_off) | reinterpret_cast<uintptr_t>(seg_end) |
       reinterpret_cast<uintptr_t>(seg_bad)) & 7u)
    return MTBLX_E_INVAL;
  return mtblx_where_impl_plan(recs, where, seg_off, nseg, totals, seg_end, seg_bad, ws,
                               reinterpret_cast<hipStream_t>(stream));
}

extern "C" int mtblx_where_emit(const mtblx_records* recs, const mtblx_filtered* out, const void* ws, size_t wsb,
                                void* stream) {
  if (!out || !out->flags || (reinterpret_cast<uintptr_t>(out->flags) & 3u)) return MTBLX_E_INVAL;
  if ((!out->keys && out->keys_cap) || (!out->vals && out->vals_cap) ||
      ((!out->key_end || !out->val_end) && out->rec_cap))
    return MTBLX_E_INVAL;
  if ((reinterpret_cast<uintptr_t>(out->key_end) | reinterpret_cast<uintptr_t>(out->val_end) |
       reinterpret_cast<uintptr_t>(out->src_idx)) & 7u)
    return MTBLX_E_INVAL;
  const int c = where_check(recs, ws, wsb);
  if (c != MTBLX_OK) return c;
  return mtblx_where_impl_emit(recs, out, ws, reinterpret_cast<hipStream_t>(stream));
}

// the fused aggregating walk: mtblx_scan_reduce's checks, then the predicate's and its layout against the spec's
extern "C" int mtblx_scan_reduce_where(const uint8_t* file, uint64_t file_len, uint32_t version, int verify,
                                       uint64_t index_off, uint64_t index_len, const uint64_t* tab_start,
                                       const uint64_t* tab_doff, const uint64_t* tab_dlen, const int32_t* tab_st,
                                       uint32_t ntab, const uint8_t* dec, const int32_t* type, const uint8_t* keys,
                                       const uint64_t* key_end, const uint8_t* keys2, const uint64_t* key2_end,
                                       const uint64_t* max_records, uint32_t max_blocks, uint32_t nq,
                                       mtblx_scan_result* res, uint64_t* totals, void* ws, size_t wsb,
                                       const mtblx_reduce* spec, uint64_t* fields, uint64_t* nbad,
                                       const mtblx_where* where, uint64_t* nmatch, void* stream) {
  if (!fields || !nbad || !nmatch ||
      ((reinterpret_cast<uintptr_t>(fields) | reinterpret_cast<uintptr_t>(nbad) | reinterpret_cast<uintptr_t>(nmatch)) & 7u))
    return MTBLX_E_INVAL;
  int c = spec_check(spec);
  if (c != MTBLX_OK) return c;
  c = where_spec_check(where);
  if (c != MTBLX_OK) return c;
  const bool sv = spec->op[0] & MTBLX_REDUCE_VARINT, wv = where->flags & MTBLX_WHERE_VARINT;
  if (where->nfields != spec->nfields || sv != wv) return MTBLX_E_INVAL;
  c = scan_plan_check(file, version, tab_start, tab_doff, tab_dlen, tab_st, ntab, dec, type, keys, key_end, keys2,
                      key2_end, nq, res, totals, ws, wsb);
  if (c != MTBLX_OK) return c;
  if (nq == 0) return MTBLX_OK;
  return mtblx_scan_impl_reduce(file, file_len, version, verify, index_off, index_len, tab_start, tab_doff, tab_dlen,
                                tab_st, ntab, dec, type, keys, key_end, keys2, key2_end, max_records, max_blocks, nq,
                                res, totals, ws, spec, fields, nbad, where, nmatch,
                                reinterpret_cast<hipStream_t>(stream));
}

// ---- bounds-checked diagnostic build only (csrc/bounds.h, Makefile target `bounds`) ----
#ifdef MTBLX_BOUNDS
#include <stdio.h>

#include <mutex>
#include <string>
static std::mutex g_bounds_mu;
static unsigned long long g_bounds_viol = 0, g_bounds_fault = 0;
static std::string g_bounds_first;

extern "C" void mtblx_bounds_note(const char* kernel, uint64_t line, uint64_t addr, uint64_t nbytes, int fault) {
  std::lock_guard<std::mutex> lk(g_bounds_mu);
  if (fault) ++g_bounds_fault;
  else ++g_bounds_viol;
  if (g_bounds_first.empty()) {
    char buf[512];
    snprintf(buf, sizeof(buf), "%s %s line %llu addr 0x%llx bytes %llu", fault ? "FAULT" : "OOB", kernel,
             (unsigned long long)line, (unsigned long long)addr, (unsigned long long)nbytes);
    g_bounds_first = buf;
  }
}
#endif

// Violations recorded by the bounds-checked build (violations | faults << 32), the first one
// described in buf.  The product build has nothing to report: -1.
extern "C" long long mtblx_bounds_report(char* buf, size_t cap) {
#ifdef MTBLX_BOUNDS
  std::lock_guard<std::mutex> lk(g_bounds_mu);
  if (buf && cap) snprintf(buf, cap, "%s", g_bounds_first.c_str());
  return (long long)(g_bounds_viol | (g_bounds_fault << 32));
#else
  (void)buf;
  (void)cap;
  return -1;
#endif
}

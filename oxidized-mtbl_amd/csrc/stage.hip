// stage.hip — Snappy files in the Reader, on the MI355X (gfx950): the stored blocks of a directory
// become a staged batch of decompressed blocks and a lookup table without leaving the device
// (include/mtblx.h "device staging of Snappy blocks", DESIGN.md §4 "Snappy files in the Reader").
//
//   mtblx_stage_plan / _emit   Reader::block's decompress step (src/reader.rs:166-170) for the
//                              entries of a directory (all, or an ascending selection): gather the
//                              stored extents (entries the reference panics on before it
//                              decompresses are skipped), lay the outputs out from the preambles
//                              (mtblx_snappy_dir), decompress with snappy_dev.hip's kernels and
//                              their variant choice (mtblx_snappy_decompress_dev), then write the
//                              mtblx_block_batch directory and the rows mtblx_get_decompressed takes
//   mtblx_scan_touch           which directory entries a batch of queries will open: the fresh
//                              index seek of Reader::get / ReaderIntoIter::new_from for the start
//                              key and the bound, ORed into a bitmap.  A hint: the lookup kernels
//                              report what is missing
//   mtblx_bitmap_compact       set bits (minus an exclusion mask) -> ascending ordinals
//   mtblx_table_gather         per-ordinal rows -> the compact table the lookup kernels search
//   mtblx_dir_ascends          whether the stored content starts ascend with the ordinal
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bounds.h"
#include "mtblx.h"
#include "mtblx_host.h"
#include "reader_dev.h"

namespace mtblx_stage {

constexpr int kThreads = 256;

struct Layout {
  size_t hdr, src_off, dst_off, src_len, dst_len, status, dec_len, skip, snap, total;
};
static inline size_t up256(size_t x) { return (x + 255u) & ~(size_t)255u; }
static inline Layout layout(uint32_t n) {
  Layout L;
  L.hdr = 0;   // u64 [4]: mtblx_snappy_dir's totals (bytes, max length, corrupt preambles), skipped entries
  L.src_off = 256;
  L.dst_off = L.src_off + up256(8ull * n);
  L.src_len = L.dst_off + up256(8ull * n);
  L.dst_len = L.src_len + up256(4ull * n);
  L.status = L.dst_len + up256(4ull * n);
  L.dec_len = L.status + up256(4ull * n);
  L.skip = L.dec_len + up256(4ull * n);
  L.snap = L.skip + up256(n);
  L.total = L.snap + up256(mtblx_snappy_workspace_bytes(n));
  return L;
}

// entry j of the selection -> its stored extent; an entry Reader::block panics on before it
// decompresses (framing, checksum) is skipped: no stored bytes, no error
__global__ void __launch_bounds__(kThreads) k_stage_gather(uint64_t file_len, const uint64_t* blk_off,
                                                           const uint32_t* blk_len, const int32_t* dir_st,
                                                           const uint8_t* bad, uint32_t ndir, const uint32_t* sel,
                                                           uint32_t n, uint64_t* src_off, uint32_t* src_len,
                                                           uint8_t* skip, uint64_t* hdr) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= n) return;
  if (sel) MTBLX_CHK(sel + j, 4);
  const uint32_t o = sel ? sel[j] : j;
  bool sk = o >= ndir;
  uint64_t off = 0;
  uint32_t len = 0;
  if (!sk) {
    MTBLX_CHK(dir_st + o, 4);
    sk = dir_st[o] != MTBLX_DIR_OK;
    if (!sk && bad) { MTBLX_CHK(bad + o, 1); sk = bad[o] != 0; }
  }
  if (!sk) {
    MTBLX_CHK(blk_off + o, 8);
    MTBLX_CHK(blk_len + o, 4);
    off = blk_off[o];
    len = blk_len[o];
    if (off > file_len || len > file_len - off) { sk = true; off = 0; len = 0; }   // not a framed extent
  }
  MTBLX_CHK(src_off + j, 8);
  MTBLX_CHK(src_len + j, 4);
  MTBLX_CHK(skip + j, 1);
  src_off[j] = off;
  src_len[j] = len;
  skip[j] = sk ? 1 : 0;
  if (sk) atomicAdd(reinterpret_cast<unsigned long long*>(hdr + 3), 1ull);
}

// the decompressed blocks' directory and the table rows
__global__ void __launch_bounds__(kThreads) k_stage_finish(const uint64_t* blk_off, uint32_t ndir, const uint32_t* sel,
                                                           uint32_t n, uint64_t base, const uint64_t* ws_off,
                                                           const uint32_t* ws_dec, const int32_t* ws_st,
                                                           const uint8_t* skip, uint64_t* dst_off, uint32_t* dec_len,
                                                           uint64_t* tab_start, uint64_t* tab_doff, uint64_t* tab_dlen,
                                                           int32_t* tab_st, int by_ordinal) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= n) return;
  if (sel) MTBLX_CHK(sel + j, 4);
  const uint32_t o = sel ? sel[j] : j;
  MTBLX_CHK(ws_off + j, 8);
  MTBLX_CHK(ws_dec + j, 4);
  MTBLX_CHK(ws_st + j, 4);
  MTBLX_CHK(skip + j, 1);
  const bool sk = skip[j] != 0;
  const bool err = !sk && ws_st[j] != MTBLX_SNAPPY_OK;
  const uint64_t at = base + ws_off[j];
  const uint32_t len = (sk || err) ? 0u : ws_dec[j];
  if (dst_off) { MTBLX_CHK(dst_off + j, 8); dst_off[j] = at; }
  if (dec_len) { MTBLX_CHK(dec_len + j, 4); dec_len[j] = len; }
  if (!tab_start) return;
  if (by_ordinal && o >= ndir) return;
  const uint32_t r = by_ordinal ? o : j;
  uint64_t start = 0;
  if (o < ndir) { MTBLX_CHK(blk_off + o, 8); start = blk_off[o]; }
  MTBLX_CHK(tab_start + r, 8);
  MTBLX_CHK(tab_doff + r, 8);
  MTBLX_CHK(tab_dlen + r, 8);
  MTBLX_CHK(tab_st + r, 4);
  tab_start[r] = start;
  tab_doff[r] = at;
  tab_dlen[r] = len;
  tab_st[r] = err ? 1 : 0;
}

// the directory ordinal of the index entry at `entry` (the scan chain's offsets, ascending), or
// nent when the iterator is past the last entry; ~0u when it lies off the chain
__device__ __forceinline__ uint32_t ordinal_of(const uint64_t* eoffs, uint32_t nent, uint64_t entry, bool valid) {
  if (!valid) return nent;
  uint32_t lo = 0, hi = nent;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) / 2;
    MTBLX_CHK(eoffs + mid, 8);
    if (eoffs[mid] < entry) lo = mid + 1;
    else hi = mid;
  }
  if (lo == nent) return ~0u;
  MTBLX_CHK(eoffs + lo, 8);
  return eoffs[lo] == entry ? lo : ~0u;
}

__device__ __forceinline__ uint32_t land(const mtblx_rd::Blk& ib, const uint64_t* eoffs, uint32_t nent,
                                         const uint8_t* k, uint64_t kl) {
  using namespace mtblx_rd;
  It ii{};
  if (iter_init(ib, ii) != R_OK) return ~0u;
  if (seek(ib, ii, k, kl) != R_OK) return ~0u;
  return ordinal_of(eoffs, nent, ii.current, valid(ib, ii));
}

// one lane per query: the index seeks are short and independent
__global__ void __launch_bounds__(kThreads) k_scan_touch(const uint8_t* index, uint64_t idx_len, const uint64_t* eoffs,
                                                         uint32_t nent, const uint8_t* qkeys, const uint64_t* qend,
                                                         const uint8_t* qkeys2, const uint64_t* qend2,
                                                         const uint32_t* caps, uint32_t cap_all, uint32_t nq,
                                                         uint32_t* want, uint32_t nwords) {
  using namespace mtblx_rd;
  const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
  if (q >= nq || nent == 0) return;
  Blk ib{};
  if (block_init(index, idx_len, ib) != 0) return;
  MTBLX_CHK(qend + q, 8);
  const uint64_t k0 = q ? qend[q - 1] : 0;
  const uint32_t lo = land(ib, eoffs, nent, qkeys + k0, qend[q] - k0);
  if (lo >= nent) return;                         // past the last entry, or off the chain: nothing
  uint32_t cap = cap_all;
  if (caps) { MTBLX_CHK(caps + q, 4); cap = caps[q]; }
  if (cap == 0) return;
  uint32_t hi = nent - 1;                         // open ended
  if (qend2) {
    MTBLX_CHK(qend2 + q, 8);
    const uint64_t e0 = q ? qend2[q - 1] : 0;
    const uint64_t bl = qend2[q] - e0;
    if (bl) {
      const uint32_t b = land(ib, eoffs, nent, qkeys2 + e0, bl);
      // the block where the bound lands, plus the one the iterator opens when that block runs out
      // before the stop rule fires
      if (b < nent - 1) hi = b + 1;
    }
  }
  if (hi < lo) hi = lo;
  if (hi - lo > cap - 1) hi = lo + (cap - 1);
  for (uint32_t w = lo >> 5; w <= (hi >> 5) && w < nwords; ++w) {
    const uint32_t a = w == (lo >> 5) ? (lo & 31u) : 0u, z = w == (hi >> 5) ? (hi & 31u) : 31u;
    const uint32_t m = (z == 31u ? ~0u : ((1u << (z + 1)) - 1u)) & ~((1u << a) - 1u);
    MTBLX_CHK(want + w, 4);
    atomicOr(want + w, m);
  }
}

// one workgroup: the set bits of bits & ~exclude, ascending
__global__ void __launch_bounds__(1024) k_bitmap_compact(const uint32_t* bits, const uint32_t* exclude, uint32_t nbits,
                                                         uint32_t* list, uint32_t list_cap, uint32_t* count) {
  __shared__ uint32_t wsum[16];
  __shared__ uint32_t carry;
  const int tid = threadIdx.x;
  if (tid == 0) carry = 0;
  __syncthreads();
  const uint32_t nwords = (nbits + 31u) / 32u;
  for (uint32_t w0 = 0; w0 < nwords; w0 += 1024) {
    const uint32_t w = w0 + (uint32_t)tid;
    uint32_t v = 0;
    if (w < nwords) {
      MTBLX_CHK(bits + w, 4);
      v = bits[w];
      if (exclude) { MTBLX_CHK(exclude + w, 4); v &= ~exclude[w]; }
      if (w == nwords - 1 && (nbits & 31u)) v &= (1u << (nbits & 31u)) - 1u;
    }
    const uint32_t c = (uint32_t)__popc(v);
    uint32_t x = c;
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(x, o, 64);
      if ((tid & 63) >= o) x += y;
    }
    if ((tid & 63) == 63) wsum[tid >> 6] = x;
    __syncthreads();
    uint32_t at = carry + x - c;
    for (int i = 0; i < (tid >> 6); ++i) at += wsum[i];
    __syncthreads();
    if (tid == 1023) carry = at + c;
    while (v) {
      const uint32_t b = (uint32_t)__builtin_ctz(v);
      v &= v - 1;
      if (at < list_cap) { MTBLX_CHK(list + at, 4); list[at] = w * 32u + b; }
      ++at;
    }
    __syncthreads();
  }
  if (tid == 0) { MTBLX_CHK(count, 4); *count = carry; }
}

__global__ void __launch_bounds__(kThreads) k_table_gather(const uint32_t* list, uint32_t n, uint32_t nrow,
                                                           const uint64_t* blk_off, const uint64_t* row_doff,
                                                           const uint64_t* row_dlen, const int32_t* row_st,
                                                           uint64_t* tab_start, uint64_t* tab_doff, uint64_t* tab_dlen,
                                                           int32_t* tab_st) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= n) return;
  MTBLX_CHK(list + j, 4);
  const uint32_t o = list[j];
  MTBLX_CHK(tab_start + j, 8);
  MTBLX_CHK(tab_doff + j, 8);
  MTBLX_CHK(tab_dlen + j, 8);
  MTBLX_CHK(tab_st + j, 4);
  if (o >= nrow) {   // not a row: a block that fails like Err(Io), at a start no framing produces
    tab_start[j] = ~0ull; tab_doff[j] = 0; tab_dlen[j] = 0; tab_st[j] = 1;
    return;
  }
  MTBLX_CHK(blk_off + o, 8);
  MTBLX_CHK(row_doff + o, 8);
  MTBLX_CHK(row_dlen + o, 8);
  MTBLX_CHK(row_st + o, 4);
  tab_start[j] = blk_off[o];
  tab_doff[j] = row_doff[o];
  tab_dlen[j] = row_dlen[o];
  tab_st[j] = row_st[o];
}

__global__ void __launch_bounds__(kThreads) k_dir_ascends(const uint64_t* blk_off, const int32_t* dir_st, uint32_t ndir,
                                                          uint32_t* violations) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= ndir) return;
  MTBLX_CHK(dir_st + i, 4);
  MTBLX_CHK(blk_off + i, 8);
  bool bad = dir_st[i] != MTBLX_DIR_OK;
  if (!bad && i + 1 < ndir) { MTBLX_CHK(blk_off + i + 1, 8); bad = !(blk_off[i] < blk_off[i + 1]); }
  if (bad) atomicAdd(violations, 1u);
}

static inline dim3 grid_of(uint32_t n) { return dim3((n + kThreads - 1) / kThreads); }

}  // namespace mtblx_stage

using namespace mtblx_stage;

extern "C" size_t mtblx_stage_workspace_bytes(uint32_t n) { return layout(n).total; }

extern "C" int mtblx_stage_plan(const uint8_t* file, uint64_t file_len, const uint64_t* blk_off, const uint32_t* blk_len,
                                const int32_t* dir_st, const uint8_t* bad, uint32_t ndir, const uint32_t* sel,
                                uint32_t nsel, uint64_t* totals, void* workspace, size_t ws_bytes, void* stream) {
  if (!totals) return MTBLX_E_INVAL;
  totals[0] = totals[1] = totals[2] = 0;
  const uint32_t n = sel ? nsel : ndir;
  if (n == 0) return MTBLX_OK;
  if (!file || !blk_off || !blk_len || !dir_st || !workspace || ((uintptr_t)workspace & 255u)) return MTBLX_E_INVAL;
  const Layout L = layout(n);
  if (ws_bytes < L.total) return MTBLX_E_INVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  uint8_t* w = static_cast<uint8_t*>(workspace);
  uint64_t* hdr = reinterpret_cast<uint64_t*>(w + L.hdr);
  uint64_t* src_off = reinterpret_cast<uint64_t*>(w + L.src_off);
  uint32_t* src_len = reinterpret_cast<uint32_t*>(w + L.src_len);
  if (hipMemsetAsync(hdr, 0, 32, s) != hipSuccess) return MTBLX_E_HIP;
  MTBLX_LAUNCH((MTBLX_R(blk_off, 8ull * ndir), MTBLX_R(blk_len, 4ull * ndir), MTBLX_R(dir_st, 4ull * ndir),
                MTBLX_R(bad, ndir), MTBLX_R(sel, 4ull * n), MTBLX_R(w, L.total)),
               k_stage_gather, grid_of(n), dim3(kThreads), 0, s, file_len, blk_off, blk_len, dir_st, bad, ndir, sel, n,
               src_off, src_len, w + L.skip, hdr);
  if (hipGetLastError() != hipSuccess) return MTBLX_E_HIP;
  // the preambles and the 16-byte aligned layout; its totals are hdr[0..2] (it clears them itself,
  // so the skipped count sits behind them)
  const int rc = mtblx_snappy_dir(file, src_off, src_len, n, reinterpret_cast<uint64_t*>(w + L.dst_off),
                                  reinterpret_cast<uint32_t*>(w + L.dst_len), reinterpret_cast<int32_t*>(w + L.status),
                                  hdr, w + L.snap, L.total - L.snap, stream);
  if (rc != MTBLX_OK) return rc;
  uint64_t host[4];
  if (hipMemcpyAsync(host, hdr, sizeof host, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return MTBLX_E_HIP;
  totals[0] = host[0];
  totals[1] = host[1];
  totals[2] = host[2] - host[3];   // a skipped entry has no stored bytes: not a corrupt preamble
  return MTBLX_OK;
}

extern "C" int mtblx_stage_emit(const uint8_t* file, uint64_t file_len, const uint64_t* blk_off, uint32_t ndir,
                                const uint32_t* sel, uint32_t nsel, uint8_t* dst, uint64_t dst_cap, uint64_t base,
                                uint64_t total, uint32_t max_dec_len, uint64_t* dst_off, uint32_t* dec_len,
                                uint64_t* tab_start, uint64_t* tab_doff, uint64_t* tab_dlen, int32_t* tab_st,
                                int by_ordinal, const void* workspace, size_t ws_bytes, void* stream) {
  const uint32_t n = sel ? nsel : ndir;
  if (n == 0) return MTBLX_OK;
  if (!file || !blk_off || !dst || !workspace || ((uintptr_t)workspace & 255u)) return MTBLX_E_INVAL;
  if ((base & 15u) || base > dst_cap || total > dst_cap - base) return MTBLX_E_INVAL;
  if (tab_start && (!tab_doff || !tab_dlen || !tab_st)) return MTBLX_E_INVAL;
  const Layout L = layout(n);
  if (ws_bytes < L.total) return MTBLX_E_INVAL;
  (void)file_len;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  uint8_t* w = const_cast<uint8_t*>(static_cast<const uint8_t*>(workspace));
  const uint64_t* ws_off = reinterpret_cast<const uint64_t*>(w + L.dst_off);
  uint32_t* ws_dec = reinterpret_cast<uint32_t*>(w + L.dec_len);
  int32_t* ws_st = reinterpret_cast<int32_t*>(w + L.status);
  const int rc = mtblx_snappy_decompress_dev(file, reinterpret_cast<const uint64_t*>(w + L.src_off),
                                             reinterpret_cast<const uint32_t*>(w + L.src_len), n, dst + base, ws_off,
                                             reinterpret_cast<const uint32_t*>(w + L.dst_len), max_dec_len, ws_st, ws_dec,
                                             stream);
  if (rc != MTBLX_OK) return rc;
  const uint64_t nrow = by_ordinal ? ndir : n;
  (void)nrow;   // read by the bounds-checked build only
  MTBLX_LAUNCH((MTBLX_R(blk_off, 8ull * ndir), MTBLX_R(sel, 4ull * n), MTBLX_R(w, L.total), MTBLX_R(dst_off, 8ull * n),
                MTBLX_R(dec_len, 4ull * n), MTBLX_R(tab_start, 8ull * nrow), MTBLX_R(tab_doff, 8ull * nrow),
                MTBLX_R(tab_dlen, 8ull * nrow), MTBLX_R(tab_st, 4ull * nrow)),
               k_stage_finish, grid_of(n), dim3(kThreads), 0, s, blk_off, ndir, sel, n, base, ws_off, ws_dec, ws_st,
               w + L.skip, dst_off, dec_len, tab_start, tab_doff, tab_dlen, tab_st, by_ordinal);
  return hipGetLastError() == hipSuccess ? MTBLX_OK : MTBLX_E_HIP;
}

extern "C" int mtblx_scan_touch(const uint8_t* file, uint64_t file_len, uint64_t index_off, uint64_t index_len,
                                const uint64_t* entry_off, uint32_t nent, const uint8_t* keys, const uint64_t* key_end,
                                const uint8_t* keys2, const uint64_t* key2_end, const uint32_t* cap, uint32_t cap_all,
                                uint32_t nq, uint32_t* want, uint32_t nwords, void* stream) {
  if (nq == 0 || nent == 0) return MTBLX_OK;
  if (!file || !entry_off || !keys || !key_end || !want || (key2_end && !keys2)) return MTBLX_E_INVAL;
  if (index_off > file_len || index_len > file_len - index_off) return MTBLX_E_INVAL;
  if ((uint64_t)nwords * 32u < nent) return MTBLX_E_INVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  MTBLX_LAUNCH((MTBLX_R(file, file_len), MTBLX_R(entry_off, 8ull * nent), keys, MTBLX_R(key_end, 8ull * nq), keys2,
                MTBLX_R(key2_end, 8ull * nq), MTBLX_R(cap, 4ull * nq), MTBLX_R(want, 4ull * nwords)),
               k_scan_touch, grid_of(nq), dim3(kThreads), 0, s, file + index_off, index_len, entry_off, nent, keys,
               key_end, keys2, key2_end, cap, cap_all, nq, want, nwords);
  return hipGetLastError() == hipSuccess ? MTBLX_OK : MTBLX_E_HIP;
}

extern "C" int mtblx_bitmap_compact(const uint32_t* bits, const uint32_t* exclude, uint32_t nbits, uint32_t* list,
                                    uint32_t list_cap, uint32_t* count, void* stream) {
  if (!count || (nbits && !bits) || (list_cap && !list)) return MTBLX_E_INVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint64_t nwords = ((uint64_t)nbits + 31u) / 32u;
  (void)nwords;   // read by the bounds-checked build only
  MTBLX_LAUNCH((MTBLX_R(bits, 4ull * nwords), MTBLX_R(exclude, 4ull * nwords), MTBLX_R(list, 4ull * list_cap),
                MTBLX_R(count, 4)),
               k_bitmap_compact, dim3(1), dim3(1024), 0, s, bits, exclude, nbits, list, list_cap, count);
  return hipGetLastError() == hipSuccess ? MTBLX_OK : MTBLX_E_HIP;
}

extern "C" int mtblx_table_gather(const uint32_t* list, uint32_t n, uint32_t nrow, const uint64_t* blk_off,
                                  const uint64_t* row_doff, const uint64_t* row_dlen, const int32_t* row_st,
                                  uint64_t* tab_start, uint64_t* tab_doff, uint64_t* tab_dlen, int32_t* tab_st,
                                  void* stream) {
  if (n == 0) return MTBLX_OK;
  if (!list || !blk_off || !row_doff || !row_dlen || !row_st || !tab_start || !tab_doff || !tab_dlen || !tab_st)
    return MTBLX_E_INVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  MTBLX_LAUNCH((MTBLX_R(list, 4ull * n), MTBLX_R(blk_off, 8ull * nrow), MTBLX_R(row_doff, 8ull * nrow),
                MTBLX_R(row_dlen, 8ull * nrow), MTBLX_R(row_st, 4ull * nrow), MTBLX_R(tab_start, 8ull * n),
                MTBLX_R(tab_doff, 8ull * n), MTBLX_R(tab_dlen, 8ull * n), MTBLX_R(tab_st, 4ull * n)),
               k_table_gather, grid_of(n), dim3(kThreads), 0, s, list, n, nrow, blk_off, row_doff, row_dlen, row_st,
               tab_start, tab_doff, tab_dlen, tab_st);
  return hipGetLastError() == hipSuccess ? MTBLX_OK : MTBLX_E_HIP;
}

extern "C" int mtblx_dir_ascends(const uint64_t* blk_off, const int32_t* dir_st, uint32_t ndir, uint32_t* violations,
                                 void* stream) {
  if (!violations || (ndir && (!blk_off || !dir_st))) return MTBLX_E_INVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (hipMemsetAsync(violations, 0, 4, s) != hipSuccess) return MTBLX_E_HIP;
  if (ndir == 0) return MTBLX_OK;
  MTBLX_LAUNCH((MTBLX_R(blk_off, 8ull * ndir), MTBLX_R(dir_st, 4ull * ndir), MTBLX_R(violations, 4)), k_dir_ascends,
               grid_of(ndir), dim3(kThreads), 0, s, blk_off, dir_st, ndir, violations);
  return hipGetLastError() == hipSuccess ? MTBLX_OK : MTBLX_E_HIP;
}

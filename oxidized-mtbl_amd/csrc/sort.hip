// sort.hip — the crate's Sorter::write_chunk on the device (reference src/sorter.rs:142-197): one
// batch of records in any order, duplicate and empty keys allowed, becomes what write_chunk writes
// for it: keys ascending by Vec<u8>::cmp, one item per distinct key.
//
// Nothing but 16-byte handles moves until the end (DESIGN.md §4 "The Sorter"):
//   k_sort_skip     the bytes every key shares.  The merge reads two keys for this (its sources are
//                   sorted); here nothing is sorted, so it is the minimum over all records of the
//                   common-prefix length with record 0's key: one grid-stride pass, each thread
//                   bounded by the minimum published so far, one atomicMin per thread that lowers it
//   k_sort_tile     a workgroup builds kSortTile handles {prefix, 0, index} straight into LDS
//                   (prefix = the big-endian image of the 8 key bytes after the shared ones, zero
//                   padded, as k_merge_build), sorts them there with a bitonic network and writes
//                   them out as one sorted run.  The order is the merge's total order (key, source,
//                   index) with source 0 everywhere, so the unstable network gives the stable
//                   result; prefix ties are settled from global memory (h_keycmp).  A partial tile
//                   is padded to a power of two with sentinels, which the comparator recognises by
//                   their index field BEFORE it looks at any key: a sentinel never reaches key_of
//   k_merge_pass<TileRuns>   ceil(log2 tiles) launches of the Merger's pass over uniform runs of
//                   kSortTile << level handles clipped at n; an unpaired last run is merged with an
//                   empty one, i.e. copied
//   k_group_flags<false>, k_group_*, k_merge_emit   the Merger's grouping and gather, without the
//                   empty-key quirk: write_chunk keeps its current key in an Option (:154-188)
//
// Promised on top of the reference (sort_unstable_by, :152): the values of a key come out in input
// order.  The bounds-checked build (bounds.h) checks the accesses to the workspace and the outputs.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "mtblx.h"
#include "bounds.h"
#include "devinfo.h"
#include "merge_dev.h"
#include "reduce_dev.h"

namespace {

constexpr uint32_t kSentinel = 0xFFFFFFFFu;   // no record has this index: n < MTBLX_MERGE_MAX_RECORDS = 2^32 - 16

// common-prefix length of a and b, looking at no more than lim bytes (lim <= both lengths)
__device__ __forceinline__ uint64_t common_prefix(const uint8_t* a, const uint8_t* b, uint64_t lim) {
  uint64_t k = 0;
  for (; k + 8 <= lim; k += 8) {
    const uint64_t x = *reinterpret_cast<const u64u*>(a + k), y = *reinterpret_cast<const u64u*>(b + k);
    if (x != y) return k + ((uint64_t)__builtin_ctzll(x ^ y) >> 3);   // little endian: the lowest address first
  }
  for (; k < lim; ++k)
    if (a[k] != b[k]) break;
  return k;
}

// hdr[H_SKIP] starts at UINT64_MAX (the plan sets it) and ends at the minimum: record 0 itself
// brings it down to its own length
__global__ void __launch_bounds__(kThreads) k_sort_skip(SrcTab t, uint64_t* hdr, uint32_t n) {
  unsigned long long* w = reinterpret_cast<unsigned long long*>(hdr + H_SKIP);
  const Key k0 = key_of(t, 0, 0);
  const uint64_t seen = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  uint64_t m = seen < k0.len ? seen : k0.len;
  const uint64_t stride = (uint64_t)gridDim.x * kThreads;
  for (uint64_t r = (uint64_t)blockIdx.x * kThreads + threadIdx.x; r < n && m; r += stride) {
    const Key k = key_of(t, 0, (uint32_t)r);
    m = common_prefix(k0.p, k.p, m < k.len ? m : k.len);
  }
  if (m < seen) {
    MTBLX_CHK(w, 8);
    atomicMin(w, (unsigned long long)m);
  }
}

// the total order with the padding last: the index field decides before any key is touched
__device__ __forceinline__ bool sort_less(const SrcTab& t, Handle a, Handle b, uint64_t skip) {
  if (a.idx == kSentinel) return false;
  if (b.idx == kSentinel) return true;
  return h_less(t, a, b, skip);
}

__global__ void __launch_bounds__(kThreads) k_sort_tile(SrcTab t, const uint64_t* hdr, Handle* h0, uint32_t n) {
  __shared__ Handle s[kSortTile];
  const uint64_t skip = hdr[H_SKIP];
  const uint64_t base = (uint64_t)blockIdx.x * kSortTile;
  const uint32_t cnt = (uint32_t)(base + kSortTile < n ? (uint64_t)kSortTile : (uint64_t)n - base);   // grid = ceil(n / tile)
  uint32_t m = 1;   // the network's size: the power of two that holds the tile's records
  while (m < cnt) m <<= 1;
  for (uint32_t k = threadIdx.x; k < m; k += kThreads) {
    Handle h{~0ull, kSentinel, kSentinel};
    if (k < cnt) {
      const uint32_t r = (uint32_t)(base + k);
      const Key key = key_of(t, 0, r);
      uint64_t p = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) p = (p << 8) | (skip + j < key.len ? (uint64_t)key.p[skip + j] : 0ull);
      h = Handle{p, 0u, r};
    }
    s[k] = h;
  }
  __syncthreads();
  for (uint32_t k = 2; k <= m; k <<= 1) {
    for (uint32_t j = k >> 1; j; j >>= 1) {
      for (uint32_t q = threadIdx.x; q < (m >> 1); q += kThreads) {
        const uint32_t i = ((q & ~(j - 1u)) << 1) | (q & (j - 1u)), p = i | j;   // i has bit j clear, p = i + j < m
        const bool up = (i & k) == 0;
        const Handle a = s[i], b = s[p];
        if (up ? sort_less(t, b, a, skip) : sort_less(t, a, b, skip)) {
          s[i] = b;
          s[p] = a;
        }
      }
      __syncthreads();
    }
  }
  for (uint32_t k = threadIdx.x; k < cnt; k += kThreads) {   // the sentinels sorted behind the cnt records
    MTBLX_CHK(h0 + base + k, 16);
    h0[base + k] = s[k];
  }
}

uint32_t sort_tiles(uint64_t n) { return (uint32_t)((n + kSortTile - 1) / kSortTile); }
uint32_t sort_passes(uint64_t n) { return passes_for(sort_tiles(n)); }
uint64_t sort_mark(uint64_t n) { return kSortMagic ^ n; }

}  // namespace

extern "C" size_t mtblx_sort_impl_ws_bytes(uint64_t nrec) { return layout(nrec).total; }
extern "C" uint64_t mtblx_grid_items_sort_skip(void) { return build_grid_cap() * kThreads; }

// arguments already checked (mtblx_api.cpp): ws 256-byte aligned and large enough
// phase_ms (diagnostic, may be NULL): HIP-event times of [0] the shared-prefix scan, [1] the tile
// sort (handles built and sorted in LDS), [2 .. passes + 1] the merge passes, [passes + 2] the
// grouping; phase_cap >= passes + 3, passes = ceil(log2 ceil(n / kSortTile))
extern "C" int mtblx_sort_impl_plan(const mtblx_records* in, uint64_t* totals, void* ws, hipStream_t s,
                                    float* phase_ms, uint32_t phase_cap) {
  PhaseEvents ev(phase_ms != nullptr);
  SrcTab t;
  const uint64_t n64 = fill_tab(in, 1, &t);
  if (n64 == UINT64_MAX) return MTBLX_E_INVAL;
  const uint32_t n = (uint32_t)n64;
  const uint32_t np = sort_passes(n);
  if (phase_ms && phase_cap < np + 3) return MTBLX_E_INVAL;
  const Layout L = layout(n);
  uint8_t* w = static_cast<uint8_t*>(ws);
  uint64_t* hdr = reinterpret_cast<uint64_t*>(w + L.hdr);
  Handle* hb[2] = {reinterpret_cast<Handle*>(w + L.h0), reinterpret_cast<Handle*>(w + L.h1)};
  uint8_t* flag = w + L.flag;
  uint64_t* tiles = reinterpret_cast<uint64_t*>(w + L.tiles);
  uint64_t host[H_WORDS];
  if (hipMemsetAsync(hdr, 0, 8 * H_WORDS, s) != hipSuccess ||
      hipMemsetAsync(hdr + H_SKIP, 0xFF, 8, s) != hipSuccess)   // the atomicMin of k_sort_skip starts from the top
    return MTBLX_E_HIP;
  const dim3 b(kThreads);
  const Handle* hf = hb[np & 1];
  ev.mark(s);
  if (n) {
    const uint64_t want = ((uint64_t)n + kThreads - 1) / kThreads, cap = build_grid_cap();
    MTBLX_LAUNCH((MTBLX_R(w, L.total)), k_sort_skip, dim3((unsigned)(want < cap ? want : cap)), b, 0, s, t, hdr, n);
    ev.mark(s);
    MTBLX_LAUNCH((MTBLX_R(w, L.total)), k_sort_tile, dim3(sort_tiles(n)), b, 0, s, t, hdr, hb[0], n);
    ev.mark(s);
    for (uint32_t p = 0; p < np; ++p) {
      MTBLX_LAUNCH((MTBLX_R(w, L.total)), k_merge_pass<TileRuns>, dim3(L.ntiles), b, 0, s, t, hdr, hb[p & 1],
                   hb[(p + 1) & 1], n, p);
      ev.mark(s);
    }
    MTBLX_LAUNCH((MTBLX_R(w, L.total)), k_group_flags<false>, dim3((unsigned)want), b, 0, s, t, hdr, hf, flag, n);
    MTBLX_LAUNCH((MTBLX_R(w, L.total)), k_group_sums, dim3(L.ntiles), b, 0, s, t, hf, flag, tiles, n);
  }
  MTBLX_LAUNCH((MTBLX_R(w, L.total)), k_group_scan, dim3(1), b, 0, s, hdr, tiles, L.ntiles, n, sort_mark(n),
               nullptr);
  if (n) {
    MTBLX_LAUNCH((MTBLX_R(w, L.total)), k_group_apply, dim3(L.ntiles), b, 0, s, t, hf, flag, tiles, group_out(w, L), n);
  }
  ev.mark(s);
  if (hipGetLastError() != hipSuccess) return MTBLX_E_HIP;
  if (hipMemcpyAsync(host, hdr, 8 * H_WORDS, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return MTBLX_E_HIP;
  if (phase_ms) ev.read(phase_ms, phase_cap);
  for (int i = 0; i < 6; ++i) totals[i] = host[i];
  if (host[H_FLAGS] & MTBLX_MERGE_INTERNAL) return MTBLX_E_HIP;
  return MTBLX_OK;
}

// which of the two handle arrays holds the sorted handles follows from n alone (sort_passes)
extern "C" int mtblx_sort_impl_emit(const mtblx_records* in, int mode, const mtblx_merged* out, const void* ws,
                                    hipStream_t s) {
  SrcTab t;
  const uint64_t n64 = fill_tab(in, 1, &t);
  if (n64 == UINT64_MAX) return MTBLX_E_INVAL;
  const uint32_t n = (uint32_t)n64;
  const Layout L = layout(n);
  uint8_t* w = const_cast<uint8_t*>(static_cast<const uint8_t*>(ws));
  if (hipMemsetAsync(out->flags, 0, 4, s) != hipSuccess) return MTBLX_E_HIP;
  const Handle* hf = reinterpret_cast<const Handle*>(w + (sort_passes(n) & 1 ? L.h1 : L.h0));
  MTBLX_LAUNCH((MTBLX_R(w, L.total), MTBLX_R(out->keys, out->keys_cap), MTBLX_R(out->key_end, out->key_end_cap),
                MTBLX_R(out->vals, out->vals_cap), MTBLX_R(out->val_end, out->val_end_cap),
                MTBLX_R(out->grp_end, out->grp_end_cap), MTBLX_R(out->flags, 4)),
               k_merge_emit, dim3(n ? (unsigned)(((uint64_t)n + kEmitTile - 1) / kEmitTile) : 1u), dim3(kThreads), 0, s, t,
               reinterpret_cast<const uint64_t*>(w + L.hdr), hf, w + L.flag, group_out(w, L), *out, mode, n,
               sort_mark(n));
  return hipGetLastError() == hipSuccess ? MTBLX_OK : MTBLX_E_HIP;
}

// a reduce spec as the merge function (reduce_dev.h, reduce_emit): u64le fields in MTBLX_MERGE_FIRST's
// layout, or varint-coded fields in a layout of their own.  The workspace's per-tile arrays are written
extern "C" int mtblx_sort_impl_emit_reduce(const mtblx_records* in, const mtblx_reduce* spec, const mtblx_merged* out,
                                           void* ws, hipStream_t s) {
  RSpec sp;
  bool varint;
  if (!reduce_spec(spec, &sp, &varint)) return MTBLX_E_INVAL;
  SrcTab t;
  const uint64_t n64 = fill_tab(in, 1, &t);
  if (n64 == UINT64_MAX) return MTBLX_E_INVAL;
  const uint32_t n = (uint32_t)n64;
  const Layout L = layout(n);
  uint8_t* w = static_cast<uint8_t*>(ws);
  if (hipMemsetAsync(out->flags, 0, 4, s) != hipSuccess) return MTBLX_E_HIP;
  const Handle* hf = reinterpret_cast<const Handle*>(w + (sort_passes(n) & 1 ? L.h1 : L.h0));
  reduce_emit(t, w, L.total, L, hf, *out, sp, varint, spec->nfields, n, sort_mark(n), s);
  return hipGetLastError() == hipSuccess ? MTBLX_OK : MTBLX_E_HIP;
}

// merge.hip — the crate's Merger on the device (reference src/merger.rs): a k-way merge of sorted
// record sources with duplicate keys grouped, as MergerIter / MultiIter yield them (:172-260).
//
// Nothing but 16-byte handles moves until the end (DESIGN.md §4 "The Merger"):
//   k_merge_prefix  the bytes every key shares = the common prefix of the smallest first key and
//                   the largest last key (the sources are sorted)
//   k_merge_build   one handle per record {u64 prefix, u32 source, u32 index}: prefix = the
//                   big-endian image of the 8 key bytes after the shared ones, zero padded; the
//                   same kernel checks each source's order (a key <= its predecessor sets
//                   MTBLX_MERGE_UNSORTED).  The check comes BEFORE the merge passes: a merge-path
//                   split over an unsorted run is not monotone, so a pass must never see one
//   k_merge_pass<SrcRuns>   ceil(log2 nsrc) launches, run 2j merged with run 2j+1, an unpaired run
//                   carried over; the run boundaries come from the source table
//   k_group_flags<true>, k_group_*   head flags, the empty-key quirk, six running sums
//   k_group_select  (mtblx_merge_plan_select only) between the flags and the sums: the groups whose
//                   source mask fails the rule are flagged out, and everything after works on the rest
//   k_merge_emit    16 lanes per record gather the group's key once and the mode's values
// The last three, with the handle and its order, are shared with the Sorter (sort.hip) and live in
// merge_dev.h, which describes them.
//
// Order: keys compare as unsigned bytes then by length (Vec<u8>::cmp); equal keys by source number,
// which no pass ever reorders (run 2j holds lower source numbers than run 2j+1): the values of a
// group come out in source order.  Every pass is its own launch: no workgroup waits for another.
//
// The bounds-checked build (bounds.h) checks the accesses to the workspace and the outputs; the
// source arrays (4 pointers x 64 sources) do not fit its 24-range table and are not declared.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "mtblx.h"
#include "bounds.h"
#include "devinfo.h"
#include "merge_dev.h"   // Handle, the order, k_merge_pass, k_group_*, k_merge_emit, layout(): shared with sort.hip
#include "reduce_dev.h"  // k_reduce_tile, k_reduce_edges: the device merge functions, shared with sort.hip

namespace {

__global__ void __launch_bounds__(64) k_merge_prefix(SrcTab t, uint64_t* hdr) {
  if (threadIdx.x || blockIdx.x) return;
  // the sources holding the smallest first key and the largest last key, by their numbers (nsrc:
  // none yet); the two keys are read again from the table once the sources are known.
  // Deliberately NOT two Key structs updated in the loop ("if (!have || key_cmp(f, mn, 0) < 0) mn = f;"):
  // that form was compiled for gfx950 into code that assigned mn.p on the first source's path only
  // ("Looping launches"; regression: tests/test_grid_wrap_gpu.py::test_merge_records)
  uint32_t smin = t.nsrc, smax = t.nsrc;
  for (uint32_t s = 0; s < t.nsrc; ++s) {
    const uint32_t n = t.base[s + 1] - t.base[s];
    if (!n) continue;
    if (smin == t.nsrc) {
      smin = smax = s;
      continue;
    }
    if (key_cmp(key_of(t, s, 0), key_of(t, smin, 0), 0) < 0) smin = s;
    if (key_cmp(key_of(t, s, n - 1), key_of(t, smax, t.base[smax + 1] - t.base[smax] - 1), 0) > 0) smax = s;
  }
  uint64_t skip = 0;
  if (smin != t.nsrc) {
    const Key mn = key_of(t, smin, 0), mx = key_of(t, smax, t.base[smax + 1] - t.base[smax] - 1);
    const uint64_t m = mn.len < mx.len ? mn.len : mx.len;
    while (skip < m && mn.p[skip] == mx.p[skip]) ++skip;
  }
  MTBLX_CHK(hdr + H_SKIP, 8);
  hdr[H_SKIP] = skip;
}

__global__ void __launch_bounds__(kThreads) k_merge_build(SrcTab t, uint64_t* hdr, Handle* h0, uint32_t n) {
  const uint64_t skip = hdr[H_SKIP];
  const uint64_t stride = (uint64_t)gridDim.x * kThreads;
  for (uint64_t r = (uint64_t)blockIdx.x * kThreads + threadIdx.x; r < n; r += stride) {
    uint32_t lo = 0, hi = t.nsrc;   // the last source with base <= r (empty sources share a base)
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) / 2;
      if (t.base[mid] <= r) lo = mid; else hi = mid;
    }
    const uint32_t idx = (uint32_t)r - t.base[lo];
    const Key k = key_of(t, lo, idx);
    uint64_t p = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) p = (p << 8) | (skip + j < k.len ? (uint64_t)k.p[skip + j] : 0ull);
    if (idx && key_cmp(key_of(t, lo, idx - 1), k, 0) >= 0) atomicOr((unsigned long long*)(hdr + H_FLAGS), 1ull);
    MTBLX_CHK(h0 + r, 16);
    h0[r] = Handle{p, lo, idx};
  }
}

uint64_t planned_mark(uint64_t n, uint32_t nsrc) { return kMagic ^ n ^ ((uint64_t)nsrc << 40); }

}  // namespace

extern "C" size_t mtblx_merge_impl_ws_bytes(uint64_t nrec) { return layout(nrec).total; }

// the argument check of the two *_plan_select calls (mtblx_api.cpp): needs no device
extern "C" int mtblx_merge_impl_select_ok(const mtblx_select* sel, uint32_t nsrc) {
  mtblx_select rule;
  return select_rule(sel, nsrc, &rule) ? 1 : 0;
}

// arguments already checked (mtblx_api.cpp): ws 256-byte aligned and large enough, nsrc <= 64
// phase_ms (diagnostic, may be NULL): HIP-event times of [0] the handle build (prefix, handles, order
// check), [1 .. passes] the merge passes, [passes + 1] the grouping; phase_cap >= passes + 2
extern "C" uint64_t mtblx_grid_items_merge_build(void) { return build_grid_cap() * kThreads; }

// sel (may be NULL: no selection, totals is 6 words): the rule of mtblx_merge_plan_select, totals 8 words
extern "C" int mtblx_merge_impl_plan(const mtblx_records* src, uint32_t nsrc, const mtblx_select* sel,
                                     uint64_t* totals, void* ws, hipStream_t s, float* phase_ms,
                                     uint32_t phase_cap) {
  PhaseEvents ev(phase_ms != nullptr);
  if (phase_ms && phase_cap < passes_for(nsrc) + 2) return MTBLX_E_INVAL;
  mtblx_select rule{};
  if (sel && !select_rule(sel, nsrc, &rule)) return MTBLX_E_INVAL;
  const int nt = sel ? 8 : 6;
  SrcTab t;
  const uint64_t n64 = fill_tab(src, nsrc, &t);
  if (n64 == UINT64_MAX) return MTBLX_E_INVAL;
  const uint32_t n = (uint32_t)n64;
  const Layout L = layout(n);
  uint8_t* w = static_cast<uint8_t*>(ws);
  uint64_t* hdr = reinterpret_cast<uint64_t*>(w + L.hdr);
  Handle* hb[2] = {reinterpret_cast<Handle*>(w + L.h0), reinterpret_cast<Handle*>(w + L.h1)};
  uint8_t* flag = w + L.flag;
  uint64_t* tiles = reinterpret_cast<uint64_t*>(w + L.tiles);
  uint64_t host[H_WORDS];
  if (hipMemsetAsync(hdr, 0, 8 * H_WORDS, s) != hipSuccess) return MTBLX_E_HIP;
  const dim3 b(kThreads);
  ev.mark(s);
  if (n) {
    const uint64_t want = ((uint64_t)n + kThreads - 1) / kThreads, cap = build_grid_cap();
    MTBLX_LAUNCH((MTBLX_R(w, L.total)), k_merge_prefix, dim3(1), dim3(64), 0, s, t, hdr);
    MTBLX_LAUNCH((MTBLX_R(w, L.total)), k_merge_build, dim3((unsigned)(want < cap ? want : cap)), b, 0, s, t, hdr,
                 hb[0], n);
    // the order check gates the passes (see the head of this file)
    if (hipMemcpyAsync(host, hdr, 8 * H_WORDS, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      return MTBLX_E_HIP;
    if (host[H_FLAGS] & MTBLX_MERGE_UNSORTED) {
      memset(totals, 0, nt * sizeof(uint64_t));
      totals[5] = host[H_FLAGS];
      return MTBLX_E_FORMAT;
    }
    const uint32_t np = passes_for(nsrc);
    ev.mark(s);
    for (uint32_t p = 0; p < np; ++p) {
      MTBLX_LAUNCH((MTBLX_R(w, L.total)), k_merge_pass<SrcRuns>, dim3(L.ntiles), b, 0, s, t, hdr, hb[p & 1], hb[(p + 1) & 1], n,
                   p);
      ev.mark(s);
    }
    const Handle* hf = hb[np & 1];
    // with a selection the flags go to the gi array first (unwritten until k_group_apply) and
    // k_group_select reads them there: its workgroups read their neighbours' records
    uint8_t* fin = sel ? w + L.gi : flag;
    MTBLX_LAUNCH((MTBLX_R(w, L.total)), k_group_flags<true>, dim3((unsigned)want), b, 0, s, t, hdr, hf, fin, n);
    if (sel) MTBLX_LAUNCH((MTBLX_R(w, L.total)), k_group_select, dim3(L.ntiles), b, 0, s, hf, fin, flag,
                          reinterpret_cast<uint64_t*>(w + L.edges), n, rule);
    MTBLX_LAUNCH((MTBLX_R(w, L.total)), k_group_sums, dim3(L.ntiles), b, 0, s, t, hf, flag, tiles, n);
  }
  MTBLX_LAUNCH((MTBLX_R(w, L.total)), k_group_scan, dim3(1), b, 0, s, hdr, tiles, L.ntiles, n, planned_mark(n, nsrc),
               sel && n ? reinterpret_cast<const uint64_t*>(w + L.edges) : nullptr);
  if (n) {
    MTBLX_LAUNCH((MTBLX_R(w, L.total)), k_group_apply, dim3(L.ntiles), b, 0, s, t, hb[passes_for(nsrc) & 1], flag,
                 tiles, group_out(w, L), n);
  }
  ev.mark(s);
  if (hipGetLastError() != hipSuccess) return MTBLX_E_HIP;
  if (hipMemcpyAsync(host, hdr, 8 * H_WORDS, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return MTBLX_E_HIP;
  if (phase_ms) ev.read(phase_ms, phase_cap);
  for (int i = 0; i < 6; ++i) totals[i] = host[i];
  if (sel) {
    totals[6] = host[H_SELGROUPS];
    totals[7] = host[H_SELRECS];
  }
  if (host[H_FLAGS] & MTBLX_MERGE_UNSORTED) return MTBLX_E_FORMAT;
  if (host[H_FLAGS] & MTBLX_MERGE_INTERNAL) return MTBLX_E_HIP;
  return MTBLX_OK;
}

extern "C" int mtblx_merge_impl_emit(const mtblx_records* src, uint32_t nsrc, int mode, const mtblx_merged* out,
                                     const void* ws, hipStream_t s) {
  SrcTab t;
  const uint64_t n64 = fill_tab(src, nsrc, &t);
  if (n64 == UINT64_MAX) return MTBLX_E_INVAL;
  const uint32_t n = (uint32_t)n64;
  const Layout L = layout(n);
  uint8_t* w = const_cast<uint8_t*>(static_cast<const uint8_t*>(ws));
  if (hipMemsetAsync(out->flags, 0, 4, s) != hipSuccess) return MTBLX_E_HIP;
  const Handle* hf = reinterpret_cast<const Handle*>(w + (passes_for(nsrc) & 1 ? L.h1 : L.h0));
  MTBLX_LAUNCH((MTBLX_R(w, L.total), MTBLX_R(out->keys, out->keys_cap), MTBLX_R(out->key_end, out->key_end_cap),
                MTBLX_R(out->vals, out->vals_cap), MTBLX_R(out->val_end, out->val_end_cap),
                MTBLX_R(out->grp_end, out->grp_end_cap), MTBLX_R(out->flags, 4)),
               k_merge_emit, dim3(n ? (unsigned)(((uint64_t)n + kEmitTile - 1) / kEmitTile) : 1u), dim3(kThreads), 0, s, t,
               reinterpret_cast<const uint64_t*>(w + L.hdr), hf, w + L.flag, group_out(w, L), *out, mode, n,
               planned_mark(n, nsrc));
  return hipGetLastError() == hipSuccess ? MTBLX_OK : MTBLX_E_HIP;
}

// a reduce spec as the merge function (reduce_dev.h, reduce_emit): u64le fields in MTBLX_MERGE_FIRST's
// layout, or varint-coded fields in a layout of their own.  The workspace's per-tile arrays are written
extern "C" int mtblx_merge_impl_emit_reduce(const mtblx_records* src, uint32_t nsrc, const mtblx_reduce* spec,
                                            const mtblx_merged* out, void* ws, hipStream_t s) {
  RSpec sp;
  bool varint;
  if (!reduce_spec(spec, &sp, &varint)) return MTBLX_E_INVAL;
  SrcTab t;
  const uint64_t n64 = fill_tab(src, nsrc, &t);
  if (n64 == UINT64_MAX) return MTBLX_E_INVAL;
  const uint32_t n = (uint32_t)n64;
  const Layout L = layout(n);
  uint8_t* w = static_cast<uint8_t*>(ws);
  if (hipMemsetAsync(out->flags, 0, 4, s) != hipSuccess) return MTBLX_E_HIP;
  const Handle* hf = reinterpret_cast<const Handle*>(w + (passes_for(nsrc) & 1 ? L.h1 : L.h0));
  reduce_emit(t, w, L.total, L, hf, *out, sp, varint, spec->nfields, n, planned_mark(n, nsrc), s);
  return hipGetLastError() == hipSuccess ? MTBLX_OK : MTBLX_E_HIP;
}

// merge_seg.hip — the segmented k-way merge: every source is nseg sorted runs back to back
// (segment q of source s = its records [seg_off[s][q], seg_off[s][q + 1])), and segment q of the
// output is the Merger's result over segment q of every source (DESIGN.md §4 "Merged batched
// scans").  The segments are the queries of Reader.scan_batch: they come in any order and may
// overlap, so only the keys INSIDE a segment are ordered.
//
// The handle is merge_dev.h's, with the segment number in the upper 26 bits of `src` (the source
// needs 6).  Order: segment, then key, then source.  A source's handles are one run sorted in that
// order as they stand, so the merge is k_merge_pass<SrcRuns, SegOrder>, ceil(log2 nsrc) launches:
//   k_seg_check   seg_off[s] is 0 = off[0] <= ... <= off[nseg] = n_s, else MTBLX_MERGE_BADSEG; the
//                 kernels below index nothing once that bit is set
//   k_seg_skip    one thread per segment: skip[q] = the bytes every key of the segment shares = the
//                 common prefix of the smallest first key and the largest last key over the sources
//                 (the one global skip of merge.hip is wrong here: the sources are not sorted as a
//                 whole; no skip at all would leave every compare inside a long-prefix query tied on
//                 its 8 prefix bytes)
//   k_seg_build   one handle per record: source by the record bases, segment by a binary search
//                 of seg_off[s], prefix = key bytes [skip[q], skip[q] + 8); a key <= its
//                 predecessor in the same segment sets MTBLX_MERGE_UNSORTED (read back before any
//                 pass: a merge-path split over an unsorted run is not monotone)
//   k_seg_flags   head = the segment or the key differs from the predecessor's; the empty-key
//                 quirk per segment: an empty-key record is kept iff it is the last of its segment
//   k_seg_pos     one thread per segment: the first merged handle of a later segment
//   k_seg_strip   src &= 63: from here on the handles are the Merger's, and k_group_sums / _scan /
//                 _apply, k_merge_emit and the reduce kernels run as they are
//   k_group_select  (mtblx_merge_seg_plan_select only) after k_seg_strip, when the source is back in
//                 0..63: a group never spans a segment, so the Merger's selection runs as it is
//   k_seg_ends    seg_end[q] = the groups before that handle
// No kernel waits for another workgroup: the launches are ordered by the stream.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "mtblx.h"
#include "bounds.h"
#include "devinfo.h"
#include "merge_dev.h"
#include "reduce_dev.h"

namespace {

constexpr uint32_t kSrcBits = 6, kSrcMask = 63u;
static_assert(MTBLX_MERGE_MAX_SOURCES == 1u << kSrcBits, "the source takes the handle's low 6 bits");
static_assert(MTBLX_MERGE_MAX_SEGMENTS <= 1u << (32 - kSrcBits), "the segment takes the other 26");
// the planned mark: n in bits 0..31, nsrc (<= 64) in 32..38, nseg (<= 2^24) in 39..63
static_assert(MTBLX_MERGE_MAX_SEGMENTS <= 1u << 24, "planned_mark packs nseg into 25 bits");
constexpr uint64_t kSegMagic = 0x5345474d58534547ull;

struct SegTab {   // travels in the kernel arguments beside the SrcTab: 64 x 8 B
  const uint64_t* off[MTBLX_MERGE_MAX_SOURCES];
};

__device__ __forceinline__ uint32_t h_seg(Handle h) { return h.src >> kSrcBits; }

// segment, then key (the prefix holds the bytes after the segment's shared ones), then source
struct SegOrder {
  typedef const uint64_t* Ctx;   // skip[nseg]
  static __device__ __forceinline__ Ctx ctx(const uint64_t* hdr) { return hdr + hdr[H_SEGSKIP]; }
  static __device__ __forceinline__ int keycmp(const SrcTab& t, Handle a, Handle b, Ctx skip) {
    if (a.prefix != b.prefix) return a.prefix < b.prefix ? -1 : 1;
    MTBLX_CHK(skip + h_seg(a), 8);
    return key_cmp(key_of(t, a.src & kSrcMask, a.idx), key_of(t, b.src & kSrcMask, b.idx), skip[h_seg(a)] + 8);
  }
  static __device__ __forceinline__ bool less(const SrcTab& t, Handle a, Handle b, Ctx skip) {
    const uint32_t sa = h_seg(a), sb = h_seg(b);
    if (sa != sb) return sa < sb;
    const int c = keycmp(t, a, b, skip);
    if (c) return c < 0;
    if (a.src != b.src) return a.src < b.src;
    return a.idx < b.idx;
  }
};

__global__ void __launch_bounds__(kThreads) k_seg_check(SrcTab t, SegTab g, uint64_t* hdr, uint32_t nseg,
                                                        uint64_t skip_words) {
  const uint64_t q = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (q == 0) {
    MTBLX_CHK(hdr + H_SEGSKIP, 8);
    hdr[H_SEGSKIP] = skip_words;
  }
  if (q > nseg) return;
  bool bad = false;
  for (uint32_t s = 0; s < t.nsrc; ++s) {
    const uint64_t ns = t.base[s + 1] - t.base[s];
    const uint64_t v = g.off[s][q];
    if (q == 0 && v != 0) bad = true;
    if (q == nseg ? v != ns : g.off[s][q + 1] < v) bad = true;
  }
  if (bad) atomicOr((unsigned long long*)(hdr + H_FLAGS), (unsigned long long)MTBLX_MERGE_BADSEG);
}

__global__ void __launch_bounds__(kThreads) k_seg_skip(SrcTab t, SegTab g, const uint64_t* hdr, uint64_t* skip,
                                                       uint32_t nseg) {
  if (hdr[H_FLAGS] & MTBLX_MERGE_BADSEG) return;
  const uint64_t q = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (q >= nseg) return;
  bool have = false;
  Key mn{nullptr, 0}, mx{nullptr, 0};
  for (uint32_t s = 0; s < t.nsrc; ++s) {
    const uint64_t lo = g.off[s][q], hi = g.off[s][q + 1];
    if (hi <= lo) continue;
    const Key f = key_of(t, s, (uint32_t)lo), l = key_of(t, s, (uint32_t)(hi - 1));
    if (!have || key_cmp(f, mn, 0) < 0) mn = f;
    if (!have || key_cmp(l, mx, 0) > 0) mx = l;
    have = true;
  }
  uint64_t k = 0;
  if (have) {
    const uint64_t m = mn.len < mx.len ? mn.len : mx.len;
    while (k < m && mn.p[k] == mx.p[k]) ++k;
  }
  MTBLX_CHK(skip + q, 8);
  skip[q] = k;
}

__global__ void __launch_bounds__(kThreads) k_seg_build(SrcTab t, SegTab g, uint64_t* hdr, const uint64_t* skip,
                                                        Handle* h0, uint32_t n, uint32_t nseg) {
  if (hdr[H_FLAGS] & MTBLX_MERGE_BADSEG) return;
  const uint64_t stride = (uint64_t)gridDim.x * kThreads;
  for (uint64_t r = (uint64_t)blockIdx.x * kThreads + threadIdx.x; r < n; r += stride) {
    uint32_t lo = 0, hi = t.nsrc;   // the last source with base <= r (empty sources share a base)
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) / 2;
      if (t.base[mid] <= r) lo = mid; else hi = mid;
    }
    const uint32_t idx = (uint32_t)r - t.base[lo];
    const uint64_t* off = g.off[lo];
    uint32_t q0 = 0, q1 = nseg;     // the last segment with off <= idx (off[nseg] = n_s > idx; empty segments share an offset)
    while (q1 - q0 > 1) {
      const uint32_t mid = q0 + (q1 - q0) / 2;
      if (off[mid] <= idx) q0 = mid; else q1 = mid;
    }
    const Key k = key_of(t, lo, idx);
    MTBLX_CHK(skip + q0, 8);
    const uint64_t sk = skip[q0];
    uint64_t p = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) p = (p << 8) | (sk + j < k.len ? (uint64_t)k.p[sk + j] : 0ull);
    if (idx > off[q0] && key_cmp(key_of(t, lo, idx - 1), k, 0) >= 0)
      atomicOr((unsigned long long*)(hdr + H_FLAGS), (unsigned long long)MTBLX_MERGE_UNSORTED);
    MTBLX_CHK(h0 + r, 16);
    h0[r] = Handle{p, (q0 << kSrcBits) | lo, idx};
  }
}

// flag[i] as k_group_flags<true> writes it, with "the very last record" read as "the last record of
// its segment" and a segment change always a head
__global__ void __launch_bounds__(kThreads) k_seg_flags(SrcTab t, uint64_t* hdr, const Handle* h, uint8_t* flag,
                                                        uint32_t n) {
  const SegOrder::Ctx skip = SegOrder::ctx(hdr);
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  MTBLX_CHK(h + i, 16);
  const Handle c = h[i];
  const uint64_t klen = key_of(t, c.src & kSrcMask, c.idx).len;
  const bool last = i + 1 == n || h_seg(h[i + 1]) != h_seg(c);
  const bool dropped = klen == 0 && !last;
  bool head = !dropped;
  if (i) {
    const Handle p = h[i - 1];
    if (h_seg(p) != h_seg(c)) {
      if (h_seg(p) > h_seg(c)) atomicOr((unsigned long long*)(hdr + H_FLAGS), (unsigned long long)MTBLX_MERGE_INTERNAL);
    } else if (head && klen) {
      const int o = SegOrder::keycmp(t, p, c, skip);
      head = o != 0;
      if (o > 0 || (o == 0 && (p.src > c.src || (p.src == c.src && p.idx >= c.idx))))
        atomicOr((unsigned long long*)(hdr + H_FLAGS), (unsigned long long)MTBLX_MERGE_UNSORTED);
    }
  }
  // Here a dropped record can FOLLOW a kept one (the previous segment's last), where the Merger's
  // only lead the whole order.  The shared kernels find a group's tail by the next record's head
  // bit, and skip a dropped record before they look at that bit: so a dropped record carries it too
  MTBLX_CHK(flag + i, 1);
  flag[i] = (uint8_t)(dropped ? 3 : head ? 1 : 0);
}

// pos[q] = the first merged handle of a segment after q (n if there is none)
__global__ void __launch_bounds__(kThreads) k_seg_pos(const Handle* h, uint32_t* pos, uint32_t n, uint32_t nseg) {
  const uint64_t q = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (q >= nseg) return;
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    MTBLX_CHK(h + mid, 16);
    if (h_seg(h[mid]) <= q) lo = mid + 1; else hi = mid;
  }
  MTBLX_CHK(pos + q, 4);
  pos[q] = lo;
}

__global__ void __launch_bounds__(kThreads) k_seg_strip(Handle* h, uint32_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  MTBLX_CHK(&h[i].src, 4);
  h[i].src &= kSrcMask;
}

// after k_group_apply: the groups before record p = gi[p] + 1 - (p is a head)
__global__ void __launch_bounds__(kThreads) k_seg_ends(const uint64_t* hdr, const uint32_t* pos, const uint32_t* gi,
                                                       const uint8_t* flag, uint64_t* seg_end, uint32_t n,
                                                       uint32_t nseg) {
  const uint64_t q = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (q >= nseg) return;
  MTBLX_CHK(pos + q, 4);
  const uint32_t p = pos[q];
  uint64_t e = hdr[H_GROUPS];
  if (p < n) {
    MTBLX_CHK(gi + p, 4);
    MTBLX_CHK(flag + p, 1);
    e = (uint32_t)(gi[p] + 1u - ((flag[p] & 3u) == 1u ? 1u : 0u));
  }
  MTBLX_CHK(seg_end + q, 8);
  seg_end[q] = e;
}

struct SegLayout {
  Layout L;
  size_t skip, pos, total;
};

SegLayout seg_layout(uint64_t n, uint32_t nseg) {
  SegLayout S{};
  S.L = layout(n);
  size_t p = S.L.total;
  S.skip = p; p += up256(8ull * nseg);
  S.pos = p; p += up256(4ull * nseg);
  S.total = p;
  return S;
}

uint64_t planned_mark(uint64_t n, uint32_t nsrc, uint32_t nseg) {
  return kSegMagic ^ n ^ ((uint64_t)nsrc << 32) ^ ((uint64_t)nseg << 39);
}

// -> false if a source that has segments to bound comes without its offsets
bool fill_seg(const uint64_t* const* seg_off, uint32_t nsrc, SegTab* g) {
  memset(g, 0, sizeof(*g));
  for (uint32_t i = 0; i < nsrc; ++i) {
    if (!seg_off || !seg_off[i]) return false;
    g->off[i] = seg_off[i];
  }
  return true;
}

// one thread per item; never an empty grid (every kernel checks its index)
unsigned blocks_for(uint64_t items) { return items ? (unsigned)((items + kThreads - 1) / kThreads) : 1u; }

}  // namespace

extern "C" size_t mtblx_merge_seg_impl_ws_bytes(uint64_t nrec, uint32_t nseg) { return seg_layout(nrec, nseg).total; }
extern "C" uint64_t mtblx_grid_items_seg_build(void) { return build_grid_cap() * kThreads; }

// arguments already checked (mtblx_api.cpp): ws 256-byte aligned and large enough, nsrc <= 64,
// nseg <= MTBLX_MERGE_MAX_SEGMENTS, no NULL seg_off entry.  phase_ms (diagnostic, may be NULL):
// [0] the offsets' check, the skips, the handles, [1 .. passes] the merge passes, [passes + 1] the
// grouping and the segment ends; phase_cap >= passes + 2
// sel (may be NULL: no selection, totals is 6 words): the rule of mtblx_merge_seg_plan_select, totals 8 words
extern "C" int mtblx_merge_seg_impl_plan(const mtblx_records* src, const uint64_t* const* seg_off, uint32_t nsrc,
                                         uint32_t nseg, const mtblx_select* sel, uint64_t* totals, uint64_t* seg_end,
                                         void* ws, hipStream_t s, float* phase_ms, uint32_t phase_cap) {
  PhaseEvents ev(phase_ms != nullptr);
  if (phase_ms && phase_cap < passes_for(nsrc) + 2) return MTBLX_E_INVAL;
  mtblx_select rule{};
  if (sel && !select_rule(sel, nsrc, &rule)) return MTBLX_E_INVAL;
  const int nt = sel ? 8 : 6;
  SrcTab t;
  SegTab g;
  const uint64_t n64 = fill_tab(src, nsrc, &t);
  if (n64 == UINT64_MAX || !fill_seg(seg_off, nsrc, &g)) return MTBLX_E_INVAL;
  const uint32_t n = (uint32_t)n64;
  const SegLayout S = seg_layout(n, nseg);
  const Layout& L = S.L;
  uint8_t* w = static_cast<uint8_t*>(ws);
  uint64_t* hdr = reinterpret_cast<uint64_t*>(w + L.hdr);
  Handle* hb[2] = {reinterpret_cast<Handle*>(w + L.h0), reinterpret_cast<Handle*>(w + L.h1)};
  uint8_t* flag = w + L.flag;
  uint64_t* tiles = reinterpret_cast<uint64_t*>(w + L.tiles);
  uint64_t* skip = reinterpret_cast<uint64_t*>(w + S.skip);
  uint32_t* pos = reinterpret_cast<uint32_t*>(w + S.pos);
  const GroupOut go = group_out(w, L);
  uint64_t host[H_WORDS];
  if (hipMemsetAsync(hdr, 0, 8 * H_WORDS, s) != hipSuccess) return MTBLX_E_HIP;
  const dim3 b(kThreads);
  const uint32_t np = passes_for(nsrc);
  Handle* hf = hb[np & 1];
  ev.mark(s);
  if (nsrc) {
    MTBLX_LAUNCH((MTBLX_R(w, S.total)), k_seg_check, dim3(blocks_for((uint64_t)nseg + 1)), b, 0, s, t, g, hdr, nseg,
                 (uint64_t)((S.skip - L.hdr) / 8));
    if (n) {
      const uint64_t want = blocks_for(n), cap = build_grid_cap();
      MTBLX_LAUNCH((MTBLX_R(w, S.total)), k_seg_skip, dim3(blocks_for(nseg)), b, 0, s, t, g, hdr, skip, nseg);
      MTBLX_LAUNCH((MTBLX_R(w, S.total)), k_seg_build, dim3((unsigned)(want < cap ? want : cap)), b, 0, s, t, g, hdr,
                   skip, hb[0], n, nseg);
    }
    // the two input checks gate everything that trusts the handles (see the head of this file)
    if (hipMemcpyAsync(host, hdr, 8 * H_WORDS, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      return MTBLX_E_HIP;
    if (host[H_FLAGS] & (MTBLX_MERGE_BADSEG | MTBLX_MERGE_UNSORTED)) {
      memset(totals, 0, nt * sizeof(uint64_t));
      totals[5] = host[H_FLAGS];
      return MTBLX_E_FORMAT;
    }
  }
  ev.mark(s);
  if (n) {
    for (uint32_t p = 0; p < np; ++p) {
      MTBLX_LAUNCH((MTBLX_R(w, S.total)), (k_merge_pass<SrcRuns, SegOrder>), dim3(L.ntiles), b, 0, s, t, hdr, hb[p & 1],
                   hb[(p + 1) & 1], n, p);
      ev.mark(s);
    }
    // with a selection the flags go to the gi array first (unwritten until k_group_apply) and
    // k_group_select reads them there: its workgroups read their neighbours' records
    uint8_t* fin = sel ? w + L.gi : flag;
    MTBLX_LAUNCH((MTBLX_R(w, S.total)), k_seg_flags, dim3(blocks_for(n)), b, 0, s, t, hdr, hf, fin, n);
    if (nseg) MTBLX_LAUNCH((MTBLX_R(w, S.total)), k_seg_pos, dim3(blocks_for(nseg)), b, 0, s, hf, pos, n, nseg);
    MTBLX_LAUNCH((MTBLX_R(w, S.total)), k_seg_strip, dim3(blocks_for(n)), b, 0, s, hf, n);
    if (sel) MTBLX_LAUNCH((MTBLX_R(w, S.total)), k_group_select, dim3(L.ntiles), b, 0, s, hf, fin, flag,
                          reinterpret_cast<uint64_t*>(w + L.edges), n, rule);
    MTBLX_LAUNCH((MTBLX_R(w, S.total)), k_group_sums, dim3(L.ntiles), b, 0, s, t, hf, flag, tiles, n);
  }
  MTBLX_LAUNCH((MTBLX_R(w, S.total)), k_group_scan, dim3(1), b, 0, s, hdr, tiles, L.ntiles, n,
               planned_mark(n, nsrc, nseg), sel && n ? reinterpret_cast<const uint64_t*>(w + L.edges) : nullptr);
  if (n) {
    MTBLX_LAUNCH((MTBLX_R(w, S.total)), k_group_apply, dim3(L.ntiles), b, 0, s, t, hf, flag, tiles, go, n);
    if (nseg)
      MTBLX_LAUNCH((MTBLX_R(w, S.total), MTBLX_R(seg_end, 8ull * nseg)), k_seg_ends, dim3(blocks_for(nseg)), b, 0, s, hdr,
                   pos, go.gi, flag, seg_end, n, nseg);
  } else if (nseg) {
    if (hipMemsetAsync(seg_end, 0, 8ull * nseg, s) != hipSuccess) return MTBLX_E_HIP;
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

// spec == NULL: the plain emit in `mode`; else the reduce emit (reduce_emit of reduce_dev.h).  The
// handles were stripped by the plan: both read them as the Merger's.
extern "C" int mtblx_merge_seg_impl_emit(const mtblx_records* src, uint32_t nsrc, uint32_t nseg, int mode,
                                         const mtblx_reduce* spec, const mtblx_merged* out, void* ws, hipStream_t s) {
  RSpec sp{};
  bool varint = false;
  if (spec && !reduce_spec(spec, &sp, &varint)) return MTBLX_E_INVAL;
  SrcTab t;
  const uint64_t n64 = fill_tab(src, nsrc, &t);
  if (n64 == UINT64_MAX) return MTBLX_E_INVAL;
  const uint32_t n = (uint32_t)n64;
  const SegLayout S = seg_layout(n, nseg);
  const Layout& L = S.L;
  uint8_t* w = static_cast<uint8_t*>(ws);
  if (hipMemsetAsync(out->flags, 0, 4, s) != hipSuccess) return MTBLX_E_HIP;
  const Handle* hf = reinterpret_cast<const Handle*>(w + (passes_for(nsrc) & 1 ? L.h1 : L.h0));
  const uint64_t mark = planned_mark(n, nsrc, nseg);
  if (spec) {
    reduce_emit(t, w, S.total, L, hf, *out, sp, varint, spec->nfields, n, mark, s);
    return hipGetLastError() == hipSuccess ? MTBLX_OK : MTBLX_E_HIP;
  }
  MTBLX_LAUNCH((MTBLX_R(w, S.total), MTBLX_R(out->keys, out->keys_cap), MTBLX_R(out->key_end, out->key_end_cap),
                MTBLX_R(out->vals, out->vals_cap), MTBLX_R(out->val_end, out->val_end_cap),
                MTBLX_R(out->grp_end, out->grp_end_cap), MTBLX_R(out->flags, 4)),
               k_merge_emit, dim3(n ? (unsigned)(((uint64_t)n + kEmitTile - 1) / kEmitTile) : 1u), dim3(kThreads), 0, s, t,
               reinterpret_cast<const uint64_t*>(w + L.hdr), hf, w + L.flag, group_out(w, L), *out,
               mode, n, mark);
  return hipGetLastError() == hipSuccess ? MTBLX_OK : MTBLX_E_HIP;
}

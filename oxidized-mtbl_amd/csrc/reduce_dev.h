// reduce_dev.h — the device merge functions of the Merger (merge.hip) and the Sorter (sort.hip):
// a reduce spec of 1 to 8 unsigned 64-bit little-endian fields, each summed (mod 2^64), min-ed or
// max-ed over the values of a group (include/mtblx.h "Device merge functions").
//
// The output has MTBLX_MERGE_FIRST's layout, so the emit is k_merge_emit in FIRST mode (keys,
// key_end, every group's first value at foff, val_end: a group of one is finished by it) followed
// by a segmented reduction over the merged handle order that overwrites the W = 8 * F bytes of
// every group of two or more:
//   k_reduce_tile   a workgroup owns kTile consecutive merged records, kPer per thread.  A record
//                   of a group of two or more (not both head and tail) brings its F fields, or,
//                   where its value is not W bytes long, the "bad" bit and MTBLX_MERGE_BADVALUE.  An
//                   inclusive segmented scan keyed on the head flags (thread-serial over kPer
//                   records, __shfl_up inside the wave, LDS across the four waves) leaves the
//                   group's result with its tail; a tail whose head lies in the same tile stores it
//                   at the group's slot.  What crosses the tile's edges goes to the tile's edge
//                   record: the lead partial (the records before the first head; the whole tile if
//                   it has none), the trail partial (from the last head to the tile's end), whether
//                   the tile has a head, whether the trail's group goes on, the trail's head index
//   k_reduce_edges  a wave per tile whose trailing group goes on: its trail combined with the lead
//                   partials of the following tiles up to and including the first with a head (or
//                   the last tile), 64 tiles per step, stored at the head's slot
// The slot of a group of two or more whose values are all W bytes long is [foff[i] - W, foff[i])
// for every record i of it but the head (foff counts first-value bytes of the groups up to and
// including i's once i is past the head).  A group with a bad value is not stored at all: its slot
// keeps the first value k_merge_emit put there, so nothing is written outside a slot.
// No workgroup waits for another: the launches are ordered by the stream.  The ops are
// associative and commutative and the results exact, so no result depends on evaluation order; the
// output slots are unaligned and written with plain (packed) stores, never with atomics.
//
// Varint-coded values (ENC = R_VARINT; include/mtblx.h "Varint-coded values"): a value is F LEB128
// varints back to back and a group's result is as long as its result needs, so the output has a
// layout of its own and the emit (reduce_emit below) is
//   length pass   k_reduce_tile / k_reduce_edges with LEN: the same reduction, and where the u64le
//                 kernels store a result these write the group's encoded length to val_end[group];
//                 a group of one writes its own value's length, a group with a bad value its first
//                 value's (the layout stays defined; MTBLX_MERGE_BADVALUE is set)
//   k_vend_*      the in-place inclusive scan of val_end[0, groups): tile sums, one workgroup over
//                 the tile sums, apply (three launches, a per-tile array in the workspace)
//   store pass    the reduction again; a good group's result is encoded at val_end[group - 1], a
//                 bad group's first value copied there by the one thread that holds the group
//   k_merge_emit  in kEmitSingles mode: keys, key_end, and every group of one copied to its slot
// Every store is checked against the capacities and sets MTBLX_MERGE_OVERFLOW as r_store does;
// val_end entries past val_end_cap are neither written nor scanned nor read.
#pragma once
#include "merge_dev.h"
#include "reduce_ops.h"   // RSpec, the op table, Seg and its join: shared with reduce_seg.hip and scan.hip

namespace {

constexpr int kEdgeWords = kReduceEdgeWords;   // per tile: lead[8], trail[8], meta, lead bad (the layout reserves 8 * kEdgeWords B)
// meta: bit 0 the tile has a head, bit 2 the trail's group goes on past the tile, bit 3 trail bad,
// bits 32.. the record index of the trail's head.  lead bad: a value of another length in the lead
enum { E_LEAD = 0, E_TRAIL = 8, E_META = 16, E_LBAD = 17 };

// the group's W bytes at vals + off, if they fit; -> false on overflow
template <int F>
__device__ __forceinline__ bool r_store(const mtblx_merged& o, uint64_t off, const uint64_t* v) {
  if (off + 8u * F > o.vals_cap) return false;
  MTBLX_CHK(o.vals + off, 8 * F);
#pragma unroll
  for (int f = 0; f < F; ++f) *reinterpret_cast<u64u*>(o.vals + off + 8 * f) = v[f];
  return true;
}

// A varint group of two or more is finished by the one thread that holds its result: g the group,
// hidx its head's record, v the reduced fields, bad: it holds a value that is not F varints.  LEN:
// val_end[g] = the result's encoded length (bad: the first value's).  Else, after the scan of
// val_end: the result encoded (bad: the first value copied) at val_end[g - 1].  -> false on overflow
template <int F, bool LEN>
__device__ __forceinline__ bool r_finish_varint(const SrcTab& t, const Handle* h, const mtblx_merged& o, uint64_t g,
                                                uint32_t hidx, bool bad, const uint64_t* v) {
  const uint8_t* fp = nullptr;
  uint64_t len;
  if (bad) {
    MTBLX_CHK(h + hidx, 16);
    const Handle c = h[hidx];
    uint64_t vs;
    len = val_len(t, c.src, c.idx, &vs);
    fp = t.s[c.src].vals + vs;
  } else {
    len = r_varint_len_all<F>(v);
  }
  if (8 * (g + 1) > o.val_end_cap) return false;
  if (LEN) {
    MTBLX_CHK(o.val_end + g, 8);
    o.val_end[g] = len;
    return true;
  }
  uint64_t off = 0;
  if (g) {
    MTBLX_CHK(o.val_end + g - 1, 8);
    off = o.val_end[g - 1];
  }
  if (off + len > o.vals_cap) return false;
  if (len) MTBLX_CHK(o.vals + off, len);
  if (bad) {
    for (uint64_t j = 0; j < len; ++j) o.vals[off + j] = fp[j];
  } else {
    r_store_varint<F>(o.vals + off, v);
  }
  return true;
}

// ENC = R_U64LE: as described at the head of this file (LEN is false, gidx unused).  ENC = R_VARINT:
// the length pass (LEN) or the store pass of the varint emit; gidx = the group of every record
template <int F, int ENC, bool LEN>
__global__ void __launch_bounds__(kThreads) k_reduce_tile(SrcTab t, const uint64_t* hdr, const Handle* h,
                                                          const uint8_t* flag, const uint64_t* foff,
                                                          const uint32_t* gidx, mtblx_merged o, uint64_t* edges,
                                                          RSpec sp, uint32_t n, uint64_t planned) {
  if (hdr[H_PLANNED] != planned) return;   // k_merge_emit reports it
  __shared__ uint64_t wv[kThreads / 64][F];   // the waves' runs
  __shared__ uint32_t wfl[kThreads / 64], whi[kThreads / 64];
  constexpr uint64_t W = 8u * F;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t tile0 = (uint64_t)blockIdx.x * kTile;
  const uint64_t i0 = tile0 + (uint64_t)threadIdx.x * kPer;
  // st: bit 0 head, bit 1 tail, bit 2 kept (in range and not dropped), bit 3 bad
  uint64_t v[kPer][F];
  uint32_t st[kPer];
  bool anybad = false, over = false;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const uint64_t i = i0 + k;
    st[k] = 0;
#pragma unroll
    for (int f = 0; f < F; ++f) v[k][f] = r_ident(r_op(sp, f));
    if (i >= n) continue;
    MTBLX_CHK(flag + i, 1);
    const uint8_t fl = flag[i];
    if (fl & 2) continue;
    const bool head = fl & 1, tail = i + 1 == n || (flag[i + 1] & 1);
    st[k] = (head ? 1u : 0u) | (tail ? 2u : 0u) | 4u;
    // a group of one: finished by k_merge_emit, whatever its bytes (the varint length pass gives it its length)
    if (head && tail && !(ENC == R_VARINT && LEN)) continue;
    MTBLX_CHK(h + i, 16);
    const Handle c = h[i];
    uint64_t vs;
    const uint64_t vlen = val_len(t, c.src, c.idx, &vs);
    if (head && tail) {
      MTBLX_CHK(gidx + i, 4);
      const uint64_t g = gidx[i];
      if (8 * (g + 1) <= o.val_end_cap) {
        MTBLX_CHK(o.val_end + g, 8);
        o.val_end[g] = vlen;
      } else {
        over = true;
      }
      continue;
    }
    const uint8_t* vp = t.s[c.src].vals + vs;   // any alignment
    bool good;
    if (ENC == R_VARINT) {
      good = r_load_varint<F, false>(vp, vlen, v[k]);
    } else {
      good = vlen == W;
      if (good) {
#pragma unroll
        for (int f = 0; f < F; ++f) v[k][f] = *reinterpret_cast<const u64u*>(vp + 8 * f);
      }
    }
    if (!good) {
      st[k] |= 8u;
      anybad = true;
    }
  }
  if (anybad) atomicOr(o.flags, MTBLX_MERGE_BADVALUE);
  // the thread's run, the wave's inclusive scan of the runs, the waves before this one
  Seg<F> a = seg_ident<F>(sp);
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    if (!(st[k] & 4u)) continue;
    Seg<F> e;
#pragma unroll
    for (int f = 0; f < F; ++f) e.v[f] = v[k][f];
    e.fl = (st[k] & 1u) | ((st[k] & 8u) >> 2);
    e.hidx = (uint32_t)(i0 + k);
    a = seg_join<F>(sp, a, e);
  }
  Seg<F> x = a;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const Seg<F> y = seg_shfl_up<F>(x, s);
    if (lane >= s) x = seg_join<F>(sp, y, x);
  }
  if (lane == 63) {
#pragma unroll
    for (int f = 0; f < F; ++f) wv[w][f] = x.v[f];
    wfl[w] = x.fl;
    whi[w] = x.hidx;
  }
  Seg<F> acc = seg_shfl_up<F>(x, 1);   // the runs of the wave's lanes before this one
  if (lane == 0) acc = seg_ident<F>(sp);
  __syncthreads();
  Seg<F> before = seg_ident<F>(sp);
#pragma unroll
  for (int k = 0; k < kThreads / 64 - 1; ++k)
    if (k < w) {
      Seg<F> y;
#pragma unroll
      for (int f = 0; f < F; ++f) y.v[f] = wv[k][f];
      y.fl = wfl[k];
      y.hidx = whi[k];
      before = seg_join<F>(sp, before, y);
    }
  acc = seg_join<F>(sp, before, acc);   // everything of the tile before this thread's records
  uint64_t* edge = edges + (uint64_t)blockIdx.x * kEdgeWords;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    if (!(st[k] & 4u)) continue;
    const uint64_t i = i0 + k;
    if ((st[k] & 1u) && !(acc.fl & 1u)) {   // the tile's first head: what came before it is the lead
      MTBLX_CHK(edge + E_LEAD, 8 * F);
#pragma unroll
      for (int f = 0; f < F; ++f) edge[E_LEAD + f] = acc.v[f];
      MTBLX_CHK(edge + E_LBAD, 8);
      edge[E_LBAD] = (acc.fl >> 1) & 1u;
    }
    Seg<F> e;
#pragma unroll
    for (int f = 0; f < F; ++f) e.v[f] = v[k][f];
    e.fl = (st[k] & 1u) | ((st[k] & 8u) >> 2);
    e.hidx = (uint32_t)i;
    acc = seg_join<F>(sp, acc, e);
    if (ENC == R_VARINT) {
      if ((st[k] & 3u) == 2u && (acc.fl & 1u)) {   // the tail of a group of two or more, all of it here
        MTBLX_CHK(gidx + i, 4);
        if (!r_finish_varint<F, LEN>(t, h, o, gidx[i], acc.hidx, acc.fl & 2u, acc.v)) over = true;
      }
    } else if ((st[k] & 3u) == 2u && acc.fl == 1u) {   // the tail of a group of two or more, all of it here and good
      MTBLX_CHK(foff + i, 8);
      if (!r_store<F>(o, foff[i] - W, acc.v)) over = true;
    }
  }
  if (over) atomicOr(o.flags, MTBLX_MERGE_OVERFLOW);
  if (threadIdx.x == kThreads - 1) {   // acc: the whole tile (the threads past n bring nothing)
    const uint64_t last = (tile0 + kTile < n ? tile0 + kTile : (uint64_t)n) - 1;
    const bool has = acc.fl & 1u;
    // the next record goes on with the trail's group iff it is a kept non-head.  A record flagged
    // out (bit 1) without the head bit is no member of it: after a selection (k_group_select) the
    // later records of a rejected group can follow the trail's tail across the tile's edge
    const bool open = has && last + 1 < n && !(flag[last + 1] & 3);
    uint32_t m = has ? 1u : 0u;
    if (has) {
      m |= open ? 4u : 0u;
      m |= (acc.fl & 2u) ? 8u : 0u;
      MTBLX_CHK(edge + E_TRAIL, 8 * F);
#pragma unroll
      for (int f = 0; f < F; ++f) edge[E_TRAIL + f] = acc.v[f];
    } else {
      MTBLX_CHK(edge + E_LEAD, 8 * F);
#pragma unroll
      for (int f = 0; f < F; ++f) edge[E_LEAD + f] = acc.v[f];
      MTBLX_CHK(edge + E_LBAD, 8);
      edge[E_LBAD] = (acc.fl >> 1) & 1u;
    }
    MTBLX_CHK(edge + E_META, 8);
    edge[E_META] = (uint64_t)m | ((uint64_t)acc.hidx << 32);
  }
}

template <int F, int ENC, bool LEN>
__global__ void __launch_bounds__(kThreads) k_reduce_edges(SrcTab t, const uint64_t* hdr, const Handle* h,
                                                           const uint64_t* foff, const uint32_t* gidx, mtblx_merged o,
                                                           const uint64_t* edges, RSpec sp, uint32_t ntiles,
                                                           uint64_t planned) {
  if (hdr[H_PLANNED] != planned) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t tile = (uint64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);   // the same for the whole wave
  if (tile >= ntiles) return;
  const uint64_t* mine = edges + tile * kEdgeWords;
  MTBLX_CHK(mine + E_META, 8);
  const uint64_t meta = mine[E_META];
  if ((meta & 5u) != 5u) return;   // no head, or the trail's group ends with the tile
  uint64_t p[F];
  bool bad = meta & 8u;
#pragma unroll
  for (int f = 0; f < F; ++f) p[f] = lane == 0 ? mine[E_TRAIL + f] : r_ident(r_op(sp, f));
  for (uint64_t base = tile + 1; base < ntiles; base += 64) {
    const uint64_t u = base + lane;
    const uint64_t* e = edges + u * kEdgeWords;
    uint64_t m = 0;
    if (u < ntiles) {
      MTBLX_CHK(e + E_META, 8);
      m = e[E_META];
    }
    const unsigned long long heads = __ballot(u < ntiles && (m & 1u));
    const uint32_t first = heads ? (uint32_t)__builtin_ctzll(heads) : 64u;   // the lane whose tile ends the group
    if (u < ntiles && lane <= first) {
      bad = bad || e[E_LBAD];
#pragma unroll
      for (int f = 0; f < F; ++f) p[f] = r_apply(r_op(sp, f), p[f], e[E_LEAD + f]);
    }
    if (heads) break;
  }
#pragma unroll
  for (int s = 32; s; s >>= 1) {
#pragma unroll
    for (int f = 0; f < F; ++f)
      p[f] = r_apply(r_op(sp, f), p[f], (uint64_t)__shfl_xor((unsigned long long)p[f], s, 64));
  }
  const bool anybad = __ballot(bad) != 0;   // the records themselves have set MTBLX_MERGE_BADVALUE
  const uint32_t hidx = (uint32_t)(meta >> 32);
  if (ENC == R_VARINT) {
    if (lane == 0) {
      MTBLX_CHK(gidx + hidx, 4);
      if (!r_finish_varint<F, LEN>(t, h, o, gidx[hidx], hidx, anybad, p)) atomicOr(o.flags, MTBLX_MERGE_OVERFLOW);
    }
    return;
  }
  if (anybad) return;
  if (lane == 0) {
    MTBLX_CHK(foff + hidx, 8);
    if (!r_store<F>(o, foff[hidx], p)) atomicOr(o.flags, MTBLX_MERGE_OVERFLOW);
  }
}

// ---- the varint emit's scan: val_end[0, m) -> its inclusive prefix sums, in place; m = the groups
// val_end can hold.  A workgroup owns kTile entries, kPer per thread; vt = one sum per tile ----
__device__ __forceinline__ uint64_t vend_count(const uint64_t* hdr, const mtblx_merged& o) {
  const uint64_t g = hdr[H_GROUPS], c = o.val_end_cap / 8;
  return g < c ? g : c;
}

__global__ void __launch_bounds__(kThreads) k_vend_sums(const uint64_t* hdr, mtblx_merged o, uint64_t* vt,
                                                        uint64_t planned) {
  if (hdr[H_PLANNED] != planned) return;
  __shared__ uint64_t wsum[kThreads / 64];
  const uint64_t m = vend_count(hdr, o);
  const uint64_t i0 = (uint64_t)blockIdx.x * kTile + (uint64_t)threadIdx.x * kPer;
  uint64_t sum = 0;
#pragma unroll
  for (int k = 0; k < kPer; ++k)
    if (i0 + k < m) {
      MTBLX_CHK(o.val_end + i0 + k, 8);
      sum += o.val_end[i0 + k];
    }
  uint64_t tot;
  (void)block_scan(sum, wsum, &tot);
  if (threadIdx.x == 0) {
    MTBLX_CHK(vt + blockIdx.x, 8);
    vt[blockIdx.x] = tot;
  }
}

// one workgroup: the tile sums -> their exclusive prefixes, in place
__global__ void __launch_bounds__(kThreads) k_vend_scan(const uint64_t* hdr, uint64_t* vt, uint32_t ntiles,
                                                        uint64_t planned) {
  if (hdr[H_PLANNED] != planned) return;
  __shared__ uint64_t wsum[kThreads / 64];
  uint64_t carry = 0;
  for (uint32_t b = 0; b < ntiles; b += kThreads) {
    const uint32_t i = b + threadIdx.x;
    if (i < ntiles) MTBLX_CHK(vt + i, 8);
    const uint64_t v = i < ntiles ? vt[i] : 0;
    uint64_t tot;
    const uint64_t e = block_scan(v, wsum, &tot);
    if (i < ntiles) vt[i] = carry + e;
    carry += tot;
  }
}

__global__ void __launch_bounds__(kThreads) k_vend_apply(const uint64_t* hdr, mtblx_merged o, const uint64_t* vt,
                                                         uint64_t planned) {
  if (hdr[H_PLANNED] != planned) return;
  __shared__ uint64_t wsum[kThreads / 64];
  const uint64_t m = vend_count(hdr, o);
  const uint64_t i0 = (uint64_t)blockIdx.x * kTile + (uint64_t)threadIdx.x * kPer;
  uint64_t x[kPer], sum = 0;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    x[k] = 0;
    if (i0 + k < m) {
      MTBLX_CHK(o.val_end + i0 + k, 8);
      x[k] = o.val_end[i0 + k];
    }
    sum += x[k];
  }
  uint64_t tot;
  MTBLX_CHK(vt + blockIdx.x, 8);
  uint64_t e = block_scan(sum, wsum, &tot) + vt[blockIdx.x];
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    e += x[k];
    if (i0 + k < m) o.val_end[i0 + k] = e;
  }
}

// ---- host side ----
#define MTBLX_REDUCE_RANGES \
  (MTBLX_R(w, wtotal), MTBLX_R(o.vals, o.vals_cap), MTBLX_R(o.val_end, o.val_end_cap), MTBLX_R(o.flags, 4))

template <int F, int ENC, bool LEN>
void reduce_pass(const SrcTab& t, uint8_t* w, size_t wtotal, const Layout& L, const Handle* hf, const mtblx_merged& o,
                 RSpec sp, uint32_t n, uint64_t planned, hipStream_t s) {
  const uint64_t* hdr = reinterpret_cast<const uint64_t*>(w + L.hdr);
  const uint64_t* foff = reinterpret_cast<const uint64_t*>(w + L.foff);
  const uint32_t* gidx = reinterpret_cast<const uint32_t*>(w + L.gi);
  uint64_t* edges = reinterpret_cast<uint64_t*>(w + L.edges);
  MTBLX_LAUNCH(MTBLX_REDUCE_RANGES, (k_reduce_tile<F, ENC, LEN>), dim3(L.ntiles), dim3(kThreads), 0, s, t, hdr, hf,
               w + L.flag, foff, gidx, o, edges, sp, n, planned);
  MTBLX_LAUNCH(MTBLX_REDUCE_RANGES, (k_reduce_edges<F, ENC, LEN>),
               dim3((L.ntiles + kThreads / 64 - 1) / (kThreads / 64)), dim3(kThreads), 0, s, t, hdr, hf, foff, gidx, o,
               edges, sp, L.ntiles, planned);
}

template <int F>
void reduce_launch_f(const SrcTab& t, uint8_t* w, size_t wtotal, const Layout& L, const Handle* hf,
                     const mtblx_merged& o, RSpec sp, bool varint, uint32_t n, uint64_t planned, hipStream_t s) {
  if (!varint) {
    reduce_pass<F, R_U64LE, false>(t, w, wtotal, L, hf, o, sp, n, planned, s);
    return;
  }
  const uint64_t* hdr = reinterpret_cast<const uint64_t*>(w + L.hdr);
  uint64_t* vt = reinterpret_cast<uint64_t*>(w + L.vtiles);
  reduce_pass<F, R_VARINT, true>(t, w, wtotal, L, hf, o, sp, n, planned, s);
  MTBLX_LAUNCH(MTBLX_REDUCE_RANGES, k_vend_sums, dim3(L.ntiles), dim3(kThreads), 0, s, hdr, o, vt, planned);
  MTBLX_LAUNCH(MTBLX_REDUCE_RANGES, k_vend_scan, dim3(1), dim3(kThreads), 0, s, hdr, vt, L.ntiles, planned);
  MTBLX_LAUNCH(MTBLX_REDUCE_RANGES, k_vend_apply, dim3(L.ntiles), dim3(kThreads), 0, s, hdr, o, vt, planned);
  reduce_pass<F, R_VARINT, false>(t, w, wtotal, L, hf, o, sp, n, planned, s);
}

// The reduce emit of the Merger, the Sorter and the segmented merge, on stream s.  u64le: k_merge_emit
// in FIRST mode, then the reduction over the groups of two or more.  varint: the passes at the head
// of this file, k_merge_emit (kEmitSingles) last.  wtotal: the workspace's bytes (bounds build)
void reduce_emit(const SrcTab& t, uint8_t* w, size_t wtotal, const Layout& L, const Handle* hf, const mtblx_merged& o,
                 RSpec sp, bool varint, uint32_t nfields, uint32_t n, uint64_t planned, hipStream_t s) {
  const uint64_t* hdr = reinterpret_cast<const uint64_t*>(w + L.hdr);
  const dim3 eg(n ? (unsigned)(((uint64_t)n + kEmitTile - 1) / kEmitTile) : 1u);
  if (!varint)
    MTBLX_LAUNCH((MTBLX_R(w, wtotal), MTBLX_R(o.keys, o.keys_cap), MTBLX_R(o.key_end, o.key_end_cap),
                  MTBLX_R(o.vals, o.vals_cap), MTBLX_R(o.val_end, o.val_end_cap), MTBLX_R(o.flags, 4)),
                 k_merge_emit, eg, dim3(kThreads), 0, s, t, hdr, hf, w + L.flag, group_out(w, L), o, MTBLX_MERGE_FIRST,
                 n, planned);
  if (n) {
    switch (nfields) {
      case 1: reduce_launch_f<1>(t, w, wtotal, L, hf, o, sp, varint, n, planned, s); break;
      case 2: reduce_launch_f<2>(t, w, wtotal, L, hf, o, sp, varint, n, planned, s); break;
      case 3: reduce_launch_f<3>(t, w, wtotal, L, hf, o, sp, varint, n, planned, s); break;
      case 4: reduce_launch_f<4>(t, w, wtotal, L, hf, o, sp, varint, n, planned, s); break;
      case 5: reduce_launch_f<5>(t, w, wtotal, L, hf, o, sp, varint, n, planned, s); break;
      case 6: reduce_launch_f<6>(t, w, wtotal, L, hf, o, sp, varint, n, planned, s); break;
      case 7: reduce_launch_f<7>(t, w, wtotal, L, hf, o, sp, varint, n, planned, s); break;
      default: reduce_launch_f<8>(t, w, wtotal, L, hf, o, sp, varint, n, planned, s); break;
    }
  }
  if (varint)
    MTBLX_LAUNCH((MTBLX_R(w, wtotal), MTBLX_R(o.keys, o.keys_cap), MTBLX_R(o.key_end, o.key_end_cap),
                  MTBLX_R(o.vals, o.vals_cap), MTBLX_R(o.val_end, o.val_end_cap), MTBLX_R(o.flags, 4)),
                 k_merge_emit, eg, dim3(kThreads), 0, s, t, hdr, hf, w + L.flag, group_out(w, L), o, kEmitSingles, n,
                 planned);
}
#undef MTBLX_REDUCE_RANGES

}  // namespace

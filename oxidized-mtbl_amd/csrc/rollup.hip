// rollup.hip — rollups on the MI355X (gfx950): records grouped by a prefix of their key, and field
// rows encoded as values (include/mtblx.h "Rollups", DESIGN.md §4 "Rollups").
//
// The group key of a key is its first L bytes (MTBLX_GROUP_LENGTH) or the key up to and including
// the count-th occurrence of a delimiter byte (MTBLX_GROUP_DELIM); a key too short for the rule is
// its own group key.  A group is a run of adjacent records with one group key inside one segment.
//
// The plan (mtblx_rollup_plan):
//   k_rollup_segcheck  a thread per entry of seg_off: 0 = off[0] <= ... <= off[nseg] = n, else
//                      MTBLX_ROLLUP_BADSEG in the workspace header and every later kernel returns
//   k_rollup_glen      (delimiter rule) 16 lanes per record walk the key 16 bytes at a time, count the
//                      delimiters with a ballot and keep a running count across the chunks: the
//                      length of the group key -> glen[r].  The length rule needs no pass: its group
//                      key length is min(key length, L), from key_end alone
//   k_rollup_heads     16 lanes per record: r is a head iff r == 0, r starts a segment (a search over
//                      seg_off for the first record of a 16-lane group, advancing from there), its
//                      group key is as long as its predecessor's no more, or a byte differs -> flag[r].
//                      A record reads its predecessor's KEY, never its predecessor's result
//   k_rollup_sums      per tile of kRollTile records: heads, and the group key bytes of the heads
//   k_rollup_scan      one workgroup: the tile sums -> exclusive prefixes in place, the totals
//                      {groups, group key bytes} to the header and to the caller's device words,
//                      the planned mark
// The emit (mtblx_rollup_emit), each kernel gated on the mark, the flag and the capacities:
//   k_rollup_apply     the tile's scan again: head r of group g writes key_end[g] and grp_rec[g]
//   k_rollup_gather    16 lanes per group move its key (copy16 of lane_dev.h)
//   k_rollup_segs      a thread per entry of seg_off: seg_grp[q] = the groups that begin before
//                      record seg_off[q], by a search over grp_rec; grp_rec[groups] = n
// mtblx_reduce_encode: u64le rows are copied; varint rows take k_renc_sums (encoded lengths per
// tile), k_renc_scan (one workgroup) and k_renc_store (the tile's scan again, val_end and the bytes).
// Every kernel is its own launch and no workgroup waits for another.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bounds.h"
#include "lane_dev.h"
#include "mtblx.h"
#include "reduce_ops.h"

namespace {

constexpr int kRollTile = 1024;                  // records per workgroup of the scans, 4 per thread
constexpr int kRollPer = kRollTile / kThreads;
constexpr int kLaneTile = 256;                   // records (groups) per workgroup of the 16-lane kernels
static_assert(kRollPer * kThreads == kRollTile, "tile");
static_assert(kLaneTile == kThreads, "16 groups of 16 lanes, 16 records each");
enum { RH_GROUPS = 0, RH_KEYB, RH_FLAGS, RH_PLANNED, RH_WORDS = 32 };
constexpr uint64_t kRollMagic = 0x4d54424c58524f4cull;
typedef uint64_t lu64u __attribute__((aligned(1)));

struct GSpec {   // a checked mtblx_group
  uint64_t length;
  uint32_t delim, count;
};

// key r = keys[*start, *start + the result); END offsets that step back give an empty key
__device__ __forceinline__ uint64_t key_span(const mtblx_records& rec, uint64_t r, uint64_t* start) {
  uint64_t ks = 0;
  if (r) {
    MTBLX_CHK(rec.key_end + r - 1, 8);
    ks = rec.key_end[r - 1];
  }
  MTBLX_CHK(rec.key_end + r, 8);
  const uint64_t ke = rec.key_end[r];
  *start = ks;
  return ke >= ks ? ke - ks : 0;
}

// the length of record r's group key, klen being its key's length
template <int KIND>
__device__ __forceinline__ uint64_t glen_of(const GSpec& g, const uint64_t* glen, uint64_t r, uint64_t klen) {
  if (KIND == MTBLX_GROUP_LENGTH) return klen < g.length ? klen : g.length;
  MTBLX_CHK(glen + r, 8);
  return glen[r];
}

__global__ void __launch_bounds__(kThreads) k_rollup_segcheck(const uint64_t* seg_off, uint32_t nseg, uint64_t n,
                                                              uint64_t* hdr) {
  const uint64_t q = (uint64_t)blockIdx.x * kThreads + threadIdx.x;   // entries 0 .. nseg
  if (q > nseg) return;
  MTBLX_CHK(seg_off + q, 8);
  const uint64_t a = seg_off[q];
  bool bad = q == 0 && a != 0;
  if (q == nseg) {
    bad = bad || a != n;
  } else {
    MTBLX_CHK(seg_off + q + 1, 8);
    bad = bad || a > seg_off[q + 1];
  }
  if (bad) atomicOr(reinterpret_cast<unsigned long long*>(hdr + RH_FLAGS), (unsigned long long)MTBLX_ROLLUP_BADSEG);
}

// the delimiter rule's group key lengths.  A wave holds four 16-lane groups; every loop below is
// uniform over the wave (the ballots want all of its lanes), a group that is done only idles
__global__ void __launch_bounds__(kThreads) k_rollup_glen(mtblx_records rec, GSpec g, uint64_t* glen,
                                                          const uint64_t* hdr) {
  if (hdr[RH_FLAGS] & MTBLX_ROLLUP_BADSEG) return;
  const uint32_t grp = threadIdx.x >> 4, l = threadIdx.x & 15;
  const uint32_t sh = threadIdx.x & 48u;   // where the group's 16 bits sit in the wave's ballot
  const uint64_t tile0 = (uint64_t)blockIdx.x * kLaneTile;
  for (uint32_t it = 0; it < (uint32_t)kLaneTile / 16; ++it) {
    const uint64_t r = tile0 + it * 16 + grp;
    const bool live = r < rec.n;
    uint64_t ks = 0, klen = 0;
    if (live) klen = key_span(rec, r, &ks);
    const uint8_t* kp = rec.keys + ks;
    uint64_t out = klen, seen = 0;   // fewer than count delimiters: the whole key
    bool found = false;
    for (uint64_t base = 0; __any(live && !found && base < klen); base += 16) {
      bool hit = false;
      if (live && !found && base + l < klen) {
        MTBLX_CHK(kp + base + l, 1);
        hit = kp[base + l] == g.delim;
      }
      uint32_t m = (uint32_t)(__ballot(hit) >> sh) & 0xFFFFu;
      if (live && !found && seen + __popc(m) >= g.count) {
        for (uint64_t k = g.count - seen; k > 1; --k) m &= m - 1;   // drop the delimiters before the count-th
        out = base + (uint32_t)__ffs((int)m);                       // up to and including it
        found = true;
      }
      seen += __popc(m);
    }
    if (live && l == 0) {
      MTBLX_CHK(glen + r, 8);
      glen[r] = out;
    }
  }
}

// the segments among [a, nseg) that begin at or before record i, plus a
__device__ __forceinline__ uint32_t roll_upper(const uint64_t* seg_off, uint32_t a, uint32_t nseg, uint64_t i) {
  uint32_t lo = a, hi = nseg;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    MTBLX_CHK(seg_off + mid, 8);
    if (seg_off[mid] <= i) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// a 16-lane group owns 16 consecutive records, so the segment search runs once per group and
// advances by one load per record
template <int KIND>
__global__ void __launch_bounds__(kThreads) k_rollup_heads(mtblx_records rec, GSpec g, const uint64_t* glen,
                                                           const uint64_t* seg_off, uint32_t nseg, uint8_t* flag,
                                                           const uint64_t* hdr) {
  if (hdr[RH_FLAGS] & MTBLX_ROLLUP_BADSEG) return;
  const uint32_t grp = threadIdx.x >> 4, l = threadIdx.x & 15;
  const uint32_t sh = threadIdx.x & 48u;
  const uint64_t r0 = (uint64_t)blockIdx.x * kLaneTile + grp * 16u;
  uint32_t c = 0;   // the segments that begin at or before the record at hand
  if (nseg && r0 < rec.n && r0) c = roll_upper(seg_off, 0, nseg, r0 - 1);
  for (uint32_t it = 0; it < 16; ++it) {
    const uint64_t r = r0 + it;
    const bool live = r < rec.n;
    bool head = r == 0;
    if (live && nseg && c < nseg) {
      MTBLX_CHK(seg_off + c, 8);
      if (seg_off[c] <= r) {   // a segment begins here; empty ones may begin here too
        c = roll_upper(seg_off, c + 1, nseg, r);
        head = true;
      }
    }
    uint64_t ks = 0, ps = 0, gl = 0;
    bool cmp = false;
    if (live) {
      gl = glen_of<KIND>(g, glen, r, key_span(rec, r, &ks));
      if (!head) {
        const uint64_t pl = glen_of<KIND>(g, glen, r - 1, key_span(rec, r - 1, &ps));
        if (pl != gl) head = true;
        else cmp = true;
      }
    }
    const uint8_t* kp = rec.keys + ks;
    const uint8_t* pp = rec.keys + ps;
    for (uint64_t base = 0; __any(cmp && base < gl); base += 16) {
      bool ne = false;
      if (cmp && base + l < gl) {
        MTBLX_CHK(kp + base + l, 1);
        MTBLX_CHK(pp + base + l, 1);
        ne = kp[base + l] != pp[base + l];
      }
      if ((uint32_t)(__ballot(ne) >> sh) & 0xFFFFu) {
        head = true;
        cmp = false;
      }
    }
    if (live && l == 0) {
      MTBLX_CHK(flag + r, 1);
      flag[r] = head ? 1 : 0;
    }
  }
}

// what record i brings to the two running sums: a group, and its group key's bytes
template <int KIND>
__device__ __forceinline__ void roll_contrib(const mtblx_records& rec, const GSpec& g, const uint64_t* glen,
                                             const uint8_t* flag, uint64_t i, uint64_t* heads, uint64_t* bytes) {
  *heads = *bytes = 0;
  if (i >= rec.n) return;
  MTBLX_CHK(flag + i, 1);
  if (!flag[i]) return;
  uint64_t ks;
  *heads = 1;
  *bytes = glen_of<KIND>(g, glen, i, key_span(rec, i, &ks));
}

template <int KIND>
__global__ void __launch_bounds__(kThreads) k_rollup_sums(mtblx_records rec, GSpec g, const uint64_t* glen,
                                                          const uint8_t* flag, uint64_t* tiles, const uint64_t* hdr) {
  if (hdr[RH_FLAGS] & MTBLX_ROLLUP_BADSEG) return;
  __shared__ uint64_t wsum[kThreads / 64];
  const uint64_t i0 = (uint64_t)blockIdx.x * kRollTile + (uint64_t)threadIdx.x * kRollPer;
  uint64_t s0 = 0, s1 = 0;
#pragma unroll
  for (int k = 0; k < kRollPer; ++k) {
    uint64_t h, b;
    roll_contrib<KIND>(rec, g, glen, flag, i0 + k, &h, &b);
    s0 += h;
    s1 += b;
  }
  uint64_t t0, t1;
  (void)block_scan(s0, wsum, &t0);
  (void)block_scan(s1, wsum, &t1);
  if (threadIdx.x == 0) {
    MTBLX_CHK(tiles + 2ull * blockIdx.x, 16);
    tiles[2ull * blockIdx.x] = t0;
    tiles[2ull * blockIdx.x + 1] = t1;
  }
}

// one workgroup: the tile sums -> their exclusive prefixes (in place), the totals, the planned mark.
// After a bad seg_off the totals are zero and the mark is still set: the emit then reports the flag
__global__ void __launch_bounds__(kThreads) k_rollup_scan(uint64_t* hdr, uint64_t* tiles, uint32_t ntiles,
                                                          uint64_t* totals, uint64_t planned) {
  __shared__ uint64_t wsum[kThreads / 64];
  const bool bad = hdr[RH_FLAGS] & MTBLX_ROLLUP_BADSEG;
  uint64_t carry[2] = {0, 0};
  for (uint32_t b = 0; !bad && b < ntiles; b += kThreads) {
    const uint32_t i = b + threadIdx.x;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      if (i < ntiles) MTBLX_CHK(tiles + 2ull * i + q, 8);
      const uint64_t v = i < ntiles ? tiles[2ull * i + q] : 0;
      uint64_t tot;
      const uint64_t e = block_scan(v, wsum, &tot);
      if (i < ntiles) tiles[2ull * i + q] = carry[q] + e;
      carry[q] += tot;
    }
  }
  if (threadIdx.x == 0) {
    MTBLX_CHK(hdr, 8 * RH_WORDS);
    MTBLX_CHK(totals, 16);
    hdr[RH_GROUPS] = totals[0] = carry[0];
    hdr[RH_KEYB] = totals[1] = carry[1];
    hdr[RH_PLANNED] = planned;
  }
}

// ---- emit ----
// the gate every emit kernel passes: the workspace is that of a plan over these arguments, the plan
// met no bad seg_off, and every output holds the totals.  `tell`: the one thread that reports
__device__ __forceinline__ bool roll_gate(const uint64_t* hdr, const mtblx_rolled& o, uint64_t planned, uint32_t nseg,
                                          bool tell) {
  uint32_t f = 0;
  if (hdr[RH_PLANNED] != planned) {
    f = MTBLX_ROLLUP_NOT_PLANNED;
  } else if (hdr[RH_FLAGS] & MTBLX_ROLLUP_BADSEG) {
    f = MTBLX_ROLLUP_BADSEG;
  } else {
    const uint64_t G = hdr[RH_GROUPS];
    if (hdr[RH_KEYB] > o.keys_cap || 8 * G > o.key_end_cap || 8 * (G + 1) > o.grp_rec_cap ||
        (nseg && 8 * ((uint64_t)nseg + 1) > o.seg_grp_cap))
      f = MTBLX_ROLLUP_OVERFLOW;
  }
  if (f && tell) atomicOr(o.flags, f);
  return f == 0;
}

template <int KIND>
__global__ void __launch_bounds__(kThreads) k_rollup_apply(mtblx_records rec, GSpec g, const uint64_t* glen,
                                                           const uint8_t* flag, const uint64_t* tiles,
                                                           const uint64_t* hdr, mtblx_rolled o, uint64_t planned,
                                                           uint32_t nseg) {
  if (!roll_gate(hdr, o, planned, nseg, false)) return;   // k_rollup_segs reports
  __shared__ uint64_t wsum[kThreads / 64];
  const uint64_t i0 = (uint64_t)blockIdx.x * kRollTile + (uint64_t)threadIdx.x * kRollPer;
  uint64_t h[kRollPer], b[kRollPer], s0 = 0, s1 = 0;
#pragma unroll
  for (int k = 0; k < kRollPer; ++k) {
    roll_contrib<KIND>(rec, g, glen, flag, i0 + k, &h[k], &b[k]);
    s0 += h[k];
    s1 += b[k];
  }
  uint64_t tot;
  MTBLX_CHK(tiles + 2ull * blockIdx.x, 16);
  uint64_t e0 = block_scan(s0, wsum, &tot) + tiles[2ull * blockIdx.x];
  uint64_t e1 = block_scan(s1, wsum, &tot) + tiles[2ull * blockIdx.x + 1];
#pragma unroll
  for (int k = 0; k < kRollPer; ++k) {
    if (h[k]) {   // i0 + k < n; e0 < groups, e1 + b[k] <= group key bytes: the gate has checked the capacities
      MTBLX_CHK(o.key_end + e0, 8);
      MTBLX_CHK(o.grp_rec + e0, 8);
      o.key_end[e0] = e1 + b[k];
      o.grp_rec[e0] = i0 + k;
    }
    e0 += h[k];
    e1 += b[k];
  }
}

// group g's key: the first bytes of its first record's key, to where key_end says
__global__ void __launch_bounds__(kThreads) k_rollup_gather(mtblx_records rec, const uint64_t* hdr, mtblx_rolled o,
                                                            uint64_t planned, uint32_t nseg) {
  if (!roll_gate(hdr, o, planned, nseg, false)) return;
  const uint32_t grp = threadIdx.x >> 4, l = threadIdx.x & 15;
  const uint64_t G = hdr[RH_GROUPS];
  const uint64_t tile0 = (uint64_t)blockIdx.x * kLaneTile;
  for (uint32_t it = 0; it < (uint32_t)kLaneTile / 16; ++it) {
    const uint64_t gi = tile0 + it * 16 + grp;
    if (gi >= G) break;
    MTBLX_CHK(o.grp_rec + gi, 8);
    MTBLX_CHK(o.key_end + gi, 8);
    const uint64_t r = o.grp_rec[gi];
    uint64_t off = 0, ks;
    if (gi) {
      MTBLX_CHK(o.key_end + gi - 1, 8);
      off = o.key_end[gi - 1];
    }
    const uint64_t len = o.key_end[gi] - off;   // <= the key's length
    (void)key_span(rec, r, &ks);
    copy16(o.keys + off, rec.keys + ks, len, l);
  }
}

__global__ void __launch_bounds__(kThreads) k_rollup_segs(const uint64_t* seg_off, uint32_t nseg, uint64_t n,
                                                          const uint64_t* hdr, mtblx_rolled o, uint64_t planned) {
  const uint64_t q = (uint64_t)blockIdx.x * kThreads + threadIdx.x;   // entries 0 .. nseg
  if (!roll_gate(hdr, o, planned, nseg, q == 0)) return;
  const uint64_t G = hdr[RH_GROUPS];
  if (q == 0) {
    MTBLX_CHK(o.grp_rec + G, 8);
    o.grp_rec[G] = n;
  }
  if (nseg == 0 || q > nseg) return;
  MTBLX_CHK(seg_off + q, 8);
  const uint64_t r = seg_off[q];
  uint64_t lo = 0, hi = G;   // the groups whose first record lies before r
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    MTBLX_CHK(o.grp_rec + mid, 8);
    if (o.grp_rec[mid] < r) lo = mid + 1;
    else hi = mid;
  }
  MTBLX_CHK(o.seg_grp + q, 8);
  o.seg_grp[q] = lo;
}

// ---- field rows -> values ----
__global__ void __launch_bounds__(kThreads) k_renc_copy(const uint64_t* fields, uint64_t n, uint32_t nf, uint8_t* vals,
                                                        uint64_t* val_end) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;   // one word of fields
  if (i >= n * nf) return;
  MTBLX_CHK(fields + i, 8);
  MTBLX_CHK(vals + 8 * i, 8);
  *reinterpret_cast<lu64u*>(vals + 8 * i) = fields[i];
  if (i < n) {
    MTBLX_CHK(val_end + i, 8);
    val_end[i] = 8ull * nf * (i + 1);
  }
}

template <int F>
__device__ __forceinline__ uint64_t renc_row(const uint64_t* fields, uint64_t i, uint64_t n, uint64_t* v) {
  if (i >= n) return 0;
  MTBLX_CHK(fields + i * F, 8 * F);
#pragma unroll
  for (int f = 0; f < F; ++f) v[f] = fields[i * F + f];
  return r_varint_len_all<F>(v);
}

template <int F>
__global__ void __launch_bounds__(kThreads) k_renc_sums(const uint64_t* fields, uint64_t n, uint64_t* tiles) {
  __shared__ uint64_t wsum[kThreads / 64];
  const uint64_t i0 = (uint64_t)blockIdx.x * kRollTile + (uint64_t)threadIdx.x * kRollPer;
  uint64_t s = 0;
#pragma unroll
  for (int k = 0; k < kRollPer; ++k) {
    uint64_t v[F];
    s += renc_row<F>(fields, i0 + k, n, v);
  }
  uint64_t tot;
  (void)block_scan(s, wsum, &tot);
  if (threadIdx.x == 0) {
    MTBLX_CHK(tiles + blockIdx.x, 8);
    tiles[blockIdx.x] = tot;
  }
}

__global__ void __launch_bounds__(kThreads) k_renc_scan(uint64_t* tiles, uint32_t ntiles) {
  __shared__ uint64_t wsum[kThreads / 64];
  uint64_t carry = 0;
  for (uint32_t b = 0; b < ntiles; b += kThreads) {
    const uint32_t i = b + threadIdx.x;
    if (i < ntiles) MTBLX_CHK(tiles + i, 8);
    const uint64_t v = i < ntiles ? tiles[i] : 0;
    uint64_t tot;
    const uint64_t e = block_scan(v, wsum, &tot);
    if (i < ntiles) tiles[i] = carry + e;
    carry += tot;
  }
}

// a row takes at most 10 * F bytes and cap >= 10 * F * n (checked on the host): every store fits
template <int F>
__global__ void __launch_bounds__(kThreads) k_renc_store(const uint64_t* fields, uint64_t n, const uint64_t* tiles,
                                                         uint8_t* vals, uint64_t* val_end) {
  __shared__ uint64_t wsum[kThreads / 64];
  const uint64_t i0 = (uint64_t)blockIdx.x * kRollTile + (uint64_t)threadIdx.x * kRollPer;
  uint64_t v[kRollPer][F], len[kRollPer], s = 0;
#pragma unroll
  for (int k = 0; k < kRollPer; ++k) {
    len[k] = renc_row<F>(fields, i0 + k, n, v[k]);
    s += len[k];
  }
  uint64_t tot;
  MTBLX_CHK(tiles + blockIdx.x, 8);
  uint64_t e = block_scan(s, wsum, &tot) + tiles[blockIdx.x];
#pragma unroll
  for (int k = 0; k < kRollPer; ++k) {
    if (i0 + k < n) {
      MTBLX_CHK(vals + e, len[k]);
      MTBLX_CHK(val_end + i0 + k, 8);
      r_store_varint<F>(vals + e, v[k]);
      val_end[i0 + k] = e + len[k];
    }
    e += len[k];
  }
}

template <int F>
void renc_launch(const uint64_t* fields, uint64_t n, uint8_t* vals, uint64_t* val_end, uint64_t cap, uint64_t* tiles,
                 uint32_t ntiles, hipStream_t s) {
  MTBLX_LAUNCH((MTBLX_R(fields, 8 * n * F), MTBLX_R(tiles, 8ull * ntiles)), (k_renc_sums<F>), dim3(ntiles),
               dim3(kThreads), 0, s, fields, n, tiles);
  MTBLX_LAUNCH((MTBLX_R(tiles, 8ull * ntiles)), k_renc_scan, dim3(1), dim3(kThreads), 0, s, tiles, ntiles);
  MTBLX_LAUNCH((MTBLX_R(fields, 8 * n * F), MTBLX_R(tiles, 8ull * ntiles), MTBLX_R(vals, cap), MTBLX_R(val_end, 8 * n)),
               (k_renc_store<F>), dim3(ntiles), dim3(kThreads), 0, s, fields, n, tiles, vals, val_end);
}

struct RollLayout {
  size_t glen, flag, tiles, total;
  uint32_t ntiles;
};

RollLayout roll_layout(uint64_t n) {
  RollLayout L{};
  L.ntiles = (uint32_t)((n + kRollTile - 1) / kRollTile);
  L.glen = 8 * RH_WORDS;
  L.flag = L.glen + up256(8 * n);
  L.tiles = L.flag + up256(n);
  L.total = L.tiles + up256(16ull * L.ntiles);
  return L;
}

// the mark of a plan over n records, nseg segments and this rule: an emit with other arguments
// finds another word in the header
uint64_t roll_mark(uint64_t n, uint32_t nseg, const mtblx_group& g) {
  uint64_t h = kRollMagic ^ n ^ ((uint64_t)nseg << 32);
  const uint64_t w[4] = {g.kind, g.length, g.delim, g.count};
  for (uint64_t x : w) h = (h ^ x) * 0x9E3779B97F4A7C15ull + 0x7F4A7C15ull;
  return h | 1u;   // never the zero the plan leaves in a cleared header
}

GSpec gspec_of(const mtblx_group& g) {
  GSpec s;
  s.length = g.length;
  s.delim = g.delim;
  s.count = g.count;
  return s;
}

}  // namespace

extern "C" uint32_t mtblx_rollup_tile(void) { return (uint32_t)kRollTile; }

extern "C" size_t mtblx_rollup_impl_ws_bytes(uint64_t n) { return roll_layout(n).total; }

// arguments already checked (mtblx_api.cpp)
extern "C" int mtblx_rollup_impl_plan(const mtblx_records* recs, const mtblx_group* group, const uint64_t* seg_off,
                                      uint32_t nseg, uint64_t* totals, void* ws, hipStream_t s) {
  const mtblx_records rec = *recs;
  const uint64_t n = rec.n;
  const RollLayout L = roll_layout(n);
  uint8_t* w = static_cast<uint8_t*>(ws);
  uint64_t* hdr = reinterpret_cast<uint64_t*>(w);
  uint64_t* glen = reinterpret_cast<uint64_t*>(w + L.glen);
  uint8_t* flag = w + L.flag;
  uint64_t* tiles = reinterpret_cast<uint64_t*>(w + L.tiles);
  const GSpec g = gspec_of(*group);
  const bool delim = group->kind == MTBLX_GROUP_DELIM;
  if (hipMemsetAsync(hdr, 0, 8 * RH_WORDS, s) != hipSuccess) return MTBLX_E_HIP;
  if (nseg)
    MTBLX_LAUNCH((MTBLX_R(seg_off, 8ull * nseg + 8), MTBLX_R(hdr, 8 * RH_WORDS)), k_rollup_segcheck,
                 dim3((unsigned)(((uint64_t)nseg + kThreads) / kThreads)), dim3(kThreads), 0, s, seg_off, nseg, n, hdr);
  if (n) {
    const dim3 lanes((unsigned)((n + kLaneTile - 1) / kLaneTile)), tiled(L.ntiles), b(kThreads);
    if (delim) {
      MTBLX_LAUNCH((MTBLX_R(rec.key_end, 8 * n), rec.keys, MTBLX_R(glen, 8 * n), MTBLX_R(hdr, 8 * RH_WORDS)),
                   k_rollup_glen, lanes, b, 0, s, rec, g, glen, hdr);
      MTBLX_LAUNCH((MTBLX_R(rec.key_end, 8 * n), rec.keys, MTBLX_R(glen, 8 * n), MTBLX_R(seg_off, 8ull * nseg + 8),
                    MTBLX_R(flag, n), MTBLX_R(hdr, 8 * RH_WORDS)),
                   (k_rollup_heads<MTBLX_GROUP_DELIM>), lanes, b, 0, s, rec, g, glen, seg_off, nseg, flag, hdr);
      MTBLX_LAUNCH((MTBLX_R(rec.key_end, 8 * n), MTBLX_R(glen, 8 * n), MTBLX_R(flag, n), MTBLX_R(tiles, 16ull * L.ntiles),
                    MTBLX_R(hdr, 8 * RH_WORDS)),
                   (k_rollup_sums<MTBLX_GROUP_DELIM>), tiled, b, 0, s, rec, g, glen, flag, tiles, hdr);
    } else {
      MTBLX_LAUNCH((MTBLX_R(rec.key_end, 8 * n), rec.keys, MTBLX_R(seg_off, 8ull * nseg + 8), MTBLX_R(flag, n),
                    MTBLX_R(hdr, 8 * RH_WORDS)),
                   (k_rollup_heads<MTBLX_GROUP_LENGTH>), lanes, b, 0, s, rec, g, glen, seg_off, nseg, flag, hdr);
      MTBLX_LAUNCH((MTBLX_R(rec.key_end, 8 * n), MTBLX_R(flag, n), MTBLX_R(tiles, 16ull * L.ntiles),
                    MTBLX_R(hdr, 8 * RH_WORDS)),
                   (k_rollup_sums<MTBLX_GROUP_LENGTH>), tiled, b, 0, s, rec, g, glen, flag, tiles, hdr);
    }
  }
  MTBLX_LAUNCH((MTBLX_R(hdr, 8 * RH_WORDS), MTBLX_R(tiles, 16ull * L.ntiles), MTBLX_R(totals, 16)), k_rollup_scan,
               dim3(1), dim3(kThreads), 0, s, hdr, tiles, L.ntiles, totals, roll_mark(n, nseg, *group));
  return hipGetLastError() == hipSuccess ? MTBLX_OK : MTBLX_E_HIP;
}

extern "C" int mtblx_rollup_impl_emit(const mtblx_records* recs, const mtblx_group* group, const uint64_t* seg_off,
                                      uint32_t nseg, const mtblx_rolled* out, const void* ws, hipStream_t s) {
  const mtblx_records rec = *recs;
  const uint64_t n = rec.n;
  const RollLayout L = roll_layout(n);
  const uint8_t* w = static_cast<const uint8_t*>(ws);
  const uint64_t* hdr = reinterpret_cast<const uint64_t*>(w);
  const uint64_t* glen = reinterpret_cast<const uint64_t*>(w + L.glen);
  const uint8_t* flag = w + L.flag;
  const uint64_t* tiles = reinterpret_cast<const uint64_t*>(w + L.tiles);
  const GSpec g = gspec_of(*group);
  const mtblx_rolled o = *out;
  const uint64_t mark = roll_mark(n, nseg, *group);
  if (hipMemsetAsync(o.flags, 0, 4, s) != hipSuccess) return MTBLX_E_HIP;
  if (n) {
    const dim3 tiled(L.ntiles), b(kThreads);
    if (group->kind == MTBLX_GROUP_DELIM)
      MTBLX_LAUNCH((MTBLX_R(rec.key_end, 8 * n), MTBLX_R(glen, 8 * n), MTBLX_R(flag, n), MTBLX_R(tiles, 16ull * L.ntiles),
                    MTBLX_R(hdr, 8 * RH_WORDS), MTBLX_R(o.key_end, o.key_end_cap), MTBLX_R(o.grp_rec, o.grp_rec_cap)),
                   (k_rollup_apply<MTBLX_GROUP_DELIM>), tiled, b, 0, s, rec, g, glen, flag, tiles, hdr, o, mark, nseg);
    else
      MTBLX_LAUNCH((MTBLX_R(rec.key_end, 8 * n), MTBLX_R(flag, n), MTBLX_R(tiles, 16ull * L.ntiles),
                    MTBLX_R(hdr, 8 * RH_WORDS), MTBLX_R(o.key_end, o.key_end_cap), MTBLX_R(o.grp_rec, o.grp_rec_cap)),
                   (k_rollup_apply<MTBLX_GROUP_LENGTH>), tiled, b, 0, s, rec, g, glen, flag, tiles, hdr, o, mark, nseg);
    // the groups are at most the records: a grid over n covers them, a workgroup past them returns
    MTBLX_LAUNCH((MTBLX_R(rec.key_end, 8 * n), rec.keys, MTBLX_R(hdr, 8 * RH_WORDS), MTBLX_R(o.keys, o.keys_cap),
                  MTBLX_R(o.key_end, o.key_end_cap), MTBLX_R(o.grp_rec, o.grp_rec_cap)),
                 k_rollup_gather, dim3((unsigned)((n + kLaneTile - 1) / kLaneTile)), b, 0, s, rec, hdr, o, mark, nseg);
  }
  MTBLX_LAUNCH((MTBLX_R(seg_off, 8ull * nseg + 8), MTBLX_R(hdr, 8 * RH_WORDS), MTBLX_R(o.grp_rec, o.grp_rec_cap),
                MTBLX_R(o.seg_grp, o.seg_grp_cap), MTBLX_R(o.flags, 4)),
               k_rollup_segs, dim3((unsigned)(((uint64_t)nseg + kThreads) / kThreads)), dim3(kThreads), 0, s, seg_off,
               nseg, n, hdr, o, mark);
  return hipGetLastError() == hipSuccess ? MTBLX_OK : MTBLX_E_HIP;
}

extern "C" size_t mtblx_reduce_encode_impl_ws_bytes(uint64_t n) {
  return up256(8 * ((n + kRollTile - 1) / kRollTile)) + 256u;
}

extern "C" int mtblx_reduce_encode_impl(const uint64_t* fields, uint64_t n, const mtblx_reduce* spec, uint8_t* vals,
                                        uint64_t* val_end, uint64_t cap, void* ws, hipStream_t s) {
  RSpec sp;
  bool varint;
  if (!reduce_spec(spec, &sp, &varint)) return MTBLX_E_INVAL;
  const uint32_t nf = spec->nfields;
  if (n == 0) return MTBLX_OK;
  if (!varint) {
    MTBLX_LAUNCH((MTBLX_R(fields, 8 * n * nf), MTBLX_R(vals, cap), MTBLX_R(val_end, 8 * n)), k_renc_copy,
                 dim3((unsigned)((n * nf + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, fields, n, nf, vals,
                 val_end);
    return hipGetLastError() == hipSuccess ? MTBLX_OK : MTBLX_E_HIP;
  }
  uint64_t* tiles = static_cast<uint64_t*>(ws);
  const uint32_t ntiles = (uint32_t)((n + kRollTile - 1) / kRollTile);
  switch (nf) {
    case 1: renc_launch<1>(fields, n, vals, val_end, cap, tiles, ntiles, s); break;
    case 2: renc_launch<2>(fields, n, vals, val_end, cap, tiles, ntiles, s); break;
    case 3: renc_launch<3>(fields, n, vals, val_end, cap, tiles, ntiles, s); break;
    case 4: renc_launch<4>(fields, n, vals, val_end, cap, tiles, ntiles, s); break;
    case 5: renc_launch<5>(fields, n, vals, val_end, cap, tiles, ntiles, s); break;
    case 6: renc_launch<6>(fields, n, vals, val_end, cap, tiles, ntiles, s); break;
    case 7: renc_launch<7>(fields, n, vals, val_end, cap, tiles, ntiles, s); break;
    default: renc_launch<8>(fields, n, vals, val_end, cap, tiles, ntiles, s); break;
  }
  return hipGetLastError() == hipSuccess ? MTBLX_OK : MTBLX_E_HIP;
}

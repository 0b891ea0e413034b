// merge_dev.h — what the device Merger (merge.hip), the device Sorter (sort.hip) and the segmented
// merge (merge_seg.hip) share: the 16-byte handle, the total order on handles, the merge-path pass,
// the grouping scan, the gather and the workspace layout (DESIGN.md §4 "The Merger", "The Sorter",
// "Merged batched scans").
//
//   k_merge_pass    run 2j merged with run 2j+1, an unpaired run carried over.  A workgroup owns
//                   kTile consecutive output handles; for every pair of runs its slice touches it
//                   finds its two input sub-ranges by a (64-way, one wave per diagonal) search on
//                   the diagonal, stages them in LDS, ranks every handle against the other
//                   sub-range there and writes the slice with coalesced 16-byte stores.  The run
//                   boundaries come from the source table (SrcRuns: the merge, run j of a level =
//                   sources [j << level, (j + 1) << level)) or from a uniform run length clipped
//                   at n (TileRuns: the sort, run j = handles [j * kSortTile << level, ...))
//   k_group_*       head flags (key != predecessor's), the empty-key quirk (merge only), and six
//                   running sums (groups, key bytes, values, value bytes, first-value bytes,
//                   last-value bytes) as a three-launch scan: tile sums, one workgroup over the
//                   tile sums, apply
//   k_group_select  set operations (the merge and the segmented merge, on request): between the
//                   flags and the sums, the groups whose source mask fails a rule are flagged out
//   k_merge_emit   16 lanes per record gather the group's key once and the mode's values
//
// Order: keys compare as unsigned bytes then by length (Vec<u8>::cmp); equal keys by source number,
// then by record index.  The order is total, so no pass ever reorders equal keys: run 2j holds
// lower (source, index) pairs than run 2j+1.  Every pass is its own launch: no workgroup waits for
// another.  Everything here sits in an unnamed namespace: each of the translation units gets
// its own copy, as with bounds.h.  The passes take their order as a policy (KeyOrder below; the
// segmented merge orders by segment first).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "mtblx.h"
#include "bounds.h"
#include "devinfo.h"
#include "lane_dev.h"   // kThreads, block_scan, copy16, up256

namespace {

constexpr int kTile = 1024;                 // handles per workgroup slice: 2 x 16 KiB of LDS, so
                                            // 5 workgroups (20 waves) fit a CU's 160 KiB
constexpr int kPer = kTile / kThreads;      // records per thread in the grouping kernels
constexpr int kEmitTile = 256;              // records per workgroup of the emit: 16 per 16-lane group, each a
                                            // chain of dependent loads (handle -> END offsets -> bytes), so
                                            // the gather wants many waves in flight rather than long loops
constexpr int kSortTile = MTBLX_SORT_TILE;  // handles per sorted run of the Sorter's tile sort (sort.hip)
constexpr uint64_t kMagic = 0x4d54424c584d5247ull;
// the Sorter's planned mark differs from the Merger's in bits no record or source count reaches
constexpr uint64_t kSortMagic = 0x5354424c58535254ull;

// workgroups of the handle-building launches (k_merge_build, k_seg_build, k_sort_skip): kThreads
// records per workgroup and trip, at most 16 workgroups per CU.  The launches and
// mtblx_debug_grid_items() share it.
inline uint64_t build_grid_cap() { return (uint64_t)mtblx_dev::cu_count() * 16u; }

// workspace header words (u64)
enum { H_GROUPS = 0, H_KEYB, H_NVAL, H_VALB, H_DROPPED, H_FLAGS, H_SKIP, H_PLANNED, H_FIRSTB, H_LASTB,
       H_SEGSKIP,   // merge_seg.hip: u64 words from the header to the per-segment skip array
       H_SELGROUPS, H_SELRECS,   // the groups a selection (k_group_select) left out, the records in them
       H_WORDS = 32 };
constexpr int kReduceEdgeWords = 18;   // u64 words per tile of the device merge functions' edge array (reduce_dev.h)
// k_merge_emit's internal mode, after the public MTBLX_MERGE_* ones: the last step of the varint reduce
// emit (reduce_dev.h): keys and key_end as ever, and only the groups of one bring their value, to
// where the scanned val_end says their slot begins; val_end itself is not written
constexpr int kEmitSingles = 16;
constexpr int kChan = 6;   // groups, key bytes, values, value bytes, first-value bytes, last-value bytes

struct alignas(16) Handle {
  uint64_t prefix;
  uint32_t src;
  uint32_t idx;
};

struct SrcTab {   // travels in the kernel arguments: 64 x 40 B + 65 x 4 B
  mtblx_records s[MTBLX_MERGE_MAX_SOURCES];
  uint32_t base[MTBLX_MERGE_MAX_SOURCES + 1];   // records before source i (N < 2^32 - 16)
  uint32_t nsrc;
};

typedef uint64_t u64u __attribute__((aligned(1)));

struct Key {
  const uint8_t* p;
  uint64_t len;
};

__device__ __forceinline__ Key key_of(const SrcTab& t, uint32_t s, uint32_t i) {
  const uint64_t* ke = t.s[s].key_end;
  const uint64_t b = i ? ke[i - 1] : 0;
  return Key{t.s[s].keys + b, ke[i] - b};
}

__device__ __forceinline__ uint64_t val_len(const SrcTab& t, uint32_t s, uint32_t i, uint64_t* start) {
  const uint64_t* ve = t.s[s].val_end;
  const uint64_t b = i ? ve[i - 1] : 0;
  *start = b;
  return ve[i] - b;
}

// Vec<u8>::cmp of two keys whose first `from` bytes (clamped to the shorter length) are known equal
__device__ __forceinline__ int key_cmp(Key a, Key b, uint64_t from) {
  const uint64_t m = a.len < b.len ? a.len : b.len;
  uint64_t k = from < m ? from : m;
  for (; k + 8 <= m; k += 8) {
    const uint64_t x = *reinterpret_cast<const u64u*>(a.p + k), y = *reinterpret_cast<const u64u*>(b.p + k);
    if (x != y) return __builtin_bswap64(x) < __builtin_bswap64(y) ? -1 : 1;
  }
  for (; k < m; ++k) {
    const uint8_t x = a.p[k], y = b.p[k];
    if (x != y) return x < y ? -1 : 1;
  }
  return a.len < b.len ? -1 : a.len > b.len ? 1 : 0;
}

// equal prefixes: the bytes up to skip + 8 (or the shorter key's end) are equal, the rest is in memory
__device__ __forceinline__ int h_keycmp(const SrcTab& t, Handle a, Handle b, uint64_t skip) {
  if (a.prefix != b.prefix) return a.prefix < b.prefix ? -1 : 1;
  return key_cmp(key_of(t, a.src, a.idx), key_of(t, b.src, b.idx), skip + 8);
}

// the total order: key, then source number, then index (the merge never needs the index: equal keys
// inside one sorted source are refused; the sort has source 0 everywhere and lives on it)
__device__ __forceinline__ bool h_less(const SrcTab& t, Handle a, Handle b, uint64_t skip) {
  const int c = h_keycmp(t, a, b, skip);
  if (c) return c < 0;
  if (a.src != b.src) return a.src < b.src;
  return a.idx < b.idx;
}

// The order a pass merges by, as a policy: ctx() reads what the order needs from the workspace
// header once per kernel, less() is the total order.  KeyOrder is the one above (the Merger, the
// Sorter); merge_seg.hip brings its own (segment, key, source).
struct KeyOrder {
  typedef uint64_t Ctx;   // the shared key bytes
  static __device__ __forceinline__ Ctx ctx(const uint64_t* hdr) { return hdr[H_SKIP]; }
  static __device__ __forceinline__ bool less(const SrcTab& t, Handle a, Handle b, Ctx skip) {
    return h_less(t, a, b, skip);
  }
};

// Where the sorted runs of a pass lie.  start(): handles before run j of a level; count(): the
// runs of level 0.
struct SrcRuns {   // the merge: run j = sources [j << level, (j + 1) << level)
  static __device__ __forceinline__ uint32_t start(const SrcTab& t, uint32_t, uint32_t j, uint32_t level) {
    const uint64_t s = (uint64_t)j << level;
    return t.base[s < t.nsrc ? (uint32_t)s : t.nsrc];
  }
  static __device__ __forceinline__ uint32_t count(const SrcTab& t, uint32_t) { return t.nsrc; }
};
struct TileRuns {   // the sort: run j = handles [j * (kSortTile << level), (j + 1) * (kSortTile << level)) below n
  static __device__ __forceinline__ uint32_t start(const SrcTab&, uint32_t n, uint32_t j, uint32_t level) {
    const uint64_t s = ((uint64_t)j << level) * (uint64_t)kSortTile;   // j <= 2^22, level <= 22: no overflow
    return s < n ? (uint32_t)s : n;
  }
  static __device__ __forceinline__ uint32_t count(const SrcTab&, uint32_t n) {
    return (uint32_t)(((uint64_t)n + kSortTile - 1) / kSortTile);
  }
};

// merge path: how many of the first d outputs of A (na) merged with B (nb) come from A.  Called by
// all 64 lanes of a wave with the same arguments: "A[mid] < B[d - 1 - mid]" holds for every mid
// below the answer and for none from it on, so each step probes 64 evenly spaced mids at once and
// a ballot keeps the one interval where the answer lies: ceil(log64) dependent global loads where a
// two-way search by one lane makes log2 of them (the chain every slice waits for before it stages)
template <class Ord = KeyOrder>
__device__ __forceinline__ uint32_t merge_path(const SrcTab& t, const Handle* a, uint32_t na, const Handle* b,
                                               uint32_t nb, uint32_t d, typename Ord::Ctx skip) {
  uint32_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;   // the answer is in [lo, hi]
  const uint32_t lane = threadIdx.x & 63u;
  while (lo < hi) {
    const uint32_t step = (hi - lo + 63u) / 64u;
    const uint64_t mid = (uint64_t)lo + (uint64_t)lane * step;
    bool below = false;
    if (mid < hi) {
      MTBLX_CHK(a + mid, 16);
      MTBLX_CHK(b + (d - 1 - mid), 16);
      below = Ord::less(t, a[mid], b[d - 1 - mid], skip);
    }
    const uint32_t c = (uint32_t)__popcll(__ballot(below));   // the probes below the answer: the first c
    const uint64_t next = (uint64_t)lo + (uint64_t)c * step;  // probe c, the first not below (if it exists)
    if (c < 64u && next < hi) hi = (uint32_t)next;
    if (c) lo = lo + (c - 1u) * step + 1u;
  }
  return lo;
}

template <class Runs, class Ord = KeyOrder>
__global__ void __launch_bounds__(kThreads) k_merge_pass(SrcTab t, uint64_t* hdr, const Handle* in, Handle* out,
                                                         uint32_t n, uint32_t level) {
  __shared__ Handle sin[kTile];
  __shared__ Handle sout[kTile];
  __shared__ uint32_t part[2];
  const typename Ord::Ctx skip = Ord::ctx(hdr);
  const uint64_t lo = (uint64_t)blockIdx.x * kTile;
  const uint64_t hi = lo + kTile < n ? lo + kTile : n;
  const uint32_t npair = (uint32_t)(((uint64_t)Runs::count(t, n) + (2ull << level) - 1) >> (level + 1));
  uint32_t j0 = 0, j1 = npair;   // the last pair starting at or before lo
  while (j1 - j0 > 1) {
    const uint32_t mid = (j0 + j1) / 2;
    if (Runs::start(t, n, mid, level + 1) <= lo) j0 = mid; else j1 = mid;
  }
  for (uint32_t j = j0; j < npair; ++j) {
    const uint32_t ps = Runs::start(t, n, j, level + 1);
    if (ps >= hi) break;
    const uint32_t pm = Runs::start(t, n, 2 * j + 1, level), pe = Runs::start(t, n, j + 1, level + 1);
    if (pe <= lo) continue;
    const uint32_t na = pm - ps, nb = pe - pm;
    const uint32_t d0 = (uint32_t)(lo > ps ? lo - ps : 0), d1 = (uint32_t)((hi < pe ? hi : pe) - ps);
    const uint32_t cnt = d1 - d0;
    const uint32_t wave = threadIdx.x >> 6;
    if (wave < 2) {   // wave 0: the slice's first diagonal, wave 1: its last
      const uint32_t r = merge_path<Ord>(t, in + ps, na, in + pm, nb, wave ? d1 : d0, skip);
      if ((threadIdx.x & 63u) == 0) part[wave] = r;
    }
    __syncthreads();
    const uint32_t a0 = part[0], a1 = part[1], b0 = d0 - a0, b1 = d1 - a1;
    const uint32_t ca = a1 - a0, cb = b1 - b0;
    // sorted runs give monotone splits; anything else must not index anything
    const bool ok = a1 >= a0 && b1 >= b0 && a1 <= na && b1 <= nb && ca + cb == cnt && cnt <= (uint32_t)kTile;
    if (ok) {
      for (uint32_t k = threadIdx.x; k < cnt; k += kThreads) {
        const Handle* p = k < ca ? in + ps + a0 + k : in + pm + b0 + (k - ca);
        MTBLX_CHK(p, 16);
        sin[k] = *p;
      }
      __syncthreads();
      for (uint32_t k = threadIdx.x; k < cnt; k += kThreads) {
        const Handle h = sin[k];
        // the order is total ((source, index) pairs differ across the two runs): rank = own position +
        // the other sub-range's handles below h, by a binary search in LDS
        const bool isa = k < ca;
        uint32_t l = isa ? ca : 0, r = isa ? cnt : ca;
        const uint32_t first = l;
        while (l < r) {
          const uint32_t mid = l + (r - l) / 2;
          if (Ord::less(t, sin[mid], h, skip)) l = mid + 1; else r = mid;
        }
        sout[(isa ? k : k - ca) + (l - first)] = h;
      }
      __syncthreads();
      for (uint32_t k = threadIdx.x; k < cnt; k += kThreads) {
        MTBLX_CHK(out + ps + d0 + k, 16);
        out[ps + d0 + k] = sout[k];
      }
    } else if (threadIdx.x == 0) {
      atomicOr((unsigned long long*)(hdr + H_FLAGS), 2ull);
    }
    __syncthreads();
  }
}

// ---- grouping ----
// flag[i]: bit 0 = record i (merged order) starts a group, bit 1 = dropped by the empty-key quirk
// (or, later, left out by k_group_select: every kernel after it skips both alike).
// MergerIter::next (src/merger.rs:182-186) uses cur_key.is_empty() for "no current key": every
// empty-key record re-adopts the next heap entry's key and clears cur_vals, so the empty-key
// records (at most one per sorted source: the first ones in merged order) vanish when any record
// follows, and only the last taken survives -- as a group of one -- when none does.  In merged
// order that is: an empty-key record is kept iff it is the very last record.
// kQuirk = false (the sort; Sorter::write_chunk, src/sorter.rs:154-188, keeps its current key in an
// Option): an empty-key group is a group like any other.  A broken order sets MTBLX_MERGE_UNSORTED
// in the merge and, in the sort, whose input has no order to break, MTBLX_MERGE_INTERNAL.
template <bool kQuirk>
__global__ void __launch_bounds__(kThreads) k_group_flags(SrcTab t, uint64_t* hdr, const Handle* h, uint8_t* flag,
                                                          uint32_t n) {
  const uint64_t skip = hdr[H_SKIP];
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  MTBLX_CHK(h + i, 16);
  const Handle c = h[i];
  const uint64_t klen = key_of(t, c.src, c.idx).len;
  const bool dropped = kQuirk && klen == 0 && i + 1 != n;
  bool head = !dropped;
  if (head && i && (klen || !kQuirk)) {
    const Handle p = h[i - 1];
    const int o = h_keycmp(t, p, c, skip);
    head = o != 0;
    // the order itself is re-checked here: descending, or equal keys not ascending in (source, index).
    // For the merge that is "not in source order": equal keys of one source never get this far
    if (o > 0 || (o == 0 && (p.src > c.src || (p.src == c.src && p.idx >= c.idx))))
      atomicOr((unsigned long long*)(hdr + H_FLAGS), kQuirk ? 1ull : 2ull);
  }
  MTBLX_CHK(flag + i, 1);
  flag[i] = (uint8_t)((head ? 1 : 0) | (dropped ? 2 : 0));
}

// ---- selection (set operations; include/mtblx.h "Set operations") ----
// A group (a kept head and the kept non-heads after it) holds at most one record per source, so its
// membership is one 64-bit mask and it is never longer than 64 records.  k_group_select keeps the
// groups whose mask passes the rule and gives every record of the others bit 1; a rejected head
// keeps bit 0, because contrib(), k_merge_emit and the reducers find a group's tail as
// flag[i + 1] & 1 and the kept group in front of a rejected one must still see its end.  Records the
// quirk dropped belong to no group and pass through.
// One launch: a workgroup owns kTile records and stages their flags and source bits with a halo of
// 63 records on each side in LDS (a group of a tile's record lies inside it), the "bit 0" bits as a
// bitmap (a ballot per 64 records), from which a record finds its group's first and last record with
// one clz / ctz.  Six doubling steps of a segmented OR leave every group's mask with its last record,
// which evaluates the rule once; every member reads the verdict there.  The input flags are read
// from `fin`, a copy apart from `flag` (the plans let the flag kernels write into the gi array,
// unused until k_group_apply): a workgroup reads its neighbours' records in the halo while they write.
// What a tile leaves out (groups, records) goes to two words per tile of `part` (the reducers' edge
// array, unused until an emit), which k_group_scan adds up: no two workgroups write one address.
constexpr int kSelHalo = MTBLX_MERGE_MAX_SOURCES - 1;
constexpr int kSelWin = kTile + 2 * 64;     // the tile and the two halos, padded to whole bitmap words
constexpr int kSelWords = kSelWin / 64;
constexpr int kSelPer = (kSelWin + kThreads - 1) / kThreads;
static_assert(kSelWin % 64 == 0 && kSelHalo < 64 && kThreads % 64 == 0, "a wave's ballot is one bitmap word");

// the first record of p's run: the last window position <= p whose bit is set
__device__ __forceinline__ uint32_t sel_first(const uint64_t* bnd, uint32_t p) {
  const uint32_t w = p >> 6;
  const uint64_t x = bnd[w] & (~0ull >> (63u - (p & 63u)));
  if (x) return (w << 6) + 63u - (uint32_t)__builtin_clzll(x);
  if (w && bnd[w - 1]) return ((w - 1) << 6) + 63u - (uint32_t)__builtin_clzll(bnd[w - 1]);
  return p > (uint32_t)kSelHalo ? p - kSelHalo : 0u;   // a run cut by the window's edge (halo records only)
}

// the last record of p's run: the position before the first one > p whose bit is set
__device__ __forceinline__ uint32_t sel_last(const uint64_t* bnd, uint32_t p) {
  const uint32_t q = p + 1;
  if (q >= (uint32_t)kSelWin) return p;
  const uint32_t w = q >> 6;
  const uint64_t x = bnd[w] >> (q & 63u);
  if (x) return q + (uint32_t)__builtin_ctzll(x) - 1u;
  if (w + 1 < (uint32_t)kSelWords && bnd[w + 1]) return ((w + 1) << 6) + (uint32_t)__builtin_ctzll(bnd[w + 1]) - 1u;
  return p + kSelHalo < (uint32_t)kSelWin ? p + kSelHalo : (uint32_t)kSelWin - 1u;
}

// sel.min_count >= 1 (the host has normalised it).  The Sorter has no sources and never launches it
[[maybe_unused]] __global__ void __launch_bounds__(kThreads)
k_group_select(const Handle* h, const uint8_t* fin, uint8_t* flag, uint64_t* part, uint32_t n, mtblx_select sel) {
  __shared__ uint64_t m[2][kSelWin];
  __shared__ uint64_t bnd[kSelWords];
  __shared__ uint8_t fl[kSelWin], rej[kSelWin];
  __shared__ uint32_t cnt[2];
  const uint64_t lo = (uint64_t)blockIdx.x * kTile;
  const uint64_t hi = lo + kTile < n ? lo + kTile : n;
  const uint64_t wlo = lo >= (uint64_t)kSelHalo ? lo - kSelHalo : 0;
  const uint64_t whi = hi + kSelHalo < n ? hi + kSelHalo : n;
  if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
#pragma unroll
  for (int it = 0; it < kSelPer; ++it) {
    const uint32_t p = threadIdx.x + it * kThreads;
    if (p >= (uint32_t)kSelWin) break;   // the same for a whole wave
    const uint64_t rec = wlo + p;
    uint8_t f = 3;   // past the window: not kept, and the end of whatever run reaches it
    uint64_t mk = 0;
    if (rec < whi) {
      MTBLX_CHK(fin + rec, 1);
      f = fin[rec];
      if (!(f & 2)) {
        MTBLX_CHK(&h[rec].src, 4);
        mk = 1ull << (h[rec].src & 63u);
      }
    }
    fl[p] = f;
    rej[p] = 0;
    m[0][p] = mk;
    const uint64_t b = __ballot(f & 1);
    if ((threadIdx.x & 63u) == 0) bnd[p >> 6] = b;
  }
  __syncthreads();
  uint32_t first[kSelPer], last[kSelPer];
#pragma unroll
  for (int it = 0; it < kSelPer; ++it) {
    const uint32_t p = threadIdx.x + it * kThreads;
    first[it] = last[it] = 0;
    if (p < (uint32_t)kSelWin) {
      first[it] = sel_first(bnd, p);
      last[it] = sel_last(bnd, p);
    }
  }
  int cur = 0;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {   // the inclusive segmented OR: 64 records in six steps
#pragma unroll
    for (int it = 0; it < kSelPer; ++it) {
      const uint32_t p = threadIdx.x + it * kThreads;
      if (p < (uint32_t)kSelWin) {
        uint64_t v = m[cur][p];
        if (p >= first[it] + d) v |= m[cur][p - d];
        m[cur ^ 1][p] = v;
      }
    }
    __syncthreads();
    cur ^= 1;
  }
#pragma unroll
  for (int it = 0; it < kSelPer; ++it) {   // the rule, once per group: by its last record
    const uint32_t p = threadIdx.x + it * kThreads;
    if (p < (uint32_t)kSelWin && last[it] == p && !(fl[p] & 2)) {
      const uint64_t g = m[cur][p];
      const uint32_t c = (uint32_t)__popcll(g);
      const bool keep = (g & sel.require) == sel.require && !(g & sel.exclude) && c >= sel.min_count &&
                        c <= sel.max_count;
      rej[p] = keep ? 0 : 1;
    }
  }
  __syncthreads();
  const uint32_t t0 = (uint32_t)(lo - wlo), t1 = (uint32_t)(hi - wlo);   // the tile inside the window
#pragma unroll
  for (int it = 0; it < kSelPer; ++it) {
    const uint32_t p = threadIdx.x + it * kThreads;
    if (p >= (uint32_t)kSelWin) break;   // the same for a whole wave
    const bool mine = p >= t0 && p < t1;
    const uint8_t f = fl[p];
    const bool out = mine && !(f & 2) && rej[last[it]];
    if (mine) {
      MTBLX_CHK(flag + wlo + p, 1);
      flag[wlo + p] = (uint8_t)(out ? f | 2 : f);
    }
    const uint64_t recs = __ballot(out), heads = __ballot(out && (f & 1));
    if ((threadIdx.x & 63u) == 0 && recs) {
      atomicAdd(&cnt[0], (uint32_t)__popcll(heads));
      atomicAdd(&cnt[1], (uint32_t)__popcll(recs));
    }
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    MTBLX_CHK(part + 2ull * blockIdx.x + threadIdx.x, 8);
    part[2ull * blockIdx.x + threadIdx.x] = cnt[threadIdx.x];
  }
}

// The rule as k_group_select takes it (min_count 0 reads as 1), or false: a bit at or above nsrc, a
// source both required and excluded, max_count outside 1..64, max(min_count, 1) > max_count
inline bool select_rule(const mtblx_select* sel, uint32_t nsrc, mtblx_select* out) {
  const uint64_t all = nsrc >= 64 ? ~0ull : (1ull << nsrc) - 1;
  const uint32_t mn = sel->min_count ? sel->min_count : 1u;
  if (((sel->require | sel->exclude) & ~all) || (sel->require & sel->exclude)) return false;
  if (sel->max_count == 0 || sel->max_count > MTBLX_MERGE_MAX_SOURCES || mn > sel->max_count) return false;
  *out = mtblx_select{sel->require, sel->exclude, mn, sel->max_count};
  return true;
}

struct Contrib {
  uint64_t c[kChan];
};

__device__ __forceinline__ Contrib contrib(const SrcTab& t, const Handle* h, const uint8_t* flag, uint64_t i,
                                           uint32_t n) {
  Contrib r{};
  if (i >= n) return r;
  MTBLX_CHK(flag + i, 1);
  const uint8_t f = flag[i];
  if (f & 2) return r;
  const Handle c = h[i];
  uint64_t vs;
  const uint64_t vlen = val_len(t, c.src, c.idx, &vs);
  const bool head = f & 1, tail = i + 1 == n || (flag[i + 1] & 1);
  r.c[0] = head;
  r.c[1] = head ? key_of(t, c.src, c.idx).len : 0;
  r.c[2] = 1;
  r.c[3] = vlen;
  r.c[4] = head ? vlen : 0;
  r.c[5] = tail ? vlen : 0;
  return r;
}

__global__ void __launch_bounds__(kThreads) k_group_sums(SrcTab t, const Handle* h, const uint8_t* flag,
                                                         uint64_t* tiles, uint32_t n) {
  __shared__ uint64_t wsum[kThreads / 64];
  uint64_t s[kChan] = {};
  const uint64_t i0 = (uint64_t)blockIdx.x * kTile + (uint64_t)threadIdx.x * kPer;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const Contrib c = contrib(t, h, flag, i0 + k, n);
#pragma unroll
    for (int q = 0; q < kChan; ++q) s[q] += c.c[q];
  }
#pragma unroll
  for (int q = 0; q < kChan; ++q) {
    uint64_t tot;
    (void)block_scan(s[q], wsum, &tot);
    if (threadIdx.x == 0) {
      MTBLX_CHK(tiles + (uint64_t)blockIdx.x * kChan + q, 8);
      tiles[(uint64_t)blockIdx.x * kChan + q] = tot;
    }
  }
}

// one workgroup: the tile sums -> their exclusive prefixes (in place), the totals, the planned mark.
// selpart (NULL: no selection ran): k_group_select's two words per tile, added up into the header
__global__ void __launch_bounds__(kThreads) k_group_scan(uint64_t* hdr, uint64_t* tiles, uint32_t ntiles, uint32_t n,
                                                         uint64_t planned, const uint64_t* selpart) {
  __shared__ uint64_t wsum[kThreads / 64];
  uint64_t carry[kChan] = {};
  uint64_t left[2] = {};   // the groups a selection left out, the records in them
  for (uint32_t b = 0; b < ntiles; b += kThreads) {
    const uint32_t i = b + threadIdx.x;
    if (selpart) {   // the same for the whole workgroup
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if (i < ntiles) MTBLX_CHK(selpart + 2ull * i + q, 8);
        uint64_t tot;
        (void)block_scan(i < ntiles ? selpart[2ull * i + q] : 0, wsum, &tot);
        left[q] += tot;
      }
    }
#pragma unroll
    for (int q = 0; q < kChan; ++q) {
      if (i < ntiles) MTBLX_CHK(tiles + (uint64_t)i * kChan + q, 8);
      const uint64_t v = i < ntiles ? tiles[(uint64_t)i * kChan + q] : 0;
      uint64_t tot;
      const uint64_t e = block_scan(v, wsum, &tot);
      if (i < ntiles) tiles[(uint64_t)i * kChan + q] = carry[q] + e;
      carry[q] += tot;
    }
  }
  if (threadIdx.x == 0) {
    MTBLX_CHK(hdr, 8 * H_WORDS);
    hdr[H_GROUPS] = carry[0];
    hdr[H_KEYB] = carry[1];
    hdr[H_NVAL] = carry[2];
    hdr[H_VALB] = carry[3];
    hdr[H_DROPPED] = (uint64_t)n - carry[2] - left[1];   // the quirk's drops alone
    hdr[H_SELGROUPS] = left[0];
    hdr[H_SELRECS] = left[1];
    hdr[H_FIRSTB] = carry[4];
    hdr[H_LASTB] = carry[5];
    hdr[H_PLANNED] = planned;
  }
}

struct GroupOut {
  uint32_t* gi;     // group of record i
  uint32_t* vi;     // kept records before i (its slot in the grouped value list)
  uint64_t* koff;   // key bytes of the groups before i's
  uint64_t* voff;   // value bytes of the kept records before i
  uint64_t* foff;   // first-value bytes of the groups before i's
  uint64_t* loff;   // last-value bytes of the groups ending before i
};

__global__ void __launch_bounds__(kThreads) k_group_apply(SrcTab t, const Handle* h, const uint8_t* flag,
                                                          const uint64_t* tiles, GroupOut g, uint32_t n) {
  __shared__ uint64_t wsum[kThreads / 64];
  Contrib c[kPer];
  uint64_t s[kChan] = {};
  const uint64_t i0 = (uint64_t)blockIdx.x * kTile + (uint64_t)threadIdx.x * kPer;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    c[k] = contrib(t, h, flag, i0 + k, n);
#pragma unroll
    for (int q = 0; q < kChan; ++q) s[q] += c[k].c[q];
  }
  uint64_t e[kChan];
#pragma unroll
  for (int q = 0; q < kChan; ++q) {
    uint64_t tot;
    e[q] = block_scan(s[q], wsum, &tot) + tiles[(uint64_t)blockIdx.x * kChan + q];
  }
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const uint64_t i = i0 + k;
    if (i < n) {
      MTBLX_CHK(g.gi + i, 4);
      MTBLX_CHK(g.vi + i, 4);
      MTBLX_CHK(g.koff + i, 8);
      MTBLX_CHK(g.voff + i, 8);
      MTBLX_CHK(g.foff + i, 8);
      MTBLX_CHK(g.loff + i, 8);
      g.gi[i] = (uint32_t)(e[0] + c[k].c[0]) - 1u;   // heads up to and including i, minus one
      g.vi[i] = (uint32_t)e[2];
      g.koff[i] = e[1];
      g.voff[i] = e[3];
      g.foff[i] = e[4];
      g.loff[i] = e[5];
    }
#pragma unroll
    for (int q = 0; q < kChan; ++q) e[q] += c[k].c[q];
  }
}

// ---- emit ----
__global__ void __launch_bounds__(kThreads) k_merge_emit(SrcTab t, const uint64_t* hdr, const Handle* h,
                                                         const uint8_t* flag, GroupOut g, mtblx_merged o, int mode,
                                                         uint32_t n, uint64_t planned) {
  if (hdr[H_PLANNED] != planned) {   // not the workspace of a successful plan over these sources
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(o.flags, MTBLX_MERGE_NOT_PLANNED);
    return;
  }
  const uint32_t grp = threadIdx.x >> 4, l = threadIdx.x & 15;
  const uint64_t tile0 = (uint64_t)blockIdx.x * kEmitTile;
  for (uint32_t it = 0; it < (uint32_t)kEmitTile / 16; ++it) {
    const uint64_t i = tile0 + it * 16 + grp;
    if (i >= n) break;
    const uint8_t f = flag[i];
    if (f & 2) continue;
    const bool head = f & 1, tail = i + 1 == n || (flag[i + 1] & 1);
    const Handle c = h[i];
    const uint64_t gi = g.gi[i];
    bool over = false;
    if (head) {
      const Key k = key_of(t, c.src, c.idx);
      const uint64_t off = g.koff[i];
      if (off + k.len <= o.keys_cap) copy16(o.keys + off, k.p, k.len, l); else over = true;
      if (8 * (gi + 1) <= o.key_end_cap) {
        if (l == 0) {
          MTBLX_CHK(o.key_end + gi, 8);
          o.key_end[gi] = off + k.len;
        }
      } else over = true;
    }
    uint64_t vs;
    const uint64_t vlen = val_len(t, c.src, c.idx, &vs);
    const uint8_t* vp = t.s[c.src].vals + vs;
    bool copy = true, end = tail;
    uint64_t off = g.voff[i], slot = gi;
    if (mode == MTBLX_MERGE_GROUPS) {
      slot = g.vi[i];
      end = true;
      if (tail) {
        if (8 * (gi + 1) <= o.grp_end_cap) {
          if (l == 0) {
            MTBLX_CHK(o.grp_end + gi, 8);
            o.grp_end[gi] = slot + 1;
          }
        } else over = true;
      }
    } else if (mode == MTBLX_MERGE_FIRST) {
      copy = end = head;
      off = g.foff[i];
    } else if (mode == MTBLX_MERGE_LAST) {
      copy = end = tail;
      off = g.loff[i];
    } else if (mode == kEmitSingles) {
      copy = head && tail;
      end = false;
      if (copy) {
        if (8 * (gi + 1) <= o.val_end_cap) {
          off = 0;
          if (gi) {
            MTBLX_CHK(o.val_end + gi - 1, 8);
            off = o.val_end[gi - 1];
          }
        } else {
          copy = false;
          over = true;
        }
      }
    }
    if (copy) {
      if (off + vlen <= o.vals_cap) copy16(o.vals + off, vp, vlen, l); else over = true;
    }
    if (end) {
      if (8 * (slot + 1) <= o.val_end_cap) {
        if (l == 0) {
          MTBLX_CHK(o.val_end + slot, 8);
          o.val_end[slot] = off + vlen;
        }
      } else over = true;
    }
    if (over && l == 0) atomicOr(o.flags, MTBLX_MERGE_OVERFLOW);
  }
}

// ---- host side ----
struct Layout {
  size_t hdr, h0, h1, flag, gi, vi, koff, voff, foff, loff, tiles, edges, vtiles, total;
  uint32_t ntiles;
};

Layout layout(uint64_t n) {
  Layout L{};
  L.ntiles = (uint32_t)((n + kTile - 1) / kTile);
  size_t p = 0;
  L.hdr = p; p += up256(8 * H_WORDS);
  L.h0 = p; p += up256(16 * n);
  L.h1 = p; p += up256(16 * n);
  L.flag = p; p += up256(n + 16);
  L.gi = p; p += up256(4 * n);
  L.vi = p; p += up256(4 * n);
  L.koff = p; p += up256(8 * n);
  L.voff = p; p += up256(8 * n);
  L.foff = p; p += up256(8 * n);
  L.loff = p; p += up256(8 * n);
  L.tiles = p; p += up256(8ull * kChan * L.ntiles);
  L.edges = p; p += up256(8ull * kReduceEdgeWords * L.ntiles);   // the reducers' per-tile edge records (reduce_dev.h)
  L.vtiles = p; p += up256(8ull * L.ntiles);   // the varint reduce emit's per-tile sums of val_end (reduce_dev.h)
  L.total = p;
  return L;
}

uint32_t passes_for(uint32_t nruns) {   // ceil(log2) of the level-0 runs: sources (merge), tiles (sort: <= 2^22)
  uint32_t p = 0;
  while ((1u << p) < nruns) ++p;
  return p;
}

// -> N, or UINT64_MAX if the sources break the limits
uint64_t fill_tab(const mtblx_records* src, uint32_t nsrc, SrcTab* t) {
  memset(t, 0, sizeof(*t));
  t->nsrc = nsrc;
  uint64_t n = 0;
  for (uint32_t i = 0; i < nsrc; ++i) {
    t->s[i] = src[i];
    t->base[i] = (uint32_t)n;
    if (src[i].n >= MTBLX_MERGE_MAX_RECORDS) return UINT64_MAX;
    // keys / vals may be NULL where every key / value of the source is empty
    if (src[i].n && (!src[i].key_end || !src[i].val_end)) return UINT64_MAX;
    n += src[i].n;
    if (n >= MTBLX_MERGE_MAX_RECORDS) return UINT64_MAX;
  }
  for (uint32_t i = nsrc; i <= MTBLX_MERGE_MAX_SOURCES; ++i) t->base[i] = (uint32_t)n;
  return n;
}

struct PhaseEvents {   // phase boundaries of a plan, recorded only when timing (the *_plan_timed calls)
  hipEvent_t e[40];    // the merge marks <= 9, the sort <= 3 + 22 passes
  uint32_t n = 0;
  bool on;
  explicit PhaseEvents(bool o) : on(o) {}
  void mark(hipStream_t st) {
    if (on && n < sizeof(e) / sizeof(e[0]) && hipEventCreate(&e[n]) == hipSuccess) (void)hipEventRecord(e[n++], st);
  }
  void read(float* phase_ms, uint32_t phase_cap) const {
    for (uint32_t i = 0; i < phase_cap; ++i) phase_ms[i] = 0.f;
    for (uint32_t i = 0; i + 1 < n && i < phase_cap; ++i) (void)hipEventElapsedTime(&phase_ms[i], e[i], e[i + 1]);
  }
  ~PhaseEvents() {
    for (uint32_t i = 0; i < n; ++i) (void)hipEventDestroy(e[i]);
  }
};

GroupOut group_out(uint8_t* w, const Layout& L) {
  return GroupOut{reinterpret_cast<uint32_t*>(w + L.gi),   reinterpret_cast<uint32_t*>(w + L.vi),
                  reinterpret_cast<uint64_t*>(w + L.koff), reinterpret_cast<uint64_t*>(w + L.voff),
                  reinterpret_cast<uint64_t*>(w + L.foff), reinterpret_cast<uint64_t*>(w + L.loff)};
}

}  // namespace

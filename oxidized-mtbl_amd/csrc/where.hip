// where.hip — value predicates on the MI355X (gfx950): records kept or dropped by the fields of
// their value (include/mtblx.h "Value predicates", DESIGN.md §4 "Value predicates").
//
// A value holds F fields in the layout of a reduce spec (F little-endian u64 words, or F varints back
// to back); an mtblx_where puts at most one inclusive range on each field, inside or outside.  A
// value that is not well-formed is BAD: its record is dropped and counted, never kept.
//
// The plan (mtblx_where_plan):
//   k_where_segcheck  a thread per entry of seg_off: 0 = off[0] <= ... <= off[nseg] = n, else
//                     MTBLX_WHERE_BADSEG in the workspace header and every later kernel returns
//   k_where_eval      a workgroup owns kWhereTile consecutive records, kWherePer per thread: the
//                     value is decoded where it lies (any alignment; reduce_ops.h's loader for the
//                     varints), the predicate evaluated ONCE, bit 0 (keep) / bit 1 (bad) left in
//                     flag[r], and the tile's four sums {kept, kept key bytes, kept value bytes, bad}
//   k_where_scan      one workgroup: the tile sums -> exclusive prefixes in place, the totals to the
//                     header, the planned mark
//   k_where_segs      a thread per segment: the kept / bad records before record seg_off[q] are the
//                     prefix of its tile plus the flags of the tile's records before it (8 flags per
//                     load, two popcounts) -> seg_end[q], seg_bad[q]
// then one read-back of the header.  The emit (mtblx_where_emit), gated on the mark, the flag and the
// capacities:
//   k_where_emit      the tile's scan again over the flags: kept record e writes key_end[e],
//                     val_end[e], src_idx[e].  Adjacent kept records are contiguous in the source, so
//                     the tile's kept bytes are a few RUNS; their (destination, source) offsets go to
//                     LDS and the whole workgroup moves the tile's bytes 16 at a time by destination
//                     address (a search over the runs per 16 bytes; one 16-byte load and one aligned
//                     16-byte store where the 16 bytes lie in one run, bytes elsewhere).  One key of
//                     70 000 bytes is 4 375 such steps over 256 lanes, not one lane's loop.
// Every kernel is its own launch and no workgroup waits for another; one segment of a million
// records costs what a million segments cost.  All positions are 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bounds.h"
#include "lane_dev.h"
#include "mtblx.h"
#include "reduce_ops.h"

namespace {

constexpr int kWhereTile = 1024;                 // records per workgroup, 4 per thread
constexpr int kWherePer = kWhereTile / kThreads;
static_assert(kWherePer * kThreads == kWhereTile, "tile");
static_assert(kWhereTile % 8 == 0, "k_where_segs reads the flags of a tile 8 at a time");
enum { WH_KEPT = 0, WH_KEYB, WH_VALB, WH_BAD, WH_REJ, WH_FLAGS, WH_PLANNED, WH_WORDS = 32 };
enum { WF_KEEP = 1, WF_BAD = 2 };
constexpr uint64_t kWhereMagic = 0x4d54424c58574852ull;   // "MTBLXWHR"
typedef uint64_t wu64u __attribute__((aligned(1)));

struct WSpec {   // a checked mtblx_where; travels in the kernel arguments, indexed by unrolled loops only
  uint64_t lo[MTBLX_REDUCE_MAX_FIELDS], hi[MTBLX_REDUCE_MAX_FIELDS];
  uint32_t mask, outside, any;
};

// the contract of include/mtblx.h for one well-formed value
template <int F>
__device__ __forceinline__ bool where_keeps(const WSpec& w, const uint64_t* v) {
  uint32_t pass = 0;
#pragma unroll
  for (int f = 0; f < F; ++f) {
    const bool in = w.lo[f] <= v[f] && v[f] <= w.hi[f];
    if (in != (bool)((w.outside >> f) & 1u)) pass |= 1u << f;
  }
  pass &= w.mask;
  return w.any ? pass != 0 : pass == w.mask;
}

// [*start, *start + the result) of END offsets `end`; offsets that step back give an empty span
__device__ __forceinline__ uint64_t span_of(const uint64_t* end, uint64_t r, uint64_t* start) {
  uint64_t s = 0;
  if (r) {
    MTBLX_CHK(end + r - 1, 8);
    s = end[r - 1];
  }
  MTBLX_CHK(end + r, 8);
  const uint64_t e = end[r];
  *start = s;
  return e >= s ? e - s : 0;
}

__global__ void __launch_bounds__(kThreads) k_where_segcheck(const uint64_t* seg_off, uint32_t nseg, uint64_t n,
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
  if (bad) atomicOr(reinterpret_cast<unsigned long long*>(hdr + WH_FLAGS), (unsigned long long)MTBLX_WHERE_BADSEG);
}

template <int F, int ENC>
__global__ void __launch_bounds__(kThreads) k_where_eval(mtblx_records rec, WSpec w, uint8_t* flag, uint64_t* tiles,
                                                         const uint64_t* hdr) {
  if (hdr[WH_FLAGS] & MTBLX_WHERE_BADSEG) return;
  __shared__ uint64_t wsum[kThreads / 64];
  constexpr uint64_t W = 8u * F;
  const uint64_t i0 = (uint64_t)blockIdx.x * kWhereTile + (uint64_t)threadIdx.x * kWherePer;
  uint64_t s[4] = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < kWherePer; ++k) {
    const uint64_t i = i0 + k;
    if (i >= rec.n) continue;
    MTBLX_CHK(rec.val_end + i, 8);
    uint64_t vs = 0;
    if (i) {
      MTBLX_CHK(rec.val_end + i - 1, 8);
      vs = rec.val_end[i - 1];
    }
    const uint64_t vlen = rec.val_end[i] - vs;   // END offsets that step back: a huge length, a bad value
    const uint8_t* vp = rec.vals + vs;           // any alignment
    uint64_t v[F];
    bool ok;
    if (ENC == R_VARINT) {
      ok = r_load_varint<F, true>(vp, vlen, v);
    } else {
      ok = vlen == W;
      if (ok) {
        MTBLX_CHK(vp, W);
#pragma unroll
        for (int f = 0; f < F; ++f) v[f] = *reinterpret_cast<const wu64u*>(vp + 8 * f);
      }
    }
    const bool keep = ok && where_keeps<F>(w, v);
    MTBLX_CHK(flag + i, 1);
    flag[i] = keep ? WF_KEEP : ok ? 0 : WF_BAD;
    if (keep) {
      uint64_t ks;
      s[0] += 1;
      s[1] += span_of(rec.key_end, i, &ks);
      s[2] += vlen;
    }
    if (!ok) s[3] += 1;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    uint64_t tot;
    (void)block_scan(s[j], wsum, &tot);
    if (threadIdx.x == 0) {
      MTBLX_CHK(tiles + 4ull * blockIdx.x + j, 8);
      tiles[4ull * blockIdx.x + j] = tot;
    }
  }
}

// one workgroup: the tile sums -> their exclusive prefixes (in place), the totals, the planned mark.
// After a bad seg_off the totals are zero and the mark is still set: the emit then reports the flag
__global__ void __launch_bounds__(kThreads) k_where_scan(uint64_t* hdr, uint64_t* tiles, uint32_t ntiles, uint64_t n,
                                                         uint64_t planned) {
  __shared__ uint64_t wsum[kThreads / 64];
  const bool bad = hdr[WH_FLAGS] & MTBLX_WHERE_BADSEG;
  uint64_t carry[4] = {0, 0, 0, 0};
  for (uint32_t b = 0; !bad && b < ntiles; b += kThreads) {
    const uint32_t i = b + threadIdx.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (i < ntiles) MTBLX_CHK(tiles + 4ull * i + j, 8);
      const uint64_t v = i < ntiles ? tiles[4ull * i + j] : 0;
      uint64_t tot;
      const uint64_t e = block_scan(v, wsum, &tot);
      if (i < ntiles) tiles[4ull * i + j] = carry[j] + e;
      carry[j] += tot;
    }
  }
  if (threadIdx.x == 0) {
    MTBLX_CHK(hdr, 8 * WH_WORDS);
    hdr[WH_KEPT] = carry[0];
    hdr[WH_KEYB] = carry[1];
    hdr[WH_VALB] = carry[2];
    hdr[WH_BAD] = carry[3];
    hdr[WH_REJ] = bad ? 0 : n - carry[0] - carry[3];
    hdr[WH_PLANNED] = planned;
  }
}

// the kept and the bad records before record r <= n: the tile's prefix and the flags of the tile's
// records before r.  flag is 256-byte aligned and a tile begins at a multiple of 8 flags; the bytes
// of a word at or past r are masked out, so flags past n (never written) do not count
__device__ __forceinline__ void where_before(const uint64_t* hdr, const uint64_t* tiles, const uint8_t* flag, uint64_t r,
                                             uint64_t n, uint64_t* kept, uint64_t* bad) {
  if (r >= n) {
    *kept = hdr[WH_KEPT];
    *bad = hdr[WH_BAD];
    return;
  }
  const uint64_t t = r / kWhereTile;
  MTBLX_CHK(tiles + 4 * t, 32);
  uint64_t k = tiles[4 * t], b = tiles[4 * t + 3];
  for (uint64_t p = t * kWhereTile; p < r; p += 8) {
    MTBLX_CHK(flag + p, 8);
    uint64_t x = *reinterpret_cast<const uint64_t*>(flag + p);
    if (r - p < 8) x &= (1ull << (8 * (r - p))) - 1;
    k += __popcll(x & 0x0101010101010101ull);
    b += __popcll(x & 0x0202020202020202ull);
  }
  *kept = k;
  *bad = b;
}

__global__ void __launch_bounds__(kThreads) k_where_segs(const uint64_t* seg_off, uint32_t nseg, uint64_t n,
                                                         const uint64_t* hdr, const uint64_t* tiles, const uint8_t* flag,
                                                         uint64_t* seg_end, uint64_t* seg_bad) {
  if (hdr[WH_FLAGS] & MTBLX_WHERE_BADSEG) return;
  const uint64_t q = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (q >= nseg) return;
  MTBLX_CHK(seg_off + q, 16);
  uint64_t k1, b1;
  where_before(hdr, tiles, flag, seg_off[q + 1], n, &k1, &b1);   // the check has passed: both are <= n
  MTBLX_CHK(seg_end + q, 8);
  seg_end[q] = k1;
  if (seg_bad) {
    uint64_t k0, b0;
    where_before(hdr, tiles, flag, seg_off[q], n, &k0, &b0);
    MTBLX_CHK(seg_bad + q, 8);
    seg_bad[q] = b1 - b0;
  }
}

// ---- emit ----
// the gate the emit kernel passes: the workspace is that of a plan over this record count, the plan
// met no bad seg_off, and every output holds the totals.  `tell`: the one thread that reports
__device__ __forceinline__ bool where_gate(const uint64_t* hdr, const mtblx_filtered& o, uint64_t planned, bool tell) {
  uint32_t f = 0;
  if (hdr[WH_PLANNED] != planned) {
    f = MTBLX_WHERE_NOT_PLANNED;
  } else if (hdr[WH_FLAGS] & MTBLX_WHERE_BADSEG) {
    f = MTBLX_WHERE_BADSEG;
  } else if (hdr[WH_KEYB] > o.keys_cap || hdr[WH_VALB] > o.vals_cap || hdr[WH_KEPT] > o.rec_cap) {
    f = MTBLX_WHERE_OVERFLOW;
  }
  if (f && tell) atomicOr(o.flags, f);
  return f == 0;
}

// The workgroup moves B bytes to d[0 .. B): byte x comes from s[run_src[r] + x - run_dst[r]] for the
// run r with run_dst[r] <= x < run_dst[r + 1] (run_dst[0] = 0, run_dst[nruns] = B, both in LDS; empty
// runs are legal).  The steps are the 16-byte lines of d's ADDRESS: a line inside one run is one
// unaligned 16-byte load and one aligned 16-byte store, any other goes by bytes
__device__ __forceinline__ void run_copy(uint8_t* d, const uint8_t* s, uint64_t B, const uint64_t* run_dst,
                                         const uint64_t* run_src, uint32_t nruns) {
  if (B == 0) return;
  const uint64_t lead = (uint64_t)((uintptr_t)d & 15u);
  const uint64_t nlines = (B + lead + 15) >> 4;
  for (uint64_t c = threadIdx.x; c < nlines; c += kThreads) {
    const uint64_t x0 = c ? 16 * c - lead : 0;
    const uint64_t x1 = 16 * c - lead + 16 < B ? 16 * c - lead + 16 : B;   // c == 0: 16 - lead, no wrap
    uint32_t lo = 0, hi = nruns;   // the runs that begin at or before x0: at least one
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (run_dst[mid] <= x0) lo = mid + 1;
      else hi = mid;
    }
    uint32_t r = lo - 1;
    uint64_t rend = run_dst[r + 1];
    if (x1 - x0 == 16 && rend >= x1) {
      const uint8_t* sp = s + run_src[r] + (x0 - run_dst[r]);
      MTBLX_CHK(sp, 16);
      MTBLX_CHK(d + x0, 16);
      *reinterpret_cast<v4u*>(d + x0) = *reinterpret_cast<const v4uu*>(sp);
      continue;
    }
    for (uint64_t x = x0; x < x1; ++x) {
      while (x >= rend) {   // x < B = run_dst[nruns]: r stays below nruns
        ++r;
        rend = run_dst[r + 1];
      }
      const uint8_t* sp = s + run_src[r] + (x - run_dst[r]);
      MTBLX_CHK(sp, 1);
      MTBLX_CHK(d + x, 1);
      d[x] = *sp;
    }
  }
}

__global__ void __launch_bounds__(kThreads) k_where_emit(mtblx_records rec, const uint8_t* flag, const uint64_t* tiles,
                                                         const uint64_t* hdr, mtblx_filtered o, uint64_t planned) {
  if (!where_gate(hdr, o, planned, blockIdx.x == 0 && threadIdx.x == 0)) return;
  __shared__ uint64_t wsum[kThreads / 64];
  __shared__ uint64_t run_dst[kWhereTile + 1], run_src[kWhereTile];
  const uint64_t n = rec.n;
  const uint64_t tile0 = (uint64_t)blockIdx.x * kWhereTile;
  const uint64_t i0 = tile0 + (uint64_t)threadIdx.x * kWherePer;
  // the thread's records; prev / prev_cut: the record before the thread's first was kept / its key
  // offsets stepped back (its key is then empty and the next key does not continue it)
  bool keep[kWherePer], khead[kWherePer], vhead[kWherePer];
  uint64_t ks[kWherePer], kl[kWherePer], vs[kWherePer], vl[kWherePer];
  bool prev = false, prev_cut = false;
  if (threadIdx.x && i0 < n) {
    MTBLX_CHK(flag + i0 - 1, 1);
    prev = flag[i0 - 1] & WF_KEEP;
    if (prev && i0 >= 2) {
      MTBLX_CHK(rec.key_end + i0 - 2, 16);
      prev_cut = rec.key_end[i0 - 1] < rec.key_end[i0 - 2];
    }
  }
  uint64_t s[5] = {0, 0, 0, 0, 0};   // kept, key bytes, value bytes, key runs, value runs
#pragma unroll
  for (int k = 0; k < kWherePer; ++k) {
    const uint64_t i = i0 + k;
    keep[k] = khead[k] = vhead[k] = false;
    ks[k] = kl[k] = vs[k] = vl[k] = 0;
    if (i < n) {
      MTBLX_CHK(flag + i, 1);
      keep[k] = flag[i] & WF_KEEP;
    }
    bool cut = false;
    if (keep[k]) {
      kl[k] = span_of(rec.key_end, i, &ks[k]);
      vl[k] = span_of(rec.val_end, i, &vs[k]);   // a kept value is well-formed: no step back
      MTBLX_CHK(rec.key_end + i, 8);
      cut = rec.key_end[i] < ks[k];
      khead[k] = !prev || prev_cut;
      vhead[k] = !prev;
      s[0] += 1;
      s[1] += kl[k];
      s[2] += vl[k];
      s[3] += khead[k];
      s[4] += vhead[k];
    }
    prev = keep[k];
    prev_cut = cut;
  }
  uint64_t e[5], tot[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) e[j] = block_scan(s[j], wsum, &tot[j]);
  MTBLX_CHK(tiles + 4ull * blockIdx.x, 32);
  const uint64_t base_rec = tiles[4ull * blockIdx.x], base_kb = tiles[4ull * blockIdx.x + 1],
                 base_vb = tiles[4ull * blockIdx.x + 2];
  // the ends, and the key runs.  base + e < the totals: the gate has checked the capacities
  {
    uint64_t er = e[0], ek = e[1], ev = e[2], rk = e[3];
#pragma unroll
    for (int k = 0; k < kWherePer; ++k) {
      if (!keep[k]) continue;
      MTBLX_CHK(o.key_end + base_rec + er, 8);
      MTBLX_CHK(o.val_end + base_rec + er, 8);
      o.key_end[base_rec + er] = base_kb + ek + kl[k];
      o.val_end[base_rec + er] = base_vb + ev + vl[k];
      if (o.src_idx) {
        MTBLX_CHK(o.src_idx + base_rec + er, 8);
        o.src_idx[base_rec + er] = i0 + k;
      }
      if (khead[k]) {
        run_dst[rk] = ek;
        run_src[rk] = ks[k];
        ++rk;
      }
      ++er;
      ek += kl[k];
      ev += vl[k];
    }
  }
  if (threadIdx.x == 0) run_dst[tot[3]] = tot[1];
  __syncthreads();
  run_copy(o.keys + base_kb, rec.keys, tot[1], run_dst, run_src, (uint32_t)tot[3]);
  __syncthreads();
  {
    uint64_t ev = e[2], rv = e[4];
#pragma unroll
    for (int k = 0; k < kWherePer; ++k) {
      if (!keep[k]) continue;
      if (vhead[k]) {
        run_dst[rv] = ev;
        run_src[rv] = vs[k];
        ++rv;
      }
      ev += vl[k];
    }
  }
  if (threadIdx.x == 0) run_dst[tot[4]] = tot[2];
  __syncthreads();
  run_copy(o.vals + base_vb, rec.vals, tot[2], run_dst, run_src, (uint32_t)tot[4]);
}

// n == 0: nothing to write, but the gate still reports
__global__ void k_where_gate0(const uint64_t* hdr, mtblx_filtered o, uint64_t planned) {
  (void)where_gate(hdr, o, planned, threadIdx.x == 0);
}

struct WhereLayout {
  size_t flag, tiles, total;
  uint32_t ntiles;
};

WhereLayout where_layout(uint64_t n) {
  WhereLayout L{};
  L.ntiles = (uint32_t)((n + kWhereTile - 1) / kWhereTile);
  L.flag = 8 * WH_WORDS;
  L.tiles = L.flag + up256(n + 8);   // k_where_segs reads whole words of flags
  L.total = L.tiles + up256(32ull * L.ntiles);
  return L;
}

// the mark of a plan over n records: an emit over another count, or over the workspace of any other
// call, finds another word in the header
uint64_t where_mark(uint64_t n) {
  const uint64_t h = ((kWhereMagic ^ n) * 0x9E3779B97F4A7C15ull) + 0x57484552ull;
  return h | 1u;   // never the zero the plan leaves in a cleared header
}

WSpec wspec_of(const mtblx_where& w) {
  WSpec s{};
  for (uint32_t f = 0; f < MTBLX_REDUCE_MAX_FIELDS; ++f) {
    s.lo[f] = w.lo[f];
    s.hi[f] = w.hi[f];
  }
  s.mask = w.mask;
  s.outside = w.outside;
  s.any = w.flags & MTBLX_WHERE_ANY;
  return s;
}

template <int F, int ENC>
void eval_launch_e(const mtblx_records& rec, const WSpec& w, uint8_t* flag, uint64_t* tiles, const uint64_t* hdr,
                   const WhereLayout& L, hipStream_t s) {
  MTBLX_LAUNCH((MTBLX_R(rec.val_end, 8 * rec.n), MTBLX_R(rec.key_end, 8 * rec.n), rec.vals, MTBLX_R(flag, rec.n),
                MTBLX_R(tiles, 32ull * L.ntiles), MTBLX_R(hdr, 8 * WH_WORDS)),
               (k_where_eval<F, ENC>), dim3(L.ntiles), dim3(kThreads), 0, s, rec, w, flag, tiles, hdr);
}

template <int F>
void eval_launch(bool varint, const mtblx_records& rec, const WSpec& w, uint8_t* flag, uint64_t* tiles,
                 const uint64_t* hdr, const WhereLayout& L, hipStream_t s) {
  if (varint) eval_launch_e<F, R_VARINT>(rec, w, flag, tiles, hdr, L, s);
  else eval_launch_e<F, R_U64LE>(rec, w, flag, tiles, hdr, L, s);
}

}  // namespace

extern "C" uint32_t mtblx_where_tile(void) { return (uint32_t)kWhereTile; }

extern "C" size_t mtblx_where_impl_ws_bytes(uint64_t n) { return where_layout(n).total; }

// arguments already checked (mtblx_api.cpp).  Synchronous: totals is host memory
extern "C" int mtblx_where_impl_plan(const mtblx_records* recs, const mtblx_where* where, const uint64_t* seg_off,
                                     uint32_t nseg, uint64_t* totals, uint64_t* seg_end, uint64_t* seg_bad, void* ws,
                                     hipStream_t s) {
  const mtblx_records rec = *recs;
  const uint64_t n = rec.n;
  const WhereLayout L = where_layout(n);
  uint8_t* w = static_cast<uint8_t*>(ws);
  uint64_t* hdr = reinterpret_cast<uint64_t*>(w);
  uint8_t* flag = w + L.flag;
  uint64_t* tiles = reinterpret_cast<uint64_t*>(w + L.tiles);
  const WSpec sp = wspec_of(*where);
  const bool varint = where->flags & MTBLX_WHERE_VARINT;
  if (hipMemsetAsync(hdr, 0, 8 * WH_WORDS, s) != hipSuccess) return MTBLX_E_HIP;
  if (nseg)
    MTBLX_LAUNCH((MTBLX_R(seg_off, 8ull * nseg + 8), MTBLX_R(hdr, 8 * WH_WORDS)), k_where_segcheck,
                 dim3((unsigned)(((uint64_t)nseg + kThreads) / kThreads)), dim3(kThreads), 0, s, seg_off, nseg, n, hdr);
  if (n) {
    switch (where->nfields) {
      case 1: eval_launch<1>(varint, rec, sp, flag, tiles, hdr, L, s); break;
      case 2: eval_launch<2>(varint, rec, sp, flag, tiles, hdr, L, s); break;
      case 3: eval_launch<3>(varint, rec, sp, flag, tiles, hdr, L, s); break;
      case 4: eval_launch<4>(varint, rec, sp, flag, tiles, hdr, L, s); break;
      case 5: eval_launch<5>(varint, rec, sp, flag, tiles, hdr, L, s); break;
      case 6: eval_launch<6>(varint, rec, sp, flag, tiles, hdr, L, s); break;
      case 7: eval_launch<7>(varint, rec, sp, flag, tiles, hdr, L, s); break;
      default: eval_launch<8>(varint, rec, sp, flag, tiles, hdr, L, s); break;
    }
  }
  MTBLX_LAUNCH((MTBLX_R(hdr, 8 * WH_WORDS), MTBLX_R(tiles, 32ull * L.ntiles)), k_where_scan, dim3(1), dim3(kThreads), 0,
               s, hdr, tiles, L.ntiles, n, where_mark(n));
  if (nseg)
    MTBLX_LAUNCH((MTBLX_R(seg_off, 8ull * nseg + 8), MTBLX_R(hdr, 8 * WH_WORDS), MTBLX_R(tiles, 32ull * L.ntiles),
                  MTBLX_R(flag, up256(n + 8)), MTBLX_R(seg_end, 8ull * nseg), MTBLX_R(seg_bad, 8ull * nseg)),
                 k_where_segs, dim3((unsigned)(((uint64_t)nseg + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, seg_off,
                 nseg, n, hdr, tiles, flag, seg_end, seg_bad);
  if (hipGetLastError() != hipSuccess) return MTBLX_E_HIP;
  uint64_t host[WH_WORDS];
  if (hipMemcpyAsync(host, hdr, 8 * WH_WORDS, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return MTBLX_E_HIP;
  for (int i = 0; i < 6; ++i) totals[i] = host[i];
  return (host[WH_FLAGS] & MTBLX_WHERE_BADSEG) ? MTBLX_E_FORMAT : MTBLX_OK;
}

extern "C" int mtblx_where_impl_emit(const mtblx_records* recs, const mtblx_filtered* out, const void* ws,
                                     hipStream_t s) {
  const mtblx_records rec = *recs;
  const uint64_t n = rec.n;
  const WhereLayout L = where_layout(n);
  const uint8_t* w = static_cast<const uint8_t*>(ws);
  const uint64_t* hdr = reinterpret_cast<const uint64_t*>(w);
  const uint8_t* flag = w + L.flag;
  const uint64_t* tiles = reinterpret_cast<const uint64_t*>(w + L.tiles);
  const mtblx_filtered o = *out;
  if (hipMemsetAsync(o.flags, 0, 4, s) != hipSuccess) return MTBLX_E_HIP;
  if (n)
    MTBLX_LAUNCH((MTBLX_R(rec.key_end, 8 * n), MTBLX_R(rec.val_end, 8 * n), rec.keys, rec.vals, MTBLX_R(flag, n),
                  MTBLX_R(tiles, 32ull * L.ntiles), MTBLX_R(hdr, 8 * WH_WORDS), MTBLX_R(o.keys, o.keys_cap),
                  MTBLX_R(o.vals, o.vals_cap), MTBLX_R(o.key_end, 8 * o.rec_cap), MTBLX_R(o.val_end, 8 * o.rec_cap),
                  MTBLX_R(o.src_idx, 8 * o.rec_cap), MTBLX_R(o.flags, 4)),
                 k_where_emit, dim3(L.ntiles), dim3(kThreads), 0, s, rec, flag, tiles, hdr, o, where_mark(n));
  else
    MTBLX_LAUNCH((MTBLX_R(hdr, 8 * WH_WORDS), MTBLX_R(o.flags, 4)), k_where_gate0, dim3(1), dim3(64), 0, s, hdr, o,
                 where_mark(n));
  return hipGetLastError() == hipSuccess ? MTBLX_OK : MTBLX_E_HIP;
}

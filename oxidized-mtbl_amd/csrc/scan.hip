// scan.hip — batched scans on the MI355X (gfx950): Reader::iter_from / get / iter_prefix /
// iter_range for many queries in two launches and one read-back (include/mtblx.h "batched scans",
// DESIGN.md §4 "Batched scans").
//
// Per query the walk is ReaderIntoIter::new_from + next() (src/reader.rs:256-405), restated with
// the helpers of reader_dev.h exactly as k_get (reader.hip) does for its two steps:
//   k_scan_plan     one wave per query, wave-uniform; the lanes share the CRC-32C of every block
//                   the query opens.  No key is materialised: It tracks the common prefix with the
//                   start key (== the stop key of Get / GetPrefix); a range carries a second It
//                   against its end key, fed the same entries.  Counts the records, saves the
//                   landing (index entry, restart index, entry offset) and classifies the query:
//                   OK, LARGE (more than max_blocks Reader::block calls) or FALLBACK (anything
//                   the reference answers with a panic, an Err or never: the exact seek primitives
//                   keep those quirks)
//   k_scan_offsets  one workgroup: exclusive scan of the three counts over the OK queries, the
//                   totals, and the plan's mark
//   k_scan_emit     one wave per OK query, the key in MTBLX_SCAN_MAX_KEY bytes of LDS.  It starts
//                   at the saved landing, follows the index chain, and writes exactly the planned
//                   number of records: no comparison and no checksum is repeated.  Every write is
//                   checked against the query's planned slot and the caller's capacities.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "bounds.h"
#include "devinfo.h"
#include "crc_dev.h"
#include "mtblx.h"
#include "reader_dev.h"
#include "reduce_ops.h"

namespace mtblx_rd {

constexpr uint64_t kScanMagic = 0x6d74626c7363616eull;   // "mtblscan"
constexpr uint64_t kMaxKey = MTBLX_SCAN_MAX_KEY;
enum { H_REC = 0, H_KEY, H_VAL, H_BAD, H_MARK, H_WORDS };

// where the plan's seek landed: the emit starts here
struct Land {
  uint64_t ix_entry;   // offset of the landed index entry in the index block
  uint64_t d_entry;    // offset of the landed entry in the sought block (>= its restart offset: none)
  uint32_t restart;    // the restart interval the data seek walked
  uint32_t pad;
  uint64_t pad2;
};
static_assert(sizeof(Land) == 32, "workspace layout");
static_assert(sizeof(mtblx_scan_result) == 64, "ABI");

struct Layout {
  size_t hdr, type, res, land, total;
};
static inline size_t up256(size_t x) { return (x + 255u) & ~(size_t)255u; }
static inline Layout layout(uint32_t nq) {
  Layout L;
  L.hdr = 0;
  L.type = 256;
  L.res = L.type + up256(4ull * nq);
  L.land = L.res + up256(sizeof(mtblx_scan_result) * (size_t)nq);
  L.total = L.land + up256(sizeof(Land) * (size_t)nq);
  return L;
}
static inline uint64_t planned_mark(uint32_t nq) { return kScanMagic ^ ((uint64_t)nq << 32) ^ nq; }

struct Targets {
  const uint8_t* t;    // the start key: both seeks, and the stop key of Get / GetPrefix
  uint64_t tl;
  const uint8_t* k2;   // GetRange's end key
  uint64_t k2l;
  bool two;            // a range: jt tracks k2
};

// parse_next_key on both trackers: jt sees the same entries, so it ends the same way
__device__ __forceinline__ int step(const Blk& b, It& it, It& jt, const Targets& g) {
  const int r = parse_next_key(b, it, g.t, g.tl);
  if (g.two) (void)parse_next_key(b, jt, g.k2, g.k2l);
  return r;
}

// BlockIter::seek (src/block.rs:154-194) as reader_dev.h's seek(), with the second tracker and the
// restart interval it walked.  R_TOOLONG: a key of the interval is longer than the emit's buffer.
__device__ __forceinline__ int seek2(const Blk& b, It& it, It& jt, const Targets& g, uint32_t& left_out) {
  uint32_t left = 0, right = b.n - 1;
  left_out = 0;
  while (left < right) {
    const uint32_t mid = (uint32_t)(((uint64_t)left + right + 1) / 2);
    uint32_t sh, ns, vl;
    uint64_t ko;
    if (decode_entry(b, restart_point(b, mid), b.R, sh, ns, vl, ko) != R_OK) return R_PANIC;
    if (sh != 0) return R_OK;                                 // "corruption": early return
    if (ko + ns > b.L) return R_PANIC;
    const uint64_t c = match_len(b.d + ko, g.t, ns < g.tl ? ns : g.tl);
    const int r = (c < ns && c < g.tl) ? (b.d[ko + c] < g.t[c] ? -1 : 1) : (ns < g.tl ? -1 : (ns > g.tl ? 1 : 0));
    if (r < 0) left = mid;
    else right = mid - 1;
  }
  left_out = left;
  restart_at(b, it, left);
  jt = it;
  for (uint64_t steps = 0;; ++steps) {
    const uint64_t before = it.current;
    const int r = step(b, it, jt, g);
    if (r != R_OK) return r == R_END ? R_OK : r;
    if (it.klen > kMaxKey) return R_TOOLONG;
    if (cmp_key(it, g.tl) >= 0) return R_OK;
    if (it.next == it.current || (steps > 0 && it.current == before)) return R_LOOP;
  }
}

// the reducing walk's extra arguments (mtblx_scan_reduce): lane f < nf keeps field f's accumulator
struct Red {
  RSpec sp;
  uint32_t nf;
  uint64_t* fields;   // [nq * nf]
  uint64_t* nbad;     // [nq]
};

// what a lane of the reducing walk carries: its op, its accumulator, the values of another length
template <bool ON>
struct RAcc {};
template <>
struct RAcc<true> {
  uint32_t op = 0;
  uint64_t acc = 0, bad = 0;
};
struct RedV : Red {};   // the same with varint-coded values: the encoding is the kernel's template argument
__device__ __forceinline__ const Red& red_of(const Red& r) { return r; }

// the predicate of the fused walk (mtblx_scan_reduce_where): a further trailing argument after the
// Red / RedV.  Lane f < nf keeps field f's bounds beside its accumulator
struct Whr {
  uint64_t lo[MTBLX_REDUCE_MAX_FIELDS], hi[MTBLX_REDUCE_MAX_FIELDS];
  uint32_t mask, outside, any;
  uint64_t* nmatch;   // [nq]
};
__device__ __forceinline__ const Red& red_of(const Red& r, const Whr&) { return r; }
__device__ __forceinline__ const Whr& whr_of(const Red&, const Whr& w) { return w; }
struct WAcc : RAcc<true> {   // what a lane of the fused walk carries: RAcc<true>, and
  uint64_t lo = 0, hi = 0, match = 0;
  bool on = false, outside = false;   // this lane's field is constrained; must lie outside [lo, hi]
};
template <bool RED, bool WHR>
struct AccOf { typedef RAcc<RED> type; };
template <>
struct AccOf<true, true> { typedef WAcc type; };
// one compare per lane and one ballot: the bits of the constrained fields that pass, against the mask
__device__ __forceinline__ bool whr_keeps(const WAcc& wa, const Whr& wh, uint64_t x) {
  const bool in = wa.lo <= x && x <= wa.hi;
  const uint32_t pass = (uint32_t)__ballot(wa.on && in != wa.outside);
  return wh.any ? pass != 0 : pass == wh.mask;
}

template <class... RD>
struct IsVarint { static constexpr bool value = false; };
template <>
struct IsVarint<RedV> { static constexpr bool value = true; };
template <>
struct IsVarint<RedV, Whr> { static constexpr bool value = true; };

// The plan walk, a kernel template on its trailing arguments.  k_scan_plan<> is the plan as it
// always was, with the same kernel arguments.  k_scan_plan<Red> (mtblx_scan_reduce) also folds every
// accepted record whose value is 8 * nf bytes long into the lanes' accumulators where the walk
// counts it, and counts the others in nbad.  k_scan_plan<RedV> does so for the values that are nf
// varints back to back (reduce_ops.h, r_load_varint_lane).  k_scan_plan<Red, Whr> and
// k_scan_plan<RedV, Whr> (mtblx_scan_reduce_where) evaluate the predicate on the fields a record's
// value was just decoded to, fold the kept values alone and count them in nmatch; the counts of the
// plan, the stop rules and max_records do not see the predicate.
template <class... RD>
__global__ void __launch_bounds__(256) k_scan_plan(const uint8_t* file, uint64_t file_len, uint32_t version, int verify,
                                                   uint64_t idx_off, uint64_t idx_len, DecTab tab, const int32_t* type,
                                                   const uint8_t* qkeys, const uint64_t* qend, const uint8_t* qkeys2,
                                                   const uint64_t* qend2, const uint64_t* maxrec, uint32_t max_blocks,
                                                   uint32_t nq, mtblx_scan_result* wres, Land* land, RD... red) {
  constexpr bool RED = sizeof...(RD) != 0;
  constexpr bool WHR = sizeof...(RD) == 2;
  __shared__ uint32_t T[256];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) T[i] = mtblx_crc::kTab.byte[i];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const uint32_t waves = gridDim.x * (blockDim.x / 64);
  const FileCtx f{file, file_len, version, verify, T, lane, tab};
  for (uint32_t q = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); q < nq; q += waves) {
    MTBLX_CHK(type + q, 4);
    MTBLX_CHK(qend + q, 8);
    const int32_t ty = type[q];
    const uint64_t k0 = q ? qend[q - 1] : 0;
    Targets g{qkeys + k0, qend[q] - k0, qkeys, 0, ty == 3};
    if (g.two) {
      MTBLX_CHK(qend2 + q, 8);
      const uint64_t e0 = q ? qend2[q - 1] : 0;
      g.k2 = qkeys2 + e0;
      g.k2l = qend2[q] - e0;
    }
    uint64_t mr = ~0ull;
    if (maxrec) { MTBLX_CHK(maxrec + q, 8); mr = maxrec[q]; }
    int32_t st = MTBLX_SCAN_FALLBACK, end = 0;
    uint64_t nrec = 0, kb = 0, vb = 0;
    uint32_t blocks = 0;
    Land ld{};
    Blk ib{}, db{};
    It ii{}, di{}, dj{};
    typename AccOf<RED, WHR>::type ra;
    if constexpr (RED) {
      ra.op = r_op(red_of(red...).sp, lane & 7);
      ra.acc = r_ident(ra.op);
    }
    if constexpr (WHR) {
      const Whr& wh = whr_of(red...);
#pragma unroll
      for (int f = 0; f < MTBLX_REDUCE_MAX_FIELDS; ++f)
        if ((lane & 7) == f) {
          ra.lo = wh.lo[f];
          ra.hi = wh.hi[f];
        }
      ra.on = lane < MTBLX_REDUCE_MAX_FIELDS && ((wh.mask >> lane) & 1u);
      ra.outside = lane < MTBLX_REDUCE_MAX_FIELDS && ((wh.outside >> lane) & 1u);
    }
    do {
      if (block_init(file + idx_off, idx_len, ib) != 0) break;   // the Reader's index block
      if (iter_init(ib, ii) != R_OK) break;
      if (seek(ib, ii, g.t, g.tl) != R_OK) break;                 // new_from: index_iter.seek(key)
      ld.ix_entry = ii.current;
      if (!valid(ib, ii)) { st = MTBLX_SCAN_OK; break; }          // no block: next() -> None
      // phase 0: new_from opens the landed block and seeks it; 1: the first next() (no bi.next());
      // 2: every later next()
      int phase = 0;
      for (;;) {
        if (ty == 1 && nrec == 1) { st = MTBLX_SCAN_OK; break; }   // Reader::get takes one (:111-122)
        if (phase != 0 && nrec >= mr) { st = MTBLX_SCAN_OK; end = 1; break; }
        const bool val = phase != 0 && valid(db, di);
        bool adv = phase == 2 && val;                              // bi.next() parses an entry
        const bool open = !val;                                    // get() is None: the next block
        if (open) {
          if (phase != 0) {                                        // index_iter.next()
            if (!valid(ib, ii)) { st = MTBLX_SCAN_OK; break; }
            const int r = parse_next_key(ib, ii, g.t, g.tl);
            if (r == R_PANIC || r == R_LOOP) break;
            if (!valid(ib, ii)) { st = MTBLX_SCAN_OK; break; }
            if (ii.next == ii.current) break;                      // a zero-progress index entry
          }
          if (blocks >= max_blocks) { st = MTBLX_SCAN_LARGE; break; }
          uint64_t ms = 0, ml = 0;
          if (block_at_index(f, ib, ii, db, ms, ml) != 1) break;   // Reader::block: panic, Err, missing
          ++blocks;
          if (db.L > kU32) break;                                  // a block >= 4 GiB
          if (iter_init(db, di) != R_OK) break;
          if (phase == 0) {
            if (seek2(db, di, dj, g, ld.restart) != R_OK) break;   // bi.seek(key)
            ld.d_entry = di.current;
            phase = 1;
            continue;
          }
          restart_at(db, di, 0);                                   // seek_to_first
          dj = di;
          adv = true;
        }
        phase = 2;
        if (adv) {
          const int r = step(db, di, dj, g);
          if (r == R_PANIC || r == R_LOOP) break;
        }
        if (!valid(db, di)) {
          if (open) { st = MTBLX_SCAN_OK; break; }                 // an empty block: entry? -> None
          continue;                                                // bi.next() hit the block's end
        }
        if (di.voff + di.vlen > db.L) break;                       // get()'s slice
        if (di.klen > kMaxKey) break;
        if (di.next == di.current) break;                          // zero progress: never returns
        bool stop = false;                                         // src/reader.rs:385-402
        if (ty == 1) stop = cmp_key(di, g.tl) != 0;
        else if (ty == 2) stop = di.c != g.tl;
        else if (ty == 3) stop = cmp_key(dj, g.k2l) > 0;
        if (stop) { st = MTBLX_SCAN_OK; break; }
        ++nrec;
        kb += di.klen;
        vb += di.vlen;
        if constexpr (RED) {   // the value is db.d + [voff, voff + vlen), inside the block (checked above)
          const Red& rd = red_of(red...);
          if constexpr (WHR) {   // the mask names fields below nf only: lanes at or above nf never vote
            const Whr& wh = whr_of(red...);
            uint64_t x = 0;
            bool ok;
            if constexpr (IsVarint<RD...>::value) {
              ok = r_load_varint_lane<true>(db.d + di.voff, di.vlen, rd.nf, (uint32_t)lane, &x);
            } else {
              ok = di.vlen == 8ull * rd.nf;
              if (ok && (uint32_t)lane < rd.nf) {
                const uint8_t* vp = db.d + di.voff + 8u * (uint32_t)lane;   // any alignment
                MTBLX_CHK(vp, 8);
                x = *reinterpret_cast<const u64u*>(vp);
              }
            }
            if (!ok) {
              ++ra.bad;
            } else if (whr_keeps(ra, wh, x)) {
              ++ra.match;
              if ((uint32_t)lane < rd.nf) ra.acc = r_apply(ra.op, ra.acc, x);
            }
          } else if constexpr (IsVarint<RD...>::value) {
            uint64_t x = 0;
            if (!r_load_varint_lane<true>(db.d + di.voff, di.vlen, rd.nf, (uint32_t)lane, &x)) ++ra.bad;
            else if ((uint32_t)lane < rd.nf) ra.acc = r_apply(ra.op, ra.acc, x);
          } else if (di.vlen != 8ull * rd.nf) {
            ++ra.bad;
          } else if ((uint32_t)lane < rd.nf) {
            const uint8_t* vp = db.d + di.voff + 8u * (uint32_t)lane;   // any alignment
            MTBLX_CHK(vp, 8);
            ra.acc = r_apply(ra.op, ra.acc, *reinterpret_cast<const u64u*>(vp));
          }
        }
      }
    } while (false);
    mtblx_scan_result R{};
    R.status = st;
    R.blocks = blocks;
    if (st == MTBLX_SCAN_OK) {
      R.end = end;
      R.nrec = nrec;
      R.key_bytes = kb;
      R.val_bytes = vb;
    }
    MTBLX_CHK(wres + q, sizeof(R));
    MTBLX_CHK(land + q, sizeof(ld));
    if (lane == 0) { wres[q] = R; land[q] = ld; }
    if constexpr (RED) {   // not OK: zero fields and zero nbad, as the counts
      const bool ok = st == MTBLX_SCAN_OK;
      const Red& rd = red_of(red...);
      if ((uint32_t)lane < rd.nf) {
        uint64_t* fp = rd.fields + (uint64_t)q * rd.nf + (uint32_t)lane;
        MTBLX_CHK(fp, 8);
        *fp = ok ? ra.acc : 0;
      }
      MTBLX_CHK(rd.nbad + q, 8);
      if (lane == 0) rd.nbad[q] = ok ? ra.bad : 0;
      if constexpr (WHR) {
        const Whr& wh = whr_of(red...);
        MTBLX_CHK(wh.nmatch + q, 8);
        if (lane == 0) wh.nmatch[q] = ok ? ra.match : 0;
      }
    }
  }
}

__global__ void __launch_bounds__(1024) k_scan_offsets(mtblx_scan_result* wres, mtblx_scan_result* res, uint32_t nq,
                                                       uint64_t* hdr, uint64_t mark) {
  __shared__ uint64_t wsum[3][16];
  __shared__ uint64_t carry[3];
  __shared__ unsigned long long nbad;
  const int tid = threadIdx.x;
  if (tid == 0) { carry[0] = carry[1] = carry[2] = 0; nbad = 0; }
  __syncthreads();
  for (uint32_t base = 0; base < nq; base += blockDim.x) {
    const uint32_t r = base + tid;
    mtblx_scan_result R{};
    if (r < nq) { MTBLX_CHK(wres + r, sizeof(R)); R = wres[r]; }
    const bool ok = r < nq && R.status == MTBLX_SCAN_OK;
    if (r < nq && !ok) atomicAdd(&nbad, 1ull);
    const uint64_t v[3] = {ok ? R.nrec : 0, ok ? R.key_bytes : 0, ok ? R.val_bytes : 0};
    uint64_t x[3] = {v[0], v[1], v[2]};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      for (int o = 1; o < 64; o <<= 1) {
        const uint64_t y = __shfl_up(x[a], o, 64);
        if ((tid & 63) >= o) x[a] += y;
      }
      if ((tid & 63) == 63) wsum[a][tid >> 6] = x[a];
    }
    __syncthreads();
    uint64_t excl[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      uint64_t wp = 0;
      for (int w = 0; w < (tid >> 6); ++w) wp += wsum[a][w];
      excl[a] = carry[a] + wp + x[a] - v[a];
    }
    __syncthreads();
    if (tid == (int)blockDim.x - 1) {
#pragma unroll
      for (int a = 0; a < 3; ++a) carry[a] = excl[a] + v[a];
    }
    if (r < nq) {
      R.rec_base = excl[0];
      R.key_base = excl[1];
      R.val_base = excl[2];
      MTBLX_CHK(res + r, sizeof(R));
      wres[r] = R;
      res[r] = R;
    }
    __syncthreads();
  }
  if (tid == 0) {
    MTBLX_CHK(hdr, 8 * H_WORDS);
    hdr[H_REC] = carry[0];
    hdr[H_KEY] = carry[1];
    hdr[H_VAL] = carry[2];
    hdr[H_BAD] = nbad;
    hdr[H_MARK] = mark;
  }
}

// the index entry at `cur` as the chain of seek_to_first + next reaches it: its value and successor
__device__ __forceinline__ bool index_entry(const Blk& ib, uint64_t cur, It& ii) {
  if (cur >= ib.R) return false;
  uint32_t sh, ns, vl;
  uint64_t p;
  if (decode_entry(ib, cur, ib.R, sh, ns, vl, p) != R_OK) return false;
  if (p + ns + vl > ib.L) return false;
  ii.current = cur;
  ii.voff = p + ns;
  ii.vlen = vl;
  ii.next = p + ns + vl;
  return true;
}

__global__ void __launch_bounds__(64) k_scan_emit(const uint8_t* file, uint64_t file_len, uint32_t version,
                                                  uint64_t idx_off, uint64_t idx_len, DecTab tab, uint32_t nq,
                                                  const uint64_t* hdr, const mtblx_scan_result* wres, const Land* land,
                                                  mtblx_scanned out, uint64_t mark) {
  __shared__ uint8_t K[MTBLX_SCAN_MAX_KEY];
  const int lane = threadIdx.x;
  MTBLX_CHK(hdr + H_MARK, 8);
  MTBLX_CHK(out.flags, 4);
  if (hdr[H_MARK] != mark) {
    if (blockIdx.x == 0 && lane == 0) atomicOr(out.flags, MTBLX_SCAN_NOT_PLANNED);
    return;
  }
  const FileCtx f{file, file_len, version, 0, nullptr, lane, tab};
  for (uint32_t q = blockIdx.x; q < nq; q += gridDim.x) {
    MTBLX_CHK(wres + q, sizeof(mtblx_scan_result));
    MTBLX_CHK(land + q, sizeof(Land));
    const mtblx_scan_result R = wres[q];
    if (R.status != MTBLX_SCAN_OK || R.nrec == 0) continue;
    const Land ld = land[q];
    uint32_t fl = 0;
    uint64_t n = 0, kb = 0, vb = 0;
    Blk ib{}, db{};
    It ii{};
    SIt it{};
    do {
      fl = MTBLX_SCAN_INTERNAL;   // cleared where the walk ends as planned
      if (block_init(file + idx_off, idx_len, ib) != 0) break;
      ii.next = ld.ix_entry;
      int phase = 0;       // 0: the sought block; 2: afterwards
      bool chk = false;    // the first entry at or past the landing must be the landing
      uint64_t skip = 0;   // sought block: the entries before the landing only rebuild the key
      while (n < R.nrec) {
        const bool val = phase != 0 && it.current < db.R;
        bool adv = val;
        const bool open = !val;
        if (open) {
          if (!index_entry(ib, ii.next, ii)) break;
          uint64_t start = 0, sz = 0, ms = 0, ml = 0;
          uint32_t crc = 0;
          if (frame_at_index(f, ib, ii, start, sz, crc) != 1) break;
          if (block_after_crc(f, start, sz, db, ms, ml) != 1) break;
          if (db.L > kU32 || db.n == 0) break;
          it = SIt{};
          it.kcap = ~0ull >> 1;   // the plan has checked the capacity assert
          it.has_next = true;
          it.current = db.R;
          skip = 0;
          if (phase == 0) {
            phase = 2;
            if (ld.d_entry >= db.R) continue;                      // the seek ran past the block
            if (ld.restart >= db.n) break;
            skip = ld.d_entry;
            chk = true;
            it.next = restart_point(db, ld.restart);
          } else {
            it.next = restart_point(db, 0);
          }
          adv = true;
        }
        if (adv) {
          const int r = s_parse(db, it, K, kMaxKey, lane);
          if (r == R_END && !open) continue;                       // the block's end: the next block
          if (r != R_OK) break;
          if (it.next == it.current) break;
        }
        if (it.current < skip) continue;
        if (chk && it.current != skip) break;
        chk = false;
        const uint64_t kl = it.klen, vl = it.vlen;
        if (it.voff + vl > db.L) break;
        if (kb + kl > R.key_bytes || vb + vl > R.val_bytes) break;   // outside the planned slot
        const uint64_t gk = R.key_base + kb, gv = R.val_base + vb, gr = R.rec_base + n;
        if (gr >= out.rec_cap || gk + kl > out.keys_cap || gv + vl > out.vals_cap) {
          fl = MTBLX_SCAN_OVERFLOW;   // this record and the query's later ones are not written
          break;
        }
        uint8_t* kd = out.keys + gk;
        for (uint64_t j = (uint64_t)lane; j < kl; j += 64) {
          MTBLX_CHK(kd + j, 1);
          kd[j] = K[j];
        }
        const uint8_t* vs = db.d + it.voff;
        uint8_t* vo = out.vals + gv;
        uint64_t j0 = 0;
        if (vl >= 4096) {   // 16 bytes per lane, as k_block_seek
          typedef uint32_t v4u __attribute__((ext_vector_type(4), aligned(1)));
          const uint64_t nv = vl / 16;
          for (uint64_t c = (uint64_t)lane; c < nv; c += 64) {
            MTBLX_CHK(vo + 16 * c, 16);
            MTBLX_CHK(vs + 16 * c, 16);
            *reinterpret_cast<v4u*>(vo + 16 * c) = *reinterpret_cast<const v4u*>(vs + 16 * c);
          }
          j0 = 16 * nv;
        }
        for (uint64_t j = j0 + (uint64_t)lane; j < vl; j += 64) {
          MTBLX_CHK(vo + j, 1);
          MTBLX_CHK(vs + j, 1);
          vo[j] = vs[j];
        }
        MTBLX_CHK(out.key_end + gr, 8);
        MTBLX_CHK(out.val_end + gr, 8);
        if (lane == 0) {
          out.key_end[gr] = gk + kl;
          out.val_end[gr] = gv + vl;
        }
        ++n;
        kb += kl;
        vb += vl;
      }
      if (fl == MTBLX_SCAN_INTERNAL && n == R.nrec && kb == R.key_bytes && vb == R.val_bytes) fl = 0;
    } while (false);
    if (fl && lane == 0) atomicOr(out.flags, fl);
  }
}

// Launch sizes.  k_scan_plan: kPlanWaves queries (one per wave) per workgroup and trip, at most 8
// workgroups per CU; k_scan_emit: one query per workgroup and trip, at most 16 per CU.  The
// launches and mtblx_debug_grid_items() share these.
constexpr uint64_t kPlanWaves = 256 / 64;
inline uint64_t plan_grid_cap() { return (uint64_t)mtblx_dev::cu_count() * 8u; }
inline uint64_t emit_grid_cap() { return (uint64_t)mtblx_dev::cu_count() * 16u; }

}  // namespace mtblx_rd

extern "C" size_t mtblx_scan_impl_ws_bytes(uint32_t nq) { return mtblx_rd::layout(nq).total; }

extern "C" int mtblx_scan_impl_reduce(const uint8_t* file, uint64_t file_len, uint32_t version, int verify,
                                      uint64_t index_off, uint64_t index_len, const uint64_t* tab_start,
                                      const uint64_t* tab_doff, const uint64_t* tab_dlen, const int32_t* tab_st,
                                      uint32_t ntab_in, const uint8_t* dec, const int32_t* type, const uint8_t* keys,
                                      const uint64_t* key_end, const uint8_t* keys2, const uint64_t* key2_end,
                                      const uint64_t* max_records, uint32_t max_blocks, uint32_t nq,
                                      mtblx_scan_result* res, uint64_t* totals, void* ws, const mtblx_reduce* spec,
                                      uint64_t* fields, uint64_t* nbad, const mtblx_where* where, uint64_t* nmatch,
                                      hipStream_t s);

// arguments already checked (mtblx_api.cpp): ws 256-byte aligned and large enough, every type in 0..3
extern "C" int mtblx_scan_impl_plan(const uint8_t* file, uint64_t file_len, uint32_t version, int verify,
                                    uint64_t index_off, uint64_t index_len, const uint64_t* tab_start,
                                    const uint64_t* tab_doff, const uint64_t* tab_dlen, const int32_t* tab_st,
                                    uint32_t ntab_in, const uint8_t* dec, const int32_t* type, const uint8_t* keys, const uint64_t* key_end, const uint8_t* keys2,
                                    const uint64_t* key2_end, const uint64_t* max_records, uint32_t max_blocks,
                                    uint32_t nq, mtblx_scan_result* res, uint64_t* totals, void* ws, hipStream_t s) {
  return mtblx_scan_impl_reduce(file, file_len, version, verify, index_off, index_len, tab_start, tab_doff, tab_dlen,
                                tab_st, ntab_in, dec, type, keys, key_end, keys2, key2_end, max_records, max_blocks, nq,
                                res, totals, ws, nullptr, nullptr, nullptr, nullptr, nullptr, s);
}

// spec == NULL: the plan alone.  Else k_scan_plan<Red> (k_scan_plan<RedV> for a varint spec) takes
// k_scan_plan<>'s place and fills fields / nbad; with `where` (its layout is the spec's: checked by
// mtblx_api.cpp) k_scan_plan<Red, Whr> / k_scan_plan<RedV, Whr> do and fill nmatch too.
extern "C" int mtblx_scan_impl_reduce(const uint8_t* file, uint64_t file_len, uint32_t version, int verify,
                                      uint64_t index_off, uint64_t index_len, const uint64_t* tab_start,
                                      const uint64_t* tab_doff, const uint64_t* tab_dlen, const int32_t* tab_st,
                                      uint32_t ntab_in, const uint8_t* dec, const int32_t* type, const uint8_t* keys,
                                      const uint64_t* key_end, const uint8_t* keys2, const uint64_t* key2_end,
                                      const uint64_t* max_records, uint32_t max_blocks, uint32_t nq,
                                      mtblx_scan_result* res, uint64_t* totals, void* ws, const mtblx_reduce* spec,
                                      uint64_t* fields, uint64_t* nbad, const mtblx_where* where, uint64_t* nmatch,
                                      hipStream_t s) {
  using namespace mtblx_rd;
  RedV rd{};
  bool varint = false;
  if (spec) {
    if (!reduce_spec(spec, &rd.sp, &varint)) return MTBLX_E_INVAL;
    rd.nf = spec->nfields;
    rd.fields = fields;
    rd.nbad = nbad;
  }
  Whr wh{};
  if (where) {
    if (!spec) return MTBLX_E_INVAL;
    for (uint32_t f = 0; f < MTBLX_REDUCE_MAX_FIELDS; ++f) {
      wh.lo[f] = where->lo[f];
      wh.hi[f] = where->hi[f];
    }
    wh.mask = where->mask;
    wh.outside = where->outside;
    wh.any = where->flags & MTBLX_WHERE_ANY;
    wh.nmatch = nmatch;
  }
  const DecTab tab = dec ? DecTab{tab_start, tab_doff, tab_dlen, tab_st, ntab_in, dec}
                         : DecTab{nullptr, nullptr, nullptr, nullptr, 0u, nullptr};
  const Layout L = layout(nq);
  uint8_t* w = static_cast<uint8_t*>(ws);
  uint64_t* hdr = reinterpret_cast<uint64_t*>(w + L.hdr);
  int32_t* dtype = reinterpret_cast<int32_t*>(w + L.type);
  mtblx_scan_result* wres = reinterpret_cast<mtblx_scan_result*>(w + L.res);
  Land* land = reinterpret_cast<Land*>(w + L.land);
  if (hipMemsetAsync(hdr, 0, 8 * H_WORDS, s) != hipSuccess) return MTBLX_E_HIP;
  if (hipMemcpyAsync(dtype, type, 4ull * nq, hipMemcpyHostToDevice, s) != hipSuccess) return MTBLX_E_HIP;
  const uint64_t need = ((uint64_t)nq + kPlanWaves - 1u) / kPlanWaves, cap = plan_grid_cap();
  const uint64_t ntab = tab.dec ? tab.n : 0;
  (void)ntab;   // read by the bounds-checked build only
  if (where && varint)
    MTBLX_LAUNCH((MTBLX_R(file, file_len), MTBLX_R(tab.start, 8ull * ntab), MTBLX_R(tab.doff, 8ull * ntab),
                  MTBLX_R(tab.dlen, 8ull * ntab), MTBLX_R(tab.st, 4ull * ntab), tab.dec, keys,
                  MTBLX_R(key_end, 8ull * nq), keys2, MTBLX_R(key2_end, 8ull * nq), MTBLX_R(max_records, 8ull * nq),
                  MTBLX_R(w, L.total), MTBLX_R(fields, 8ull * nq * rd.nf), MTBLX_R(nbad, 8ull * nq),
                  MTBLX_R(nmatch, 8ull * nq)),
                 (k_scan_plan<RedV, Whr>), dim3((unsigned)(need < cap ? need : cap)), dim3(256), 0, s, file, file_len,
                 version, verify, index_off, index_len, tab, dtype, keys, key_end, keys2, key2_end, max_records,
                 max_blocks, nq, wres, land, rd, wh);
  else if (where)
    MTBLX_LAUNCH((MTBLX_R(file, file_len), MTBLX_R(tab.start, 8ull * ntab), MTBLX_R(tab.doff, 8ull * ntab),
                  MTBLX_R(tab.dlen, 8ull * ntab), MTBLX_R(tab.st, 4ull * ntab), tab.dec, keys,
                  MTBLX_R(key_end, 8ull * nq), keys2, MTBLX_R(key2_end, 8ull * nq), MTBLX_R(max_records, 8ull * nq),
                  MTBLX_R(w, L.total), MTBLX_R(fields, 8ull * nq * rd.nf), MTBLX_R(nbad, 8ull * nq),
                  MTBLX_R(nmatch, 8ull * nq)),
                 (k_scan_plan<Red, Whr>), dim3((unsigned)(need < cap ? need : cap)), dim3(256), 0, s, file, file_len,
                 version, verify, index_off, index_len, tab, dtype, keys, key_end, keys2, key2_end, max_records,
                 max_blocks, nq, wres, land, static_cast<const Red&>(rd), wh);
  else if (!spec)
    MTBLX_LAUNCH((MTBLX_R(file, file_len), MTBLX_R(tab.start, 8ull * ntab), MTBLX_R(tab.doff, 8ull * ntab),
                  MTBLX_R(tab.dlen, 8ull * ntab), MTBLX_R(tab.st, 4ull * ntab), tab.dec, keys,
                  MTBLX_R(key_end, 8ull * nq), keys2, MTBLX_R(key2_end, 8ull * nq), MTBLX_R(max_records, 8ull * nq),
                  MTBLX_R(w, L.total)),
                 k_scan_plan<>, dim3((unsigned)(need < cap ? need : cap)), dim3(256), 0, s, file, file_len, version,
                 verify, index_off, index_len, tab, dtype, keys, key_end, keys2, key2_end, max_records, max_blocks, nq,
                 wres, land);
  else if (varint)
    MTBLX_LAUNCH((MTBLX_R(file, file_len), MTBLX_R(tab.start, 8ull * ntab), MTBLX_R(tab.doff, 8ull * ntab),
                  MTBLX_R(tab.dlen, 8ull * ntab), MTBLX_R(tab.st, 4ull * ntab), tab.dec, keys,
                  MTBLX_R(key_end, 8ull * nq), keys2, MTBLX_R(key2_end, 8ull * nq), MTBLX_R(max_records, 8ull * nq),
                  MTBLX_R(w, L.total), MTBLX_R(fields, 8ull * nq * rd.nf), MTBLX_R(nbad, 8ull * nq)),
                 k_scan_plan<RedV>, dim3((unsigned)(need < cap ? need : cap)), dim3(256), 0, s, file, file_len, version,
                 verify, index_off, index_len, tab, dtype, keys, key_end, keys2, key2_end, max_records, max_blocks, nq,
                 wres, land, rd);
  else
    MTBLX_LAUNCH((MTBLX_R(file, file_len), MTBLX_R(tab.start, 8ull * ntab), MTBLX_R(tab.doff, 8ull * ntab),
                  MTBLX_R(tab.dlen, 8ull * ntab), MTBLX_R(tab.st, 4ull * ntab), tab.dec, keys,
                  MTBLX_R(key_end, 8ull * nq), keys2, MTBLX_R(key2_end, 8ull * nq), MTBLX_R(max_records, 8ull * nq),
                  MTBLX_R(w, L.total), MTBLX_R(fields, 8ull * nq * rd.nf), MTBLX_R(nbad, 8ull * nq)),
                 k_scan_plan<Red>, dim3((unsigned)(need < cap ? need : cap)), dim3(256), 0, s, file, file_len, version,
                 verify, index_off, index_len, tab, dtype, keys, key_end, keys2, key2_end, max_records, max_blocks, nq,
                 wres, land, static_cast<const Red&>(rd));
  MTBLX_LAUNCH((MTBLX_R(w, L.total), MTBLX_R(res, sizeof(mtblx_scan_result) * (uint64_t)nq)), k_scan_offsets, dim3(1),
               dim3(1024), 0, s, wres, res, nq, hdr, planned_mark(nq));
  if (hipGetLastError() != hipSuccess) return MTBLX_E_HIP;
  uint64_t host[H_WORDS];
  if (hipMemcpyAsync(host, hdr, 8 * H_WORDS, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return MTBLX_E_HIP;
  for (int i = 0; i < 4; ++i) totals[i] = host[i];
  return MTBLX_OK;
}

// queries one launch starts before a wave (plan) or a workgroup (emit) takes its second one
extern "C" uint64_t mtblx_grid_items_scan_plan(void) { return mtblx_rd::plan_grid_cap() * mtblx_rd::kPlanWaves; }
extern "C" uint64_t mtblx_grid_items_scan_emit(void) { return mtblx_rd::emit_grid_cap(); }

extern "C" int mtblx_scan_impl_emit(const uint8_t* file, uint64_t file_len, uint32_t version, uint64_t index_off,
                                    uint64_t index_len, const uint64_t* tab_start, const uint64_t* tab_doff,
                                    const uint64_t* tab_dlen, const int32_t* tab_st, uint32_t ntab_in,
                                    const uint8_t* dec, uint32_t nq, const mtblx_scanned* out, const void* ws,
                                    hipStream_t s) {
  using namespace mtblx_rd;
  const DecTab tab = dec ? DecTab{tab_start, tab_doff, tab_dlen, tab_st, ntab_in, dec}
                         : DecTab{nullptr, nullptr, nullptr, nullptr, 0u, nullptr};
  const Layout L = layout(nq);
  const uint8_t* w = static_cast<const uint8_t*>(ws);
  if (hipMemsetAsync(out->flags, 0, 4, s) != hipSuccess) return MTBLX_E_HIP;
  const uint64_t cap = emit_grid_cap();
  const uint64_t ntab = tab.dec ? tab.n : 0;
  (void)ntab;   // read by the bounds-checked build only
  MTBLX_LAUNCH((MTBLX_R(file, file_len), MTBLX_R(tab.start, 8ull * ntab), MTBLX_R(tab.doff, 8ull * ntab),
                MTBLX_R(tab.dlen, 8ull * ntab), MTBLX_R(tab.st, 4ull * ntab), tab.dec, MTBLX_R(w, L.total),
                MTBLX_R(out->keys, out->keys_cap), MTBLX_R(out->vals, out->vals_cap),
                MTBLX_R(out->key_end, 8 * out->rec_cap), MTBLX_R(out->val_end, 8 * out->rec_cap),
                MTBLX_R(out->flags, 4)),
               k_scan_emit, dim3((unsigned)(nq < cap ? nq : cap)), dim3(64), 0, s, file, file_len, version, index_off,
               index_len, tab, nq, reinterpret_cast<const uint64_t*>(w + L.hdr),
               reinterpret_cast<const mtblx_scan_result*>(w + L.res), reinterpret_cast<const Land*>(w + L.land), *out,
               planned_mark(nq));
  return hipGetLastError() == hipSuccess ? MTBLX_OK : MTBLX_E_HIP;
}

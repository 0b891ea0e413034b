// reduce_seg.hip — segmented reduction over records on the MI355X (gfx950): mtblx_reduce_segments
// (include/mtblx.h "Aggregating scans", DESIGN.md §4 "Aggregating scans").
//
// Segment s is the records [seg_lo[s], seg_hi[s]) of one mtblx_records; per segment the F fields of
// a reduce spec are reduced over the values that are exactly W = 8 * F bytes long, and the others are
// counted in nbad[s].  With a varint spec (ENC = R_VARINT) the values that count are those that are
// exactly F varints back to back (reduce_ops.h, r_load_varint).  Records in no segment bring nothing.
//   k_rseg_check  a thread per segment: seg_lo[s] <= seg_hi[s] <= seg_lo[s + 1], seg_hi[nseg - 1] <= n;
//                 a violation sets MTBLX_REDUCE_BADSEG in *flags and the two kernels below return
//                 without writing
//   k_rseg_init   fields <- the ops' identities, nbad <- 0
//   k_rseg_tile   a workgroup owns kSegTile consecutive records, kSegPer per thread.  A thread finds
//                 the segment of its first record by binary search over seg_lo and advances from
//                 there (one load per record; a fresh search only where the next segment has begun).
//                 The inclusive segmented scan of reduce_ops.h, keyed on "the record's segment
//                 differs from its predecessor's" (thread-serial, __shfl_up inside the wave, LDS
//                 across the four waves), leaves one partial per (tile, segment) with the segment's
//                 last record in the tile; it goes out with one u64 atomic per field.
// A segment of a million records is a thousand tiles' partials on one line; a million segments of
// one record are a million atomics on their own words: no workgroup waits for another and no
// thread's work depends on a segment's length.  The ops are associative and commutative and the
// results exact, so the order in which the atomics land does not show.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bounds.h"
#include "mtblx.h"
#include "reduce_ops.h"

namespace {

constexpr int kSegThreads = 256;
constexpr int kSegTile = MTBLX_REDUCE_SEG_TILE;
constexpr int kSegPer = kSegTile / kSegThreads;
constexpr uint32_t kNoSeg = 0xFFFFFFFFu;
static_assert(kSegPer * kSegThreads == kSegTile, "tile");
typedef uint64_t ru64u __attribute__((aligned(1)));

__global__ void __launch_bounds__(kSegThreads) k_rseg_check(const uint64_t* seg_lo, const uint64_t* seg_hi,
                                                            uint32_t nseg, uint64_t n, uint32_t* flags) {
  const uint64_t s = (uint64_t)blockIdx.x * kSegThreads + threadIdx.x;
  if (s >= nseg) return;
  MTBLX_CHK(seg_lo + s, 8);
  MTBLX_CHK(seg_hi + s, 8);
  const uint64_t lo = seg_lo[s], hi = seg_hi[s];
  uint64_t next = n;
  if (s + 1 < nseg) {
    MTBLX_CHK(seg_lo + s + 1, 8);
    next = seg_lo[s + 1];
  }
  if (lo > hi || hi > next || hi > n) atomicOr(flags, MTBLX_REDUCE_BADSEG);
}

__global__ void __launch_bounds__(kSegThreads) k_rseg_init(uint64_t* fields, uint64_t* nbad, uint32_t nseg,
                                                           uint32_t nf, RSpec sp, const uint32_t* flags) {
  if (*flags & MTBLX_REDUCE_BADSEG) return;
  const uint64_t i = (uint64_t)blockIdx.x * kSegThreads + threadIdx.x;   // one word of fields
  if (i >= (uint64_t)nseg * nf) return;
  MTBLX_CHK(fields + i, 8);
  fields[i] = r_ident(r_op(sp, (int)(i % nf)));
  if (i < nseg) {
    MTBLX_CHK(nbad + i, 8);
    nbad[i] = 0;
  }
}

// the number of segments in [a, nseg) whose seg_lo <= i, plus a: the segment that may hold i is the one before
__device__ __forceinline__ uint32_t seg_upper(const uint64_t* seg_lo, uint32_t a, uint32_t nseg, uint64_t i) {
  uint32_t lo = a, hi = nseg;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    MTBLX_CHK(seg_lo + mid, 8);
    if (seg_lo[mid] <= i) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// c = the segments that begin at or before record i - 1 -> the same for record i
__device__ __forceinline__ uint32_t seg_advance(const uint64_t* seg_lo, uint32_t c, uint32_t nseg, uint64_t i) {
  if (c < nseg) {
    MTBLX_CHK(seg_lo + c, 8);
    if (seg_lo[c] <= i) c = seg_upper(seg_lo, c + 1, nseg, i);
  }
  return c;
}

// the segment that holds record i, given c = the segments that begin at or before it.  Sorted
// segments: every segment before c - 1 ends at or before seg_lo[c - 1] <= i.
__device__ __forceinline__ uint32_t seg_of(const uint64_t* seg_hi, uint32_t c, uint64_t i) {
  if (c == 0) return kNoSeg;
  MTBLX_CHK(seg_hi + (c - 1), 8);
  return i < seg_hi[c - 1] ? c - 1 : kNoSeg;
}

// a run's partial, and how many values of another length it met since its last head
template <int F>
struct SegB {
  Seg<F> s;      // hidx: the segment of the run's last head (kNoSeg: records of no segment)
  uint32_t nb;
};

template <int F>
__device__ __forceinline__ SegB<F> segb_join(const RSpec& sp, const SegB<F>& a, const SegB<F>& b) {
  SegB<F> r;
  r.s = seg_join<F>(sp, a.s, b.s);
  r.nb = (b.s.fl & 1u) ? b.nb : a.nb + b.nb;
  return r;
}

template <int F>
__device__ __forceinline__ SegB<F> segb_shfl_up(const SegB<F>& x, int o) {
  SegB<F> r;
  r.s = seg_shfl_up<F>(x.s, o);
  r.nb = __shfl_up(x.nb, o, 64);
  return r;
}

template <int F, int ENC>
__global__ void __launch_bounds__(kSegThreads) k_rseg_tile(mtblx_records rec, const uint64_t* seg_lo,
                                                           const uint64_t* seg_hi, uint32_t nseg, RSpec sp,
                                                           uint64_t* fields, uint64_t* nbad, const uint32_t* flags) {
  if (*flags & MTBLX_REDUCE_BADSEG) return;
  __shared__ uint64_t wv[kSegThreads / 64][F];   // the waves' runs
  __shared__ uint32_t wfl[kSegThreads / 64], whi[kSegThreads / 64], wnb[kSegThreads / 64];
  constexpr uint64_t W = 8u * F;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t n = rec.n;
  const uint64_t tile0 = (uint64_t)blockIdx.x * kSegTile;
  const uint64_t tend = tile0 + kSegTile < n ? tile0 + kSegTile : n;   // tile0 < n: the grid covers n
  const uint64_t i0 = tile0 + (uint64_t)threadIdx.x * kSegPer;
  // sid[k]: the segment of record i0 + k - 1 (k = 0: the predecessor, kNoSeg at the tile's start;
  // k = kSegPer + 1: the successor, kNoSeg at the tile's end)
  uint32_t sid[kSegPer + 2];
  uint64_t v[kSegPer][F];
  bool bad[kSegPer];
  uint32_t c = 0;
  sid[0] = kNoSeg;
  if (i0 < tend) {
    const uint64_t j = threadIdx.x ? i0 - 1 : i0;
    c = seg_upper(seg_lo, 0, nseg, j);
    sid[0] = threadIdx.x ? seg_of(seg_hi, c, j) : kNoSeg;
  }
#pragma unroll
  for (int k = 0; k <= kSegPer; ++k) {
    const uint64_t i = i0 + k;
    sid[k + 1] = kNoSeg;
    if (i >= tend) continue;
    c = seg_advance(seg_lo, c, nseg, i);
    sid[k + 1] = seg_of(seg_hi, c, i);
  }
#pragma unroll
  for (int k = 0; k < kSegPer; ++k) {
    const uint64_t i = i0 + k;
    bad[k] = false;
#pragma unroll
    for (int f = 0; f < F; ++f) v[k][f] = r_ident(r_op(sp, f));
    if (i >= tend || sid[k + 1] == kNoSeg) continue;
    MTBLX_CHK(rec.val_end + i, 8);
    uint64_t vs = 0;
    if (i) {
      MTBLX_CHK(rec.val_end + i - 1, 8);
      vs = rec.val_end[i - 1];
    }
    const uint64_t vlen = rec.val_end[i] - vs;
    const uint8_t* vp = rec.vals + vs;   // any alignment
    if (ENC == R_VARINT) {
      bad[k] = !r_load_varint<F, true>(vp, vlen, v[k]);
    } else if (vlen == W) {
      MTBLX_CHK(vp, W);
#pragma unroll
      for (int f = 0; f < F; ++f) v[k][f] = *reinterpret_cast<const ru64u*>(vp + 8 * f);
    } else {
      bad[k] = true;
    }
  }
  // the thread's run, the wave's inclusive scan of the runs, the waves before this one.  A record
  // is a head where its segment differs from its predecessor's (the tile's first record always is)
  SegB<F> a;
  a.s = seg_ident<F>(sp);
  a.nb = 0;
#pragma unroll
  for (int k = 0; k < kSegPer; ++k) {
    if (i0 + k >= tend) continue;
    SegB<F> e;
#pragma unroll
    for (int f = 0; f < F; ++f) e.s.v[f] = v[k][f];
    e.s.fl = (i0 + k == tile0 || sid[k + 1] != sid[k]) ? 1u : 0u;
    e.s.hidx = sid[k + 1];
    e.nb = bad[k] ? 1u : 0u;
    a = segb_join<F>(sp, a, e);
  }
  SegB<F> x = a;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const SegB<F> y = segb_shfl_up<F>(x, s);
    if (lane >= s) x = segb_join<F>(sp, y, x);
  }
  if (lane == 63) {
#pragma unroll
    for (int f = 0; f < F; ++f) wv[w][f] = x.s.v[f];
    wfl[w] = x.s.fl;
    whi[w] = x.s.hidx;
    wnb[w] = x.nb;
  }
  SegB<F> acc = segb_shfl_up<F>(x, 1);   // the runs of the wave's lanes before this one
  if (lane == 0) {
    acc.s = seg_ident<F>(sp);
    acc.nb = 0;
  }
  __syncthreads();
  SegB<F> before;
  before.s = seg_ident<F>(sp);
  before.nb = 0;
#pragma unroll
  for (int k = 0; k < kSegThreads / 64 - 1; ++k)
    if (k < w) {
      SegB<F> y;
#pragma unroll
      for (int f = 0; f < F; ++f) y.s.v[f] = wv[k][f];
      y.s.fl = wfl[k];
      y.s.hidx = whi[k];
      y.nb = wnb[k];
      before = segb_join<F>(sp, before, y);
    }
  acc = segb_join<F>(sp, before, acc);   // everything of the tile before this thread's records
#pragma unroll
  for (int k = 0; k < kSegPer; ++k) {
    const uint64_t i = i0 + k;
    if (i >= tend) continue;
    SegB<F> e;
#pragma unroll
    for (int f = 0; f < F; ++f) e.s.v[f] = v[k][f];
    e.s.fl = (i == tile0 || sid[k + 1] != sid[k]) ? 1u : 0u;
    e.s.hidx = sid[k + 1];
    e.nb = bad[k] ? 1u : 0u;
    acc = segb_join<F>(sp, acc, e);
    const uint32_t s = sid[k + 1];
    if (s == kNoSeg || (i + 1 < tend && sid[k + 2] == s)) continue;
    // the segment's last record in this tile: acc is the (tile, segment) partial.  s < nseg
    unsigned long long* fp = reinterpret_cast<unsigned long long*>(fields + (uint64_t)s * F);
    MTBLX_CHK(fp, W);
#pragma unroll
    for (int f = 0; f < F; ++f) {
      const uint32_t op = r_op(sp, f);
      const unsigned long long y = acc.s.v[f];
      if (y == r_ident(op)) continue;   // brings nothing
      if (op == MTBLX_REDUCE_SUM) atomicAdd(fp + f, y);
      else if (op == MTBLX_REDUCE_MIN) atomicMin(fp + f, y);
      else atomicMax(fp + f, y);
    }
    if (acc.nb) {
      MTBLX_CHK(nbad + s, 8);
      atomicAdd(reinterpret_cast<unsigned long long*>(nbad + s), (unsigned long long)acc.nb);
    }
  }
}

template <int F, int ENC>
void rseg_launch_e(const mtblx_records& rec, const uint64_t* seg_lo, const uint64_t* seg_hi, uint32_t nseg, RSpec sp,
                   uint64_t* fields, uint64_t* nbad, uint32_t* flags, hipStream_t s) {
  const uint64_t ntiles = (rec.n + kSegTile - 1) / kSegTile;
  MTBLX_LAUNCH((MTBLX_R(rec.val_end, 8 * rec.n), rec.vals, MTBLX_R(seg_lo, 8ull * nseg), MTBLX_R(seg_hi, 8ull * nseg),
                MTBLX_R(fields, 8ull * nseg * F), MTBLX_R(nbad, 8ull * nseg), MTBLX_R(flags, 4)),
               (k_rseg_tile<F, ENC>), dim3((unsigned)ntiles), dim3(kSegThreads), 0, s, rec, seg_lo, seg_hi, nseg, sp,
               fields, nbad, flags);
}

template <int F>
void rseg_launch(bool varint, const mtblx_records& rec, const uint64_t* seg_lo, const uint64_t* seg_hi, uint32_t nseg,
                 RSpec sp, uint64_t* fields, uint64_t* nbad, uint32_t* flags, hipStream_t s) {
  if (varint) rseg_launch_e<F, R_VARINT>(rec, seg_lo, seg_hi, nseg, sp, fields, nbad, flags, s);
  else rseg_launch_e<F, R_U64LE>(rec, seg_lo, seg_hi, nseg, sp, fields, nbad, flags, s);
}

}  // namespace

extern "C" uint32_t mtblx_reduce_seg_tile(void) { return (uint32_t)kSegTile; }

// arguments already checked (mtblx_api.cpp): aligned arrays, 0 < nseg <= MTBLX_REDUCE_MAX_SEGMENTS
extern "C" int mtblx_reduce_seg_impl(const mtblx_records* recs, const uint64_t* seg_lo, const uint64_t* seg_hi,
                                     uint32_t nseg, const mtblx_reduce* spec, uint64_t* fields, uint64_t* nbad,
                                     uint32_t* flags, hipStream_t s) {
  RSpec sp;
  bool varint;
  if (!reduce_spec(spec, &sp, &varint)) return MTBLX_E_INVAL;
  const uint32_t nf = spec->nfields;
  const mtblx_records rec = *recs;
  if (hipMemsetAsync(flags, 0, 4, s) != hipSuccess) return MTBLX_E_HIP;
  MTBLX_LAUNCH((MTBLX_R(seg_lo, 8ull * nseg), MTBLX_R(seg_hi, 8ull * nseg), MTBLX_R(flags, 4)), k_rseg_check,
               dim3((unsigned)(((uint64_t)nseg + kSegThreads - 1) / kSegThreads)), dim3(kSegThreads), 0, s, seg_lo, seg_hi, nseg,
               rec.n,
               flags);
  const uint64_t words = (uint64_t)nseg * nf;
  MTBLX_LAUNCH((MTBLX_R(fields, 8 * words), MTBLX_R(nbad, 8ull * nseg), MTBLX_R(flags, 4)), k_rseg_init,
               dim3((unsigned)((words + kSegThreads - 1) / kSegThreads)), dim3(kSegThreads), 0, s, fields, nbad, nseg,
               nf, sp, flags);
  if (rec.n) {
    switch (nf) {
      case 1: rseg_launch<1>(varint, rec, seg_lo, seg_hi, nseg, sp, fields, nbad, flags, s); break;
      case 2: rseg_launch<2>(varint, rec, seg_lo, seg_hi, nseg, sp, fields, nbad, flags, s); break;
      case 3: rseg_launch<3>(varint, rec, seg_lo, seg_hi, nseg, sp, fields, nbad, flags, s); break;
      case 4: rseg_launch<4>(varint, rec, seg_lo, seg_hi, nseg, sp, fields, nbad, flags, s); break;
      case 5: rseg_launch<5>(varint, rec, seg_lo, seg_hi, nseg, sp, fields, nbad, flags, s); break;
      case 6: rseg_launch<6>(varint, rec, seg_lo, seg_hi, nseg, sp, fields, nbad, flags, s); break;
      case 7: rseg_launch<7>(varint, rec, seg_lo, seg_hi, nseg, sp, fields, nbad, flags, s); break;
      default: rseg_launch<8>(varint, rec, seg_lo, seg_hi, nseg, sp, fields, nbad, flags, s); break;
    }
  }
  return hipGetLastError() == hipSuccess ? MTBLX_OK : MTBLX_E_HIP;
}

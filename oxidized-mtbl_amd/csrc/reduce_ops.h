// reduce_ops.h — what the reducing kernels share (include/mtblx.h "Device merge functions"): the
// op table of a reduce spec and the join of the segmented scan.  Used by the merge functions of the
// Merger and the Sorter (reduce_dev.h), by the segmented reduction over records (reduce_seg.hip)
// and by the reducing scan walk (scan.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bounds.h"
#include "mtblx.h"

namespace {

// how a value holds its fields (the MTBLX_REDUCE_VARINT bit of the spec's ops): a template
// parameter of the reducing kernels, never a run-time branch per field
enum { R_U64LE = 0, R_VARINT = 1 };

struct RSpec {       // travels in the kernel arguments; op of field f = (ops >> 8 f) & 0xFF, so no
  uint64_t ops;      // kernel indexes an array with a run-time field number
};

__device__ __forceinline__ uint32_t r_op(const RSpec& sp, int f) { return (uint32_t)(sp.ops >> (8 * f)) & 0xFFu; }
__device__ __forceinline__ uint64_t r_ident(uint32_t op) { return op == MTBLX_REDUCE_MIN ? ~0ull : 0ull; }
__device__ __forceinline__ uint64_t r_apply(uint32_t op, uint64_t a, uint64_t b) {
  return op == MTBLX_REDUCE_SUM ? a + b : op == MTBLX_REDUCE_MIN ? (a < b ? a : b) : (a > b ? a : b);
}

// ---- varint-coded values (include/mtblx.h "Varint-coded values") ----
// F varints back to back in [vp, vp + vlen), each read as varint_decode64 (src/varint.rs:78-97)
// reads the rest of the value: at most 10 bytes looked at, 7 bits each, what a tenth byte holds
// above 2^64 dropped by the shift, a non-canonical encoding taken as it is.  -> false (v untouched)
// where a field has no terminator within its 10 bytes or the value's end, where the rest is empty,
// or where bytes are left after the F-th field.  No byte at or past vp + vlen is read: every load
// is guarded by p < vlen.  kChk: the allocation that holds the values is among the launch's ranges
// (bounds.h), so the bounds build checks every byte load against it; the emit kernels of
// reduce_dev.h read their sources unchecked, as merge_dev.h does
template <int F, bool kChk>
__device__ __forceinline__ bool r_load_varint(const uint8_t* vp, uint64_t vlen, uint64_t* v) {
  if (vlen < (uint64_t)F || vlen > 10u * F) return false;   // every field takes 1 to 10 bytes
  uint64_t x[F];
  uint32_t p = 0;
  const uint32_t end = (uint32_t)vlen;
#pragma unroll
  for (int f = 0; f < F; ++f) {
    uint64_t a = 0;
    bool done = false;
#pragma nounroll
    for (uint32_t sh = 0; sh < 70u && p < end; sh += 7) {
      if (kChk) MTBLX_CHK(vp + p, 1);
      const uint32_t b = vp[p++];
      a |= (uint64_t)(b & 0x7fu) << sh;
      if (!(b & 0x80u)) {
        done = true;
        break;
      }
    }
    if (!done) return false;
    x[f] = a;
  }
  if (p != end) return false;
#pragma unroll
  for (int f = 0; f < F; ++f) v[f] = x[f];
  return true;
}

// the same over a run-time field count, for a wave whose lane f keeps field f (scan.hip): every lane
// walks the whole value (the loads are the same in all lanes) and keeps its own field in *mine
template <bool kChk>
__device__ __forceinline__ bool r_load_varint_lane(const uint8_t* vp, uint64_t vlen, uint32_t nf, uint32_t lane,
                                                   uint64_t* mine) {
  if (vlen < (uint64_t)nf || vlen > 10ull * nf) return false;
  uint32_t p = 0;
  const uint32_t end = (uint32_t)vlen;
  for (uint32_t f = 0; f < nf; ++f) {
    uint64_t a = 0;
    bool done = false;
    for (uint32_t sh = 0; sh < 70u && p < end; sh += 7) {
      if (kChk) MTBLX_CHK(vp + p, 1);
      const uint32_t b = vp[p++];
      a |= (uint64_t)(b & 0x7fu) << sh;
      if (!(b & 0x80u)) {
        done = true;
        break;
      }
    }
    if (!done) return false;
    if (f == lane) *mine = a;
  }
  return p == end;
}

// the bytes varint_encode64 (src/varint.rs:64-76) gives x: 1 for 0, else ceil(bits / 7)
__device__ __forceinline__ uint32_t r_varint_len(uint64_t x) {
  return x ? (uint32_t)(64 - __builtin_clzll(x) + 6) / 7u : 1u;
}

template <int F>
__device__ __forceinline__ uint64_t r_varint_len_all(const uint64_t* v) {
  uint64_t n = 0;
#pragma unroll
  for (int f = 0; f < F; ++f) n += r_varint_len(v[f]);
  return n;
}

// varint_encode64 of the F fields back to back at d (the caller has checked the capacity and, in
// the bounds build, the extent: r_varint_len_all bytes)
template <int F>
__device__ __forceinline__ void r_store_varint(uint8_t* d, const uint64_t* v) {
#pragma unroll
  for (int f = 0; f < F; ++f) {
    uint64_t x = v[f];
#pragma nounroll
    while (x >= 128u) {
      *d++ = (uint8_t)(x | 128u);
      x >>= 7;
    }
    *d++ = (uint8_t)x;
  }
}

// a run of records: v = the fields reduced since the run's last head (or over the whole run if it
// has none), fl bit 0 = the run has a head, bit 1 = a bad value since that head, hidx = that head
template <int F>
struct Seg {
  uint64_t v[F];
  uint32_t fl, hidx;
};

template <int F>
__device__ __forceinline__ Seg<F> seg_ident(const RSpec& sp) {
  Seg<F> r;
#pragma unroll
  for (int f = 0; f < F; ++f) r.v[f] = r_ident(r_op(sp, f));
  r.fl = 0;
  r.hidx = 0;
  return r;
}

// run a followed by run b
template <int F>
__device__ __forceinline__ Seg<F> seg_join(const RSpec& sp, const Seg<F>& a, const Seg<F>& b) {
  const bool cut = b.fl & 1u;
  Seg<F> r;
#pragma unroll
  for (int f = 0; f < F; ++f) r.v[f] = cut ? b.v[f] : r_apply(r_op(sp, f), a.v[f], b.v[f]);
  r.fl = cut ? b.fl : (a.fl | b.fl);
  r.hidx = cut ? b.hidx : a.hidx;
  return r;
}

template <int F>
__device__ __forceinline__ Seg<F> seg_shfl_up(const Seg<F>& x, int o) {
  Seg<F> r;
#pragma unroll
  for (int f = 0; f < F; ++f) r.v[f] = __shfl_up((unsigned long long)x.v[f], o, 64);
  r.fl = __shfl_up(x.fl, o, 64);
  r.hidx = __shfl_up(x.hidx, o, 64);
  return r;
}

// ---- host side ----
// -> false if the spec is not one (mtblx_api.cpp has checked it already).  The op table keeps the
// ops alone; *varint: every op carries MTBLX_REDUCE_VARINT (none: false; a mix is no spec)
inline bool reduce_spec(const mtblx_reduce* spec, RSpec* sp, bool* varint) {
  if (!spec || spec->nfields < 1 || spec->nfields > MTBLX_REDUCE_MAX_FIELDS) return false;
  sp->ops = 0;
  uint32_t nv = 0;
  for (uint32_t f = 0; f < spec->nfields; ++f) {
    const uint32_t op = spec->op[f] & ~MTBLX_REDUCE_VARINT;
    if (op > MTBLX_REDUCE_MAX) return false;
    if (spec->op[f] & MTBLX_REDUCE_VARINT) ++nv;
    sp->ops |= (uint64_t)op << (8 * f);
  }
  if (nv != 0 && nv != spec->nfields) return false;
  *varint = nv != 0;
  return true;
}

}  // namespace

// reduce_ops.h — what the reducing kernels share (include/mtblx.h "Device merge functions"): the
// op table of a reduce spec and the join of the segmented scan.  Used by the merge functions of the
// Merger and the Sorter (reduce_dev.h), by the segmented reduction over records (reduce_seg.hip)
// and by the reducing scan walk (scan.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mtblx.h"

namespace {

struct RSpec {       // travels in the kernel arguments; op of field f = (ops >> 8 f) & 0xFF, so no
  uint64_t ops;      // kernel indexes an array with a run-time field number
};

__device__ __forceinline__ uint32_t r_op(const RSpec& sp, int f) { return (uint32_t)(sp.ops >> (8 * f)) & 0xFFu; }
__device__ __forceinline__ uint64_t r_ident(uint32_t op) { return op == MTBLX_REDUCE_MIN ? ~0ull : 0ull; }
__device__ __forceinline__ uint64_t r_apply(uint32_t op, uint64_t a, uint64_t b) {
  return op == MTBLX_REDUCE_SUM ? a + b : op == MTBLX_REDUCE_MIN ? (a < b ? a : b) : (a > b ? a : b);
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
// -> false if the spec is not one (mtblx_api.cpp has checked it already)
inline bool reduce_spec(const mtblx_reduce* spec, RSpec* sp) {
  if (!spec || spec->nfields < 1 || spec->nfields > MTBLX_REDUCE_MAX_FIELDS) return false;
  sp->ops = 0;
  for (uint32_t f = 0; f < spec->nfields; ++f) {
    if (spec->op[f] > MTBLX_REDUCE_MAX) return false;
    sp->ops |= (uint64_t)spec->op[f] << (8 * f);
  }
  return true;
}

}  // namespace

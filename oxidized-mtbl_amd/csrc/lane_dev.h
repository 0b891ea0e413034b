// lane_dev.h — the two small device pieces that the grouping kernels of merge_dev.h and the rollup
// (rollup.hip) share: the exclusive scan over a workgroup of kThreads threads and the
// 16-lanes-per-record byte mover.  Everything sits in an unnamed namespace, as in merge_dev.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bounds.h"

namespace {

constexpr int kThreads = 256;

typedef uint32_t v4u __attribute__((ext_vector_type(4)));
typedef uint32_t v4uu __attribute__((ext_vector_type(4), aligned(1)));

// exclusive scan of one value per thread over the workgroup's 256 threads; total = the sum
__device__ __forceinline__ uint64_t block_scan(uint64_t v, uint64_t* wsum, uint64_t* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned long long x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) wsum[w] = x;
  __syncthreads();
  uint64_t base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < kThreads / 64; ++k) {
    const uint64_t s = wsum[k];
    if (k < w) base += s;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return base + x - v;
}

// 16 lanes move len bytes: bytes up to the destination's 16-byte boundary, then 16-byte stores
// (aligned loads where the source is aligned the same way, unaligned 16-byte loads elsewhere),
// then the ragged end.  len == 0 falls through every step.
__device__ __forceinline__ void copy16(uint8_t* d, const uint8_t* s, uint64_t len, uint32_t l) {
  uint64_t head = (16u - (uint32_t)((uintptr_t)d & 15u)) & 15u;
  if (head > len) head = len;
  if (l < head) {
    MTBLX_CHK(d + l, 1);
    d[l] = s[l];
  }
  const uint64_t body = (len - head) >> 4;
  const uint8_t* sb = s + head;
  uint8_t* db = d + head;
  const bool aligned = ((uintptr_t)sb & 15u) == 0;
  for (uint64_t c = l; c < body; c += 16) {
    v4u v;
    if (aligned) v = *reinterpret_cast<const v4u*>(sb + 16 * c);
    else v = *reinterpret_cast<const v4uu*>(sb + 16 * c);
    MTBLX_CHK(db + 16 * c, 16);
    *reinterpret_cast<v4u*>(db + 16 * c) = v;
  }
  const uint64_t done = head + 16 * body;
  if (l < len - done) {
    MTBLX_CHK(d + done + l, 1);
    d[done + l] = s[done + l];
  }
}

inline size_t up256(size_t x) { return (x + 255u) & ~(size_t)255u; }

}  // namespace

// snappy_comp.hip — MI355X (gfx950) Snappy raw COMPRESSION of a batch of blocks, and the
// write_block framing of the compressed contents: the device Writer's CompressionType::Snappy.
//
//   snappy_compress   /root/reference/src/compression.rs:126-130  snap::raw::Encoder::compress_vec
//   write_block       src/writer.rs:203-237   varint64(len) | crc32c(stored bytes) LE | stored bytes
//
// Compressed bytes are not pinned to the reference (snappy_host.cpp header): any
// valid raw stream that decodes to the block is a correct write_block.  The stream written here
// has the host compressor's element set: varint32 length, literals, copy-1 and copy-2, no copy-4,
// and no match crosses a 64 KiB fragment boundary (offsets fit 16 bits by construction).
//
// k_snappy_compress: one wave per block, fragment after fragment (a block is one fragment unless
// a record is larger than 64 KiB, so this is "one wave per fragment" for every block the Writer
// cuts at the usual sizes; DESIGN.md §4 "The Snappy writer").  The wave's hash table lives in LDS:
// 2^12 entries of 32 bits, (generation << 16 | fragment-relative position).  The generation is
// bumped per fragment, so the table is cleared once per wave, not once per fragment.
//   per step at cursor ip: lane l takes position ip + l, loads its 4 bytes, hashes them, reads
//   the table entry, verifies the candidate's 4 bytes; a ballot picks the FIRST matching lane;
//   the positions up to and including it are published; the pending literal is emitted by all
//   64 lanes; the match is extended 256 bytes per step (4 per lane, ballot on the first
//   mismatch); the copy elements follow emit_copy's split rules (snappy_host.cpp); the cursor
//   continues at the match end.  Without a match all 64 positions are published and the cursor
//   advances by 64.
// Determinism: the table is only written with atomicMax, and a step's reads all precede its
// writes (one wave, program order), so an entry is the highest position published so far
// whatever order the hardware retires colliding lanes in.  Equal inputs give equal bytes.
// Bounds: a lane loads 4 source bytes only at positions p with p + 4 <= fragment length, the
// ragged tail is compared and copied byte by byte, and a block is compressed only if its slot
// holds mtblx_snappy_max_compressed_len(n) bytes, which no stream built here exceeds (a copy
// element is never longer than the bytes it covers; a literal adds at most 3 bytes per 61+).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mtblx.h"
#include "bounds.h"
#include "devinfo.h"

namespace mtblx_sc {

constexpr int kWave = 64;
constexpr int kWaves = 4;                      // waves (blocks in flight) per workgroup
constexpr int kThreads = kWave * kWaves;
constexpr int kHashBits = 12;                  // 16 KiB per wave, 64 KiB per workgroup: two per CU
constexpr uint32_t kFrag = 1u << 16;
constexpr uint32_t kGenEnd = 1u << 16;         // generations 1 .. 65535, then the table is cleared

typedef uint32_t u32u __attribute__((aligned(1)));
typedef uint32_t v4uu __attribute__((ext_vector_type(4), aligned(1)));

__device__ __forceinline__ uint32_t ld32(const uint8_t* p) {
  MTBLX_CHK(p, 4);
  return *reinterpret_cast<const u32u*>(p);
}
__device__ __forceinline__ void st32(uint8_t* p, uint32_t v) {
  MTBLX_CHK(p, 4);
  *reinterpret_cast<u32u*>(p) = v;
}
__device__ __forceinline__ uint32_t hash4(uint32_t x) { return (x * 0x1e35a7bdu) >> (32 - kHashBits); }
__device__ __forceinline__ uint64_t max_len(uint64_t n) { return 32 + n + n / 6; }   // mtblx_snappy_max_compressed_len
__device__ __forceinline__ uint32_t vlen64(uint64_t v) {
  uint32_t n = 1;
  while (v >= 128) { v >>= 7; ++n; }
  return n;
}
__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// d[0 .. len) = s[0 .. len) by the wave: 4 bytes per lane per pass, the last 1..3 bytes by one lane
__device__ __forceinline__ void wave_copy(uint8_t* d, const uint8_t* s, uint32_t len, uint32_t lane) {
  uint32_t i = 4u * lane;
  for (; i + 4 <= len; i += 4u * kWave) st32(d + i, ld32(s + i));
  if (i < len) {
    MTBLX_CHK(s + i, len - i);
    MTBLX_CHK(d + i, len - i);
    for (uint32_t j = i; j < len; ++j) d[j] = s[j];
  }
}

// emit_literal's header (snappy_host.cpp): len - 1 < 60 in the tag, else 1 or 2 length bytes
// (a fragment is at most 65536 bytes).  -> header bytes; lane 0 writes
__device__ __forceinline__ uint32_t literal_header(uint8_t* o, uint32_t len, uint32_t lane) {
  const uint32_t n = len - 1;
  const uint32_t hb = n < 60 ? 1u : n < 256 ? 2u : 3u;
  if (lane == 0) {
    MTBLX_CHK(o, hb);
    if (hb == 1) {
      o[0] = (uint8_t)(n << 2);
    } else {
      o[0] = (uint8_t)((58 + hb) << 2);
      o[1] = (uint8_t)n;
      if (hb == 3) o[2] = (uint8_t)(n >> 8);
    }
  }
  return hb;
}

// emit_copy (snappy_host.cpp:121-137): 64-byte copy-2 elements while len >= 68, one of 60 if more
// than 64 remain, then the rest (copy-1 if < 12 bytes at an offset < 2048).  -> bytes written
__device__ __forceinline__ uint32_t emit_copy(uint8_t* o, uint32_t off, uint32_t len, uint32_t lane) {
  const uint32_t n64 = len >= 68 ? (len - 68) / 64 + 1 : 0;
  uint32_t rem = len - 64 * n64;
  for (uint32_t k = lane; k < n64; k += kWave) {
    uint8_t* e = o + 3 * k;
    MTBLX_CHK(e, 3);
    e[0] = (uint8_t)(2 | (63 << 2));
    e[1] = (uint8_t)off;
    e[2] = (uint8_t)(off >> 8);
  }
  uint32_t w = 3 * n64;
  const bool mid = rem > 64;
  if (mid) rem -= 60;
  const bool one = rem < 12 && off < 2048;
  if (lane == 0) {
    uint8_t* e = o + w;
    MTBLX_CHK(e, (mid ? 3 : 0) + (one ? 2 : 3));
    if (mid) {
      e[0] = (uint8_t)(2 | (59 << 2));
      e[1] = (uint8_t)off;
      e[2] = (uint8_t)(off >> 8);
      e += 3;
    }
    if (one) {
      e[0] = (uint8_t)(1 | ((rem - 4) << 2) | ((off >> 8) << 5));
      e[1] = (uint8_t)off;
    } else {
      e[0] = (uint8_t)(2 | ((rem - 1) << 2));
      e[1] = (uint8_t)off;
      e[2] = (uint8_t)(off >> 8);
    }
  }
  return w + (mid ? 3 : 0) + (one ? 2 : 3);
}

// one fragment in[0 .. n), 1 <= n <= 65536, appended at o -> bytes written
__device__ uint32_t compress_fragment(const uint8_t* in, uint32_t n, uint8_t* o, uint32_t* table, uint32_t gen,
                                      uint32_t lane) {
  const uint32_t tag = gen << 16;
  uint32_t ip = 0, lit = 0, op = 0;
  while (ip + 4 <= n) {
    const uint32_t pos = ip + lane;
    const bool valid = pos + 4 <= n;
    uint32_t cur = 0, h = 0, cand = 0;
    bool ok = false;
    if (valid) {
      cur = ld32(in + pos);
      h = hash4(cur);
      const uint32_t e = __hip_atomic_load(&table[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      cand = e & 0xFFFFu;
      // this fragment's entry, before the lane's own position: cand + 4 <= pos + 3 < n
      if ((e & 0xFFFF0000u) == tag && cand < pos) ok = ld32(in + cand) == cur;
    }
    const uint64_t m = __ballot(ok);
    const uint32_t fl = m ? (uint32_t)__builtin_ctzll(m) : (uint32_t)kWave;
    // every read of the step is done (the ballot waited for them): publish up to the match
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    if (valid && lane <= fl)
      (void)__hip_atomic_fetch_max(&table[h], tag | pos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    __builtin_amdgcn_wave_barrier();
    if (!m) {
      ip += kWave;
      continue;
    }
    const uint32_t mpos = ip + fl;
    const uint32_t off = mpos - uni((uint32_t)__shfl((int)cand, (int)fl, kWave));
    if (mpos > lit) {
      op += literal_header(o + op, mpos - lit, lane);
      wave_copy(o + op, in + lit, mpos - lit, lane);
      op += mpos - lit;
    }
    uint32_t len = 4;
    for (;;) {   // extend: lane l compares bytes [q, q + 4) with the bytes `off` before them
      const uint32_t q = mpos + len + 4u * lane;
      uint32_t nm = 0;
      if (q + 4 <= n) {
        const uint32_t x = ld32(in + q) ^ ld32(in + q - off);
        nm = x ? (uint32_t)__builtin_ctz(x) >> 3 : 4u;
      } else {
        while (q + nm < n && in[q + nm] == in[q + nm - off]) ++nm;   // at most 3 bytes before n
      }
      const uint64_t mm = __ballot(nm < 4);
      if (mm) {
        const int f = __builtin_ctzll(mm);
        len += 4u * (uint32_t)f + uni((uint32_t)__shfl((int)nm, f, kWave));
        break;
      }
      len += 4u * kWave;
    }
    op += emit_copy(o + op, off, len, lane);
    ip = lit = mpos + len;
  }
  if (lit < n) {
    op += literal_header(o + op, n - lit, lane);
    wave_copy(o + op, in + lit, n - lit, lane);
    op += n - lit;
  }
  return op;
}

__global__ void __launch_bounds__(kThreads) k_snappy_compress(const uint8_t* __restrict__ src,
                                                             const uint64_t* __restrict__ src_off,
                                                             const uint32_t* __restrict__ src_len, uint32_t nblk,
                                                             uint8_t* __restrict__ dst, uint64_t dst_cap,
                                                             const uint64_t* __restrict__ dst_off,
                                                             uint32_t* __restrict__ dst_len,
                                                             int32_t* __restrict__ status) {
  __shared__ uint32_t s_table[kWaves][1 << kHashBits];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wv = uni(threadIdx.x >> 6);
  uint32_t* table = s_table[wv];
  for (uint32_t i = lane; i < (1u << kHashBits); i += kWave) table[i] = 0;
  __builtin_amdgcn_wave_barrier();
  uint32_t gen = 0;
  const uint32_t W = gridDim.x * kWaves;
  for (uint32_t b = blockIdx.x * kWaves + wv; b < nblk; b += W) {
    MTBLX_CHK(src_off + b, 8);
    MTBLX_CHK(src_len + b, 4);
    MTBLX_CHK(dst_off + b, 8);
    const uint32_t n = src_len[b];
    const uint8_t* in = src + src_off[b];
    const uint64_t d0 = dst_off[b];
    uint64_t d1 = b + 1 < nblk ? dst_off[b + 1] : dst_cap;   // the slot: up to the next block's
    if (d1 > dst_cap) d1 = dst_cap;
    if (d0 > d1 || d1 - d0 < max_len(n)) {   // nothing is written for the block
      if (lane == 0) {
        status[b] = MTBLX_ST_OVERFLOW;
        dst_len[b] = 0;
      }
      continue;
    }
    uint8_t* o = dst + d0;
    uint32_t op = vlen64(n);
    if (lane == 0) {   // varint32 of the uncompressed length (n == 0: the single byte 0x00)
      MTBLX_CHK(o, op);
      uint32_t v = n;
      uint8_t* p = o;
      while (v >= 128) { *p++ = (uint8_t)(v | 128); v >>= 7; }
      *p = (uint8_t)v;
    }
    for (uint64_t p = 0; p < n; p += kFrag) {
      if (++gen == kGenEnd) {
        for (uint32_t i = lane; i < (1u << kHashBits); i += kWave) table[i] = 0;
        __builtin_amdgcn_wave_barrier();
        gen = 1;
      }
      const uint32_t fn = n - p < kFrag ? (uint32_t)(n - p) : kFrag;
      op += compress_fragment(in + p, fn, o + op, table, gen, lane);
    }
    if (lane == 0) {
      status[b] = MTBLX_ST_OK;
      dst_len[b] = op;
    }
  }
}

// exclusive scan over n block lengths by one workgroup.
//   kSlots: x = max_len(len) rounded up to 16; off[b] = the prefix; totals[0] = the sum
//   kFrame: x = vlen64(len) + 4 + len; off[b] = the prefix + vlen64(len) + 4 (the content
//           start); totals[0] = the sum, totals[1] = 1 if it exceeds cap
enum ScanMode { kSlots, kFrame };
template <ScanMode M>
__global__ void __launch_bounds__(1024) k_len_scan(const uint32_t* __restrict__ len, uint32_t n,
                                                   uint64_t* __restrict__ off, uint64_t* __restrict__ totals,
                                                   uint64_t cap) {
  __shared__ uint64_t ws[16];
  __shared__ uint64_t carry;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (uint64_t base = 0; base < n; base += 1024) {
    const uint64_t i = base + tid;
    uint64_t x = 0, head = 0;
    if (i < n) {
      MTBLX_CHK(len + i, 4);
      const uint64_t L = len[i];
      if (M == kSlots) {
        x = (max_len(L) + 15u) & ~15ull;
      } else {
        head = vlen64(L) + 4u;
        x = head + L;
      }
    }
    uint64_t v = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint64_t u = __shfl_up(v, d, 64);
      if (lane >= d) v += u;
    }
    if (lane == 63) ws[wv] = v;
    __syncthreads();
    uint64_t o = carry;
    for (int k = 0; k < wv; ++k) o += ws[k];
    if (i < n) {
      MTBLX_CHK(off + i, 8);
      off[i] = o + v - x + head;
    }
    __syncthreads();
    if (tid == 1023) carry = o + v;
    __syncthreads();
  }
  if (tid == 0) {
    MTBLX_CHK(totals, M == kFrame ? 16 : 8);
    totals[0] = carry;
    if (M == kFrame) totals[1] = carry > cap ? 1u : 0u;
  }
}

// write_block's header and payload of every block: one wave per block.  blk_off[b] is the content
// start (k_len_scan<kFrame>); a block that would end past out_cap is skipped (totals[1] says so).
__global__ void __launch_bounds__(kThreads) k_frame_write(const uint8_t* __restrict__ src,
                                                         const uint64_t* __restrict__ src_off,
                                                         const uint32_t* __restrict__ src_len, uint32_t nblk,
                                                         const uint32_t* __restrict__ crc, uint8_t* __restrict__ out,
                                                         uint64_t out_cap, const uint64_t* __restrict__ blk_off) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t W = gridDim.x * kWaves;
  for (uint32_t b = blockIdx.x * kWaves + uni(threadIdx.x >> 6); b < nblk; b += W) {
    MTBLX_CHK(src_off + b, 8);
    MTBLX_CHK(src_len + b, 4);
    MTBLX_CHK(blk_off + b, 8);
    const uint32_t L = src_len[b];
    const uint64_t c0 = blk_off[b];
    if (c0 + L > out_cap) continue;
    if (lane == 0) {   // varint64(len) | crc32c LE
      const uint32_t hb = vlen64(L);
      uint8_t* p = out + c0 - 4 - hb;
      MTBLX_CHK(p, hb + 4);
      MTBLX_CHK(crc + b, 4);
      uint32_t v = L;
      while (v >= 128) { *p++ = (uint8_t)(v | 128); v >>= 7; }
      *p++ = (uint8_t)v;
      const uint32_t c = crc[b];
      for (int k = 0; k < 4; ++k) p[k] = (uint8_t)(c >> (8 * k));
    }
    const uint8_t* s = src + src_off[b];
    uint8_t* d = out + c0;
    uint32_t i = 16u * lane;
    for (; i + 16 <= L; i += 16u * kWave) {
      MTBLX_CHK(s + i, 16);
      MTBLX_CHK(d + i, 16);
      *reinterpret_cast<v4uu*>(d + i) = *reinterpret_cast<const v4uu*>(s + i);
    }
    if (i < L) {
      MTBLX_CHK(s + i, L - i);
      MTBLX_CHK(d + i, L - i);
      for (uint32_t j = i; j < L; ++j) d[j] = s[j];
    }
  }
}

// one wave per block, at most two workgroups per CU (LDS); shared with mtblx_debug_grid_items()
inline uint32_t wave_grid_cap() { return (uint32_t)mtblx_dev::cu_count() * 2u; }
inline dim3 wave_grid(uint32_t nblk) {
  const uint32_t need = (nblk + kWaves - 1u) / kWaves;
  const uint32_t cap = wave_grid_cap();
  return dim3(need < cap ? need : cap);
}

}  // namespace mtblx_sc

// blocks a k_snappy_compress / k_frame_write launch starts before a wave takes its second one
extern "C" uint64_t mtblx_grid_items_snappy_comp(void) { return (uint64_t)mtblx_sc::wave_grid_cap() * mtblx_sc::kWaves; }

extern "C" size_t mtblx_snappy_compress_workspace_bytes(uint32_t nblk) { return 4ull * nblk + 256; }

extern "C" int mtblx_snappy_slots(const uint32_t* src_len, uint32_t nblk, uint64_t* dst_off, uint64_t* totals,
                                  void* workspace, size_t ws_bytes, void* stream) {
  using namespace mtblx_sc;
  (void)workspace;
  (void)ws_bytes;
  if (!totals || (nblk && (!src_len || !dst_off))) return MTBLX_E_INVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (nblk == 0) return hipMemsetAsync(totals, 0, 8, s) == hipSuccess ? MTBLX_OK : MTBLX_E_HIP;
  MTBLX_LAUNCH((MTBLX_R(src_len, 4ull * nblk), MTBLX_R(dst_off, 8ull * nblk), MTBLX_R(totals, 8)),
               (k_len_scan<kSlots>), dim3(1), dim3(1024), 0, s, src_len, nblk, dst_off, totals, 0ull);
  return hipGetLastError() == hipSuccess ? MTBLX_OK : MTBLX_E_HIP;
}

extern "C" int mtblx_snappy_compress_dev(const uint8_t* src, const uint64_t* src_off, const uint32_t* src_len,
                                         uint32_t nblk, uint8_t* dst, uint64_t dst_cap, const uint64_t* dst_off,
                                         uint32_t* dst_len, int32_t* status, void* workspace, size_t ws_bytes,
                                         void* stream) {
  using namespace mtblx_sc;
  (void)workspace;
  (void)ws_bytes;
  if (nblk == 0) return MTBLX_OK;
  if (!src || !src_off || !src_len || !dst || !dst_off || !dst_len || !status) return MTBLX_E_INVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  MTBLX_LAUNCH((src, MTBLX_R(src_off, 8ull * nblk), MTBLX_R(src_len, 4ull * nblk), MTBLX_R(dst, dst_cap),
                MTBLX_R(dst_off, 8ull * nblk), MTBLX_R(dst_len, 4ull * nblk), MTBLX_R(status, 4ull * nblk)),
               k_snappy_compress, wave_grid(nblk), dim3(kThreads), 0, s, src, src_off, src_len, nblk, dst, dst_cap,
               dst_off, dst_len, status);
  return hipGetLastError() == hipSuccess ? MTBLX_OK : MTBLX_E_HIP;
}

extern "C" int mtblx_frame_blocks(const uint8_t* src, const uint64_t* src_off, const uint32_t* src_len, uint32_t nblk,
                                  uint8_t* out, uint64_t out_cap, uint64_t* blk_off, uint64_t* totals,
                                  void* workspace, size_t ws_bytes, void* stream) {
  using namespace mtblx_sc;
  if (!totals) return MTBLX_E_INVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (nblk == 0) return hipMemsetAsync(totals, 0, 16, s) == hipSuccess ? MTBLX_OK : MTBLX_E_HIP;   // no workspace needed
  if (!src || !src_off || !src_len || !out || !blk_off || !workspace) return MTBLX_E_INVAL;
  if (ws_bytes < mtblx_snappy_compress_workspace_bytes(nblk) || ((uintptr_t)workspace & 3u)) return MTBLX_E_INVAL;
  uint32_t* crc = static_cast<uint32_t*>(workspace);
  MTBLX_LAUNCH((MTBLX_R(src_len, 4ull * nblk), MTBLX_R(blk_off, 8ull * nblk), MTBLX_R(totals, 16)),
               (k_len_scan<kFrame>), dim3(1), dim3(1024), 0, s, src_len, nblk, blk_off, totals, out_cap);
  if (hipGetLastError() != hipSuccess) return MTBLX_E_HIP;
  // the stored bytes' checksums by the library's CRC kernel.  No extent of `src` is known here:
  // that kernel reads whole 16-byte aligned chunks around a block only where they lie inside the
  // extent it is given, so with an open extent it may read up to 15 bytes beyond a range, inside
  // the aligned 16 bytes (hence the page) that hold the range's last byte.
  const mtblx_block_batch bb{src, 1ull << 62, src_off, src_len, nblk, 0};
  const int rc = mtblx_crc32c_blocks(&bb, crc, nullptr, 0, stream);
  if (rc != MTBLX_OK) return rc;
  MTBLX_LAUNCH((src, MTBLX_R(src_off, 8ull * nblk), MTBLX_R(src_len, 4ull * nblk), MTBLX_R(crc, 4ull * nblk),
                MTBLX_R(out, out_cap), MTBLX_R(blk_off, 8ull * nblk)),
               k_frame_write, wave_grid(nblk), dim3(kThreads), 0, s, src, src_off, src_len, nblk, crc, out, out_cap,
               blk_off);
  return hipGetLastError() == hipSuccess ? MTBLX_OK : MTBLX_E_HIP;
}

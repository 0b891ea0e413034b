// reader_dev.h — the device restatement of the reference's block reader, shared by reader.hip
// (mtblx_get, the seek primitives) and scan.hip (the batched scans):
//   varint_decode64 / varint_decode32            src/varint.rs
//   Block::init, BlockIter::{init, restart_point, parse_next_key, seek, valid}, decode_entry
//                                                src/block.rs:16-49, :75-238
//   block_at_index + Reader::block               src/reader.rs:139-186 (framing, checksum, the
//                                                caller's decompressed-block table, Block::init)
// Two iterators: It never materialises the key (it tracks the common prefix with one target and
// the sign of the first difference); SIt keeps the key bytes in a caller buffer (s_parse).
// Every global access goes through MTBLX_CHK (bounds.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bounds.h"
#include "crc_dev.h"
#include "mtblx.h"

namespace mtblx_rd {

// varint_length_packed over d[0..n) (src/varint.rs:1-10): 0 if no terminator
__device__ __forceinline__ uint32_t length_packed(const uint8_t* d, uint64_t n) {
  for (uint64_t i = 0; i < n; ++i) {
    MTBLX_CHK(d + i, 1);
    if (!(d[i] & 0x80u)) return (uint32_t)i + 1;
  }
  return 0;
}

// varint_decode64 on the slice d[0..n) (src/varint.rs:78-97 with varint_decode32 :44-61).
// Returns the consumed length (0 = unterminated), or -1 where the reference panics
// (n == 0: it indexes data[0]; fewer than 4 bytes on the 64-bit path: data[1..3]).
__device__ __forceinline__ int dec64(const uint8_t* d, uint64_t n, uint64_t& v) {
  if (n == 0) return -1;
  MTBLX_CHK(d, 1);
  const uint32_t l = length_packed(d, n < 10 ? n : 10);
  if (l < 5) {
    const uint32_t l32 = length_packed(d, n < 5 ? n : 5);
    uint32_t val = d[0] & 0x7fu;
    if (l32 > 1) val |= (uint32_t)(d[1] & 0x7fu) << 7;
    if (l32 > 2) val |= (uint32_t)(d[2] & 0x7fu) << 14;
    if (l32 > 3) val |= (uint32_t)(d[3] & 0x7fu) << 21;
    if (l32 > 4) val |= (uint32_t)d[4] << 28;
    v = val;
    return (int)l32;
  }
  MTBLX_CHK(d, l);
  uint64_t val = (uint64_t)(d[0] & 0x7fu) | ((uint64_t)(d[1] & 0x7fu) << 7) | ((uint64_t)(d[2] & 0x7fu) << 14) |
                 ((uint64_t)(d[3] & 0x7fu) << 21);
  uint32_t shift = 28;
  for (uint32_t i = 4; i < l; ++i) {
    val |= (uint64_t)(d[i] & 0x7fu) << shift;
    shift += 7;
  }
  v = val;
  return (int)l;
}

constexpr uint64_t kU32 = 0xFFFFFFFFull;

struct Blk {
  const uint8_t* d;
  uint64_t L, R;
  uint32_t n;
  bool wide;   // u64 restart array (blocks >= 4 GiB)
};

struct It {
  uint64_t current, next, klen, kcap, c, voff, vlen;
  int cmp;            // sign of key[c] - target[c] when c < min(klen, tlen), else 0
  bool has_next;
  bool has_val;       // `val` is Some: an entry has been parsed (src/block.rs:70-71, :136)
};

enum { R_OK = 1, R_END = 0, R_PANIC = -1, R_LOOP = -2 };

__device__ __forceinline__ uint32_t rd32g(const uint8_t* p) {
  MTBLX_CHK(p, 4);
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// varint_decode32 on d[0..n), n >= 1
__device__ __forceinline__ uint32_t dec32g(const uint8_t* d, uint64_t n, uint32_t& v) {
  MTBLX_CHK(d, 1);
  const uint32_t l = length_packed(d, n < 5 ? n : 5);
  uint32_t val = d[0] & 0x7fu;
  if (l > 1) val |= (uint32_t)(d[1] & 0x7fu) << 7;
  if (l > 2) val |= (uint32_t)(d[2] & 0x7fu) << 14;
  if (l > 3) val |= (uint32_t)(d[3] & 0x7fu) << 21;
  if (l > 4) val |= (uint32_t)d[4] << 28;
  v = val;
  return l;
}

// Block::init (src/block.rs:16-49): 0 ok, 1 InvalidBlock, -1 panic.  A restart offset past
// u32::MAX means a u64 restart array (blocks >= 4 GiB, src/block.rs:25-42).
__device__ __forceinline__ int block_init(const uint8_t* d, uint64_t L, Blk& b) {
  if (L < 4) return 1;
  if (L < 8) return -1;
  const uint32_t n = rd32g(d + L - 4);
  uint64_t ro = L - (1ull + n) * 4ull;
  if (ro > kU32) {
    ro = L - (4ull + (uint64_t)n * 8ull);
    if (ro <= kU32) return 1;
  }
  if (ro > L - 4) return 1;
  b.d = d; b.L = L; b.R = ro; b.n = n; b.wide = ro > kU32;
  return 0;
}

// BlockIter::restart_point (src/block.rs:95-104): a u64 array keeps the 4-byte stride of the
// u32 one (the reference indexes `restarts + idx * 4` either way)
__device__ __forceinline__ uint64_t restart_point(const Blk& b, uint32_t i) {
  const uint8_t* p = b.d + b.R + 4ull * i;
  return b.wide ? ((uint64_t)rd32g(p) | ((uint64_t)rd32g(p + 4) << 32)) : (uint64_t)rd32g(p);
}

// decode_entry (src/block.rs:216-238): R_OK or R_PANIC
__device__ __forceinline__ int decode_entry(const Blk& b, uint64_t p, uint64_t limit, uint32_t& sh, uint32_t& ns,
                                            uint32_t& vl, uint64_t& pout) {
  if (limit - p < 3) return R_PANIC;
  if (p + 2 >= b.L) return R_PANIC;
  MTBLX_CHK(b.d + p, 3);
  uint32_t x = b.d[p], y = b.d[p + 1], z = b.d[p + 2];
  if ((x | y | z) < 128u) {
    p += 3;
  } else {
    if (p >= b.L) return R_PANIC;
    p += dec32g(b.d + p, b.L - p, x);
    if (p >= b.L) return R_PANIC;
    p += dec32g(b.d + p, b.L - p, y);
    if (p >= b.L) return R_PANIC;
    p += dec32g(b.d + p, b.L - p, z);
    if (!(p <= limit)) return R_PANIC;
  }
  const uint64_t sum = (uint64_t)y + z;
  if (sum > kU32 || (limit - p) < sum) return R_PANIC;
  sh = x; ns = y; vl = z; pout = p;
  return R_OK;
}

// the number of equal leading bytes of a[0..n) and b[0..n): 8-byte loads (never past n), the
// first difference by the lowest set byte of the XOR; then the last < 8 bytes one at a time
typedef uint64_t __attribute__((aligned(1))) u64u;
__device__ __forceinline__ uint64_t match_len(const uint8_t* a, const uint8_t* b, uint64_t n) {
  uint64_t c = 0;
  while (c + 8 <= n) {
    MTBLX_CHK(a + c, 8), MTBLX_CHK(b + c, 8);
    const uint64_t x = *reinterpret_cast<const u64u*>(a + c) ^ *reinterpret_cast<const u64u*>(b + c);
    if (x) return c + (uint64_t)(__builtin_ctzll(x) >> 3);
    c += 8;
  }
  while (c < n && (MTBLX_CHK(a + c, 1), MTBLX_CHK(b + c, 1), a[c] == b[c])) ++c;
  return c;
}

__device__ __forceinline__ int cmp_key(const It& it, uint64_t tlen) {   // Ord of key vs target
  if (it.cmp) return it.cmp;
  return it.klen < tlen ? -1 : (it.klen > tlen ? 1 : 0);
}

__device__ __forceinline__ void restart_at(const Blk& b, It& it, uint32_t i) {   // seek_to_restart_point
  it.klen = 0; it.c = 0; it.cmp = 0;
  it.has_next = true;
  it.next = restart_point(b, i);
}

// parse_next_key (src/block.rs:119-143) with the common-prefix tracking; R_OK / R_END /
// R_PANIC / R_LOOP (an entry that does not advance: the reference spins forever)
__device__ int parse_next_key(const Blk& b, It& it, const uint8_t* t, uint64_t tlen) {
  const uint64_t prev = it.current;
  it.current = it.has_next ? it.next : 0;
  if (it.current >= b.R) { it.current = b.R; return R_END; }
  uint32_t sh, ns, vl;
  uint64_t p;
  if (decode_entry(b, it.current, b.R, sh, ns, vl, p) != R_OK) return R_PANIC;
  if (!(it.kcap >= sh)) return R_PANIC;                     // Vec capacity assert (:132)
  const uint64_t m = sh < it.klen ? sh : it.klen;           // truncate (:134)
  if (p + ns > b.L) return R_PANIC;
  if (ns > 0 && it.kcap - m < ns) {                         // Vec growth (:135)
    uint64_t c = it.kcap * 2, req = m + ns;
    if (req > c) c = req;
    if (c < 8) c = 8;
    it.kcap = c;
  }
  if (m <= it.c) {            // the kept prefix matches the target: compare the suffix
    const uint64_t lim = ns < tlen - (tlen < m ? tlen : m) ? ns : tlen - (tlen < m ? tlen : m);
    const uint64_t j = m < tlen ? match_len(b.d + p, t + m, lim) : 0;
    const uint64_t c = m + j;
    it.cmp = (j < ns && c < tlen) ? (b.d[p + j] < t[c] ? -1 : 1) : 0;
    it.c = c;
  }                           // else: the first difference lies in the kept prefix
  it.klen = m + ns;
  it.has_next = true;
  it.next = p + ns + vl;
  it.voff = p + ns;
  it.vlen = vl;
  it.has_val = true;
  if (it.next == it.current && it.current == prev) return R_LOOP;
  return R_OK;
}

// BlockIter::seek (src/block.rs:154-194)
__device__ int seek(const Blk& b, It& it, const uint8_t* t, uint64_t tlen) {
  uint32_t left = 0, right = b.n - 1;
  while (left < right) {
    const uint32_t mid = (uint32_t)(((uint64_t)left + right + 1) / 2);
    uint32_t sh, ns, vl;
    uint64_t ko;
    if (decode_entry(b, restart_point(b, mid), b.R, sh, ns, vl, ko) != R_OK) return R_PANIC;
    if (sh != 0) return R_OK;                                 // "corruption": early return
    if (ko + ns > b.L) return R_PANIC;
    const uint64_t c = match_len(b.d + ko, t, ns < tlen ? ns : tlen);
    const int r = (c < ns && c < tlen) ? (b.d[ko + c] < t[c] ? -1 : 1) : (ns < tlen ? -1 : (ns > tlen ? 1 : 0));
    if (r < 0) left = mid;
    else right = mid - 1;
  }
  restart_at(b, it, left);
  for (uint64_t steps = 0;; ++steps) {
    const uint64_t before = it.current;
    const int r = parse_next_key(b, it, t, tlen);
    if (r != R_OK) return r == R_END ? R_OK : r;
    if (cmp_key(it, tlen) >= 0) return R_OK;
    if (it.next == it.current || (steps > 0 && it.current == before)) return R_LOOP;
  }
}

__device__ __forceinline__ bool valid(const Blk& b, const It& it) { return it.current < b.R; }

// BlockIter::init (src/block.rs:75-93)
__device__ __forceinline__ int iter_init(const Blk& b, It& it) {
  if (b.n == 0) return R_PANIC;
  it.current = b.R; it.has_next = false; it.next = 0; it.has_val = false;
  it.klen = 0; it.kcap = 0; it.c = 0; it.cmp = 0; it.voff = 0; it.vlen = 0;
  return R_OK;
}

// decompressed blocks of a compressed file (mtblx_get_decompressed), sorted by stored start
struct DecTab {
  const uint64_t* start;
  const uint64_t* doff;
  const uint64_t* dlen;
  const int32_t* st;
  uint32_t n;
  const uint8_t* dec;
};

struct FileCtx {
  const uint8_t* file;
  uint64_t len;
  uint32_t version;
  int verify;
  const uint32_t* T;   // crc byte table (LDS)
  int lane;
  DecTab tab;          // tab.dec == nullptr: the file is not compressed
};

// block_at_index + Reader::block (src/reader.rs:177-186, :139-174), in two halves around the
// checksum.  frame_at_index: the landed index entry's offset and the block's framing ->
// 0 = None (get() -> None), R_PANIC, 1 = framed: content [start, start + sz), stored checksum crc.
__device__ __forceinline__ int frame_at_index(const FileCtx& f, const Blk& ib, const It& ii, uint64_t& start,
                                              uint64_t& sz, uint32_t& crc) {
  if (!valid(ib, ii)) return 0;                                // get() -> None
  if (ii.voff + ii.vlen > ib.L) return R_PANIC;
  uint64_t off = 0;
  if (dec64(ib.d + ii.voff, ii.vlen, off) < 0) return R_PANIC;
  if (!(off < f.len)) return R_PANIC;
  uint64_t ll;
  if (f.version == 0) {
    if (off + 4 > f.len) return R_PANIC;
    ll = 4; sz = rd32g(f.file + off);
  } else {
    const int k = dec64(f.file + off, f.len - off, sz);
    if (k < 0) return R_PANIC;
    ll = (uint64_t)k;
  }
  start = off + ll + 4;
  if (start > f.len || sz > f.len - start) return R_PANIC;
  crc = rd32g(f.file + off + ll);
  return 1;
}
// after the checksum (when verified): decompression (the caller's table) and Block::init ->
// 1 = Some(block), R_PANIC, 2 = Err(InvalidBlock), 3 = a compressed block the caller's table does
// not hold (its stored content [mstart, + msz) passed framing and the checksum)
__device__ __forceinline__ int block_after_crc(const FileCtx& f, uint64_t start, uint64_t sz, Blk& out,
                                               uint64_t& mstart, uint64_t& msz) {
  const uint8_t* content = f.file + start;
  if (f.tab.dec) {   // decompress (src/reader.rs:166-170): the caller's decompressed copy
    uint32_t lo = 0, hi = f.tab.n;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) / 2;
      MTBLX_CHK(f.tab.start + mid, 8);
      if (f.tab.start[mid] < start) lo = mid + 1;
      else hi = mid;
    }
    if (lo == f.tab.n || f.tab.start[lo] != start) {   // not decompressed by the caller (yet)
      mstart = start;
      msz = sz;
      return 3;
    }
    if (f.tab.st[lo] != 0) return 2;   // the crate's decompress error: Err(Io)
    MTBLX_CHK(f.tab.doff + lo, 8);
    MTBLX_CHK(f.tab.dlen + lo, 8);
    content = f.tab.dec + f.tab.doff[lo];
    sz = f.tab.dlen[lo];
  }
  const int bi = block_init(content, sz, out);
  if (bi == 1) return 2;
  if (bi < 0) return R_PANIC;
  return 1;
}
// the whole of it, for a wave-uniform caller (the checksum shared by the wave's lanes)
__device__ int block_at_index(const FileCtx& f, const Blk& ib, const It& ii, Blk& out, uint64_t& mstart,
                              uint64_t& msz) {
  uint64_t start = 0, sz = 0;
  uint32_t crc = 0;
  const int fr = frame_at_index(f, ib, ii, start, sz, crc);
  if (fr != 1) return fr;
  if (f.verify && mtblx_crc::wave_crc32c(f.file + start, sz, f.T, f.lane) != crc) return R_PANIC;
  return block_after_crc(f, start, sz, out, mstart, msz);
}

enum { R_TOOLONG = -3 };

struct SIt {
  uint64_t current, next, klen, kcap, voff, vlen;
  bool has_next, has_val;
};

// Ord of K[0..kl) vs t[0..tl), the wave together
__device__ int wave_cmp(const uint8_t* K, uint64_t kl, const uint8_t* t, uint64_t tl, int lane) {
  const uint64_t m = kl < tl ? kl : tl;
  for (uint64_t c0 = 0; c0 < m; c0 += 64) {
    const uint64_t c = c0 + (uint64_t)lane;
    if (c < m) { MTBLX_CHK(K + c, 1); MTBLX_CHK(t + c, 1); }
    const bool diff = c < m && K[c] != t[c];
    const uint64_t bal = __ballot(diff);
    if (bal) {
      const uint64_t cc = c0 + (uint64_t)__builtin_ctzll(bal);
      return K[cc] < t[cc] ? -1 : 1;
    }
  }
  return kl < tl ? -1 : (kl > tl ? 1 : 0);
}

// parse_next_key (src/block.rs:119-143): R_OK / R_END / R_PANIC / R_TOOLONG (key past klim,
// the key buffer's size)
__device__ __forceinline__ int s_parse(const Blk& b, SIt& it, uint8_t* K, uint64_t klim, int lane) {
  it.current = it.has_next ? it.next : 0;
  if (it.current >= b.R) { it.current = b.R; return R_END; }
  uint32_t sh, ns, vl;
  uint64_t p;
  if (decode_entry(b, it.current, b.R, sh, ns, vl, p) != R_OK) return R_PANIC;
  if (!(it.kcap >= sh)) return R_PANIC;                       // Vec capacity assert (:132)
  const uint64_t m = sh < it.klen ? sh : it.klen;             // truncate (:134)
  if (p + ns > b.L) return R_PANIC;
  if (ns > 0 && it.kcap - m < ns) {                           // Vec growth (:135)
    uint64_t c = it.kcap * 2, req = m + ns;
    if (req > c) c = req;
    if (c < 8) c = 8;
    it.kcap = c;
  }
  if (m + ns > klim) return R_TOOLONG;
  for (uint32_t j = (uint32_t)lane; j < ns; j += 64) {
    MTBLX_CHK(K + m + j, 1);
    MTBLX_CHK(b.d + p + j, 1);
    K[m + j] = b.d[p + j];
  }
  __syncthreads();   // one-wave workgroup: orders the key writes (LDS or global) before other lanes read K
  it.klen = m + ns;
  it.has_next = true;
  it.next = p + ns + vl;
  it.voff = p + ns;
  it.vlen = vl;
  it.has_val = true;
  return R_OK;
}

}  // namespace mtblx_rd

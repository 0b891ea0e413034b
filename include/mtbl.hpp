// mtbl.hpp — C++ mirror of oxidized-mtbl's public surface over libmtblx's C ABI.
//
// The reference is a Rust crate; Rust is not in this image, so the host side above the C ABI
// is C++ (header-only, C++17, compiled with hipcc).  Same names, argument meaning and error
// behaviour as the crate, for the path this library accelerates:
//
//   WriterBuilder / Writer      /root/reference/src/writer.rs:15-201   (mtblx_writer_*)
//   ReaderBuilder / Reader      src/reader.rs:15-135                    (footer, framing: host;
//                                                                        index, directory, CRC,
//                                                                        block decode: device)
//   Reader::get                 src/reader.rs:111-122                   (mtblx_get, batched seek)
//   ReaderIntoIter::next / seek src/reader.rs:219-405                   (device seek + decode of the
//   Reader::into_iter / iter_prefix / iter_range / iter_from             blocks the iteration reaches,
//                                                                        records served on the host)
//   Metadata                    src/metadata.rs:11-24
//   MergerBuilder / Merger      src/merger.rs:66-260                    (mtblx_merge_plan / _emit: the k-way
//                                                                        merge and the grouping on the device)
//   Merger::scan_batch          (not in the crate: MergerIter over iter_from / get / iter_prefix / iter_range
//                                of every source for a batch of queries; mtblx_merge_seg_plan / _emit)
//   SorterBuilder / Sorter      src/sorter.rs:17-258                    (mtblx_sort_plan / _emit: the sort of
//                                                                        a chunk on the device; the chunks
//                                                                        merged by the device Merger)
//   MtblError                  src/error.rs:44-52
//
// Errors: where the crate returns Err(Error::Mtbl(e)) this throws mtbl::Error(e); where it
// returns Err(Error::Io) (a snappy stream snap rejects) it throws mtbl::Error(kIo); where it
// panics (checksum assert_eq, out-of-range slices, corrupt entries, "out-of-order key") it
// throws mtbl::Panic.  Iteration reproduces ReaderIntoIter's end rules exactly (an empty
// block after the first ends it; records yielded before a panic are kept, then Panic).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <functional>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "mtblx.h"
#include "mtblx_host.h"

namespace mtbl {

using Bytes = std::vector<uint8_t>;

// src/lib.rs:4-8
constexpr uint64_t DEFAULT_BLOCK_RESTART_INTERVAL = 16;
constexpr uint64_t DEFAULT_BLOCK_SIZE = 8192;
constexpr uint64_t MIN_BLOCK_SIZE = 1024;
constexpr uint64_t METADATA_SIZE = 512;

// src/compression.rs:6-15
enum class CompressionType : uint32_t { None = 0, Snappy = 1, Zlib = 2, Lz4 = 3, Lz4hc = 4, Zstd = 5 };

// src/error.rs:44-52 (+ Io)
enum class MtblError : int {
  InvalidMetadataSize = MTBLX_ERR_INVALID_METADATA_SIZE,
  InvalidIndexBlockOffset = MTBLX_ERR_INVALID_INDEX_BLOCK_OFFSET,
  InvalidIndexLength = MTBLX_ERR_INVALID_INDEX_LENGTH,
  InvalidFormatVersion = MTBLX_ERR_INVALID_FORMAT_VERSION,
  InvalidCompressionAlgorithm = MTBLX_ERR_INVALID_COMPRESSION_ALGORITHM,
  InvalidBlock = MTBLX_ERR_INVALID_BLOCK,
  Io = MTBLX_ERR_IO,
};

inline const char* error_name(MtblError e) {
  switch (e) {
    case MtblError::InvalidMetadataSize: return "InvalidMetadataSize";
    case MtblError::InvalidIndexBlockOffset: return "InvalidIndexBlockOffset";
    case MtblError::InvalidIndexLength: return "InvalidIndexLength";
    case MtblError::InvalidFormatVersion: return "InvalidFormatVersion";
    case MtblError::InvalidCompressionAlgorithm: return "InvalidCompressionAlgorithm";
    case MtblError::InvalidBlock: return "InvalidBlock";
    case MtblError::Io: return "Io";
  }
  return "?";
}

struct Error : std::runtime_error {
  MtblError kind;
  explicit Error(MtblError k) : std::runtime_error(error_name(k)), kind(k) {}
};
struct Panic : std::runtime_error {   // where the reference panics
  explicit Panic(const std::string& w) : std::runtime_error(w) {}
};

namespace detail {
inline void hip_check(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string("HIP: ") + what + ": " + hipGetErrorString(e));
}
inline void abi_check(int rc, const char* what) {
  if (rc != MTBLX_OK) throw std::runtime_error(std::string(what) + " failed: " + std::to_string(rc));
}
// totals[3] bit 1: the launch's look-back timed out and nothing it wrote may be used (mtblx.h)
inline void launch_check(uint64_t flags, const char* what) {
  if (flags & 2ull) throw std::runtime_error(std::string(what) + ": look-back timeout, outputs discarded");
}
// device buffer (hipMalloc), freed with the owner
struct DevBuf {
  void* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  explicit DevBuf(size_t bytes) : n(bytes) { hip_check(hipMalloc(&p, bytes ? bytes : 1), "hipMalloc"); }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { reset(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
    return *this;
  }
  ~DevBuf() { reset(); }
  void reset() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
  template <class T> T* as() const { return static_cast<T*>(p); }
};
// one query of mtblx_block_seek_batch, or -- kbuf allocated: the iterator's key past 64 KiB --
// of mtblx_block_seek_batch_kbuf with the key in kbuf
// (vsrc allocated: mtblx_block_seek_batch_ex, the value bytes left to mtblx_copy_ranges)
inline int block_seek_call(const uint8_t* base, const DevBuf& key, const DevBuf& kend, const DevBuf& q, const DevBuf& k,
                           uint64_t keys_cap, const DevBuf& v, uint64_t vals_cap, const DevBuf& ke, const DevBuf& ve,
                           const DevBuf& kc, uint64_t rec_cap, const DevBuf& kbuf, const DevBuf& vsrc) {
  const auto* kk = static_cast<const uint8_t*>(key.p);
  const auto* kn = static_cast<const uint64_t*>(kend.p);
  auto* qq = static_cast<mtblx_block_seek*>(q.p);
  if (vsrc.p)
    return mtblx_block_seek_batch_ex(base, kk, kn, 1, qq, k.as<uint8_t>(), keys_cap, v.as<uint8_t>(), vals_cap,
                                     ke.as<uint64_t>(), ve.as<uint64_t>(), kc.as<uint64_t>(), rec_cap,
                                     kbuf.p ? kbuf.as<uint8_t>() : nullptr, kbuf.p ? kbuf.n : 0, vsrc.as<uint64_t>(),
                                     nullptr);
  if (kbuf.p)
    return mtblx_block_seek_batch_kbuf(base, kk, kn, 1, qq, k.as<uint8_t>(), keys_cap, v.as<uint8_t>(), vals_cap,
                                       ke.as<uint64_t>(), ve.as<uint64_t>(), kc.as<uint64_t>(), rec_cap,
                                       kbuf.as<uint8_t>(), kbuf.n, nullptr);
  return mtblx_block_seek_batch(base, kk, kn, 1, qq, k.as<uint8_t>(), keys_cap, v.as<uint8_t>(), vals_cap,
                                ke.as<uint64_t>(), ve.as<uint64_t>(), kc.as<uint64_t>(), rec_cap, nullptr);
}
template <class T>
inline DevBuf upload(const T* src, size_t count) {
  DevBuf b(count * sizeof(T));
  if (count) hip_check(hipMemcpy(b.p, src, count * sizeof(T), hipMemcpyHostToDevice), "H2D");
  return b;
}
template <class T>
inline std::vector<T> download(const void* src, size_t count) {
  std::vector<T> v(count);
  if (count) hip_check(hipMemcpy(v.data(), src, count * sizeof(T), hipMemcpyDeviceToHost), "D2H");
  return v;
}

// a key (possibly empty: one readable zero byte) on the device
inline DevBuf upload_key(const Bytes& k) {
  static const uint8_t zero = 0;
  return k.empty() ? upload(&zero, 1) : upload(k.data(), k.size());
}

// decoded blocks, downloaded to the host (the layout of mtblx_decoded)
struct Decoded {
  std::vector<uint32_t> nrec, key_end, val_end;
  std::vector<uint64_t> rec_base, key_base, val_base;
  std::vector<int32_t> status;
  Bytes keys, vals;
  // decode_batch_positions: offset of every record's value in its block's content (vals stays empty)
  std::vector<uint32_t> val_pos;
};

// count -> allocate -> decode -> download, for the batch {data, off, len} on the device.
// positions: mtblx_decode_blocks_valpos -- no value byte is written or downloaded; h.val_pos[r] is
// where record r's value starts in its block (BlockIter::get's val_offset, src/block.rs:204-213).
inline Decoded decode_batch_impl(const uint8_t* d_data, uint64_t data_len, const uint64_t* d_off, const uint32_t* d_len,
                                 uint32_t nblk, uint32_t max_len, bool positions) {
  Decoded h;
  if (nblk == 0) return h;
  mtblx_block_batch in{d_data, data_len, d_off, d_len, nblk, max_len};
  const size_t wsb = mtblx_decode_workspace_bytes(nblk);
  DevBuf ws(wsb);
  hip_check(hipMemset(ws.p, 0, wsb), "memset");
  DevBuf per(8 * 4 * (size_t)nblk + 32);   // nrec | status | rec_base | key_base | val_base | totals
  uint8_t* b = per.as<uint8_t>();
  mtblx_decoded out{};
  out.nrec = reinterpret_cast<uint32_t*>(b);
  out.status = reinterpret_cast<int32_t*>(b + 4ull * nblk);
  out.rec_base = reinterpret_cast<uint64_t*>(b + 8ull * nblk);
  out.key_base = reinterpret_cast<uint64_t*>(b + 16ull * nblk);
  out.val_base = reinterpret_cast<uint64_t*>(b + 24ull * nblk);
  out.totals = reinterpret_cast<uint64_t*>(b + 32ull * nblk);
  abi_check(mtblx_count_blocks(&in, &out, ws.p, wsb, nullptr), "mtblx_count_blocks");
  hip_check(hipDeviceSynchronize(), "sync");
  const auto tot = download<uint64_t>(out.totals, 4);
  launch_check(tot[3], "mtblx_count_blocks");
  DevBuf ke(4 * tot[0] + 4), ve(4 * tot[0] + 4), kk(tot[1] + 1), vv(positions ? 4 * tot[0] + 4 : tot[2] + 1);
  out.key_end = ke.as<uint32_t>();
  out.val_end = ve.as<uint32_t>();
  out.rec_cap = tot[0];
  out.keys = kk.as<uint8_t>();
  out.keys_cap = tot[1];
  if (positions) {
    abi_check(mtblx_decode_blocks_valpos(&in, &out, vv.as<uint32_t>(), ws.p, wsb, nullptr), "mtblx_decode_blocks_valpos");
  } else {
    out.vals = vv.as<uint8_t>();
    out.vals_cap = tot[2];
    abi_check(mtblx_decode_blocks(&in, &out, ws.p, wsb, nullptr), "mtblx_decode_blocks");
  }
  hip_check(hipDeviceSynchronize(), "sync");
  launch_check(download<uint64_t>(out.totals, 4)[3], positions ? "mtblx_decode_blocks_valpos" : "mtblx_decode_blocks");
  h.nrec = download<uint32_t>(out.nrec, nblk);
  h.status = download<int32_t>(out.status, nblk);
  h.rec_base = download<uint64_t>(out.rec_base, nblk);
  h.key_base = download<uint64_t>(out.key_base, nblk);
  h.val_base = download<uint64_t>(out.val_base, nblk);
  h.key_end = download<uint32_t>(out.key_end, tot[0]);
  h.val_end = download<uint32_t>(out.val_end, tot[0]);
  h.keys = download<uint8_t>(out.keys, tot[1]);
  if (positions) h.val_pos = download<uint32_t>(vv.p, tot[0]);
  else h.vals = download<uint8_t>(out.vals, tot[2]);
  return h;
}
inline Decoded decode_batch(const uint8_t* d_data, uint64_t data_len, const uint64_t* d_off, const uint32_t* d_len,
                            uint32_t nblk, uint32_t max_len) {
  return decode_batch_impl(d_data, data_len, d_off, d_len, nblk, max_len, false);
}
// decode_batch with the values left in the batch: value r of block b is the caller's
// data[off[b] + val_pos[r] .. + len), len = val_end[r] - (i ? val_end[r-1] : 0)
inline Decoded decode_batch_positions(const uint8_t* d_data, uint64_t data_len, const uint64_t* d_off,
                                      const uint32_t* d_len, uint32_t nblk, uint32_t max_len) {
  return decode_batch_impl(d_data, data_len, d_off, d_len, nblk, max_len, true);
}
}  // namespace detail

// ------------------------------------------------------------------ Writer (src/writer.rs)
class Writer {
 public:
  Writer(uint64_t block_size, uint64_t restart_interval, CompressionType c, uint32_t level = 0)
      : w_(mtblx_writer_new(block_size, restart_interval, static_cast<uint32_t>(c))) {
    // Lz4 / Lz4hc build a writer whose data-block flushes return Err (Error(Io) below), as the
    // crate's do; NULL = an unknown type, or Zstd without libzstd.so.1 on this host
    if (!w_) throw std::invalid_argument("CompressionType: unknown, or Zstd without libzstd.so.1");
    mtblx_writer_set_level(w_, level);
  }
  Writer(const Writer&) = delete;
  Writer& operator=(const Writer&) = delete;
  Writer(Writer&& o) noexcept : w_(o.w_) { o.w_ = nullptr; }
  ~Writer() { if (w_) mtblx_writer_free(w_); }
  static Writer memory();   // WriterBuilder::default().memory()

  // src/writer.rs:112-149: "out-of-order key" panics; a flush whose compressor returns Err is
  // Err(Io) (the record is not inserted), and the insert after it panics on the data block's
  // `assert!(!self.finished)` (src/block_builder.rs:51)
  void insert(const uint8_t* key, size_t klen, const uint8_t* val, size_t vlen) {
    check(mtblx_writer_insert(w_, key, klen, val, vlen));
  }
  void insert(const Bytes& k, const Bytes& v) { insert(k.data(), k.size(), v.data(), v.size()); }
  void insert(const std::string& k, const std::string& v) {
    insert(reinterpret_cast<const uint8_t*>(k.data()), k.size(), reinterpret_cast<const uint8_t*>(v.data()), v.size());
  }
  // src/writer.rs:155-181: the finished file
  Bytes into_inner() {
    uint8_t* p = nullptr;
    uint64_t n = 0;
    check(mtblx_writer_finish(w_, &p, &n));
    Bytes out(p, p + n);
    mtblx_free(p);
    return out;
  }

 private:
  static void check(int rc) {
    if (rc == MTBLX_OK) return;
    if (rc == MTBLX_E_IO) throw Error(MtblError::Io);
    if (rc == MTBLX_E_FORMAT) throw Panic("out-of-order key");
    throw Panic("BlockBuilder::add: assertion failed (or the writer already panicked)");
  }
  mtblx_writer* w_;
};

class WriterBuilder {   // src/writer.rs:15-80
 public:
  WriterBuilder& compression_type(CompressionType c) { c_ = c; return *this; }
  WriterBuilder& compression_level(uint32_t l) { level_ = l; return *this; }
  WriterBuilder& block_size(uint64_t n) { bs_ = std::max(n, MIN_BLOCK_SIZE); return *this; }
  WriterBuilder& block_restart_interval(uint64_t n) { iv_ = n; return *this; }
  Writer memory() const { return Writer(bs_, iv_, c_, level_); }

 private:
  CompressionType c_ = CompressionType::None;
  uint64_t bs_ = DEFAULT_BLOCK_SIZE, iv_ = DEFAULT_BLOCK_RESTART_INTERVAL;
  uint32_t level_ = 0;   // DEFAULT_COMPRESSION_LEVEL (src/lib.rs:8)
};
inline Writer Writer::memory() { return WriterBuilder().memory(); }

// ------------------------------------------------------------------ Reader (src/reader.rs)
struct Metadata {   // src/metadata.rs:11-24
  uint64_t index_block_offset, data_block_size, compression_algorithm, count_entries, count_data_blocks,
      bytes_data_blocks, bytes_index_block, bytes_keys, bytes_values;
};

struct Record {   // a (key, value) pair served by the iterators (views into the Reader)
  const uint8_t* key;
  size_t key_len;
  const uint8_t* val;
  size_t val_len;
  Bytes key_bytes() const { return Bytes(key, key + key_len); }
  Bytes val_bytes() const { return Bytes(val, val + val_len); }
};

class Reader;
struct MergeReduce;

// one query's answer of Reader::reduce_batch (mtblx.h "Aggregating scans"): nrec records yielded, nbad of
// them with a value of another length than 8 * nfields (left out and counted), fields[f] = op[f] over
// field f of the others (the op's identity over nothing); fields past nfields are 0
struct Reduced {
  uint64_t fields[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint64_t nrec = 0, nbad = 0;
};

// one query of Reader::scan_batch
struct ScanQuery {
  enum Kind { From = 0, Get = 1, Prefix = 2, Range = 3 };   // mtblx_scan_plan's numbering
  Kind kind = From;
  Bytes key;                             // the start key / the key / the prefix
  Bytes key2;                            // Range: the inclusive end
  std::optional<uint64_t> max_records;   // stop after this many records
};

// ReaderIntoIter (src/reader.rs:219-405): built by Reader::into_iter (new), iter_from
// (new_from), iter_prefix (new_get_prefix), iter_range (new_get_range); next() and the
// mid-iteration seek() (:302-335).  The device seeks and decodes (mtblx_index_seek_batch,
// mtblx_block_seek_batch, mtblx_entry_offsets, mtblx_decode_blocks over the blocks the
// iteration reaches, in growing chunks); the host keeps the reference's state: first, valid,
// the index position and block_offset (0 from the constructors, never updated by next(), so a
// seek landing on a block at that offset re-seeks the block the iterator holds, with that
// iterator's key capacity).  seek() re-seeks the LIVE index iterator (:303) and seeks the data
// block to the landed index entry's key (`key` is shadowed at :305).  On a regular index block
// (mtblx_entry_offsets) the index position is a directory entry; on a corrupt one (read with
// verification off) the live index iterator is driven on the device with
// mtblx_block_seek_batch (seek with its key capacity, early return kept, resume), on the scan
// chain or off it.  next() returns a view valid until the next next()/seek(); it throws Error
// where the reference returns Some(Err) (the iterator is then exhausted), Panic where it
// panics or never returns.
class ReaderIntoIter {
 public:
  std::optional<Record> next();
  bool seek(const Bytes& key);   // Ok(true), or throws
  bool seek(const std::string& k) { return seek(Bytes(k.begin(), k.end())); }
  // drain into owned (key, value) pairs
  std::vector<std::pair<Bytes, Bytes>> collect() {
    std::vector<std::pair<Bytes, Bytes>> out;
    while (auto r = next()) out.emplace_back(r->key_bytes(), r->val_bytes());
    return out;
  }

 private:
  friend class Reader;
  enum Kind { kIter = 0, kGet = 1, kPrefix = 2, kRange = 3 };
  struct Content {   // a block's content on the device (decompressed copy for compressed files)
    std::shared_ptr<detail::DevBuf> own;
    const uint8_t* base = nullptr;
    uint64_t off = 0, len = 0;
  };
  struct Bi {        // one BlockIter: the records it yields from its position on (host copies)
    Content c;
    Bytes keys, vals;
    std::vector<uint64_t> ke, ve;   // END offsets
    int end = MTBLX_EMIT_END;       // after the last record
    std::vector<uint64_t> kcaps;    // key capacity at each record (empty + !kcaps_known: replay)
    bool kcaps_known = false;
    uint64_t kcap_end = 0;
    size_t pos = 0;
    std::optional<Bytes> last_val;  // val of the last entry a seek parsed
    size_t n() const { return ke.size(); }
    Record rec(size_t i) const {
      const uint64_t k0 = i ? ke[i - 1] : 0, v0 = i ? ve[i - 1] : 0;
      return Record{keys.data() + k0, (size_t)(ke[i] - k0), vals.data() + v0, (size_t)(ve[i] - v0)};
    }
  };
  struct Loaded {    // a block as next() loads it: an outcome code or the Bi
    int code = 0;    // 0 ok, 1 panic (framing / checksum), 2 Err(Io), 3 Err(InvalidBlock), 4 >= 4 GiB
    Bi bi;
  };
  struct IxList {    // the live index iterator of an irregular index: the records next() visits
    Bi b;            // from its position on (b.pos), emitted by mtblx_block_seek_batch
    uint64_t stop_off = 0;
    int64_t ord0 = -1;   // directory entry of record 0 when on the scan chain, else -1
    bool valid() const { return b.pos < b.n(); }
    uint64_t kcap() const { return valid() ? b.kcaps[b.pos] : b.kcap_end; }
  };
  static constexpr uint64_t kIxEmit = 256;   // index records per emission
  struct EmitResult {
    mtblx_block_seek res;
    Bi b;
  };
  ReaderIntoIter(const Reader* r, Kind t, Bytes k) : r_(r), type_(t), k_(std::move(k)) {}
  void init_iter();
  void init_from(const Bytes& key);
  Bi load(size_t i);
  // BlockIter::seek / seek_to_first / resume on one block content, no status checks
  static EmitResult emit(const Content& c, const Bytes* key, int first, uint64_t kcap, uint64_t max_records,
                         uint64_t resume_off = 0);
  static Bi seek_block(const Content& c, const Bytes* key, uint64_t kcap);   // key null: seek_to_first
  uint64_t kcap_now(Bi& b);
  void ix_seek(const Bytes& key);
  bool ix_next();
  Bi ix_load();
  IxList ix_list(EmitResult&& e, int64_t ord0) const;
  const Reader* r_;
  Kind type_;
  Bytes k_;
  uint64_t block_offset_ = 0;
  bool first_ = true, valid_ = true;
  std::optional<Bi> bi_;
  int64_t e_ = -1;                  // index position, -1: the index iterator is invalid
  std::optional<IxList> ix_;        // irregular index: the live index iterator
  size_t chunk0_ = 0, grow_ = 1;
  std::vector<Loaded> chunk_;
  size_t vchunk0_ = 0;              // irregular index: prefetched blocks of ix_ (by record)
  std::vector<Loaded> vchunk_;
};

class Reader {
 public:
  // Reader::new (src/reader.rs:99-101): ReaderBuilder::default().read(data), checksums on
  static Reader open(const Bytes& data);
  static Reader open(const uint8_t* data, size_t len);
  Metadata metadata() const { return meta_; }
  uint32_t file_version() const { return version_; }   // Metadata::file_version: 0 FormatV1, 1 FormatV2
  // Reader::into_iter (src/reader.rs:124-126)
  ReaderIntoIter into_iter() const {
    ReaderIntoIter it(this, ReaderIntoIter::kIter, {});
    it.init_iter();
    return it;
  }
  // src/reader.rs:111-122, on the device (mtblx_get: index seek -> block_at_index -> BlockIter::seek)
  std::optional<Bytes> get(const uint8_t* key, size_t klen) const;
  std::optional<Bytes> get(const std::string& k) const {
    return get(reinterpret_cast<const uint8_t*>(k.data()), k.size());
  }
  // src/reader.rs:128-138: seek-based, touching only the blocks the iteration reaches
  ReaderIntoIter iter_from(const Bytes& key) const { return make(ReaderIntoIter::kIter, key, key); }
  ReaderIntoIter iter_prefix(const Bytes& prefix) const { return make(ReaderIntoIter::kPrefix, prefix, prefix); }
  ReaderIntoIter iter_range(const Bytes& start, const Bytes& end) const {   // end inclusive
    return make(ReaderIntoIter::kRange, start, end);
  }
  size_t len() const;   // records the full iteration yields before it ends (decodes the file once)
  // iter_from / get / iter_prefix / iter_range for a batch of queries in two launches
  // (mtblx_scan_plan + mtblx_scan_emit): the records of every query, in query order.  Queries the
  // kernels hand back (MTBLX_SCAN_LARGE: more than max_blocks data blocks; MTBLX_SCAN_FALLBACK) go
  // through this Reader's own iter_from / iter_prefix / iter_range / get, which throw where the
  // reference errs or panics; so does every query of a compressed file or an irregular index.
  // served (may be null): per query, 1 where the kernels answered it.
  using Records = std::vector<std::pair<Bytes, Bytes>>;
  std::vector<Records> scan_batch(const std::vector<ScanQuery>& queries, uint32_t max_blocks = 64,
                                  std::vector<uint8_t>* served = nullptr) const;
  // scan_batch that aggregates (mtblx_scan_reduce): per query, `reduce` folded over the values of the
  // records scan_batch would return, in one walk that materialises no record.  The queries the kernel
  // hands back, and every query of a compressed file or an irregular index, go the way scan_batch
  // sends them and their records are folded on the host.  served as in scan_batch.
  std::vector<Reduced> reduce_batch(const std::vector<ScanQuery>& queries, const MergeReduce& reduce,
                                    uint32_t max_blocks = 64, std::vector<uint8_t>* served = nullptr) const;
  // blocks this Reader has decompressed on the host so far (Zlib / Zstd; a Snappy file's blocks are
  // decompressed on the device when the iterator loads them, and on the host only by a seek's own
  // block and by blocks >= 4 GiB)
  uint64_t host_decompressed_blocks() const { return host_dec_blocks_; }

 private:
  friend class ReaderBuilder;
  friend class ReaderIntoIter;
  Reader(const uint8_t* data, size_t len, bool verify);
  ReaderIntoIter make(ReaderIntoIter::Kind t, const Bytes& seek_key, const Bytes& k) const {
    ReaderIntoIter it(this, t, k);
    it.init_from(seek_key);
    return it;
  }
  Records scan_one(const ScanQuery& q) const;   // one query through the iterators
  mtblx_index_seek index_seek(const Bytes& key) const;
  Bytes index_key(size_t i) const {   // separator key of directory entry i
    const uint32_t a = i ? ikend_[i - 1] : 0;
    return Bytes(ikeys_.begin() + a, ikeys_.begin() + ikend_[i]);
  }
  void index_chain() const;
  bool regular() const { index_chain(); return regular_; }
  std::optional<size_t> chain_ordinal(uint64_t entry) const;
  size_t ordinal(uint64_t entry) const;
  ReaderIntoIter::Content index_content() const {
    return ReaderIntoIter::Content{nullptr, dfile_.as<uint8_t>(), index_off_, index_len_};
  }
  ReaderIntoIter::Content seek_content(const mtblx_index_seek& s) const;
  ReaderIntoIter::Content value_content(const Bytes& value) const;
  struct Framing {   // block_at_index + Reader::block framing of some index entries
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    std::vector<int32_t> st;
    std::vector<uint64_t> block_off;   // the block offset (for contents >= 4 GiB)
  };
  Framing frame_values(const std::vector<Bytes>& values) const;
  std::vector<ReaderIntoIter::Loaded> load_range(size_t i0, size_t i1) const;
  std::vector<ReaderIntoIter::Loaded> load_framed(const Framing& f) const;
  void load_big(uint64_t block_off, ReaderIntoIter::Loaded& L) const;
  void load_content(const ReaderIntoIter::Content& c, ReaderIntoIter::Loaded& L) const;
  Bytes file_;
  detail::DevBuf dfile_;
  bool verify_;
  uint32_t version_ = 1;
  Metadata meta_{};
  uint64_t index_off_ = 0, index_len_ = 0;
  uint32_t nent_ = 0;
  int32_t index_status_ = MTBLX_ST_OK;
  std::vector<uint64_t> boff_;
  std::vector<uint32_t> blen_;
  std::vector<int32_t> dst_;
  Bytes ikeys_;                  // the index block's keys (separators) and END offsets
  std::vector<uint32_t> ikend_;
  detail::DevBuf d_off_, d_len_;
  std::vector<std::pair<uint32_t, uint64_t>> big_;   // entries whose content is >= 4 GiB: block offset
  mutable std::vector<uint64_t> eoffs_;
  mutable bool eoffs_known_ = false, regular_ = false;
  mutable std::optional<size_t> len_;
  mutable uint64_t host_dec_blocks_ = 0;
};

class ReaderBuilder {   // src/reader.rs:15-30
 public:
  ReaderBuilder& verify_checksums(bool v) { verify_ = v; return *this; }
  Reader read(const Bytes& data) const { return Reader(data.data(), data.size(), verify_); }
  Reader read(const uint8_t* data, size_t len) const { return Reader(data, len, verify_); }

 private:
  bool verify_ = true;
};

inline Reader Reader::open(const Bytes& data) { return ReaderBuilder().read(data); }
inline Reader Reader::open(const uint8_t* data, size_t len) { return ReaderBuilder().read(data, len); }

inline Reader::Reader(const uint8_t* data, size_t len, bool verify) : file_(data, data + len), verify_(verify) {
  using namespace detail;
  // ReaderBuilder::read (src/reader.rs:31-81): footer, index framing + checksum (host)
  mtblx_footer f{};
  if (mtblx_read_footer(file_.data(), file_.size(), &f) != MTBLX_OK) throw Error(static_cast<MtblError>(f.err));
  std::memcpy(&meta_, f.meta, sizeof(meta_));
  version_ = f.version;
  uint64_t coff = 0, clen = 0;
  int panic = 0;
  const int rc = mtblx_frame_block(file_.data(), file_.size(), version_, meta_.index_block_offset, verify ? 1 : 0,
                                   &coff, &clen, &panic);
  if (panic) throw Panic("index block framing / checksum (src/reader.rs:52-74)");
  if (rc != MTBLX_OK) throw Error(MtblError::InvalidIndexLength);
  index_off_ = coff;
  index_len_ = clen;
  dfile_ = upload(file_.data(), file_.size());
  // the index block, decoded on the device like any block
  const uint64_t ioff = coff;
  const uint32_t ilen = (uint32_t)clen;
  DevBuf d_ioff = upload(&ioff, 1), d_ilen = upload(&ilen, 1);
  const Decoded idx = decode_batch(dfile_.as<uint8_t>(), file_.size(), d_ioff.as<uint64_t>(), d_ilen.as<uint32_t>(),
                                   1, ilen);
  if (idx.status[0] == MTBLX_ST_INVALID_BLOCK) throw Error(MtblError::InvalidBlock);   // src/reader.rs:76
  nent_ = idx.nrec[0];
  index_status_ = idx.status[0];
  ikeys_ = idx.keys;
  ikend_.assign(idx.key_end.begin(), idx.key_end.begin() + nent_);
  // block_at_index + Reader::block framing for every index entry (device); checksums are
  // checked per block when the iteration loads it
  boff_.assign(nent_, 0);
  blen_.assign(nent_, 0);
  dst_.assign(nent_, 0);
  d_off_ = DevBuf(8ull * nent_);
  d_len_ = DevBuf(4ull * nent_);
  if (nent_) {
    DevBuf d_vals = upload(idx.vals.data(), idx.vals.size()), d_vend = upload(idx.val_end.data(), nent_);
    DevBuf d_dst(4ull * nent_);
    abi_check(mtblx_block_dir(dfile_.as<uint8_t>(), file_.size(), version_, d_vals.as<uint8_t>(),
                              d_vend.as<uint32_t>(), 0, nent_, d_off_.as<uint64_t>(), d_len_.as<uint32_t>(),
                              d_dst.as<int32_t>(), nullptr),
              "mtblx_block_dir");
    hip_check(hipDeviceSynchronize(), "sync");
    boff_ = download<uint64_t>(d_off_.p, nent_);
    blen_ = download<uint32_t>(d_len_.p, nent_);
    dst_ = download<int32_t>(d_dst.p, nent_);
    for (uint32_t i = 0; i < nent_; ++i) {   // block_at_index's offset of >= 4 GiB blocks (host)
      if (dst_[i] != MTBLX_DIR_UNSUPPORTED) continue;
      const uint32_t v0 = i ? idx.val_end[i - 1] : 0;
      uint64_t o = 0;
      mtblx_varint_decode64(idx.vals.data() + v0, idx.val_end[i] - v0, &o);
      big_.emplace_back(i, o);
    }
  }
}

// blocks [i0, i1) as next() loads them: Reader::block (framing, checksum, host decompression
// -- compression stays on the host per the north star) + one device decode of the range
inline std::vector<ReaderIntoIter::Loaded> Reader::load_range(size_t i0, size_t i1) const {
  Framing f;
  f.off.assign(boff_.begin() + i0, boff_.begin() + i1);
  f.len.assign(blen_.begin() + i0, blen_.begin() + i1);
  f.st.assign(dst_.begin() + i0, dst_.begin() + i1);
  f.block_off.assign(i1 - i0, 0);
  for (const auto& e : big_)
    if (e.first >= i0 && e.first < i1) f.block_off[e.first - i0] = e.second;
  return load_framed(f);
}

// block_at_index + Reader::block framing of arbitrary index values on the device (mtblx_block_dir)
inline Reader::Framing Reader::frame_values(const std::vector<Bytes>& values) const {
  using namespace detail;
  const uint32_t n = (uint32_t)values.size();
  Framing f;
  Bytes blob;
  std::vector<uint32_t> vend(n);
  for (uint32_t i = 0; i < n; ++i) {
    blob.insert(blob.end(), values[i].begin(), values[i].end());
    vend[i] = (uint32_t)blob.size();
  }
  if (blob.empty()) blob.push_back(0);
  DevBuf d_v = upload(blob.data(), blob.size()), d_ve = upload(vend.data(), n);
  DevBuf d_o(8ull * n), d_l(4ull * n), d_s(4ull * n);
  abi_check(mtblx_block_dir(dfile_.as<uint8_t>(), file_.size(), version_, d_v.as<uint8_t>(), d_ve.as<uint32_t>(), 0, n,
                            d_o.as<uint64_t>(), d_l.as<uint32_t>(), d_s.as<int32_t>(), nullptr),
            "mtblx_block_dir");
  hip_check(hipDeviceSynchronize(), "sync");
  f.off = download<uint64_t>(d_o.p, n);
  f.len = download<uint32_t>(d_l.p, n);
  f.st = download<int32_t>(d_s.p, n);
  f.block_off.assign(n, 0);
  for (uint32_t i = 0; i < n; ++i)
    if (f.st[i] == MTBLX_DIR_UNSUPPORTED) mtblx_varint_decode64(values[i].data(), values[i].size(), &f.block_off[i]);
  return f;
}

inline std::vector<ReaderIntoIter::Loaded> Reader::load_framed(const Framing& f) const {
  using namespace detail;
  const uint32_t n = (uint32_t)f.off.size();
  std::vector<ReaderIntoIter::Loaded> out(n);
  std::vector<uint8_t> bad(n, 0);
  std::vector<uint32_t> l2(f.len);
  for (uint32_t i = 0; i < n; ++i)
    if (f.st[i] != MTBLX_DIR_OK) l2[i] = 0;   // never decoded: the iteration stops before it
  DevBuf d_l2 = upload(l2.data(), n), d_off = upload(f.off.data(), n);
  const uint64_t* d_o = d_off.as<uint64_t>();
  const uint32_t mx = n ? *std::max_element(l2.begin(), l2.end()) : 0;
  if (verify_ && n) {
    DevBuf d_bad(n);
    mtblx_block_batch in{dfile_.as<uint8_t>(), file_.size(), d_o, d_l2.as<uint32_t>(), n, mx};
    abi_check(mtblx_crc32c_blocks(&in, nullptr, d_bad.as<uint8_t>(), 1, nullptr), "mtblx_crc32c_blocks");
    hip_check(hipDeviceSynchronize(), "sync");
    bad = download<uint8_t>(d_bad.p, n);
  }
  std::vector<uint8_t> zerr(n, 0);
  std::shared_ptr<DevBuf> ubuf;
  std::vector<uint64_t> uoff(n, 0);
  std::vector<uint32_t> ul(n, 0);
  std::vector<uint64_t> ulen(n, 0);
  Decoded dec;
  if (meta_.compression_algorithm == 1 && n) {
    // Snappy: the stored bytes stay on the device (mtblx_stage_plan / _emit); a preamble is a u32, so
    // no decompressed content here is >= 4 GiB
    DevBuf d_st = upload(f.st.data(), n), d_bad = upload(bad.data(), n);
    const size_t wsb = mtblx_stage_workspace_bytes(n);
    DevBuf ws(wsb);
    uint64_t tot[3] = {0, 0, 0};
    abi_check(mtblx_stage_plan(dfile_.as<uint8_t>(), file_.size(), d_o, d_l2.as<uint32_t>(), d_st.as<int32_t>(),
                               d_bad.as<uint8_t>(), n, nullptr, 0, tot, ws.p, wsb, nullptr),
              "mtblx_stage_plan");
    ubuf = std::make_shared<DevBuf>(tot[0] + 16);
    DevBuf d_uo(8ull * n), d_ul(4ull * n), t0(8ull * n), t1(8ull * n), t2(8ull * n), t3(4ull * n);
    abi_check(mtblx_stage_emit(dfile_.as<uint8_t>(), file_.size(), d_o, n, nullptr, 0, ubuf->as<uint8_t>(), tot[0] + 16, 0,
                               tot[0], (uint32_t)tot[1], d_uo.as<uint64_t>(), d_ul.as<uint32_t>(), t0.as<uint64_t>(),
                               t1.as<uint64_t>(), t2.as<uint64_t>(), t3.as<int32_t>(), 0, ws.p, wsb, nullptr),
              "mtblx_stage_emit");
    hip_check(hipDeviceSynchronize(), "sync");
    uoff = download<uint64_t>(d_uo.p, n);
    ul = download<uint32_t>(d_ul.p, n);
    const std::vector<int32_t> zst = download<int32_t>(t3.p, n);
    uint32_t umx = 0;
    for (uint32_t i = 0; i < n; ++i) {
      zerr[i] = zst[i] != 0;
      ulen[i] = ul[i];
      umx = std::max(umx, ul[i]);
    }
    dec = decode_batch(ubuf->as<uint8_t>(), tot[0] + 16, d_uo.as<uint64_t>(), d_ul.as<uint32_t>(), n, umx);
  } else if (meta_.compression_algorithm != 0) {
    std::vector<uint64_t> so(n, 0);
    std::vector<uint32_t> sn(n, 0);
    std::vector<int32_t> zst(n, 0);
    for (uint32_t i = 0; i < n; ++i)
      if (f.st[i] == MTBLX_DIR_OK && !bad[i]) { so[i] = f.off[i]; sn[i] = f.len[i]; ++host_dec_blocks_; }
    uint8_t* hb = nullptr;
    mtblx_decompress_blocks(static_cast<uint32_t>(meta_.compression_algorithm), file_.data(), so.data(), sn.data(), n,
                            16, &hb, uoff.data(), ulen.data(), zst.data());
    if (!hb) throw std::bad_alloc();
    uint32_t umx = 0;
    uint64_t tot = 0;
    for (uint32_t i = 0; i < n; ++i) {
      zerr[i] = sn[i] && zst[i] != MTBLX_CODEC_OK;
      // a content >= 4 GiB stays out of the batch (u32 lengths): the emitting seek decodes it below
      ul[i] = zerr[i] || ulen[i] > 0xFFFFFFFFull ? 0u : (uint32_t)ulen[i];
      umx = std::max(umx, ul[i]);
      tot = std::max(tot, uoff[i] + ulen[i]);
    }
    ubuf = std::make_shared<DevBuf>(tot + 1);
    if (tot) hip_check(hipMemcpy(ubuf->p, hb, tot, hipMemcpyHostToDevice), "H2D");
    mtblx_free(hb);
    DevBuf d_uo = upload(uoff.data(), n), d_ul = upload(ul.data(), n);
    dec = decode_batch(ubuf->as<uint8_t>(), tot + 1, d_uo.as<uint64_t>(), d_ul.as<uint32_t>(), n, umx);
  } else {
    dec = decode_batch(dfile_.as<uint8_t>(), file_.size(), d_o, d_l2.as<uint32_t>(), n, mx);
  }
  for (uint32_t i = 0; i < n; ++i) {
    auto& L = out[i];
    if (f.st[i] == MTBLX_DIR_UNSUPPORTED) {   // content >= 4 GiB (u64 restart array)
      load_big(f.block_off[i], L);
      continue;
    }
    if (f.st[i] != MTBLX_DIR_OK || bad[i]) { L.code = 1; continue; }
    if (zerr[i]) { L.code = 2; continue; }
    if (ubuf && ulen[i] > 0xFFFFFFFFull) {   // decompressed content >= 4 GiB (u64 restart array)
      load_content(ReaderIntoIter::Content{ubuf, ubuf->as<uint8_t>(), uoff[i], ulen[i]}, L);
      continue;
    }
    const int32_t s = dec.status[i];
    if (s == MTBLX_ST_INVALID_BLOCK) { L.code = 3; continue; }
    if (s == MTBLX_ST_UNSUPPORTED) { L.code = 4; continue; }
    auto& b = L.bi;
    if (ubuf) b.c = ReaderIntoIter::Content{ubuf, ubuf->as<uint8_t>(), uoff[i], ul[i]};
    else b.c = ReaderIntoIter::Content{nullptr, dfile_.as<uint8_t>(), f.off[i], f.len[i]};
    b.end = s == MTBLX_ST_CORRUPT ? MTBLX_EMIT_PANIC : s == MTBLX_ST_LOOP ? MTBLX_EMIT_LOOP : MTBLX_EMIT_END;
    const uint64_t r0 = dec.rec_base[i], kb = dec.key_base[i], vb = dec.val_base[i];
    uint64_t kend = 0, vend = 0;
    for (uint32_t q = 0; q < dec.nrec[i]; ++q) {
      kend = dec.key_end[r0 + q];
      vend = dec.val_end[r0 + q];
      b.ke.push_back(kend);
      b.ve.push_back(vend);
    }
    b.keys.assign(dec.keys.begin() + kb, dec.keys.begin() + kb + kend);
    b.vals.assign(dec.vals.begin() + vb, dec.vals.begin() + vb + vend);
  }
  return out;
}

// Reader::block + Block::init + the scan of a block >= 4 GiB: framing and checksum on the host
// (mtblx_frame_block), the scan on the device (the emitting block seek, seek_to_first)
inline void Reader::load_big(uint64_t boff, ReaderIntoIter::Loaded& L) const {
  using namespace detail;
  uint64_t coff = 0, clen = 0;
  int panic = 0;
  if (mtblx_frame_block(file_.data(), file_.size(), version_, boff, verify_ ? 1 : 0, &coff, &clen, &panic) != MTBLX_OK) {
    L.code = 1;
    return;
  }
  if (meta_.compression_algorithm == 0) {
    load_content(ReaderIntoIter::Content{nullptr, dfile_.as<uint8_t>(), coff, clen}, L);
    return;
  }
  uint8_t* hb = nullptr;   // src/reader.rs:166-170 on the host, any size
  uint64_t un = 0;
  ++host_dec_blocks_;
  if (mtblx_decompress(static_cast<uint32_t>(meta_.compression_algorithm), file_.data() + coff, clen, &hb, &un) !=
      MTBLX_CODEC_OK) {
    if (hb) mtblx_free(hb);
    L.code = 2;
    return;
  }
  auto buf = std::make_shared<DevBuf>(un + 1);
  if (un) hip_check(hipMemcpy(buf->p, hb, un, hipMemcpyHostToDevice), "H2D");
  mtblx_free(hb);
  load_content(ReaderIntoIter::Content{buf, buf->as<uint8_t>(), 0, un}, L);
}

// Block::init + seek_to_first + the records of one content (any size) on the device
inline void Reader::load_content(const ReaderIntoIter::Content& c, ReaderIntoIter::Loaded& L) const {
  try {
    L.bi = ReaderIntoIter::seek_block(c, nullptr, 0);
  } catch (const Error&) {
    L.code = 3;
  } catch (const Panic&) {
    L.code = 1;
  }
}

inline size_t Reader::len() const {
  if (!len_) {
    ReaderIntoIter it = into_iter();
    size_t n = 0;
    try {
      while (it.next()) ++n;
    } catch (const std::exception&) {   // the records before an Err / panic count
    }
    len_ = n;
  }
  return *len_;
}

inline mtblx_index_seek Reader::index_seek(const Bytes& key) const {
  using namespace detail;
  const uint64_t kend = key.size();
  DevBuf d_key = upload_key(key), d_kend = upload(&kend, 1);
  DevBuf d_out(sizeof(mtblx_index_seek));
  abi_check(mtblx_index_seek_batch(dfile_.as<uint8_t>(), file_.size(), version_, verify_ ? 1 : 0, index_off_,
                                   index_len_, d_key.as<uint8_t>(), d_kend.as<uint64_t>(), 1,
                                   d_out.as<mtblx_index_seek>(), nullptr),
            "mtblx_index_seek_batch");
  hip_check(hipDeviceSynchronize(), "sync");
  return download<mtblx_index_seek>(d_out.p, 1)[0];
}

// the index scan chain's entry offsets and whether the index block is regular (mtblx.h)
inline void Reader::index_chain() const {
  using namespace detail;
  if (eoffs_known_) return;
  const uint64_t cap = index_len_ / 3 + 1;   // an entry takes >= 3 bytes
  DevBuf d_offs(8ull * cap), d_cnt(8), d_reg(4);
  abi_check(mtblx_entry_offsets(dfile_.as<uint8_t>() + index_off_, index_len_, d_offs.as<uint64_t>(), cap,
                                d_cnt.as<uint64_t>(), d_reg.as<uint32_t>(), nullptr),
            "mtblx_entry_offsets");
  hip_check(hipDeviceSynchronize(), "sync");
  const uint64_t cnt = std::min<uint64_t>(download<uint64_t>(d_cnt.p, 1)[0], cap);
  eoffs_ = download<uint64_t>(d_offs.p, cnt);
  regular_ = download<uint32_t>(d_reg.p, 1)[0] == 1 && index_status_ == MTBLX_ST_OK;
  eoffs_known_ = true;
}

inline std::optional<size_t> Reader::chain_ordinal(uint64_t entry) const {
  index_chain();
  const auto it = std::lower_bound(eoffs_.begin(), eoffs_.end(), entry);
  if (it == eoffs_.end() || *it != entry) return std::nullopt;
  return (size_t)(it - eoffs_.begin());
}

inline size_t Reader::ordinal(uint64_t entry) const {   // a regular index's landing
  const auto o = chain_ordinal(entry);
  if (!o || *o >= nent_) throw std::runtime_error("index seek landed off the directory of a regular index");
  return *o;
}

// Reader::block (src/reader.rs:139-175) at the offset an index value names: framing and
// checksum (host), decompression (host) -> the content BlockIter reads; throws like the crate
inline ReaderIntoIter::Content Reader::value_content(const Bytes& value) const {
  using namespace detail;
  uint64_t boff = 0;
  if (mtblx_varint_decode64(value.data(), value.size(), &boff) < 0) throw Panic("varint_decode64 of the index value");
  uint64_t coff = 0, clen = 0;
  int panic = 0;
  mtblx_frame_block(file_.data(), file_.size(), version_, boff, verify_ ? 1 : 0, &coff, &clen, &panic);
  if (panic) throw Panic("Reader::block: framing / checksum");
  if (meta_.compression_algorithm == 0) return ReaderIntoIter::Content{nullptr, dfile_.as<uint8_t>(), coff, clen};
  uint8_t* out = nullptr;
  uint64_t n = 0;
  ++host_dec_blocks_;
  if (mtblx_decompress(static_cast<uint32_t>(meta_.compression_algorithm), file_.data() + coff, clen, &out, &n) !=
      MTBLX_CODEC_OK)
    throw Error(MtblError::Io);
  auto own = std::make_shared<DevBuf>(upload(out, n ? n : 1));
  mtblx_free(out);
  return ReaderIntoIter::Content{own, own->as<uint8_t>(), 0, n};
}

inline ReaderIntoIter::Content Reader::seek_content(const mtblx_index_seek& s) const {
  using namespace detail;
  if (s.block_status == MTBLX_SEEK_PANIC) throw Panic("Reader::block");
  if (meta_.compression_algorithm == 0) {
    if (s.block_status == MTBLX_SEEK_ERR) throw Error(MtblError::InvalidBlock);
    if (s.block_status == MTBLX_SEEK_UNSUPPORTED) throw std::runtime_error("index seek: unexpected block status");
    return ReaderIntoIter::Content{nullptr, dfile_.as<uint8_t>(), s.data_off, s.data_len};
  }
  // compressed: decompress on the host, Block::init runs on the result (mtblx_block_seek_batch)
  uint8_t* out = nullptr;
  uint64_t n = 0;
  ++host_dec_blocks_;
  if (mtblx_decompress(static_cast<uint32_t>(meta_.compression_algorithm), file_.data() + s.data_off, s.data_len, &out,
                       &n) != MTBLX_CODEC_OK)
    throw Error(MtblError::Io);
  auto own = std::make_shared<DevBuf>(upload(out, n ? n : 1));
  mtblx_free(out);
  return ReaderIntoIter::Content{own, own->as<uint8_t>(), 0, n};
}

inline ReaderIntoIter::EmitResult ReaderIntoIter::emit(const Content& c, const Bytes* key, int first, uint64_t kcap,
                                                       uint64_t max_records, uint64_t resume_off) {
  using namespace detail;
  mtblx_block_seek q{};
  q.data_off = c.off;
  q.data_len = c.len;
  q.kcap = kcap;
  q.max_records = max_records;
  q.first = first;
  q.resume_off = resume_off;
  // output sized exactly from a first counting pass when the block is big (>= 4 GiB blocks)
  const bool big = c.len > (64ull << 20);
  uint64_t rec_cap = std::min<uint64_t>(max_records, big ? 4096 : c.len / 3 + 1),
           keys_cap = big ? 1 << 20 : 2 * c.len + 64, vals_cap = big ? 1 << 20 : c.len + 16;
  const Bytes none;
  const uint64_t kend = key ? key->size() : 0;
  DevBuf d_key = upload_key(key ? *key : none), d_kend = upload(&kend, 1);
  DevBuf kbuf;   // allocated once a key runs past the 64 KiB LDS key
  for (int attempt = 0; attempt < 4; ++attempt) {
    DevBuf d_q = upload(&q, 1), d_k(keys_cap + 1), d_v(vals_cap + 1), d_ke(8 * rec_cap + 8), d_ve(8 * rec_cap + 8),
        d_kc(8 * rec_cap + 8);
    DevBuf d_vs = big ? DevBuf(8 * rec_cap + 8) : DevBuf();   // big blocks: values moved by the whole grid
    abi_check(block_seek_call(c.base, d_key, d_kend, d_q, d_k, keys_cap, d_v, vals_cap, d_ke, d_ve, d_kc, rec_cap, kbuf,
                              d_vs),
              "mtblx_block_seek_batch");
    hip_check(hipDeviceSynchronize(), "sync");
    EmitResult r;
    r.res = download<mtblx_block_seek>(d_q.p, 1)[0];
    if (r.res.status == MTBLX_SEEK_UNSUPPORTED && !kbuf.p) {   // any key this iterator can build fits
      kbuf = DevBuf(kend + c.len + 64);
      continue;
    }
    if (r.res.end == MTBLX_EMIT_OVERFLOW) {
      rec_cap = r.res.nrec;
      keys_cap = r.res.key_bytes;
      vals_cap = r.res.val_bytes;
      continue;
    }
    Bi& b = r.b;
    b.c = c;
    b.end = r.res.end;
    b.ke = download<uint64_t>(d_ke.p, r.res.nrec);
    b.ve = download<uint64_t>(d_ve.p, r.res.nrec);
    b.kcaps = download<uint64_t>(d_kc.p, r.res.nrec);
    b.kcaps_known = true;
    b.kcap_end = r.res.kcap;
    b.keys = download<uint8_t>(d_k.p, r.res.key_bytes);
    if (big && r.res.nrec) {   // the values: mtblx_copy_ranges from the block content
      const std::vector<uint64_t> vs = download<uint64_t>(d_vs.p, r.res.nrec);
      std::vector<uint64_t> so(r.res.nrec), dofs(r.res.nrec), ln(r.res.nrec), cb(r.res.nrec);
      uint64_t prev = 0, chunks = 0;
      for (uint64_t i = 0; i < r.res.nrec; ++i) {
        so[i] = c.off + vs[i];
        dofs[i] = prev;
        ln[i] = b.ve[i] - prev;
        cb[i] = chunks;
        chunks += (ln[i] + 15) / 16;
        prev = b.ve[i];
      }
      DevBuf d_so = upload(so.data(), so.size()), d_do = upload(dofs.data(), dofs.size()),
             d_ln = upload(ln.data(), ln.size()), d_cb = upload(cb.data(), cb.size());
      abi_check(mtblx_copy_ranges(c.base, d_so.as<uint64_t>(), d_v.as<uint8_t>(), d_do.as<uint64_t>(),
                                  d_ln.as<uint64_t>(), d_cb.as<uint64_t>(), (uint32_t)r.res.nrec, chunks, nullptr),
                "mtblx_copy_ranges");
      hip_check(hipDeviceSynchronize(), "sync");
    }
    b.vals = download<uint8_t>(d_v.p, r.res.val_bytes);
    // (a corrupt entry's value may run past the content: ReaderIntoGet could not slice it either)
    if (r.res.has_val && r.res.last_voff <= c.len && r.res.last_vlen <= c.len - r.res.last_voff)
      b.last_val = download<uint8_t>(c.base + c.off + r.res.last_voff, r.res.last_vlen);
    return r;
  }
  throw std::runtime_error("mtblx_block_seek_batch: output sizes did not converge");
}

inline ReaderIntoIter::Bi ReaderIntoIter::seek_block(const Content& c, const Bytes* key, uint64_t kcap) {
  EmitResult r = emit(c, key, key ? 0 : 1, kcap, ~0ull >> 2);
  if (r.res.status == MTBLX_SEEK_ERR) throw Error(MtblError::InvalidBlock);
  if (r.res.status == MTBLX_SEEK_PANIC) throw Panic("BlockIter::seek");
  if (r.res.status == MTBLX_SEEK_LOOP) throw Panic("BlockIter::seek never returns");
  if (r.res.status == MTBLX_SEEK_UNSUPPORTED) throw std::runtime_error("emitting seek: key buffer too small");
  return std::move(r.b);
}

// the key Vec's capacity of the held iterator now (parse_next_key's END leaves it unchanged)
inline uint64_t ReaderIntoIter::kcap_now(Bi& b) {
  using namespace detail;
  if (b.n() == 0) return b.kcap_end;
  if (!b.kcaps_known) {   // records from the bulk decoder: replay seek_to_first + next on the device
    mtblx_block_seek q{};
    q.data_off = b.c.off;
    q.data_len = b.c.len;
    q.max_records = b.n();
    q.first = 1;
    const uint64_t kend = 0;
    const uint8_t z = 0;
    DevBuf d_key = upload(&z, 1), d_kend = upload(&kend, 1), d_q = upload(&q, 1);
    // only the key capacities are needed: the value bytes are deferred (vsrc) and never moved
    DevBuf d_k(2 * b.c.len + 65), d_v, d_ke(8 * b.n() + 8), d_ve(8 * b.n() + 8), d_kc(8 * b.n() + 8),
        d_vs(8 * b.n() + 8);
    DevBuf kbuf;
    for (int attempt = 0; attempt < 2; ++attempt) {
      abi_check(block_seek_call(b.c.base, d_key, d_kend, d_q, d_k, 2 * b.c.len + 64, d_v, b.c.len + 16, d_ke, d_ve, d_kc,
                                b.n(), kbuf, d_vs),
                "mtblx_block_seek_batch");
      hip_check(hipDeviceSynchronize(), "sync");
      if (download<mtblx_block_seek>(d_q.p, 1)[0].status != MTBLX_SEEK_UNSUPPORTED || kbuf.p) break;
      kbuf = DevBuf(b.c.len + 64);   // a key past 64 KiB: again with the key in device memory
      hip_check(hipMemcpy(d_q.p, &q, sizeof(q), hipMemcpyHostToDevice), "H2D");
    }
    b.kcaps = download<uint64_t>(d_kc.p, b.n());
    b.kcaps_known = true;
  }
  return b.kcaps[std::min(b.pos, b.n() - 1)];
}

inline ReaderIntoIter::Bi ReaderIntoIter::load(size_t i) {
  if (chunk_.empty() || i < chunk0_ || i >= chunk0_ + chunk_.size()) {
    const size_t n = std::min<size_t>(r_->nent_ - i, grow_);
    grow_ = std::min<size_t>(2 * grow_, 256);
    chunk_ = r_->load_range(i, i + n);
    chunk0_ = i;
  }
  Loaded& L = chunk_[i - chunk0_];
  switch (L.code) {
    case 1: throw Panic("Reader::block: framing / checksum");
    case 2: throw Error(MtblError::Io);
    case 3: throw Error(MtblError::InvalidBlock);
    case 4: throw std::runtime_error("block >= 4 GiB");
  }
  return L.bi;
}

inline ReaderIntoIter::IxList ReaderIntoIter::ix_list(EmitResult&& e, int64_t ord0) const {
  if (e.res.status == MTBLX_SEEK_PANIC) throw Panic("index seek");
  if (e.res.status == MTBLX_SEEK_LOOP) throw Panic("index seek never returns");
  if (e.res.status == MTBLX_SEEK_UNSUPPORTED) throw std::runtime_error("emitting seek: key buffer too small");
  IxList l;
  l.b = std::move(e.b);
  l.stop_off = e.res.stop_off;
  l.ord0 = ord0;
  return l;
}

inline void ReaderIntoIter::init_iter() {   // new (src/reader.rs:231-254)
  if (r_->nent_ == 0) {
    if (r_->index_status_ == MTBLX_ST_CORRUPT) throw Panic("index block: first entry");
    if (!r_->regular()) ix_ = IxList{};
    return;
  }
  if (r_->regular()) {
    e_ = 0;
  } else {   // the scan's own chain = the directory, with its key capacities
    ix_ = ix_list(emit(r_->index_content(), nullptr, 1, 0, kIxEmit), 0);
  }
  bi_ = load(0);
}

inline void ReaderIntoIter::init_from(const Bytes& key) {   // new_from (src/reader.rs:256-279)
  if (!r_->regular()) {   // a fresh live index iterator, seeked
    ix_ = IxList{};
    ix_seek(key);
    if (!ix_->valid()) return;
    bi_ = seek_block(r_->value_content(ix_->b.rec(ix_->b.pos).val_bytes()), &key, 0);
    return;
  }
  const mtblx_index_seek s = r_->index_seek(key);
  if (s.status == MTBLX_SEEK_PANIC) throw Panic("index seek");
  if (s.status == MTBLX_SEEK_LOOP) throw Panic("index seek never returns");
  if (!s.valid) return;
  e_ = (int64_t)r_->ordinal(s.entry);
  bi_ = seek_block(r_->seek_content(s), &key, 0);
}

// index_iter.seek(key) on the live iterator of an irregular index (src/block.rs:154-194)
inline void ReaderIntoIter::ix_seek(const Bytes& key) {
  EmitResult e = emit(r_->index_content(), &key, 0, ix_->kcap(), kIxEmit);
  if (e.res.status == MTBLX_SEEK_OK && e.res.early) return;   // corrupt restart: the old position stays
  int64_t ord0 = -1;
  if (e.res.status == MTBLX_SEEK_OK && e.res.nrec) {
    const auto o = r_->chain_ordinal(e.res.entry);
    if (o) ord0 = (int64_t)*o;
  }
  ix_ = ix_list(std::move(e), ord0);
  vchunk_.clear();
}

// index_iter.next() (src/block.rs:196-202) on the live iterator
inline bool ReaderIntoIter::ix_next() {
  IxList& ix = *ix_;
  if (!ix.valid()) return false;
  if (ix.b.pos + 1 < ix.b.n()) { ++ix.b.pos; return true; }
  if (ix.b.end == MTBLX_EMIT_END) { ix.b.pos = ix.b.n(); return false; }
  if (ix.b.end == MTBLX_EMIT_PANIC) throw Panic("index block: next entry");
  if (ix.b.end == MTBLX_EMIT_LOOP) return true;   // a zero-progress entry: the same record again
  // EMIT_MAX: the entry after the last record, parsed from that record's key and capacity
  const Bytes k = ix.b.rec(ix.b.n() - 1).key_bytes();
  EmitResult e = emit(r_->index_content(), &k, 2, ix.b.kcaps.back(), kIxEmit, ix.stop_off);
  if (e.res.status == MTBLX_SEEK_PANIC) throw Panic("index block: next entry");
  const int64_t ord0 = ix.ord0 < 0 ? -1 : ix.ord0 + (int64_t)ix.b.n();
  ix_ = ix_list(std::move(e), ord0);
  vchunk_.clear();
  return ix_->valid();
}

// block_at_index of the live index iterator's record (Reader::block + seek_to_first)
inline ReaderIntoIter::Bi ReaderIntoIter::ix_load() {
  const IxList& ix = *ix_;
  const size_t pos = ix.b.pos;
  if (ix.ord0 >= 0 && (size_t)ix.ord0 + pos < r_->nent_) return load((size_t)ix.ord0 + pos);
  if (vchunk_.empty() || pos < vchunk0_ || pos >= vchunk0_ + vchunk_.size()) {
    const size_t n = std::min<size_t>(ix.b.n() - pos, grow_);
    grow_ = std::min<size_t>(2 * grow_, 256);
    std::vector<Bytes> vals;
    for (size_t q = pos; q < pos + n; ++q) vals.push_back(ix.b.rec(q).val_bytes());
    vchunk_ = r_->load_framed(r_->frame_values(vals));
    vchunk0_ = pos;
  }
  Loaded& L = vchunk_[pos - vchunk0_];
  switch (L.code) {
    case 1: throw Panic("Reader::block: framing / checksum");
    case 2: throw Error(MtblError::Io);
    case 3: throw Error(MtblError::InvalidBlock);
    case 4: throw std::runtime_error("block >= 4 GiB");
  }
  return L.bi;
}

inline std::optional<Record> ReaderIntoIter::next() {   // src/reader.rs:337-405
  if (!valid_ || !bi_) return std::nullopt;
  Bi* b = &*bi_;
  if (!first_ && b->pos < b->n()) ++b->pos;   // bi.next()
  first_ = false;
  if (b->pos == b->n() && b->end == MTBLX_EMIT_PANIC) throw Panic("BlockIter::next / get");
  if (b->pos == b->n() && b->end == MTBLX_EMIT_LOOP) throw Panic("zero-progress entry: the reference never returns");
  if (b->pos == b->n()) {
    valid_ = false;
    if (ix_) {                                // irregular index: the live index iterator
      if (!ix_next()) return std::nullopt;
      Bi nb = ix_load();                      // Some(Err(e)) throws; valid stays false
      bi_ = std::move(nb);
    } else {
      if (e_ < 0) return std::nullopt;
      if ((size_t)e_ + 1 >= r_->nent_) {       // index_iter.next() past the last entry
        e_ = -1;
        if (r_->index_status_ == MTBLX_ST_CORRUPT) throw Panic("index block: next entry");
        if (r_->index_status_ == MTBLX_ST_LOOP) throw Panic("index block never returns");
        return std::nullopt;
      }
      ++e_;
      Bi nb = load((size_t)e_);                // Some(Err(e)) throws; valid stays false
      bi_ = std::move(nb);
    }
    b = &*bi_;
    if (b->n() == 0 && b->end == MTBLX_EMIT_PANIC) throw Panic("BlockIter::seek_to_first / get");
    if (b->n() == 0) return std::nullopt;
    valid_ = true;
  }
  const Record rec = b->rec(b->pos);
  const size_t kl = k_.size();
  if (type_ == kGet) {
    valid_ = rec.key_len == kl && (kl == 0 || std::memcmp(rec.key, k_.data(), kl) == 0);
  } else if (type_ == kPrefix) {
    valid_ = rec.key_len >= kl && (kl == 0 || std::memcmp(rec.key, k_.data(), kl) == 0);
  } else if (type_ == kRange) {
    const size_t m = std::min(rec.key_len, kl);
    const int c = m ? std::memcmp(rec.key, k_.data(), m) : 0;
    valid_ = !(c > 0 || (c == 0 && rec.key_len > kl));
  }
  if (!valid_) return std::nullopt;
  return rec;
}

// src/reader.rs:302-335: the block is seeked to the landed index entry's key (:305 shadows `key`)
inline bool ReaderIntoIter::seek(const Bytes& key) {
  Bytes ikey;
  uint64_t new_off = 0;
  std::optional<mtblx_index_seek> s;
  if (ix_) {                        // irregular index: the live index iterator
    ix_seek(key);
    if (!ix_->valid()) {
      valid_ = false;
      return true;
    }
    const Record ir = ix_->b.rec(ix_->b.pos);
    ikey = ir.key_bytes();
    if (mtblx_varint_decode64(ir.val, ir.val_len, &new_off) < 0) throw Panic("varint_decode64 of the index value");
  } else {
    s = r_->index_seek(key);
    if (s->status == MTBLX_SEEK_PANIC) throw Panic("index seek");
    if (s->status == MTBLX_SEEK_LOOP) throw Panic("index seek never returns");
    if (!s->valid) {   // past the last key: next() returns None
      valid_ = false;
      e_ = -1;
      return true;
    }
    e_ = (int64_t)r_->ordinal(s->entry);
    ikey = r_->index_key((size_t)e_);
    new_off = s->block_off;
  }
  if (block_offset_ != new_off) {
    block_offset_ = new_off;   // updated before the load (:322)
    Bi nb = seek_block(s ? r_->seek_content(*s) : r_->value_content(ix_->b.rec(ix_->b.pos).val_bytes()), &ikey, 0);
    bi_ = std::move(nb);
  } else if (bi_) {                 // the held block, whatever it is
    Bi nb = seek_block(bi_->c, &ikey, kcap_now(*bi_));
    bi_ = std::move(nb);
  }
  first_ = true;
  valid_ = true;
  return true;
}

inline std::optional<Bytes> Reader::get(const uint8_t* key, size_t klen) const {
  using namespace detail;
  if (meta_.compression_algorithm != 0) {   // values live in decompressed blocks: the seek iterator
    ReaderIntoIter it(this, ReaderIntoIter::kGet, Bytes(key, key + klen));
    it.init_from(Bytes(key, key + klen));
    std::optional<Bytes> held = it.bi_ ? it.bi_->last_val : std::nullopt;
    try {
      auto r = it.next();
      if (!r) return std::nullopt;
      return r->val_bytes();
    } catch (const Error&) {
      // next() returned Some(Err): Reader::get returns the OLD block iterator's val
      // (src/reader.rs:111-122, :376-379), or None
      return held;
    }
  }
  const uint64_t kend = klen;
  static const uint8_t zero = 0;   // the empty key: one readable byte (key may be null)
  DevBuf d_key = klen ? upload(key, klen) : upload(&zero, 1), d_kend = upload(&kend, 1);
  DevBuf d_st(4), d_vo(8), d_vl(8);
  abi_check(mtblx_get(dfile_.as<uint8_t>(), file_.size(), version_, verify_ ? 1 : 0, index_off_, index_len_,
                      d_key.as<uint8_t>(), d_kend.as<uint64_t>(), 1, d_st.as<int32_t>(), d_vo.as<uint64_t>(),
                      d_vl.as<uint64_t>(), nullptr),
            "mtblx_get");
  hip_check(hipDeviceSynchronize(), "sync");
  const int32_t st = download<int32_t>(d_st.p, 1)[0];
  if (st == MTBLX_GET_FOUND) {
    const uint64_t o = download<uint64_t>(d_vo.p, 1)[0], n = download<uint64_t>(d_vl.p, 1)[0];
    return Bytes(file_.begin() + o, file_.begin() + o + n);
  }
  if (st == MTBLX_GET_NONE) return std::nullopt;
  if (st == MTBLX_GET_ERR) throw Error(MtblError::InvalidBlock);
  throw Panic(st == MTBLX_GET_LOOP ? "Reader::get never returns" : "Reader::get panics");
}

inline Reader::Records Reader::scan_one(const ScanQuery& q) const {
  Records out;
  const uint64_t lim = q.max_records ? *q.max_records : ~0ull;
  if (q.kind == ScanQuery::Get) {   // Reader::get: at most one record
    if (lim == 0) return out;
    if (auto v = get(q.key.data(), q.key.size())) out.emplace_back(q.key, *v);
    return out;
  }
  ReaderIntoIter it = q.kind == ScanQuery::From ? iter_from(q.key)
                      : q.kind == ScanQuery::Prefix ? iter_prefix(q.key) : iter_range(q.key, q.key2);
  while (out.size() < lim) {
    auto r = it.next();
    if (!r) break;
    out.emplace_back(r->key_bytes(), r->val_bytes());
  }
  return out;
}

namespace detail {
// the queries as mtblx_scan_plan / mtblx_scan_reduce take them
struct ScanPack {
  Bytes kb, k2b;
  std::vector<uint64_t> ke, k2e, mr;
  std::vector<int32_t> type;
  explicit ScanPack(const std::vector<ScanQuery>& qs) : ke(qs.size()), k2e(qs.size()), mr(qs.size()), type(qs.size()) {
    for (size_t q = 0; q < qs.size(); ++q) {
      type[q] = (int32_t)qs[q].kind;
      kb.insert(kb.end(), qs[q].key.begin(), qs[q].key.end());
      if (qs[q].kind == ScanQuery::Range) k2b.insert(k2b.end(), qs[q].key2.begin(), qs[q].key2.end());
      ke[q] = kb.size();
      k2e[q] = k2b.size();
      mr[q] = qs[q].max_records ? *qs[q].max_records : ~0ull;
    }
  }
};
}  // namespace detail

inline std::vector<Reader::Records> Reader::scan_batch(const std::vector<ScanQuery>& qs, uint32_t max_blocks,
                                                       std::vector<uint8_t>* served) const {
  using namespace detail;
  const uint32_t nq = (uint32_t)qs.size();
  std::vector<Records> out(nq);
  if (served) served->assign(nq, 0);
  if (nq == 0) return out;
  if (meta_.compression_algorithm != 0 || !regular()) {
    for (uint32_t q = 0; q < nq; ++q) out[q] = scan_one(qs[q]);
    return out;
  }
  const ScanPack pack(qs);
  const std::vector<int32_t>& type = pack.type;
  const DevBuf d_k = upload_key(pack.kb), d_ke = upload(pack.ke.data(), nq), d_k2 = upload_key(pack.k2b),
               d_k2e = upload(pack.k2e.data(), nq), d_mr = upload(pack.mr.data(), nq);
  const size_t wsb = mtblx_scan_workspace_bytes(nq);
  const DevBuf ws(wsb), d_res(sizeof(mtblx_scan_result) * (size_t)nq);   // hipMalloc aligns to 256 bytes
  uint64_t totals[4];
  abi_check(mtblx_scan_plan(dfile_.as<uint8_t>(), file_.size(), version_, verify_ ? 1 : 0, index_off_, index_len_,
                            nullptr, nullptr, nullptr, nullptr, 0, nullptr, type.data(), d_k.as<uint8_t>(),
                            d_ke.as<uint64_t>(), d_k2.as<uint8_t>(), d_k2e.as<uint64_t>(), d_mr.as<uint64_t>(),
                            max_blocks, nq, d_res.as<mtblx_scan_result>(), totals, ws.p, wsb, nullptr),
            "mtblx_scan_plan");
  const uint64_t nrec = totals[0], kbytes = totals[1], vbytes = totals[2];
  const DevBuf o_k(kbytes), o_v(vbytes), o_ke(8 * nrec), o_ve(8 * nrec), o_fl(4);
  const mtblx_scanned so{o_k.as<uint8_t>(), kbytes, o_v.as<uint8_t>(), vbytes, o_ke.as<uint64_t>(), o_ve.as<uint64_t>(),
                         nrec, o_fl.as<uint32_t>()};
  abi_check(mtblx_scan_emit(dfile_.as<uint8_t>(), file_.size(), version_, index_off_, index_len_, nullptr, nullptr,
                            nullptr, nullptr, 0, nullptr, nq, &so, ws.p, wsb, nullptr),
            "mtblx_scan_emit");
  hip_check(hipDeviceSynchronize(), "sync");
  if (download<uint32_t>(o_fl.p, 1)[0] != 0) throw std::runtime_error("mtblx_scan_emit: flags set");
  const auto res = download<mtblx_scan_result>(d_res.p, nq);
  const auto hk = download<uint8_t>(o_k.p, kbytes), hv = download<uint8_t>(o_v.p, vbytes);
  const auto hke = download<uint64_t>(o_ke.p, nrec), hve = download<uint64_t>(o_ve.p, nrec);
  for (uint32_t q = 0; q < nq; ++q) {
    const mtblx_scan_result& r = res[q];
    if (r.status != MTBLX_SCAN_OK) {
      out[q] = scan_one(qs[q]);
      continue;
    }
    if (served) (*served)[q] = 1;
    uint64_t pk = r.key_base, pv = r.val_base;
    out[q].reserve(r.nrec);
    for (uint64_t i = r.rec_base; i < r.rec_base + r.nrec; ++i) {
      out[q].emplace_back(Bytes(hk.begin() + pk, hk.begin() + hke[i]), Bytes(hv.begin() + pv, hv.begin() + hve[i]));
      pk = hke[i];
      pv = hve[i];
    }
  }
  return out;
}

// ------------------------------------------------------------------ Merger (src/merger.rs)
// MergerBuilder / Merger (src/merger.rs:66-157) over the device merge (mtblx_merge_plan /
// mtblx_merge_emit, csrc/merge.hip).  The sources' records are read through Reader::into_iter
// (an Err or a panic of a source's scan throws here, where the reference returns Err from
// into_merge_iter / fill), uploaded, merged and grouped on the device, and the items served on
// the host.  Promised on top of the reference (mtblx.h): the values of a key are in the order the
// sources were added; the empty-key quirk of :182-186 is kept; an out-of-order source throws
// UnsortedSource (the reference does not check).  More than MTBLX_MERGE_MAX_SOURCES sources are
// merged in rounds with the same mode; a merge function is called once, at the end, and never
// for a group of one (:200-207).  A MergeReduce (u64 sum / min / max per 8-byte or varint-coded field, mtblx.h
// "Device merge functions") is evaluated on the device (mtblx_merge_emit_reduce), per round: the
// ops are associative and commutative and a group of one passes through, so the rounds give the
// bytes of one application; a group of two or more with a value of another length throws MergeError.
struct MergeConcat {};   // the group's values joined in source order (the reference's test merge function)
struct MergeFirst {};    // the first-added source's value
struct MergeLast {};     // the last-added source's value
using MergeFn = std::function<Bytes(const Bytes& key, const std::vector<Bytes>& values)>;
enum class ReduceEncoding { U64le, Varint };   // 8 little-endian bytes per field | one LEB128 varint per field
struct MergeReduce {     // one op (MTBLX_REDUCE_SUM / _MIN / _MAX) per u64 field, 1 to 8 of them
  std::vector<int> ops;
  // Varint: a value is ops.size() varints back to back, the result re-encoded canonically (mtblx.h
  // "Varint-coded values"); the default is the fixed-width value
  ReduceEncoding encoding = ReduceEncoding::U64le;
  static MergeReduce sum() { return MergeReduce{{MTBLX_REDUCE_SUM}}; }
  static MergeReduce min() { return MergeReduce{{MTBLX_REDUCE_MIN}}; }
  static MergeReduce max() { return MergeReduce{{MTBLX_REDUCE_MAX}}; }
  static MergeReduce varint(std::vector<int> ops) { return MergeReduce{std::move(ops), ReduceEncoding::Varint}; }
};
struct MergeError : std::runtime_error {   // the reference's Error::Merge
  MergeError() : std::runtime_error("merge: a group of two or more holds a value of another length than 8 * nfields") {}
  explicit MergeError(const mtblx_reduce* rd)   // the text names the spec's encoding
      : std::runtime_error(rd && (rd->op[0] & MTBLX_REDUCE_VARINT)
                               ? "merge: a group of two or more holds a value that is not nfields varints back to back"
                               : "merge: a group of two or more holds a value of another length than 8 * nfields") {}
};
struct UnsortedSource : std::runtime_error {
  UnsortedSource() : std::runtime_error("merge source out of order") {}
};

namespace detail {
struct HostGroups {   // mtblx_merged on the host; ge is empty in the single-value modes
  Bytes keys, vals;
  std::vector<uint64_t> ke, ve, ge;
};
// a MergeReduce as the C ABI takes it; refused here, before any device work, if it is not a spec
inline mtblx_reduce reduce_spec(const MergeReduce& r) {
  if (r.ops.empty() || r.ops.size() > MTBLX_REDUCE_MAX_FIELDS) throw std::invalid_argument("MergeReduce: 1 to 8 ops");
  mtblx_reduce spec{};
  spec.nfields = static_cast<uint32_t>(r.ops.size());
  for (size_t f = 0; f < r.ops.size(); ++f) {
    if (r.ops[f] < MTBLX_REDUCE_SUM || r.ops[f] > MTBLX_REDUCE_MAX) throw std::invalid_argument("MergeReduce: unknown op");
    spec.op[f] = static_cast<uint8_t>(r.ops[f] | (r.encoding == ReduceEncoding::Varint ? MTBLX_REDUCE_VARINT : 0u));
  }
  return spec;
}
// the fields of a varint-coded value as varint_decode64 (src/varint.rs:78-97) reads them back to
// back; -> false unless the value is exactly nf of them (mtblx.h "Varint-coded values")
inline bool varint_fields(const Bytes& v, uint32_t nf, uint64_t* out) {
  size_t p = 0;
  for (uint32_t f = 0; f < nf; ++f) {
    uint64_t x = 0;
    bool done = false;
    for (unsigned sh = 0; sh < 70 && p < v.size(); sh += 7) {
      const uint8_t b = v[p++];
      x |= static_cast<uint64_t>(b & 0x7f) << sh;
      if (!(b & 0x80)) {
        done = true;
        break;
      }
    }
    if (!done) return false;
    out[f] = x;
  }
  return p == v.size();
}
// Reduce.fold of the Python surface: the aggregating scans' semantics on the host
inline Reduced fold_host(const mtblx_reduce& spec, const Reader::Records& recs) {
  Reduced r;
  const bool varint = spec.op[0] & MTBLX_REDUCE_VARINT;
  for (uint32_t f = 0; f < spec.nfields; ++f)
    r.fields[f] = (spec.op[f] & ~MTBLX_REDUCE_VARINT) == MTBLX_REDUCE_MIN ? ~0ull : 0ull;
  for (const auto& kv : recs) {
    ++r.nrec;
    uint64_t xs[MTBLX_REDUCE_MAX_FIELDS] = {};
    if (varint ? !varint_fields(kv.second, spec.nfields, xs) : kv.second.size() != 8u * spec.nfields) {
      ++r.nbad;
      continue;
    }
    for (uint32_t f = 0; f < spec.nfields; ++f) {
      uint64_t x = xs[f];
      if (!varint)
        for (int b = 7; b >= 0; --b) x = (x << 8) | kv.second[8 * f + b];
      const unsigned op = spec.op[f] & ~MTBLX_REDUCE_VARINT;
      uint64_t& a = r.fields[f];
      a = op == MTBLX_REDUCE_SUM ? a + x : op == MTBLX_REDUCE_MIN ? (x < a ? x : a) : (x > a ? x : a);
    }
  }
  return r;
}
// one plan + emit over sources [i0, i1) (at most MTBLX_MERGE_MAX_SOURCES); with a reduce spec the
// emit is mtblx_merge_emit_reduce and `mode` is MTBLX_MERGE_FIRST, whose layout it has
inline HostGroups merge_once(const std::vector<HostGroups>& src, size_t i0, size_t i1, int mode,
                             const mtblx_reduce* rd = nullptr) {
  const uint32_t ns = static_cast<uint32_t>(i1 - i0);
  std::vector<DevBuf> bufs;
  std::vector<mtblx_records> recs(ns ? ns : 1);
  uint64_t n = 0;
  for (uint32_t i = 0; i < ns; ++i) {
    const HostGroups& s = src[i0 + i];
    bufs.push_back(upload(s.keys.data(), s.keys.size()));
    bufs.push_back(upload(s.ke.data(), s.ke.size()));
    bufs.push_back(upload(s.vals.data(), s.vals.size()));
    bufs.push_back(upload(s.ve.data(), s.ve.size()));
    const size_t b = bufs.size() - 4;
    recs[i] = mtblx_records{bufs[b].as<uint8_t>(), bufs[b + 1].as<uint64_t>(), bufs[b + 2].as<uint8_t>(),
                            bufs[b + 3].as<uint64_t>(), s.ke.size()};
    n += s.ke.size();
  }
  const size_t wsb = mtblx_merge_workspace_bytes(n, ns);
  if (!wsb) throw std::length_error("merge: 2^32 - 16 records or more");
  DevBuf ws(wsb);
  uint64_t tot[6] = {};
  const int rc = mtblx_merge_plan(recs.data(), ns, tot, ws.p, wsb, nullptr);
  if (rc == MTBLX_E_FORMAT) throw UnsortedSource();
  abi_check(rc, "mtblx_merge_plan");
  const bool grouped = mode == MTBLX_MERGE_GROUPS;
  const uint64_t nve = grouped ? tot[2] : tot[0], nge = grouped ? tot[0] : 0;
  DevBuf k(tot[1]), ke(8 * tot[0]), v(tot[3]), ve(8 * nve), ge(8 * nge), fl(4);
  const mtblx_merged out{k.as<uint8_t>(),  tot[1],  ke.as<uint64_t>(), 8 * tot[0], v.as<uint8_t>(), tot[3],
                         ve.as<uint64_t>(), 8 * nve, ge.as<uint64_t>(), 8 * nge,    fl.as<uint32_t>()};
  if (rd) abi_check(mtblx_merge_emit_reduce(recs.data(), ns, rd, &out, ws.p, wsb, nullptr), "mtblx_merge_emit_reduce");
  else abi_check(mtblx_merge_emit(recs.data(), ns, mode, &out, ws.p, wsb, nullptr), "mtblx_merge_emit");
  hip_check(hipDeviceSynchronize(), "sync");
  const uint32_t flags = download<uint32_t>(fl.p, 1)[0];
  if (flags & MTBLX_MERGE_BADVALUE) throw MergeError(rd);
  if (flags) throw std::runtime_error("mtblx_merge_emit: flags set");
  HostGroups r;
  r.ke = download<uint64_t>(ke.p, tot[0]);
  r.ve = download<uint64_t>(ve.p, nve);
  r.ge = download<uint64_t>(ge.p, nge);
  r.keys = download<uint8_t>(k.p, tot[1]);
  r.vals = download<uint8_t>(v.p, r.ve.empty() ? 0 : r.ve.back());
  return r;
}
// grouped results of consecutive source chunks -> the grouped result of all their sources: the
// groups' value bytes joined per key (CONCAT), and the groups' value lengths joined the same way.
// regroup_split makes the two CONCAT inputs of parts [i0, i1), regroup_join the result of the two merges
inline void regroup_split(const std::vector<HostGroups>& parts, size_t i0, size_t i1, std::vector<HostGroups>& a,
                          std::vector<HostGroups>& b) {
  a.assign(i1 - i0, HostGroups());
  b.assign(i1 - i0, HostGroups());
  for (size_t i = i0; i < i1; ++i) {
    const HostGroups& p = parts[i];
    HostGroups &x = a[i - i0], &y = b[i - i0];
    x.keys = y.keys = p.keys;
    x.ke = y.ke = p.ke;
    x.vals = p.vals;
    for (uint64_t g : p.ge) {
      x.ve.push_back(p.ve[g - 1]);
      y.ve.push_back(8 * g);
    }
    y.vals.resize(8 * p.ve.size());
    for (size_t j = 0; j < p.ve.size(); ++j) {
      const uint64_t len = p.ve[j] - (j ? p.ve[j - 1] : 0);
      std::memcpy(y.vals.data() + 8 * j, &len, 8);
    }
  }
}
inline HostGroups regroup_join(HostGroups va, const HostGroups& vb) {
  HostGroups r;
  r.keys = std::move(va.keys);
  r.ke = std::move(va.ke);
  r.vals = std::move(va.vals);
  uint64_t end = 0;
  for (size_t j = 0; j < vb.vals.size() / 8; ++j) {
    uint64_t len;
    std::memcpy(&len, vb.vals.data() + 8 * j, 8);
    r.ve.push_back(end += len);
  }
  for (uint64_t e : vb.ve) r.ge.push_back(e / 8);
  return r;
}
inline HostGroups regroup(const std::vector<HostGroups>& parts, size_t i0, size_t i1) {
  std::vector<HostGroups> a, b;
  regroup_split(parts, i0, i1, a, b);
  HostGroups va = merge_once(a, 0, a.size(), MTBLX_MERGE_CONCAT);
  return regroup_join(std::move(va), merge_once(b, 0, b.size(), MTBLX_MERGE_CONCAT));
}
inline HostGroups merge_all(std::vector<HostGroups> src, int mode, const mtblx_reduce* rd = nullptr) {
  bool first = true;
  while (first || src.size() > 1) {
    std::vector<HostGroups> next;
    for (size_t i = 0; i < src.size() || (first && src.empty() && next.empty()); i += MTBLX_MERGE_MAX_SOURCES) {
      const size_t e = std::min(src.size(), i + MTBLX_MERGE_MAX_SOURCES);
      next.push_back(mode == MTBLX_MERGE_GROUPS && !first ? regroup(src, i, e) : merge_once(src, i, e, mode, rd));
    }
    src = std::move(next);
    first = false;
  }
  return std::move(src[0]);
}
inline Bytes slice(const Bytes& b, const std::vector<uint64_t>& end, size_t i) {
  return Bytes(b.begin() + (i ? end[i - 1] : 0), b.begin() + end[i]);
}

// ---- the segmented merge (mtblx_merge_seg_plan / _emit, csrc/merge_seg.hip): every source is nseg
// sorted runs back to back, cut by off[i] (nseg + 1 offsets); segment q of the result is the merge
// of segment q of every source, its groups [seg_end[q-1], seg_end[q])
struct SegGroups {
  HostGroups g;
  std::vector<uint64_t> seg_end;
};
using SegOffsets = std::vector<std::vector<uint64_t>>;
// one plan + emit over sources [i0, i1) (at most MTBLX_MERGE_MAX_SOURCES), as merge_once
inline SegGroups merge_seg_once(const std::vector<HostGroups>& src, const SegOffsets& off, size_t i0, size_t i1,
                                uint32_t nseg, int mode, const mtblx_reduce* rd = nullptr) {
  const uint32_t ns = static_cast<uint32_t>(i1 - i0);
  std::vector<DevBuf> bufs;
  std::vector<mtblx_records> recs(ns ? ns : 1);
  std::vector<const uint64_t*> offp(ns ? ns : 1, nullptr);
  uint64_t n = 0;
  for (uint32_t i = 0; i < ns; ++i) {
    const HostGroups& s = src[i0 + i];
    if (off[i0 + i].size() != (size_t)nseg + 1) throw std::invalid_argument("merge: nseg + 1 offsets per source");
    bufs.push_back(upload(s.keys.data(), s.keys.size()));
    bufs.push_back(upload(s.ke.data(), s.ke.size()));
    bufs.push_back(upload(s.vals.data(), s.vals.size()));
    bufs.push_back(upload(s.ve.data(), s.ve.size()));
    bufs.push_back(upload(off[i0 + i].data(), off[i0 + i].size()));
    const size_t b = bufs.size() - 5;
    recs[i] = mtblx_records{bufs[b].as<uint8_t>(), bufs[b + 1].as<uint64_t>(), bufs[b + 2].as<uint8_t>(),
                            bufs[b + 3].as<uint64_t>(), s.ke.size()};
    offp[i] = bufs[b + 4].as<uint64_t>();
    n += s.ke.size();
  }
  const size_t wsb = mtblx_merge_seg_workspace_bytes(n, ns, nseg);
  if (!wsb) throw std::length_error("merge: 2^32 - 16 records or more, or more than 2^24 queries");
  DevBuf ws(wsb), se(8 * (size_t)nseg);
  uint64_t tot[6] = {};
  const int rc = mtblx_merge_seg_plan(recs.data(), offp.data(), ns, nseg, tot, se.as<uint64_t>(), ws.p, wsb, nullptr);
  if (rc == MTBLX_E_FORMAT && !(tot[5] & MTBLX_MERGE_BADSEG)) throw UnsortedSource();
  abi_check(rc, "mtblx_merge_seg_plan");
  const bool grouped = mode == MTBLX_MERGE_GROUPS;
  const uint64_t nve = grouped ? tot[2] : tot[0], nge = grouped ? tot[0] : 0;
  DevBuf k(tot[1]), ke(8 * tot[0]), v(tot[3]), ve(8 * nve), ge(8 * nge), fl(4);
  const mtblx_merged out{k.as<uint8_t>(),  tot[1],  ke.as<uint64_t>(), 8 * tot[0], v.as<uint8_t>(), tot[3],
                         ve.as<uint64_t>(), 8 * nve, ge.as<uint64_t>(), 8 * nge,    fl.as<uint32_t>()};
  if (rd)
    abi_check(mtblx_merge_seg_emit_reduce(recs.data(), offp.data(), ns, nseg, rd, &out, ws.p, wsb, nullptr),
              "mtblx_merge_seg_emit_reduce");
  else
    abi_check(mtblx_merge_seg_emit(recs.data(), offp.data(), ns, nseg, mode, &out, ws.p, wsb, nullptr),
              "mtblx_merge_seg_emit");
  hip_check(hipDeviceSynchronize(), "sync");
  const uint32_t flags = download<uint32_t>(fl.p, 1)[0];
  if (flags & MTBLX_MERGE_BADVALUE) throw MergeError(rd);
  if (flags) throw std::runtime_error("mtblx_merge_seg_emit: flags set");
  SegGroups r;
  r.seg_end = download<uint64_t>(se.p, nseg);
  r.g.ke = download<uint64_t>(ke.p, tot[0]);
  r.g.ve = download<uint64_t>(ve.p, nve);
  r.g.ge = download<uint64_t>(ge.p, nge);
  r.g.keys = download<uint8_t>(k.p, tot[1]);
  r.g.vals = download<uint8_t>(v.p, r.g.ve.empty() ? 0 : r.g.ve.back());
  return r;
}
// any number of sources: rounds of MTBLX_MERGE_MAX_SOURCES with the same mode, a round's output cut
// by {0, seg_end...} being a source of the next; GROUPS through the two CONCATs of regroup
inline SegGroups merge_seg_all(std::vector<HostGroups> src, SegOffsets off, uint32_t nseg, int mode,
                               const mtblx_reduce* rd = nullptr) {
  bool first = true;
  while (first || src.size() > 1) {
    std::vector<HostGroups> next;
    SegOffsets noff;
    for (size_t i = 0; i < src.size() || (first && src.empty() && next.empty()); i += MTBLX_MERGE_MAX_SOURCES) {
      const size_t e = std::min(src.size(), i + MTBLX_MERGE_MAX_SOURCES);
      SegGroups r;
      if (mode == MTBLX_MERGE_GROUPS && !first) {
        std::vector<HostGroups> a, b;
        regroup_split(src, i, e, a, b);
        const SegOffsets o(off.begin() + i, off.begin() + e);
        SegGroups va = merge_seg_once(a, o, 0, a.size(), nseg, MTBLX_MERGE_CONCAT);
        r.g = regroup_join(std::move(va.g), merge_seg_once(b, o, 0, b.size(), nseg, MTBLX_MERGE_CONCAT).g);
        r.seg_end = std::move(va.seg_end);
      } else {
        r = merge_seg_once(src, off, i, e, nseg, mode, rd);
      }
      std::vector<uint64_t> o(1, 0);
      o.insert(o.end(), r.seg_end.begin(), r.seg_end.end());
      next.push_back(std::move(r.g));
      noff.push_back(std::move(o));
    }
    src = std::move(next);
    off = std::move(noff);
    first = false;
  }
  SegGroups r;
  r.g = std::move(src[0]);
  r.seg_end.assign(off[0].begin() + 1, off[0].end());
  return r;
}
}  // namespace detail

inline std::vector<Reduced> Reader::reduce_batch(const std::vector<ScanQuery>& qs, const MergeReduce& reduce,
                                                 uint32_t max_blocks, std::vector<uint8_t>* served) const {
  using namespace detail;
  const mtblx_reduce spec = reduce_spec(reduce);   // refused before any device work
  const uint32_t nq = (uint32_t)qs.size(), nf = spec.nfields;
  std::vector<Reduced> out(nq);
  if (served) served->assign(nq, 0);
  if (nq == 0) return out;
  if (meta_.compression_algorithm != 0 || !regular()) {
    for (uint32_t q = 0; q < nq; ++q) out[q] = fold_host(spec, scan_one(qs[q]));
    return out;
  }
  const ScanPack pk(qs);
  const DevBuf d_k = upload_key(pk.kb), d_ke = upload(pk.ke.data(), nq), d_k2 = upload_key(pk.k2b),
               d_k2e = upload(pk.k2e.data(), nq), d_mr = upload(pk.mr.data(), nq);
  const size_t wsb = mtblx_scan_workspace_bytes(nq);
  const DevBuf ws(wsb), d_res(sizeof(mtblx_scan_result) * (size_t)nq), d_f(8 * (size_t)nq * nf), d_nb(8 * (size_t)nq);
  uint64_t totals[4];
  abi_check(mtblx_scan_reduce(dfile_.as<uint8_t>(), file_.size(), version_, verify_ ? 1 : 0, index_off_, index_len_,
                              nullptr, nullptr, nullptr, nullptr, 0, nullptr, pk.type.data(), d_k.as<uint8_t>(),
                              d_ke.as<uint64_t>(), d_k2.as<uint8_t>(), d_k2e.as<uint64_t>(), d_mr.as<uint64_t>(),
                              max_blocks, nq, d_res.as<mtblx_scan_result>(), totals, ws.p, wsb, &spec,
                              d_f.as<uint64_t>(), d_nb.as<uint64_t>(), nullptr),
            "mtblx_scan_reduce");
  const auto res = download<mtblx_scan_result>(d_res.p, nq);   // the call has synchronised
  const auto hf = download<uint64_t>(d_f.p, (size_t)nq * nf), hb = download<uint64_t>(d_nb.p, nq);
  for (uint32_t q = 0; q < nq; ++q) {
    if (res[q].status != MTBLX_SCAN_OK) {
      out[q] = fold_host(spec, scan_one(qs[q]));
      continue;
    }
    if (served) (*served)[q] = 1;
    for (uint32_t f = 0; f < nf; ++f) out[q].fields[f] = hf[(size_t)q * nf + f];
    out[q].nrec = res[q].nrec;
    out[q].nbad = hb[q];
  }
  return out;
}

class Merger;
class MergerBuilder {   // src/merger.rs:66-94
 public:
  explicit MergerBuilder(MergeFn f) : mode_(MTBLX_MERGE_GROUPS), fn_(std::move(f)) {}
  explicit MergerBuilder(MergeConcat) : mode_(MTBLX_MERGE_CONCAT) {}
  explicit MergerBuilder(MergeFirst) : mode_(MTBLX_MERGE_FIRST) {}
  explicit MergerBuilder(MergeLast) : mode_(MTBLX_MERGE_LAST) {}
  explicit MergerBuilder(const MergeReduce& r) : mode_(MTBLX_MERGE_FIRST), rd_(detail::reduce_spec(r)), reduce_(true) {}
  MergerBuilder& add(Reader source) { push(std::move(source)); return *this; }
  void push(Reader source) { sources_.push_back(std::move(source)); }
  MergerBuilder& extend(std::vector<Reader> sources) {
    for (Reader& r : sources) sources_.push_back(std::move(r));
    return *this;
  }
  Merger build();

 private:
  int mode_;
  MergeFn fn_;
  mtblx_reduce rd_{};   // used when reduce_: mode_ is then MTBLX_MERGE_FIRST, the layout of the result
  bool reduce_ = false;
  std::vector<Reader> sources_;
};

class Merger {
 public:
  template <class F>
  static MergerBuilder builder(F merge) { return MergerBuilder(std::move(merge)); }
  // MultiIter (:216-260) drained: (key, values) per distinct key, the values in source order
  std::vector<std::pair<Bytes, std::vector<Bytes>>> into_iter() const {
    const detail::HostGroups g = run(MTBLX_MERGE_GROUPS);
    std::vector<std::pair<Bytes, std::vector<Bytes>>> out;
    for (size_t i = 0; i < g.ke.size(); ++i) {
      std::vector<Bytes> vs;
      for (uint64_t j = i ? g.ge[i - 1] : 0; j < g.ge[i]; ++j) vs.push_back(detail::slice(g.vals, g.ve, j));
      out.emplace_back(detail::slice(g.keys, g.ke, i), std::move(vs));
    }
    return out;
  }
  // MergerIter (:159-214) drained: (key, merged value) per distinct key
  std::vector<std::pair<Bytes, Bytes>> into_merge_iter() const {
    std::vector<std::pair<Bytes, Bytes>> out;
    if (mode_ == MTBLX_MERGE_GROUPS) {
      for (auto& kv : into_iter())
        out.emplace_back(std::move(kv.first), kv.second.size() == 1 ? std::move(kv.second[0]) : fn_(kv.first, kv.second));
      return out;
    }
    const detail::HostGroups g = run(mode_);
    for (size_t i = 0; i < g.ke.size(); ++i)
      out.emplace_back(detail::slice(g.keys, g.ke, i), detail::slice(g.vals, g.ve, i));
    return out;
  }
  // src/merger.rs:149-156
  void write_into(Writer& w) const {
    for (const auto& kv : into_merge_iter()) w.insert(kv.first, kv.second);
  }
  // MergerIter over iter_from / get / iter_prefix / iter_range of every source, for a batch of
  // queries: out[q] is what into_merge_iter would yield if each source were opened with query q,
  // the empty-key quirk applied inside the query (mtblx.h "Segmented merge").  Every source answers
  // the batch with Reader::scan_batch; the queries the kernels served in every source are merged
  // by ONE segmented merge (mtblx_merge_seg_plan / _emit; rounds of 64 sources), the others
  // (max_blocks, a compressed source, an irregular index) by the Merger's merge over the per-source
  // answers.  A query's max_records = m keeps the first m items of its unlimited result: every
  // source is asked for m + 1 records (a source's record at position p >= m + 1 has at least
  // p - 1 >= m distinct kept keys before it; the - 1 is the empty key the quirk may drop).  With a
  // MergeReduce, MergeError is thrown iff a bad group lies among the at most S * (m + 1) records
  // fetched for a query.  served (may be null): per query, 1 where the segmented merge answered it.
  std::vector<std::vector<std::pair<Bytes, Bytes>>> scan_batch(const std::vector<ScanQuery>& queries,
                                                                uint32_t max_blocks = 64,
                                                                std::vector<uint8_t>* served = nullptr) const {
    const uint32_t nq = static_cast<uint32_t>(queries.size());
    const size_t ns = sources_.size();
    std::vector<ScanQuery> ask = queries;
    for (ScanQuery& q : ask)
      if (q.max_records && *q.max_records != ~0ull) q.max_records = *q.max_records + 1;
    std::vector<std::vector<Reader::Records>> ans(ns);
    std::vector<uint8_t> kernel(nq, 1);
    for (size_t s = 0; s < ns; ++s) {
      std::vector<uint8_t> sv;
      ans[s] = sources_[s].scan_batch(ask, max_blocks, &sv);
      for (uint32_t q = 0; q < nq; ++q) kernel[q] &= sv[q];
    }
    const mtblx_reduce* rd = reduce_ ? &rd_ : nullptr;
    std::vector<detail::HostGroups> src(ns);
    detail::SegOffsets off(ns);
    for (size_t s = 0; s < ns; ++s) {
      off[s].push_back(0);
      for (uint32_t q = 0; q < nq; ++q) {
        if (kernel[q]) append(src[s], ans[s][q]);
        off[s].push_back(src[s].ke.size());
      }
    }
    const detail::SegGroups m = detail::merge_seg_all(std::move(src), std::move(off), nq, mode_, rd);
    std::vector<std::vector<std::pair<Bytes, Bytes>>> out(nq);
    for (uint32_t q = 0; q < nq; ++q) {
      const uint64_t lim = queries[q].max_records ? *queries[q].max_records : ~0ull;
      if (kernel[q]) {
        const uint64_t g0 = q ? m.seg_end[q - 1] : 0;
        out[q] = items(m.g, g0, g0 + std::min<uint64_t>(lim, m.seg_end[q] - g0));   // the cut is a view
        continue;
      }
      std::vector<detail::HostGroups> one(ns);
      for (size_t s = 0; s < ns; ++s) append(one[s], ans[s][q]);
      const detail::HostGroups g = detail::merge_all(std::move(one), mode_, rd);
      out[q] = items(g, 0, std::min<uint64_t>(lim, g.ke.size()));
    }
    if (served) *served = std::move(kernel);
    return out;
  }

 private:
  friend class MergerBuilder;
  static void append(detail::HostGroups& s, const Reader::Records& recs) {
    for (const auto& kv : recs) {
      s.keys.insert(s.keys.end(), kv.first.begin(), kv.first.end());
      s.vals.insert(s.vals.end(), kv.second.begin(), kv.second.end());
      s.ke.push_back(s.keys.size());
      s.ve.push_back(s.vals.size());
    }
  }
  // MergerIter's items [g0, g1) of a result in this Merger's mode: the merge function runs on the
  // host for the groups of two or more, as in into_merge_iter
  std::vector<std::pair<Bytes, Bytes>> items(const detail::HostGroups& g, uint64_t g0, uint64_t g1) const {
    std::vector<std::pair<Bytes, Bytes>> out;
    for (uint64_t i = g0; i < g1; ++i) {
      if (mode_ != MTBLX_MERGE_GROUPS) {
        out.emplace_back(detail::slice(g.keys, g.ke, i), detail::slice(g.vals, g.ve, i));
        continue;
      }
      std::vector<Bytes> vs;
      for (uint64_t j = i ? g.ge[i - 1] : 0; j < g.ge[i]; ++j) vs.push_back(detail::slice(g.vals, g.ve, j));
      Bytes k = detail::slice(g.keys, g.ke, i);
      Bytes v = vs.size() == 1 ? std::move(vs[0]) : fn_(k, vs);
      out.emplace_back(std::move(k), std::move(v));
    }
    return out;
  }
  Merger(int mode, MergeFn fn, std::vector<Reader> s, const mtblx_reduce& rd, bool reduce)
      : mode_(mode), fn_(std::move(fn)), rd_(rd), reduce_(reduce), sources_(std::move(s)) {}
  detail::HostGroups run(int mode) const {
    std::vector<detail::HostGroups> src(sources_.size());
    for (size_t i = 0; i < sources_.size(); ++i) {
      ReaderIntoIter it = sources_[i].into_iter();
      detail::HostGroups& s = src[i];
      while (auto r = it.next()) {
        s.keys.insert(s.keys.end(), r->key, r->key + r->key_len);
        s.vals.insert(s.vals.end(), r->val, r->val + r->val_len);
        s.ke.push_back(s.keys.size());
        s.ve.push_back(s.vals.size());
      }
    }
    return detail::merge_all(std::move(src), mode, reduce_ && mode != MTBLX_MERGE_GROUPS ? &rd_ : nullptr);
  }
  int mode_;
  MergeFn fn_;
  mtblx_reduce rd_;
  bool reduce_;
  std::vector<Reader> sources_;
};
inline Merger MergerBuilder::build() { return Merger(mode_, std::move(fn_), std::move(sources_), rd_, reduce_); }

// ------------------------------------------------------------------ Sorter (src/sorter.rs)
// SorterBuilder / Sorter (src/sorter.rs:25-258) over the device sort (mtblx_sort_plan /
// mtblx_sort_emit, csrc/sort.hip) and detail::merge_all.  insert keeps the reference's memory rule
// (:128-137); write_chunk (:142-197) is one device sort of the pending records; merge_chunks
// (:199-233) and the final merge of into_iter (:244-257) are the device Merger over the chunks,
// oldest first, with its empty-key quirk -- exactly where the reference has it.  Chunks are kept in
// host memory between the device calls, not in compressed temp files: chunk_compression_type /
// _level are accepted and stored and have no effect.  Promised on top of the reference (mtblx.h):
// the values of a key are in insertion order (the reference sorts with sort_unstable_by).  A merge
// function is never called for a group of one (:166-170).  A MergeReduce is evaluated on the device
// per chunk (mtblx_sort_emit_reduce) and again over the chunks (mtblx_merge_emit_reduce), as the
// reference applies its merge function; the bytes are those of one application (mtblx.h).
constexpr size_t DEFAULT_NB_CHUNKS = 25, MIN_NB_CHUNKS = 1;                              // src/lib.rs:11-12
constexpr size_t DEFAULT_SORTER_MEMORY = 1073741824, MIN_SORTER_MEMORY = 10485760;       // :13-14
constexpr size_t INITIAL_SORTER_VEC_SIZE = 131072;                                       // :15

namespace detail {
// one mtblx_sort_plan + mtblx_sort_emit (with a reduce spec: mtblx_sort_emit_reduce, mode
// MTBLX_MERGE_FIRST) over one batch of records in any order
inline HostGroups sort_once(const HostGroups& s, int mode, const mtblx_reduce* rd = nullptr) {
  const DevBuf dk = upload(s.keys.data(), s.keys.size()), dke = upload(s.ke.data(), s.ke.size()),
               dv = upload(s.vals.data(), s.vals.size()), dve = upload(s.ve.data(), s.ve.size());
  const mtblx_records rec{dk.as<uint8_t>(), dke.as<uint64_t>(), dv.as<uint8_t>(), dve.as<uint64_t>(), s.ke.size()};
  const size_t wsb = mtblx_sort_workspace_bytes(rec.n);
  if (!wsb) throw std::length_error("sort: 2^32 - 16 records or more");
  DevBuf ws(wsb);
  uint64_t tot[6] = {};
  abi_check(mtblx_sort_plan(&rec, tot, ws.p, wsb, nullptr), "mtblx_sort_plan");
  const bool grouped = mode == MTBLX_MERGE_GROUPS;
  const uint64_t nve = grouped ? tot[2] : tot[0], nge = grouped ? tot[0] : 0;
  DevBuf k(tot[1]), ke(8 * tot[0]), v(tot[3]), ve(8 * nve), ge(8 * nge), fl(4);
  const mtblx_merged out{k.as<uint8_t>(),  tot[1],  ke.as<uint64_t>(), 8 * tot[0], v.as<uint8_t>(), tot[3],
                         ve.as<uint64_t>(), 8 * nve, ge.as<uint64_t>(), 8 * nge,    fl.as<uint32_t>()};
  if (rd) abi_check(mtblx_sort_emit_reduce(&rec, rd, &out, ws.p, wsb, nullptr), "mtblx_sort_emit_reduce");
  else abi_check(mtblx_sort_emit(&rec, mode, &out, ws.p, wsb, nullptr), "mtblx_sort_emit");
  hip_check(hipDeviceSynchronize(), "sync");
  const uint32_t flags = download<uint32_t>(fl.p, 1)[0];
  if (flags & MTBLX_MERGE_BADVALUE) throw MergeError(rd);
  if (flags) throw std::runtime_error("mtblx_sort_emit: flags set");
  HostGroups r;
  r.ke = download<uint64_t>(ke.p, tot[0]);
  r.ve = download<uint64_t>(ve.p, nve);
  r.ge = download<uint64_t>(ge.p, nge);
  r.keys = download<uint8_t>(k.p, tot[1]);
  r.vals = download<uint8_t>(v.p, r.ve.empty() ? 0 : r.ve.back());
  return r;
}
// grouped items -> one record per key: a group of one passes through, fn merges the others
inline HostGroups apply_fn(const HostGroups& g, const MergeFn& fn) {
  HostGroups r;
  for (size_t i = 0; i < g.ke.size(); ++i) {
    const Bytes key = slice(g.keys, g.ke, i);
    std::vector<Bytes> vs;
    for (uint64_t j = i ? g.ge[i - 1] : 0; j < g.ge[i]; ++j) vs.push_back(slice(g.vals, g.ve, j));
    const Bytes v = vs.size() == 1 ? std::move(vs[0]) : fn(key, vs);
    r.keys.insert(r.keys.end(), key.begin(), key.end());
    r.vals.insert(r.vals.end(), v.begin(), v.end());
    r.ke.push_back(r.keys.size());
    r.ve.push_back(r.vals.size());
  }
  return r;
}
}  // namespace detail

class Sorter;
class SorterBuilder {   // src/sorter.rs:17-70
 public:
  explicit SorterBuilder(MergeFn f) : mode_(MTBLX_MERGE_GROUPS), fn_(std::move(f)) {}
  explicit SorterBuilder(MergeConcat) : mode_(MTBLX_MERGE_CONCAT) {}
  explicit SorterBuilder(MergeFirst) : mode_(MTBLX_MERGE_FIRST) {}
  explicit SorterBuilder(MergeLast) : mode_(MTBLX_MERGE_LAST) {}
  explicit SorterBuilder(const MergeReduce& r) : mode_(MTBLX_MERGE_FIRST), rd_(detail::reduce_spec(r)), reduce_(true) {}
  SorterBuilder& max_memory(size_t memory) { max_memory_ = std::max(memory, MIN_SORTER_MEMORY); return *this; }         // :37
  SorterBuilder& max_nb_chunks(size_t nb_chunks) { max_nb_chunks_ = std::max(nb_chunks, MIN_NB_CHUNKS); return *this; }  // :44
  SorterBuilder& chunk_compression_type(CompressionType c) { ctype_ = c; return *this; }   // stored, no effect
  SorterBuilder& chunk_compression_level(uint32_t l) { clevel_ = l; return *this; }        // stored, no effect
  Sorter build();

 private:
  int mode_;
  MergeFn fn_;
  mtblx_reduce rd_{};   // used when reduce_: mode_ is then MTBLX_MERGE_FIRST, the layout of the result
  bool reduce_ = false;
  size_t max_memory_ = DEFAULT_SORTER_MEMORY, max_nb_chunks_ = DEFAULT_NB_CHUNKS;   // :28-29
  CompressionType ctype_ = CompressionType::Snappy;                                  // :30
  uint32_t clevel_ = 0;                                                              // :31
};

class Sorter {
 public:
  template <class F>
  static SorterBuilder builder(F merge) { return SorterBuilder(std::move(merge)); }   // :108-110
  template <class F>
  explicit Sorter(F merge);                                                            // :112-114
  // :120-140
  void insert(const uint8_t* key, size_t klen, const uint8_t* val, size_t vlen) {
    entry_bytes_ += klen + vlen;                                       // :128
    // entries.push (:129) and entries.capacity() (:131): the Vec starts at INITIAL_SORTER_VEC_SIZE,
    // doubles when a push finds it full and keeps its capacity through drain(..).  The doubling is
    // std's current amortised growth, an implementation detail, emulated because the rule reads it
    if (len_ == capacity_) capacity_ *= 2;
    ++len_;
    pending_.keys.insert(pending_.keys.end(), key, key + klen);
    pending_.vals.insert(pending_.vals.end(), val, val + vlen);
    pending_.ke.push_back(pending_.keys.size());
    pending_.ve.push_back(pending_.vals.size());
    if (entry_bytes_ + capacity_ * 32 >= max_memory_) {                // :131-132, 32 = size_of::<Entry>()
      write_chunk();
      if (chunks_.size() > max_nb_chunks_) merge_chunks();             // :134-136
    }
  }
  void insert(const Bytes& k, const Bytes& v) { insert(k.data(), k.size(), v.data(), v.size()); }
  void insert(const std::string& k, const std::string& v) {
    insert(reinterpret_cast<const uint8_t*>(k.data()), k.size(), reinterpret_cast<const uint8_t*>(v.data()), v.size());
  }
  // :244-257, drained: (key, merged value) per distinct key.  Consumes the pending records.
  std::vector<std::pair<Bytes, Bytes>> into_iter() {
    write_chunk();                                                     // :246, also when nothing is pending
    const detail::HostGroups g = merged();                             // :253-256; no merge_chunks here
    std::vector<std::pair<Bytes, Bytes>> out;
    for (size_t i = 0; i < g.ke.size(); ++i)
      out.emplace_back(detail::slice(g.keys, g.ke, i), detail::slice(g.vals, g.ve, i));
    return out;
  }
  // :235-242
  void write_into(Writer& w) {
    for (const auto& kv : into_iter()) w.insert(kv.first, kv.second);
  }
  const std::vector<size_t>& chunk_sizes() const { return chunk_sizes_; }   // records per write_chunk, in order
  size_t merges() const { return merges_; }                                // runs of merge_chunks

 private:
  friend class SorterBuilder;
  Sorter(int mode, MergeFn fn, const mtblx_reduce& rd, bool reduce, size_t max_memory, size_t max_nb_chunks)
      : mode_(mode), fn_(std::move(fn)), rd_(rd), reduce_(reduce), max_memory_(max_memory), max_nb_chunks_(max_nb_chunks) {}
  const mtblx_reduce* rd() const { return reduce_ ? &rd_ : nullptr; }
  void write_chunk() {                                                 // :142-197
    chunk_sizes_.push_back(pending_.ke.size());
    chunks_.push_back(mode_ == MTBLX_MERGE_GROUPS ? detail::apply_fn(detail::sort_once(pending_, mode_), fn_)
                                                  : detail::sort_once(pending_, mode_, rd()));
    pending_ = detail::HostGroups();
    entry_bytes_ = 0;                                                  // :192
    len_ = 0;                                                          // :155 drain(..): the capacity stays
  }
  detail::HostGroups merged() const {   // a Merger over the chunks, oldest first
    return mode_ == MTBLX_MERGE_GROUPS ? detail::apply_fn(detail::merge_all(chunks_, mode_), fn_)
                                       : detail::merge_all(chunks_, mode_, rd());
  }
  void merge_chunks() {                                                // :199-233: the result is the only, hence oldest, chunk
    detail::HostGroups m = merged();
    chunks_.clear();
    chunks_.push_back(std::move(m));
    ++merges_;
  }
  int mode_;
  MergeFn fn_;
  mtblx_reduce rd_;
  bool reduce_;
  size_t max_memory_, max_nb_chunks_;
  std::vector<detail::HostGroups> chunks_;
  detail::HostGroups pending_;
  size_t entry_bytes_ = 0, len_ = 0, capacity_ = INITIAL_SORTER_VEC_SIZE, merges_ = 0;
  std::vector<size_t> chunk_sizes_;
};
inline Sorter SorterBuilder::build() { return Sorter(mode_, std::move(fn_), rd_, reduce_, max_memory_, max_nb_chunks_); }
template <class F>
inline Sorter::Sorter(F merge) : Sorter(SorterBuilder(std::move(merge)).build()) {}

}  // namespace mtbl

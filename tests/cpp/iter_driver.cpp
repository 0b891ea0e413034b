// iter_driver — runs scripts against the C++ surface (include/mtbl.hpp) and writes what happened,
// so tests/test_cpp_iter.py can compare mtbl::Reader / ReaderIntoIter with the oracle script for
// script.  Only the public API is used.  One process opens one file and runs many scripts.
//
//   iter_driver FILE SCRIPT OUT
//
// SCRIPT and OUT are little-endian binary; `bytes` is a u32 length and that many bytes.
//   command                                              result (starts with the command's tag)
//   'O' u8 verify                                        u8 outcome, bytes error
//   'I' u8 mode, bytes key, bytes key2, u32 nops, ops    u8 end, bytes error, u32 nops, {u64 yielded, u8 code},
//       op: u8 0, u64 n (up to n next())                 u64 nrec, {bytes key, bytes value}
//           u8 1, bytes key (seek)
//   'S' u8 mode, bytes key, bytes key2, u64 max_records  u8 end, bytes error, u64 nrec, {bytes key, bytes value}
//   'G' bytes key                                        u8 outcome, bytes error, bytes value
//   'L'                                                  u8 outcome, bytes error, u64 len
//   'B' u32 max_blocks, u32 nq,                          u8 outcome, bytes error, u32 nq,
//       {u8 kind, bytes key, bytes key2, u8 has, u64 max}  {u64 nrec, {bytes key, bytes value}}, nq served bytes
// mode: 0 into_iter, 1 iter_from, 2 iter_prefix, 3 iter_range; kind: ScanQuery::Kind.
// end: 0 clean, 1 Error at open or construction, 2 Error in next(), 3 Panic.  op code: 0 ok, 1 nullopt,
// 2 Error (the script goes on with its next op).  outcome: 0 ok / a value, 1 none, 2 Error, 3 Panic.
// error: error_name(kind) of the Error that set `end` / `outcome`, else of the last Error an op met.
// After a failed 'O' every command reports that failure as its own end / outcome.
// Any other exception (std::runtime_error of the header, HIP errors) is a failure of the driver:
// it is printed to stderr and the exit status is 1.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "mtbl.hpp"

using mtbl::Bytes;

namespace {
struct In {
  Bytes d;
  size_t p = 0;
  void need(size_t n) const {
    if (d.size() - p < n) throw std::runtime_error("script truncated");
  }
  bool done() const { return p == d.size(); }
  uint8_t u8() { need(1); return d[p++]; }
  uint32_t u32() { need(4); uint32_t v; std::memcpy(&v, d.data() + p, 4); p += 4; return v; }
  uint64_t u64() { need(8); uint64_t v; std::memcpy(&v, d.data() + p, 8); p += 8; return v; }
  Bytes bytes() {
    const uint32_t n = u32();
    need(n);
    Bytes b(d.begin() + p, d.begin() + p + n);
    p += n;
    return b;
  }
};

struct Out {
  std::string s;
  void u8(uint8_t v) { s.push_back((char)v); }
  void u32(uint32_t v) { s.append(reinterpret_cast<const char*>(&v), 4); }
  void u64(uint64_t v) { s.append(reinterpret_cast<const char*>(&v), 8); }
  void bytes(const uint8_t* p, size_t n) {
    if (n > 0xFFFFFFFFull) throw std::runtime_error("a key or value of 4 GiB or more");
    u32((uint32_t)n);
    s.append(reinterpret_cast<const char*>(p), n);
  }
  void bytes(const Bytes& b) { bytes(b.data(), b.size()); }
  void str(const std::string& b) { bytes(reinterpret_cast<const uint8_t*>(b.data()), b.size()); }
  void rec(const mtbl::Record& r) { bytes(r.key, r.key_len); bytes(r.val, r.val_len); }
};

Bytes read_file(const char* path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw std::runtime_error(std::string("cannot read ") + path);
  return Bytes(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

enum { kEndNone = 0, kEndErrOpen = 1, kEndErrNext = 2, kEndPanic = 3 };

struct State {
  std::unique_ptr<mtbl::Reader> reader;
  int open_end = kEndErrOpen;   // how the last 'O' failed, when reader is null
  std::string open_err = "no open";
};

mtbl::ReaderIntoIter make_iter(const mtbl::Reader& r, int mode, const Bytes& key, const Bytes& key2) {
  switch (mode) {
    case 0: return r.into_iter();
    case 1: return r.iter_from(key);
    case 2: return r.iter_prefix(key);
    case 3: return r.iter_range(key, key2);
  }
  throw std::runtime_error("script: unknown iterator mode");
}

void cmd_open(State& st, const Bytes& file, In& in, Out& out) {
  const bool verify = in.u8() != 0;
  st.reader.reset();
  out.u8('O');
  try {
    st.reader = std::make_unique<mtbl::Reader>(mtbl::ReaderBuilder().verify_checksums(verify).read(file));
    out.u8(0);
    out.str("");
  } catch (const mtbl::Error& e) {
    st.open_end = kEndErrOpen;
    st.open_err = mtbl::error_name(e.kind);
    out.u8(1);
    out.str(st.open_err);
  } catch (const mtbl::Panic&) {
    st.open_end = kEndPanic;
    st.open_err.clear();
    out.u8(2);
    out.str("");
  }
}

struct Op {
  bool seek;
  uint64_t n;
  Bytes key;
};

void cmd_iter(State& st, In& in, Out& out) {
  const int mode = in.u8();
  const Bytes key = in.bytes(), key2 = in.bytes();
  std::vector<Op> ops(in.u32());
  for (Op& o : ops) {
    o.seek = in.u8() != 0;
    if (o.seek) o.key = in.bytes();
    else o.n = in.u64();
  }
  int end = kEndNone;
  std::string err;
  std::vector<std::pair<uint64_t, uint8_t>> done;
  Out recs;
  uint64_t nrec = 0;
  std::optional<mtbl::ReaderIntoIter> it;
  if (!st.reader) {
    end = st.open_end;
    err = st.open_err;
  } else {
    try {
      it.emplace(make_iter(*st.reader, mode, key, key2));
    } catch (const mtbl::Error& e) {
      end = kEndErrOpen;
      err = mtbl::error_name(e.kind);
    } catch (const mtbl::Panic&) {
      end = kEndPanic;
    }
  }
  if (it) {
    try {
      for (const Op& o : ops) {
        if (o.seek) {
          try {
            it->seek(o.key);
            done.emplace_back(0, 0);
          } catch (const mtbl::Error& e) {
            done.emplace_back(0, 2);
            err = mtbl::error_name(e.kind);
          }
          continue;
        }
        uint64_t n = 0;
        uint8_t code = 0;
        for (uint64_t i = 0; i < o.n; ++i) {
          try {
            const auto r = it->next();
            if (!r) { code = 1; break; }
            recs.rec(*r);
            ++nrec;
            ++n;
          } catch (const mtbl::Error& e) {
            code = 2;
            err = mtbl::error_name(e.kind);
            break;
          }
        }
        done.emplace_back(n, code);
      }
    } catch (const mtbl::Panic&) {   // ends the script; the records before it are kept
      end = kEndPanic;
    }
  }
  out.u8('I');
  out.u8((uint8_t)end);
  out.str(err);
  out.u32((uint32_t)done.size());
  for (const auto& d : done) { out.u64(d.first); out.u8(d.second); }
  out.u64(nrec);
  out.s += recs.s;
}

void cmd_scan(State& st, In& in, Out& out) {
  const int mode = in.u8();
  const Bytes key = in.bytes(), key2 = in.bytes();
  const uint64_t max_records = in.u64();
  int end = kEndNone;
  std::string err;
  Out recs;
  uint64_t nrec = 0;
  if (!st.reader) {
    end = st.open_end;
    err = st.open_err;
  } else {
    bool built = false;
    try {
      mtbl::ReaderIntoIter it = make_iter(*st.reader, mode, key, key2);
      built = true;
      while (nrec < max_records) {
        const auto r = it.next();
        if (!r) break;
        recs.rec(*r);
        ++nrec;
      }
    } catch (const mtbl::Error& e) {
      end = built ? kEndErrNext : kEndErrOpen;
      err = mtbl::error_name(e.kind);
    } catch (const mtbl::Panic&) {
      end = kEndPanic;
    }
  }
  out.u8('S');
  out.u8((uint8_t)end);
  out.str(err);
  out.u64(nrec);
  out.s += recs.s;
}

// outcome of a command that has no records of its own before a failure
template <class F>
void guarded(State& st, Out& out, char tag, F&& body) {
  out.u8((uint8_t)tag);
  if (!st.reader) {
    out.u8(st.open_end == kEndPanic ? 3 : 2);
    out.str(st.open_err);
    return;
  }
  Out ok;
  try {
    body(ok);
  } catch (const mtbl::Error& e) {
    out.u8(2);
    out.str(mtbl::error_name(e.kind));
    return;
  } catch (const mtbl::Panic&) {
    out.u8(3);
    out.str("");
    return;
  }
  out.s += ok.s;
}

void cmd_get(State& st, In& in, Out& out) {
  const Bytes key = in.bytes();
  guarded(st, out, 'G', [&](Out& o) {
    const auto v = st.reader->get(key.data(), key.size());
    o.u8(v ? 0 : 1);
    o.str("");
    o.bytes(v ? *v : Bytes());
  });
}

void cmd_len(State& st, Out& out) {
  guarded(st, out, 'L', [&](Out& o) {
    const uint64_t n = st.reader->len();
    o.u8(0);
    o.str("");
    o.u64(n);
  });
}

void cmd_scan_batch(State& st, In& in, Out& out) {
  const uint32_t max_blocks = in.u32();
  std::vector<mtbl::ScanQuery> qs(in.u32());
  for (mtbl::ScanQuery& q : qs) {
    const int kind = in.u8();
    if (kind > 3) throw std::runtime_error("script: unknown query kind");
    q.kind = static_cast<mtbl::ScanQuery::Kind>(kind);
    q.key = in.bytes();
    q.key2 = in.bytes();
    const bool has = in.u8() != 0;
    const uint64_t m = in.u64();
    if (has) q.max_records = m;
  }
  guarded(st, out, 'B', [&](Out& o) {
    std::vector<uint8_t> served;
    const auto res = st.reader->scan_batch(qs, max_blocks, &served);
    if (res.size() != qs.size() || served.size() != qs.size()) throw std::runtime_error("scan_batch: result count");
    o.u8(0);
    o.str("");
    o.u32((uint32_t)res.size());
    for (const auto& recs : res) {
      o.u64(recs.size());
      for (const auto& kv : recs) { o.bytes(kv.first); o.bytes(kv.second); }
    }
    for (uint8_t s : served) o.u8(s);
  });
}

int run(const char* file_path, const char* script_path, const char* out_path) {
  const Bytes file = read_file(file_path);
  In in;
  in.d = read_file(script_path);
  std::FILE* f = std::fopen(out_path, "wb");
  if (!f) throw std::runtime_error(std::string("cannot write ") + out_path);
  State st;
  while (!in.done()) {
    Out out;
    const uint8_t c = in.u8();
    switch (c) {
      case 'O': cmd_open(st, file, in, out); break;
      case 'I': cmd_iter(st, in, out); break;
      case 'S': cmd_scan(st, in, out); break;
      case 'G': cmd_get(st, in, out); break;
      case 'L': cmd_len(st, out); break;
      case 'B': cmd_scan_batch(st, in, out); break;
      default: throw std::runtime_error("script: unknown command");
    }
    if (std::fwrite(out.s.data(), 1, out.s.size(), f) != out.s.size()) throw std::runtime_error("short write");
  }
  if (std::fclose(f) != 0) throw std::runtime_error("close failed");
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: iter_driver FILE SCRIPT OUT\n");
    return 2;
  }
  try {
    return run(argv[1], argv[2], argv[3]);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "iter_driver: %s\n", e.what());
    return 1;
  }
}

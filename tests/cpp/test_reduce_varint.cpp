// test_reduce_varint — mtbl::MergeReduce with ReduceEncoding::Varint (include/mtbl.hpp over
// mtblx_merge_emit_reduce / mtblx_sort_emit_reduce / mtblx_scan_reduce with MTBLX_REDUCE_VARINT) against
// a MergeFn that decodes, reduces and re-encodes on the host:
//   1. the Merger over 3 sources and over 70 (two rounds of 64; one key common to all 70), one
//      field summed, then three fields (min, max, sum); field lengths from 1 to 10 bytes
//   2. the Sorter: 5 000 records in random order over 700 keys plus one hot key, and a value that is
//      no varint alone in its group, which passes through; 127 + 1 and a sum that wraps
//   3. MergeError: a group of two with an unterminated value, in the Merger and in the Sorter; the
//      MergeFn throws for the same input
//   4. Reader::reduce_batch with a varint MergeReduce (get / prefix / range / from) against the same
//      fold over the records the test wrote, bad values among them
// Runs on the GPU.  Prints "OK <n>" on success, exits 1 on failure.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "mtbl.hpp"

static int g_checks = 0;
#define CHECK(c)                                                        \
  do {                                                                  \
    ++g_checks;                                                         \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

static mtbl::Bytes bytes(const std::string& s) { return mtbl::Bytes(s.begin(), s.end()); }

// varint_encode64 (src/varint.rs:64-76)
static void put(mtbl::Bytes& out, uint64_t x) {
  while (x >= 128) {
    out.push_back((uint8_t)(x | 128));
    x >>= 7;
  }
  out.push_back((uint8_t)x);
}

static mtbl::Bytes varints(std::initializer_list<uint64_t> xs) {
  mtbl::Bytes out;
  for (uint64_t x : xs) put(out, x);
  return out;
}

struct BadValue : std::runtime_error {
  BadValue() : std::runtime_error("bad value") {}
};

// nf varints back to back, each read within 10 bytes; anything else throws
static std::vector<uint64_t> fields(const mtbl::Bytes& v, size_t nf) {
  std::vector<uint64_t> out;
  size_t p = 0;
  for (size_t f = 0; f < nf; ++f) {
    uint64_t x = 0;
    bool done = false;
    for (int j = 0; j < 10 && p < v.size() && !done; ++j) {
      const uint8_t b = v[p++];
      x |= (uint64_t)(b & 0x7f) << (7 * j);
      done = !(b & 0x80);
    }
    if (!done) throw BadValue();
    out.push_back(x);
  }
  if (p != v.size()) throw BadValue();
  return out;
}

// the same function on the host: ops[f] 0 sum, 1 min, 2 max
static mtbl::MergeFn host_fn(std::vector<int> ops) {
  return [ops](const mtbl::Bytes&, const std::vector<mtbl::Bytes>& vs) {
    CHECK(vs.size() != 1);
    std::vector<uint64_t> acc = fields(vs[0], ops.size());
    for (size_t i = 1; i < vs.size(); ++i) {
      const std::vector<uint64_t> y = fields(vs[i], ops.size());
      for (size_t f = 0; f < ops.size(); ++f)
        acc[f] = ops[f] == 0 ? acc[f] + y[f] : ops[f] == 1 ? (y[f] < acc[f] ? y[f] : acc[f]) : (y[f] > acc[f] ? y[f] : acc[f]);
    }
    mtbl::Bytes out;
    for (uint64_t x : acc) put(out, x);
    return out;
  };
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {   // xorshift64*
  g_rng ^= g_rng >> 12;
  g_rng ^= g_rng << 25;
  g_rng ^= g_rng >> 27;
  return g_rng * 0x2545F4914F6CDD1Dull;
}
// a value whose encoding is 1 to 10 bytes long, every length as likely as another
static uint64_t rnd_len() {
  const int bits = 1 + (int)(rnd() % 64);
  return rnd() >> (64 - bits);
}

static mtbl::Bytes value(size_t nfields) {
  mtbl::Bytes v;
  for (size_t f = 0; f < nfields; ++f) put(v, rnd_len());
  return v;
}

// nsrc sorted sources: "common" in every one, keys shared by every third source, private keys
static std::vector<std::vector<std::pair<mtbl::Bytes, mtbl::Bytes>>> make_sources(int nsrc, size_t nfields) {
  std::vector<std::vector<std::pair<mtbl::Bytes, mtbl::Bytes>>> out(nsrc);
  char k[32];
  for (int s = 0; s < nsrc; ++s) {
    out[s].emplace_back(bytes("common"), value(nfields));
    for (int j = 0; j < 40; ++j) {
      std::snprintf(k, sizeof k, "p%02d-%03d", s, j);
      out[s].emplace_back(bytes(k), value(nfields));
    }
    for (int j = s % 3; j < 60; j += 3) {
      std::snprintf(k, sizeof k, "s%03d", j / 3 * 3 + (s % 2));
      if (out[s].back().first < bytes(k)) out[s].emplace_back(bytes(k), value(nfields));
    }
  }
  return out;
}

static std::vector<mtbl::Reader> readers(const std::vector<std::vector<std::pair<mtbl::Bytes, mtbl::Bytes>>>& src) {
  std::vector<mtbl::Reader> out;
  for (const auto& s : src) {
    mtbl::Writer w = mtbl::WriterBuilder().memory();
    for (const auto& kv : s) w.insert(kv.first, kv.second);
    out.push_back(mtbl::Reader::open(w.into_inner()));
  }
  return out;
}

int main() {
  // ---- 1. the Merger
  for (int nsrc : {3, 70}) {
    for (const std::vector<int>& ops : {std::vector<int>{MTBLX_REDUCE_SUM},
                                        std::vector<int>{MTBLX_REDUCE_MIN, MTBLX_REDUCE_MAX, MTBLX_REDUCE_SUM}}) {
      const auto src = make_sources(nsrc, ops.size());
      mtbl::MergerBuilder a = mtbl::Merger::builder(mtbl::MergeReduce::varint(ops)),
                          b = mtbl::Merger::builder(host_fn(ops));
      a.extend(readers(src));
      b.extend(readers(src));
      const auto got = a.build().into_merge_iter(), want = b.build().into_merge_iter();
      CHECK(got.size() == want.size() && !got.empty());
      CHECK(got == want);
      CHECK(got[0].first == bytes("common"));
      uint64_t sum = 0;   // "common": one value of every source; the summed field is the last one
      for (const auto& s : src) sum += fields(s[0].second, ops.size()).back();
      CHECK(fields(got[0].second, ops.size()).back() == sum);
    }
  }
  CHECK(mtbl::MergeReduce::varint({MTBLX_REDUCE_SUM}).encoding == mtbl::ReduceEncoding::Varint);
  CHECK(mtbl::MergeReduce::sum().encoding == mtbl::ReduceEncoding::U64le);
  // ---- 2. the Sorter
  for (const std::vector<int>& ops : {std::vector<int>{MTBLX_REDUCE_MAX}, std::vector<int>{MTBLX_REDUCE_SUM, MTBLX_REDUCE_MIN}}) {
    mtbl::Sorter a(mtbl::MergeReduce::varint(ops)), b(host_fn(ops));
    char k[32];
    for (int i = 0; i < 5000; ++i) {
      const uint64_t r = rnd();
      if (i % 3 == 0) std::snprintf(k, sizeof k, "hot");   // one group of 1 667 values: it crosses a tile of 1024
      else std::snprintf(k, sizeof k, "key-%04d", (int)(r % 700));
      const mtbl::Bytes v = value(ops.size());
      a.insert(bytes(k), v);
      b.insert(bytes(k), v);
    }
    a.insert(bytes("alone"), mtbl::Bytes(3, 0x80));   // unterminated, and alone: passes through
    b.insert(bytes("alone"), mtbl::Bytes(3, 0x80));
    const auto got = a.into_iter(), want = b.into_iter();
    CHECK(got.size() == want.size() && got.size() > 600);
    CHECK(got == want);
    CHECK(got[0].first == bytes("alone") && got[0].second == mtbl::Bytes(3, 0x80));
  }
  {
    mtbl::SorterBuilder sb = mtbl::Sorter::builder(mtbl::MergeReduce::varint({MTBLX_REDUCE_SUM}));
    mtbl::Sorter s = sb.build();
    s.insert(bytes("k"), varints({~0ull}));
    s.insert(bytes("k"), varints({2}));
    s.insert(bytes("l"), varints({127}));
    s.insert(bytes("l"), mtbl::Bytes{0x81, 0x00});   // 1, not canonical
    const auto got = s.into_iter();
    CHECK(got.size() == 2);
    CHECK(got[0].second == mtbl::Bytes{0x01});          // 2^64 - 1 + 2 wraps to 1: ten bytes in, one out
    CHECK((got[1].second == mtbl::Bytes{0x80, 0x01}));  // 127 + 1: one byte first, two out
  }
  // ---- 3. MergeError
  {
    const std::vector<std::vector<std::pair<mtbl::Bytes, mtbl::Bytes>>> src = {
        {{bytes("a"), varints({1})}, {bytes("m"), mtbl::Bytes(2, 0x80)}}, {{bytes("m"), varints({5})}, {bytes("z"), bytes("q")}}};
    mtbl::MergerBuilder a = mtbl::Merger::builder(mtbl::MergeReduce::varint({MTBLX_REDUCE_SUM})),
                        b = mtbl::Merger::builder(host_fn({0}));
    a.extend(readers(src));
    b.extend(readers(src));
    bool threw = false, host_threw = false;
    try {
      a.build().into_merge_iter();
    } catch (const mtbl::MergeError&) {
      threw = true;
    }
    try {
      b.build().into_merge_iter();
    } catch (const BadValue&) {
      host_threw = true;
    }
    CHECK(threw && host_threw);
    mtbl::Sorter s(mtbl::MergeReduce::varint({MTBLX_REDUCE_SUM}));
    s.insert(bytes("m"), varints({5}));
    s.insert(bytes("m"), varints({5, 6}));   // a trailing byte
    threw = false;
    try {
      s.into_iter();
    } catch (const mtbl::MergeError&) {
      threw = true;
    }
    CHECK(threw);
  }
  // ---- 4. Reader::reduce_batch
  {
    mtbl::Writer w = mtbl::WriterBuilder().block_size(512).memory();
    std::vector<std::pair<mtbl::Bytes, mtbl::Bytes>> recs;
    char k[32];
    for (int i = 0; i < 2000; ++i) {
      std::snprintf(k, sizeof k, "k%02d-%04d", i / 100, i);
      recs.emplace_back(bytes(k), i % 97 == 5 ? mtbl::Bytes(4, 0xff) : value(3));
      w.insert(recs.back().first, recs.back().second);
    }
    const mtbl::Reader r = mtbl::Reader::open(w.into_inner());
    const std::vector<int> ops = {MTBLX_REDUCE_MIN, MTBLX_REDUCE_MAX, MTBLX_REDUCE_SUM};
    std::vector<mtbl::ScanQuery> qs;
    auto query = [&](mtbl::ScanQuery::Kind kind, const mtbl::Bytes& key, const mtbl::Bytes& key2 = mtbl::Bytes()) {
      mtbl::ScanQuery q;
      q.kind = kind;
      q.key = key;
      q.key2 = key2;
      qs.push_back(q);
    };
    query(mtbl::ScanQuery::Prefix, bytes("k03-"));
    query(mtbl::ScanQuery::Get, recs[1999].first);
    query(mtbl::ScanQuery::Range, bytes("k05-0510"), bytes("k07-0777"));
    query(mtbl::ScanQuery::From, bytes("k19-"));
    query(mtbl::ScanQuery::Prefix, bytes("nothing"));
    const auto got = r.reduce_batch(qs, mtbl::MergeReduce::varint(ops));
    CHECK(got.size() == qs.size());
    auto want = [&](size_t lo, size_t hi) {
      mtbl::Reduced e;
      e.fields[0] = ~0ull;
      for (size_t i = lo; i < hi; ++i) {
        ++e.nrec;
        std::vector<uint64_t> x;
        try {
          x = fields(recs[i].second, 3);
        } catch (const BadValue&) {
          ++e.nbad;
          continue;
        }
        e.fields[0] = x[0] < e.fields[0] ? x[0] : e.fields[0];
        e.fields[1] = x[1] > e.fields[1] ? x[1] : e.fields[1];
        e.fields[2] += x[2];
      }
      return e;
    };
    const mtbl::Reduced e[5] = {want(300, 400), want(1999, 2000), want(510, 778), want(1900, 2000), want(0, 0)};
    for (size_t q = 0; q < qs.size(); ++q) {
      CHECK(got[q].nrec == e[q].nrec && got[q].nbad == e[q].nbad);
      for (int f = 0; f < 3; ++f) CHECK(got[q].fields[f] == e[q].fields[f]);
    }
    CHECK(e[0].nbad >= 1 && e[2].nbad >= 2);
  }
  std::printf("OK %d\n", g_checks);
  return 0;
}

// test_reduce — mtbl::MergeReduce (include/mtbl.hpp over mtblx_merge_emit_reduce /
// mtblx_sort_emit_reduce) against a MergeFn that computes the same function on the host:
//   1. the Merger over 3 sources and over 70 (two rounds of 64; one key common to all 70), one
//      field summed, then three fields (sum, min, max)
//   2. the Sorter: 5 000 records in random order over 700 keys plus one hot key, and a value of 3
//      bytes alone in its group, which passes through
//   3. MergeError: a group of two with a 7-byte value, in the Merger and in the Sorter; the MergeFn
//      throws for the same input
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

static mtbl::Bytes u64s(std::initializer_list<uint64_t> xs) {
  mtbl::Bytes out;
  for (uint64_t x : xs)
    for (int b = 0; b < 8; ++b) out.push_back((uint8_t)(x >> (8 * b)));
  return out;
}

static uint64_t field(const mtbl::Bytes& v, size_t f) {
  uint64_t x = 0;
  for (int b = 7; b >= 0; --b) x = (x << 8) | v[8 * f + b];
  return x;
}

struct BadLength : std::runtime_error {
  BadLength() : std::runtime_error("bad length") {}
};

// the same function on the host: ops[f] 0 sum, 1 min, 2 max
static mtbl::MergeFn host_fn(std::vector<int> ops) {
  return [ops](const mtbl::Bytes&, const std::vector<mtbl::Bytes>& vs) {
    CHECK(vs.size() != 1);
    for (const auto& v : vs)
      if (v.size() != 8 * ops.size()) throw BadLength();
    mtbl::Bytes out;
    for (size_t f = 0; f < ops.size(); ++f) {
      uint64_t x = field(vs[0], f);
      for (size_t i = 1; i < vs.size(); ++i) {
        const uint64_t y = field(vs[i], f);
        x = ops[f] == 0 ? x + y : ops[f] == 1 ? (y < x ? y : x) : (y > x ? y : x);
      }
      const mtbl::Bytes w = u64s({x});
      out.insert(out.end(), w.begin(), w.end());
    }
    return out;
  };
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {   // xorshift64*: values over the whole 64 bits, so sums wrap and the top bit is set
  g_rng ^= g_rng >> 12;
  g_rng ^= g_rng << 25;
  g_rng ^= g_rng >> 27;
  return g_rng * 0x2545F4914F6CDD1Dull;
}

// nsrc sorted sources: "common" in every one, keys shared by every third source, private keys
static std::vector<std::vector<std::pair<mtbl::Bytes, mtbl::Bytes>>> make_sources(int nsrc, size_t nfields) {
  std::vector<std::vector<std::pair<mtbl::Bytes, mtbl::Bytes>>> out(nsrc);
  char k[32];
  for (int s = 0; s < nsrc; ++s) {
    auto value = [&] {
      mtbl::Bytes v;
      for (size_t f = 0; f < nfields; ++f) {
        const mtbl::Bytes w = u64s({rnd()});
        v.insert(v.end(), w.begin(), w.end());
      }
      return v;
    };
    out[s].emplace_back(bytes("common"), value());
    for (int j = 0; j < 40; ++j) {
      std::snprintf(k, sizeof k, "p%02d-%03d", s, j);
      out[s].emplace_back(bytes(k), value());
    }
    for (int j = s % 3; j < 60; j += 3) {
      std::snprintf(k, sizeof k, "s%03d", j / 3 * 3 + (s % 2));   // some shared by many sources, some by few
      if (out[s].back().first < bytes(k)) out[s].emplace_back(bytes(k), value());
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
                                        std::vector<int>{MTBLX_REDUCE_SUM, MTBLX_REDUCE_MIN, MTBLX_REDUCE_MAX}}) {
      const auto src = make_sources(nsrc, ops.size());
      mtbl::MergerBuilder a = mtbl::Merger::builder(mtbl::MergeReduce{ops}), b = mtbl::Merger::builder(host_fn(ops));
      a.extend(readers(src));
      b.extend(readers(src));
      const auto got = a.build().into_merge_iter(), want = b.build().into_merge_iter();
      CHECK(got.size() == want.size() && !got.empty());
      CHECK(got == want);
      CHECK(got[0].first == bytes("common"));
      uint64_t sum = 0;   // "common": one value of every source
      for (const auto& s : src) sum += field(s[0].second, 0);
      CHECK(field(got[0].second, 0) == sum);
    }
  }
  CHECK(mtbl::MergeReduce::sum().ops == std::vector<int>{MTBLX_REDUCE_SUM});
  CHECK(mtbl::MergeReduce::min().ops == std::vector<int>{MTBLX_REDUCE_MIN});
  CHECK(mtbl::MergeReduce::max().ops == std::vector<int>{MTBLX_REDUCE_MAX});
  // ---- 2. the Sorter
  for (const std::vector<int>& ops : {std::vector<int>{MTBLX_REDUCE_MAX}, std::vector<int>{MTBLX_REDUCE_SUM, MTBLX_REDUCE_MIN}}) {
    mtbl::Sorter a(mtbl::MergeReduce{ops}), b(host_fn(ops));
    char k[32];
    for (int i = 0; i < 5000; ++i) {
      const uint64_t r = rnd();
      if (i % 3 == 0) std::snprintf(k, sizeof k, "hot");   // one group of 1 667 values: it crosses a tile of 1024
      else std::snprintf(k, sizeof k, "key-%04d", (int)(r % 700));
      mtbl::Bytes v;
      for (size_t f = 0; f < ops.size(); ++f) {
        const mtbl::Bytes w = u64s({rnd()});
        v.insert(v.end(), w.begin(), w.end());
      }
      a.insert(bytes(k), v);
      b.insert(bytes(k), v);
    }
    a.insert(bytes("alone"), bytes("xyz"));
    b.insert(bytes("alone"), bytes("xyz"));
    const auto got = a.into_iter(), want = b.into_iter();
    CHECK(got.size() == want.size() && got.size() > 600);
    CHECK(got == want);
    CHECK(got[0].first == bytes("alone") && got[0].second == bytes("xyz"));
  }
  {
    mtbl::SorterBuilder sb = mtbl::Sorter::builder(mtbl::MergeReduce::sum());
    mtbl::Sorter s = sb.build();
    s.insert(bytes("k"), u64s({~0ull}));
    s.insert(bytes("k"), u64s({2}));
    const auto got = s.into_iter();
    CHECK(got.size() == 1 && got[0].second == u64s({1}));   // 2^64 - 1 + 2 wraps to 1
  }
  // ---- 3. MergeError
  {
    const std::vector<std::vector<std::pair<mtbl::Bytes, mtbl::Bytes>>> src = {
        {{bytes("a"), u64s({1})}, {bytes("m"), mtbl::Bytes(7, 1)}}, {{bytes("m"), u64s({5})}, {bytes("z"), bytes("q")}}};
    mtbl::MergerBuilder a = mtbl::Merger::builder(mtbl::MergeReduce::sum()), b = mtbl::Merger::builder(host_fn({0}));
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
    } catch (const BadLength&) {
      host_threw = true;
    }
    CHECK(threw && host_threw);
    mtbl::Sorter s(mtbl::MergeReduce::sum());
    s.insert(bytes("m"), u64s({5}));
    s.insert(bytes("m"), mtbl::Bytes(7, 1));
    threw = false;
    try {
      s.into_iter();
    } catch (const mtbl::MergeError&) {
      threw = true;
    }
    CHECK(threw);
    bool refused = false;   // not a spec: refused before any device work
    try {
      mtbl::MergerBuilder bad = mtbl::Merger::builder(mtbl::MergeReduce{{0, 1, 2, 0, 1, 2, 0, 1, 2}});
    } catch (const std::invalid_argument&) {
      refused = true;
    }
    CHECK(refused);
  }
  std::printf("OK %d\n", g_checks);
  return 0;
}

// test_merger — mtbl::Merger (include/mtbl.hpp over mtblx_merge_plan / mtblx_merge_emit):
//   1. the reference's own `easy` scenario (src/merger.rs:267-304): ten overlapping sources of
//      {:010} keys with empty values, a concat merge function that must never see a group of one;
//      the merged keys are strictly increasing, and write_into gives a file that reads back the same
//   2. the stability promise: 64 sources holding the same 300 keys, every value its source's
//      number: MultiIter's values are 0 .. 63 in order for every key, and first / last / concat agree
// Runs on the GPU.  Prints "OK <n>" on success, exits 1 on failure.
#include <cstdio>
#include <cstdlib>
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

static std::vector<mtbl::Reader> easy_sources() {
  std::vector<mtbl::Reader> out;
  char k[16];
  for (int i = 0; i < 10; ++i) {
    mtbl::Writer w = mtbl::WriterBuilder().memory();
    for (int j = i; j < 30 * (i + 1); ++j) {
      std::snprintf(k, sizeof k, "%010d", j);
      w.insert(std::string(k), std::string());   // "{:010}".repeat(j / 10_000) is empty
    }
    out.push_back(mtbl::Reader::open(w.into_inner()));
  }
  return out;
}

int main() {
  // ---- 1. easy
  int calls = 0;
  mtbl::MergeFn concat = [&calls](const mtbl::Bytes&, const std::vector<mtbl::Bytes>& vs) {
    CHECK(vs.size() != 1);
    ++calls;
    mtbl::Bytes out;
    for (const auto& v : vs) out.insert(out.end(), v.begin(), v.end());
    return out;
  };
  {
    mtbl::MergerBuilder b = mtbl::Merger::builder(concat);
    b.extend(easy_sources());
    const mtbl::Merger m = b.build();
    const auto items = m.into_merge_iter();
    CHECK(items.size() == 300);
    char k[16];
    for (size_t i = 0; i < items.size(); ++i) {
      std::snprintf(k, sizeof k, "%010d", (int)i);
      CHECK(items[i].first == bytes(k));
      CHECK(items[i].second.empty());
      if (i) CHECK(items[i - 1].first < items[i].first);
    }
    CHECK(calls > 0);
    const auto groups = m.into_iter();
    CHECK(groups.size() == 300 && groups[0].second.size() == 1 && groups[9].second.size() == 10 &&
          groups[299].second.size() == 1);
    mtbl::Writer w = mtbl::WriterBuilder().memory();
    m.write_into(w);
    const mtbl::Reader back = mtbl::Reader::open(w.into_inner());
    CHECK(back.into_iter().collect() == items);
    // the built-in concat gives the same stream
    mtbl::MergerBuilder b2 = mtbl::Merger::builder(mtbl::MergeConcat{});
    b2.extend(easy_sources());
    CHECK(b2.build().into_merge_iter() == items);
  }
  // ---- 2. stability: 64 sources, the same keys, values = source number
  {
    auto sources = [] {
      std::vector<mtbl::Reader> out;
      char k[16];
      for (int s = 0; s < 64; ++s) {
        mtbl::Writer w = mtbl::WriterBuilder().memory();
        for (int j = 0; j < 300; ++j) {
          std::snprintf(k, sizeof k, "key-%06d", j);
          w.insert(bytes(k), mtbl::Bytes(1 + s % 3, (uint8_t)s));
        }
        out.push_back(mtbl::Reader::open(w.into_inner()));
      }
      return out;
    };
    mtbl::MergerBuilder b = mtbl::Merger::builder(mtbl::MergeFn([](const mtbl::Bytes&, const std::vector<mtbl::Bytes>& v) {
      return v[0];
    }));
    b.extend(sources());
    const auto groups = b.build().into_iter();
    CHECK(groups.size() == 300);
    mtbl::Bytes joined;
    for (int s = 0; s < 64; ++s) joined.insert(joined.end(), 1 + s % 3, (uint8_t)s);
    for (const auto& g : groups) {
      CHECK(g.second.size() == 64);
      for (int s = 0; s < 64; ++s) CHECK(g.second[s] == mtbl::Bytes(1 + s % 3, (uint8_t)s));
    }
    mtbl::MergerBuilder bc = mtbl::Merger::builder(mtbl::MergeConcat{}), bf = mtbl::Merger::builder(mtbl::MergeFirst{}),
                        bl = mtbl::Merger::builder(mtbl::MergeLast{});
    bc.extend(sources());
    bf.extend(sources());
    bl.extend(sources());
    const auto c = bc.build().into_merge_iter(), f = bf.build().into_merge_iter(), l = bl.build().into_merge_iter();
    CHECK(c.size() == 300 && f.size() == 300 && l.size() == 300);
    for (size_t i = 0; i < 300; ++i) {
      CHECK(c[i].first == groups[i].first && f[i].first == groups[i].first && l[i].first == groups[i].first);
      CHECK(c[i].second == joined);
      CHECK(f[i].second == mtbl::Bytes(1, 0));
      CHECK(l[i].second == mtbl::Bytes(1, 63));
    }
  }
  std::printf("OK %d\n", g_checks);
  return 0;
}

// test_sorter — mtbl::Sorter (include/mtbl.hpp over mtblx_sort_plan / mtblx_sort_emit and the
// device Merger):
//   1. the reference's own `simple` test (src/sorter.rs:264-295): abstract -> lollol, allo -> lol,
//      hello -> kiki, with a merge function that must never see a group of one; write_into gives a
//      file that reads back the same; the built-in concat gives the same stream
//   2. the stability promise: 3000 records over 30 keys in a scattered order, every value its
//      insertion number: concat joins every key's values in insertion order, first / last pick
//      the first / last inserted, and a merge function sees them in that order
//   3. the chunk rule (:128-137): 8 B keys + 1016 B values with max_memory at its minimum cut a
//      chunk at every 6144th insert; with max_nb_chunks(1) the chunks are merged on the way
// Runs on the GPU.  Prints "OK <n>" on success, exits 1 on failure.
#include <cstdio>
#include <cstdlib>
#include <map>
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

int main() {
  // ---- 1. simple
  {
    int calls = 0;
    mtbl::MergeFn merge = [&calls](const mtbl::Bytes&, const std::vector<mtbl::Bytes>& vs) {
      CHECK(vs.size() != 1);
      ++calls;
      mtbl::Bytes out;
      for (const auto& v : vs) out.insert(out.end(), v.begin(), v.end());
      return out;
    };
    const std::vector<std::pair<mtbl::Bytes, mtbl::Bytes>> want = {
        {bytes("abstract"), bytes("lollol")}, {bytes("allo"), bytes("lol")}, {bytes("hello"), bytes("kiki")}};
    auto fill = [](mtbl::Sorter& s) {
      s.insert(std::string("hello"), std::string("kiki"));
      s.insert(std::string("abstract"), std::string("lol"));
      s.insert(std::string("allo"), std::string("lol"));
      s.insert(std::string("abstract"), std::string("lol"));
    };
    mtbl::Sorter s = mtbl::SorterBuilder(merge).chunk_compression_type(mtbl::CompressionType::Snappy).build();
    fill(s);
    mtbl::Writer w = mtbl::WriterBuilder().memory();
    s.write_into(w);
    CHECK(calls == 1);
    CHECK(s.chunk_sizes() == std::vector<size_t>{4} && s.merges() == 0);
    const mtbl::Reader back = mtbl::Reader::open(w.into_inner());
    CHECK(back.into_iter().collect() == want);
    mtbl::Sorter c(mtbl::MergeConcat{});
    fill(c);
    CHECK(c.into_iter() == want);
    mtbl::Sorter e = mtbl::Sorter::builder(mtbl::MergeConcat{}).build();   // nothing inserted: an empty chunk, no item
    CHECK(e.into_iter().empty() && e.chunk_sizes() == std::vector<size_t>{0});
  }
  // ---- 2. stability: 3000 records over 30 keys, values = insertion number
  {
    std::map<std::string, std::vector<std::string>> by_key;
    std::vector<std::pair<std::string, std::string>> recs;
    char k[16];
    for (int i = 0; i < 3000; ++i) {
      std::snprintf(k, sizeof k, "key-%02d", (i * 7919 + i / 30) % 30);
      recs.emplace_back(k, std::to_string(i) + ";");
      by_key[k].push_back(recs.back().second);
    }
    CHECK(by_key.size() == 30);
    mtbl::Sorter sc(mtbl::MergeConcat{}), sf(mtbl::MergeFirst{}), sl(mtbl::MergeLast{});
    bool in_order = true;
    mtbl::Sorter sfn(mtbl::MergeFn([&](const mtbl::Bytes& key, const std::vector<mtbl::Bytes>& vs) {
      const auto& want = by_key[std::string(key.begin(), key.end())];
      in_order = in_order && vs.size() == want.size();
      for (size_t j = 0; in_order && j < vs.size(); ++j) in_order = vs[j] == bytes(want[j]);
      return vs[0];
    }));
    for (const auto& r : recs) {
      sc.insert(r.first, r.second);
      sf.insert(r.first, r.second);
      sl.insert(r.first, r.second);
      sfn.insert(r.first, r.second);
    }
    const auto c = sc.into_iter(), f = sf.into_iter(), l = sl.into_iter(), g = sfn.into_iter();
    CHECK(c.size() == 30 && f.size() == 30 && l.size() == 30 && g.size() == 30);
    CHECK(in_order);
    size_t i = 0;
    for (const auto& kv : by_key) {   // std::map: keys ascending
      std::string joined;
      for (const auto& v : kv.second) joined += v;
      CHECK(c[i].first == bytes(kv.first) && f[i].first == bytes(kv.first) && l[i].first == bytes(kv.first));
      CHECK(c[i].second == bytes(joined));
      CHECK(f[i].second == bytes(kv.second.front()));
      CHECK(l[i].second == bytes(kv.second.back()));
      CHECK(g[i].second == bytes(kv.second.front()));
      ++i;
    }
  }
  // ---- 3. the chunk rule: 6144 * 1024 + 131072 * 32 = 10485760
  {
    mtbl::Sorter s = mtbl::Sorter::builder(mtbl::MergeLast{}).max_memory(0).max_nb_chunks(1).build();
    char k[16], num[16];
    for (int i = 0; i < 2 * 6144 + 10; ++i) {
      std::snprintf(k, sizeof k, "%08d", i % 8000);   // keys 0 .. 4297 occur twice, in different chunks
      std::snprintf(num, sizeof num, "%08d", i);
      std::string v(1016, 'p');                       // the value starts with its insertion number
      v.replace(0, 8, num);
      s.insert(std::string(k), v);
      if (i == 6142) CHECK(s.chunk_sizes().empty());
    }
    CHECK((s.chunk_sizes() == std::vector<size_t>{6144, 6144}) && s.merges() == 1);
    const auto out = s.into_iter();
    CHECK((s.chunk_sizes() == std::vector<size_t>{6144, 6144, 10}) && s.merges() == 1);
    CHECK(out.size() == 8000);
    for (int j = 0; j < 8000; ++j) {
      std::snprintf(k, sizeof k, "%08d", j);
      CHECK(out[j].first == bytes(k) && out[j].second.size() == 1016);
      char want[16];
      std::snprintf(want, sizeof want, "%08d", j < 2 * 6144 + 10 - 8000 ? j + 8000 : j);   // the last inserted
      CHECK(std::string(out[j].second.begin(), out[j].second.begin() + 8) == want);
    }
  }
  std::printf("OK %d\n", g_checks);
  return 0;
}

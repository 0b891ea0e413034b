// test_scan_reduce — mtbl::Reader::reduce_batch (include/mtbl.hpp over mtblx_scan_reduce) against
// expectations written by tests/test_cpp_scan_reduce.py from the oracle's records and Reduce.fold.
//
//   test_scan_reduce <file.mtbl> <case.txt>
// case.txt: "ops <op>..." , "max_blocks <n>", then one line per query:
//   <kind 0..3> <key hex | -> <key2 hex | -> <limit | -1> <field>... <nrec> <nbad> <served 0 | 1 | -1>
// Runs on the GPU.  Prints "OK <n>" on success, exits 1 on failure.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "mtbl.hpp"

static int g_checks = 0;
#define CHECK(c)                                                        \
  do {                                                                  \
    ++g_checks;                                                         \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s (query %d)\n", __FILE__, __LINE__, #c, g_query); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)
static int g_query = -1;

static mtbl::Bytes unhex(const std::string& h) {
  mtbl::Bytes out;
  if (h == "-") return out;
  for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((uint8_t)std::stoul(h.substr(i, 2), nullptr, 16));
  return out;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: test_scan_reduce <file.mtbl> <case.txt>\n");
    return 2;
  }
  std::ifstream f(argv[1], std::ios::binary);
  const mtbl::Bytes data((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  CHECK(!data.empty());
  const mtbl::Reader r = mtbl::Reader::open(data);
  std::ifstream c(argv[2]);
  mtbl::MergeReduce red;
  uint32_t max_blocks = 64;
  std::vector<mtbl::ScanQuery> qs;
  std::vector<mtbl::Reduced> want;
  std::vector<int> want_served;
  std::string line;
  while (std::getline(c, line)) {
    std::istringstream in(line);
    std::string w;
    in >> w;
    if (w == "ops") {
      int op;
      while (in >> op) red.ops.push_back(op);
    } else if (w == "max_blocks") {
      in >> max_blocks;
    } else if (!w.empty()) {
      mtbl::ScanQuery q;
      std::string k, k2;
      long long lim;
      q.kind = (mtbl::ScanQuery::Kind)std::stoi(w);
      in >> k >> k2 >> lim;
      q.key = unhex(k);
      q.key2 = unhex(k2);
      if (lim >= 0) q.max_records = (uint64_t)lim;
      mtbl::Reduced e;
      for (size_t i = 0; i < red.ops.size(); ++i) in >> e.fields[i];
      int sv;
      in >> e.nrec >> e.nbad >> sv;
      CHECK(!in.fail());
      qs.push_back(q);
      want.push_back(e);
      want_served.push_back(sv);
    }
  }
  CHECK(!red.ops.empty() && !qs.empty());
  std::vector<uint8_t> served;
  const auto got = r.reduce_batch(qs, red, max_blocks, &served);
  CHECK(got.size() == qs.size() && served.size() == qs.size());
  int kernel = 0;
  for (size_t i = 0; i < qs.size(); ++i) {
    g_query = (int)i;
    for (int fi = 0; fi < 8; ++fi) CHECK(got[i].fields[fi] == want[i].fields[fi]);
    CHECK(got[i].nrec == want[i].nrec && got[i].nbad == want[i].nbad);
    if (want_served[i] >= 0) CHECK(served[i] == want_served[i]);
    kernel += served[i];
  }
  g_query = -1;
  CHECK(r.reduce_batch({}, red).empty());
  bool threw = false;
  try {
    r.reduce_batch(qs, mtbl::MergeReduce{{}});
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  CHECK(threw);
  std::printf("OK %d kernel %d\n", g_checks, kernel);
  return 0;
}

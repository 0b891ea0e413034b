// test_merger_scan — mtbl::Merger::scan_batch (include/mtbl.hpp over Reader::scan_batch and
// mtblx_merge_seg_plan / mtblx_merge_seg_emit), driven by tests/test_cpp_merger_scan.py:
//   test_merger_scan <merge> <max_blocks> <queries file> <source .mtbl>...
// <merge>: concat | first | last | sum (MergeReduce::sum) | fn (a MergeFn that joins the values and
// must never see a group of one).  The queries file holds one query per line:
//   <from|get|prefix|range> <hex key or -> <hex key2 or -> <max_records or ->
// The answers go to stdout, one line "Q <index> <items> <served>" per query followed by one line
// "<hex key or -> <hex value or ->" per item; the Python side compares them with its model.
// Runs on the GPU.  Exits 1 with a message on any error.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "mtbl.hpp"

static mtbl::Bytes unhex(const std::string& s) {
  mtbl::Bytes out;
  if (s == "-") return out;
  for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)std::stoi(s.substr(i, 2), nullptr, 16));
  return out;
}

static std::string hex(const mtbl::Bytes& b) {
  if (b.empty()) return "-";
  static const char* d = "0123456789abcdef";
  std::string out;
  for (uint8_t c : b) {
    out.push_back(d[c >> 4]);
    out.push_back(d[c & 15]);
  }
  return out;
}

static mtbl::MergerBuilder builder(const std::string& merge) {
  if (merge == "concat") return mtbl::Merger::builder(mtbl::MergeConcat{});
  if (merge == "first") return mtbl::Merger::builder(mtbl::MergeFirst{});
  if (merge == "last") return mtbl::Merger::builder(mtbl::MergeLast{});
  if (merge == "sum") return mtbl::Merger::builder(mtbl::MergeReduce::sum());
  if (merge == "fn")
    return mtbl::Merger::builder(mtbl::MergeFn([](const mtbl::Bytes&, const std::vector<mtbl::Bytes>& vs) {
      if (vs.size() < 2) {
        std::fprintf(stderr, "the merge function was called for a group of %zu\n", vs.size());
        std::exit(1);
      }
      mtbl::Bytes out;
      for (const auto& v : vs) out.insert(out.end(), v.begin(), v.end());
      return out;
    }));
  std::fprintf(stderr, "unknown merge %s\n", merge.c_str());
  std::exit(1);
}

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: test_merger_scan <merge> <max_blocks> <queries> <source>...\n");
    return 1;
  }
  try {
    std::vector<mtbl::ScanQuery> qs;
    std::ifstream qf(argv[3]);
    std::string line;
    while (std::getline(qf, line)) {
      std::istringstream is(line);
      std::string kind, k, k2, lim;
      if (!(is >> kind >> k >> k2 >> lim)) continue;
      mtbl::ScanQuery q;
      q.kind = kind == "from" ? mtbl::ScanQuery::From : kind == "get" ? mtbl::ScanQuery::Get
               : kind == "prefix" ? mtbl::ScanQuery::Prefix : mtbl::ScanQuery::Range;
      q.key = unhex(k);
      q.key2 = unhex(k2);
      if (lim != "-") q.max_records = std::stoull(lim);
      qs.push_back(q);
    }
    mtbl::MergerBuilder b = builder(argv[1]);
    for (int i = 4; i < argc; ++i) {
      std::ifstream f(argv[i], std::ios::binary);
      b.push(mtbl::Reader::open(mtbl::Bytes(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>())));
    }
    const mtbl::Merger m = b.build();
    std::vector<uint8_t> served;
    const auto out = m.scan_batch(qs, (uint32_t)std::stoul(argv[2]), &served);
    if (out.size() != qs.size() || served.size() != qs.size()) {
      std::fprintf(stderr, "%zu answers for %zu queries\n", out.size(), qs.size());
      return 1;
    }
    for (size_t q = 0; q < out.size(); ++q) {
      std::printf("Q %zu %zu %d\n", q, out[q].size(), (int)served[q]);
      for (const auto& kv : out[q]) std::printf("%s %s\n", hex(kv.first).c_str(), hex(kv.second).c_str());
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 1;
  }
  return 0;
}

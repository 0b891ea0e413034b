// test_scan_batch — mtbl::Reader::scan_batch (include/mtbl.hpp over mtblx_scan_plan / mtblx_scan_emit):
// a batch of from / get / prefix / range queries on a file of 20000 counter keys equals the same
// queries run one at a time through iter_from / iter_prefix / iter_range / get, whether the kernels
// served a query or handed it back (more than max_blocks data blocks).
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

static mtbl::ScanQuery query(mtbl::ScanQuery::Kind kind, const std::string& k, const std::string& k2 = "",
                             std::optional<uint64_t> max_records = std::nullopt) {
  mtbl::ScanQuery q;
  q.kind = kind;
  q.key = bytes(k);
  q.key2 = bytes(k2);
  q.max_records = max_records;
  return q;
}

static mtbl::Reader::Records one(const mtbl::Reader& r, const mtbl::ScanQuery& q) {
  mtbl::Reader::Records out;
  const uint64_t lim = q.max_records ? *q.max_records : ~0ull;
  if (q.kind == mtbl::ScanQuery::Get) {
    if (auto v = r.get(q.key.data(), q.key.size())) out.emplace_back(q.key, *v);
    return out;
  }
  mtbl::ReaderIntoIter it = q.kind == mtbl::ScanQuery::From ? r.iter_from(q.key)
                            : q.kind == mtbl::ScanQuery::Prefix ? r.iter_prefix(q.key) : r.iter_range(q.key, q.key2);
  while (out.size() < lim) {
    auto rec = it.next();
    if (!rec) break;
    out.emplace_back(rec->key_bytes(), rec->val_bytes());
  }
  return out;
}

int main() {
  mtbl::Writer w = mtbl::WriterBuilder().block_size(1024).memory();
  char k[16];
  for (int i = 0; i < 20000; ++i) {
    std::snprintf(k, sizeof k, "k%06d", i);
    w.insert(std::string(k), std::string((size_t)(i % 50), 'v'));
  }
  const mtbl::Reader r = mtbl::Reader::open(w.into_inner());
  using Q = mtbl::ScanQuery;
  std::vector<Q> qs = {query(Q::Prefix, "k01234"),         query(Q::Prefix, "k012"),
                       query(Q::Range, "k000100", "k000130"), query(Q::From, "k019990", "", 5),
                       query(Q::From, "k019990"),          query(Q::Get, "k000777"),
                       query(Q::Get, "nokey"),             query(Q::Range, "k5", "k4"),
                       query(Q::Prefix, "zz"),             query(Q::From, "", "", 0),
                       query(Q::Prefix, "k00")};
  for (int i = 0; i < 70; ++i) {
    std::snprintf(k, sizeof k, "k%04d", 37 * i);
    qs.push_back(query(Q::Prefix, k));
  }
  std::vector<uint8_t> served;
  const auto got = r.scan_batch(qs, 64, &served);
  CHECK(got.size() == qs.size() && served.size() == qs.size());
  for (size_t i = 0; i < qs.size(); ++i) {
    CHECK(got[i] == one(r, qs[i]));
    CHECK(served[i] == (i == 10 ? 0 : 1));   // "k00": 10000 records, far more than 64 blocks
  }
  CHECK(got[0].size() == 10 && got[1].size() == 1000 && got[2].size() == 31 && got[3].size() == 5);
  CHECK(got[4].size() == 10 && got[5].size() == 1 && got[6].empty() && got[7].empty() && got[9].empty());
  CHECK(got[5][0].second == mtbl::Bytes(777 % 50, 'v'));
  // more than max_blocks data blocks: handed back and answered by the iterators
  const auto small = r.scan_batch(qs, 2, &served);
  for (size_t i = 0; i < qs.size(); ++i) CHECK(small[i] == got[i]);
  CHECK(served[0] == 1 && served[1] == 0 && served[10] == 0);
  CHECK(r.scan_batch({}).empty());
  std::printf("OK %d\n", g_checks);
  return 0;
}

// test_valpos — detail::decode_batch_positions (include/mtbl.hpp, mtblx_decode_blocks_valpos) on a
// cfg1 file written by the C++ Writer: every value read from the file through its position
// (BlockIter::get's val_offset, src/block.rs:204-213) equals the one decode_batch copied, and
// every other output of the two calls is the same.
// Runs on the GPU.  Prints "OK <n>" on success, exits 1 on failure.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "mtbl.hpp"
#include "mtblx_host.h"

static int g_checks = 0;
#define CHECK(c)                                                        \
  do {                                                                  \
    ++g_checks;                                                         \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

int main() {
  // cfg1 records (examples/dump.rs plumbing): key "{:010}", value "{:010}" x (1 + i % 8)
  mtbl::Writer w = mtbl::WriterBuilder().compression_type(mtbl::CompressionType::None).block_size(4096).memory();
  char k[16];
  const int nrec = 10000;
  for (int i = 0; i < nrec; ++i) {
    std::snprintf(k, sizeof k, "%010d", i);
    std::string val;
    for (int r = 0; r < 1 + i % 8; ++r) val += k;
    w.insert(k, val);
  }
  const mtbl::Bytes file = w.into_inner();

  // the data blocks' content windows: frames from offset 0 up to the index block (src/reader.rs:140-164)
  mtblx_footer ft{};
  CHECK(mtblx_read_footer(file.data(), file.size(), &ft) == 0);
  std::vector<uint64_t> off;
  std::vector<uint32_t> len;
  uint32_t max_len = 0;
  for (uint64_t at = 0; at < ft.meta[0];) {
    uint64_t co = 0, cl = 0;
    int panic = 0;
    CHECK(mtblx_frame_block(file.data(), file.size(), ft.version, at, 1, &co, &cl, &panic) == 0 && !panic);
    off.push_back(co);
    len.push_back((uint32_t)cl);
    max_len = std::max(max_len, (uint32_t)cl);
    at = co + cl;
  }
  const uint32_t nblk = (uint32_t)off.size();
  CHECK(nblk == ft.meta[4] && nblk > 10);

  using namespace mtbl::detail;
  DevBuf d_file = upload(file.data(), file.size()), d_off = upload(off.data(), nblk), d_len = upload(len.data(), nblk);
  const Decoded a = decode_batch(d_file.as<uint8_t>(), file.size(), d_off.as<uint64_t>(), d_len.as<uint32_t>(), nblk,
                                 max_len);
  const Decoded p = decode_batch_positions(d_file.as<uint8_t>(), file.size(), d_off.as<uint64_t>(),
                                           d_len.as<uint32_t>(), nblk, max_len);
  CHECK(a.val_pos.empty() && p.vals.empty());
  CHECK(p.nrec == a.nrec && p.status == a.status && p.rec_base == a.rec_base && p.key_base == a.key_base &&
        p.val_base == a.val_base && p.key_end == a.key_end && p.val_end == a.val_end && p.keys == a.keys);
  CHECK(p.val_pos.size() == (size_t)nrec && a.val_end.size() == (size_t)nrec);
  size_t seen = 0;
  for (uint32_t b = 0; b < nblk; ++b) {
    CHECK(a.status[b] == MTBLX_ST_OK);
    uint32_t pv = 0;
    for (uint32_t i = 0; i < a.nrec[b]; ++i) {
      const uint64_t r = a.rec_base[b] + i;
      const uint32_t n = a.val_end[r] - pv;
      CHECK((uint64_t)p.val_pos[r] + n <= (uint64_t)len[b] - 4);
      CHECK(std::memcmp(file.data() + off[b] + p.val_pos[r], a.vals.data() + a.val_base[b] + pv, n) == 0);
      pv = a.val_end[r];
      ++seen;
    }
  }
  CHECK(seen == (size_t)nrec);
  std::printf("OK %d\n", g_checks);
  return 0;
}

// test_snappy_reader — mtbl::Reader over a Snappy file (include/mtbl.hpp: load_framed stages the
// blocks on the device, mtblx_stage_plan / mtblx_stage_emit).  Reads the .mtbl file named on the
// command line (argv[2] == "noverify": checksums off), iterates it to the end and prints
//   one line "<hex key> <hex value>" per record,
//   "END none" | "END err <error name>" | "END panic"      how the iteration ended,
//   "HOSTDEC <n>"                                          Reader::host_decompressed_blocks().
// tests/test_cpp_snappy_reader.py compares the dump with the oracle's.  Runs on the GPU.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>

#include "mtbl.hpp"

static void hex(const mtbl::Bytes& b) {
  for (uint8_t c : b) std::printf("%02x", c);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  if (!in) return 2;
  const mtbl::Bytes data((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  const bool verify = !(argc > 2 && std::string(argv[2]) == "noverify");
  try {
    const mtbl::Reader r = mtbl::ReaderBuilder().verify_checksums(verify).read(data);
    std::string end = "none";
    try {
      mtbl::ReaderIntoIter it = r.into_iter();
      while (auto rec = it.next()) {
        hex(rec->key_bytes());
        std::printf(" ");
        hex(rec->val_bytes());
        std::printf("\n");
      }
    } catch (const mtbl::Error& e) {
      end = std::string("err ") + e.what();
    } catch (const mtbl::Panic&) {
      end = "panic";
    }
    std::printf("END %s\nHOSTDEC %llu\n", end.c_str(), (unsigned long long)r.host_decompressed_blocks());
  } catch (const mtbl::Error& e) {
    std::printf("END err %s\nHOSTDEC 0\n", e.what());
  } catch (const mtbl::Panic&) {
    std::printf("END panic\nHOSTDEC 0\n");
  }
  return 0;
}

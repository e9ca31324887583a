// Stand-alone runner (tests/test_unit_ops_host.py builds it with -fsanitize=address,undefined, with and without
// -DHM_BOUNDS): csrc/unit_ops.h on the CPU.  usage: unit_ops_host CASES RESULTS
// CASES is a sequence of blocks of u32 words: table (0 Fq, 1 Fr, 2 curve), op, n, then n input records; RESULTS gets the
// same blocks with the n output records.  A violated HM_BOUNDS precondition aborts with its message.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "unit_ops.h"

using namespace hm;

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s CASES RESULTS\n", argv[0]);
    return 2;
  }
  std::FILE* fi = std::fopen(argv[1], "rb");
  std::FILE* fo = std::fopen(argv[2], "wb");
  if (!fi || !fo) {
    std::fprintf(stderr, "cannot open the case or the result file\n");
    return 2;
  }
  uint32_t head[3];
  size_t cases = 0;
  while (std::fread(head, 4, 3, fi) == 3) {
    const uint32_t table = head[0], op = head[1], n = head[2];
    if (table > 2 || n > (1u << 24)) {
      std::fprintf(stderr, "bad block header %u %u %u\n", table, op, n);
      return 2;
    }
    const size_t wi = table == 2 ? unit::CURVE_IN_WORDS : unit::FIELD_IN_WORDS;
    const size_t wo = table == 2 ? unit::CURVE_OUT_WORDS : unit::FIELD_OUT_WORDS;
    std::vector<uint32_t> in(wi * n), out(wo * n, 0u);
    if (std::fread(in.data(), 4, in.size(), fi) != in.size()) {
      std::fprintf(stderr, "truncated block %u %u %u\n", table, op, n);
      return 2;
    }
    for (size_t i = 0; i < n; ++i) {
      bool known;
      if (table == 0) known = unit::field_op<FqParams>((int)op, &in[wi * i], &out[wo * i]);
      else if (table == 1) known = unit::field_op<FrParams>((int)op, &in[wi * i], &out[wo * i]);
      else known = unit::curve_op((int)op, &in[wi * i], &out[wo * i]);
      if (!known) {
        std::fprintf(stderr, "table %u has no op %u\n", table, op);
        return 2;
      }
    }
    if (std::fwrite(head, 4, 3, fo) != 3 || std::fwrite(out.data(), 4, out.size(), fo) != out.size()) {
      std::fprintf(stderr, "cannot write the results\n");
      return 2;
    }
    cases += n;
  }
  std::fclose(fi);
  if (std::fclose(fo) != 0) return 2;
  std::printf("ok: %zu cases\n", cases);
  return 0;
}

// Stand-alone runner (tests/test_graph_plan_host.py builds it with -fsanitize=address,undefined): csrc/graph_lower.h's
// graph_check_call and graph_launch_plan over the sweep of that test -- kind x log_size 0..30 x segments {1, 2, 5, 8} x units
// {1, 2, 3, 4, 7, 64, 65, 2^20} x n_slots {0, 1, 37} x max_blocks {1, 5, 1280} -- with the column tables the check walks held in
// real arrays of exactly n_columns entries, so that a read past either is seen.  Prints the admitted rows and a checksum of their
// plans, which the test compares with its own through libhm_hostcheck.so; the plan's invariants are asserted here too.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "graph_lower.h"

using namespace hm;

int main() {
  const uint32_t segments[] = {1, 2, 5, 8}, n_slots[] = {0, 1, 37}, max_blocks[] = {1, 5, 1280};
  const uint64_t units[] = {1, 2, 3, 4, 7, 64, 65, 1ull << 20};
  const size_t n_dyn = 6;
  alignas(16) static unsigned char cell[64];
  uint64_t rows = 0, refused = 0, sum = 0;
  for (uint32_t kind = 0; kind < 3; ++kind)
    for (uint32_t log_size = 0; log_size <= 30; ++log_size)
      for (uint32_t seg : segments)
        for (uint64_t u : units) {
          if (kind == GRAPH_SINGLE && u != 1) continue;
          const size_t n_columns = 1 + (log_size + seg) % 7;
          std::vector<const void*> bases(n_columns, cell);
          std::vector<uint64_t> strides(n_columns, 8);
          const uint64_t size = (uint64_t)seg << log_size;
          const GraphCall c{(GraphCallKind)kind, n_columns, (size_t)u, n_dyn, log_size, seg, log_size & 1u, cell, size * 8, bases.data(),
                            kind == GRAPH_SINGLE ? nullptr : strides.data(), nullptr};
          const char* why = graph_check_call(c, n_columns, n_dyn);
          if (why) {
            if (std::strncmp(why, "graph:", 6) != 0) return std::printf("a reason without its prefix: %s\n", why), 1;
            ++refused;
            continue;
          }
          for (uint32_t slots : n_slots)
            for (uint32_t cap : max_blocks) {
              const GraphPlan p = graph_launch_plan((GraphCallKind)kind, size, u, slots, n_dyn, cap);
              const uint64_t full = 256ull * cap;
              const bool ok = p.size == size && p.blocks >= 1 && p.blocks <= cap && p.T == 256 * p.blocks &&
                              256ull * p.blocks >= (p.lanes < full ? p.lanes : full) && ((uint64_t)p.rows_per << p.log_c) == 256 && p.log_c <= 8 &&
                              (1ull << p.log_c) < 2 * u && (kind == GRAPH_CIRCUITS || p.log_c == 0) &&
                              p.scratch_bytes == (size_t)slots * 9 * p.T * 4 && p.args_bytes % 4 == 0;
              if (!ok) return std::printf("invariant broken: kind %u size %llu units %llu slots %u cap %u\n", kind, (unsigned long long)size,
                                          (unsigned long long)u, slots, cap), 1;
              ++rows;
              sum += p.blocks + 3 * p.log_c + 5 * p.lanes + 7 * (uint64_t)p.scratch_bytes + 11 * (uint64_t)p.args_bytes;
            }
        }
  std::printf("rows %llu refused %llu checksum %llu\n", (unsigned long long)rows, (unsigned long long)refused, (unsigned long long)sum);
  return 0;
}

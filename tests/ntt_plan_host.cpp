// Stand-alone runner (tests/test_ntt_plan_host.py builds it with -fsanitize=address,undefined): csrc/ntt_plan.inc's ntt_check_call and
// ntt_plan over the sweep of that test -- log_n 0..28 x batch {1, 2, 3, 48, 65535} x cosets {0, 1, 2, 16} x log_z 0..min(log_n, 12) x the
// forms the C entries make x in place / out of place.  Prints the admitted rows, the refused ones and a checksum of the plans, which the
// test compares with its own through libhm_hostcheck.so; the plan's invariants are asserted here too.
#include <cstddef>
#include <cstdint>
#include <cstdio>

namespace hm {
#include "ntt_plan.inc"
}
using namespace hm;

int main() {
  const uint64_t batches[] = {1, 2, 3, 48, 65535};
  const uint32_t cosets[] = {0, 1, 2, 16};
  const uint32_t forms[] = {0, NTT_F_SCALE, NTT_F_COSET3, NTT_F_SCALE | NTT_F_COSET3, NTT_F_SCALE | NTT_F_POST3, NTT_F_IN_TABLE, NTT_F_IN_TABLES,
                            NTT_F_SCALE | NTT_F_OUT_TABLE, NTT_F_SCALE | NTT_F_OUT_TABLES};
  const uintptr_t out = (1ull << 56) + 0x1000, in = 0x1000;
  uint64_t rows = 0, refused = 0, sum = 0;
  for (uint32_t log_n = 0; log_n <= 28; ++log_n)
    for (uint64_t batch : batches)
      for (uint32_t cs : cosets)
        for (uint32_t fused : forms)
          for (int in_place = 1; in_place >= 0; --in_place) {
            const bool tabled = (fused & (NTT_F_IN_TABLES | NTT_F_OUT_TABLES)) != 0;
            if ((cs != 0) != tabled) continue;
            if ((fused & (NTT_F_OUT_TABLE | NTT_F_OUT_TABLES)) && !in_place) continue;
            const uint32_t z_max = (fused == 0 || fused == NTT_F_COSET3) ? (log_n < 12 ? log_n : 12) : 0;
            for (uint32_t log_z = 0; log_z <= z_max; ++log_z) {
              const NttCall c{log_n, batch, (fused & NTT_F_IN_TABLES) ? cs : 0u, (fused & NTT_F_OUT_TABLES) ? cs : 0u, log_z, fused, in_place != 0, in, out};
              if (ntt_check_call(c)) {
                ++refused;
                continue;
              }
              const NttPlan p = ntt_plan(c);
              const uint64_t n = 1ull << log_n;
              uint64_t counts = 0;
              for (uint32_t i = 0; i < p.tables.n_tables; ++i) counts += p.tables.table[i].count;
              bool ok = p.passes >= 1 && p.passes <= 3 && p.digits[0] + p.digits[1] + p.digits[2] == log_n && p.tables.n_tables <= (uint32_t)NTT_TABLES_MAX &&
                        p.tables.bytes == 36 * counts && p.scratch_bytes == (p.passes > 1 ? n * 32 * p.arrays : 0);
              uint64_t term = p.passes + 3 * p.scratch_bytes + 5 * p.tables.bytes + 29 * p.tail + 31 * p.arrays;
              for (uint32_t i = 0; i < p.passes && ok; ++i) {
                const NttPassPlan& q = p.pass[i];
                const NttPassHead& h = q.head;
                ok = h.s <= (uint32_t)NTT_LOG_TILE && h.s + h.log_c <= (uint32_t)NTT_LOG_TILE && ((uint64_t)q.grid[0] << (h.s + h.log_c)) == n &&
                     q.grid[0] >= 1 && q.grid[0] < (1u << 31) && q.grid[1] >= 1 && q.grid[1] <= 65535 && q.grid[2] >= 1 && q.grid[2] <= 65535 &&
                     q.stage >= 0 && q.stage < (int)p.tables.n_tables && q.tw_lo < (int)p.tables.n_tables && q.tw_hi < (int)p.tables.n_tables &&
                     q.src == (i == 0 ? (in_place ? NTT_BUF_ARRAY : NTT_BUF_INPUT) : NTT_BUF_SCRATCH) &&
                     q.dst == (i + 1 == p.passes ? NTT_BUF_ARRAY : NTT_BUF_SCRATCH) && (h.last || q.tw_lo >= 0) && (h.last || h.direct_tw || q.tw_hi >= 0);
                if (ok) ok = p.tables.table[q.stage].count >= (h.s == 0 ? 1u : 1u << (h.s - 1));
                if (ok && !h.last) {                              // the largest twiddle index of the pass's epilogue lies inside its tables
                  const uint64_t product = ((1ull << h.log_stride) - 1) * ((1ull << h.s) - 1), shift_m = log_n - (h.s + h.log_stride);
                  if (h.direct_tw) ok = product < p.tables.table[q.tw_lo].count && p.tables.table[q.tw_lo].shift == shift_m;
                  else ok = ((product << shift_m) >> h.log_lb) < p.tables.table[q.tw_hi].count && p.tables.table[q.tw_lo].count == (1u << h.log_lb);
                }
                term += 7 * ((uint64_t)q.grid[0] * (i + 1) + q.grid[1] + q.grid[2] + h.log_c + 11 * q.variant + 13 * q.src + 17 * q.dst + 19 * h.direct_tw +
                             23 * (uint64_t)(q.tw_lo + 1));
              }
              if (log_z) ok = ok && p.passes >= 2 && log_z <= p.digits[0];
              if (!ok) return std::printf("invariant broken: log_n %u batch %llu cosets %u fused %u log_z %u in place %d\n", log_n, (unsigned long long)batch,
                                          cs, fused, log_z, in_place), 1;
              ++rows;
              sum += term;
            }
          }
  std::printf("rows %llu refused %llu checksum %llu\n", (unsigned long long)rows, (unsigned long long)refused, (unsigned long long)sum);
  return 0;
}

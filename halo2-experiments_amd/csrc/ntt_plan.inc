// ntt_plan.inc -- the host side of the NTT as pure functions: what a call may ask for, the digits, the scalar parameters, variant, grid
// and buffers of every pass, the scratch bytes and the twiddle tables with their exact byte total.  No kernel, launch, HIP call,
// environment read, static state or heap allocation: ntt.hip's one driver (ntt_run) launches what a plan says, host_check.cpp exports
// the same functions to tests/test_ntt_plan_host.py, which sweeps every shape the C ABI admits.  Included once per unit
// (hm_internal.h; host_check.cpp) inside namespace hm, after <cstddef> and <cstdint>.

// ---- constants the plan shares with the kernels; the macros are measurement knobs (tools/ab_ntt.sh) -------------------------------
#ifndef HM_NTT_LOG_TILE
#define HM_NTT_LOG_TILE 11
#endif
#ifndef HM_NTT_THREADS
#define HM_NTT_THREADS 512
#endif
// Sub-problems up to 2^NTT_DIRECT_LOG get a DIRECT inter-pass twiddle table (omega_m^e for every e < m, 36 B per entry: 75 MB at
// 2^21) instead of two sqrt-sized tables and a forming product per element.  Round 5 (tools/ntt_plans.py, profiles/r05_ntt_plans.txt):
// 16 -> 21 together with the smaller digit first takes 6.7 % of the VALU instructions out of a 2^21 transform (3 328 -> 3 105 lane
// instructions per element) and 4-6 % off every prover-sized shape (48 x 2^21: 11.5 -> 10.9 ms); the table is read as 36-byte
// gathers and the transform stays VALU-bound.  Beyond 2^21 the plan has three passes and only its middle pass can be direct (a direct
// first-pass table is used by two-pass plans only: in a three-pass plan the first pass's m is n but the middle pass's is not).
#ifndef HM_NTT_DIRECT_LOG
#define HM_NTT_DIRECT_LOG 21
#endif
// two passes while both digits fit a tile (measured: 2-8 % faster than three up to 2^21, slower at 2^22 where the 11-bit digit leaves
// single-column, 32-byte accesses)
#ifndef HM_NTT_2PASS_MAX
#define HM_NTT_2PASS_MAX 21
#endif
constexpr int NTT_LOG_TILE = HM_NTT_LOG_TILE;
constexpr int NTT_THREADS = HM_NTT_THREADS;
constexpr uint32_t NTT_DIRECT_LOG = HM_NTT_DIRECT_LOG;
constexpr uint32_t NTT_2PASS_MAX = HM_NTT_2PASS_MAX;
constexpr uint32_t NTT_LOG_N_MAX = 28;       // Fr has 2-adicity 28
constexpr uint32_t NTT_BATCH_MAX = 65535;    // arrays of one launch chain: gridDim.y
constexpr uint32_t NTT_COSETS_MAX = 16;      // coset tables of one launch chain: NttCosetTables, gridDim.z
constexpr uint32_t NTT_TABLE_ENTRY_BYTES = 36;
constexpr int NTT_TABLES_MAX = 6;            // lo, hi, mid and a stage table per pass
static_assert(3 * NTT_LOG_TILE >= (int)NTT_LOG_N_MAX && 2 * NTT_LOG_TILE >= (int)NTT_2PASS_MAX, "three digits of a tile cover every size");

// ---- what one call asks for ---------------------------------------------------------------------------------------------------------
enum : uint32_t {
  NTT_F_SCALE = 1,        // every output *= scale (the ifft divisor)
  NTT_F_COSET3 = 2,       // input element i *= coset[i % 3] (coeff_to_extended)
  NTT_F_POST3 = 4,        // output element i *= post3[i % 3] (extended_to_coeff)
  NTT_F_IN_TABLE = 8,     // input element i *= table[i] / 32, one table for every array (the transform on a coset)
  NTT_F_IN_TABLES = 16,   // ... fwd_cosets tables: every input onto every coset, output array (b, c) = number b * fwd_cosets + c
  NTT_F_OUT_TABLE = 32,   // after the transform, element i *= table[i] / 32, one table for every array (coset_to_coeff)
  NTT_F_OUT_TABLES = 64,  // ... one table per array: inv_cosets arrays (cosets_to_coeff)
  NTT_F_ALL = 127,
};
struct NttCall {
  uint32_t log_n;         // transform size
  uint64_t batch;         // arrays as the entry counts them: the inputs of the forward forms
  uint32_t fwd_cosets;    // NTT_F_IN_TABLES: 0 .. 16 (0: nothing to do)
  uint32_t inv_cosets;    // NTT_F_OUT_TABLES: 0 .. 16 (0: nothing to do)
  uint32_t log_z;         // extending form: the input holds `batch` compact arrays of n >> log_z coefficients (the rest are zero)
  uint32_t fused;         // NTT_F_*
  bool in_place;          // the arrays at `out` are transformed where they are; else `in` is read and `out` written
  uintptr_t in, out;      // device addresses, as far as alignment and overlap need them (in is not read when in_place)
};
// arrays the passes after the first work on, and the output holds
inline uint64_t ntt_call_arrays(const NttCall& c) {
  if (c.fused & NTT_F_IN_TABLES) return c.batch * c.fwd_cosets;
  if (c.fused & NTT_F_OUT_TABLES) return c.batch * c.inv_cosets;
  return c.batch;
}

// ---- the digits -----------------------------------------------------------------------------------------------------------------
// n = R0 * R1 * R2, every digit at most a tile; two passes: the smaller digit first (2^21 = 2^10 x 2^11: the first pass then has two
// columns per tile).  -> passes
inline int ntt_digits(uint32_t log_n, uint32_t digits[3]) {
  digits[0] = digits[1] = digits[2] = 0;
  if (log_n <= (uint32_t)NTT_LOG_TILE) {
    digits[0] = log_n;
    return 1;
  }
  const int passes = log_n <= NTT_2PASS_MAX ? 2 : 3;
  uint32_t rem = log_n;
  for (int p = 0; p < passes; ++p) {
    digits[p] = (rem + (passes - p) - 1) / (passes - p);
    rem -= digits[p];
  }
  if (passes == 2 && digits[0] > digits[1]) { const uint32_t t = digits[0]; digits[0] = digits[1]; digits[1] = t; }
  return passes;
}
// The extending form (the zero part of the padded input is neither read nor written) applies: the first pass's stages 0 .. log_z - 1
// are skipped inside its digit, and a single pass has no scratch to write out of place into.
inline bool ntt_extending_applies(uint32_t log_n, uint32_t log_z) {
  uint32_t digits[3];
  return log_z > 0 && log_n <= NTT_LOG_N_MAX && ntt_digits(log_n, digits) >= 2 && log_z <= digits[0];
}

// ---- every refusal that needs no device, in one order; the C entries prepend their name -------------------------------------------
inline const char* ntt_check_call(const NttCall& c) {
  if (c.log_n > NTT_LOG_N_MAX) return "log_n > 28 (Fr has 2-adicity 28)";
  if (c.log_z > c.log_n) return "the input is longer than the transform (need log_n <= log_ext <= 28)";
  if (c.fwd_cosets > NTT_COSETS_MAX || c.inv_cosets > NTT_COSETS_MAX) return "more than 16 cosets per call";
  if (c.batch > NTT_BATCH_MAX) return "batch > 65535";
  if (ntt_call_arrays(c) > NTT_BATCH_MAX) return "batch * cosets > 65535";
  // shapes no C entry forms
  const uint32_t f = c.fused;
  if (f & ~(uint32_t)NTT_F_ALL) return "unknown fused constant";
  if ((f & NTT_F_IN_TABLE) && (f & NTT_F_IN_TABLES)) return "one input table or several, not both";
  if ((f & NTT_F_OUT_TABLE) && (f & NTT_F_OUT_TABLES)) return "one output table or several, not both";
  if ((f & (NTT_F_IN_TABLE | NTT_F_IN_TABLES)) && (f & (NTT_F_OUT_TABLE | NTT_F_OUT_TABLES))) return "input tables and output tables in one call";
  if ((f & NTT_F_OUT_TABLES) && c.batch > 1) return "the inverse multi-coset form takes one array per coset";
  if (c.log_z != 0 && (c.in_place || (f & (NTT_F_IN_TABLE | NTT_F_IN_TABLES)))) return "the extending form is out of place and has no input table";
  if (c.log_z != 0 && !ntt_extending_applies(c.log_n, c.log_z)) return "the extending form needs a multi-pass plan and log_z <= first digit";
  if (ntt_call_arrays(c) == 0) return nullptr;      // nothing is read or written
  if ((c.out & 15) || (!c.in_place && (c.in & 15))) return "a data pointer is not 16-byte aligned";
  const uint64_t in_bytes = (c.batch << (c.log_n - c.log_z)) * 32, out_bytes = (ntt_call_arrays(c) << c.log_n) * 32;
  if (f & NTT_F_IN_TABLES) {                         // every input is read once per coset: the output may not even be the input
    if (c.in_place || (c.in < c.out + out_bytes && c.out < c.in + in_bytes)) return "the output overlaps the coefficients";
  } else if (!c.in_place && c.log_z == 0 && c.in < c.out + out_bytes && c.out < c.in + in_bytes) {
    return "output partially overlaps the coefficients";   // (the extending form's first pass has read everything before `out` is written)
  }
  return nullptr;
}

// ---- the plan -------------------------------------------------------------------------------------------------------------------
// The scalar head of the pass kernels' parameter block (ntt.hip: NttPassParams = this, then the 54 fused constant words)
struct NttPassHead {
  uint32_t log_n;        // transform size
  uint32_t s;            // log2 of this pass's digit R
  uint32_t log_stride;   // log2 of the element stride between consecutive digit values (non-last passes)
  uint32_t log_c;        // log2 of the columns (non-last) / rows (last) per tile
  uint32_t last;         // 1: stride-1 pass with the digit-reversing, canonicalising store
  uint32_t log_r0;       // last pass of a 3-pass plan: log2 R0 (else 0)
  uint32_t log_rows;     // last pass: log2 of the number of rows = log_n - s
  uint32_t log_lb;       // split point of the two-level inter-pass twiddle table
  uint32_t fin_mode;     // last pass: 0 = canonicalise only, 1 = multiply by fin[0], 2 = output i *= fin[i % 3]
  uint32_t has_coset;    // first pass: multiply a[i] by coset[i % 3] on load
  uint32_t direct_tw;    // non-last pass: tw_lo holds omega_m^e for every e < m (no forming product)
  uint32_t log_z;        // first pass of an extending transform: the input holds only the first n >> log_z
                         // coefficients (the rest are zero by definition); 0 = ordinary transform
  uint32_t has_table;    // first pass: multiply a[i] by in_scale[i] on load (the transform on a coset shift * <omega>: in_scale
                         // holds 32 * shift^i as external words, so that the product of two external words is the external
                         // word of a[i] * shift^i -- the radix is 2^261)
};
enum NttVariant : uint32_t { NTT_PLAIN = 0, NTT_FUSED = 1, NTT_TABLE = 2 };        // ntt_pass_kernel<.., FUSED, TABLE>
enum NttBuffer : uint32_t { NTT_BUF_INPUT = 0, NTT_BUF_ARRAY = 1, NTT_BUF_SCRATCH = 2 };
enum NttTail : uint32_t { NTT_TAIL_NONE = 0, NTT_TAIL_TABLE = 1, NTT_TAIL_TABLES = 2 };   // fr_mul_table_kernel / fr_mul_tables_kernel
enum NttTableRole : uint32_t { NTT_TW_LO = 0, NTT_TW_HI = 1, NTT_TW_MID = 2, NTT_TW_STAGE = 3 };
// table[j] = omega^(j << shift), j < count
struct NttTableSpec {
  uint32_t role, count, shift;
};
struct NttTableSet {
  uint32_t n_tables;
  NttTableSpec table[NTT_TABLES_MAX];
  uint64_t bytes;              // NTT_TABLE_ENTRY_BYTES x the sum of the counts
  int8_t lo, hi, mid;          // index of the role's table, -1: the plan has none
  int8_t stage[3];             // ... of every pass's stage table
};
struct NttPassPlan {
  NttPassHead head;
  uint32_t variant;            // NttVariant
  uint32_t grid[3];
  uint32_t src, dst;           // NttBuffer
  int8_t stage, tw_lo, tw_hi;  // indices into the table set; -1: a null pointer (the pass does not read it)
};
struct NttPlan {
  uint32_t passes;             // 0: nothing to do
  uint32_t digits[3];
  uint64_t arrays;
  uint32_t lds_bytes;
  uint64_t scratch_bytes;      // the ping-pong buffer: n x 32 x arrays with more than one pass, else none
  NttPassPlan pass[3];
  uint32_t tail, tail_grid[2]; // the inverse coset forms' table product, 256 lanes per block
  NttTableSet tables;
};

// The twiddle tables of a size: omega_n^e for every e < n when a two-pass plan's first pass reads them directly, else lo / hi with the
// forming product, and the middle pass's direct table while it fits; then omega_R^j, j < R / 2, per distinct digit.
inline NttTableSet ntt_table_set(uint32_t log_n) {
  NttTableSet t{};
  t.lo = t.hi = t.mid = -1;
  uint32_t digits[3];
  const int passes = ntt_digits(log_n, digits);
  auto add = [&](uint32_t role, uint32_t count, uint32_t shift) -> int8_t {
    t.table[t.n_tables] = NttTableSpec{role, count, shift};
    t.bytes += (uint64_t)count * NTT_TABLE_ENTRY_BYTES;
    return (int8_t)t.n_tables++;
  };
  if (passes == 2 && log_n <= NTT_DIRECT_LOG) {
    t.lo = add(NTT_TW_LO, 1u << log_n, 0);
  } else if (passes > 1) {
    const uint32_t log_lb = (log_n + 1) / 2, log_m1 = log_n - digits[0];       // log_m1: size of the middle pass's sub-problem
    t.lo = add(NTT_TW_LO, 1u << log_lb, 0);
    t.hi = add(NTT_TW_HI, 1u << (log_n - log_lb), log_lb);
    if (passes == 3 && log_m1 <= NTT_DIRECT_LOG) t.mid = add(NTT_TW_MID, 1u << log_m1, digits[0]);   // omega_m1^e = omega_n^(e << s0)
  }
  for (int p = 0; p < 3; ++p) {
    t.stage[p] = -1;
    if (p >= passes) continue;
    for (int q = 0; q < p; ++q)
      if (digits[q] == digits[p]) t.stage[p] = t.stage[q];
    if (t.stage[p] < 0) t.stage[p] = add(NTT_TW_STAGE, digits[p] == 0 ? 1u : 1u << (digits[p] - 1), log_n - digits[p]);
  }
  return t;
}

// The launch plan of an ADMITTED call (ntt_check_call).
inline NttPlan ntt_plan(const NttCall& c) {
  NttPlan pl{};
  pl.arrays = ntt_call_arrays(c);
  if (pl.arrays == 0) return pl;
  pl.passes = (uint32_t)ntt_digits(c.log_n, pl.digits);
  pl.tables = ntt_table_set(c.log_n);
  pl.lds_bytes = (uint32_t)(9 * sizeof(uint32_t)) << NTT_LOG_TILE;
  pl.scratch_bytes = pl.passes > 1 ? (pl.arrays << c.log_n) * 32 : 0;
  const bool tabled = (c.fused & (NTT_F_IN_TABLE | NTT_F_IN_TABLES)) != 0;
  const uint32_t fin_mode = (c.fused & NTT_F_POST3) ? 2u : (c.fused & NTT_F_SCALE) ? 1u : 0u;
  uint32_t log_stride = c.log_n;
  for (uint32_t p = 0; p < pl.passes; ++p) {
    NttPassPlan& pp = pl.pass[p];
    NttPassHead& h = pp.head;
    h.log_n = c.log_n;
    h.s = pl.digits[p];
    log_stride -= h.s;
    h.log_stride = log_stride;
    h.last = p == pl.passes - 1 ? 1u : 0u;
    h.log_lb = (c.log_n + 1) / 2;
    h.log_rows = c.log_n - h.s;
    h.log_r0 = (h.last && pl.passes == 3) ? pl.digits[0] : 0u;
    h.fin_mode = h.last ? fin_mode : 0u;
    h.has_coset = (p == 0 && (c.fused & NTT_F_COSET3)) ? 1u : 0u;
    h.log_z = p == 0 ? c.log_z : 0u;
    h.has_table = (p == 0 && tabled) ? 1u : 0u;
    const uint32_t avail = h.last ? h.log_rows : h.log_stride;       // columns / rows that exist
    h.log_c = (uint32_t)NTT_LOG_TILE > h.s ? (uint32_t)NTT_LOG_TILE - h.s : 0u;
    if (h.log_c > avail) h.log_c = avail;
    pp.stage = pl.tables.stage[p];
    pp.tw_lo = pl.tables.lo;
    pp.tw_hi = pl.tables.hi;
    if (!h.last) {
      if (pl.tables.hi < 0) {
        h.direct_tw = 1;             // lo = omega_n^e; omega_m^e = omega_n^(e << (log_n - log_m)) only for p == 0 (m = n)
      } else if (p == 1 && pl.tables.mid >= 0) {
        h.direct_tw = 1;
        pp.tw_lo = pl.tables.mid;
      }
    }
    pp.variant = h.has_table ? NTT_TABLE : (h.has_coset | h.fin_mode) ? NTT_FUSED : NTT_PLAIN;
    pp.grid[0] = (uint32_t)((1ull << c.log_n) >> (h.s + h.log_c));   // tiles
    // the table variant's first pass reads `batch` inputs and writes batch * cosets arrays (blockIdx.z = the coset)
    pp.grid[1] = (uint32_t)(h.has_table ? c.batch : pl.arrays);
    pp.grid[2] = (h.has_table && (c.fused & NTT_F_IN_TABLES)) ? c.fwd_cosets : 1u;
    pp.src = p == 0 ? (c.in_place ? NTT_BUF_ARRAY : NTT_BUF_INPUT) : NTT_BUF_SCRATCH;
    pp.dst = h.last ? NTT_BUF_ARRAY : NTT_BUF_SCRATCH;
  }
  pl.tail = (c.fused & NTT_F_OUT_TABLES) ? NTT_TAIL_TABLES : (c.fused & NTT_F_OUT_TABLE) ? NTT_TAIL_TABLE : NTT_TAIL_NONE;
  if (pl.tail) {
    pl.tail_grid[0] = (uint32_t)(((1ull << c.log_n) + 255) / 256);
    pl.tail_grid[1] = (uint32_t)pl.arrays;
  }
  return pl;
}

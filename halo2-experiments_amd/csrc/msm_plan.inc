// msm_plan.inc -- the host side of the MSM as pure functions: which window, which kernel variant of every stage, every grid and
// dynamic LDS size, and the workspace as a table of regions.  No kernel, launch, HIP call, environment read, atomic or static state:
// msm.hip and msm_small.hip launch what a plan says, host_check.cpp exports the same functions to tests/test_msm_plan_host.py, which
// sweeps every input the C ABI accepts.  Included once per unit (msm_dev.h; host_check.cpp) inside namespace hm, after <algorithm>,
// <cmath>, <cstddef> and <cstdint>.

// ---- constants the plan shares with the kernels ---------------------------------------------------------------------
constexpr int PT_WORDS = 28;  // device Jacobian record: 27 limbs + identity flag
constexpr int ACC_THREADS = 64;
constexpr int WIN_THREADS = 256;
constexpr int WAVE_THREADS = 64;
constexpr int MSM_GROUP_MAX = 8;      // == HM_MSM_GROUP (hm_internal.h): scalar arrays one launch chain carries
#ifndef HM_TARGET_TASKS      // measurement knob (tools/ab_build.sh)
#define HM_TARGET_TASKS 327680
#endif
constexpr uint32_t TARGET_TASKS = HM_TARGET_TASKS;   // 256 CUs x 4 SIMDs x 5 waves x 64 lanes
constexpr int DIGITS_THREADS = 256;
constexpr int DIGITS_COUNT_THREADS = 1024;
#ifndef HM_SORT_THREADS
#define HM_SORT_THREADS 1024
#endif
constexpr int SORT_THREADS = HM_SORT_THREADS;
#ifndef HM_P1_IPT
#define HM_P1_IPT 4
#endif
constexpr int P1_IPT_DEFAULT = HM_P1_IPT;
#ifndef HM_P1_BIG_IPT        // tiles for 512 .. 2048 coarse bins (the shared-bucket-set plan, the plain layout from 2^21 points).
#define HM_P1_BIG_IPT 16     // Measured at 2^24 on the table, whole sort: 8 items per lane 3.19 ms, 16 (with part 2's 16) 3.00 ms --
#endif                       // 16 items = a 64-byte run per coarse bin and tile instead of 32 (140 KiB of LDS, one workgroup per CU)
constexpr int P1_BIG_IPT = HM_P1_BIG_IPT;
#ifndef HM_P2_IPT
#define HM_P2_IPT 16         // 16 384-item tiles (8: +0.06 ms, 4: +0.35 ms of sort at 2^24)
#endif
constexpr int P2_IPT = HM_P2_IPT;
constexpr int P2_TILE = SORT_THREADS * P2_IPT;
constexpr uint32_t PS_MAX_SC = 1024;                // super-chunks of a positional plan (their boundaries live in LDS)
constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS = 8;                       // items per lane; a block covers 2048 buckets
constexpr int SCAN_BLOCK = SCAN_THREADS * SCAN_ITEMS;
constexpr uint32_t TASK_KEYS = 1024;
constexpr int ORDER_THREADS = 1024;   // == TASK_KEYS: one LDS counter per lane
constexpr int ORDER_ITEMS = 4;        // buckets per lane
constexpr uint32_t FINALIZE_SERIAL = 8;
constexpr uint32_t FINALIZE_SLICE = 2048;   // partials one workgroup sums in the first level of a very hot bucket
#ifndef HM_SUM_PER_LANE
#define HM_SUM_PER_LANE 4     // measured: 4 beats 16 by 0.06-0.07 ms at every size (more workgroups, shorter serial sums)
#endif
constexpr uint32_t SUM_SPAN = WIN_THREADS * HM_SUM_PER_LANE;
// msm_small.hip
constexpr int SA_THREADS = 256;       // A: one lane per scalar
constexpr int SS_THREADS = 1024;      // B: one workgroup per (window, bucket range)
constexpr uint32_t S_TASK_KEYS = 1024;
constexpr uint32_t S_MAX_L = 1023;
// hipFuncAttributeMaxDynamicSharedMemorySize of the sort kernels: the default, what the LDS-histogram kernels are given, and what
// a workgroup may ask for dynamically beside the vector-load kernels' static tables
constexpr uint32_t MSM_LDS_DEFAULT = 64 * 1024;
constexpr uint32_t MSM_LDS_FINE = 32768 * 4;
constexpr uint32_t MSM_LDS_ALL = 160 * 1024 - 6 * 1024;
constexpr uint32_t MSM_S_LDS_SORT = (uint32_t)(((size_t)16416 + 2 * S_TASK_KEYS + 32) * 4);   // msm_s_sort_kernel

// plan errors carry the C ABI's codes (include/halo2_mi355x.h)
constexpr int MSM_PLAN_OK = 0, MSM_PLAN_BAD_ARG = -1, MSM_PLAN_INTERNAL = -5;

// ---- knobs ----------------------------------------------------------------------------------------------------------
// What a call may be told from outside: hm_msm_set_window and the three switches the tests use as their reference arm
// (-1 = unset, else 0 / 1).  msm.hip fills one per call (msm_read_knobs).
struct MsmKnobs {
  int window_override = 0;
  int digits_count = -1;    // HALO2_MI355X_DIGITS_COUNT: 0 = the separate histogram pass, 1 = the counting form wherever it is valid
  int k3b_copy = -1;        // HALO2_MI355X_K3B_COPY=1: msm_bucket_finalize_kernel writes every bucket and the reduction reads only those
  int k4_wave_sums = -1;    // HALO2_MI355X_K4_WAVE_SUMS: 0 = the workgroup form of the row / column sums, 1 = the one-wave form
};

static inline uint32_t ilog2(size_t n) {
  uint32_t l = 0;
  while ((n >> (l + 1)) != 0) ++l;
  return l;
}

// ---- windows ----------------------------------------------------------------------------------------------------------
// The 255 digit bits over W windows as evenly as possible: windows [0, n_wide) are `wide` bits, the others wide - 1.
// (W - 1 full windows and a short top one would send every point's top digit into the lowest 2^(short - 1) buckets:
// at 2^24 points, c = 22, 4 096 buckets with 4 192 points each beside a mean of 96.)
static inline void balanced_windows(uint32_t W, uint32_t* wide, uint32_t* n_wide) {
  const uint32_t base = 255 / W, rest = 255 - base * W;
  *wide = rest ? base + 1 : base;
  *n_wide = rest ? rest : W;
}

// Window size for a precomputed (single bucket set) base set of n points: minimise
// n * W(c) mixed additions + ~3 * 2^(c-1) addition-equivalents of bucket reduction.
static inline uint32_t plan_precomp_window(size_t n) {
  uint32_t best = 8;
  double best_cost = 1e300;
  // (capped at 22: the model knows additions only.  Measured at 2^25 / 2^26, c = 24 against 22: K3 26.6 / 51.4 against
  // 28.6 / 56.0 ms, but the sort 8.8 / 16.6 against 6.0 / 12.0 -- 2^23 buckets need 4 096 coarse bins, two items per bin
  // and first-level tile -- and the bucket reduction 2.8 against 1.3: whole MSM 39.2 / 72.2 against 36.5 / 70.5 ms)
  for (uint32_t c = 8; c <= 22; ++c) {
    const double W = (double)((255 + c - 1) / c);
    const double cost = (double)n * W + 3.0 * (double)(1ull << (c - 1));
    if (cost < best_cost) { best_cost = cost; best = c; }
  }
  uint32_t wide, n_wide;
  balanced_windows((255 + best - 1) / best, &wide, &n_wide);     // the widest window of the balanced split (<= best)
  return wide;
}

// the five-launch chain of msm_small.hip: n < 2^19 on a plain base set, c <= 15
static inline bool plan_small_applies(size_t n, uint32_t c, bool single_set) {
  return !single_set && n >= 1 && n < (1u << 19) && c >= 2 && c <= 15;
}

// THE place that picks c.  A table set carries its window (precomp_c); an override wins over the tables.  `live_rows` (0 = unknown):
// an upper bound on the rows that survive the digits kernel's compaction -- the window of the five-launch chain is picked for
// THOSE (an advice column with 1 100 used rows of 2^18 is a 2^10-point MSM: c = 7, not 15: its buckets are then dense, and the
// reduction's per-bucket scalar multiple has 7 bits instead of 14).
static inline uint32_t msm_window(size_t n, uint32_t precomp_c, size_t live_rows, const MsmKnobs& k) {
  if (precomp_c != 0) return precomp_c;
  if (k.window_override > 0) return (uint32_t)k.window_override;
  // Rule of thumb: log2(n) - 3 (mean bucket load ~16: short chains, almost no bucket splitting, few
  // (point, bucket) pairs), capped at c = 17, whose W = 15 windows cover the 255 digit bits exactly
  // (18, 19 and 21 leave a top window of 3-8 bits whose few buckets receive all n points, and c = 20's
  // 6.8 M buckets cost more to reduce than they save).  The table is the measured optimum per size
  // (tools/msm_sweep.py <k> <c,c,...>): between 2^15 and 2^17 the fixed costs of the sort and of the
  // bucket reduction move it up to c = 15.
  static const int8_t kWindow[21] = {4, 4, 4, 4, 4, 4, 4, 4, 5, 6, 7, 8, 9, 10, 10, 13, 15, 15, 15, 16, 17};
  // the short chain of msm_small.hip (n < 2^19) has cheaper fixed costs per bucket set: its measured optimum is
  // log2(n) - 3 up to 2^16, then c = 15, whose 17 windows cover the 255 bits exactly
  static const int8_t kWindowSmall[19] = {4, 4, 4, 4, 4, 4, 4, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15, 15};
  const uint32_t lg = ilog2(n);
  if (lg <= 18 && plan_small_applies(n, (uint32_t)kWindowSmall[lg], false)) {
    const size_t sized_for = live_rows != 0 && live_rows < n ? live_rows : n;
    return (uint32_t)kWindowSmall[ilog2(sized_for)];
  }
  return (uint32_t)(lg <= 20 ? kWindow[lg] : 17);
}

// The window of the five-launch chain for n points, or 0 when it does not apply (n >= 2^19, a precomputed set, an override
// outside its range): the same choice msm_plan makes for a single MSM.
static inline uint32_t plan_small_window(size_t n, uint32_t precomp_c, size_t live_rows, const MsmKnobs& k) {
  if (precomp_c != 0 || n == 0 || n >= (1u << 19)) return 0;
  const uint32_t c = msm_window(n, 0, live_rows, k);
  return plan_small_applies(n, c, false) ? c : 0;
}

// Several DENSE commitments over one fixed-base table in one chain of the general pipeline: every element is a bucket set
// of the same sort launches, the same K3 launch and the same two reduction launches (at most 8; 1 = a chain each).  Applies where
// a single such MSM runs the general pipeline on the table (not the five-launch plan) and the whole chain's (point, bucket) pairs
// stay below 2^31.
static inline uint32_t plan_table_group_max(size_t n, uint32_t precomp_c) {
  // (from 2^19 points a commitment fills the chip by itself, and the positional sort plan of the larger sizes has only been
  //  exercised one bucket set at a time)
  if (precomp_c < 6 || n == 0 || n >= ((size_t)1 << 19) || plan_small_applies(n, precomp_c, true)) return 1;
  const uint64_t per = (uint64_t)n * ((255 + precomp_c - 1) / precomp_c);
  uint32_t g = MSM_GROUP_MAX;
  while (g > 1 && per * g >= (1ull << 31)) --g;
  while (g > 1 && per * g * 4 > ((uint64_t)3 << 30)) --g;       // keep a chain's item arrays below 3 GiB each
  return g;
}

// ---- the general pipeline (msm.hip) -----------------------------------------------------------------------------------
enum MsmRoute : uint32_t { MSM_ROUTE_EMPTY, MSM_ROUTE_SMALL, MSM_ROUTE_GENERAL };   // n == 0; msm_small.hip; msm.hip
// the kernel variant of every stage, decided once
enum MsmDigits : uint32_t { MSM_DIGITS_PLAIN, MSM_DIGITS_COUNTING };
enum MsmFirstLevel : uint32_t { MSM_P1_NONE, MSM_P1_HIST, MSM_P1_COUNTED };         // no first level; its counts from the histogram pass / the digits pass
enum MsmP1Scatter : uint32_t { MSM_P1S_NONE, MSM_P1S_VEC, MSM_P1S_VEC_BIG, MSM_P1S_TILED, MSM_P1S_DIRECT };
enum MsmP2Scatter : uint32_t { MSM_P2S_DIGITS, MSM_P2S_DIRECT, MSM_P2S_TILED, MSM_P2S_VEC };
enum MsmItem : uint32_t { MSM_ITEM_U32, MSM_ITEM_U32_POSITIONAL, MSM_ITEM_U64 };
enum MsmTasks : uint32_t { MSM_TASKS_FILL, MSM_TASKS_ORDERED };
enum MsmReduction : uint32_t { MSM_RED_CHAIN, MSM_RED_ROWCOL, MSM_RED_ROWCOL_WAVE };

enum MsmRegion : uint32_t {
  MR_DIGITS, MR_CHIST, MR_CTOT, MR_CSTART, MR_TMP, MR_BCNT, MR_BOFF, MR_TOFF, MR_BSUM, MR_SORTED, MR_TB, MR_TORDER, MR_TKEYS,
  MR_PARTIAL, MR_BUCKET, MR_SEG, MR_SEG2, MR_RES, MR_BIG, MR_SLICES, MR_BRLIST, MR_BRCOUNT, MR_GCUR, MR_COUNT
};
struct MsmSpan { size_t off, bytes; };
struct MsmCarver {          // carves 256-byte aligned regions one after the other
  size_t off = 0;
  MsmSpan carve(size_t bytes) {
    const MsmSpan s{off, bytes};
    off += (bytes + 255) & ~(size_t)255;
    return s;
  }
};

enum MsmLaunchId : uint32_t {
  ML_DIGITS, ML_INIT, ML_P1_HIST, ML_P1_SCAN, ML_P1_STARTS, ML_P1_SCATTER, ML_BIG_REGIONS, ML_P2_HIST, ML_P2_HIST_COOP,
  ML_SCAN_PARTIAL, ML_SCAN_BLOCKSUMS, ML_SCAN_FINAL, ML_P2_SCATTER, ML_P2_SCATTER_COOP, ML_TASK_FILL, ML_TASK_HIST, ML_TASK_KEYSCAN,
  ML_TASK_ORDER, ML_ACCUMULATE, ML_FINALIZE, ML_FINALIZE_SLICES, ML_FINALIZE_BIG, ML_ROWCOL, ML_BITS, ML_SEGMENTS, ML_SUM_0,
  ML_SUM_1, ML_TO_EXT, ML_COUNT
};
struct MsmLaunch { uint32_t gx = 0, gy = 1, block = 0, lds = 0, lds_cap = MSM_LDS_DEFAULT, gz = 1; };   // gx == 0: not made

struct MsmPlan {
  int err = MSM_PLAN_OK;
  const char* err_msg = nullptr;
  MsmRoute route = MSM_ROUTE_EMPTY;
  bool single_set = false;     // all windows accumulate into ONE bucket set (a fixed-base table)
  uint32_t group = 1, c = 0, W = 0, n_wide = 0;
  uint32_t SW = 0;             // bucket sets ("sort windows"): one per MSM on a table, one per window else
  size_t sn = 0;               // items per bucket set
  uint32_t NB = 0, NBP = 0, NBT = 0;
  uint64_t pairs_max = 0;      // of the whole chain
  uint32_t L = 0, G = 0;
  size_t chunk = 0;
  uint64_t T_max = 0;
  uint32_t SEG = 0, nseg = 0, k4_m = 0, k4_h = 0, RW = 0, res_stride = 0;
  uint32_t ib = 0, fb = 0, cb = 0, NC = 0;
  uint32_t ps_G = 0, ps_gpc = 0, ps_nsc = 0, sbits = 0;    // the positional plan (ps_nsc == 0: items carry their whole index)
  uint32_t br_big = 0, br_slice = 0, br_capacity = 0;      // cooperative handling of oversized sort regions
  bool coop_sort = false, direct_buckets = false;
  MsmDigits digits = MSM_DIGITS_PLAIN;
  MsmFirstLevel first_level = MSM_P1_NONE;
  MsmP1Scatter p1_scatter = MSM_P1S_NONE;
  MsmP2Scatter p2_scatter = MSM_P2S_DIGITS;
  MsmItem item = MSM_ITEM_U32;
  MsmTasks tasks = MSM_TASKS_FILL;
  MsmReduction reduction = MSM_RED_CHAIN;
  uint32_t sum_levels = 0, sum_count[2] = {0, 0};          // msm_sum_points_kernel passes of the chain reduction: inputs of each
  MsmSpan region[MR_COUNT] = {};
  size_t ws_bytes = 0;
  MsmLaunch launch[ML_COUNT];
};

template <class Plan>
static inline Plan msm_plan_fail(Plan p, int err, const char* msg) {
  p.err = err, p.err_msg = msg;
  return p;
}

// The plan of `group` MSMs over the same n points in ONE launch chain (group > 1: only on a fixed-base table set below the
// positional plan's sizes -- plan_table_group_max -- where every element is one bucket set of the same sort and the same K3 launch).
static inline MsmPlan msm_plan(size_t n, uint32_t group, uint32_t precomp_c, const MsmKnobs& knobs) {
  MsmPlan p;
  p.group = group;
  if (n == 0) return p;
  if (n >= (1ull << 31)) return msm_plan_fail(p, MSM_PLAN_BAD_ARG, "msm: n must be < 2^31");
  if (group == 0 || group > (uint32_t)MSM_GROUP_MAX) return msm_plan_fail(p, MSM_PLAN_INTERNAL, "msm: group size out of range");
  const bool single_set = p.single_set = precomp_c != 0;
  const uint32_t c = p.c = msm_window(n, precomp_c, 0, knobs);
  if (c < 2 || c > 24) return msm_plan_fail(p, MSM_PLAN_BAD_ARG, "msm: window size out of range");
  if (plan_small_applies(n, c, single_set)) {
    if (group != 1) return msm_plan_fail(p, MSM_PLAN_INTERNAL, "msm: a table group reached the five-launch plan");
    p.route = MSM_ROUTE_SMALL;
    return p;
  }
  p.route = MSM_ROUTE_GENERAL;
  if (group > 1 && !single_set) return msm_plan_fail(p, MSM_PLAN_INTERNAL, "msm: a group needs the fixed-base table's shared bucket set");
  const uint32_t W = p.W = (255 + c - 1) / c;
  const uint32_t SW = p.SW = single_set ? group : W;
  const size_t sn = p.sn = single_set ? n * W : n;
  const uint32_t NB = p.NB = 1u << (c - 1), NBP = p.NBP = NB + 1, NBT = p.NBT = SW * NBP;
  const uint64_t pairs_max = p.pairs_max = (uint64_t)n * W * group;
  if (pairs_max >= (1ull << 31)) return msm_plan_fail(p, MSM_PLAN_BAD_ARG, "msm: n * windows must be < 2^31");
  double mean = (double)sn / (double)NB;
  p.n_wide = W;                                              // a shared bucket set: the balanced split its table was built for
  if (single_set) {
    // narrow windows fill the even buckets only (msm_digits_kernel): size the tasks for THOSE buckets' load, so that a
    // bucket stays one task (at c = 22, W = 12: 168 points in an even bucket, 24 in an odd one, 96 on average)
    uint32_t wide_b, n_wide_b;
    balanced_windows(W, &wide_b, &n_wide_b);
    mean = (double)n * n_wide_b / (double)NB + (double)n * (W - n_wide_b) / ((double)NB / 2.0);
    p.n_wide = n_wide_b;
    if (wide_b != c) return msm_plan_fail(p, MSM_PLAN_INTERNAL, "msm: the base set's table was built for another window split");
  }
  uint32_t L = (uint32_t)(mean + 4.0 * std::sqrt(mean) + 8.0);     // the mean load and four standard deviations
  {
    // small inputs: if one task per bucket would leave the chip (256 CUs x 4 SIMDs x ~5 waves x 64
    // lanes) mostly idle, cut the tasks shorter so that the launch still fills it (measured: a wave per
    // SIMD is not enough -- K3 at 2^16..2^18 is 15-40 % slower with one task per bucket)
    const double target_tasks = (double)TARGET_TASKS;
    if ((double)pairs_max / (double)L < target_tasks) L = (uint32_t)((double)pairs_max / target_tasks);
  }
  if (L < 16) L = 16;
  p.L = L;
  // chunks of the first sort level: >= 16 Ki items each, ~64 Ki at scale; G * SW workgroups should
  // cover the chip several times over (a shared bucket set has SW = 1, so it needs many chunks)
  uint32_t G = (uint32_t)((sn + 16383) / 16384);
  const uint32_t g_cap = SW >= 8 ? 256u : 4096u;
  if (G > g_cap) {
    G = (uint32_t)((sn + 65535) / 65536);
    if (G > g_cap) G = g_cap;
    if (G < 256) G = 256;
  }
  size_t chunk = (sn + G - 1) / G;
  // the device may shorten L (effective_task_len): then tasks <= 2 * TARGET_TASKS + one per bucket
  // (and never more than one per pair)
  const uint64_t T_max = p.T_max = std::min<uint64_t>(pairs_max, std::max<uint64_t>(pairs_max / L, 2ull * TARGET_TASKS) + NBT) + 1;
  // K4a: running-sum chain of 2*SEG additions per lane + a scalar multiple of <= log2(NB) bits
  // Segment length of K4a, measured per bucket count (the kernel is latency-bound: a lane's chain is
  // 2*SEG additions plus a log2(NB/SEG)-bit multiple, and the number of lanes decides how well the chip hides it)
  uint32_t SEG = NB > (1u << 16) ? 32u : NB == (1u << 15) ? 16u : NB <= (1u << 13) ? 4u : 8u;
  if (SEG > NB) SEG = NB;
  p.SEG = SEG;
  const uint32_t nseg = p.nseg = (NB + SEG - 1) / SEG;
  // a shared bucket set: row / column sums and one record per weight bit instead (msm_reduce_rowcol_kernel)
  const bool k4_2d = single_set && NB >= 16;
  const uint32_t k4_m = p.k4_m = (c - 1 + 1) / 2, k4_h = p.k4_h = (c - 1) - k4_m;        // M = 2^m columns, H = 2^h rows, M * H = NB
  if (group > 1 && !k4_2d) return msm_plan_fail(p, MSM_PLAN_INTERNAL, "msm: a table group needs the two-launch bucket reduction");
  // The reduction reads one-task buckets from their partials (load_bucket_value) unless k3b_copy asks for the copy pass; the
  // one-wave form of the row / column sums where its H + M / 2 waves give each of the chip's 1 024 SIMDs two (c >= 22; below,
  // the wide trees' shorter critical path wins), or as k4_wave_sums says.
  bool direct_buckets = false, wave_sums = false;
  if (k4_2d) {
    direct_buckets = !(knobs.k3b_copy == 1);
    wave_sums = knobs.k4_wave_sums >= 0 ? knobs.k4_wave_sums == 1 : ((1u << k4_h) + (1u << (k4_m - 1))) * SW >= 2048u;
  }
  p.direct_buckets = direct_buckets;
  p.reduction = !k4_2d ? MSM_RED_CHAIN : wave_sums ? MSM_RED_ROWCOL_WAVE : MSM_RED_ROWCOL;
  const uint32_t RW = p.RW = k4_2d ? c - 1 : SW;                               // records the host fold reads (per bucket set of a table)
  const uint32_t res_stride = p.res_stride = 4 + RW * 32;                      // words per element of a group: the totals, then its records
  // sort plan: item = [fine bucket bits | sign | item index]
  uint32_t ib = ilog2(sn) + ((sn & (sn - 1)) ? 1u : 0u);
  if (ib == 0) ib = 1;
  bool wide_items = false;
  uint32_t fb = c - 1 < 31 - ib ? c - 1 : 31 - ib;
  if (fb > 15) fb = 15;                  // 2^15 LDS counters = 128 KiB is what a workgroup may hold
  if (single_set && c >= 14 && c <= 24 && (c - 1) - fb > 10) {
    // POSITIONAL 32-bit items (msm.hip, above `struct Positional`): an item keeps the low `sbits` bits of its index; chunks of the
    // first level are 2^16 (or more) consecutive indices, so every chunk lies inside one super-chunk of 2^sbits.
    for (uint32_t cb_try = 9; cb_try <= 12 && p.ps_nsc == 0; ++cb_try) {   // 9 against 10: sort 0.69 / 0.74 ms at 2^22 (c = 20), the same at c = 22; 8 is slower
      if (c - 1 < cb_try + 5) break;
      const uint32_t fb_p = c - 1 - cb_try, sbits = 31 - fb_p;
      if (fb_p > 12 || sbits < 16) continue;                   // the tiled second level holds <= 2^12 fine counters
      size_t chunk_p = (size_t)1 << 16;
      while ((sn + chunk_p - 1) / chunk_p > 4096 && chunk_p < ((size_t)1 << sbits)) chunk_p <<= 1;
      const size_t nsc = (sn + ((size_t)1 << sbits) - 1) >> sbits;
      if (nsc > PS_MAX_SC || (sn + chunk_p - 1) / chunk_p > 4096) continue;
      ib = sbits;
      fb = fb_p;
      G = (uint32_t)((sn + chunk_p - 1) / chunk_p);
      chunk = chunk_p;
      p.ps_G = G;
      p.ps_gpc = (uint32_t)(((size_t)1 << sbits) / chunk_p);
      p.ps_nsc = (uint32_t)nsc;
      p.sbits = sbits;
    }
  }
  if (p.ps_nsc == 0 && fb < 5 && c - 1 > fb) {   // too few fine bits left in 32: switch to 64-bit items
    wide_items = true;
    fb = c - 1 < 9 ? c - 1 : 9;      // few fine runs per region: the region's write sectors must stay in L2
  }
  if (p.ps_nsc == 0 && sn >= (1u << 15) && (c - 1) - fb < 5) fb = c - 1 > 5 ? c - 1 - 5 : 0;   // >= 32 regions per set: enough workgroups
  const uint32_t cb = (c - 1) - fb, NC = 1u << cb;
  p.ib = ib, p.fb = fb, p.cb = cb, p.NC = NC, p.G = G, p.chunk = chunk;
  p.item = wide_items ? MSM_ITEM_U64 : p.ps_nsc != 0 ? MSM_ITEM_U32_POSITIONAL : MSM_ITEM_U32;
  // Coarse-bin counts from the digits pass (msm_digits_kernel<true>): a shared bucket set with a first sort level whose
  // chunks each lie inside one window, 32-bit items, the vector-load sort -- and a workgroup per chunk of points for every
  // one of the chip's 256 CUs (2^24 points): the form has n / chunk workgroups, and below that it loses more in the digits
  // kernel than the histogram pass costs (2^20 points, 16 workgroups: 0.37 against 0.03 ms).  digits_count: 0 = the separate
  // histogram pass, 1 = the counting form wherever it is valid (A/B and tests).
  bool digits_count = false;
  if (single_set && cb != 0 && !wide_items && n % chunk == 0 && (size_t)G * chunk == sn && (size_t)W * NC * 4 <= 48 * 1024)
    digits_count = knobs.digits_count >= 0 ? knobs.digits_count == 1 : (n / chunk) * group >= 256;
  p.digits = digits_count ? MSM_DIGITS_COUNTING : MSM_DIGITS_PLAIN;
  p.first_level = !cb ? MSM_P1_NONE : digits_count ? MSM_P1_COUNTED : MSM_P1_HIST;
  p.tasks = pairs_max < (1u << 19) ? MSM_TASKS_FILL : MSM_TASKS_ORDERED;   // small inputs: three more launches cost more than the idle lanes they would save

  // cooperative sort of oversized regions (hot buckets): split anything above 4x the mean region
  const uint64_t mean_region = pairs_max / ((uint64_t)NC * SW) + 1;
  const uint64_t slice = std::max<uint64_t>((mean_region + P2_TILE - 1) / P2_TILE * P2_TILE, 4 * (uint64_t)P2_TILE);
  p.br_slice = (uint32_t)slice;
  p.br_big = (uint32_t)(4 * slice);
  p.br_capacity = (uint32_t)(pairs_max / slice + pairs_max / p.br_big + 2);
  const bool coop_sort = p.coop_sort = cb != 0 && (fb <= 11 || (p.ps_nsc != 0 && fb <= 12));   // 2^12 fine counters only where the positional plan asks for them

  // ---- workspace ----------------------------------------------------------------------------
  MsmCarver cv;
  p.region[MR_DIGITS] = cv.carve((size_t)W * n * 4 * group);
  p.region[MR_CHIST] = cv.carve((size_t)SW * G * NC * 4);
  p.region[MR_CTOT] = cv.carve((size_t)SW * NC * 4);
  p.region[MR_CSTART] = cv.carve(((size_t)SW * NC + 1) * 4);
  p.region[MR_TMP] = cv.carve(cb ? pairs_max * (wide_items ? 8 : 4) : 4);
  p.region[MR_BCNT] = cv.carve((size_t)NBT * 4);
  p.region[MR_BOFF] = cv.carve((size_t)NBT * 4);
  p.region[MR_TOFF] = cv.carve(((size_t)NBT + 1) * 4);
  p.region[MR_BSUM] = cv.carve(((size_t)NBT / SCAN_BLOCK + 2) * 8);
  p.region[MR_SORTED] = cv.carve(pairs_max * 4);
  p.region[MR_TB] = cv.carve(T_max * 4);
  p.region[MR_TORDER] = cv.carve(T_max * 4);
  p.region[MR_TKEYS] = cv.carve(2 * TASK_KEYS * 4);
  p.region[MR_PARTIAL] = cv.carve(T_max * PT_WORDS * 4);
  p.region[MR_BUCKET] = cv.carve((size_t)NBT * PT_WORDS * 4);
  p.region[MR_SEG] = cv.carve(k4_2d ? (((size_t)1 << k4_m) + ((size_t)1 << k4_h)) * PT_WORDS * 4 * SW : (size_t)SW * nseg * PT_WORDS * 4);
  p.region[MR_SEG2] = cv.carve(((size_t)SW * (nseg / SUM_SPAN + 1)) * PT_WORDS * 4);
  p.region[MR_RES] = cv.carve((size_t)(single_set ? group : 1u) * res_stride * 4);   // per element: 4 totals words, then its records (one D2H copy)
  p.region[MR_BIG] = cv.carve(((size_t)NBT + 4) * 4);
  p.region[MR_SLICES] = cv.carve((T_max / FINALIZE_SLICE + T_max / (FINALIZE_SERIAL + 1) + 2) * 8);
  p.region[MR_BRLIST] = cv.carve(coop_sort ? (size_t)p.br_capacity * 8 : 8);
  p.region[MR_BRCOUNT] = cv.carve(16);
  p.region[MR_GCUR] = cv.carve(coop_sort ? (size_t)NBT * 4 : 4);
  p.ws_bytes = cv.off;
  if (!coop_sort) p.br_big = 0xffffffffu;    // the non-tiled scatter has no cooperative form: nothing is "big"

  // ---- launches: (grid x, grid y, block, dynamic LDS, the kernel's LDS limit) -------------------------
  auto set = [&p](uint32_t id, uint32_t gx, uint32_t gy, int block, size_t lds = 0, uint32_t cap = MSM_LDS_DEFAULT) {
    p.launch[id] = MsmLaunch{gx, gy, (uint32_t)block, (uint32_t)lds, cap};
  };
  if (digits_count) set(ML_DIGITS, (uint32_t)(n / chunk), group, DIGITS_COUNT_THREADS, (size_t)W * NC * 4);
  else set(ML_DIGITS, (uint32_t)((n + DIGITS_THREADS - 1) / DIGITS_THREADS), group, DIGITS_THREADS);
  set(ML_INIT, std::max<uint32_t>(4, (uint32_t)std::min<size_t>(((size_t)NBT + 255) / 256, 2048)), 1, 256);
  const size_t lds_fine = (size_t)4 << fb, lds_coarse = (size_t)NC * 4;
  if (cb) {
    if (!digits_count) set(ML_P1_HIST, G, SW, SORT_THREADS, lds_coarse);   // else the digits kernel left the coarse-bin counts behind
    set(ML_P1_SCAN, SW * NC, 1, 64);
    set(ML_P1_STARTS, 1, 1, 1024);
    // first-level scatter: LDS-sorted tiles while NC <= 4096 -- the vector-load form for 32-bit items (big tiles for 512 .. 2048
    // coarse bins), the tiled form for 64-bit items -- else straight from the digits
    p.p1_scatter = NC > 4096 ? MSM_P1S_DIRECT : wide_items ? MSM_P1S_TILED : NC >= 512 && NC <= 2048 ? MSM_P1S_VEC_BIG : MSM_P1S_VEC;
    const size_t tile = (size_t)SORT_THREADS * (p.p1_scatter == MSM_P1S_VEC_BIG ? P1_BIG_IPT : P1_IPT_DEFAULT);
    if (p.p1_scatter == MSM_P1S_DIRECT) set(ML_P1_SCATTER, G, SW, SORT_THREADS, lds_coarse);
    else set(ML_P1_SCATTER, G, SW, SORT_THREADS, ((size_t)3 * NC + 32 + tile) * 4 + tile * (wide_items ? 8 : 4), wide_items ? MSM_LDS_FINE : MSM_LDS_ALL);
    set(ML_BIG_REGIONS, (SW * NC + 255) / 256, 1, 256);
    set(ML_P2_HIST_COOP, p.br_capacity, 1, SORT_THREADS, lds_fine, MSM_LDS_FINE);
  }
  set(ML_P2_HIST, cb ? NC : 1, SW, SORT_THREADS, lds_fine, MSM_LDS_FINE);
  const uint32_t nblocks = (NBT + SCAN_BLOCK - 1) / SCAN_BLOCK;
  set(ML_SCAN_PARTIAL, nblocks, 1, SCAN_THREADS);
  set(ML_SCAN_BLOCKSUMS, 1, 1, SCAN_THREADS);
  set(ML_SCAN_FINAL, nblocks, 1, SCAN_THREADS);
  if (coop_sort) {      // the tiled form for 64-bit items, the vector-load form for 32-bit items
    const size_t lds_tiled = ((size_t)3 * (1u << fb) + 32 + P2_TILE) * 4 + (size_t)P2_TILE * 2;
    p.p2_scatter = wide_items ? MSM_P2S_TILED : MSM_P2S_VEC;
    set(ML_P2_SCATTER, NC, SW, SORT_THREADS, lds_tiled, MSM_LDS_ALL);
    set(ML_P2_SCATTER_COOP, p.br_capacity, 1, SORT_THREADS, lds_tiled, MSM_LDS_ALL);
  } else {
    p.p2_scatter = cb ? MSM_P2S_DIRECT : MSM_P2S_DIGITS;
    set(ML_P2_SCATTER, cb ? NC : 1, SW, SORT_THREADS, lds_fine, MSM_LDS_FINE);
  }
  const uint32_t og = (NBT + ORDER_THREADS * ORDER_ITEMS - 1) / (ORDER_THREADS * ORDER_ITEMS);
  if (p.tasks == MSM_TASKS_FILL) set(ML_TASK_FILL, (NBT + 255) / 256, 1, 256);
  else set(ML_TASK_HIST, og, 1, ORDER_THREADS), set(ML_TASK_KEYSCAN, 1, 1, ORDER_THREADS), set(ML_TASK_ORDER, og, 1, ORDER_THREADS);
  set(ML_ACCUMULATE, (uint32_t)((T_max + ACC_THREADS - 1) / ACC_THREADS), 1, ACC_THREADS);
  set(ML_FINALIZE, (NBT + ACC_THREADS - 1) / ACC_THREADS, 1, ACC_THREADS);
  set(ML_FINALIZE_SLICES, (uint32_t)std::min<uint64_t>(T_max / FINALIZE_SLICE + 1, 2048), 1, WIN_THREADS);          // at most: the full slices
  set(ML_FINALIZE_BIG, (uint32_t)std::min<uint64_t>(T_max / (FINALIZE_SERIAL + 1) + 1, 2048), 1, WIN_THREADS);     // ... the queued buckets
  if (k4_2d) {
    if (wave_sums) set(ML_ROWCOL, (1u << k4_h) + (1u << (k4_m - 1)), SW, WAVE_THREADS);
    else set(ML_ROWCOL, (1u << k4_m) + (1u << k4_h), SW, WIN_THREADS);
    set(ML_BITS, RW, SW, WIN_THREADS);
  } else {
    set(ML_SEGMENTS, (SW * nseg + ACC_THREADS - 1) / ACC_THREADS, 1, ACC_THREADS);
    for (uint32_t count = nseg; count > 1; count = (count + SUM_SPAN - 1) / SUM_SPAN) {
      if (p.sum_levels == 2) return msm_plan_fail(p, MSM_PLAN_INTERNAL, "msm: more than two levels of segment sums");
      p.sum_count[p.sum_levels] = count;
      set(ML_SUM_0 + p.sum_levels++, (count + SUM_SPAN - 1) / SUM_SPAN, SW, WIN_THREADS);
    }
    set(ML_TO_EXT, (SW + 63) / 64, 1, 64);
  }
  if (RW > 128) return msm_plan_fail(p, MSM_PLAN_INTERNAL, "msm: more than 128 windows");
  return p;
}

// ---- the five-launch chain (msm_small.hip) ----------------------------------------------------------------------------
enum MsmSmallRegion : uint32_t {
  MSR_DIGITS, MSR_TOFF, MSR_GCTR, MSR_NZ, MSR_NZC, MSR_DESC, MSR_SORTED, MSR_PARTIAL, MSR_SEG1, MSR_BLKIDX, MSR_ELEMENT_COUNT,
  MSR_RES = MSR_ELEMENT_COUNT, MSR_LIVE, MSR_COUNT       // one copy per element of the group, then the group's results and counters
};
enum MsmSmallLaunchId : uint32_t { MSL_DIGITS, MSL_SORT, MSL_ACCUMULATE, MSL_REDUCE1, MSL_REDUCE2, MSL_COUNT };
struct MsmSmallPlan {
  int err = MSM_PLAN_OK;
  const char* err_msg = nullptr;
  uint32_t group = 1, W = 0, wide = 0, n_wide = 0, NB = 0;
  uint64_t pairs_max = 0;
  uint32_t H = 0, NBh = 0, V = 0, L = 0, SEG = 0, nseg = 0, G1n = 0;
  uint32_t segs_per_window = 0;        // first-level sums the last kernel adds per window: H * G1n
  uint64_t T_max = 0;
  MsmSpan region[MSR_COUNT] = {};      // [0, MSR_ELEMENT_COUNT): offsets inside one element's ws_stride bytes
  size_t ws_stride = 0;                // one element's arrays; the group's results follow them all
  uint32_t res_stride = 0;             // words per element: totals, then the window sums
  size_t ws_bytes = 0;
  MsmLaunch launch[MSL_COUNT];
};

static inline MsmSmallPlan msm_small_plan(size_t n, uint32_t group, uint32_t c) {
  MsmSmallPlan p;
  p.group = group;
  if (group < 1 || group > (uint32_t)MSM_GROUP_MAX) return msm_plan_fail(p, MSM_PLAN_INTERNAL, "msm (small plan): bad group size");
  const uint32_t W = p.W = (255 + c - 1) / c;
  if (W > 128) return msm_plan_fail(p, MSM_PLAN_INTERNAL, "msm: more than 128 windows");
  // balanced widths: n_wide windows of `wide` bits, the rest of wide - 1 (wide <= c)
  balanced_windows(W, &p.wide, &p.n_wide);
  const uint32_t NB = p.NB = 1u << (p.wide - 1);
  const uint64_t pairs_max = p.pairs_max = (uint64_t)n * W;
  // bucket-range splits per window: more sort workgroups once one workgroup per window streams too long
  uint32_t H = 1;
  while (H < 8 && (uint64_t)n / H > (1u << 15) && NB / (2 * H) >= 64) H *= 2;
  while (H > 1 && NB / H < 2) H /= 2;
  p.H = H;
  const uint32_t NBh = p.NBh = NB / H, V = p.V = W * H;
  // Task length.  K3's chain costs L mixed additions, D then sums ~mean/L Jacobian partials per bucket (1.6x
  // the instructions each): short tasks only pay while they are needed to fill the chip.
  const double mean = (double)n / (double)NB;
  uint32_t L = (uint32_t)(mean + 4.0 * std::sqrt(mean) + 8.0);
  {
    uint64_t by_fill = pairs_max / 327680;
    if (by_fill < 16) by_fill = 16;          // measured: 12 .. 16 beats 8 at every size below 2^18
    if (by_fill < L) L = (uint32_t)by_fill;
  }
  if (L < 2) L = 2;
  if (L > S_MAX_L) L = S_MAX_L;
  p.L = L;
  // D's segment length: at most one 256-lane workgroup per CU over all virtual windows -- one wave per SIMD;
  // what costs is the depth of a lane's chain (2 SEG additions + a log2(NB)-bit multiple), not the work
  uint32_t SEG = 2;
  while (SEG < NBh && (uint64_t)V * ((NBh / SEG + WIN_THREADS - 1) / WIN_THREADS) > 256) ++SEG;
  // a group multiplies the workgroups: then count WAVES with a segment to sum -- one per SIMD (1024) over the whole group
  // (never fewer than one wave per virtual window and element: 64 segments there is the coarsest useful cut)
  if (group > 1)
    while (SEG < NBh && (NBh + SEG - 1) / SEG > 64 && (uint64_t)V * group * (((NBh + SEG - 1) / SEG + 63) / 64) > 1024) ++SEG;
  if (SEG > NBh) SEG = NBh;
  p.SEG = SEG;
  const uint32_t nseg = p.nseg = (NBh + SEG - 1) / SEG;
  const uint32_t G1n = p.G1n = (nseg + WIN_THREADS - 1) / WIN_THREADS;
  p.segs_per_window = H * G1n;
  // sum over all buckets of ceil(cnt / L) <= pairs / L + number of buckets
  const uint64_t T_max = p.T_max = pairs_max / L + (uint64_t)V * NBh + 64;

  MsmCarver cv;
  p.region[MSR_DIGITS] = cv.carve((size_t)((n + SA_THREADS - 1) / SA_THREADS * SA_THREADS) * W * 4);   // rows padded to whole blocks
  p.region[MSR_TOFF] = cv.carve((size_t)V * (NBh + 2) * 4);
  p.region[MSR_GCTR] = cv.carve(16);
  p.region[MSR_NZ] = cv.carve((size_t)V * NBh * 4);
  p.region[MSR_NZC] = cv.carve((size_t)V * 4);
  p.region[MSR_DESC] = cv.carve(T_max * 16);
  p.region[MSR_SORTED] = cv.carve(pairs_max * 4);
  p.region[MSR_PARTIAL] = cv.carve(T_max * PT_WORDS * 4);
  p.region[MSR_SEG1] = cv.carve((size_t)V * G1n * PT_WORDS * 4);
  p.region[MSR_BLKIDX] = cv.carve(((n + SA_THREADS - 1) / SA_THREADS) * 4);
  p.ws_stride = cv.off;
  p.res_stride = 4 + W * 32;
  cv.off = p.ws_stride * group;
  p.region[MSR_RES] = cv.carve((size_t)group * p.res_stride * 4);
  p.region[MSR_LIVE] = MsmSpan{cv.off, (size_t)MSM_GROUP_MAX * 4};     // the group's survivor counters, together
  p.ws_bytes = cv.off + (size_t)MSM_GROUP_MAX * 4;

  const uint32_t lds_sort = (uint32_t)(((size_t)((NBh + 1 + 31) & ~31u) + 2 * S_TASK_KEYS + 32) * 4);
  p.launch[MSL_DIGITS] = MsmLaunch{(uint32_t)((n + SA_THREADS - 1) / SA_THREADS), group, SA_THREADS};
  p.launch[MSL_SORT] = MsmLaunch{V, group, SS_THREADS, lds_sort, MSM_S_LDS_SORT};
  p.launch[MSL_ACCUMULATE] = MsmLaunch{(uint32_t)((T_max + ACC_THREADS - 1) / ACC_THREADS), group, ACC_THREADS};
  p.launch[MSL_REDUCE1] = MsmLaunch{G1n, V, WIN_THREADS, 0, MSM_LDS_DEFAULT, group};
  p.launch[MSL_REDUCE2] = MsmLaunch{W, group, WIN_THREADS};
  return p;
}

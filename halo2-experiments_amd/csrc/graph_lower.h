// graph_lower.h -- the host-only, GPU-free part of graph.hip's program "compilation": the instruction encoding, the
// validation of hm_graph_create and the lowering passes (copy propagation, register forwarding and store elision, the
// static value-bound analysis, linear-scan slot allocation).  graph.hip includes it and uploads the result;
// host_check.cpp (libhm_hostcheck.so, the HM_BOUNDS build) includes it too, lowers the same programs and interprets
// them with bound tracking, so that every decision below is tested on a machine without a GPU
// (tests/test_graph_lowering_host.py) and against the kernel on one (tests/test_graph_programs_gpu.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <map>
#include <vector>

#if defined(__HIPCC__)
#define HM_GRAPH_HD __host__ __device__ inline
#else
#define HM_GRAPH_HD inline
#endif

namespace hm {

enum GraphOp : uint32_t { GOP_ADD = 0, GOP_SUB = 1, GOP_MUL = 2, GOP_SQUARE = 3, GOP_DOUBLE = 4, GOP_NEGATE = 5, GOP_STORE = 6, GOP_MULADD = 7 };
enum GraphSrc : uint32_t { GSRC_CONST = 0, GSRC_INTER = 1, GSRC_COLUMN = 2, GSRC_PREV = 3 };
// a source is one word: kind (bits 30..31) | rotation index (bits 20..29) | index (bits 0..19); a column source uses
// index bits 0..13 for the column and bits 14..19 for the column's log2 row count when it is SHORTER than the domain
// (read at row mod 2^that; 0 = a full-size column): the period lives in the instruction, not in a per-call table.
HM_GRAPH_HD uint32_t gsrc_kind(uint32_t s) { return s >> 30; }
HM_GRAPH_HD uint32_t gsrc_rot(uint32_t s) { return (s >> 20) & 1023u; }
HM_GRAPH_HD uint32_t gsrc_index(uint32_t s) { return s & 0xfffffu; }
HM_GRAPH_HD uint32_t gsrc_column(uint32_t s) { return s & 0x3fffu; }
HM_GRAPH_HD uint32_t gsrc_log_rows(uint32_t s) { return (s >> 14) & 63u; }

struct GraphCalc {      // device form: 5 words; op carries the forwarding flags in bits 8..11
  uint32_t op, a, b, c, target;
};
// Expression trees are evaluated depth first, so the result of calculation k is very often an operand of k + 1 and of
// nothing else (45 % of all intermediate reads and 55 % of all writes of the MerkleSumTree program): the lowering marks
// those operands "take the previous result from registers" and those targets "never stored", which removes that share
// of the [slot][word][lane] scratch traffic -- the interpreter is bound by it, not by the arithmetic.
constexpr uint32_t GF_A_PREV = 1u << 8, GF_B_PREV = 1u << 9, GF_C_PREV = 1u << 10, GF_NO_STORE = 1u << 11;
// Lazy reductions.  An intermediate is a normalised element (29-bit limbs) of value < GE_CAP * r, not < 3r: products
// accept that (inputs < 18r give outputs < 3r; the column sums depend on the limbs only), so a sum or difference needs
// its ~50-instruction modular reduction only when its STATIC bound -- propagated through the program at lowering time --
// would pass GE_CAP.  GF_NO_REDUCE: carry propagation only.  GF_SUB_WIDE: the subtrahend may exceed 3r, so the
// subtraction adds 20r instead of 4r (and is always reduced).  Bounds of every combination: hc_graph_bounds_closure
// (host_check.cpp, HM_BOUNDS build), tests/test_ff29_host.py; the bounds propagated through whole programs against
// the tracked ones: hc_graph_replay, tests/test_graph_lowering_host.py.
constexpr uint32_t GF_NO_REDUCE = 1u << 12, GF_SUB_WIDE = 1u << 13;
constexpr double GE_CAP = 16.0, GE_COLUMN_BOUND = 6.0;     // a packed 256-bit word is < 2^256 < 5.3 r whatever it holds

constexpr uint32_t GE_MAX_COLUMNS = 256;
constexpr uint32_t GE_MAX_DYN = 16;

// The address rule of hm_graph_evaluate_proofs_dev (graph.hip: graph_proofs_kernel), one lane per (proof, row) with the rows running
// fastest: lane -> (proof, row of the proof); (row, rotation) -> the row a column source reads, wrapped inside the row's segment
// and then inside a short column's period, exactly as in the single evaluation; (proof, row, column stride) -> the cell's u32 word
// behind the column's base (stride 0: one column for all proofs); (proof, word) -> the word of the per-proof constant table
// (proofs x n_dynamic x 9 internal words).  Nothing here ever adds a proof's rows to another proof's: a rotation at the last row of
// proof b lands on proof b's first row.  host_check.cpp runs the same functions (hc_graph_proofs_address).
// (proofs * rows <= 2^32, so a lane fits 32 bits, and rows = 2^32 leaves room for proof 0 alone: a 32-bit division)
// graph_source_row is the row rule of all three kernels: segment_mask = segment length - 1 (one segment = the whole domain in the
// ordinary call, one coset of the extended domain in hm_graph_evaluate_segments_dev); a short column (the vanishing polynomial's
// inverse pattern) is periodic.
HM_GRAPH_HD uint32_t graph_proofs_proof(uint64_t lane, uint64_t rows) { return rows >> 32 ? 0u : (uint32_t)lane / (uint32_t)rows; }
HM_GRAPH_HD uint64_t graph_source_row(uint64_t row, int64_t rotation, uint64_t segment_mask, uint32_t log_rows) {
  uint64_t r = (row & ~segment_mask) | ((row + (uint64_t)rotation) & segment_mask);      // two's complement: a negative rotation wraps
  if (log_rows != 0) r &= (1ull << log_rows) - 1ull;
  return r;
}
HM_GRAPH_HD uint64_t graph_proofs_cell(uint64_t proof, uint64_t row, uint64_t stride_words) { return stride_words * proof + row * 8; }
HM_GRAPH_HD uint64_t graph_proofs_dyn(uint64_t proof, uint32_t n_dynamic, uint32_t word) { return proof * (n_dynamic * 9u) + word; }

inline bool graph_src_ok(uint32_t s, size_t n_const, size_t n_inter, size_t n_cols, size_t n_rot) {
  switch (gsrc_kind(s)) {
    case GSRC_CONST: return gsrc_index(s) < n_const;
    case GSRC_INTER: return gsrc_index(s) < n_inter;
    case GSRC_COLUMN: return gsrc_column(s) < n_cols && gsrc_rot(s) < n_rot && gsrc_log_rows(s) <= 30;
    default: return true;
  }
}

// What hm_graph_create promises about a program before anything is allocated: nullptr, or the reason it is refused.
inline const char* graph_validate(const uint32_t* calcs5, size_t n_calc, size_t n_const_static, size_t n_dynamic, size_t n_rot, size_t n_columns,
                                  uint32_t n_intermediates) {
  if (n_dynamic > GE_MAX_DYN) return "graph: more than 16 per-call constants";
  const size_t n_const = n_const_static + n_dynamic;
  if (n_calc > (1u << 24) || n_const >= (1u << 20) || n_rot > 1024 || n_columns > GE_MAX_COLUMNS || n_intermediates >= (1u << 20))
    return "graph: program too large for the instruction encoding";
  std::vector<char> defined(n_intermediates, 0);
  for (size_t k = 0; k < n_calc; ++k) {
    const uint32_t* c = calcs5 + 5 * k;
    if (c[0] > GOP_MULADD) return "graph: unknown operation";
    const int nsrc = c[0] == GOP_MULADD ? 3 : (c[0] <= GOP_MUL ? 2 : 1);
    for (int j = 0; j < nsrc; ++j) {
      const uint32_t s = c[1 + j];
      if (!graph_src_ok(s, n_const, n_intermediates, n_columns, n_rot)) return "graph: source out of range";
      if (gsrc_kind(s) == GSRC_INTER && !defined[gsrc_index(s)]) return "graph: intermediate read before it is written";
    }
    if (c[4] >= n_intermediates) return "graph: target out of range";
    if (defined[c[4]]) return "graph: intermediate written twice (every calculation owns its target)";
    defined[c[4]] = 1;
  }
  return nullptr;
}

// What hm_graph_evaluate_circuits_dev admits, checked on a VALIDATED program as it was created: a value that is linear in
// PreviousValue the way GraphEvaluator.add_custom_gates builds it.  PreviousValue occurs once in the whole program, as the
// start of the Horner (MulAdd) chain that ends in the last calculation; every step of the chain has the same factor, a
// constant (of the program or of the call); no step's value is read by anything but the next step.  The value is then
// Prev * f^steps + G(row), with G what the program leaves for Prev = 0.  -> nullptr and (factor source word, steps), or
// the reason the program is refused.
inline const char* graph_linear_shape(const uint32_t* calcs5, size_t n_calc, uint32_t n_intermediates, uint32_t* factor_src, uint32_t* steps) {
  if (n_calc == 0) return "graph: an empty program is not linear in PreviousValue";
  auto nsrc_of = [](uint32_t op) { return op == GOP_MULADD ? 3 : (op <= GOP_MUL ? 2 : 1); };
  std::vector<uint32_t> defined_by(n_intermediates, 0xffffffffu), reads(n_intermediates, 0);
  size_t prev_reads = 0;
  for (size_t k = 0; k < n_calc; ++k) {
    const uint32_t* c = calcs5 + 5 * k;
    for (int j = 0; j < nsrc_of(c[0]); ++j) {
      if (gsrc_kind(c[1 + j]) == GSRC_PREV) ++prev_reads;
      if (gsrc_kind(c[1 + j]) == GSRC_INTER) ++reads[gsrc_index(c[1 + j])];
    }
    defined_by[c[4]] = (uint32_t)k;
  }
  if (prev_reads != 1) return "graph: PreviousValue must be read exactly once";
  const uint32_t* last = calcs5 + 5 * (n_calc - 1);
  if (last[0] != GOP_MULADD || gsrc_kind(last[2]) != GSRC_CONST) return "graph: the last calculation must be a Horner step with a constant factor";
  if (reads[last[4]] != 0) return "graph: the value of the Horner chain is read inside the program";
  const uint32_t factor = last[2];
  uint32_t count = 0;
  for (const uint32_t* c = last;;) {
    if (c[0] != GOP_MULADD || c[2] != factor) return "graph: the Horner chain from PreviousValue must use one factor";
    ++count;
    if (gsrc_kind(c[1]) == GSRC_PREV) break;
    if (gsrc_kind(c[1]) != GSRC_INTER) return "graph: PreviousValue is not the start of the final Horner chain";
    if (reads[gsrc_index(c[1])] != 1) return "graph: a step of the Horner chain is read outside the chain";
    c = calcs5 + 5 * defined_by[gsrc_index(c[1])];
  }
  *factor_src = factor;
  *steps = count;
  return nullptr;
}

// ---- one call of the evaluator: what it is, whether it is admitted, how it is launched (graph.hip: graph_run) ----
// The argument blocks as the kernels read them (graph.hip says why they travel through a device buffer).
struct GraphColumns {
  const uint32_t* p[GE_MAX_COLUMNS];
  uint32_t dyn[GE_MAX_DYN * 9];   // challenges, beta, gamma, theta, y ... of THIS proof, internal form
  uint32_t n_static;              // constants [0, n_static) come from the program, [n_static, ..) from dyn
};
struct GraphCircuitColumns {
  const uint32_t* p[GE_MAX_COLUMNS];
  uint64_t stride[GE_MAX_COLUMNS];   // u32 words from circuit c's column to circuit c + 1's; 0: one column for all circuits
  uint32_t dyn[GE_MAX_DYN * 9];
  uint32_t fold[9];                  // f^T, internal form
  uint32_t n_static;
};
struct GraphProofColumns {           // followed by the constant table: proofs x n_dynamic x 9 internal words
  const uint32_t* p[GE_MAX_COLUMNS];
  uint64_t stride[GE_MAX_COLUMNS];   // u32 words from proof b's column to proof b + 1's; 0: one column for all proofs
  uint32_t n_static, n_dynamic;
};

enum GraphCallKind : uint32_t { GRAPH_SINGLE = 0, GRAPH_CIRCUITS = 1, GRAPH_PROOFS = 2 };
struct GraphCall {
  GraphCallKind kind;
  size_t n_columns, units, n_dyn;    // units: circuits or proofs (1 for the single kind); n_dyn: per-call constants of ONE unit
  uint32_t log_size, segments, flags;
  const void* d_values;
  uint64_t values_stride;            // u32 words between two proofs' values (the proofs kind with units > 1; unread otherwise)
  const void* const* bases;          // n_columns device pointers: unit 0's columns
  const uint64_t* strides;           // u32 words to the next unit's column; null for the single kind
  const uint64_t* dyn_ext;           // n_dyn (the proofs kind: units * n_dyn) x 4 Montgomery words on the host; not read by the check
};

// Every refusal of a call that needs no walk of the program, in the order the entries have always applied them: nullptr, or the
// reason.  The kernels read and write cells as two uint4, whatever the kind: the values and every column base are 16-byte
// aligned, every stride a multiple of 4 words.  tests/test_graph_plan_host.py holds the table of refusals.
inline const char* graph_check_call(const GraphCall& c, size_t program_columns, size_t program_dynamic) {
  if (c.flags & ~1u) return "graph: unknown flag";                                   // HM_GRAPH_COLUMNS_INTERNAL is bit 0
  if (c.units == 0) return c.kind == GRAPH_PROOFS ? "graph: proofs must be >= 1" : "graph: circuits must be >= 1";
  if (c.kind != GRAPH_SINGLE && c.n_columns > GE_MAX_COLUMNS) return "graph: more columns than the column table holds";
  if (c.n_columns != program_columns) return "graph: the program was built for another number of columns";
  if (c.n_dyn != program_dynamic) return "graph: the program was built for another number of per-call constants";
  if (c.log_size > 30) return "graph: log_size > 30";
  if (c.segments == 0 || ((uint64_t)c.segments << c.log_size) > (1ull << 32)) return "graph: segments must be >= 1 and rows <= 2^32";
  const uint64_t size = (uint64_t)c.segments << c.log_size;
  if (c.units > (1ull << 32) / size) return c.kind == GRAPH_PROOFS ? "graph: proofs * rows > 2^32" : "graph: circuits * rows > 2^32";
  if ((uintptr_t)c.d_values % 16) return "graph: the values are not 16-byte aligned";
  if (c.kind == GRAPH_PROOFS && c.units > 1 && (c.values_stride < size * 8 || c.values_stride % 4))
    return "graph: the values stride must be a multiple of 4 words and hold the rows of one proof";
  for (size_t i = 0; i < c.n_columns; ++i) {
    if (!c.bases[i]) return "graph: null column pointer";
    if ((uintptr_t)c.bases[i] % 16) return "graph: a column base is not 16-byte aligned";
    if (c.strides && c.strides[i] % 4) return "graph: a column stride is not a multiple of 4 words";
  }
  return nullptr;
}

// The launch of an admitted call: `size` rows, `units` circuits or proofs, a program lowered to n_slots scratch slots, at most
// max_blocks workgroups of 256 lanes.  Enough lanes to fill the chip, few enough that the intermediates' scratch
// ([slot][word][lane], 9 words a slot) stays cache-sized.  single / proofs: one lane per (unit, row).  circuits: C = 2^log_c
// circuits side by side in a workgroup of 256 / C rows -- as many as it takes for the grid to reach the single kind's block
// count, no more than the circuits there are (units = 1 gives C = 1: the single kind's shape); `lanes` are those of one group
// of C circuits.  Swept against the three formulas this replaced and its invariants: tests/test_graph_plan_host.py.
struct GraphPlan {
  uint64_t size, lanes;
  uint32_t blocks, T, log_c, rows_per;
  size_t scratch_bytes, args_bytes;
};
inline GraphPlan graph_launch_plan(GraphCallKind kind, uint64_t size, uint64_t units, uint32_t n_slots, size_t n_dyn, uint32_t max_blocks) {
  constexpr uint64_t W = 256;                                                           // graph_interp.h: GE_THREADS
  GraphPlan p{};
  p.size = size;
  if (kind == GRAPH_CIRCUITS)
    while (p.log_c < 8 && (1ull << p.log_c) < units && ((size << p.log_c) + W - 1) / W < max_blocks) ++p.log_c;
  p.rows_per = (uint32_t)(W >> p.log_c);
  p.lanes = kind == GRAPH_PROOFS ? units * size : size << p.log_c;
  p.blocks = (uint32_t)std::min<uint64_t>(kind == GRAPH_CIRCUITS ? (size + p.rows_per - 1) / p.rows_per : (p.lanes + W - 1) / W, max_blocks);
  p.T = p.blocks * (uint32_t)W;
  p.scratch_bytes = (size_t)n_slots * 9 * p.T * 4;
  p.args_bytes = kind == GRAPH_SINGLE     ? sizeof(GraphColumns)
                 : kind == GRAPH_CIRCUITS ? sizeof(GraphCircuitColumns)
                                          : sizeof(GraphProofColumns) + std::max<size_t>(units * n_dyn, 1) * 9 * 4;
  return p;
}

struct GraphLowered {       // a validated program lowered for one column format, still on the host
  std::vector<GraphCalc> calcs;
  std::vector<double> bound;              // per lowered calculation: the static bound (units of r) of the value it leaves
  uint32_t n_slots = 1, result_src = 0, result_prev = 0;
  uint32_t stores_of_constants_removed = 0, stores_of_columns_removed = 0;     // copy propagation, for the tests' coverage
};

// Lower the validated program for one column format.  Steps: (1) copy propagation -- a Store of a constant, or of a
// column when columns need no conversion, defines nothing new: its users read the source directly (upstream stores every
// queried cell once so that the CPU loop converts it once; here a column read costs what a scratch read costs);
// (2) forwarding flags and store elision (see GF_*); (3) linear-scan slot allocation by liveness for what is still stored.
inline void graph_lower_host(const uint32_t* calcs5, size_t n_in, uint32_t n_inter, bool internal_cols, GraphLowered& out) {
  auto nsrc_of = [](uint32_t op) { return op == GOP_MULADD ? 3 : (op <= GOP_MUL ? 2 : 1); };
  // (1) copy propagation
  std::vector<uint32_t> alias(n_inter, 0xffffffffu);          // intermediate -> the source word that replaces it
  auto resolve = [&](uint32_t s) { return gsrc_kind(s) == GSRC_INTER && alias[gsrc_index(s)] != 0xffffffffu ? alias[gsrc_index(s)] : s; };
  struct Ins { uint32_t op, src[3], target; };
  std::vector<Ins> prog;
  prog.reserve(n_in);
  for (size_t k = 0; k < n_in; ++k) {
    const uint32_t* c = &calcs5[5 * k];
    Ins in{c[0], {resolve(c[1]), resolve(c[2]), resolve(c[3])}, c[4]};
    if (in.op == GOP_STORE) {
      const uint32_t kd = gsrc_kind(in.src[0]);
      if (kd == GSRC_CONST || (kd == GSRC_COLUMN && internal_cols)) {
        alias[in.target] = in.src[0];
        ++(kd == GSRC_CONST ? out.stores_of_constants_removed : out.stores_of_columns_removed);
        continue;
      }
    }
    prog.push_back(in);
  }
  uint32_t result_src = n_in ? resolve((GSRC_INTER << 30) | calcs5[5 * (n_in - 1) + 4]) : ((GSRC_INTER << 30) | 0u);
  const size_t n = prog.size();
  // (2) uses of every intermediate; forwarding and store elision
  std::vector<std::vector<uint32_t>> uses(n_inter);
  for (size_t k = 0; k < n; ++k)
    for (int j = 0; j < nsrc_of(prog[k].op); ++j)
      if (gsrc_kind(prog[k].src[j]) == GSRC_INTER) uses[gsrc_index(prog[k].src[j])].push_back((uint32_t)k);
  const bool result_is_inter = n_in != 0 && gsrc_kind(result_src) == GSRC_INTER;
  const bool result_prev = result_is_inter && n != 0 && prog[n - 1].target == gsrc_index(result_src);
  std::vector<uint32_t> flags(n, 0);
  std::vector<char> stored(n, 1);
  for (size_t k = 0; k < n; ++k) {
    if (k > 0)
      for (int j = 0; j < nsrc_of(prog[k].op); ++j)
        if (gsrc_kind(prog[k].src[j]) == GSRC_INTER && gsrc_index(prog[k].src[j]) == prog[k - 1].target)
          flags[k] |= j == 0 ? GF_A_PREV : (j == 1 ? GF_B_PREV : GF_C_PREV);
    bool only_next = true;
    for (uint32_t u : uses[prog[k].target]) only_next = only_next && u == (uint32_t)k + 1;
    const bool is_result = result_is_inter && prog[k].target == gsrc_index(result_src);
    if (only_next && (!is_result || (result_prev && k == n - 1))) {     // read (if at all) by the next instruction only
      stored[k] = 0;
      flags[k] |= GF_NO_STORE;
    }
  }
  // (2b) static value bounds (in units of r) -> which sums and differences keep their reduction
  out.bound.assign(n, 3.0);
  {
    std::vector<double> vb(n_inter, 3.0);
    auto bound_of = [&](uint32_t sw) -> double {
      switch (gsrc_kind(sw)) {
        case GSRC_CONST: return 1.0;                                  // canonical constants
        case GSRC_INTER: return vb[gsrc_index(sw)];
        case GSRC_COLUMN: return internal_cols ? GE_COLUMN_BOUND : 3.0;   // external words pass through a product
        default: return 3.0;                                          // PreviousValue: a product output
      }
    };
    for (size_t k = 0; k < n; ++k) {
      const Ins& in = prog[k];
      double r = 3.0;
      uint32_t f = 0;
      switch (in.op) {
        case GOP_ADD: r = bound_of(in.src[0]) + bound_of(in.src[1]); break;
        case GOP_DOUBLE: r = 2.0 * bound_of(in.src[0]); break;
        case GOP_MULADD: r = 3.0 + bound_of(in.src[2]); break;
        case GOP_SUB:
        case GOP_NEGATE: {
          const double minuend = in.op == GOP_SUB ? bound_of(in.src[0]) : 0.0;
          const double subtrahend = bound_of(in.src[in.op == GOP_SUB ? 1 : 0]);
          if (subtrahend <= 3.0) {
            r = minuend + 4.0;
          } else {
            f |= GF_SUB_WIDE;                                         // reduced in the kernel whatever r is
            r = 1e9;
          }
          break;
        }
        case GOP_STORE: r = bound_of(in.src[0]); f |= GF_NO_REDUCE; break;     // a copy
        default: r = 3.0; f |= GF_NO_REDUCE; break;                   // Mul / Square: product outputs (the flag is not read)
      }
      if (!(f & (GF_NO_REDUCE | GF_SUB_WIDE))) {
        if (r <= GE_CAP) f |= GF_NO_REDUCE;
        else r = 3.0;                                                 // reduced
      } else if (f & GF_SUB_WIDE) {
        r = 3.0;
      }
      vb[in.target] = r;
      out.bound[k] = r;
      flags[k] |= f;
    }
  }
  // (3) slots for what is stored
  std::vector<uint32_t> last_use(n_inter, 0), slot_of(n_inter, 0xffffffffu), free_slots;
  for (size_t k = 0; k < n; ++k)
    for (int j = 0; j < nsrc_of(prog[k].op); ++j)
      if (gsrc_kind(prog[k].src[j]) == GSRC_INTER) last_use[gsrc_index(prog[k].src[j])] = (uint32_t)k;
  if (result_is_inter && !result_prev) last_use[gsrc_index(result_src)] = (uint32_t)n;
  std::multimap<uint32_t, uint32_t> expiring;                  // last use -> slot
  std::vector<GraphCalc>& dev = out.calcs;
  dev.assign(n, GraphCalc{});
  uint32_t n_slots = 0;
  auto remap = [&](uint32_t s) -> uint32_t {
    if (gsrc_kind(s) != GSRC_INTER) return s;
    const uint32_t sl = slot_of[gsrc_index(s)];
    return (GSRC_INTER << 30) | (sl == 0xffffffffu ? 0u : sl);   // a never-stored operand is always taken from registers
  };
  for (size_t k = 0; k < n; ++k) {
    const Ins& in = prog[k];
    const int ns = nsrc_of(in.op);
    GraphCalc d{in.op | flags[k], remap(in.src[0]), ns > 1 ? remap(in.src[1]) : 0u, ns > 2 ? remap(in.src[2]) : 0u, 0};
    // slots whose value was read for the last time BEFORE this instruction are free (its own operands are read before
    // its target is written, so a slot expiring AT k may be reused as k's target)
    while (!expiring.empty() && expiring.begin()->first <= (uint32_t)k) {
      free_slots.push_back(expiring.begin()->second);
      expiring.erase(expiring.begin());
    }
    if (stored[k]) {
      uint32_t slot;
      if (!free_slots.empty()) {
        slot = free_slots.back();
        free_slots.pop_back();
      } else {
        slot = n_slots++;
      }
      slot_of[in.target] = slot;
      // a value that is never read again still needs its slot for this one instruction
      expiring.emplace(last_use[in.target] > (uint32_t)k ? last_use[in.target] : (uint32_t)k + 1, slot);
      d.target = slot;
    }
    dev[k] = d;
  }
  out.n_slots = n_slots ? n_slots : 1;
  out.result_prev = result_prev ? 1u : 0u;
  out.result_src = result_is_inter ? remap(result_src) : result_src;
}

}  // namespace hm

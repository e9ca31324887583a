// graph.hip -- evaluate_h's gate arithmetic on the device (second half): the GraphEvaluator of
// halo2_proofs::plonk::evaluation (the crate pinned at /root/reference/Cargo.toml:10; reached from create_proof,
// /root/reference/src/circuits/utils.rs:40-48).  Upstream flattens every gate / lookup expression of a circuit
// into a straight-line program over "value sources" and runs it once per row of the extended domain on the CPU:
//
//     ValueSource   Constant(i) | Intermediate(i) | Fixed(col, rot) | Advice(col, rot) | Instance(col, rot)
//                   | Challenge(i) | Beta | Gamma | Theta | Y | PreviousValue
//     Calculation   Add | Sub | Mul | Square | Double | Negate | Horner(start, parts, factor) | Store
//     row index of a rotated query: (idx + rot * 2^(extended_k - k)) mod 2^extended_k
//
// Here: one lane per row, all columns resident in HBM (extended-domain arrays, external Montgomery words), the
// program interpreted instruction by instruction with wave-uniform decode.  Fixed / Advice / Instance are one
// column table; challenges, beta, gamma, theta, y are constants of the call (the mirror in evaluation.py maps
// them); Horner is lowered to MulAdd steps.  Intermediates live in a scratch array laid out [slot][word][lane] so
// that every access is coalesced; the host first maps the program's intermediates to slots by liveness (upstream
// gives every calculation a fresh index; only a few dozen are live at once), so the scratch stays L2-sized.
// Values are kept in ff29's internal form (< 3r, normalised limbs); a column word is converted on load.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <map>

#include "g1.h"
#include "graph_interp.h"
#include "graph_lower.h"
#include "hm_internal.h"
#include "host_fr.h"

namespace hm {

// the instruction encoding (GraphOp, GraphSrc, GraphCalc, GF_*, GE_CAP ...), graph_validate and graph_lower_host: graph_lower.h,
// shared with the host replay of host_check.cpp; the interpreter body (ge_fetch, ge_reduce, ge_run and the column-word loads):
// graph_interp.h, shared with the witness checker's kernel (mock.hip)

// The call's column table and per-call constants (2.6 KiB) travel through a DEVICE buffer of the stream's AuxSlot,
// filled by a stream-ordered copy ahead of the launch.  Rounds 1-2 passed the struct by value, and a variant with a
// BYTE table in it (the columns' periods) aborted at run time.  What is known (tools/ubench/kernarg_byval.hip,
// profiles/r04_kernarg_byval.txt, profiles/r05_kernarg_isa.txt): not the argument's size (3 176 bytes of kernarg, limit
// 4 096; no scratch).  A dynamically indexed table of 32- or 64-bit entries in a by-value argument is read with SCALAR
// loads from the kernarg segment (s_load_dword s, s[0:1], s_off), which work; a table of BYTES cannot be (s_load has no
// sub-dword form), so the compiler emits a VECTOR load addressed through the kernarg pointer (global_load_ubyte v, v,
// s[0:1] offset:...).  A stand-alone kernel of that shape faulted ONCE on this stack and runs without the byte table --
// a correlation, not an established cause: the load is legal ISA, s[0:1] is intact and the offset in range.  HYPOTHESIS:
// the vector path cannot read the runtime's kernarg buffer here.  The library does not rest on it: this kernel takes ONE
// pointer to a device copy (every table access an ordinary global load, a 72-byte argument block whatever the program's
// shape), and tests/test_isa.py asserts on the built objects that no kernel of the library addresses a vector memory
// instruction through its kernarg pointer.  tests/test_evaluation.py runs 256 columns, short-period columns and 16
// per-call constants through it.  The three argument blocks (GraphColumns, GraphCircuitColumns, GraphProofColumns): graph_lower.h.
static_assert(GE_THREADS == 256 && HM_GRAPH_COLUMNS_INTERNAL == 1, "graph_lower.h: graph_launch_plan, graph_check_call");
static_assert(offsetof(GraphColumns, p) == 0 && offsetof(GraphCircuitColumns, p) == 0 && offsetof(GraphProofColumns, p) == 0 &&
                  offsetof(GraphCircuitColumns, stride) == sizeof(void*) * GE_MAX_COLUMNS &&
                  offsetof(GraphProofColumns, stride) == sizeof(void*) * GE_MAX_COLUMNS,
              "graph_run fills the pointers, then the strides, of whichever block the kind has");

// where graph_evaluate_kernel's lane takes what the program names (graph_interp.h: Source)
template <bool INTERNAL>
struct EvalSource {
  const GraphColumns* __restrict__ columns;
  const int32_t* __restrict__ rotations;
  uint64_t idx, mask;
  const uint32_t* __restrict__ prev;
  __device__ __forceinline__ uint32_t n_static() const { return columns->n_static; }
  __device__ __forceinline__ uint32_t dyn(uint32_t word) const { return columns->dyn[word]; }
  __device__ __forceinline__ Fr column(uint32_t src) const {
    const uint64_t row = graph_source_row(idx, (int64_t)rotations[gsrc_rot(src)], mask, gsrc_log_rows(src));
    const uint32_t* cell = columns->p[gsrc_column(src)] + row * 8;
    return INTERNAL ? ge_from_internal(cell) : ge_from_ext(cell);
  }
  __device__ __forceinline__ Fr previous() const { return ge_from_ext(prev); }
};

template <bool INTERNAL>
__global__ __launch_bounds__(GE_THREADS) void graph_evaluate_kernel(const GraphColumns* __restrict__ columns,
                                                                    const uint32_t* __restrict__ consts,
                                                                    const int32_t* __restrict__ rotations,
                                                                    const GraphCalc* __restrict__ calcs, uint32_t n_calc, uint32_t result_src,
                                                                    uint32_t result_prev, uint32_t* __restrict__ scratch,
                                                                    uint32_t* __restrict__ values, uint64_t size, uint32_t log_segment) {
  const uint32_t T = gridDim.x * GE_THREADS;
  const uint32_t lane_slot = blockIdx.x * GE_THREADS + threadIdx.x;
  const uint64_t mask = (1ull << log_segment) - 1;
  for (uint64_t idx = lane_slot; idx < size; idx += T) {
    uint32_t* vrow = values + idx * 8;
    const EvalSource<INTERNAL> from{columns, rotations, idx, mask, vrow};
    const Fr res = ge_run(from, consts, calcs, n_calc, result_src, result_prev, scratch, T, lane_slot);
    ge_store_ext(vrow, ge_reduce(res));
  }
}

// ---- host: program "compilation" (validation, Horner-free device form, liveness slot allocation) and launch ----
// Lower the validated program for one column format (graph_lower.h: copy propagation, forwarding and store elision, static
// bounds, slot allocation) and upload the device form.
static int graph_lower(const GraphProgram& g, bool internal_cols, GraphVariant& out) {
  GraphLowered low;
  graph_lower_host(g.calcs5.data(), g.calcs5.size() / 5, g.n_intermediates, internal_cols, low);
  const size_t n = low.calcs.size();
  out.n_calc = (uint32_t)n;
  out.n_slots = low.n_slots;
  out.result_prev = low.result_prev;
  out.result_src = low.result_src;
  HM_HIP_CHECK(hipMalloc(&out.d_calcs, std::max<size_t>(n, 1) * sizeof(GraphCalc)));
  if (n) HM_HIP_CHECK(hipMemcpy(out.d_calcs, low.calcs.data(), n * sizeof(GraphCalc), hipMemcpyHostToDevice));
  out.ready = true;
  return HM_OK;
}

int graph_create(DeviceCtx& ctx, const uint32_t* calcs5, size_t n_calc, const uint64_t* constants_ext, size_t n_const_static,
                 size_t n_dynamic, const int32_t* rotations, size_t n_rot, size_t n_columns, uint32_t n_intermediates,
                 uint64_t* out_handle) {
  if (const char* why = graph_validate(calcs5, n_calc, n_const_static, n_dynamic, n_rot, n_columns, n_intermediates))
    return hm_fail(HM_ERR_BAD_ARG, why);
  auto g = std::make_unique<GraphProgram>();
  g->n_columns = n_columns;
  g->n_static = (uint32_t)n_const_static;
  g->n_dynamic = (uint32_t)n_dynamic;
  g->n_intermediates = n_intermediates;
  g->calcs5.assign(calcs5, calcs5 + 5 * n_calc);
  g->consts_ext.assign(constants_ext, constants_ext + 4 * n_const_static);
  // constants -> internal form
  std::vector<uint32_t> c9(std::max<size_t>(n_const_static, 1) * 9, 0);
  for (size_t i = 0; i < n_const_static; ++i) host::fr_to_internal9(host::fr_load(constants_ext + 4 * i), &c9[9 * i]);
  const size_t b_const = c9.size() * 4, b_rot = std::max<size_t>(n_rot, 1) * 4;
  HM_HIP_CHECK(hipMalloc(&g->d_blob, b_const + b_rot));
  uint8_t* blob = (uint8_t*)g->d_blob;
  g->d_consts = (uint32_t*)blob;
  g->d_rot = (int32_t*)(blob + b_const);
  int rc = HM_OK;
  if (hipMemcpy(g->d_consts, c9.data(), b_const, hipMemcpyHostToDevice) != hipSuccess ||
      (n_rot && hipMemcpy(g->d_rot, rotations, n_rot * 4, hipMemcpyHostToDevice) != hipSuccess))
    rc = hm_fail(HM_ERR_HIP, "graph: upload failed");
  if (rc == HM_OK) rc = graph_lower(*g, false, g->variant[0]);    // the internal-columns form is lowered on first use
  if (rc != HM_OK) {
    graph_release(*g);
    return rc;
  }
  g->handle = ctx.next_handle++;
  *out_handle = g->handle;
  ctx.graphs.push_back(std::move(g));
  return HM_OK;
}

void graph_release(GraphProgram& g) {
  if (g.d_blob) (void)hipFree(g.d_blob);
  g.d_blob = nullptr;
  for (auto& v : g.variant) {
    if (v.d_calcs) (void)hipFree(v.d_calcs);
    v = GraphVariant{};
  }
}

// ---- several circuits of one constraint system in one launch (hm_graph_evaluate_circuits_dev) ----
// The program is linear in PreviousValue (graph_lower.h: graph_linear_shape): value = Prev * f^T + G(row).  `circuits`
// successive evaluations on the same values therefore fold as acc = acc * f^T + G_c(row), c = 0 .. circuits - 1, and the G_c
// are independent: one lane per (circuit, row) runs the program with PreviousValue = 0.  A workgroup covers 256 / C rows x
// C circuits (C a power of two the host chooses so that the grid fills the chip when rows alone do not); the C partials of
// a row meet in LDS, and the lane of circuit 0 folds them into an accumulator it keeps in registers across the groups of C
// circuits.  No partial goes to HBM.  Bounds: a partial is ge_reduce'd (< 3r) before it is written to LDS, the accumulator
// enters as a product output (ge_from_ext, < 3r), f^T is a canonical constant (< r); fe_mul takes inputs < 18r and leaves
// < 3r, the sum is < 6r and ge_reduce brings it back below 3r: the classes of one non-lazy MulAdd step of ge_run
// (host_check.cpp: hc_graph_circuits_replay tracks them).  Rows run fastest inside a workgroup (thread = circuit * rows + row),
// so that a wave reads consecutive cells of a column.
template <bool INTERNAL>
struct CircuitSource {
  const GraphCircuitColumns* __restrict__ columns;
  const int32_t* __restrict__ rotations;
  uint64_t idx, mask, circuit;
  __device__ __forceinline__ uint32_t n_static() const { return columns->n_static; }
  __device__ __forceinline__ uint32_t dyn(uint32_t word) const { return columns->dyn[word]; }
  __device__ __forceinline__ Fr column(uint32_t src) const {
    const uint64_t row = graph_source_row(idx, (int64_t)rotations[gsrc_rot(src)], mask, gsrc_log_rows(src));
    const uint32_t col = gsrc_column(src);
    const uint32_t* cell = columns->p[col] + columns->stride[col] * circuit + row * 8;
    return INTERNAL ? ge_from_internal(cell) : ge_from_ext(cell);
  }
  __device__ __forceinline__ Fr previous() const { return fe_zero<FrParams>(); }
};

template <bool INTERNAL>
__global__ __launch_bounds__(GE_THREADS) void graph_circuits_kernel(const GraphCircuitColumns* __restrict__ columns,
                                                                    const uint32_t* __restrict__ consts,
                                                                    const int32_t* __restrict__ rotations,
                                                                    const GraphCalc* __restrict__ calcs, uint32_t n_calc, uint32_t result_src,
                                                                    uint32_t result_prev, uint32_t* __restrict__ scratch,
                                                                    uint32_t* __restrict__ values, uint64_t size, uint32_t log_segment,
                                                                    uint32_t circuits, uint32_t log_c) {
  __shared__ uint32_t part[9 * GE_THREADS];            // [word][thread]: the group's partials
  const uint32_t C = 1u << log_c, rows_per = GE_THREADS >> log_c;
  const uint32_t T = gridDim.x * GE_THREADS;
  const uint32_t lane_slot = blockIdx.x * GE_THREADS + threadIdx.x;
  const uint32_t r = threadIdx.x & (rows_per - 1), cl = threadIdx.x / rows_per;
  const uint64_t mask = (1ull << log_segment) - 1;
  Fr fold;
#pragma unroll
  for (int i = 0; i < 9; ++i) fold.l[i] = columns->fold[i];
  HM_DECLARE(fold, 1.0);
  // the trip counts of both loops are the same for every thread of the workgroup: the barriers are reached by all
  for (uint64_t base = (uint64_t)blockIdx.x * rows_per; base < size; base += (uint64_t)gridDim.x * rows_per) {
    const uint64_t idx = base + r;
    const bool live = idx < size, folds = live && cl == 0;
    uint32_t* vrow = values + idx * 8;
    Fr acc = fe_zero<FrParams>();
    if (folds) acc = ge_from_ext(vrow);
    for (uint32_t c0 = 0; c0 < circuits; c0 += C) {
      if (live && c0 + cl < circuits) {
        const CircuitSource<INTERNAL> from{columns, rotations, idx, mask, (uint64_t)(c0 + cl)};
        const Fr g = ge_reduce(ge_run(from, consts, calcs, n_calc, result_src, result_prev, scratch, T, lane_slot));
#pragma unroll
        for (int i = 0; i < 9; ++i) part[i * GE_THREADS + threadIdx.x] = g.l[i];
      }
      __syncthreads();
      if (folds) {
        const uint32_t here = circuits - c0 < C ? circuits - c0 : C;
        for (uint32_t j = 0; j < here; ++j) {
          Fr p;
#pragma unroll
          for (int i = 0; i < 9; ++i) p.l[i] = part[i * GE_THREADS + j * rows_per + r];
          HM_DECLARE(p, 3.0);
          acc = ge_reduce(fe_add(fe_mul(acc, fold), p));
        }
      }
      __syncthreads();
    }
    if (folds) ge_store_ext(vrow, acc);
  }
}

// ---- several INDEPENDENT proofs of one constraint system in one launch (hm_graph_evaluate_proofs_dev) ----
// Every proof has its own per-call constants (theta, beta, gamma, y of its own transcript), its own columns (or a shared one at
// stride 0) and its own values: nothing is folded across proofs, PreviousValue is the proof's own, and any program is admitted.
// One lane per (proof, row), rows fastest (graph_lower.h: graph_proofs_*), so that a wave reads consecutive cells of a column.  The
// constants come from a device table of proofs x n_dynamic x 9 internal words that follows the column table in the slot's argument
// buffer.  A wave straddles proofs when a proof has fewer than 64 rows, so the table is read with an ordinary per-lane load
// (dyn_row is a per-lane pointer; nothing assumes it uniform).  The arithmetic is ge_run's, unchanged: no bound class arises
// that graph_evaluate_kernel does not have (constants enter as canonical internal words, < r; columns and PreviousValue as there).
template <bool INTERNAL>
struct ProofSource {
  const GraphProofColumns* __restrict__ columns;
  const int32_t* __restrict__ rotations;
  const uint32_t* __restrict__ dyn_table;
  uint64_t mask;
  uint32_t idx, proof, n_dynamic;             // idx: the row inside the proof (rows <= 2^32 and idx < rows)
  const uint32_t* __restrict__ prev;
  __device__ __forceinline__ uint32_t n_static() const { return columns->n_static; }
  __device__ __forceinline__ uint32_t dyn(uint32_t word) const { return dyn_table[graph_proofs_dyn(proof, n_dynamic, word)]; }   // per lane
  __device__ __forceinline__ Fr column(uint32_t src) const {
    const uint64_t row = graph_source_row(idx, (int64_t)rotations[gsrc_rot(src)], mask, gsrc_log_rows(src));
    const uint32_t col = gsrc_column(src);
    const uint32_t* cell = columns->p[col] + graph_proofs_cell(proof, row, columns->stride[col]);
    return INTERNAL ? ge_from_internal(cell) : ge_from_ext(cell);
  }
  __device__ __forceinline__ Fr previous() const { return ge_from_ext(prev); }
};

template <bool INTERNAL>
__global__ __launch_bounds__(GE_THREADS) void graph_proofs_kernel(const GraphProofColumns* __restrict__ columns,
                                                                  const uint32_t* __restrict__ dyn_table,
                                                                  const uint32_t* __restrict__ consts,
                                                                  const int32_t* __restrict__ rotations,
                                                                  const GraphCalc* __restrict__ calcs, uint32_t n_calc, uint32_t result_src,
                                                                  uint32_t result_prev, uint32_t* __restrict__ scratch,
                                                                  uint32_t* __restrict__ values, uint64_t values_stride, uint64_t size,
                                                                  uint64_t lanes, uint32_t log_segment) {
  const uint32_t T = gridDim.x * GE_THREADS;
  const uint32_t lane_slot = blockIdx.x * GE_THREADS + threadIdx.x;
  const uint64_t mask = (1ull << log_segment) - 1;
  const uint32_t n_dynamic = columns->n_dynamic;
  for (uint64_t lane = lane_slot; lane < lanes; lane += T) {
    const uint32_t proof = graph_proofs_proof(lane, size), idx = (uint32_t)(lane - (uint64_t)proof * size);
    uint32_t* vrow = values + graph_proofs_cell(proof, idx, values_stride);
    const ProofSource<INTERNAL> from{columns, rotations, dyn_table, mask, idx, proof, n_dynamic, vrow};
    const Fr res = ge_run(from, consts, calcs, n_calc, result_src, result_prev, scratch, T, lane_slot);
    ge_store_ext(vrow, ge_reduce(res));
  }
}

// ---- the one driver of the three kinds of call (hm_graph_evaluate*_dev, the quotient routes) ----
// 93 VGPRs: five waves per SIMD fit, i.e. five 256-lane workgroups per CU -- the interpreter's loads from the scratch
// (Infinity Cache latency) need them: measured on the MerkleSumTree program over 2^21 rows, 512 / 768 / 1024 / 1280 / 2048
// workgroups: 12.4 / 10.5 / 10.3 / 9.9 / 10.0 ms.  At 1280 the kernel issues 4.6e11 VALU wave-instructions per second
// (SQ_INSTS_VALU 4.21e9 in 9.2 ms): it is bound by VALU issue like K3 and the NTT, no longer by its scratch traffic.
uint32_t graph_max_blocks() {      // the only reader of HALO2_MI355X_GRAPH_BLOCKS (mock.hip asks here); never below one block
  static const uint32_t max_blocks = [] { const char* v = std::getenv("HALO2_MI355X_GRAPH_BLOCKS"); return std::max<uint32_t>((uint32_t)(v && *v ? std::atoi(v) : 1280), 1); }();
  return max_blocks;
}

// In order: the check (graph_lower.h: graph_check_call), for circuits the linear shape and f^steps, the column format's variant, the
// plan (graph_launch_plan), the argument block on the host -- every refusal and everything that can throw lies before the slot is
// taken -- then the slot's scratch, the block's upload, the launch.  aux_scope records the slot's event whatever comes of those.
int graph_run(DeviceCtx& ctx, GraphProgram& g, const GraphCall& c, hipStream_t stream) {
  if (const char* why = graph_check_call(c, g.n_columns, g.n_dynamic)) return hm_fail(HM_ERR_BAD_ARG, why);
  host::Fr4 f_pow = host::FR_ONE;
  if (c.kind == GRAPH_CIRCUITS) {
    // The program is linear in PreviousValue: f^steps on the host (Montgomery words in, Montgomery words out); steps >= 1
    uint32_t factor_src = 0, steps = 0;
    if (const char* why = graph_linear_shape(g.calcs5.data(), g.calcs5.size() / 5, g.n_intermediates, &factor_src, &steps))
      return hm_fail(HM_ERR_BAD_ARG, why);
    const uint32_t fi = gsrc_index(factor_src);
    const host::Fr4 f = host::fr_load(fi < g.n_static ? &g.consts_ext[4 * (size_t)fi] : c.dyn_ext + 4 * (size_t)(fi - g.n_static));
    f_pow = f;
    for (uint32_t i = 1; i < steps; ++i) f_pow = host::fr_mul(f_pow, f);
  }
  const bool internal_cols = (c.flags & HM_GRAPH_COLUMNS_INTERNAL) != 0;
  GraphVariant& v = g.variant[internal_cols ? 1 : 0];
  if (!v.ready) {
    const int rc = graph_lower(g, internal_cols, v);
    if (rc != HM_OK) return rc;
  }
  const GraphPlan p = graph_launch_plan(c.kind, (uint64_t)c.segments << c.log_size, c.units, v.n_slots, c.n_dyn, graph_max_blocks());
  // the argument block: the kind's column table -- p, then stride where the kind has one, then the constants -- and, for proofs,
  // the constant table behind it (one upload)
  std::vector<uint32_t> block(p.args_bytes / 4, 0);
  const uint32_t** ptrs = reinterpret_cast<const uint32_t**>(block.data());
  uint64_t* strides = reinterpret_cast<uint64_t*>(ptrs + GE_MAX_COLUMNS);
  for (size_t i = 0; i < c.n_columns; ++i) {
    ptrs[i] = (const uint32_t*)c.bases[i];
    if (c.strides) strides[i] = c.strides[i];
  }
  uint32_t* dyn = nullptr;
  if (c.kind == GRAPH_SINGLE) {
    GraphColumns& cols = *reinterpret_cast<GraphColumns*>(block.data());
    cols.n_static = g.n_static, dyn = cols.dyn;
  } else if (c.kind == GRAPH_CIRCUITS) {
    GraphCircuitColumns& cols = *reinterpret_cast<GraphCircuitColumns*>(block.data());
    cols.n_static = g.n_static, dyn = cols.dyn;
    host::fr_to_internal9(f_pow, cols.fold);
  } else {
    GraphProofColumns& cols = *reinterpret_cast<GraphProofColumns*>(block.data());
    cols.n_static = g.n_static, cols.n_dynamic = (uint32_t)c.n_dyn, dyn = block.data() + sizeof(GraphProofColumns) / 4;
  }
  for (size_t i = 0; i < (c.kind == GRAPH_PROOFS ? c.units : 1) * c.n_dyn; ++i) host::fr_to_internal9(host::fr_load(c.dyn_ext + 4 * i), dyn + 9 * i);
  return aux_scope(ctx, stream, [&](AuxSlot& slot) -> int {
    uint32_t* buf = (uint32_t*)aux_buffer(slot, AuxBuf::scratch, p.scratch_bytes, "graph");
    uint8_t* d_block = buf ? (uint8_t*)aux_buffer(slot, AuxBuf::args, p.args_bytes, "graph") : nullptr;
    if (!d_block) return HM_ERR_HIP;
    // pageable source: the runtime has taken its copy of `block` when this returns; the copy itself is ordered on `stream`
    // ahead of the launch and behind the previous launch that read the buffer
    HM_HIP_CHECK(hipMemcpyAsync(d_block, block.data(), p.args_bytes, hipMemcpyHostToDevice, stream));
    if (c.kind == GRAPH_SINGLE)
      ge_launch(internal_cols, graph_evaluate_kernel<true>, graph_evaluate_kernel<false>, p.blocks, stream, d_block, g.d_consts, g.d_rot, v.d_calcs,
                v.n_calc, v.result_src, v.result_prev, buf, c.d_values, p.size, c.log_size);
    else if (c.kind == GRAPH_CIRCUITS)
      ge_launch(internal_cols, graph_circuits_kernel<true>, graph_circuits_kernel<false>, p.blocks, stream, d_block, g.d_consts, g.d_rot, v.d_calcs,
                v.n_calc, v.result_src, v.result_prev, buf, c.d_values, p.size, c.log_size, c.units, p.log_c);
    else
      ge_launch(internal_cols, graph_proofs_kernel<true>, graph_proofs_kernel<false>, p.blocks, stream, d_block, d_block + sizeof(GraphProofColumns),
                g.d_consts, g.d_rot, v.d_calcs, v.n_calc, v.result_src, v.result_prev, buf, c.d_values, c.units > 1 ? c.values_stride : 0, p.size,
                p.lanes, c.log_size);
    HM_HIP_CHECK(hipGetLastError());
    return HM_OK;
  });
}
}  // namespace hm

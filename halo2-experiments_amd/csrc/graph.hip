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
// per-call constants through it.
struct GraphColumns {
  const uint32_t* p[GE_MAX_COLUMNS];
  uint32_t dyn[GE_MAX_DYN * 9];   // challenges, beta, gamma, theta, y ... of THIS proof, internal form
  uint32_t n_static;              // constants [0, n_static) come from the program, [n_static, ..) from dyn
};

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
    // two's complement: a negative rotation wraps -- inside the row's SEGMENT (mask = segment length - 1; one segment = the
    // whole domain in the ordinary call, one coset of the extended domain in hm_graph_evaluate_segments_dev)
    uint64_t row = (idx & ~mask) | ((idx + (uint64_t)(int64_t)rotations[gsrc_rot(src)]) & mask);
    const uint32_t lr = gsrc_log_rows(src);          // a short column (the vanishing polynomial's inverse pattern) is periodic
    if (lr != 0) row &= (1ull << lr) - 1ull;
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
    uint32_t w[8];
    fe_to_ext(w, ge_reduce(res));
    uint4* dst = reinterpret_cast<uint4*>(vrow);
    dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
    dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
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

// rows = segments << log_segment; rotations wrap inside a segment (segments == 1: the ordinary evaluation over 2^log_segment rows)
int graph_evaluate(DeviceCtx& ctx, GraphProgram& g, const void* const* d_columns, size_t n_columns, const uint64_t* dyn_ext,
                   size_t n_dyn, uint32_t log_size, uint32_t segments, void* d_values, uint32_t flags, hipStream_t stream) {
  if (flags & ~(uint32_t)HM_GRAPH_COLUMNS_INTERNAL) return hm_fail(HM_ERR_BAD_ARG, "graph: unknown flag");
  const bool internal_cols = (flags & HM_GRAPH_COLUMNS_INTERNAL) != 0;
  GraphVariant& v = g.variant[internal_cols ? 1 : 0];
  if (!v.ready) {
    const int rc = graph_lower(g, internal_cols, v);
    if (rc != HM_OK) return rc;
  }
  if (n_columns != g.n_columns) return hm_fail(HM_ERR_BAD_ARG, "graph: the program was built for another number of columns");
  if (n_dyn != g.n_dynamic) return hm_fail(HM_ERR_BAD_ARG, "graph: the program was built for another number of per-call constants");
  if (log_size > 30) return hm_fail(HM_ERR_BAD_ARG, "graph: log_size > 30");
  if (segments == 0 || ((uint64_t)segments << log_size) > (1ull << 32)) return hm_fail(HM_ERR_BAD_ARG, "graph: segments must be >= 1 and rows <= 2^32");
  const uint64_t size = (uint64_t)segments << log_size;
  // enough lanes to fill the chip, few enough that the intermediates' scratch stays cache-sized
  // 93 VGPRs: five waves per SIMD fit, i.e. five 256-lane workgroups per CU -- the interpreter's loads from the scratch
  // (Infinity Cache latency) need them: measured on the MerkleSumTree program over 2^21 rows, 512 / 768 / 1024 / 1280 / 2048
  // workgroups: 12.4 / 10.5 / 10.3 / 9.9 / 10.0 ms.  At 1280 the kernel issues 4.6e11 VALU wave-instructions per second
  // (SQ_INSTS_VALU 4.21e9 in 9.2 ms): it is bound by VALU issue like K3 and the NTT, no longer by its scratch traffic.
  static const uint32_t max_blocks = [] { const char* v = std::getenv("HALO2_MI355X_GRAPH_BLOCKS"); return (uint32_t)(v && *v ? std::atoi(v) : 1280); }();
  uint32_t blocks = (uint32_t)std::min<uint64_t>((size + GE_THREADS - 1) / GE_THREADS, max_blocks);
  const uint32_t T = blocks * GE_THREADS;
  AuxSlot* slot = aux_acquire(ctx, stream);
  if (!slot) return HM_ERR_HIP;
  const size_t b_scratch = (size_t)v.n_slots * 9 * T * 4;
  uint8_t* buf = (uint8_t*)slot->scratch.ensure(b_scratch);
  if (!buf) return hm_fail(HM_ERR_HIP, "graph: scratch allocation failed");
  GraphColumns cols;
  std::memset(&cols, 0, sizeof cols);
  for (size_t i = 0; i < n_columns; ++i) {
    if (!d_columns[i]) return hm_fail(HM_ERR_BAD_ARG, "graph: null column pointer");
    cols.p[i] = (const uint32_t*)d_columns[i];
  }
  cols.n_static = g.n_static;
  for (size_t i = 0; i < n_dyn; ++i) host::fr_to_internal9(host::fr_load(dyn_ext + 4 * i), &cols.dyn[9 * i]);
  GraphColumns* d_cols = (GraphColumns*)slot->args.ensure(sizeof(GraphColumns));
  if (!d_cols) return hm_fail(HM_ERR_HIP, "graph: argument buffer allocation failed");
  // pageable source: the runtime has taken its copy of `cols` when this returns; the copy itself is ordered on `stream`
  // ahead of the launch and behind the previous launch that read the buffer
  HM_HIP_CHECK(hipMemcpyAsync(d_cols, &cols, sizeof cols, hipMemcpyHostToDevice, stream));
  if (internal_cols)
    hipLaunchKernelGGL(graph_evaluate_kernel<true>, dim3(blocks), dim3(GE_THREADS), 0, stream, (const GraphColumns*)d_cols,
                       (const uint32_t*)g.d_consts, (const int32_t*)g.d_rot, (const GraphCalc*)v.d_calcs, v.n_calc, v.result_src,
                       v.result_prev, (uint32_t*)buf, (uint32_t*)d_values, size, log_size);
  else
    hipLaunchKernelGGL(graph_evaluate_kernel<false>, dim3(blocks), dim3(GE_THREADS), 0, stream, (const GraphColumns*)d_cols,
                       (const uint32_t*)g.d_consts, (const int32_t*)g.d_rot, (const GraphCalc*)v.d_calcs, v.n_calc, v.result_src,
                       v.result_prev, (uint32_t*)buf, (uint32_t*)d_values, size, log_size);
  HM_HIP_CHECK(hipGetLastError());
  return aux_release(ctx, slot, stream);
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
struct GraphCircuitColumns {
  const uint32_t* p[GE_MAX_COLUMNS];
  uint64_t stride[GE_MAX_COLUMNS];   // u32 words from circuit c's column to circuit c + 1's; 0: one column for all circuits
  uint32_t dyn[GE_MAX_DYN * 9];
  uint32_t fold[9];                  // f^T, internal form
  uint32_t n_static;
};

template <bool INTERNAL>
struct CircuitSource {
  const GraphCircuitColumns* __restrict__ columns;
  const int32_t* __restrict__ rotations;
  uint64_t idx, mask, circuit;
  __device__ __forceinline__ uint32_t n_static() const { return columns->n_static; }
  __device__ __forceinline__ uint32_t dyn(uint32_t word) const { return columns->dyn[word]; }
  __device__ __forceinline__ Fr column(uint32_t src) const {
    uint64_t row = (idx & ~mask) | ((idx + (uint64_t)(int64_t)rotations[gsrc_rot(src)]) & mask);
    const uint32_t lr = gsrc_log_rows(src);
    if (lr != 0) row &= (1ull << lr) - 1ull;
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
    if (folds) {
      uint32_t w[8];
      fe_to_ext(w, acc);
      uint4* dst = reinterpret_cast<uint4*>(vrow);
      dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
      dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
    }
  }
}

int graph_evaluate_circuits(DeviceCtx& ctx, GraphProgram& g, const void* const* column_bases, const uint64_t* column_strides, size_t n_columns,
                            size_t circuits, const uint64_t* dyn_ext, size_t n_dyn, uint32_t log_size, uint32_t segments, void* d_values,
                            uint32_t flags, hipStream_t stream) {
  if (flags & ~(uint32_t)HM_GRAPH_COLUMNS_INTERNAL) return hm_fail(HM_ERR_BAD_ARG, "graph: unknown flag");
  if (circuits == 0) return hm_fail(HM_ERR_BAD_ARG, "graph: circuits must be >= 1");
  if (n_columns > GE_MAX_COLUMNS) return hm_fail(HM_ERR_BAD_ARG, "graph: more columns than the column table holds");
  if (n_columns != g.n_columns) return hm_fail(HM_ERR_BAD_ARG, "graph: the program was built for another number of columns");
  if (n_dyn != g.n_dynamic) return hm_fail(HM_ERR_BAD_ARG, "graph: the program was built for another number of per-call constants");
  if (log_size > 30) return hm_fail(HM_ERR_BAD_ARG, "graph: log_size > 30");
  if (segments == 0 || ((uint64_t)segments << log_size) > (1ull << 32)) return hm_fail(HM_ERR_BAD_ARG, "graph: segments must be >= 1 and rows <= 2^32");
  const uint64_t size = (uint64_t)segments << log_size;
  if (circuits > (1ull << 32) / size) return hm_fail(HM_ERR_BAD_ARG, "graph: circuits * rows > 2^32");
  if ((uintptr_t)d_values % 16) return hm_fail(HM_ERR_BAD_ARG, "graph: the values are not 16-byte aligned");
  for (size_t i = 0; i < n_columns; ++i) {
    if (!column_bases[i]) return hm_fail(HM_ERR_BAD_ARG, "graph: null column pointer");
    if ((uintptr_t)column_bases[i] % 16) return hm_fail(HM_ERR_BAD_ARG, "graph: a column base is not 16-byte aligned");
    if (column_strides[i] % 4) return hm_fail(HM_ERR_BAD_ARG, "graph: a column stride is not a multiple of 4 words");
  }
  uint32_t factor_src = 0, steps = 0;
  if (const char* why = graph_linear_shape(g.calcs5.data(), g.calcs5.size() / 5, g.n_intermediates, &factor_src, &steps))
    return hm_fail(HM_ERR_BAD_ARG, why);
  const bool internal_cols = (flags & HM_GRAPH_COLUMNS_INTERNAL) != 0;
  GraphVariant& v = g.variant[internal_cols ? 1 : 0];
  if (!v.ready) {
    const int rc = graph_lower(g, internal_cols, v);
    if (rc != HM_OK) return rc;
  }
  // f^steps on the host (Montgomery words in, Montgomery words out); steps >= 1
  const uint32_t fi = gsrc_index(factor_src);
  const host::Fr4 f = host::fr_load(fi < g.n_static ? &g.consts_ext[4 * (size_t)fi] : dyn_ext + 4 * (size_t)(fi - g.n_static));
  host::Fr4 f_pow = f;
  for (uint32_t i = 1; i < steps; ++i) f_pow = host::fr_mul(f_pow, f);
  // C circuits side by side in a workgroup: as many as it takes for the grid to reach graph_evaluate's block count, no more
  // than the circuits there are.  circuits = 1 gives C = 1: graph_evaluate_kernel's shape.
  static const uint32_t max_blocks = [] { const char* e = std::getenv("HALO2_MI355X_GRAPH_BLOCKS"); return (uint32_t)(e && *e ? std::atoi(e) : 1280); }();
  uint32_t log_c = 0;
  while (log_c < 8 && (1ull << log_c) < circuits && ((size << log_c) + GE_THREADS - 1) / GE_THREADS < max_blocks) ++log_c;
  const uint64_t rows_per = GE_THREADS >> log_c;
  const uint32_t blocks = (uint32_t)std::min<uint64_t>((size + rows_per - 1) / rows_per, max_blocks);
  const uint32_t T = blocks * GE_THREADS;
  AuxSlot* slot = aux_acquire(ctx, stream);
  if (!slot) return HM_ERR_HIP;
  const size_t b_scratch = (size_t)v.n_slots * 9 * T * 4;
  uint8_t* buf = (uint8_t*)slot->scratch.ensure(b_scratch);
  if (!buf) return hm_fail(HM_ERR_HIP, "graph: scratch allocation failed");
  GraphCircuitColumns cols;
  std::memset(&cols, 0, sizeof cols);
  for (size_t i = 0; i < n_columns; ++i) {
    cols.p[i] = (const uint32_t*)column_bases[i];
    cols.stride[i] = column_strides[i];
  }
  cols.n_static = g.n_static;
  for (size_t i = 0; i < n_dyn; ++i) host::fr_to_internal9(host::fr_load(dyn_ext + 4 * i), &cols.dyn[9 * i]);
  host::fr_to_internal9(f_pow, cols.fold);
  GraphCircuitColumns* d_cols = (GraphCircuitColumns*)slot->args.ensure(sizeof(GraphCircuitColumns));
  if (!d_cols) return hm_fail(HM_ERR_HIP, "graph: argument buffer allocation failed");
  HM_HIP_CHECK(hipMemcpyAsync(d_cols, &cols, sizeof cols, hipMemcpyHostToDevice, stream));
  if (internal_cols)
    hipLaunchKernelGGL(graph_circuits_kernel<true>, dim3(blocks), dim3(GE_THREADS), 0, stream, (const GraphCircuitColumns*)d_cols,
                       (const uint32_t*)g.d_consts, (const int32_t*)g.d_rot, (const GraphCalc*)v.d_calcs, v.n_calc, v.result_src,
                       v.result_prev, (uint32_t*)buf, (uint32_t*)d_values, size, log_size, (uint32_t)circuits, log_c);
  else
    hipLaunchKernelGGL(graph_circuits_kernel<false>, dim3(blocks), dim3(GE_THREADS), 0, stream, (const GraphCircuitColumns*)d_cols,
                       (const uint32_t*)g.d_consts, (const int32_t*)g.d_rot, (const GraphCalc*)v.d_calcs, v.n_calc, v.result_src,
                       v.result_prev, (uint32_t*)buf, (uint32_t*)d_values, size, log_size, (uint32_t)circuits, log_c);
  HM_HIP_CHECK(hipGetLastError());
  return aux_release(ctx, slot, stream);
}

// ---- several INDEPENDENT proofs of one constraint system in one launch (hm_graph_evaluate_proofs_dev) ----
// Every proof has its own per-call constants (theta, beta, gamma, y of its own transcript), its own columns (or a shared one at
// stride 0) and its own values: nothing is folded across proofs, PreviousValue is the proof's own, and any program is admitted.
// One lane per (proof, row), rows fastest (graph_lower.h: graph_proofs_*), so that a wave reads consecutive cells of a column.  The
// constants come from a device table of proofs x n_dynamic x 9 internal words that follows the column table in the slot's argument
// buffer.  A wave straddles proofs when a proof has fewer than 64 rows, so the table is read with an ordinary per-lane load
// (dyn_row is a per-lane pointer; nothing assumes it uniform).  The arithmetic is ge_run's, unchanged: no bound class arises
// that graph_evaluate_kernel does not have (constants enter as canonical internal words, < r; columns and PreviousValue as there).
struct GraphProofColumns {
  const uint32_t* p[GE_MAX_COLUMNS];
  uint64_t stride[GE_MAX_COLUMNS];   // u32 words from proof b's column to proof b + 1's; 0: one column for all proofs
  uint32_t n_static, n_dynamic;
};

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
    const uint64_t row = graph_proofs_row(idx, (int64_t)rotations[gsrc_rot(src)], mask, gsrc_log_rows(src));
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
    uint32_t w[8];
    fe_to_ext(w, ge_reduce(res));
    uint4* dst = reinterpret_cast<uint4*>(vrow);
    dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
    dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
  }
}

int graph_evaluate_proofs(DeviceCtx& ctx, GraphProgram& g, const void* const* column_bases, const uint64_t* column_strides, size_t n_columns,
                          size_t proofs, const uint64_t* dyn_ext, size_t n_dyn, uint32_t log_size, uint32_t segments, void* d_values,
                          uint64_t values_stride, uint32_t flags, hipStream_t stream) {
  if (flags & ~(uint32_t)HM_GRAPH_COLUMNS_INTERNAL) return hm_fail(HM_ERR_BAD_ARG, "graph: unknown flag");
  if (proofs == 0) return hm_fail(HM_ERR_BAD_ARG, "graph: proofs must be >= 1");
  if (n_columns > GE_MAX_COLUMNS) return hm_fail(HM_ERR_BAD_ARG, "graph: more columns than the column table holds");
  if (n_columns != g.n_columns) return hm_fail(HM_ERR_BAD_ARG, "graph: the program was built for another number of columns");
  if (n_dyn != g.n_dynamic) return hm_fail(HM_ERR_BAD_ARG, "graph: the program was built for another number of per-call constants");
  if (log_size > 30) return hm_fail(HM_ERR_BAD_ARG, "graph: log_size > 30");
  if (segments == 0 || ((uint64_t)segments << log_size) > (1ull << 32)) return hm_fail(HM_ERR_BAD_ARG, "graph: segments must be >= 1 and rows <= 2^32");
  const uint64_t size = (uint64_t)segments << log_size;
  if (proofs > (1ull << 32) / size) return hm_fail(HM_ERR_BAD_ARG, "graph: proofs * rows > 2^32");
  if ((uintptr_t)d_values % 16) return hm_fail(HM_ERR_BAD_ARG, "graph: the values are not 16-byte aligned");
  if (proofs > 1 && (values_stride < size * 8 || values_stride % 4))
    return hm_fail(HM_ERR_BAD_ARG, "graph: the values stride must be a multiple of 4 words and hold the rows of one proof");
  for (size_t i = 0; i < n_columns; ++i) {
    if (!column_bases[i]) return hm_fail(HM_ERR_BAD_ARG, "graph: null column pointer");
    if ((uintptr_t)column_bases[i] % 16) return hm_fail(HM_ERR_BAD_ARG, "graph: a column base is not 16-byte aligned");
    if (column_strides[i] % 4) return hm_fail(HM_ERR_BAD_ARG, "graph: a column stride is not a multiple of 4 words");
  }
  const bool internal_cols = (flags & HM_GRAPH_COLUMNS_INTERNAL) != 0;
  GraphVariant& v = g.variant[internal_cols ? 1 : 0];
  if (!v.ready) {
    const int rc = graph_lower(g, internal_cols, v);
    if (rc != HM_OK) return rc;
  }
  // graph_evaluate's grid cap and scratch rule, the lanes being proofs * rows
  static const uint32_t max_blocks = [] { const char* e = std::getenv("HALO2_MI355X_GRAPH_BLOCKS"); return (uint32_t)(e && *e ? std::atoi(e) : 1280); }();
  const uint64_t lanes = (uint64_t)proofs * size;
  const uint32_t blocks = (uint32_t)std::min<uint64_t>((lanes + GE_THREADS - 1) / GE_THREADS, max_blocks);
  const uint32_t T = blocks * GE_THREADS;
  AuxSlot* slot = aux_acquire(ctx, stream);
  if (!slot) return HM_ERR_HIP;
  const size_t b_scratch = (size_t)v.n_slots * 9 * T * 4;
  uint8_t* buf = (uint8_t*)slot->scratch.ensure(b_scratch);
  if (!buf) return hm_fail(HM_ERR_HIP, "graph: scratch allocation failed");
  // the argument block: the column table, then the constant table (one upload)
  const size_t n_table = std::max<size_t>(proofs * n_dyn, 1) * 9;
  std::vector<uint32_t> block(sizeof(GraphProofColumns) / 4 + n_table, 0);
  GraphProofColumns& cols = *reinterpret_cast<GraphProofColumns*>(block.data());
  for (size_t i = 0; i < n_columns; ++i) {
    cols.p[i] = (const uint32_t*)column_bases[i];
    cols.stride[i] = column_strides[i];
  }
  cols.n_static = g.n_static;
  cols.n_dynamic = (uint32_t)n_dyn;
  uint32_t* table = block.data() + sizeof(GraphProofColumns) / 4;
  for (size_t i = 0; i < proofs * n_dyn; ++i) host::fr_to_internal9(host::fr_load(dyn_ext + 4 * i), table + 9 * i);
  uint8_t* d_block = (uint8_t*)slot->args.ensure(block.size() * 4);
  if (!d_block) return hm_fail(HM_ERR_HIP, "graph: argument buffer allocation failed");
  // pageable source: the runtime has taken its copy of `block` when this returns (graph_evaluate)
  HM_HIP_CHECK(hipMemcpyAsync(d_block, block.data(), block.size() * 4, hipMemcpyHostToDevice, stream));
  const GraphProofColumns* d_cols = (const GraphProofColumns*)d_block;
  const uint32_t* d_table = (const uint32_t*)(d_block + sizeof(GraphProofColumns));
  const uint64_t vstride = proofs > 1 ? values_stride : 0;
  if (internal_cols)
    hipLaunchKernelGGL(graph_proofs_kernel<true>, dim3(blocks), dim3(GE_THREADS), 0, stream, d_cols, d_table, (const uint32_t*)g.d_consts,
                       (const int32_t*)g.d_rot, (const GraphCalc*)v.d_calcs, v.n_calc, v.result_src, v.result_prev, (uint32_t*)buf,
                       (uint32_t*)d_values, vstride, size, lanes, log_size);
  else
    hipLaunchKernelGGL(graph_proofs_kernel<false>, dim3(blocks), dim3(GE_THREADS), 0, stream, d_cols, d_table, (const uint32_t*)g.d_consts,
                       (const int32_t*)g.d_rot, (const GraphCalc*)v.d_calcs, v.n_calc, v.result_src, v.result_prev, (uint32_t*)buf,
                       (uint32_t*)d_values, vstride, size, lanes, log_size);
  HM_HIP_CHECK(hipGetLastError());
  return aux_release(ctx, slot, stream);
}

}  // namespace hm

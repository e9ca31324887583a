// mock.hip -- MockProver::verify for a BATCH of witnesses on the device (upstream halo2_proofs dev.rs: every gate polynomial on
// every usable row, both cells of every copy constraint, every lookup input in its table; mock_prover.py is the caller).
//
// The witnesses of m users lie as the witness kernels leave them: m x num_advice x n elements of advice, m x rows_i of every
// instance column, the fixed columns once.  One BATCHED column table names them -- per column { base, words per user, rows
// present }: a fixed column has stride 0, an instance column reads as zero above its rows (no m x n instance array exists) -- and
// travels in a device buffer like GraphColumns (graph.hip says why).  Three passes read the batch through it:
//   gates    graph_check_kernel<SINK_NONZERO>: an hm_graph_create program (graph_interp.h, the interpreter of
//            graph_evaluate_kernel) on one lane per (user, usable row), or per entry of a list of such lanes; a rotation wraps
//            inside the user's own 2^k rows; the value is not stored: != 0 mod r is a failure
//   lookups  graph_check_kernel<SINK_NOT_IN_TABLE>: the value's canonical integer (one product) is binary-searched in the sorted
//            keys of the table (lookup.hip: convert + sort)
//   copies   one lane per (user, copy): the two cells' words compared
// Failures are APPENDED: one ballot per wave, one atomicAdd per wave with a failure on the call's counter, every failing lane
// writes its record if its slot is below the capacity -- the counter keeps counting, so the total is exact whatever the
// capacity -- and sets its user's byte in a flag array.  Nothing else is written.
// The kernels and the drivers mock_program_run / mock_copies_run; the sorted keys come from lookup.hip (lookup_sorted_keys_run).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "g1.h"
#include "graph_interp.h"
#include "graph_lower.h"
#include "hm_internal.h"
#include "host_fr.h"
#include "mock_check.h"

namespace hm {

struct CheckColumns {
  const uint32_t* p[GE_MAX_COLUMNS];
  uint64_t stride[GE_MAX_COLUMNS];     // words from one user's column to the next user's (0: one column for all)
  uint32_t rows[GE_MAX_COLUMNS];       // rows present; a cell above them is zero
  uint32_t perm[GE_MAX_COLUMNS];       // the copies' pass: entry of this table that permutation column j is
  uint32_t dyn[GE_MAX_DYN * 9];        // the per-call constants (y ...), internal form
  uint32_t n_static;
};

struct CheckSink {
  uint64_t* records;
  uint64_t cap;
  unsigned long long* counter;
  uint8_t* flags;
};

// the whole wave comes here together
__device__ __forceinline__ void mock_append(bool fail, uint64_t rec, const CheckSink& sink) {
  const uint64_t ballot = __ballot(fail);
  if (ballot == 0) return;
  const uint32_t lane = threadIdx.x & 63u, leader = (uint32_t)__builtin_ctzll(ballot);
  unsigned long long base = 0;
  if (lane == leader) base = atomicAdd(sink.counter, (unsigned long long)__popcll(ballot));
  base = __shfl(base, (int)leader, 64);
  if (fail) {
    const uint64_t slot = base + (uint64_t)__popcll(ballot & ((1ull << lane) - 1ull));
    if (slot < sink.cap) sink.records[slot] = rec;
    sink.flags[mock_record_user(rec)] = 1;
  }
}

__device__ __forceinline__ bool mock_cell_words(const CheckColumns* __restrict__ cols, uint32_t c, uint64_t user, uint32_t row, uint4& lo,
                                                uint4& hi) {
  if (row >= cols->rows[c]) {
    lo = hi = make_uint4(0, 0, 0, 0);
    return false;
  }
  const uint4* q = reinterpret_cast<const uint4*>(cols->p[c] + user * cols->stride[c] + (uint64_t)row * 8);
  lo = q[0];
  hi = q[1];
  return true;
}

struct CheckSource {
  const CheckColumns* __restrict__ cols;
  const int32_t* __restrict__ rotations;
  uint64_t user;                       // inside the table
  uint32_t row, row_mask;
  __device__ __forceinline__ uint32_t n_static() const { return cols->n_static; }
  __device__ __forceinline__ uint32_t dyn(uint32_t word) const { return cols->dyn[word]; }
  __device__ __forceinline__ Fr column(uint32_t src) const {
    uint32_t r = (row + (uint32_t)rotations[gsrc_rot(src)]) & row_mask;     // wraps inside the user's own rows
    const uint32_t lr = gsrc_log_rows(src);
    if (lr != 0) r &= (1u << lr) - 1u;
    const uint32_t c = gsrc_column(src);
    if (r >= cols->rows[c]) {
      Fr z = fe_zero<FrParams>();
      HM_DECLARE(z, 1.0);
      return z;
    }
    return ge_from_ext(cols->p[c] + user * cols->stride[c] + (uint64_t)r * 8);
  }
  __device__ __forceinline__ Fr previous() const {
    Fr z = fe_zero<FrParams>();
    HM_DECLARE(z, 1.0);
    return z;
  }
};

constexpr int SINK_NONZERO = 0, SINK_NOT_IN_TABLE = 1;

// lanes: m * usable (user, row) pairs in user-major order, or the entries of `list` (records of an earlier pass; one that names a
// user or row outside the batch is skipped).  Records carry user_base + the user's index in the table.
template <int SINK>
__global__ __launch_bounds__(GE_THREADS) void graph_check_kernel(const CheckColumns* __restrict__ cols, const uint32_t* __restrict__ consts,
                                                                 const int32_t* __restrict__ rotations, const GraphCalc* __restrict__ calcs,
                                                                 uint32_t n_calc, uint32_t result_src, uint32_t result_prev,
                                                                 uint32_t* __restrict__ scratch, uint64_t lanes, uint32_t usable, uint32_t log_n,
                                                                 uint32_t m, uint32_t user_base, const uint64_t* __restrict__ list,
                                                                 const uint32_t* __restrict__ keys, uint64_t n_keys, CheckSink sink) {
  const uint32_t T = gridDim.x * GE_THREADS;
  const uint32_t lane_slot = blockIdx.x * GE_THREADS + threadIdx.x;
  for (uint64_t base = (uint64_t)blockIdx.x * GE_THREADS; base < lanes; base += T) {      // the same trip count for a whole workgroup
    const uint64_t idx = base + threadIdx.x;
    bool on = idx < lanes, fail = false;
    uint32_t user = 0, row = 0;
    if (on) {
      if (list) {
        const uint64_t rec = list[idx];
        user = mock_record_user(rec) - user_base;
        row = mock_record_index(rec);
        on = user < m && row < usable;
      } else {
        user = (uint32_t)(idx / usable);
        row = (uint32_t)(idx % usable);
      }
    }
    if (on) {
      const CheckSource from{cols, rotations, (uint64_t)user, row, (1u << log_n) - 1u};
      const Fr res = ge_reduce(ge_run(from, consts, calcs, n_calc, result_src, result_prev, scratch, T, lane_slot));
      if (SINK == SINK_NONZERO) {
        fail = !fe_is_zero_mod(res);
      } else {
        uint32_t key[8];
        mock_value_key(key, res);
        fail = !mock_key_found(keys, n_keys, key);
      }
    }
    mock_append(fail, mock_record(user_base + user, row), sink);
  }
}

// lanes = m * n_copies; d_pairs: cell ids as keygen's (permutation column * 2^k + row); a pair naming a column outside the
// permutation is skipped; a copy between two columns shared by all users is checked for user 0 only
__global__ __launch_bounds__(GE_THREADS) void mock_copies_kernel(const CheckColumns* __restrict__ cols, const uint32_t* __restrict__ d_pairs,
                                                                 uint32_t n_copies, uint32_t n_perm, uint32_t log_n, uint64_t lanes,
                                                                 CheckSink sink) {
  const uint32_t T = gridDim.x * GE_THREADS;
  for (uint64_t base = (uint64_t)blockIdx.x * GE_THREADS; base < lanes; base += T) {
    const uint64_t idx = base + threadIdx.x;
    bool fail = false;
    uint32_t user = 0, ci = 0;
    if (idx < lanes) {
      user = (uint32_t)(idx / n_copies);
      ci = (uint32_t)(idx % n_copies);
      const uint32_t a = d_pairs[2 * (size_t)ci], b = d_pairs[2 * (size_t)ci + 1];
      const uint32_t ja = a >> log_n, jb = b >> log_n, row_mask = (1u << log_n) - 1u;
      if (ja < n_perm && jb < n_perm) {
        const uint32_t ca = cols->perm[ja], cb = cols->perm[jb];
        const bool shared = cols->stride[ca] == 0 && cols->stride[cb] == 0;
        if (!shared || user == 0) {
          uint4 alo, ahi, blo, bhi;
          mock_cell_words(cols, ca, user, a & row_mask, alo, ahi);
          mock_cell_words(cols, cb, user, b & row_mask, blo, bhi);
          fail = alo.x != blo.x || alo.y != blo.y || alo.z != blo.z || alo.w != blo.w || ahi.x != bhi.x || ahi.y != bhi.y ||
                 ahi.z != bhi.z || ahi.w != bhi.w;
        }
      }
    }
    mock_append(fail, mock_record(user, ci), sink);
  }
}

// ---- host ----
// as the evaluator's single kind: enough lanes to fill the chip, few enough that the intermediates' scratch stays cache-sized
static uint32_t mock_blocks(uint64_t lanes) { return graph_launch_plan(GRAPH_SINGLE, lanes, 1, 0, 0, graph_max_blocks()).blocks; }

// the batched table into the slot's argument buffer, ordered on `stream` ahead of the launch that reads it
static int mock_table_upload(AuxSlot& slot, const MockTable& t, const GraphProgram* g, const uint64_t* dyn_ext, size_t n_dyn,
                             const uint32_t* perm, size_t n_perm, hipStream_t stream, CheckColumns** out) {
  CheckColumns cols;
  std::memset(&cols, 0, sizeof cols);
  for (size_t i = 0; i < t.n; ++i) {
    cols.p[i] = (const uint32_t*)t.bases[i];
    cols.stride[i] = t.strides[i];
    cols.rows[i] = t.rows[i];
  }
  for (size_t j = 0; j < n_perm; ++j) cols.perm[j] = perm[j];
  cols.n_static = g ? g->n_static : 0;
  for (size_t i = 0; i < n_dyn; ++i) host::fr_to_internal9(host::fr_load(dyn_ext + 4 * i), &cols.dyn[9 * i]);
  CheckColumns* d_cols = (CheckColumns*)aux_buffer(slot, AuxBuf::args, sizeof(CheckColumns), "mock");
  if (!d_cols) return HM_ERR_HIP;
  // pageable source: the runtime has taken its copy of `cols` when this returns (as graph_run's block)
  HM_HIP_CHECK(hipMemcpyAsync(d_cols, &cols, sizeof cols, hipMemcpyHostToDevice, stream));
  *out = d_cols;
  return HM_OK;
}

int mock_program_run(DeviceCtx& ctx, GraphProgram& g, const MockTable& t, const uint64_t* dyn_ext, size_t n_dyn, uint32_t k,
                     uint32_t usable, size_t m, uint32_t user_base, const uint64_t* d_list, size_t n_list, const uint32_t* d_table_values,
                     const MockSink& out, hipStream_t stream) {
  GraphVariant& v = g.variant[0];                    // external-form columns: lowered by hm_graph_create
  if (!v.ready) return hm_fail(HM_ERR_INTERNAL, "mock: the program has no lowered form");
  if (t.n != g.n_columns) return hm_fail(HM_ERR_BAD_ARG, "mock: the program was built for another number of columns");
  if (n_dyn != g.n_dynamic) return hm_fail(HM_ERR_BAD_ARG, "mock: the program was built for another number of per-call constants");
  const uint64_t lanes = d_list ? (uint64_t)n_list : (uint64_t)m * usable;
  if (lanes == 0) return HM_OK;
  const GraphPlan p = graph_launch_plan(GRAPH_SINGLE, lanes, 1, v.n_slots, 0, graph_max_blocks());
  const size_t b_scratch = (p.scratch_bytes + 255) & ~(size_t)255;       // the keys behind it stay 256-byte aligned
  const size_t b_keys = d_table_values ? lookup_sorted_keys_bytes(usable) : 0;
  const CheckSink sink{out.d_records, out.cap, (unsigned long long*)out.d_counter, out.d_user_flags};
  return aux_scope(ctx, stream, [&](AuxSlot& slot) -> int {
    uint8_t* buf = (uint8_t*)aux_buffer(slot, AuxBuf::scratch, b_scratch + b_keys, "mock");
    if (!buf) return HM_ERR_HIP;
    if (d_table_values)
      if (const int rc = lookup_sorted_keys_run(ctx, d_table_values, usable, buf + b_scratch, stream)) return rc;
    CheckColumns* d_cols = nullptr;
    if (const int rc = mock_table_upload(slot, t, &g, dyn_ext, n_dyn, nullptr, 0, stream, &d_cols)) return rc;
    ge_launch(d_table_values != nullptr, graph_check_kernel<SINK_NOT_IN_TABLE>, graph_check_kernel<SINK_NONZERO>, p.blocks, stream, d_cols, g.d_consts,
              g.d_rot, v.d_calcs, v.n_calc, v.result_src, v.result_prev, buf, lanes, usable, k, m, user_base, d_list,
              d_table_values ? buf + b_scratch : nullptr, d_table_values ? usable : 0u, sink);
    HM_HIP_CHECK(hipGetLastError());
    return HM_OK;
  });
}

int mock_copies_run(DeviceCtx& ctx, const MockTable& t, const uint32_t* perm, size_t n_perm, const uint32_t* d_pairs, size_t n_copies,
                    uint32_t k, size_t m, const MockSink& out, hipStream_t stream) {
  const uint64_t lanes = (uint64_t)m * n_copies;
  if (lanes == 0) return HM_OK;
  const CheckSink sink{out.d_records, out.cap, (unsigned long long*)out.d_counter, out.d_user_flags};
  return aux_scope(ctx, stream, [&](AuxSlot& slot) -> int {
    CheckColumns* d_cols = nullptr;
    if (const int rc = mock_table_upload(slot, t, nullptr, nullptr, 0, perm, n_perm, stream, &d_cols)) return rc;
    hipLaunchKernelGGL(mock_copies_kernel, dim3(mock_blocks(lanes)), dim3(GE_THREADS), 0, stream, (const CheckColumns*)d_cols, d_pairs,
                       (uint32_t)n_copies, (uint32_t)n_perm, k, lanes, sink);
    HM_HIP_CHECK(hipGetLastError());
    return HM_OK;
  });
}

}  // namespace hm

// verify.hip -- the device side of a batch verification (batch_verifier.py is the caller): the kernels and the drivers
//   verify_read_run, verify_colsum_run    a batch of proofs read slot by slot, the column sums of its shared scalars (verify_read.inc)
//   verify_terms_run                      the per-proof terms of the opening checks, one lane per proof (verify_terms.inc)
//   verify_terms_multi_run                the same for multi-circuit proofs: a wavefront per proof, a lane per circuit.  Two kernels
//                                         and two launch shapes over one phase-b walk, behind one driver (verify_terms_launch)
//   verify_terms_gwc_run                  the terms of proofs that end in the GWC multiopen: one lane per proof, the same phase a and
//                                         numerator, the point groups' phase b (vg_phase_b), the same driver
//   verify_sums_run                       the two G1 points of every proof's own check, one workgroup per proof (verify_sums.inc)
//   blake2b_run, verify_transcript_run    Blake2b-512 and the proofs' transcripts on it, one lane per proof (transcript.inc)
//   keccak256_run, verify_read_evm_run,   Keccak-256, and the read and the transcripts of proofs in the EVM encoding: uncompressed
//   verify_transcript_evm_run             big-endian points, a Keccak transcript that absorbs the proof verbatim (keccak.inc)
// The .inc files hold the per-slot, per-proof and per-message functions, the plan's and the schedule's checks: host_check.cpp and
// capi_verify.hip compile them too.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "fq_inverse.h"
#include "g1_mul.h"
#include "graph_interp.h"
#include "graph_lower.h"
#include "hm_internal.h"
#include "msm_dev.h"

namespace hm {

#include "g1_codec.inc"      // the decompression of a point slot (g1_decompress_one)
#include "verify_read.inc"
#include "verify_terms.inc"
#include "verify_sums.inc"
#include "transcript.inc"
#include "keccak.inc"

// ---- the read and the column sums ------------------------------------------------------------
__device__ __forceinline__ void vr_load8(const uint32_t* __restrict__ p, uint32_t (&w)[8]) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 a = q[0], b = q[1];
  w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w, w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w;
}
__device__ __forceinline__ void vr_store8(uint32_t* __restrict__ p, const uint32_t (&w)[8]) {
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(w[0], w[1], w[2], w[3]);
  q[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

__global__ __launch_bounds__(ACC_THREADS) void verify_read_kernel(const uint32_t* __restrict__ proofs, const uint32_t* __restrict__ slot_table,
                                                                  uint32_t slots, uint64_t lanes, uint32_t own_points, uint32_t n_points,
                                                                  uint32_t n_scalars, uint32_t* __restrict__ points, uint32_t* __restrict__ tail,
                                                                  uint32_t* __restrict__ ybytes, uint32_t* __restrict__ scalars,
                                                                  uint32_t* __restrict__ bad) {
  const uint64_t i = (uint64_t)blockIdx.x * ACC_THREADS + threadIdx.x;
  if (i >= lanes) return;
  const uint64_t b = i / slots;
  const uint32_t entry = slot_table[i % slots], index = entry & VR_INDEX;
  uint32_t w[8];
  vr_load8(proofs + i * 8, w);
  bool ok;
  if (entry & VR_POINT) {
    const bool in_tail = (entry & VR_TAIL) != 0;
    ok = index < n_points && (in_tail || index < own_points);
    if (ok) {
      uint32_t ox[8], oy[8], ycan[8];
      ok = proof_point_one(w, ox, oy, ycan);
      uint32_t* dst = in_tail ? tail + b * 16 : points + (b * own_points + index) * 16;
      vr_store8(dst, ox);
      vr_store8(dst + 8, oy);
      vr_store8(ybytes + (b * n_points + index) * 8, ycan);
    }
  } else {
    ok = index < n_scalars;
    if (ok) {
      uint32_t out[8];
      ok = proof_scalar_one(w, out);
      vr_store8(scalars + (b * n_scalars + index) * 8, out);
    }
  }
  if (!ok) atomicOr(bad + b, 1u);
}

constexpr int COLSUM_THREADS = 256;

__global__ __launch_bounds__(COLSUM_THREADS) void verify_colsum_kernel(const uint32_t* __restrict__ rows, uint32_t cols, uint64_t lo, uint64_t hi,
                                                                       uint32_t* __restrict__ out) {
  __shared__ uint32_t sh[9][COLSUM_THREADS];
  const uint32_t c = blockIdx.x, t = threadIdx.x;
  Fr acc = fe_zero<FrParams>();
  for (uint64_t r = lo + t; r < hi; r += COLSUM_THREADS) {
    uint32_t w[8];
    vr_load8(rows + (r * cols + c) * 8, w);
    acc = colsum_step(acc, w);
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) sh[k][t] = acc.l[k];
  __syncthreads();
  for (uint32_t s = COLSUM_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) {
      Fr o;
#pragma unroll
      for (int k = 0; k < 9; ++k) o.l[k] = sh[k][t + s];
      HM_DECLARE(o, 3.0);
      acc = colsum_join(acc, o);
#pragma unroll
      for (int k = 0; k < 9; ++k) sh[k][t] = acc.l[k];
    }
    __syncthreads();
  }
  if (t == 0) {
    uint32_t w[8];
    colsum_finish(acc, w);
    vr_store8(out + (size_t)c * 8, w);
  }
}

// A batch of proofs (verify_read.inc).  Both are asynchronous on `stream`; every index the read kernel takes from the device table is
// checked there against the sizes given here.
int verify_read_run(const uint32_t* d_proofs, size_t n_proofs, const uint32_t* d_slot_table, uint32_t slots, uint32_t own_points,
                    uint32_t n_points, uint32_t n_scalars, uint32_t* d_points, uint32_t* d_tail, uint32_t* d_ybytes, uint32_t* d_scalars,
                    uint32_t* d_bad, hipStream_t stream) {
  const uint64_t lanes = (uint64_t)n_proofs * slots;
  if (lanes == 0) return HM_OK;
  hipLaunchKernelGGL(verify_read_kernel, dim3((uint32_t)((lanes + ACC_THREADS - 1) / ACC_THREADS)), dim3(ACC_THREADS), 0, stream, d_proofs,
                     d_slot_table, slots, lanes, own_points, n_points, n_scalars, d_points, d_tail, d_ybytes, d_scalars, d_bad);
  HM_HIP_CHECK(hipGetLastError());
  return HM_OK;
}

int verify_colsum_run(const uint32_t* d_rows, uint32_t cols, size_t lo, size_t hi, uint32_t* d_out, hipStream_t stream) {
  if (cols == 0) return HM_OK;
  hipLaunchKernelGGL(verify_colsum_kernel, dim3(cols), dim3(COLSUM_THREADS), 0, stream, d_rows, cols, (uint64_t)lo, (uint64_t)hi, d_out);
  HM_HIP_CHECK(hipGetLastError());
  return HM_OK;
}

// ---- the terms -------------------------------------------------------------------------------
struct VerifySource {
  const uint32_t* __restrict__ plan;
  VtMem m;
  uint32_t static_consts;
  __device__ __forceinline__ uint32_t n_static() const { return static_consts; }
  // the program's per-call constants are beta, gamma, theta, y, in that order (evaluation.GraphEvaluator.lower)
  __device__ __forceinline__ uint32_t dyn(uint32_t word) const {
    const uint32_t j = word / 9, limb = word - 9 * j;
    const uint32_t rec = j == 0 ? VT_BETA : j == 1 ? VT_GAMMA : j == 2 ? VT_THETA : VT_Y;
    return m.ws[((size_t)(plan[VT_N_VALS] + rec) * 9 + limb) * m.T + m.lane];
  }
  __device__ __forceinline__ Fr column(uint32_t src) const {
    const uint32_t col = gsrc_column(src), rot = gsrc_rot(src);
    uint32_t slot = VT_NO_SLOT;
    if (col < plan[VT_N_COLS] && rot < plan[VT_N_ROT]) slot = plan[plan[VT_OFF_COLMAP] + col * plan[VT_N_ROT] + rot];
    if (slot >= plan[VT_N_VALS]) return fe_zero<FrParams>();
    return vt_load(m, slot);
  }
  __device__ __forceinline__ Fr previous() const { return fe_zero<FrParams>(); }
};

__global__ __launch_bounds__(GE_THREADS) void verify_terms_kernel(const uint32_t* __restrict__ plan, const uint32_t* __restrict__ consts,
                                                                  const GraphCalc* __restrict__ calcs, uint32_t n_calc, uint32_t result_src,
                                                                  uint32_t result_prev, uint32_t n_static, uint32_t* __restrict__ ws,
                                                                  uint32_t n_proofs, const uint32_t* __restrict__ records,
                                                                  const uint32_t* __restrict__ evals, const uint32_t* __restrict__ inst,
                                                                  uint32_t* __restrict__ bad, uint32_t* __restrict__ own,
                                                                  uint32_t* __restrict__ shared, uint32_t* __restrict__ h2r,
                                                                  uint32_t* __restrict__ h2l) {
  const uint32_t T = gridDim.x * GE_THREADS, lane = blockIdx.x * GE_THREADS + threadIdx.x;
  if (lane >= n_proofs) return;
  const size_t b = lane;
  uint32_t* my_own = own + b * plan[VT_N_OWN] * 8;
  uint32_t* my_shared = shared + b * plan[VT_N_SHARED] * 8;
  vt_zero_lane(plan, VtSingle{}, my_own, my_shared, h2r + b * 8, h2l + b * 8);
  if (bad[b]) return;
  const VtMem m{ws, T, lane};
  bool ok = vt_phase_a(plan, m, records + b * VT_REC * 8, evals + b * plan[VT_N_SCALARS] * 8, inst + b * plan[VT_INST_ELEMS] * 8);
  const VerifySource from{plan, m, n_static};
  const Fr num = ge_reduce(ge_run(from, consts, calcs, n_calc, result_src, result_prev, ws + (size_t)vt_ws_program(plan) * 9 * T, T, lane));
  ok = vt_phase_b(plan, m, num, my_own, my_shared, h2r + b * 8, h2l + b * 8) && ok;
  if (!ok) {
    bad[b] = 1;
    vt_zero_lane(plan, VtSingle{}, my_own, my_shared, h2r + b * 8, h2l + b * 8);
  }
}

// ---- the terms of multi-circuit proofs: a wavefront per proof, a lane per circuit ---------------
// The sum over the lanes of ONE wavefront, by cross-lane moves alone: every lane of the wave calls it (an idle lane brings zero), every
// lane returns lane 0's total.  No LDS, no atomics, nothing leaves the wave.
__device__ __forceinline__ Fr vtm_wave_sum(Fr acc) {
  static_assert(VM_MAX_CIRCUITS == 64, "a gfx950 wavefront has 64 lanes");
  for (int off = 32; off > 0; off >>= 1) {
    Fr other;
#pragma unroll
    for (int i = 0; i < 9; ++i) other.l[i] = __shfl_down(acc.l[i], off, 64);
    HM_DECLARE(other, 3.0);
    acc = vt_add(acc, other);                                    // lanes at and above 64 - off add their own word: never read below
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) acc.l[i] = __shfl(acc.l[i], 0, 64);
  return acc;
}

__global__ __launch_bounds__(GE_THREADS) void verify_terms_multi_kernel(const uint32_t* __restrict__ mp, const uint32_t* __restrict__ consts,
                                                                        const GraphCalc* __restrict__ calcs, uint32_t n_calc,
                                                                        uint32_t result_src, uint32_t result_prev, uint32_t n_static,
                                                                        uint32_t* __restrict__ ws, uint32_t n_proofs,
                                                                        const uint32_t* __restrict__ records, const uint32_t* __restrict__ evals,
                                                                        const uint32_t* __restrict__ inst, uint32_t* __restrict__ bad,
                                                                        uint32_t* __restrict__ own, uint32_t* __restrict__ shared,
                                                                        uint32_t* __restrict__ h2r, uint32_t* __restrict__ h2l) {
  static_assert(GE_THREADS % 64 == 0, "whole wavefronts per workgroup");
  const uint32_t T = gridDim.x * GE_THREADS, lane = blockIdx.x * GE_THREADS + threadIdx.x;
  const size_t b = lane / 64;                                    // the same for a whole wavefront
  const uint32_t c = lane % 64;
  if (b >= n_proofs) return;
  const uint32_t* lp = vtm_lane_plan(mp);
  const uint32_t circuits = mp[VM_CIRCUITS];
  const bool active = c < circuits;
  uint32_t* my_own = own + b * mp[VM_N_OWN] * 8;
  uint32_t* my_shared = shared + b * lp[VT_N_SHARED] * 8;
  const VtmLane me{mp, c};
  vt_zero_lane(lp, me, my_own, my_shared, h2r + b * 8, h2l + b * 8);
  if (bad[b]) return;
  const VtMem m{ws, T, lane};
  bool ok = true;
  Fr term = fe_zero<FrParams>();
  HM_DECLARE(term, 3.0);
  if (active) {
    ok = vtm_phase_a(mp, m, c, records + b * VT_REC * 8, evals + b * mp[VM_N_SCALARS] * 8, inst + (b * circuits + c) * lp[VT_INST_ELEMS] * 8);
    const VerifySource from{lp, m, n_static};
    const Fr fold = ge_reduce(ge_run(from, consts, calcs, n_calc, result_src, result_prev, ws + (size_t)vt_ws_program(lp) * 9 * T, T, lane));
    term = vtm_numerator_term(mp, m, c, fold);
  }
  const Fr num = vtm_wave_sum(term);
  VtmShare mine{fe_zero<FrParams>(), fe_zero<FrParams>(), fe_zero<FrParams>(), true};
  HM_DECLARE(mine.r_outer, 3.0);
  if (active) {
    mine = vt_set_walk(lp, m, me, num, my_own, my_shared);
    ok = ok && mine.ok;
  }
  const Fr r_outer = vtm_wave_sum(mine.r_outer);
  const bool failed = __ballot(active && !ok) != 0;               // any lane of the proof
  if (failed) {
    vt_zero_lane(lp, me, my_own, my_shared, h2r + b * 8, h2l + b * 8);
    if (c == 0) bad[b] = 1;
  } else if (c == 0) {
    vt_finish(lp, mp[VM_N_OWN], m, r_outer, mine, my_own, my_shared, h2r + b * 8, h2l + b * 8);
  }
}

// ---- the terms of GWC proofs: one lane per proof, the point groups in place of the rotation sets ---
// The arguments are verify_terms_kernel's, so that one driver launches all three: `w_left` (n_proofs x q x 4 words, r_b u^i) stands
// where that kernel takes h2r, and the last pointer is not looked at.
__global__ __launch_bounds__(GE_THREADS) void verify_terms_gwc_kernel(const uint32_t* __restrict__ plan, const uint32_t* __restrict__ consts,
                                                                      const GraphCalc* __restrict__ calcs, uint32_t n_calc, uint32_t result_src,
                                                                      uint32_t result_prev, uint32_t n_static, uint32_t* __restrict__ ws,
                                                                      uint32_t n_proofs, const uint32_t* __restrict__ records,
                                                                      const uint32_t* __restrict__ evals, const uint32_t* __restrict__ inst,
                                                                      uint32_t* __restrict__ bad, uint32_t* __restrict__ own,
                                                                      uint32_t* __restrict__ shared, uint32_t* __restrict__ w_left,
                                                                      uint32_t* __restrict__) {
  const uint32_t T = gridDim.x * GE_THREADS, lane = blockIdx.x * GE_THREADS + threadIdx.x;
  if (lane >= n_proofs) return;
  const size_t b = lane;
  uint32_t* my_own = own + b * plan[VT_N_OWN] * 8;
  uint32_t* my_shared = shared + b * plan[VT_N_SHARED] * 8;
  uint32_t* my_left = w_left + b * plan[VT_N_SETS] * 8;
  vg_zero_lane(plan, my_own, my_shared, my_left);
  if (bad[b]) return;
  const VtMem m{ws, T, lane};
  const bool ok = vg_phase_a(plan, m, records + b * VG_REC * 8, evals + b * plan[VT_N_SCALARS] * 8, inst + b * plan[VT_INST_ELEMS] * 8);
  const VerifySource from{plan, m, n_static};
  const Fr num = ge_reduce(ge_run(from, consts, calcs, n_calc, result_src, result_prev, ws + (size_t)vt_ws_program(plan) * 9 * T, T, lane));
  vg_phase_b(plan, m, num, my_own, my_shared, my_left);
  if (!ok) {
    bad[b] = 1;
    vg_zero_lane(plan, my_own, my_shared, my_left);
  }
}

// ---- the drivers of the terms kernels -----------------------------------------------------------
using VerifyTermsKernel = decltype(&verify_terms_kernel);         // the three kernels take the same arguments

// What both drivers do behind their plan's check (`why`: its verdict, reported behind the program's own checks as before): `what`
// opens every message, `lane_plan` sizes a lane's workspace, `lanes` is the launch's width.  The arguments were checked by the caller
// (capi_verify.hip) -- but for the plan, which is checked before anything is launched.
static int verify_terms_launch(const char* what, const char* why, DeviceCtx& ctx, GraphProgram& g, const uint32_t* plan, size_t n_words,
                               const uint32_t* lane_plan, size_t n_columns, size_t n_dynamic, size_t n_proofs, size_t lanes,
                               VerifyTermsKernel kernel, const uint32_t* d_records, const uint32_t* d_evals, const uint32_t* d_inst,
                               uint32_t* d_bad, uint32_t* d_own, uint32_t* d_shared, uint32_t* d_h2r, uint32_t* d_h2l, hipStream_t stream) {
  GraphVariant& v = g.variant[0];
  if (!v.ready) return hm_fail(HM_ERR_INTERNAL, std::string(what) + ": the program has no lowered form");
  if (n_columns != g.n_columns) return hm_fail(HM_ERR_BAD_ARG, std::string(what) + ": the program was built for another number of columns");
  if (n_dynamic != g.n_dynamic || n_dynamic != 4)
    return hm_fail(HM_ERR_BAD_ARG, std::string(what) + ": the program must take beta, gamma, theta, y as its per-call constants");
  if (why) return hm_fail(HM_ERR_BAD_ARG, why);
  const uint32_t blocks = (uint32_t)((lanes + GE_THREADS - 1) / GE_THREADS), T = blocks * GE_THREADS;
  const size_t slots = (size_t)vt_ws_program(lane_plan) + v.n_slots;
  return aux_scope(ctx, stream, [&](AuxSlot& slot) -> int {
    uint32_t* ws = (uint32_t*)aux_buffer(slot, AuxBuf::scratch, slots * 9 * T * 4, what);
    uint32_t* d_plan = ws ? (uint32_t*)aux_buffer(slot, AuxBuf::args, n_words * 4, what) : nullptr;
    if (!d_plan) return HM_ERR_HIP;
    // pageable source: the runtime has taken its copy of the plan when this returns (as the witness checker's table)
    HM_HIP_CHECK(hipMemcpyAsync(d_plan, plan, n_words * 4, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(GE_THREADS), 0, stream, (const uint32_t*)d_plan, (const uint32_t*)g.d_consts,
                       (const GraphCalc*)v.d_calcs, v.n_calc, v.result_src, v.result_prev, g.n_static, ws, (uint32_t)n_proofs, d_records, d_evals,
                       d_inst, d_bad, d_own, d_shared, d_h2r, d_h2l);
    HM_HIP_CHECK(hipGetLastError());
    return HM_OK;
  });
}

// one lane per proof
int verify_terms_run(DeviceCtx& ctx, GraphProgram& g, const uint32_t* plan, size_t n_words, size_t n_columns, size_t n_dynamic, size_t n_proofs,
                     const uint32_t* d_records, const uint32_t* d_evals, const uint32_t* d_inst, uint32_t* d_bad, uint32_t* d_own,
                     uint32_t* d_shared, uint32_t* d_h2r, uint32_t* d_h2l, hipStream_t stream) {
  return verify_terms_launch("verify terms", vt_plan_problem(plan, n_words, n_columns), ctx, g, plan, n_words, plan, n_columns, n_dynamic,
                             n_proofs, n_proofs, verify_terms_kernel, d_records, d_evals, d_inst, d_bad, d_own, d_shared, d_h2r, d_h2l, stream);
}

// proofs of `circuits` circuits each: 64 lanes per proof
int verify_terms_multi_run(DeviceCtx& ctx, GraphProgram& g, const uint32_t* plan, size_t n_words, size_t n_columns, size_t n_dynamic,
                           size_t n_proofs, uint32_t circuits, const uint32_t* d_records, const uint32_t* d_evals, const uint32_t* d_inst,
                           uint32_t* d_bad, uint32_t* d_own, uint32_t* d_shared, uint32_t* d_h2r, uint32_t* d_h2l, hipStream_t stream) {
  const char* why = vtm_plan_problem(plan, n_words, n_columns, circuits);
  return verify_terms_launch("verify terms multi", why, ctx, g, plan, n_words, why ? plan : vtm_lane_plan(plan), n_columns, n_dynamic, n_proofs,
                             n_proofs * 64, verify_terms_multi_kernel, d_records, d_evals, d_inst, d_bad, d_own, d_shared, d_h2r, d_h2l, stream);
}

// GWC proofs, one lane per proof: d_w_left takes the place of d_h2r, and there is no d_h2l
int verify_terms_gwc_run(DeviceCtx& ctx, GraphProgram& g, const uint32_t* plan, size_t n_words, size_t n_columns, size_t n_dynamic,
                         size_t n_proofs, const uint32_t* d_records, const uint32_t* d_evals, const uint32_t* d_inst, uint32_t* d_bad,
                         uint32_t* d_own, uint32_t* d_shared, uint32_t* d_w_left, hipStream_t stream) {
  return verify_terms_launch("verify terms gwc", vg_plan_problem(plan, n_words, n_columns), ctx, g, plan, n_words, plan, n_columns, n_dynamic,
                             n_proofs, n_proofs, verify_terms_gwc_kernel, d_records, d_evals, d_inst, d_bad, d_own, d_shared, d_w_left, nullptr,
                             stream);
}

// ---- the per-proof sums -----------------------------------------------------------------------
// One workgroup per proof (verify_sums.inc): the lanes' partial sums, the fold through LDS, then lanes 0 and 1 normalise -R_b and L_b.
// The flag is the same for the whole workgroup, so a flagged proof leaves before the first barrier.
__global__ __launch_bounds__(VS_THREADS) void verify_sums_kernel(VsArgs a, const uint32_t* __restrict__ bad, uint32_t* __restrict__ out) {
  __shared__ __align__(16) uint32_t tree[(VS_THREADS + 1) * VS_ACC_WORDS];
  const uint64_t b = blockIdx.x;
  const uint32_t t = threadIdx.x;
  uint32_t* rows = out + b * 2 * VS_ROW_WORDS;
  if (bad[b]) {
    if (t < 2 * VS_ROW_WORDS) rows[t] = 0;
    return;
  }
  uint32_t* left = tree + VS_THREADS * VS_ACC_WORDS;
  vs_lane(a, b, t, VS_THREADS, tree + t * VS_ACC_WORDS, left);
  __syncthreads();
  for (uint32_t off = VS_THREADS / 2; off > 0; off >>= 1) {
    if (t < off) vs_fold_step(tree, t, off);
    __syncthreads();
  }
  if (t < 2) vs_finish(t == 0 ? tree : left, t == 0, rows + (t == 0 ? VS_ROW_WORDS : 0));
}

// the arguments were checked by the caller (capi_verify.hip): one launch, asynchronous on `stream`
int verify_sums_run(const uint32_t* d_bases, size_t n_proofs, uint32_t own_points, uint32_t shared_points, const uint32_t* d_own,
                    const uint32_t* d_shared, const uint32_t* d_h2r, const uint32_t* d_h2l, const uint32_t* d_bad, uint32_t* d_pairs,
                    hipStream_t stream) {
  const VsArgs a{d_bases, d_own, d_shared, d_h2r, d_h2l, (uint64_t)n_proofs, own_points, shared_points};
  hipLaunchKernelGGL(verify_sums_kernel, dim3((uint32_t)n_proofs), dim3(VS_THREADS), 0, stream, a, d_bad, d_pairs);
  HM_HIP_CHECK(hipGetLastError());
  return HM_OK;
}

// ---- Blake2b and the transcripts -------------------------------------------------------------
__global__ __launch_bounds__(TR_THREADS) void blake2b_kernel(const uint8_t* __restrict__ msgs, uint64_t stride, const uint32_t* __restrict__ lens,
                                                             uint64_t n, uint64_t personal_lo, uint64_t personal_hi, uint32_t* __restrict__ out) {
  __shared__ uint32_t block[B2_BLOCK_WORDS][TR_THREADS];
  const uint64_t i = (uint64_t)blockIdx.x * TR_THREADS + threadIdx.x;
  if (i >= n) return;
  uint32_t* digest = out + i * 16;
  const uint32_t len = lens[i];
  if (len > stride) {                                            // a length that leaves the message's room: zeros, nothing read
#pragma unroll
    for (int k = 0; k < 16; ++k) digest[k] = 0;
    return;
  }
  b2_hash_lane(B2Buf{&block[0][threadIdx.x], TR_THREADS}, msgs + i * stride, len, personal_lo, personal_hi, digest);
}

__global__ __launch_bounds__(TR_THREADS) void verify_transcript_kernel(const uint32_t* __restrict__ proofs, uint32_t n_proofs,
                                                                       const uint32_t* __restrict__ slot_table, uint32_t slots,
                                                                       uint32_t n_points, const uint32_t* __restrict__ ybytes,
                                                                       const uint32_t* __restrict__ preamble,
                                                                       const uint32_t* __restrict__ counts, uint32_t stride,
                                                                       const uint32_t* __restrict__ sched, uint32_t n_pairs,
                                                                       uint32_t* __restrict__ bad, uint32_t* __restrict__ records,
                                                                       uint32_t record_elems) {
  __shared__ uint32_t block[B2_BLOCK_WORDS + TR_STAGE_WORDS][TR_THREADS];
  const uint32_t b = blockIdx.x * TR_THREADS + threadIdx.x;
  if (b >= n_proofs) return;
  tr_proof_one(B2Buf{&block[0][threadIdx.x], TR_THREADS}, b, proofs, slot_table, slots, n_points, ybytes, preamble, counts, stride, sched,
               n_pairs, bad, records, record_elems);
}

// the arguments were checked by the caller (capi_verify.hip)
int blake2b_run(const uint8_t* d_msgs, size_t stride, const uint32_t* d_lens, size_t n, const uint8_t* personal16, uint32_t* d_out,
                hipStream_t stream) {
  uint64_t personal[2] = {0, 0};
  if (personal16) std::memcpy(personal, personal16, 16);
  hipLaunchKernelGGL(blake2b_kernel, dim3((uint32_t)((n + TR_THREADS - 1) / TR_THREADS)), dim3(TR_THREADS), 0, stream, d_msgs, (uint64_t)stride,
                     d_lens, (uint64_t)n, personal[0], personal[1], d_out);
  HM_HIP_CHECK(hipGetLastError());
  return HM_OK;
}

int verify_transcript_run(DeviceCtx& ctx, const uint32_t* d_proofs, size_t n_proofs, const uint32_t* d_slot_table, uint32_t slots,
                          uint32_t n_points, const uint32_t* d_ybytes, const uint32_t* d_preamble, const uint32_t* d_counts, uint32_t stride,
                          const uint32_t* schedule, size_t n_pairs, uint32_t* d_bad, uint32_t* d_records, uint32_t record_elems,
                          hipStream_t stream) {
  if (const char* why = tr_schedule_problem(schedule, n_pairs, slots, record_elems)) return hm_fail(HM_ERR_BAD_ARG, why);
  return aux_scope(ctx, stream, [&](AuxSlot& slot) -> int {
    uint32_t* d_sched = (uint32_t*)aux_buffer(slot, AuxBuf::args, n_pairs * 8, "verify transcript");
    if (!d_sched) return HM_ERR_HIP;
    // pageable source: the runtime has taken its copy of the schedule when this returns (as the terms plan)
    HM_HIP_CHECK(hipMemcpyAsync(d_sched, schedule, n_pairs * 8, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(verify_transcript_kernel, dim3((uint32_t)((n_proofs + TR_THREADS - 1) / TR_THREADS)), dim3(TR_THREADS), 0, stream, d_proofs,
                       (uint32_t)n_proofs, d_slot_table, slots, n_points, d_ybytes, d_preamble, d_counts, stride, (const uint32_t*)d_sched,
                       (uint32_t)n_pairs, d_bad, d_records, record_elems);
    HM_HIP_CHECK(hipGetLastError());
    return HM_OK;
  });
}

// ---- the EVM encoding: Keccak-256, the uncompressed read, the transcripts ---------------------
__global__ __launch_bounds__(KC_THREADS) void keccak256_kernel(const uint8_t* __restrict__ msgs, uint64_t stride, const uint32_t* __restrict__ lens,
                                                               uint64_t n, uint32_t* __restrict__ out) {
  __shared__ uint32_t block[KC_BLOCK_WORDS][KC_THREADS];
  const uint64_t i = (uint64_t)blockIdx.x * KC_THREADS + threadIdx.x;
  if (i >= n) return;
  uint32_t* digest = out + i * 8;
  const uint32_t len = lens[i];
  if (len > stride) {                                            // a length that leaves the message's room: zeros, nothing read
#pragma unroll
    for (int k = 0; k < 8; ++k) digest[k] = 0;
    return;
  }
  kc_hash_lane(KcBuf{&block[0][threadIdx.x], KC_THREADS}, msgs + i * stride, len, KC_DOMAIN, digest);
}

__global__ __launch_bounds__(ACC_THREADS) void verify_read_evm_kernel(const uint32_t* __restrict__ proofs, const uint32_t* __restrict__ slot_table,
                                                                      uint32_t slots, uint64_t lanes, uint32_t own_points, uint32_t n_scalars,
                                                                      uint32_t* __restrict__ points, uint32_t* __restrict__ tail,
                                                                      uint32_t* __restrict__ scalars, uint32_t* __restrict__ bad) {
  const uint64_t i = (uint64_t)blockIdx.x * ACC_THREADS + threadIdx.x;
  if (i >= lanes) return;
  const uint64_t b = i / slots;
  const uint32_t slot = (uint32_t)(i - b * slots);
  if (!evm_read_slot(proofs + b * slots * 8, slot, slots, slot_table[slot], own_points, n_scalars, points + b * own_points * 16, tail + b * 16,
                     scalars + b * n_scalars * 8))
    atomicOr(bad + b, 1u);
}

__global__ __launch_bounds__(KC_THREADS) void verify_transcript_evm_kernel(const uint32_t* __restrict__ proofs, uint32_t n_proofs, uint32_t slots,
                                                                           const uint32_t* __restrict__ preamble,
                                                                           const uint32_t* __restrict__ counts, uint32_t stride,
                                                                           const uint32_t* __restrict__ sched, uint32_t n_pairs,
                                                                           uint32_t* __restrict__ bad, uint32_t* __restrict__ records,
                                                                           uint32_t record_elems) {
  __shared__ uint32_t block[KC_BLOCK_WORDS][KC_THREADS];
  const uint32_t b = blockIdx.x * KC_THREADS + threadIdx.x;
  if (b >= n_proofs) return;
  evm_proof_one(KcBuf{&block[0][threadIdx.x], KC_THREADS}, b, proofs, slots, preamble, counts, stride, sched, n_pairs, bad, records, record_elems);
}

// the arguments were checked by the caller (capi_verify.hip)
int keccak256_run(const uint8_t* d_msgs, size_t stride, const uint32_t* d_lens, size_t n, uint32_t* d_out, hipStream_t stream) {
  hipLaunchKernelGGL(keccak256_kernel, dim3((uint32_t)((n + KC_THREADS - 1) / KC_THREADS)), dim3(KC_THREADS), 0, stream, d_msgs, (uint64_t)stride,
                     d_lens, (uint64_t)n, d_out);
  HM_HIP_CHECK(hipGetLastError());
  return HM_OK;
}

int verify_read_evm_run(const uint32_t* d_proofs, size_t n_proofs, const uint32_t* d_slot_table, uint32_t slots, uint32_t own_points,
                        uint32_t n_scalars, uint32_t* d_points, uint32_t* d_tail, uint32_t* d_scalars, uint32_t* d_bad, hipStream_t stream) {
  const uint64_t lanes = (uint64_t)n_proofs * slots;
  if (lanes == 0) return HM_OK;
  hipLaunchKernelGGL(verify_read_evm_kernel, dim3((uint32_t)((lanes + ACC_THREADS - 1) / ACC_THREADS)), dim3(ACC_THREADS), 0, stream, d_proofs,
                     d_slot_table, slots, lanes, own_points, n_scalars, d_points, d_tail, d_scalars, d_bad);
  HM_HIP_CHECK(hipGetLastError());
  return HM_OK;
}

int verify_transcript_evm_run(DeviceCtx& ctx, const uint32_t* d_proofs, size_t n_proofs, uint32_t slots, const uint32_t* d_preamble,
                              const uint32_t* d_counts, uint32_t stride, const uint32_t* schedule, size_t n_pairs, uint32_t* d_bad,
                              uint32_t* d_records, uint32_t record_elems, hipStream_t stream) {
  if (const char* why = tr_schedule_problem(schedule, n_pairs, slots, record_elems)) return hm_fail(HM_ERR_BAD_ARG, why);
  return aux_scope(ctx, stream, [&](AuxSlot& slot) -> int {
    uint32_t* d_sched = (uint32_t*)aux_buffer(slot, AuxBuf::args, n_pairs * 8, "verify transcript");
    if (!d_sched) return HM_ERR_HIP;
    // pageable source: the runtime has taken its copy of the schedule when this returns (as the terms plan)
    HM_HIP_CHECK(hipMemcpyAsync(d_sched, schedule, n_pairs * 8, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(verify_transcript_evm_kernel, dim3((uint32_t)((n_proofs + KC_THREADS - 1) / KC_THREADS)), dim3(KC_THREADS), 0, stream,
                       d_proofs, (uint32_t)n_proofs, slots, d_preamble, d_counts, stride, (const uint32_t*)d_sched, (uint32_t)n_pairs, d_bad,
                       d_records, record_elems);
    HM_HIP_CHECK(hipGetLastError());
    return HM_OK;
  });
}

}  // namespace hm

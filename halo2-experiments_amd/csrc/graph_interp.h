// graph_interp.h -- the interpreter body of the device GraphEvaluator, shared by graph_evaluate_kernel (graph.hip: one lane per
// row of a domain, the value stored) and graph_check_kernel (mock.hip: one lane per (user, row) of a witness batch, the value
// only tested).  What differs between the two is where a column cell, a per-call constant and PreviousValue come from: a
// `Source` answers those three questions, everything else -- the decode, the arithmetic, the [slot][word][lane] scratch of the
// intermediates -- is the one body below.  Device code only; include after g1.h and graph_lower.h.
#pragma once
#include <hip/hip_runtime.h>

#include "g1.h"
#include "graph_lower.h"

namespace hm {

constexpr int GE_THREADS = 256;

__device__ __forceinline__ Fr ge_reduce(const Fr& lazy) { return fe_reduce_small(fe_norm(lazy)); }   // any lazy sum < 2^261 -> < 3r

__device__ __forceinline__ Fr ge_from_ext(const uint32_t* __restrict__ p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 lo = q[0], hi = q[1];
  const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  return fe_mul(fe_unpack<FrParams>(w), fe_const<FrParams>(FrParams::EXT2INT));
}
// A column that already holds INTERNAL-form words (32 x the external value, canonical: what the coset NTT writes when
// its fused constants are pre-multiplied by 32) needs no conversion product: a third of the MerkleSumTree program's
// multiplications were conversions of column loads.
__device__ __forceinline__ Fr ge_from_internal(const uint32_t* __restrict__ p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 lo = q[0], hi = q[1];
  const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  Fr r = fe_unpack<FrParams>(w);
  HM_DECLARE(r, GE_COLUMN_BOUND);
  return r;
}
// the store tail of the evaluating kernels: a value < 3r to the 8 external words of its row, as two uint4
__device__ __forceinline__ void ge_store_ext(uint32_t* row, const Fr& v) {
  uint32_t w[8];
  fe_to_ext(w, v);
  uint4* dst = reinterpret_cast<uint4*>(row);
  dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
  dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
}
// host: one of two instantiations of a kernel, chosen at run time, on `blocks` workgroups of GE_THREADS lanes
template <class... P, class... A>
inline void ge_launch(bool first, void (*a)(P...), void (*b)(P...), uint32_t blocks, hipStream_t stream, A... args) {
  hipLaunchKernelGGL(first ? a : b, dim3(blocks), dim3(GE_THREADS), 0, stream, (P)args...);
}

// Source: n_static() / dyn(word) -- the per-call constants behind the program's own; column(src) -- the cell a column source names
// for this lane; previous() -- PreviousValue.
template <class Source>
__device__ __forceinline__ Fr ge_fetch(uint32_t src, const Source& from, const uint32_t* __restrict__ consts,
                                       const uint32_t* __restrict__ scratch, uint32_t T, uint32_t lane_slot) {
  const uint32_t kind = gsrc_kind(src), index = gsrc_index(src);
  Fr r;
  if (kind == GSRC_INTER) {
    const uint32_t* p = scratch + (size_t)index * 9 * T + lane_slot;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.l[i] = p[(size_t)i * T];
    HM_DECLARE(r, GE_CAP);
  } else if (kind == GSRC_CONST) {
    if (index >= from.n_static()) {
      const uint32_t d = (index - from.n_static()) * 9;
#pragma unroll
      for (int i = 0; i < 9; ++i) r.l[i] = from.dyn(d + i);
    } else {
      const uint32_t* p = consts + (size_t)index * 9;
#pragma unroll
      for (int i = 0; i < 9; ++i) r.l[i] = p[i];
    }
    HM_DECLARE(r, 1.0);
  } else if (kind == GSRC_COLUMN) {
    r = from.column(src);
  } else {
    r = from.previous();
  }
  return r;
}

// One lane's run of the lowered program: -> its value (the last calculation, or the given source), not yet reduced.
template <class Source>
__device__ __forceinline__ Fr ge_run(const Source& from, const uint32_t* __restrict__ consts, const GraphCalc* __restrict__ calcs,
                                     uint32_t n_calc, uint32_t result_src, uint32_t result_prev, uint32_t* __restrict__ scratch, uint32_t T,
                                     uint32_t lane_slot) {
  Fr prev = fe_zero<FrParams>();                         // the previous calculation's result, in registers
  HM_DECLARE(prev, 3.0);
  for (uint32_t k = 0; k < n_calc; ++k) {
    const GraphCalc cc = calcs[k];                       // the same words for every lane: scalar loads
    const uint32_t op = cc.op & 0xffu;
    auto src = [&](uint32_t word, uint32_t flag) -> Fr {
      if (cc.op & flag) return prev;                     // wave-uniform branch
      return ge_fetch(word, from, consts, scratch, T, lane_slot);
    };
    const Fr a = src(cc.a, GF_A_PREV);
    Fr out;
    const bool lazy = (cc.op & GF_NO_REDUCE) != 0, wide = (cc.op & GF_SUB_WIDE) != 0;      // wave-uniform
    auto settle = [&](const Fr& t) -> Fr { return lazy ? fe_norm(t) : ge_reduce(t); };
    // hc_graph_replay (host_check.cpp) restates this switch for the HM_BOUNDS build; tests/test_graph_programs_gpu.py holds
    // the two to the same words
    switch (op) {
      case GOP_ADD:
        out = settle(fe_add(a, src(cc.b, GF_B_PREV)));
        break;
      case GOP_SUB: {
        const Fr b = src(cc.b, GF_B_PREV);
        out = wide ? ge_reduce(fe_sub<20, 29>(a, b)) : settle(fe_sub<4, 29>(a, b));
        break;
      }
      case GOP_MUL:
        out = fe_mul(a, src(cc.b, GF_B_PREV));
        break;
      case GOP_SQUARE:
        out = fe_sqr(a);
        break;
      case GOP_DOUBLE:
        out = settle(fe_dbl(a));
        break;
      case GOP_NEGATE:
        out = wide ? ge_reduce(fe_sub<20, 29>(fe_zero<FrParams>(), a)) : settle(fe_sub<4, 29>(fe_zero<FrParams>(), a));
        break;
      case GOP_MULADD: {   // a * b + c (one Horner step)
        const Fr b = src(cc.b, GF_B_PREV);
        const Fr c = src(cc.c, GF_C_PREV);
        out = settle(fe_add(fe_mul(a, b), c));
        break;
      }
      default:             // GOP_STORE
        out = a;
        break;
    }
    if (!(cc.op & GF_NO_STORE)) {
      uint32_t* p = scratch + (size_t)cc.target * 9 * T + lane_slot;
#pragma unroll
      for (int i = 0; i < 9; ++i) p[(size_t)i * T] = out.l[i];
    }
    prev = out;
  }
  // the graph's value: its last calculation (upstream GraphEvaluator::evaluate), or the given source
  Fr res = fe_zero<FrParams>();
  if (result_prev)
    res = prev;
  else if (n_calc != 0 || gsrc_kind(result_src) != GSRC_INTER)
    res = ge_fetch(result_src, from, consts, scratch, T, lane_slot);
  return res;
}

}  // namespace hm

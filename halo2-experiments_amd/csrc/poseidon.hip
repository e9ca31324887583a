// poseidon.hip -- Poseidon over BN256 Fr, the Merkle (sum) trees built from it and the witnesses of the three circuits on the device
// (DESIGN.md section 12): the kernels and the drivers poseidon_spec_create .. poseidon_witness_run.  The per-hash, per-node and
// per-lane functions and the layouts are in poseidon.inc, which host_check.cpp compiles too.
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "g1.h"
#include "hm_internal.h"
#include "host_fr.h"

namespace hm {

#include "poseidon.inc"

constexpr int PS_THREADS = 256;

__device__ __forceinline__ void ps_load_words(const uint32_t* __restrict__ p, uint32_t (&w)[8]) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 lo = q[0], hi = q[1];
  w[0] = lo.x; w[1] = lo.y; w[2] = lo.z; w[3] = lo.w;
  w[4] = hi.x; w[5] = hi.y; w[6] = hi.z; w[7] = hi.w;
}
__device__ __forceinline__ void ps_store_words(uint32_t* __restrict__ p, const uint32_t (&w)[8]) {
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(w[0], w[1], w[2], w[3]);
  q[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// message i = the W - 1 consecutive elements at in + i * in_stride (u32 words), digest i at out + i * out_stride: a flat
// message array (strides 8 (W - 1), 8) and a level of the plain width-3 tree (strides 16, 8) are the same launch
template <int W>
__global__ __launch_bounds__(PS_THREADS) void poseidon_hash_kernel(const uint32_t* __restrict__ in, uint64_t in_stride,
                                                                   uint32_t* __restrict__ out, uint64_t out_stride, uint64_t n,
                                                                   const uint32_t* __restrict__ consts, uint32_t r_f, uint32_t r_p) {
  const uint64_t i = (uint64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  if (i >= n) return;
  uint32_t msg[W - 1][8], d[8];
#pragma unroll
  for (int j = 0; j < W - 1; ++j) ps_load_words(in + i * in_stride + j * 8, msg[j]);
  poseidon_hash_one<W>(msg, consts, r_f, r_p, d);
  ps_store_words(out + i * out_stride, d);
}

// node i of a level of the sum tree from nodes 2i, 2i + 1 of the level below (16 words per node: hash, balance)
__global__ __launch_bounds__(PS_THREADS) void merkle_sum_level_kernel(const uint32_t* __restrict__ below, uint32_t* __restrict__ level,
                                                                      uint64_t n, const uint32_t* __restrict__ consts, uint32_t r_f,
                                                                      uint32_t r_p) {
  const uint64_t i = (uint64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  if (i >= n) return;
  uint32_t kids[4][8], hash[8], balance[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) ps_load_words(below + i * 32 + j * 8, kids[j]);
  fr_add_ext(kids[1], kids[3], balance);                 // merkle_sum_node_one, the balance stored before the hash runs: it does
  ps_store_words(level + i * 16 + 8, balance);           // not stay in registers across the permutation
  poseidon_hash_one<5>(kids, consts, r_f, r_p, hash);
  ps_store_words(level + i * 16, hash);
}

// sibling nodes of `m` leaves, bottom up: out[(p * depth + l) * words ..] = node ((index_p >> l) ^ 1) of level l, where level l
// starts at node 2^(depth+1) - 2^(depth-l+1) of `nodes`.  One lane per (leaf, level, element).  An index >= 2^depth gives zeros.
__global__ __launch_bounds__(PS_THREADS) void merkle_path_kernel(const uint32_t* __restrict__ nodes, uint32_t depth, uint32_t words_per_node,
                                                                 const uint64_t* __restrict__ indices, uint64_t m,
                                                                 uint32_t* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  const uint64_t per_path = (uint64_t)depth * words_per_node;
  if (t >= m * per_path) return;
  const uint64_t p = t / per_path, rest = t % per_path;
  const uint32_t l = (uint32_t)(rest / words_per_node), e = (uint32_t)(rest % words_per_node);
  const uint64_t idx = indices[p];
  uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (idx < (1ull << depth)) {
    const uint64_t level_start = (2ull << depth) - (2ull << (depth - l));
    const uint64_t node = level_start + ((idx >> l) ^ 1ull);
    ps_load_words(nodes + (node * words_per_node + e) * 8, w);
  }
  ps_store_words(out + t * 8, w);
}
// a path circuit: one lane per (user, level); the columns were cleared by the caller
template <int E>
__global__ __launch_bounds__(PS_THREADS) void merkle_witness_kernel(const WitnessArgs a) {
  const uint64_t t = (uint64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  if (t >= a.m * a.depth) return;
  merkle_witness_lane<E>(a, t / a.depth, (uint32_t)(t % a.depth));
}

// one lane per user: depth - 1 hashes in sequence (paths that come without a tree)
template <int E>
__global__ __launch_bounds__(PS_THREADS) void merkle_chain_kernel(const WitnessArgs a, uint32_t* __restrict__ run) {
  const uint64_t u = (uint64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  if (u >= a.m) return;
  merkle_chain_lane<E>(a, u, run);
}

// the Poseidon circuit: one lane per hash
__global__ __launch_bounds__(PS_THREADS) void poseidon_witness_kernel(const WitnessArgs a) {
  const uint64_t u = (uint64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  if (u >= a.m) return;
  poseidon_witness_lane(a, u);
}

// one lane per path: depth hashes in sequence
template <int E>
__global__ __launch_bounds__(PS_THREADS) void merkle_roots_kernel(const uint32_t* __restrict__ leaves, const uint32_t* __restrict__ siblings,
                                                                  const uint64_t* __restrict__ indices, uint32_t depth, uint64_t m,
                                                                  const uint32_t* __restrict__ consts, uint32_t r_f, uint32_t r_p,
                                                                  uint32_t* __restrict__ roots) {
  const uint64_t u = (uint64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  if (u >= m) return;
  merkle_root_lane<E>(leaves, siblings, indices, depth, consts, r_f, r_p, u, roots);
}

// ---- the update's launches (the plan above) ---------------------------------------------------------------------------------------
// The sort is a bitonic network on the n_pow2 keys (m << 2^depth: it is not where the time goes): every stage with partner distance
// below MU_TILE runs on a tile in LDS, the others are one launch each.
constexpr uint32_t MU_TILE = 2048;               // keys per LDS tile: 16 KiB

__global__ __launch_bounds__(PS_THREADS) void merkle_update_keys_kernel(const uint64_t* __restrict__ indices, uint64_t m, uint64_t n_pow2,
                                                                        uint32_t depth, uint64_t* __restrict__ keys) {
  const uint64_t t = (uint64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  if (t >= n_pow2) return;
  keys[t] = t < m ? merkle_update_key(indices[t], (uint32_t)t, depth) : ~0ull;
}

// one compare-exchange stage with partner distance j >= MU_TILE of the phase of length k; one lane per pair
__global__ __launch_bounds__(PS_THREADS) void merkle_update_sort_global_kernel(uint64_t* __restrict__ keys, uint64_t n, uint64_t k, uint64_t j) {
  const uint64_t t = (uint64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  if (t >= n / 2) return;
  const uint64_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
  const uint64_t a = keys[i], b = keys[l];
  if (((i & k) == 0) ? a > b : a < b) {
    keys[i] = b;
    keys[l] = a;
  }
}

// every stage with partner distance < MU_TILE of the phases k_first .. k_last (k_first = 2: the whole sort of a tile)
__global__ __launch_bounds__(PS_THREADS) void merkle_update_sort_tile_kernel(uint64_t* __restrict__ keys, uint64_t n, uint64_t k_first,
                                                                             uint64_t k_last) {
  __shared__ uint64_t lds[MU_TILE];
  const uint64_t base = (uint64_t)blockIdx.x * MU_TILE;
  const uint32_t tile = n < MU_TILE ? (uint32_t)n : MU_TILE;
  for (uint32_t e = threadIdx.x; e < tile; e += PS_THREADS) lds[e] = keys[base + e];
  __syncthreads();
  for (uint64_t k = k_first; k <= k_last; k <<= 1) {
    for (uint32_t j = (uint32_t)(k / 2 < tile ? k / 2 : tile / 2); j > 0; j >>= 1) {
      for (uint32_t t = threadIdx.x; t < tile / 2; t += PS_THREADS) {
        const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const uint64_t a = lds[i], b = lds[l];
        if ((((base + i) & k) == 0) ? a > b : a < b) {
          lds[i] = b;
          lds[l] = a;
        }
      }
      __syncthreads();
    }
  }
  for (uint32_t e = threadIdx.x; e < tile; e += PS_THREADS) keys[base + e] = lds[e];
}

// `owned` of the sorted entry p (positions >= m hold padding only)
__device__ __forceinline__ uint32_t merkle_update_owned_at(const uint64_t* __restrict__ keys, uint64_t p, uint64_t m, uint32_t depth,
                                                           uint64_t& key) {
  if (p >= m) return 0;
  key = keys[p];
  return merkle_update_owned(p ? keys[p - 1] : 0, key, p == 0, depth);
}

// hist[d] = the entries with owned = d (a workgroup counts in LDS first)
__global__ __launch_bounds__(PS_THREADS) void merkle_update_hist_kernel(const uint64_t* __restrict__ keys, uint64_t m, uint32_t depth,
                                                                        uint32_t* __restrict__ hist) {
  __shared__ uint32_t cnt[MU_BINS];
  if (threadIdx.x < MU_BINS) cnt[threadIdx.x] = 0;
  __syncthreads();
  uint64_t key = 0;
  const uint32_t d = merkle_update_owned_at(keys, (uint64_t)blockIdx.x * PS_THREADS + threadIdx.x, m, depth, key);
  if (d) atomicAdd(&cnt[d], 1u);
  __syncthreads();
  if (threadIdx.x < MU_BINS && cnt[threadIdx.x]) atomicAdd(&hist[threadIdx.x], cnt[threadIdx.x]);
}

// the counts, which are the bins' first cursors as well (bin d starts where the entries that own more levels end), and the caller's copy
__global__ __launch_bounds__(64) void merkle_update_plan_kernel(const uint32_t* __restrict__ hist, uint32_t depth, uint32_t* __restrict__ cursor,
                                                                uint32_t* __restrict__ counts, uint32_t* __restrict__ counts_out) {
  const uint32_t d = threadIdx.x;
  if (d >= MU_BINS) return;
  const uint32_t c = merkle_update_count(hist, d);
  cursor[d] = c;
  counts[d] = c;
  if (counts_out && d <= depth) counts_out[d] = c;
}

// the live entries into their bins (order[] = their leaf indices) and their leaves into level 0
template <int E>
__global__ __launch_bounds__(PS_THREADS) void merkle_update_scatter_kernel(const uint64_t* __restrict__ keys, uint64_t m, uint32_t depth,
                                                                           uint32_t* __restrict__ cursor, uint32_t* __restrict__ order,
                                                                           const uint32_t* __restrict__ new_leaves,
                                                                           uint32_t* __restrict__ nodes) {
  __shared__ uint32_t cnt[MU_BINS], base[MU_BINS];
  if (threadIdx.x < MU_BINS) cnt[threadIdx.x] = 0;
  __syncthreads();
  uint64_t key = 0;
  const uint32_t d = merkle_update_owned_at(keys, (uint64_t)blockIdx.x * PS_THREADS + threadIdx.x, m, depth, key);
  const uint32_t rank = d ? atomicAdd(&cnt[d], 1u) : 0u;
  __syncthreads();
  if (threadIdx.x < MU_BINS && cnt[threadIdx.x]) base[threadIdx.x] = atomicAdd(&cursor[threadIdx.x], cnt[threadIdx.x]);
  __syncthreads();
  if (!d) return;
  const uint32_t idx = (uint32_t)(key >> 32), pos = ~(uint32_t)key;
  order[base[d] + rank] = idx;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    uint32_t w[8];
    ps_load_words(new_leaves + ((uint64_t)pos * E + e) * 8, w);
    ps_store_words(nodes + ((uint64_t)idx * E + e) * 8, w);
  }
}

// level l: lane t < counts[l] hashes node (order[t] >> l) from its two children one level down
template <int E>
__global__ __launch_bounds__(PS_THREADS) void merkle_update_level_kernel(uint32_t* __restrict__ nodes, uint32_t depth, uint32_t l,
                                                                         const uint32_t* __restrict__ order,
                                                                         const uint32_t* __restrict__ counts,
                                                                         const uint32_t* __restrict__ consts, uint32_t r_f, uint32_t r_p) {
  const uint64_t t = (uint64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  if (t >= counts[l]) return;
  const uint64_t node = order[t] >> l;
  const uint64_t below = (2ull << depth) - (2ull << (depth - (l - 1))) + 2 * node, at = (2ull << depth) - (2ull << (depth - l)) + node;
  uint32_t kids[2 * E][8], out[E][8];
#pragma unroll
  for (int j = 0; j < 2 * E; ++j) ps_load_words(nodes + below * E * 8 + j * 8, kids[j]);
  if constexpr (E == 2)
    merkle_sum_node_one(kids, consts, r_f, r_p, out[0], out[1]);
  else
    poseidon_hash_one<3>(kids, consts, r_f, r_p, out[0]);
#pragma unroll
  for (int e = 0; e < E; ++e) ps_store_words(nodes + (at * E + e) * 8, out[e]);
}

// the constants were validated by the caller (capi_hash.hip: canonical, the shape of the spec)
int poseidon_spec_create(DeviceCtx& ctx, uint32_t width, uint32_t rate, uint32_t r_f, uint32_t r_p, const uint64_t* rc_ext,
                         const uint64_t* mds_ext, uint64_t* out_handle) {
  const size_t n_rc = (size_t)(r_f + r_p) * width, n_mds = (size_t)width * width;
  std::vector<uint32_t> h((n_rc + n_mds + 1) * 9);
  for (size_t i = 0; i < n_rc + n_mds; ++i) {
    const uint64_t* w = i < n_rc ? rc_ext + i * 4 : mds_ext + (i - n_rc) * 4;
    host::fr_to_internal9(host::fr_load(w), &h[i * 9]);
  }
  // the capacity word of ConstantLength<L>, L = rate: the field element L * 2^64, as L additions of ONE and 64 doublings
  // (a + b written as a - (0 - b): host_fr.h has no addition)
  host::Fr4 cap = {{0, 0, 0, 0}};
  const host::Fr4 zero = {{0, 0, 0, 0}};
  for (uint32_t k = 0; k < rate; ++k) cap = host::fr_sub(cap, host::fr_sub(zero, host::FR_ONE));
  for (int k = 0; k < 64; ++k) cap = host::fr_sub(cap, host::fr_sub(zero, cap));
  host::fr_to_internal9(cap, &h[(n_rc + n_mds) * 9]);
  auto s = std::make_unique<PoseidonSpec>();
  s->width = width;
  s->rate = rate;
  s->r_f = r_f;
  s->r_p = r_p;
  HM_HIP_CHECK(hipMalloc((void**)&s->d_consts, h.size() * sizeof(uint32_t)));
  if (hipError_t e = hipMemcpy(s->d_consts, h.data(), h.size() * sizeof(uint32_t), hipMemcpyHostToDevice); e != hipSuccess) {
    poseidon_spec_release(*s);
    return hm_fail(HM_ERR_HIP, std::string("hm_poseidon_create: ") + hipGetErrorString(e));
  }
  s->handle = ctx.next_handle++;
  *out_handle = s->handle;
  ctx.poseidon.push_back(std::move(s));
  return HM_OK;
}

void poseidon_spec_release(PoseidonSpec& s) {
  if (s.d_consts) (void)hipFree(s.d_consts);
  s.d_consts = nullptr;
}

int poseidon_hash_run(const PoseidonSpec& s, const uint32_t* d_in, uint64_t in_stride, uint32_t* d_out, uint64_t out_stride, size_t n,
                      hipStream_t stream) {
  if (n == 0) return HM_OK;
  const dim3 grid((unsigned)((n + PS_THREADS - 1) / PS_THREADS));
  if (s.width == 3)
    hipLaunchKernelGGL(poseidon_hash_kernel<3>, grid, dim3(PS_THREADS), 0, stream, d_in, in_stride, d_out, out_stride, (uint64_t)n,
                       s.d_consts, s.r_f, s.r_p);
  else
    hipLaunchKernelGGL(poseidon_hash_kernel<5>, grid, dim3(PS_THREADS), 0, stream, d_in, in_stride, d_out, out_stride, (uint64_t)n,
                       s.d_consts, s.r_f, s.r_p);
  HM_HIP_CHECK(hipGetLastError());
  return HM_OK;
}

// One launch per level: level l reads only level l - 1, so the chain is depth launches in stream order.  The levels that no longer
// fill the chip each take one hash latency whatever the launch shape (a node needs both children finished), so a single small kernel
// for the top would save only the launch gaps.
int merkle_build_run(const PoseidonSpec& s, uint32_t* d_nodes, uint32_t depth, hipStream_t stream) {
  const uint32_t words = s.width == 5 ? 16 : 8;
  uint64_t below = 0;                                   // first node of level l - 1
  for (uint32_t l = 1; l <= depth; ++l) {
    const uint64_t n = 1ull << (depth - l), start = below + 2 * n;
    if (s.width == 5) {
      hipLaunchKernelGGL(merkle_sum_level_kernel, dim3((unsigned)((n + PS_THREADS - 1) / PS_THREADS)), dim3(PS_THREADS), 0, stream,
                         d_nodes + below * words, d_nodes + start * words, n, s.d_consts, s.r_f, s.r_p);
      HM_HIP_CHECK(hipGetLastError());
    } else if (int rc = poseidon_hash_run(s, d_nodes + below * words, 16, d_nodes + start * words, 8, n, stream)) {
      return rc;
    }
    below = start;
  }
  return HM_OK;
}

int merkle_paths_run(const uint32_t* d_nodes, uint32_t depth, uint32_t words_per_node, const uint64_t* d_indices, size_t m,
                     uint32_t* d_out, hipStream_t stream) {
  const uint64_t lanes = (uint64_t)m * depth * words_per_node;
  if (lanes == 0) return HM_OK;
  hipLaunchKernelGGL(merkle_path_kernel, dim3((unsigned)((lanes + PS_THREADS - 1) / PS_THREADS)), dim3(PS_THREADS), 0, stream, d_nodes,
                     depth, words_per_node, d_indices, (uint64_t)m, d_out);
  HM_HIP_CHECK(hipGetLastError());
  return HM_OK;
}

int merkle_roots_run(const PoseidonSpec& s, uint32_t depth, size_t m, const uint32_t* d_leaves, const uint32_t* d_siblings,
                     const uint64_t* d_indices, uint32_t* d_roots, hipStream_t stream) {
  if (m == 0) return HM_OK;
  hipLaunchKernelGGL(s.width == 5 ? merkle_roots_kernel<2> : merkle_roots_kernel<1>, dim3((unsigned)((m + PS_THREADS - 1) / PS_THREADS)),
                     dim3(PS_THREADS), 0, stream, d_leaves, d_siblings, d_indices, depth, (uint64_t)m, s.d_consts, s.r_f, s.r_p, d_roots);
  HM_HIP_CHECK(hipGetLastError());
  return HM_OK;
}

// also keygen.hip's sort (hm_internal.h)
int merkle_update_sort(uint64_t* d_keys, uint64_t n_pow2, hipStream_t stream) {
  if (n_pow2 < 2) return HM_OK;
  const uint32_t tiles = (uint32_t)((n_pow2 + MU_TILE - 1) / MU_TILE);
  const uint64_t in_tile = n_pow2 < MU_TILE ? n_pow2 : (uint64_t)MU_TILE;
  hipLaunchKernelGGL(merkle_update_sort_tile_kernel, dim3(tiles), dim3(PS_THREADS), 0, stream, d_keys, n_pow2, (uint64_t)2, in_tile);
  for (uint64_t k = (uint64_t)MU_TILE * 2; k <= n_pow2; k <<= 1) {
    for (uint64_t j = k / 2; j >= MU_TILE; j >>= 1)
      hipLaunchKernelGGL(merkle_update_sort_global_kernel, dim3((uint32_t)((n_pow2 / 2 + PS_THREADS - 1) / PS_THREADS)), dim3(PS_THREADS), 0,
                         stream, d_keys, n_pow2, k, j);
    hipLaunchKernelGGL(merkle_update_sort_tile_kernel, dim3(tiles), dim3(PS_THREADS), 0, stream, d_keys, n_pow2, k, k);
  }
  HM_HIP_CHECK(hipGetLastError());
  return HM_OK;
}

// The plan of poseidon.inc as launches: keys, sort, histogram, counts, scatter, then one launch per level over the owners of that
// level.  Nothing comes back to the host: the grids are sized from min(m, 2^(depth - l)) and the lanes beyond the device-side count
// return.  Scratch (the keys, the ordered indices, 3 x 32 counters) is stream-ordered, as the witness entry's `run` buffer is.
static int merkle_update_launch(const PoseidonSpec& s, uint32_t* d_nodes, uint32_t depth, const uint64_t* d_indices,
                                const uint32_t* d_new_leaves, size_t m, uint32_t* d_counts, uint8_t* ws, uint64_t n_pow2, size_t o_order,
                                size_t o_small, hipStream_t stream) {
  uint64_t* d_keys = (uint64_t*)ws;
  uint32_t *d_order = (uint32_t*)(ws + o_order), *d_hist = (uint32_t*)(ws + o_small), *d_cursor = d_hist + MU_BINS, *d_cnt = d_cursor + MU_BINS;
  const auto blocks = [](uint64_t lanes) { return dim3((unsigned)((lanes + PS_THREADS - 1) / PS_THREADS)); };
  HM_HIP_CHECK(hipMemsetAsync(d_hist, 0, MU_BINS * sizeof(uint32_t), stream));
  hipLaunchKernelGGL(merkle_update_keys_kernel, blocks(n_pow2), dim3(PS_THREADS), 0, stream, d_indices, (uint64_t)m, n_pow2, depth, d_keys);
  if (int rc = merkle_update_sort(d_keys, n_pow2, stream)) return rc;
  hipLaunchKernelGGL(merkle_update_hist_kernel, blocks(m), dim3(PS_THREADS), 0, stream, (const uint64_t*)d_keys, (uint64_t)m, depth, d_hist);
  hipLaunchKernelGGL(merkle_update_plan_kernel, dim3(1), dim3(64), 0, stream, (const uint32_t*)d_hist, depth, d_cursor, d_cnt, d_counts);
  hipLaunchKernelGGL(s.width == 5 ? merkle_update_scatter_kernel<2> : merkle_update_scatter_kernel<1>, blocks(m), dim3(PS_THREADS), 0, stream,
                     (const uint64_t*)d_keys, (uint64_t)m, depth, d_cursor, d_order, d_new_leaves, d_nodes);
  for (uint32_t l = 1; l <= depth; ++l) {
    const uint64_t level = 1ull << (depth - l), lanes = m < level ? (uint64_t)m : level;
    hipLaunchKernelGGL(s.width == 5 ? merkle_update_level_kernel<2> : merkle_update_level_kernel<1>, blocks(lanes), dim3(PS_THREADS), 0, stream,
                       d_nodes, depth, l, (const uint32_t*)d_order, (const uint32_t*)d_cnt, s.d_consts, s.r_f, s.r_p);
  }
  HM_HIP_CHECK(hipGetLastError());
  return HM_OK;
}

int merkle_update_run(const PoseidonSpec& s, uint32_t* d_nodes, uint32_t depth, const uint64_t* d_indices, const uint32_t* d_new_leaves,
                      size_t m, uint32_t* d_counts, hipStream_t stream) {
  if (m == 0) {
    if (d_counts) HM_HIP_CHECK(hipMemsetAsync(d_counts, 0, (depth + 1) * sizeof(uint32_t), stream));
    return HM_OK;
  }
  uint64_t n_pow2 = 1;
  while (n_pow2 < m) n_pow2 <<= 1;
  const size_t o_order = (size_t)n_pow2 * 8, o_small = o_order + ((size_t)m * 4 + 15) / 16 * 16;
  return stream_scratch("merkle_update", o_small + 3 * MU_BINS * sizeof(uint32_t), stream, [&](uint8_t* ws) -> int {
    return merkle_update_launch(s, d_nodes, depth, d_indices, d_new_leaves, m, d_counts, ws, n_pow2, o_order, o_small, stream);
  });
}

// out = rows_used, n_advice, perm_rows, level_rows, lt_row, const_row
void witness_rows(uint32_t E, uint32_t depth, uint32_t r_f, uint32_t r_p, uint32_t (&out)[6]) {
  const WitnessLayout w = witness_layout(E, depth, r_f, r_p);
  out[0] = w.rows_used, out[1] = witness_advice(E), out[2] = w.perm_rows, out[3] = w.level_rows, out[4] = w.lt_row, out[5] = w.const_row;
}

static WitnessArgs witness_args(const PoseidonSpec& s, uint32_t depth, uint32_t log_n, size_t m, const uint32_t* d_leaves,
                                uint32_t* d_advice, uint32_t* d_instance) {
  WitnessArgs a{};
  a.leaves = d_leaves, a.advice = d_advice, a.instance = d_instance, a.consts = s.d_consts;
  a.m = m, a.depth = depth, a.log_n = log_n, a.r_f = s.r_f, a.r_p = s.r_p;
  return a;
}

// The columns are cleared, then every (user, level) lane writes its cells; without a tree a chain launch (one lane per user,
// depth - 1 hashes in sequence) first leaves the path's running nodes in stream-ordered scratch.
int merkle_witness_run(uint32_t E, const PoseidonSpec& s, uint32_t depth, uint32_t log_n, size_t m, const uint32_t* d_leaves,
                       const uint32_t* d_siblings, const uint64_t* d_indices, const uint64_t* assets_ext, const uint32_t* d_nodes,
                       uint32_t* d_advice, uint32_t* d_instance, hipStream_t stream) {
  if (m == 0) return HM_OK;
  const std::string who = E == 2 ? "merkle_sum_witness" : "merkle_witness";
  WitnessArgs a = witness_args(s, depth, log_n, m, d_leaves, d_advice, d_instance);
  a.siblings = d_siblings, a.indices = d_indices, a.nodes = d_nodes;
  if (E == 2) std::memcpy(a.assets, assets_ext, 32);
  HM_HIP_CHECK(hipMemsetAsync(d_advice, 0, (size_t)m * witness_advice(E) * ((size_t)32 << log_n), stream));
  const size_t run_bytes = !d_nodes && depth > 1 ? (size_t)m * (depth - 1) * E * 32 : 0;      // with a tree: 0 bytes, no buffer
  return stream_scratch(who.c_str(), run_bytes, stream, [&](uint8_t* run) -> int {
    int rc = HM_OK;
    if (run) {
      a.run = (const uint32_t*)run;
      hipLaunchKernelGGL(E == 2 ? merkle_chain_kernel<2> : merkle_chain_kernel<1>, dim3((unsigned)((m + PS_THREADS - 1) / PS_THREADS)),
                         dim3(PS_THREADS), 0, stream, a, (uint32_t*)run);
      if (hipError_t e = hipGetLastError(); e != hipSuccess) rc = hm_fail(HM_ERR_HIP, who + ": " + hipGetErrorString(e));
    }
    if (rc == HM_OK) {
      const uint64_t lanes = (uint64_t)m * depth;
      hipLaunchKernelGGL(E == 2 ? merkle_witness_kernel<2> : merkle_witness_kernel<1>, dim3((unsigned)((lanes + PS_THREADS - 1) / PS_THREADS)),
                         dim3(PS_THREADS), 0, stream, a);
      if (hipError_t e = hipGetLastError(); e != hipSuccess) rc = hm_fail(HM_ERR_HIP, who + ": " + hipGetErrorString(e));
    }
    return rc;
  });
}

int poseidon_witness_run(const PoseidonSpec& s, uint32_t log_n, size_t m, const uint32_t* d_msgs, uint32_t* d_advice, uint32_t* d_instance,
                         hipStream_t stream) {
  if (m == 0) return HM_OK;
  const WitnessArgs a = witness_args(s, 0, log_n, m, d_msgs, d_advice, d_instance);
  HM_HIP_CHECK(hipMemsetAsync(d_advice, 0, (size_t)m * witness_advice(0) * ((size_t)32 << log_n), stream));
  hipLaunchKernelGGL(poseidon_witness_kernel, dim3((unsigned)((m + PS_THREADS - 1) / PS_THREADS)), dim3(PS_THREADS), 0, stream, a);
  HM_HIP_CHECK(hipGetLastError());
  return HM_OK;
}

}  // namespace hm

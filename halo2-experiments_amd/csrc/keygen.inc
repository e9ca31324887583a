// keygen.inc -- permutation::keygen::Assembly on cell ids (DESIGN.md section 16): the packing of the sort keys and the link rule as
// HM_HD functions (host_check.cpp runs them on a host-sorted list), and the kernels of the union, the keys and the links.  Included
// inside namespace hm, after poseidon.inc (PS_THREADS; the sort is merkle_update's network, unchanged).
//
// A cell id is j * n + i: column j in cs.equality order, row i, n = 2^k; cells = columns * n <= 2^32.  sigma as cells:
//   - a cell no copy names maps to itself;
//   - the members of a class, by ascending id, each map to the next one, the last to the first;
// so the result depends on the SET of copies alone.  The plan:
//   union    sigma_cells, filled with the identity, is the parent array of a lock-free union-find: a lane per copy finds the two
//            roots and hooks the LARGER under the smaller by compare-and-swap (retrying from the word it lost to).  Pointers only
//            ever go down, so there is no cycle and the root of a class is its smallest cell.
//   keys     endpoint t of copy t / 2 -> (root << 32) | cell; a copy with an id >= cells gives two pads (all ones) and is counted
//   sort     ascending: the classes one after another, each by ascending cell, repeated endpoints adjacent, the pads last
//   link     the last entry of a run of equal keys writes sigma_cells[cell] = the next entry's cell when that has the same root,
//            else the root (which is the first of the class).  Every word the union changed belongs to an endpoint, and every
//            endpoint is written here, so nothing of the parent forest is left behind.
constexpr uint64_t PERM_PAD = ~0ull;

HM_HD uint64_t perm_key(uint32_t root, uint32_t cell) { return ((uint64_t)root << 32) | cell; }

// entry `key` of the sorted list, `next` behind it (PERM_PAD behind the last): true when the entry writes sigma_cells[cell] = target.
// The pad itself is the key of cell 2^32 - 1 alone in its class, which maps to itself: nothing to write either.
HM_HD bool perm_link(uint64_t key, uint64_t next, uint32_t& cell, uint32_t& target) {
  if (key == PERM_PAD || key == next) return false;
  const uint32_t root = (uint32_t)(key >> 32);
  cell = (uint32_t)key;
  target = (uint32_t)(next >> 32) == root ? (uint32_t)next : root;
  return true;
}

#if defined(__HIPCC__)
__global__ __launch_bounds__(PS_THREADS) void perm_identity_kernel(uint32_t* __restrict__ cells_out, uint64_t cells) {
  const uint64_t c = (uint64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  if (c < cells) cells_out[c] = (uint32_t)c;
}

// The parent words are read and written by lanes of every XCD while the kernel runs: device-scope accesses throughout.  A stale
// word is still an ancestor (pointers only go down), and a hook is decided by the compare-and-swap alone.
__device__ __forceinline__ uint32_t perm_parent(const uint32_t* parent, uint32_t x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t perm_find_halving(uint32_t* parent, uint32_t x) {
  for (;;) {
    const uint32_t p = perm_parent(parent, x);
    if (p == x) return x;
    const uint32_t g = perm_parent(parent, p);
    if (g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = g;
  }
}

__global__ __launch_bounds__(PS_THREADS) void perm_union_kernel(const uint2* __restrict__ copies, uint64_t m, uint64_t cells,
                                                                uint32_t* parent) {
  const uint64_t t = (uint64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  if (t >= m) return;
  const uint2 pair = copies[t];
  if (pair.x >= cells || pair.y >= cells) return;
  uint32_t a = perm_find_halving(parent, pair.x), b = perm_find_halving(parent, pair.y);
  while (a != b) {
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    const uint32_t seen = atomicCAS(parent + hi, hi, lo);
    if (seen == hi) break;
    a = perm_find_halving(parent, seen);        // hi was hooked meanwhile: go on from where it points
    b = perm_find_halving(parent, lo);
  }
}

// after the union has finished: plain reads, nothing is written to the forest
__global__ __launch_bounds__(PS_THREADS) void perm_keys_kernel(const uint32_t* __restrict__ copies, uint64_t m, uint64_t n_pow2,
                                                               uint64_t cells, const uint32_t* __restrict__ parent,
                                                               uint64_t* __restrict__ keys, uint32_t* __restrict__ dropped) {
  const uint64_t t = (uint64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  if (t >= n_pow2) return;
  uint64_t key = PERM_PAD;
  if (t < 2 * m) {
    const uint32_t cell = copies[t], other = copies[t ^ 1];
    if (cell < cells && other < cells) {
      uint32_t r = cell;
      for (uint32_t p = parent[r]; p != r; p = parent[r]) r = p;
      key = perm_key(r, cell);
    } else if (dropped && !(t & 1)) {
      atomicAdd(dropped, 1u);
    }
  }
  keys[t] = key;
}

__global__ __launch_bounds__(PS_THREADS) void perm_link_kernel(const uint64_t* __restrict__ keys, uint64_t entries, uint64_t n_pow2,
                                                               uint32_t* __restrict__ sigma_cells) {
  const uint64_t p = (uint64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  if (p >= entries) return;
  uint32_t cell, target;
  if (perm_link(keys[p], p + 1 < n_pow2 ? keys[p + 1] : PERM_PAD, cell, target)) sigma_cells[cell] = target;
}
#endif

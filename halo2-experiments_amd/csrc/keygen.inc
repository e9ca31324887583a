// keygen.inc -- permutation::keygen::Assembly on cell ids (DESIGN.md section 16): the packing of the sort keys and the link rule as
// HM_HD functions (host_check.cpp runs them on a host-sorted list); the kernels of the union, the keys and the links are in keygen.hip.
// Included inside namespace hm (the sort is merkle_update's network, unchanged).
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

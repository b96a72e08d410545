// BVH image shared by mesh_host.cpp (builder) and mesh_sdf.hip (walker); private to the library.
//   [BvhHeader 16 B][BvhNode x n_nodes, 32 B each][pad to 16 B][triangles: 9 floats each, in leaf order]
// Nodes are in depth-first pre-order: the left child of an inner node i is i+1, escape is the first node after
// i's subtree (n_nodes for the last subtree).  leaf = (first << 3) | count for a leaf of count (1..kBvhLeaf)
// triangles starting at triangle slot `first`; 0 for an inner node.
#pragma once

#include <cstddef>
#include <cstdint>

namespace disn {

constexpr int32_t kBvhMagic = 0x48564244;  // "DBVH"
constexpr int kBvhLeaf = 4;
constexpr int64_t kBvhMaxTris = int64_t(1) << 27;

struct BvhHeader {
  int32_t magic, n_nodes, n_tris, reserved;
};

struct BvhNode {
  float lo[3];
  int32_t escape;
  float hi[3];
  int32_t leaf;
};
static_assert(sizeof(BvhNode) == 32, "two 16-byte loads per node");

inline size_t bvh_tri_offset(int64_t nf) {
  return (sizeof(BvhHeader) + (size_t)(2 * nf) * sizeof(BvhNode) + 15) & ~(size_t)15;
}
inline size_t bvh_bytes(int64_t nf) { return bvh_tri_offset(nf) + (size_t)nf * 9 * sizeof(float); }

}  // namespace disn

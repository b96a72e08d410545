// Host side of mesh-to-SDF preprocessing (no device code).
//   disn_read_obj_mesh  -- Wavefront .obj vertices and faces (fan-triangulated polygons), count-then-fill
//   disn_mesh_components -- connected components of the triangles (edge or vertex connectivity), union-find
//   disn_mesh_bvh_build -- deterministic BVH over the triangle soup, laid out for the stackless walk of
//                          mesh_sdf.hip and render.hip (node format: mesh_bvh.hpp, private to the library);
//                          disn_mesh_bvh_build_order also returns the slot -> face map of the leaf order
#include "../../include/disn_amd.h"
#include "mesh_bvh.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

bool read_file(const char* path, std::string& buf) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  char chunk[1 << 16];
  size_t got;
  while ((got = std::fread(chunk, 1, sizeof chunk, f)) > 0) buf.append(chunk, got);
  const bool ok = std::ferror(f) == 0;
  std::fclose(f);
  return ok;
}

inline bool is_space(char c) { return c == ' ' || c == '\t' || c == '\r'; }

// one "f" token: v, v/vt, v//vn or v/vt/vn; only v is used.  1-based, negative = relative to the vertices
// read so far.  Returns false on a malformed or out-of-range index.
bool face_index(const char*& q, const char* eol, int64_t nv_so_far, int64_t& out) {
  char* next = nullptr;
  const long long i = std::strtoll(q, &next, 10);
  if (next == q || next > eol) return false;
  q = next;
  while (q < eol && !is_space(*q)) ++q;  // skip /vt/vn
  int64_t k;
  if (i > 0) k = i - 1;
  else if (i < 0) k = nv_so_far + i;
  else return false;
  if (k < 0 || k >= nv_so_far) return false;
  out = k;
  return true;
}

}  // namespace

extern "C" int disn_read_obj_mesh(const char* path, float* verts, int64_t vcap, int32_t* faces, int64_t fcap,
                                  int64_t* counts) {
  if (!path || !counts || vcap < 0 || fcap < 0 || (vcap > 0 && !verts) || (fcap > 0 && !faces))
    return DISN_E_ARG;
  std::string buf;
  if (!read_file(path, buf)) return DISN_E_ARG;
  int64_t nv = 0, nf = 0;
  std::vector<int64_t> poly;
  const char* p = buf.c_str();
  const char* end = p + buf.size();
  while (p < end) {
    const char* eol = static_cast<const char*>(std::memchr(p, '\n', end - p));
    if (!eol) eol = end;
    const char* q = p;
    while (q < eol && is_space(*q)) ++q;
    if (eol - q >= 2 && q[0] == 'v' && is_space(q[1])) {
      q += 2;
      float xyz[3];
      for (int c = 0; c < 3; ++c) {
        char* next = nullptr;
        xyz[c] = std::strtof(q, &next);
        if (next == q || next > eol) return DISN_E_ARG;
        q = next;
      }
      if (nv < vcap) std::memcpy(verts + 3 * nv, xyz, sizeof xyz);
      ++nv;
    } else if (eol - q >= 2 && q[0] == 'f' && is_space(q[1])) {
      q += 2;
      poly.clear();
      for (;;) {
        while (q < eol && is_space(*q)) ++q;
        if (q >= eol) break;
        int64_t k;
        if (!face_index(q, eol, nv, k)) return DISN_E_ARG;
        if (k > INT32_MAX) return DISN_E_SHAPE;
        poly.push_back(k);
      }
      if (poly.size() < 3) return DISN_E_ARG;
      for (size_t t = 1; t + 1 < poly.size(); ++t) {  // fan: (0, t, t+1) in file order
        if (nf < fcap) {
          faces[3 * nf] = (int32_t)poly[0];
          faces[3 * nf + 1] = (int32_t)poly[t];
          faces[3 * nf + 2] = (int32_t)poly[t + 1];
        }
        ++nf;
      }
    }
    p = eol + 1;
  }
  counts[0] = nv;
  counts[1] = nf;
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// BVH: median split of the triangle centroids (a+b+c, fp32) along the widest centroid axis, ties between equal
// centroids broken by triangle index, so the partition is a function of the input alone.  Leaves hold at most
// kBvhLeaf triangles, sorted by index.  Nodes are emitted in depth-first pre-order: the left child of node i is
// i+1, and escape(i) is the first node after i's subtree -- the walk needs no stack.  Every node box is the
// exact fp32 bound of its triangles' vertices, inflated by 2^-18 of its largest coordinate magnitude, which
// covers the rounding of the fp32 closest point.
namespace {

struct Builder {
  const float* v;
  const int32_t* f;
  std::vector<int32_t> idx;
  std::vector<float> cen;  // 3 per triangle
  std::vector<disn::BvhNode> nodes;

  void tri_bounds(int32_t t, float lo[3], float hi[3]) const {
    for (int k = 0; k < 3; ++k) {
      const float* p = v + 3 * (int64_t)f[3 * (int64_t)t + k];
      for (int a = 0; a < 3; ++a) {
        lo[a] = std::min(lo[a], p[a]);
        hi[a] = std::max(hi[a], p[a]);
      }
    }
  }

  void build(int64_t lo_i, int64_t hi_i) {
    const int64_t k = (int64_t)nodes.size();
    nodes.push_back(disn::BvhNode{});
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = lo_i; i < hi_i; ++i) tri_bounds(idx[i], lo, hi);
    const int64_t count = hi_i - lo_i;
    int32_t leaf = 0;
    if (count <= disn::kBvhLeaf) {
      std::sort(idx.begin() + lo_i, idx.begin() + hi_i);
      leaf = (int32_t)((lo_i << 3) | count);
    } else {
      float clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
      for (int64_t i = lo_i; i < hi_i; ++i)
        for (int a = 0; a < 3; ++a) {
          clo[a] = std::min(clo[a], cen[3 * (int64_t)idx[i] + a]);
          chi[a] = std::max(chi[a], cen[3 * (int64_t)idx[i] + a]);
        }
      int ax = 0;
      for (int a = 1; a < 3; ++a)
        if (chi[a] - clo[a] > chi[ax] - clo[ax]) ax = a;
      const int64_t mid = lo_i + count / 2;
      const float* c = cen.data();
      std::nth_element(idx.begin() + lo_i, idx.begin() + mid, idx.begin() + hi_i, [c, ax](int32_t x, int32_t y) {
        const float cx = c[3 * (int64_t)x + ax], cy = c[3 * (int64_t)y + ax];
        return cx < cy || (cx == cy && x < y);
      });
      build(lo_i, mid);
      build(mid, hi_i);
    }
    float m = 0.0f;
    for (int a = 0; a < 3; ++a) m = std::max(m, std::max(std::fabs(lo[a]), std::fabs(hi[a])));
    const float d = std::ldexp(m, -18);
    disn::BvhNode& n = nodes[k];
    for (int a = 0; a < 3; ++a) {
      n.lo[a] = lo[a] - d;
      n.hi[a] = hi[a] + d;
    }
    n.escape = (int32_t)nodes.size();
    n.leaf = leaf;
  }
};

}  // namespace

extern "C" size_t disn_mesh_bvh_bytes(int64_t nf) {
  if (nf < 1 || nf > disn::kBvhMaxTris) return 0;
  return disn::bvh_bytes(nf);
}

extern "C" int disn_mesh_bvh_build_order(const float* verts, int64_t nv, const int32_t* faces, int64_t nf,
                                         void* out, size_t out_bytes, int32_t* order) {
  if (!verts || !faces || !out || nv < 1 || nf < 1) return DISN_E_ARG;
  if (nf > disn::kBvhMaxTris || nv > INT32_MAX) return DISN_E_SHAPE;   // the faces index the vertices in int32
  if (out_bytes < disn::bvh_bytes(nf)) return DISN_E_WS;
  for (int64_t i = 0; i < 3 * nf; ++i)
    if (faces[i] < 0 || faces[i] >= nv) return DISN_E_ARG;
  Builder b;
  b.v = verts;
  b.f = faces;
  b.idx.resize(nf);
  b.cen.resize(3 * nf);
  for (int64_t t = 0; t < nf; ++t) {
    b.idx[t] = (int32_t)t;
    const float* p0 = verts + 3 * (int64_t)faces[3 * t];
    const float* p1 = verts + 3 * (int64_t)faces[3 * t + 1];
    const float* p2 = verts + 3 * (int64_t)faces[3 * t + 2];
    for (int a = 0; a < 3; ++a) b.cen[3 * t + a] = (p0[a] + p1[a]) + p2[a];
  }
  b.nodes.reserve(2 * nf);
  b.build(0, nf);
  std::memset(out, 0, disn::bvh_bytes(nf));
  disn::BvhHeader h{disn::kBvhMagic, (int32_t)b.nodes.size(), (int32_t)nf, 0};
  char* o = static_cast<char*>(out);
  std::memcpy(o, &h, sizeof h);
  std::memcpy(o + sizeof h, b.nodes.data(), b.nodes.size() * sizeof(disn::BvhNode));
  float* tri = reinterpret_cast<float*>(o + disn::bvh_tri_offset(nf));
  for (int64_t i = 0; i < nf; ++i) {
    const int32_t t = b.idx[i];
    for (int k = 0; k < 3; ++k) std::memcpy(tri + 9 * i + 3 * k, verts + 3 * (int64_t)faces[3 * (int64_t)t + k],
                                            3 * sizeof(float));
  }
  if (order) std::memcpy(order, b.idx.data(), (size_t)nf * sizeof(int32_t));
  return 0;
}

extern "C" int disn_mesh_bvh_build(const float* verts, int64_t nv, const int32_t* faces, int64_t nf, void* out,
                                   size_t out_bytes) {
  return disn_mesh_bvh_build_order(verts, nv, faces, nf, out, out_bytes, nullptr);
}

// ---- connected components of a triangle soup (postprocessing/clean_smallparts.py: pymesh.separate_mesh) ----
namespace {

struct DisjointSet {
  std::vector<int32_t> parent;
  explicit DisjointSet(int64_t n) : parent(n) {
    for (int64_t i = 0; i < n; ++i) parent[i] = (int32_t)i;
  }
  int32_t find(int32_t x) {
    while (parent[x] != x) {
      parent[x] = parent[parent[x]];
      x = parent[x];
    }
    return x;
  }
  void unite(int32_t a, int32_t b) {   // the smaller index becomes the root
    a = find(a);
    b = find(b);
    if (a == b) return;
    if (a < b) parent[b] = a;
    else parent[a] = b;
  }
};

}  // namespace

extern "C" int disn_mesh_components(const int32_t* faces, int64_t nf, int64_t nv, int connectivity, int32_t* labels,
                                    int64_t* ncomp) {
  if (nf < 0 || nv < 0 || !ncomp || (nf > 0 && (!faces || !labels)) || (connectivity != 0 && connectivity != 1))
    return DISN_E_ARG;
  if (nf > INT32_MAX / 3 || nv > INT32_MAX) return DISN_E_SHAPE;
  for (int64_t i = 0; i < 3 * nf; ++i)
    if (faces[i] < 0 || faces[i] >= nv) return DISN_E_ARG;
  DisjointSet ds(nf);
  if (connectivity == 1) {
    std::vector<int32_t> first(nv, -1);   // the first triangle seen at a vertex
    for (int64_t t = 0; t < nf; ++t)
      for (int k = 0; k < 3; ++k) {
        int32_t& f = first[faces[3 * t + k]];
        if (f < 0) f = (int32_t)t;
        else ds.unite(f, (int32_t)t);
      }
  } else {
    struct Edge {
      uint64_t key;
      int32_t tri;
    };
    std::vector<Edge> edges(3 * nf);
    for (int64_t t = 0; t < nf; ++t)
      for (int k = 0; k < 3; ++k) {
        const uint64_t a = (uint64_t)faces[3 * t + k], b = (uint64_t)faces[3 * t + (k + 1) % 3];
        edges[3 * t + k] = Edge{std::min(a, b) << 32 | std::max(a, b), (int32_t)t};
      }
    std::sort(edges.begin(), edges.end(),
              [](const Edge& x, const Edge& y) { return x.key < y.key || (x.key == y.key && x.tri < y.tri); });
    for (size_t i = 1; i < edges.size(); ++i)
      if (edges[i].key == edges[i - 1].key) ds.unite(edges[i - 1].tri, edges[i].tri);
  }
  // a root is its component's smallest triangle, so roots appear in rank order
  std::vector<int32_t> id(nf, -1);
  int64_t n = 0;
  for (int64_t t = 0; t < nf; ++t) {
    const int32_t r = ds.find((int32_t)t);
    if (id[r] < 0) id[r] = (int32_t)n++;
    labels[t] = id[r];
  }
  *ncomp = n;
  return 0;
}

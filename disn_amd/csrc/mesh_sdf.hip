// Mesh-to-SDF preprocessing (preprocessing/create_point_sdf_grid.py of the reference, whose distance field comes
// from a closed binary): unsigned distance to a triangle soup and an orientation-free sign, on gfx950.
// THIS FILE IS COMPILED WITH -ffp-contract=off: every expression below is restated operation for operation in
// tests/mesh_sdf_reference.py and the results are compared bit for bit.
//
// Unsigned distance u(p) = sqrt(min_T d2(p, T)).  d2 is the fp32 region-based closest point of Ericson
// (Real-Time Collision Detection §5.1.5) with every division guarded (a zero denominator gives 0), a
// degenerate-interior fall-back to the three edges, and for slivers (sin^2 of the angle at a <= 2^-20,
// cross = (ay*bz - az*by, az*bx - ax*bz, ax*by - ay*bx)) the minimum with the three edge distances, so that
// sliver, collinear and repeated-vertex triangles give finite, accurate values.  In the face region a point with
// n . (p - a) == 0 (n = cross, fp32) lies in the face: d2 = 0 exactly, so a point on a vertex or in the face has
// u == 0 whatever vb / s and vc / s round to (an edge point: when its parameter is exact); p is then inside the leaf's
// inflated box, so the walk below keeps the leaf (tests/test_gpu_geometry_lattice.py).  dot(a, b) = (ax*bx + ay*by) + az*bz,
// d2 = (dx*dx + dy*dy) + dz*dz, one correctly rounded sqrtf of the minimum (HIP's default fp32 sqrt lowering: correctly rounded, not v_sqrt_f32 alone).
// The BVH walk is stackless (depth-first node order + escape links, mesh_bvh.hpp): one greedy descent to the
// nearer child seeds the bound, then the full walk prunes a box when box_d2 > best * (1 + 2^-18).  Boxes are
// inflated by 2^-18 of their largest coordinate at build time, so the computed closest point of every triangle
// lies inside its leaf's box and the pruning can never drop the triangle that attains the minimum: the BVH
// result is bit-identical to the brute-force loop (brute = 1) over every triangle.
// Grid form: one 64-lane workgroup per 4x4x4 brick of nodes (the lanes of a wave walk nearly the same path).
//
// Sign.  tau = seal * h_max, F = {u >= tau}:
//   1. far flood: 6-connected components of F by label propagation (hook with atomicMin on the label of the
//      current root, then pointer jumping), at most kCclMaxIter rounds, each ended by one 4-byte read of a
//      "changed" flag: no grid barrier, no device-side spin.  The converged label of a component is its lowest
//      flat index whatever the scheduling.  O_far = components holding a node of the box boundary.
//   2. band flood: `steps` Jacobi steps; a band node (u < tau) becomes outside when a 6-neighbour is outside and
//      the closed grid edge between them crosses no closed triangle.  Crossing test (fp64 from the fp32 inputs,
//      edge along axis a at (s_b, s_c), b = (a+1)%3, c = (a+2)%3, coordinates relative to (s_b, s_c)):
//        wp = qb*rc - qc*rb;  wq = rb*pc - rc*pb;  wr = pb*qc - pc*qb;  area = (wp + wq) + wr
//        area == 0: ignored; hit when all three >= 0 or all <= 0; x = ((wp*pa + wq*qa) + wr*ra) / area,
//        crossing when min(x0, x1) <= x <= max(x0, x1).  Candidates come from the same BVH (closed boxes).
//   3. sdf = (outside ? u : -u) - offset.
#include "../../include/disn_amd.h"
#include "kernels.hpp"
#include "mesh_bvh.hpp"

namespace disn {

namespace {

constexpr float kPrune = 1.0f + 0x1p-18f;
constexpr int kCclMaxIter = 4096;

struct V3 {
  float x, y, z;
};
__device__ __forceinline__ V3 ld3(const float* p) { return V3{p[0], p[1], p[2]}; }
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 axpy(V3 a, float t, V3 d) { return V3{a.x + t * d.x, a.y + t * d.y, a.z + t * d.z}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ float dist2(V3 p, V3 q) {
  const V3 d = sub(p, q);
  return (d.x * d.x + d.y * d.y) + d.z * d.z;
}

__device__ __forceinline__ float seg_d2(V3 p, V3 a, V3 b) {
  const V3 ab = sub(b, a);
  const float den = dot(ab, ab);
  float t = den > 0.0f ? dot(sub(p, a), ab) / den : 0.0f;
  t = fminf(fmaxf(t, 0.0f), 1.0f);
  return dist2(p, axpy(a, t, ab));
}

__device__ __forceinline__ V3 cross(V3 a, V3 b) {
  return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

__device__ float ericson_d2(V3 p, V3 a, V3 b, V3 c, V3 ab, V3 ac, V3 n) {
  const V3 ap = sub(p, a);
  const float d1 = dot(ab, ap), d2 = dot(ac, ap);
  if (d1 <= 0.0f && d2 <= 0.0f) return dist2(p, a);
  const V3 bp = sub(p, b);
  const float d3 = dot(ab, bp), d4 = dot(ac, bp);
  if (d3 >= 0.0f && d4 <= d3) return dist2(p, b);
  const float vc = d1 * d4 - d3 * d2;
  if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
    const float den = d1 - d3;
    return dist2(p, axpy(a, den > 0.0f ? d1 / den : 0.0f, ab));
  }
  const V3 cp = sub(p, c);
  const float d5 = dot(ab, cp), d6 = dot(ac, cp);
  if (d6 >= 0.0f && d5 <= d6) return dist2(p, c);
  const float vb = d5 * d2 - d1 * d6;
  if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
    const float den = d2 - d6;
    return dist2(p, axpy(a, den > 0.0f ? d2 / den : 0.0f, ac));
  }
  const float va = d3 * d6 - d5 * d4;
  const float e1 = d4 - d3, e2 = d5 - d6;
  if (va <= 0.0f && e1 >= 0.0f && e2 >= 0.0f) {
    const float den = e1 + e2;
    return dist2(p, axpy(b, den > 0.0f ? e1 / den : 0.0f, sub(c, b)));
  }
  const float s = (va + vb) + vc;
  if (va >= 0.0f && vb >= 0.0f && vc >= 0.0f && s > 0.0f) {
    if (dot(n, ap) == 0.0f) return 0.0f;   // in the face's plane, foot in the face: ON the triangle (vb / s may round)
    const float v = vb / s, w = vc / s;
    return dist2(p, axpy(axpy(a, v, ab), w, ac));
  }
  return fminf(fminf(seg_d2(p, a, b), seg_d2(p, b, c)), seg_d2(p, c, a));
}

// A sliver (sin^2 of the angle at a <= 2^-20, zero-area faces included) makes the region tests noise: its
// distance is also bounded by the three edges, and the smaller value is kept.
__device__ float tri_d2(V3 p, const float* __restrict__ t) {
  const V3 a = ld3(t), b = ld3(t + 3), c = ld3(t + 6);
  const V3 ab = sub(b, a), ac = sub(c, a);
  const V3 n = cross(ab, ac);
  const float d = ericson_d2(p, a, b, c, ab, ac, n);
  if (dot(n, n) > 0x1p-20f * (dot(ab, ab) * dot(ac, ac))) return d;
  return fminf(d, fminf(fminf(seg_d2(p, a, b), seg_d2(p, b, c)), seg_d2(p, c, a)));
}

__device__ __forceinline__ float box_d2(V3 p, float4 lo, float4 hi) {
  const float ex = fmaxf(fmaxf(lo.x - p.x, p.x - hi.x), 0.0f);
  const float ey = fmaxf(fmaxf(lo.y - p.y, p.y - hi.y), 0.0f);
  const float ez = fmaxf(fmaxf(lo.z - p.z, p.z - hi.z), 0.0f);
  return (ex * ex + ey * ey) + ez * ez;
}

struct Bvh {
  const float4* nodes;  // 2 per node: (lo.xyz, escape bits), (hi.xyz, leaf bits)
  const float* tris;
  int n_tris;
};

__device__ __forceinline__ int n_nodes_of(const Bvh& h) {
  return reinterpret_cast<const BvhHeader*>(reinterpret_cast<const char*>(h.nodes) - sizeof(BvhHeader))->n_nodes;
}

__device__ __forceinline__ float leaf_min(const Bvh& h, int leaf, V3 p, float best) {
  const int first = leaf >> 3, cnt = leaf & 7;
  for (int t = 0; t < cnt; ++t) best = fminf(best, tri_d2(p, h.tris + 9 * (size_t)(first + t)));
  return best;
}

__device__ float min_d2(const Bvh& h, V3 p, int brute) {
  float best = INFINITY;
  if (brute) {
    for (int t = 0; t < h.n_tris; ++t) best = fminf(best, tri_d2(p, h.tris + 9 * (size_t)t));
    return best;
  }
  const int n = n_nodes_of(h);
  // seed: greedy descent to the nearer child (left = i+1, right = escape(i+1))
  int i = 0;
  for (;;) {
    const int leaf = __float_as_int(h.nodes[2 * i + 1].w);
    if (leaf) {
      best = leaf_min(h, leaf, p, best);
      break;
    }
    const int l = i + 1, r = __float_as_int(h.nodes[2 * l].w);
    const float dl = box_d2(p, h.nodes[2 * l], h.nodes[2 * l + 1]);
    const float dr = box_d2(p, h.nodes[2 * r], h.nodes[2 * r + 1]);
    i = dr < dl ? r : l;
  }
  i = 0;
  while (i < n) {
    const float4 lo = h.nodes[2 * i], hi = h.nodes[2 * i + 1];
    const int escape = __float_as_int(lo.w), leaf = __float_as_int(hi.w);
    if (box_d2(p, lo, hi) > best * kPrune) {
      i = escape;
    } else if (leaf) {
      best = leaf_min(h, leaf, p, best);
      i = escape;
    } else {
      ++i;
    }
  }
  return best;
}

__global__ __launch_bounds__(256) void udf_points_kernel(Bvh h, const float* __restrict__ pts, int64_t n, int brute,
                                                         float* __restrict__ dist) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  dist[i] = sqrtf(min_d2(h, ld3(pts + 3 * i), brute));
}

// one workgroup (one wave) per 4x4x4 brick; lane = lx + 4*ly + 16*lz
__global__ __launch_bounds__(64) void udf_grid_kernel(Bvh h, const float* __restrict__ xs,
                                                      const float* __restrict__ ys, const float* __restrict__ zs,
                                                      int nx, int ny, int nz, int brute, float* __restrict__ dist) {
  const int bx = (nx + 3) >> 2, by = (ny + 3) >> 2;
  const int64_t brick = blockIdx.x;
  const int cx = (int)(brick % bx), cy = (int)((brick / bx) % by), cz = (int)(brick / ((int64_t)bx * by));
  const int ix = 4 * cx + (threadIdx.x & 3), iy = 4 * cy + ((threadIdx.x >> 2) & 3), iz = 4 * cz + (threadIdx.x >> 4);
  if (ix >= nx || iy >= ny || iz >= nz) return;
  const V3 p{xs[ix], ys[iy], zs[iz]};
  dist[((int64_t)iz * ny + iy) * nx + ix] = sqrtf(min_d2(h, p, brute));
}

// ---- sign ---------------------------------------------------------------------------------------------------
struct Grid {
  const float* ax[3];
  int n[3];
};

__device__ __forceinline__ float comp(float4 v, int a) { return a == 0 ? v.x : (a == 1 ? v.y : v.z); }

__device__ bool tri_crosses(const float* __restrict__ t, int a, int b, int c, double sb, double sc, double x0,
                            double x1) {
  const double pb = (double)t[b] - sb, pc = (double)t[c] - sc;
  const double qb = (double)t[3 + b] - sb, qc = (double)t[3 + c] - sc;
  const double rb = (double)t[6 + b] - sb, rc = (double)t[6 + c] - sc;
  const double wp = qb * rc - qc * rb;
  const double wq = rb * pc - rc * pb;
  const double wr = pb * qc - pc * qb;
  const double area = (wp + wq) + wr;
  if (area == 0.0) return false;
  const bool hit = (wp >= 0.0 && wq >= 0.0 && wr >= 0.0) || (wp <= 0.0 && wq <= 0.0 && wr <= 0.0);
  if (!hit) return false;
  const double x = ((wp * (double)t[a] + wq * (double)t[3 + a]) + wr * (double)t[6 + a]) / area;
  return x0 <= x && x <= x1;
}

// does the closed edge along axis a, from xa0 to xa1 at (sb, sc), cross a closed triangle?
__device__ bool edge_crosses(const Bvh& h, int n_nodes, int a, float xa0, float xa1, float sb, float sc) {
  const int b = a == 2 ? 0 : a + 1, c = a == 0 ? 2 : a - 1;
  const float lo_x = fminf(xa0, xa1), hi_x = fmaxf(xa0, xa1);
  int i = 0;
  while (i < n_nodes) {
    const float4 lo = h.nodes[2 * i], hi = h.nodes[2 * i + 1];
    const int escape = __float_as_int(lo.w), leaf = __float_as_int(hi.w);
    const bool miss = comp(lo, a) > hi_x || comp(hi, a) < lo_x || comp(lo, b) > sb || comp(hi, b) < sb ||
                      comp(lo, c) > sc || comp(hi, c) < sc;
    if (miss) {
      i = escape;
    } else if (leaf) {
      const int first = leaf >> 3, cnt = leaf & 7;
      for (int t = 0; t < cnt; ++t)
        if (tri_crosses(h.tris + 9 * (size_t)(first + t), a, b, c, sb, sc, lo_x, hi_x)) return true;
      i = escape;
    } else {
      ++i;
    }
  }
  return false;
}

__device__ __forceinline__ void unflat(const Grid& g, int64_t i, int& ix, int& iy, int& iz) {
  ix = (int)(i % g.n[0]);
  iy = (int)((i / g.n[0]) % g.n[1]);
  iz = (int)(i / ((int64_t)g.n[0] * g.n[1]));
}

__global__ __launch_bounds__(256) void far_init_kernel(const float* __restrict__ u, int64_t N, float tau,
                                                       int* __restrict__ L) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < N) L[i] = u[i] >= tau ? (int)i : -1;
}

__global__ __launch_bounds__(256) void ccl_hook_kernel(Grid g, int64_t N, int* L, int* changed) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int r = L[i];
  if (r < 0) return;
  int ix, iy, iz;
  unflat(g, i, ix, iy, iz);
  const int64_t sy = g.n[0], sz = (int64_t)g.n[0] * g.n[1];
  int m = r;
  int v;
  if (ix > 0 && (v = L[i - 1]) >= 0) m = min(m, v);
  if (ix < g.n[0] - 1 && (v = L[i + 1]) >= 0) m = min(m, v);
  if (iy > 0 && (v = L[i - sy]) >= 0) m = min(m, v);
  if (iy < g.n[1] - 1 && (v = L[i + sy]) >= 0) m = min(m, v);
  if (iz > 0 && (v = L[i - sz]) >= 0) m = min(m, v);
  if (iz < g.n[2] - 1 && (v = L[i + sz]) >= 0) m = min(m, v);
  if (m < r) {
    atomicMin(&L[r], m);
    atomicMin(&L[i], m);
    *changed = 1;
  }
}

__global__ __launch_bounds__(256) void ccl_compress_kernel(int64_t N, int* L) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int l = L[i];
  if (l < 0) return;
  int r = l;
  for (int hop = 0; hop < 64; ++hop) {  // labels only decrease along the chain; the cap bounds the work
    const int rr = L[r];
    if (rr >= r) break;
    r = rr;
  }
  if (r < l) atomicMin(&L[i], r);
}

__global__ __launch_bounds__(256) void mark_boundary_kernel(Grid g, int64_t N, const int* __restrict__ L,
                                                            unsigned char* __restrict__ mark) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int l = L[i];
  if (l < 0) return;
  int ix, iy, iz;
  unflat(g, i, ix, iy, iz);
  if (ix == 0 || iy == 0 || iz == 0 || ix == g.n[0] - 1 || iy == g.n[1] - 1 || iz == g.n[2] - 1) mark[l] = 1;
}

__global__ __launch_bounds__(256) void outside_init_kernel(int64_t N, const int* __restrict__ L,
                                                           const unsigned char* __restrict__ mark,
                                                           unsigned char* __restrict__ O) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int l = L[i];
  O[i] = (l >= 0 && mark[l]) ? 1 : 0;
}

// bits[i] bit a: the edge from node i to its +a neighbour crosses the surface (tested only when one end is a
// band node: an edge between two far nodes cannot cross, tau > h/2)
__global__ __launch_bounds__(256) void edge_bits_kernel(Bvh h, Grid g, int64_t N, const float* __restrict__ u,
                                                        float tau, unsigned char* __restrict__ bits) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  int id[3];
  unflat(g, i, id[0], id[1], id[2]);
  const int n_nodes = n_nodes_of(h);
  const bool band_i = u[i] < tau;
  const int64_t stride[3] = {1, g.n[0], (int64_t)g.n[0] * g.n[1]};
  unsigned out = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (id[a] + 1 >= g.n[a]) continue;
    if (!band_i && !(u[i + stride[a]] < tau)) continue;
    const int b = a == 2 ? 0 : a + 1, c = a == 0 ? 2 : a - 1;
    if (edge_crosses(h, n_nodes, a, g.ax[a][id[a]], g.ax[a][id[a] + 1], g.ax[b][id[b]], g.ax[c][id[c]]))
      out |= 1u << a;
  }
  bits[i] = (unsigned char)out;
}

__global__ __launch_bounds__(256) void band_step_kernel(Grid g, int64_t N, const float* __restrict__ u, float tau,
                                                        const unsigned char* __restrict__ bits,
                                                        const unsigned char* __restrict__ O,
                                                        unsigned char* __restrict__ On) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  unsigned char o = O[i];
  if (!o && u[i] < tau) {
    int ix, iy, iz;
    unflat(g, i, ix, iy, iz);
    const int64_t sy = g.n[0], sz = (int64_t)g.n[0] * g.n[1];
    if ((ix > 0 && O[i - 1] && !(bits[i - 1] & 1)) || (ix < g.n[0] - 1 && O[i + 1] && !(bits[i] & 1)) ||
        (iy > 0 && O[i - sy] && !(bits[i - sy] & 2)) || (iy < g.n[1] - 1 && O[i + sy] && !(bits[i] & 2)) ||
        (iz > 0 && O[i - sz] && !(bits[i - sz] & 4)) || (iz < g.n[2] - 1 && O[i + sz] && !(bits[i] & 4)))
      o = 1;
  }
  On[i] = o;
}

__global__ __launch_bounds__(256) void sign_finish_kernel(int64_t N, const float* __restrict__ u,
                                                          const unsigned char* __restrict__ O, float offset,
                                                          float* __restrict__ sdf, unsigned char* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const float v = u[i];
  sdf[i] = (O[i] ? v : -v) - offset;
  if (out) out[i] = O[i];
}

Bvh bvh_view(const void* bvh, int64_t nf) {
  const char* b = static_cast<const char*>(bvh);
  return Bvh{reinterpret_cast<const float4*>(b + sizeof(BvhHeader)),
             reinterpret_cast<const float*>(b + bvh_tri_offset(nf)), (int)nf};
}

inline unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }

struct SignWs {
  int* L;
  unsigned char *mark, *O0, *O1, *bits;
  int* changed;
};

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

SignWs carve(void* ws, int64_t N) {
  char* p = static_cast<char*>(ws);
  SignWs w;
  w.L = reinterpret_cast<int*>(p);
  p += al256(4 * (size_t)N);
  w.mark = reinterpret_cast<unsigned char*>(p);
  p += al256(N);
  w.O0 = reinterpret_cast<unsigned char*>(p);
  p += al256(N);
  w.O1 = reinterpret_cast<unsigned char*>(p);
  p += al256(N);
  w.bits = reinterpret_cast<unsigned char*>(p);
  p += al256(N);
  w.changed = reinterpret_cast<int*>(p);
  return w;
}

}  // namespace

static size_t mesh_sign_ws_bytes(int64_t N) { return al256(4 * (size_t)N) + 4 * al256(N) + 256; }

static hipError_t mesh_udf_points_launch(const void* bvh, int64_t nf, const float* pts, int64_t n, int brute,
                                         float* dist, hipStream_t st) {
  udf_points_kernel<<<blocks256(n), 256, 0, st>>>(bvh_view(bvh, nf), pts, n, brute, dist);
  return hipGetLastError();
}

static hipError_t mesh_udf_grid_launch(const void* bvh, int64_t nf, const float* xs, const float* ys, const float* zs,
                                       int nx, int ny, int nz, int brute, float* dist, hipStream_t st) {
  const int64_t bricks = (int64_t)((nx + 3) >> 2) * ((ny + 3) >> 2) * ((nz + 3) >> 2);
  udf_grid_kernel<<<(unsigned)bricks, 64, 0, st>>>(bvh_view(bvh, nf), xs, ys, zs, nx, ny, nz, brute, dist);
  return hipGetLastError();
}

// 0, a hipError_t, or DISN_E_CONVERGE; synchronises `st` once per labelling round
static int mesh_sign_launch(const void* bvh, int64_t nf, const float* xs, const float* ys, const float* zs, int nx,
                            int ny, int nz, const float* u, float tau, int steps, float offset, float* sdf,
                            unsigned char* outside, void* ws, hipStream_t st) {
  const Bvh h = bvh_view(bvh, nf);
  const Grid g{{xs, ys, zs}, {nx, ny, nz}};
  const int64_t N = (int64_t)nx * ny * nz;
  const unsigned nb = blocks256(N);
  SignWs w = carve(ws, N);
  hipError_t e;
  far_init_kernel<<<nb, 256, 0, st>>>(u, N, tau, w.L);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  bool converged = false;
  for (int it = 0; it < kCclMaxIter && !converged; ++it) {
    if ((e = hipMemsetAsync(w.changed, 0, sizeof(int), st)) != hipSuccess) return (int)e;
    ccl_hook_kernel<<<nb, 256, 0, st>>>(g, N, w.L, w.changed);
    ccl_compress_kernel<<<nb, 256, 0, st>>>(N, w.L);
    int changed = 1;
    if ((e = hipMemcpyAsync(&changed, w.changed, sizeof(int), hipMemcpyDeviceToHost, st)) != hipSuccess) return (int)e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return (int)e;
    converged = changed == 0;
  }
  if (!converged) return DISN_E_CONVERGE;
  if ((e = hipMemsetAsync(w.mark, 0, (size_t)N, st)) != hipSuccess) return (int)e;
  mark_boundary_kernel<<<nb, 256, 0, st>>>(g, N, w.L, w.mark);
  outside_init_kernel<<<nb, 256, 0, st>>>(N, w.L, w.mark, w.O0);
  edge_bits_kernel<<<nb, 256, 0, st>>>(h, g, N, u, tau, w.bits);
  unsigned char *cur = w.O0, *nxt = w.O1;
  for (int s = 0; s < steps; ++s) {
    band_step_kernel<<<nb, 256, 0, st>>>(g, N, u, tau, w.bits, cur, nxt);
    unsigned char* t = cur;
    cur = nxt;
    nxt = t;
  }
  sign_finish_kernel<<<nb, 256, 0, st>>>(N, u, cur, offset, sdf, outside);
  return (int)hipGetLastError();
}

}  // namespace disn

// ---- the C entries of include/disn_amd.h: argument and workspace checks, then the launchers above ----
using namespace disn;

#define DISN_TRY(expr)                    \
  do {                                    \
    hipError_t _e = (expr);               \
    if (_e != hipSuccess) return (int)_e; \
  } while (0)

extern "C" {

static int mesh_grid_shape(int nx, int ny, int nz) {
  if (nx < 2 || ny < 2 || nz < 2) return DISN_E_ARG;
  if (!disn::fits_int(nx, ny, nz)) return DISN_E_SHAPE;  // int32 component labels
  return 0;
}

int disn_mesh_udf_points(const void* bvh, int64_t nf, const float* points, int64_t n, int brute, float* dist,
                         void* stream) {
  if (!bvh || !points || !dist || nf < 1 || n < 1) return DISN_E_ARG;
  if (nf > kBvhMaxTris || n > (int64_t)UINT32_MAX * 256) return DISN_E_SHAPE;
  DISN_TRY(mesh_udf_points_launch(bvh, nf, points, n, brute, dist, (hipStream_t)stream));
  return 0;
}

int disn_mesh_udf_grid(const void* bvh, int64_t nf, const float* xs, const float* ys, const float* zs, int nx, int ny,
                       int nz, int brute, float* dist, void* stream) {
  if (!bvh || !xs || !ys || !zs || !dist || nf < 1) return DISN_E_ARG;
  if (int rc = mesh_grid_shape(nx, ny, nz)) return rc;
  if (nf > kBvhMaxTris) return DISN_E_SHAPE;
  DISN_TRY(mesh_udf_grid_launch(bvh, nf, xs, ys, zs, nx, ny, nz, brute, dist, (hipStream_t)stream));
  return 0;
}

size_t disn_mesh_sign_workspace_bytes(int nx, int ny, int nz) {
  return mesh_grid_shape(nx, ny, nz) ? 0 : mesh_sign_ws_bytes((int64_t)nx * ny * nz);
}

int disn_mesh_sign(const void* bvh, int64_t nf, const float* xs, const float* ys, const float* zs, int nx, int ny,
                   int nz, const float* u, float tau, int steps, float offset, float* sdf, uint8_t* outside, void* ws,
                   size_t ws_bytes, void* stream) {
  if (!bvh || !xs || !ys || !zs || !u || !sdf || !ws || nf < 1 || steps < 0) return DISN_E_ARG;
  if (!(tau > 0.0f) || !(offset == offset)) return DISN_E_ARG;
  if (int rc = mesh_grid_shape(nx, ny, nz)) return rc;
  if (nf > kBvhMaxTris) return DISN_E_SHAPE;
  if (ws_bytes < mesh_sign_ws_bytes((int64_t)nx * ny * nz)) return DISN_E_WS;
  return mesh_sign_launch(bvh, nf, xs, ys, zs, nx, ny, nz, u, tau, steps, offset, sdf, outside, ws,
                          (hipStream_t)stream);
}

}  // extern "C"

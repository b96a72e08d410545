// View rendering for preprocessing (the Blender renders behind preprocessing/create_img_h5.py of the reference,
// replaced by a ray caster): V pinhole views of one triangle soup in one launch, over the BVH of mesh_host.cpp.
// THIS FILE IS COMPILED WITH -ffp-contract=off: every expression below is restated operation for operation in
// tests/render_reference.py and the results are compared bit for bit.
//
// Ray of image point (x, y) of view v: org + t * dir, dir = (d0 + x*dx) + y*dy per component, so that t is the
// camera-space depth.  Pixel (row i, col j), sample (sy, sx) of an S x S grid: x = j + (sx + 0.5)/S,
// y = i + (sy + 0.5)/S.
// Hit test: Moeller-Trumbore in fp32, two-sided.  e1 = b - a, e2 = c - a, p = dir x e2, det = e1.p (skipped when
// 0), tv = org - a, u = (tv.p)/det, q = tv x e1, v = (dir.q)/det, t = (e2.q)/det; a hit when u >= 0, v >= 0,
// u + v <= 1, t > 0.  dot(a, b) = (ax*bx + ay*by) + az*bz, cross = (ay*bz - az*by, az*bx - ax*bz, ax*by - ay*bx).
// The nearest hit wins; equal t goes to the lowest file-order face (order[slot]; the slot itself without `order`).
// Shading: n = e1 x e2 of the hit face, c = min(|n.dir| / (sqrt(n.n) * sqrt(dir.dir)), 1) (0 when the
// denominator is 0), shade = ambient + (1 - ambient) * c, colour = shade * albedo[face] (0.8 without albedo).
// Pixel: colour sums over the hit samples in (sy, sx) order, byte = floor(sum / hits * 255 + 0.5) capped at 255,
// alpha = floor(255 * hits / S^2 + 0.5); depth / face: the first sample with the smallest t.
//
// Traversal: the stackless walk of mesh_sdf.hip (pre-order nodes + escape links, two 16-byte loads per node).
// One 64-lane workgroup renders an 8 x 8 pixel tile and walks sample after sample, so the 64 rays of a wave are
// neighbours and take nearly the same path.  A node is skipped by a padded slab test: the box grows
// by pad = 2^-18 * max|org|, an axis with |dir| < 2^-100 is a containment test (no 0 * inf), the others use
// fminf / fmaxf (which drop a NaN operand), and the interval [tn, min(tf, best)] is widened by 2^-16 relative
// at both ends before it is called empty.
#include "../../include/disn_amd.h"
#include "kernels.hpp"
#include "mesh_bvh.hpp"

namespace disn {

namespace {

struct V3 {
  float x, y, z;
};
__device__ __forceinline__ V3 ld3(const float* p) { return V3{p[0], p[1], p[2]}; }
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) {
  return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

struct Scene {
  const float4* nodes;  // 2 per node: (lo.xyz, escape bits), (hi.xyz, leaf bits)
  const float* tris;    // 9 floats per slot, leaf order
  const int32_t* order; // slot -> file-order face, or NULL
  int n_tris;
};

__device__ __forceinline__ int n_nodes_of(const Scene& s) {
  return reinterpret_cast<const BvhHeader*>(reinterpret_cast<const char*>(s.nodes) - sizeof(BvhHeader))->n_nodes;
}

struct Hit {
  float t;
  int face, slot;
};

__device__ __forceinline__ void try_slot(const Scene& s, int slot, V3 org, V3 dir, Hit& best) {
  const float* tp = s.tris + 9 * (size_t)slot;
  const V3 a = ld3(tp);
  const V3 e1 = sub(ld3(tp + 3), a), e2 = sub(ld3(tp + 6), a);
  const V3 p = cross(dir, e2);
  const float det = dot(e1, p);
  if (det == 0.0f) return;
  const V3 tv = sub(org, a);
  const float u = dot(tv, p) / det;
  const V3 q = cross(tv, e1);
  const float v = dot(dir, q) / det;
  const float t = dot(e2, q) / det;
  if (!(u >= 0.0f && v >= 0.0f && u + v <= 1.0f && t > 0.0f)) return;
  if (t > best.t) return;
  const int face = s.order ? s.order[slot] : slot;
  if (t < best.t || face < best.face) best = Hit{t, face, slot};
}

struct Slab {
  V3 org, inv;
  float pad;
  bool px, py, pz;  // the axis is (numerically) parallel to the ray: containment test
};

__device__ __forceinline__ void slab_axis(float lo, float hi, float o, float inv, bool par, float pad, float& tn,
                                          float& tf, bool& miss) {
  const float l = (lo - pad) - o, h = (hi + pad) - o;
  if (par) {
    miss = miss || l > 0.0f || h < 0.0f;
  } else {
    const float t1 = l * inv, t2 = h * inv;
    tn = fmaxf(tn, fminf(t1, t2));
    tf = fminf(tf, fmaxf(t1, t2));
  }
}

__device__ __forceinline__ bool slab_miss(const Slab& r, float4 lo, float4 hi, float best) {
  float tn = 0.0f, tf = best;
  bool miss = false;
  slab_axis(lo.x, hi.x, r.org.x, r.inv.x, r.px, r.pad, tn, tf, miss);
  slab_axis(lo.y, hi.y, r.org.y, r.inv.y, r.py, r.pad, tn, tf, miss);
  slab_axis(lo.z, hi.z, r.org.z, r.inv.z, r.pz, r.pad, tn, tf, miss);
  return miss || tn * (1.0f - 0x1p-16f) > tf * (1.0f + 0x1p-16f);
}

__device__ Hit trace(const Scene& s, V3 org, V3 dir, int brute) {
  Hit best{INFINITY, 0x7fffffff, -1};
  if (brute) {
    for (int slot = 0; slot < s.n_tris; ++slot) try_slot(s, slot, org, dir, best);
    return best;
  }
  Slab r;
  r.org = org;
  r.px = fabsf(dir.x) < 0x1p-100f;
  r.py = fabsf(dir.y) < 0x1p-100f;
  r.pz = fabsf(dir.z) < 0x1p-100f;
  r.inv = V3{r.px ? 0.0f : 1.0f / dir.x, r.py ? 0.0f : 1.0f / dir.y, r.pz ? 0.0f : 1.0f / dir.z};
  r.pad = 0x1p-18f * fmaxf(fmaxf(fabsf(org.x), fabsf(org.y)), fabsf(org.z));
  const int n = n_nodes_of(s);
  int i = 0;
  while (i < n) {
    const float4 lo = s.nodes[2 * i], hi = s.nodes[2 * i + 1];
    const int escape = __float_as_int(lo.w), leaf = __float_as_int(hi.w);
    if (slab_miss(r, lo, hi, best.t)) {
      i = escape;
    } else if (leaf) {
      const int first = leaf >> 3, cnt = leaf & 7;
      for (int k = 0; k < cnt; ++k) try_slot(s, first + k, org, dir, best);
      i = escape;
    } else {
      ++i;
    }
  }
  return best;
}

// one workgroup (one wave) per 8 x 8 pixel tile of one view; lane = lx + 8*ly
__global__ __launch_bounds__(64) void render_views_kernel(Scene s, const float* __restrict__ albedo,
                                                          const float* __restrict__ cams, int H, int W, int S,
                                                          float ambient, int brute, uint32_t* __restrict__ rgba,
                                                          float* __restrict__ depth, int32_t* __restrict__ face) {
  const int j = 8 * (int)blockIdx.x + (int)(threadIdx.x & 7), i = 8 * (int)blockIdx.y + (int)(threadIdx.x >> 3);
  if (i >= H || j >= W) return;
  const int v = (int)blockIdx.z;
  const float* cam = cams + 12 * (size_t)v;
  const V3 org = ld3(cam), d0 = ld3(cam + 3), dx = ld3(cam + 6), dy = ld3(cam + 9);
  const float fs = (float)S;
  float sum_r = 0.0f, sum_g = 0.0f, sum_b = 0.0f, best_t = INFINITY;
  int hits = 0, best_face = -1;
  for (int sy = 0; sy < S; ++sy) {
    const float y = (float)i + ((float)sy + 0.5f) / fs;
    for (int sx = 0; sx < S; ++sx) {
      const float x = (float)j + ((float)sx + 0.5f) / fs;
      const V3 dir{(d0.x + x * dx.x) + y * dy.x, (d0.y + x * dx.y) + y * dy.y, (d0.z + x * dx.z) + y * dy.z};
      const Hit h = trace(s, org, dir, brute);
      if (h.slot < 0) continue;
      const float* tp = s.tris + 9 * (size_t)h.slot;
      const V3 a = ld3(tp);
      const V3 n = cross(sub(ld3(tp + 3), a), sub(ld3(tp + 6), a));
      const float den = sqrtf(dot(n, n)) * sqrtf(dot(dir, dir));
      const float c = den > 0.0f ? fminf(fabsf(dot(n, dir)) / den, 1.0f) : 0.0f;
      const float shade = ambient + (1.0f - ambient) * c;
      float ar = 0.8f, ag = 0.8f, ab = 0.8f;
      if (albedo) {
        const float* al = albedo + 3 * (size_t)h.face;
        ar = al[0], ag = al[1], ab = al[2];
      }
      sum_r += shade * ar;
      sum_g += shade * ag;
      sum_b += shade * ab;
      ++hits;
      if (h.t < best_t) {
        best_t = h.t;
        best_face = h.face;
      }
    }
  }
  const size_t pix = ((size_t)v * H + i) * W + j;
  uint32_t out = 0;
  if (hits) {
    const float n = (float)hits;
    const uint32_t r = (uint32_t)fminf(floorf(sum_r / n * 255.0f + 0.5f), 255.0f);
    const uint32_t g = (uint32_t)fminf(floorf(sum_g / n * 255.0f + 0.5f), 255.0f);
    const uint32_t b = (uint32_t)fminf(floorf(sum_b / n * 255.0f + 0.5f), 255.0f);
    const uint32_t al = (uint32_t)floorf(255.0f * n / (fs * fs) + 0.5f);
    out = r | (g << 8) | (b << 16) | (al << 24);
  }
  rgba[pix] = out;
  if (depth) depth[pix] = hits ? best_t : 0.0f;
  if (face) face[pix] = best_face;
}

}  // namespace

static hipError_t render_views_launch(const void* bvh, int64_t nf, const int32_t* order, const float* albedo,
                                      const float* cams, int V, int H, int W, int S, float ambient, int brute,
                                      uint8_t* rgba, float* depth, int32_t* face, hipStream_t st) {
  const char* b = static_cast<const char*>(bvh);
  Scene s;
  s.nodes = reinterpret_cast<const float4*>(b + sizeof(BvhHeader));
  s.tris = reinterpret_cast<const float*>(b + bvh_tri_offset(nf));
  s.order = order;
  s.n_tris = (int)nf;
  const dim3 grid((unsigned)((W + 7) / 8), (unsigned)((H + 7) / 8), (unsigned)V);
  render_views_kernel<<<grid, 64, 0, st>>>(s, albedo, cams, H, W, S, ambient, brute,
                                           reinterpret_cast<uint32_t*>(rgba), depth, face);
  return hipGetLastError();
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

int disn_render_views(const void* bvh, int64_t nf, const int32_t* order, const float* albedo, const float* cams,
                      int V, int H, int W, int S, float ambient, int brute, uint8_t* rgba, float* depth,
                      int32_t* face, void* stream) {
  if (!bvh || !cams || !rgba || nf < 1 || V < 1 || H < 1 || W < 1 || S < 1) return DISN_E_ARG;
  if (!(ambient >= 0.0f && ambient <= 1.0f)) return DISN_E_ARG;
  if (!order && (albedo || face)) return DISN_E_ARG;
  if (nf > kBvhMaxTris || S > 4 || H > 1024 || W > 1024 || V > 65535) return DISN_E_SHAPE;
  DISN_TRY(render_views_launch(bvh, nf, order, albedo, cams, V, H, W, S, ambient, brute, rgba, depth, face,
                               (hipStream_t)stream));
  return 0;
}

}  // extern "C"

// Sphere tracing of an implicit field: for V pinhole views, the first point of every pixel's ray where
// value - iso changes sign, without a grid and without a mesh.  The field itself is NOT evaluated here: the kernels
// keep a per-ray state machine, hand the caller the compacted list of points to evaluate, and take the values back.
//
//   setup    ray = org + t * dir, dir = (d0 + x*dx) + y*dy, x = j + 0.5, y = i + 0.5 (render.hip's, one sample);
//            [t0, t1] = the slab interval of the box clipped to t >= t_min; empty -> MISS, else MARCH at t = t0
//   advance  f = value / sdf_weight - iso of the k-th listed ray (inside is negative):
//              |f| <= eps                      HIT, status 1, at t
//              MARCH, f < 0, no positive yet   HIT, status 2 (the box clips the shape / the camera is inside)
//              MARCH, f < 0                    BRACKET [t_lo, t]
//              MARCH, otherwise                (t_lo, f_lo) = (t, f); t >= t1: MISS, status 0; max_steps march
//                                              evaluations used: MISS, status 4; else
//                                              t = min(t + clamp(step_scale * f, min_step, max_step) / len, t1)
//              BRACKET                         the end with f's sign is replaced; `refine` bracket evaluations used:
//                                              HIT, status 3, at t
//              the next sample of a bracket    t_lo + (w * f_lo) / (f_lo - f_hi), w = t_hi - t_lo, clamped to
//                                              [t_lo + 0.05 w, t_hi - 0.05 w]
//   collect  the compacted list of the HIT rays (status 1..3), their points, and every ray's slot in that list
//   shade    depth, normal, residual, status and rgba of every pixel from pred / grad at the hits
//
// THIS FILE IS COMPILED WITH -ffp-contract=off: tests/sdf_trace_reference.py restates every expression in float32
// and the state, the points and the outputs are compared bit for bit.  dot(a, b) = (ax*bx + ay*by) + az*bz.
//
// Compaction: one wave-wide ballot and one atomic per wave claim a range of the output list; the ORDER of a list is
// therefore unspecified, and nothing a ray computes reads another ray's state or its own position in a list.
//
// State (caller-owned, disn_trace_state_bytes): 4-byte words, field f of ray r at word f * n4 + r with n4 = n rounded
// up to a multiple of 64; include/disn_amd.h names the fields.
#include "../../include/disn_amd.h"
#include "kernels.hpp"

namespace disn {

namespace {

enum : int {
  F_T = DISN_TRACE_T, F_T1 = DISN_TRACE_T1, F_LEN = DISN_TRACE_LEN, F_TLO = DISN_TRACE_T_LO, F_FLO = DISN_TRACE_F_LO,
  F_THI = DISN_TRACE_T_HI, F_FHI = DISN_TRACE_F_HI, F_PHASE = DISN_TRACE_PHASE, F_STATUS = DISN_TRACE_STATUS,
  F_MARCH = DISN_TRACE_MARCH_EVALS, F_BRACKET = DISN_TRACE_BRACKET_EVALS, F_HAVE_LO = DISN_TRACE_HAVE_LO,
  F_SLOT = DISN_TRACE_HIT_SLOT, F_LIST = DISN_TRACE_FIELDS, F_COUNT = DISN_TRACE_FIELDS + 3
};
enum : int { PH_MARCH = 0, PH_BRACKET = 1, PH_DONE = 2 };

struct V3 {
  float x, y, z;
};
__device__ __forceinline__ V3 ld3(const float* p) { return V3{p[0], p[1], p[2]}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

struct Rays {
  const float* cams;
  unsigned H, W;
  size_t n;
};

struct State {
  float* f;
  int* i;
  size_t n4;
  __device__ __forceinline__ float& F(int field, size_t r) const { return f[(size_t)field * n4 + r]; }
  __device__ __forceinline__ int& I(int field, size_t r) const { return i[(size_t)field * n4 + r]; }
  __device__ __forceinline__ int* list(int l) const { return i + (size_t)(F_LIST + l) * n4; }
  __device__ __forceinline__ unsigned* count(int l) const {
    return reinterpret_cast<unsigned*>(i) + (size_t)F_COUNT * n4 + l;
  }
};

__device__ __forceinline__ void ray_of(const Rays& g, size_t r, V3& org, V3& dir) {
  const size_t hw = (size_t)g.H * g.W;
  const size_t v = r / hw;
  const unsigned rem = (unsigned)(r % hw), i = rem / g.W, j = rem % g.W;
  const float* cam = g.cams + 12 * v;
  org = ld3(cam);
  const V3 d0 = ld3(cam + 3), dx = ld3(cam + 6), dy = ld3(cam + 9);
  const float x = (float)j + 0.5f, y = (float)i + 0.5f;
  dir = V3{(d0.x + x * dx.x) + y * dy.x, (d0.y + x * dx.y) + y * dy.y, (d0.z + x * dx.z) + y * dy.z};
}

__device__ __forceinline__ void point_at(V3 org, V3 dir, float t, float* p) {
  p[0] = org.x + t * dir.x;
  p[1] = org.y + t * dir.y;
  p[2] = org.z + t * dir.z;
}

// position of this lane's entry in the output list (valid where `keep`); every lane of the wave must call it
__device__ __forceinline__ unsigned claim(bool keep, unsigned* count) {
  const unsigned long long b = __ballot(keep);
  const unsigned lane = __lane_id();
  unsigned base = 0;
  if (lane == 0 && b) base = atomicAdd(count, (unsigned)__popcll(b));
  base = __shfl(base, 0);
  return base + (unsigned)__popcll(b & ((1ull << lane) - 1ull));
}

__device__ __forceinline__ void slab_axis(float lo, float hi, float o, float d, float& tn, float& tf, bool& miss) {
  const float l = lo - o, h = hi - o;
  if (fabsf(d) < 0x1p-100f) {
    miss = miss || l > 0.0f || h < 0.0f;
  } else {
    const float inv = 1.0f / d;
    const float a = l * inv, b = h * inv;
    tn = fmaxf(tn, fminf(a, b));
    tf = fminf(tf, fmaxf(a, b));
  }
}

struct Box {
  float lo[3], hi[3];
};

__global__ __launch_bounds__(256) void trace_setup_kernel(Rays g, State s, Box box, float t_min,
                                                          float* __restrict__ pts) {
  const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
  bool keep = false;
  V3 org{0, 0, 0}, dir{0, 0, 0};
  float t0 = 0.0f;
  if (r < g.n) {
    ray_of(g, r, org, dir);
    const float len = sqrtf(dot(dir, dir));
    float tn = t_min, tf = INFINITY;
    bool miss = false;
    slab_axis(box.lo[0], box.hi[0], org.x, dir.x, tn, tf, miss);
    slab_axis(box.lo[1], box.hi[1], org.y, dir.y, tn, tf, miss);
    slab_axis(box.lo[2], box.hi[2], org.z, dir.z, tn, tf, miss);
    // tf stays infinite only when every axis is parallel (dir = 0): no ray; !(tn <= tf) also catches a NaN camera
    keep = !miss && tn <= tf && tf < INFINITY && len > 0.0f;
    t0 = tn;
    s.F(F_T, r) = keep ? tn : 0.0f;
    s.F(F_T1, r) = keep ? tf : 0.0f;
    s.F(F_LEN, r) = len;
    s.F(F_TLO, r) = 0.0f;
    s.F(F_FLO, r) = 0.0f;
    s.F(F_THI, r) = 0.0f;
    s.F(F_FHI, r) = 0.0f;
    s.I(F_PHASE, r) = keep ? PH_MARCH : PH_DONE;
    s.I(F_STATUS, r) = 0;
    s.I(F_MARCH, r) = 0;
    s.I(F_BRACKET, r) = 0;
    s.I(F_HAVE_LO, r) = 0;
    s.I(F_SLOT, r) = -1;
  }
  const unsigned pos = claim(keep, s.count(0));
  if (keep) {
    s.list(0)[pos] = (int)r;
    point_at(org, dir, t0, pts + 3 * (size_t)pos);
  }
}

struct March {
  float sdf_weight, iso, eps, step_scale, min_step, max_step;
  int max_steps, refine;
};

__device__ __forceinline__ float false_position(float t_lo, float f_lo, float t_hi, float f_hi) {
  const float w = t_hi - t_lo;
  const float den = f_lo - f_hi;
  const float num = w * f_lo;
  const float q = num / den;
  const float m = 0.05f * w;
  const float a = t_lo + m, b = t_hi - m;
  return fminf(fmaxf(t_lo + q, a), b);
}

__global__ __launch_bounds__(256) void trace_advance_kernel(Rays g, State s, March m, const float* __restrict__ values,
                                                            size_t n_active, int in, float* __restrict__ pts) {
  const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
  bool keep = false;
  size_t r = 0;
  float t = 0.0f;
  if (k < n_active) r = (size_t)(unsigned)s.list(in)[k];
  if (k < n_active && r < g.n) {   // (an index outside the image: a list this file did not write; skipped)
    const float f = values[k] / m.sdf_weight - m.iso;
    t = s.F(F_T, r);
    const int phase = s.I(F_PHASE, r);
    int status = 0;
    bool done = false;
    if (fabsf(f) <= m.eps) {
      status = 1;
      done = true;
    } else if (phase == PH_MARCH) {
      const int ms = s.I(F_MARCH, r) + 1;
      s.I(F_MARCH, r) = ms;
      if (f < 0.0f) {
        if (!s.I(F_HAVE_LO, r)) {
          status = 2;
          done = true;
        } else {
          s.F(F_THI, r) = t;
          s.F(F_FHI, r) = f;
          s.I(F_PHASE, r) = PH_BRACKET;
          t = false_position(s.F(F_TLO, r), s.F(F_FLO, r), t, f);
        }
      } else {
        s.F(F_TLO, r) = t;
        s.F(F_FLO, r) = f;
        s.I(F_HAVE_LO, r) = 1;
        const float t1 = s.F(F_T1, r);
        if (t >= t1) {
          status = 0;
          done = true;
        } else if (ms >= m.max_steps) {
          status = 4;
          done = true;
        } else {
          const float st = fminf(fmaxf(m.step_scale * f, m.min_step), m.max_step);
          t = fminf(t + st / s.F(F_LEN, r), t1);
        }
      }
    } else if (phase == PH_BRACKET) {
      const int bs = s.I(F_BRACKET, r) + 1;
      s.I(F_BRACKET, r) = bs;
      if (f < 0.0f) {
        s.F(F_THI, r) = t;
        s.F(F_FHI, r) = f;
      } else {
        s.F(F_TLO, r) = t;
        s.F(F_FLO, r) = f;
      }
      if (bs >= m.refine) {
        status = 3;
        done = true;
      } else {
        t = false_position(s.F(F_TLO, r), s.F(F_FLO, r), s.F(F_THI, r), s.F(F_FHI, r));
      }
    } else {
      done = true;   // a finished ray in the list (a caller's list): left as it is
      status = s.I(F_STATUS, r);
    }
    if (done) {
      s.I(F_PHASE, r) = PH_DONE;
      s.I(F_STATUS, r) = status;
    } else {
      s.F(F_T, r) = t;
      keep = true;
    }
  }
  const unsigned pos = claim(keep, s.count(1 - in));
  if (keep) {
    V3 org, dir;
    ray_of(g, r, org, dir);
    s.list(1 - in)[pos] = (int)r;
    point_at(org, dir, t, pts + 3 * (size_t)pos);
  }
}

__global__ __launch_bounds__(256) void trace_collect_kernel(Rays g, State s, float* __restrict__ pts) {
  const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
  bool keep = false;
  if (r < g.n) {
    const int st = s.I(F_STATUS, r);
    keep = s.I(F_PHASE, r) == PH_DONE && st >= 1 && st <= 3;
  }
  const unsigned pos = claim(keep, s.count(2));
  if (r < g.n) s.I(F_SLOT, r) = keep ? (int)pos : -1;
  if (keep) {
    V3 org, dir;
    ray_of(g, r, org, dir);
    s.list(2)[pos] = (int)r;
    point_at(org, dir, s.F(F_T, r), pts + 3 * (size_t)pos);
  }
}

__global__ __launch_bounds__(256) void trace_shade_kernel(Rays g, State s, const float* __restrict__ pred,
                                                          const float* __restrict__ grad, size_t n_hits,
                                                          float sdf_weight, float iso, float ambient,
                                                          float* __restrict__ depth, float* __restrict__ normal,
                                                          float* __restrict__ residual, uint8_t* __restrict__ status,
                                                          uint32_t* __restrict__ rgba) {
  const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= g.n) return;
  const int slot = s.I(F_SLOT, r);
  const bool hit = slot >= 0 && (size_t)slot < n_hits;
  float d = 0.0f, res = 0.0f;
  V3 nrm{0.0f, 0.0f, 0.0f};
  uint32_t px = 0;
  if (hit) {
    V3 org, dir;
    ray_of(g, r, org, dir);
    d = s.F(F_T, r);
    res = fabsf(pred[slot] / sdf_weight - iso);
    const V3 gr = ld3(grad + 3 * (size_t)slot);
    const float g2 = dot(gr, gr);
    const float gl = sqrtf(g2);
    if (!(g2 < 1e-12f)) nrm = V3{gr.x / gl, gr.y / gl, gr.z / gl};
    const float den = gl * sqrtf(dot(dir, dir));
    const float c = den > 0.0f ? fminf(fabsf(dot(gr, dir)) / den, 1.0f) : 0.0f;
    const float shade = ambient + (1.0f - ambient) * c;
    const uint32_t b = (uint32_t)fminf(floorf(shade * 0.8f * 255.0f + 0.5f), 255.0f);
    px = b | (b << 8) | (b << 16) | (255u << 24);
  }
  if (depth) depth[r] = d;
  if (normal) {
    normal[3 * r + 0] = nrm.x;
    normal[3 * r + 1] = nrm.y;
    normal[3 * r + 2] = nrm.z;
  }
  if (residual) residual[r] = res;
  if (status) status[r] = (uint8_t)s.I(F_STATUS, r);
  if (rgba) rgba[r] = px;
}

inline size_t pad64(size_t n) { return (n + 63) & ~size_t(63); }

inline State state_of(void* state, size_t n) {
  return State{static_cast<float*>(state), static_cast<int*>(state), pad64(n)};
}

inline Rays rays_of(const float* cams, int V, int H, int W) {
  const size_t n = (size_t)V * H * W;
  return Rays{cams, (unsigned)H, (unsigned)W, n};
}

inline unsigned blocks_of(size_t n) { return (unsigned)((n + 255) / 256); }

hipError_t clear_count(const State& s, int l, hipStream_t st) {
  return hipMemsetAsync(reinterpret_cast<unsigned*>(s.i) + (size_t)F_COUNT * s.n4 + l, 0, sizeof(unsigned), st);
}

}  // namespace

// The state machine, the lists and the counts live in the caller's state (trace_state_bytes); `pts` takes one point per
// listed ray (room for every ray at setup and collect, for n_active at advance); list `in` (0 / 1) is read, the other
// one written; the sizes are the caller's to check (the entries below)
struct TraceMarch {
  float sdf_weight, iso, eps, step_scale, min_step, max_step;
  int max_steps, refine;
};

static size_t trace_state_bytes(size_t n_rays) { return ((size_t)(DISN_TRACE_FIELDS + 3) * pad64(n_rays) + 64) * 4; }

static hipError_t trace_setup_launch(const float* cams, int V, int H, int W, const float box[6], float t_min,
                                     void* state, float* pts, hipStream_t st) {
  const Rays g = rays_of(cams, V, H, W);
  const State s = state_of(state, g.n);
  Box b;
  for (int a = 0; a < 3; ++a) b.lo[a] = box[a], b.hi[a] = box[a + 3];
  hipError_t e = hipMemsetAsync(reinterpret_cast<unsigned*>(s.i) + (size_t)F_COUNT * s.n4, 0, 64 * sizeof(unsigned), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(trace_setup_kernel, dim3(blocks_of(g.n)), dim3(256), 0, st, g, s, b, t_min, pts);
  return hipGetLastError();
}

static hipError_t trace_advance_launch(const float* cams, int V, int H, int W, const float* values, size_t n_active,
                                       int in, const TraceMarch& p, void* state, float* pts, hipStream_t st) {
  const Rays g = rays_of(cams, V, H, W);
  const State s = state_of(state, g.n);
  hipError_t e = clear_count(s, 1 - in, st);
  if (e != hipSuccess) return e;
  const March m{p.sdf_weight, p.iso, p.eps, p.step_scale, p.min_step, p.max_step, p.max_steps, p.refine};
  hipLaunchKernelGGL(trace_advance_kernel, dim3(blocks_of(n_active)), dim3(256), 0, st, g, s, m, values, n_active, in,
                     pts);
  return hipGetLastError();
}

static hipError_t trace_collect_launch(const float* cams, int V, int H, int W, void* state, float* pts,
                                       hipStream_t st) {
  const Rays g = rays_of(cams, V, H, W);
  const State s = state_of(state, g.n);
  hipError_t e = clear_count(s, 2, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(trace_collect_kernel, dim3(blocks_of(g.n)), dim3(256), 0, st, g, s, pts);
  return hipGetLastError();
}

static hipError_t trace_shade_launch(const float* cams, int V, int H, int W, const void* state, const float* pred,
                                     const float* grad, size_t n_hits, float sdf_weight, float iso, float ambient,
                                     float* depth, float* normal, float* residual, uint8_t* status, uint8_t* rgba,
                                     hipStream_t st) {
  const Rays g = rays_of(cams, V, H, W);
  const State s = state_of(const_cast<void*>(state), g.n);
  hipLaunchKernelGGL(trace_shade_kernel, dim3(blocks_of(g.n)), dim3(256), 0, st, g, s, pred, grad, n_hits, sdf_weight,
                     iso, ambient, depth, normal, residual, status, reinterpret_cast<uint32_t*>(rgba));
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

namespace {
constexpr int64_t kTraceMaxRays = int64_t(1) << 27;
int64_t trace_rays(int V, int H, int W) {   // 0: not a shape this takes
  if (V < 1 || H < 1 || W < 1 || H > 8192 || W > 8192) return 0;
  const int64_t n = (int64_t)V * H * W;
  return n <= kTraceMaxRays ? n : 0;
}
}  // namespace

size_t disn_trace_state_bytes(int64_t n_rays) {
  return n_rays >= 1 && n_rays <= kTraceMaxRays ? trace_state_bytes((size_t)n_rays) : 0;
}

int disn_trace_setup(const float* cams, int V, int H, int W, const double* sdf_params_host, float t_min, void* state,
                     size_t state_bytes, float* pts, void* stream) {
  const int64_t n = trace_rays(V, H, W);
  if (!cams || !sdf_params_host || !state || !pts || !n || !(t_min >= 0.0f)) return DISN_E_ARG;
  if (state_bytes < trace_state_bytes((size_t)n)) return DISN_E_WS;
  float box[6];
  for (int a = 0; a < 6; ++a) box[a] = (float)sdf_params_host[a];
  for (int a = 0; a < 3; ++a)
    if (!(box[a] <= box[a + 3])) return DISN_E_ARG;
  DISN_TRY(trace_setup_launch(cams, V, H, W, box, t_min, state, pts, (hipStream_t)stream));
  return 0;
}

int disn_trace_advance(const float* cams, int V, int H, int W, const float* values, int64_t n_active, int list_in,
                       float sdf_weight, float iso, float eps, float step_scale, float min_step, float max_step,
                       int max_steps, int refine, void* state, size_t state_bytes, float* pts, void* stream) {
  const int64_t n = trace_rays(V, H, W);
  if (!cams || !values || !state || !pts || !n || n_active < 1 || n_active > n || (list_in != 0 && list_in != 1))
    return DISN_E_ARG;
  if (sdf_weight == 0.0f || !(eps >= 0.0f) || !(step_scale > 0.0f) || !(min_step > 0.0f) || !(max_step >= min_step) ||
      max_steps < 1 || refine < 1)
    return DISN_E_ARG;
  if (state_bytes < trace_state_bytes((size_t)n)) return DISN_E_WS;
  const TraceMarch p{sdf_weight, iso, eps, step_scale, min_step, max_step, max_steps, refine};
  DISN_TRY(trace_advance_launch(cams, V, H, W, values, (size_t)n_active, list_in, p, state, pts, (hipStream_t)stream));
  return 0;
}

int disn_trace_collect(const float* cams, int V, int H, int W, void* state, size_t state_bytes, float* pts,
                       void* stream) {
  const int64_t n = trace_rays(V, H, W);
  if (!cams || !state || !pts || !n) return DISN_E_ARG;
  if (state_bytes < trace_state_bytes((size_t)n)) return DISN_E_WS;
  DISN_TRY(trace_collect_launch(cams, V, H, W, state, pts, (hipStream_t)stream));
  return 0;
}

int disn_trace_shade(const float* cams, int V, int H, int W, const void* state, size_t state_bytes, const float* pred,
                     const float* grad, int64_t n_hits, float sdf_weight, float iso, float ambient, float* depth,
                     float* normal, float* residual, uint8_t* status, uint8_t* rgba, void* stream) {
  const int64_t n = trace_rays(V, H, W);
  if (!cams || !state || !n || n_hits < 0 || n_hits > n || (n_hits > 0 && (!pred || !grad)) || sdf_weight == 0.0f ||
      !(ambient >= 0.0f && ambient <= 1.0f))
    return DISN_E_ARG;
  if (state_bytes < trace_state_bytes((size_t)n)) return DISN_E_WS;
  DISN_TRY(trace_shade_launch(cams, V, H, W, state, pred, grad, (size_t)n_hits, sdf_weight, iso, ambient, depth, normal,
                              residual, status, rgba, (hipStream_t)stream));
  return 0;
}

}  // extern "C"

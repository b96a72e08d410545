// Vertex colours of device meshes from their input views, and their depth maps (include/disn_amd_colour.h; the rule is
// disn_amd/postprocess.py zbuffer_arrays / colour_arrays, restated here operation by operation): B meshes back to
// back, V views each.
//
//   z-buffer  validate indices and coordinates -> one thread per (face, view): a face whose clipped bounding box holds
//             at most kSmallBox sub-pixels is rasterised by its thread, a larger one is appended to a queue -> one WAVE
//             per queued (face, view) walks the box.  The buffer's maximum is an unsigned atomic max of the float's
//             bits: positive floats order as their bits do, so no bit depends on the order.
//   colour    one thread per vertex: the views, then the views of its reflection, in a fixed order -> fill rounds: a
//             scatter over the faces into 64-bit integer sums and counts, an apply over the vertices -> the mesh means
//             of the coloured vertices (block reduction, one integer atomic add per block) -> the bytes.
//
// NO KERNEL WAITS FOR ANOTHER WORKGROUP.  EVERY LOOP IS BOUNDED: by the grid stride, by V, by kSmallBox, by a clipped
// box of at most (137 S)^2 sub-pixels.  NO FLOATING-POINT ATOMIC: the sums are integer sums, the maximum an integer
// maximum.  No host read-back: progress[r] says whether fill round r has anything to do, and a round without returns
// at once.  Compiled with -ffp-contract=off: the float32 arithmetic rounds as numpy's does.
// (mesh_of, the two validators and the host-side helpers are those of mesh_batch.hpp.)
#include "mesh_batch.hpp"

#include "../../include/disn_amd_colour.h"

namespace disn {
namespace {

constexpr int kImg = DISN_COLOUR_IMG;
constexpr int kSmallBox = 64;                  // sub-pixels a thread rasterises itself
constexpr int kBigBlocks = 1024;               // of 4 waves each, striding over the queue of large faces
constexpr int kMeanSlices = 64;                // blocks per mesh of the fallback mean
constexpr unsigned char kUncoloured = 255;     // the working state of `seen`
constexpr int kGrey16 = 32768;
constexpr float kMirrorFront = 32.0f;          // postprocess.MIRROR_FRONT
constexpr float kTiny = 1.17549435e-38f;
constexpr float kBig = 3.4028234663852886e38f;

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= kBig; }

// _screen: the gather's projection in its order of operations; false unless w > 0 and x, y, q are finite
__device__ __forceinline__ bool screen(const float* __restrict__ T, float px, float py, float pz, int S, float& x,
                                       float& y, float& q, float& u, float& v) {
  float p[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    float a = px * T[j] + py * T[3 + j];
    a = a + pz * T[6 + j];
    p[j] = a + T[9 + j];
  }
  const float w = p[2];
  if (!(w > 0.0f)) return false;
  u = p[0] / w;
  v = p[1] / w;
  q = 1.0f / w;
  x = (u + 0.5f) * (float)S;
  y = (v + 0.5f) * (float)S;
  return finite_f(x) && finite_f(y) && finite_f(q);
}

struct Tri {
  float a[3], b[3], ex[3], ey[3];
  float x0, y0, q0, gx, gy, qmin, qmax;
  int i0, i1, j0, j1;
};

// _raster_view's per-triangle part; false for a triangle the rule skips.  N = 137 S; the box is clipped to [0, N-1].
__device__ __forceinline__ bool setup_tri(const float* __restrict__ verts, const long long gv[3],
                                          const float* __restrict__ T, int S, int N, Tri& t) {
  float X[3], Y[3], Q[3], u, v;
  for (int k = 0; k < 3; ++k)
    if (!screen(T, verts[3 * gv[k]], verts[3 * gv[k] + 1], verts[3 * gv[k] + 2], S, X[k], Y[k], Q[k], u, v)) return false;
  const float area = (X[1] - X[0]) * (Y[2] - Y[0]) - (X[2] - X[0]) * (Y[1] - Y[0]);
  const float dq1 = Q[1] - Q[0], dq2 = Q[2] - Q[0];
  const float gx = (dq1 * (Y[2] - Y[0]) - dq2 * (Y[1] - Y[0])) / area;
  const float gy = (dq2 * (X[1] - X[0]) - dq1 * (X[2] - X[0])) / area;
  const float fi0 = floorf(fminf(fminf(X[0], X[1]), X[2])), fi1 = floorf(fmaxf(fmaxf(X[0], X[1]), X[2]));
  const float fj0 = floorf(fminf(fminf(Y[0], Y[1]), Y[2])), fj1 = floorf(fmaxf(fmaxf(Y[0], Y[1]), Y[2]));
  const float top = (float)(N - 1);
  if (!(finite_f(area) && area != 0.0f && finite_f(gx) && finite_f(gy) && fi1 >= 0.0f && fi0 <= top && fj1 >= 0.0f &&
        fj0 <= top))
    return false;
  const float s = area > 0.0f ? 1.0f : -1.0f;
  const int ei[3] = {1, 2, 0}, ej[3] = {2, 0, 1};
  for (int k = 0; k < 3; ++k) {
    t.a[k] = s * (Y[ei[k]] - Y[ej[k]]);
    t.b[k] = s * (X[ej[k]] - X[ei[k]]);
    t.ex[k] = X[ei[k]];
    t.ey[k] = Y[ei[k]];
  }
  t.x0 = X[0]; t.y0 = Y[0]; t.q0 = Q[0]; t.gx = gx; t.gy = gy;
  t.qmin = fminf(fminf(Q[0], Q[1]), Q[2]);
  t.qmax = fmaxf(fmaxf(Q[0], Q[1]), Q[2]);
  t.i0 = (int)fmaxf(fi0, 0.0f); t.i1 = (int)fminf(fi1, top);
  t.j0 = (int)fmaxf(fj0, 0.0f); t.j1 = (int)fminf(fj1, top);
  return true;
}

// _cover at sub-pixel (i, j), 0 <= i, j < N, and the maximum
__device__ __forceinline__ void cover(const Tri& t, int i, int j, int N, float* zb) {
  const float cx = (float)i + 0.5f, cy = (float)j + 0.5f;
  bool inside = true;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    inside &= ((t.a[k] * (cx - t.ex[k]) + t.b[k] * (cy - t.ey[k])) + 0.5f * (fabsf(t.a[k]) + fabsf(t.b[k]))) >= 0.0f;
  if (!inside) return;
  float val = t.q0 + (t.gx * (cx - t.x0) + t.gy * (cy - t.y0));
  val = val > t.qmax ? t.qmax : val;
  val = val < t.qmin ? t.qmin : val;
  val = val - (fabsf(t.gx) + fabsf(t.gy));
  val = val >= kTiny ? val : kTiny;
  atomicMax(reinterpret_cast<unsigned*>(zb) + (size_t)j * N + i, __float_as_uint(val));
}

// the face and view of raster item t, its triangle and its buffer; false when the rule (or a status) skips it
__device__ __forceinline__ bool raster_item(long long item, const float* __restrict__ verts,
                                            const int* __restrict__ faces, const long long* __restrict__ voff,
                                            const long long* __restrict__ foff, int B, const int* __restrict__ status,
                                            const float* __restrict__ tm, int V, int S, int N, float* zbuf, Tri& t,
                                            float*& zb) {
  const long long f = item / V;
  const int k = (int)(item - f * V);
  const int b = mesh_of(foff, B, f);
  if (status[b]) return false;
  long long gv[3];
  for (int c = 0; c < 3; ++c) gv[c] = voff[b] + faces[3 * f + c];
  zb = zbuf + ((size_t)b * V + k) * N * N;
  return setup_tri(verts, gv, tm + ((size_t)b * V + k) * 12, S, N, t);
}

__global__ __launch_bounds__(kThreads) void raster_kernel(const float* __restrict__ verts,
                                                          const int* __restrict__ faces,
                                                          const long long* __restrict__ voff,
                                                          const long long* __restrict__ foff, int B, long long items,
                                                          const int* __restrict__ status,
                                                          const float* __restrict__ tm, int V, int S, float* zbuf,
                                                          unsigned long long* qcount, long long* __restrict__ queue) {
  const int N = kImg * S;
  GRID_STRIDE(item, items) {
    Tri t;
    float* zb;
    if (!raster_item(item, verts, faces, voff, foff, B, status, tm, V, S, N, zbuf, t, zb)) continue;
    const int bw = t.i1 - t.i0 + 1, count = bw * (t.j1 - t.j0 + 1);
    if (count > kSmallBox) {                                   // every item appends at most once: slot < items
      const unsigned long long slot = atomicAdd(qcount, 1ull);
      if (slot < (unsigned long long)items) queue[slot] = item;
      continue;
    }
    for (int n = 0; n < count; ++n) cover(t, t.i0 + n % bw, t.j0 + n / bw, N, zb);
  }
}

// one wave per queued (face, view); the order of the queue does not reach the result
__global__ __launch_bounds__(kThreads) void raster_big_kernel(const float* __restrict__ verts,
                                                              const int* __restrict__ faces,
                                                              const long long* __restrict__ voff,
                                                              const long long* __restrict__ foff, int B,
                                                              long long items, const int* __restrict__ status,
                                                              const float* __restrict__ tm, int V, int S, float* zbuf,
                                                              const unsigned long long* __restrict__ qcount,
                                                              const long long* __restrict__ queue) {
  const int N = kImg * S;
  const int lane = threadIdx.x & 63, waves_per_block = kThreads / 64;
  unsigned long long nq = *qcount;
  if (nq > (unsigned long long)items) nq = (unsigned long long)items;
  for (unsigned long long e = (unsigned long long)blockIdx.x * waves_per_block + (threadIdx.x >> 6); e < nq;
       e += (unsigned long long)gridDim.x * waves_per_block) {
    const long long item = queue[e];
    if (item < 0 || item >= items) continue;
    Tri t;
    float* zb;
    if (!raster_item(item, verts, faces, voff, foff, B, status, tm, V, S, N, zbuf, t, zb)) continue;
    const int bw = t.i1 - t.i0 + 1, count = bw * (t.j1 - t.j0 + 1);
    for (int n = lane; n < count; n += 64) cover(t, t.i0 + n % bw, t.j0 + n / bw, N, zb);
  }
}

// _seen_view for one point
__device__ __forceinline__ bool seen_at(const float* __restrict__ T, const float* __restrict__ zb,
                                        const unsigned char* __restrict__ alpha, float px, float py, float pz, int S,
                                        int N, float tol, bool reflected, float& u, float& v) {
  float x, y, q;
  if (!screen(T, px, py, pz, S, x, y, q, u, v)) return false;
  const float fi = floorf(x), fj = floorf(y), top = (float)(N - 1);
  if (!(fi >= 0.0f && fi <= top && fj >= 0.0f && fj <= top)) return false;
  const float z = zb[(size_t)(int)fj * N + (int)fi];
  if (!(q >= (1.0f - tol) * z)) return false;
  if (reflected && !(q <= (1.0f + kMirrorFront * tol) * z)) return false;
  if (alpha) {
    const float last = (float)(kImg - 1);
    const int pu = (int)rintf(fminf(fmaxf(u, 0.0f), last)), pv = (int)rintf(fminf(fmaxf(v, 0.0f), last));
    if (!(alpha[pv * kImg + pu] > 0)) return false;
  }
  return true;
}

// _sample16: adds the three channels of one view's sample to sum (R G B)
__device__ __forceinline__ void sample16(const float* __restrict__ img, float u, float v, int bgr, long long sum[3]) {
  const float last = (float)(kImg - 1);
  const float uc = fminf(fmaxf(u, 0.0f), last), vc = fminf(fmaxf(v, 0.0f), last);
  const float fx0 = floorf(uc), fy0 = floorf(vc);
  const int x0 = (int)fx0, y0 = (int)fy0;
  const int x1 = min(x0 + 1, kImg - 1), y1 = min(y0 + 1, kImg - 1);
  const float xl = uc - fx0, yl = vc - fy0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int ch = bgr ? 2 - c : c;
    const float tl = img[(y0 * kImg + x0) * 3 + ch], tr = img[(y0 * kImg + x1) * 3 + ch];
    const float bl = img[(y1 * kImg + x0) * 3 + ch], br = img[(y1 * kImg + x1) * 3 + ch];
    const float t = tl + (tr - tl) * xl;
    const float b = bl + (br - bl) * xl;
    float val = t + (b - t) * yl;
    val = val > 0.0f ? val : 0.0f;
    val = val < 1.0f ? val : 1.0f;
    sum[c] += (long long)rintf(val * 65535.0f);
  }
}

__device__ __forceinline__ int mean_half_up(long long total, long long n) { return (int)((2 * total + n) / (2 * n)); }

// classes 1 and 2: every view, then every view of the reflection, in a fixed order in one thread
__global__ __launch_bounds__(kThreads) void vertex_kernel(const float* __restrict__ verts,
                                                          const long long* __restrict__ voff, int B, long long nv,
                                                          const int* __restrict__ status,
                                                          const float* __restrict__ images,
                                                          const unsigned char* __restrict__ alpha,
                                                          const float* __restrict__ tm, int V, int S, float tol,
                                                          int mirror_axis, int bgr, const float* __restrict__ zbuf,
                                                          int* __restrict__ c16, unsigned char* __restrict__ cls) {
  const int N = kImg * S;
  GRID_STRIDE(v, nv) {
    const int b = mesh_of(voff, B, v);
    c16[3 * v] = c16[3 * v + 1] = c16[3 * v + 2] = 0;
    cls[v] = kUncoloured;
    if (status[b]) continue;
    float p[3] = {verts[3 * v], verts[3 * v + 1], verts[3 * v + 2]};
    for (int pass = 0; pass < 2; ++pass) {
      if (pass == 1) {
        if (mirror_axis < 0) break;
        p[mirror_axis] = -p[mirror_axis];
      }
      long long sum[3] = {0, 0, 0}, n = 0;
      for (int k = 0; k < V; ++k) {
        const size_t view = (size_t)b * V + k;
        float u, w;
        if (!seen_at(tm + view * 12, zbuf + view * N * N, alpha ? alpha + view * kImg * kImg : nullptr, p[0], p[1],
                     p[2], S, N, tol, pass == 1, u, w))
          continue;
        sample16(images + view * kImg * kImg * 3, u, w, bgr, sum);
        ++n;
      }
      if (n > 0) {
        for (int c = 0; c < 3; ++c) c16[3 * v + c] = mean_half_up(sum[c], n);
        cls[v] = pass == 0 ? 1 : 2;
        break;
      }
    }
  }
}

// fill round r, first half: every uncoloured corner of a face receives the face's coloured corners
__global__ __launch_bounds__(kThreads) void fill_scatter_kernel(const int* __restrict__ faces,
                                                                const long long* __restrict__ voff,
                                                                const long long* __restrict__ foff, int B,
                                                                long long nf, const int* __restrict__ status,
                                                                const int* __restrict__ progress, int round,
                                                                const int* __restrict__ c16,
                                                                const unsigned char* __restrict__ cls,
                                                                unsigned long long* acc) {
  if (!progress[round]) return;
  GRID_STRIDE(f, nf) {
    const int b = mesh_of(foff, B, f);
    if (status[b]) continue;
    long long gv[3];
    bool done[3];
    for (int k = 0; k < 3; ++k) {
      gv[k] = voff[b] + faces[3 * f + k];
      done[k] = cls[gv[k]] != kUncoloured;
    }
    for (int k = 0; k < 3; ++k) {
      if (done[k]) continue;
      for (int m = 0; m < 3; ++m) {
        if (m == k || !done[m]) continue;
        for (int c = 0; c < 3; ++c) atomicAdd(&acc[4 * gv[k] + c], (unsigned long long)c16[3 * gv[m] + c]);
        atomicAdd(&acc[4 * gv[k] + 3], 1ull);
      }
    }
  }
}

// fill round r, second half: the integer mean; the sums go back to zero for the next round
__global__ __launch_bounds__(kThreads) void fill_apply_kernel(long long nv, int* progress, int round,
                                                              int* __restrict__ c16, unsigned char* __restrict__ cls,
                                                              unsigned long long* __restrict__ acc) {
  if (!progress[round]) return;
  GRID_STRIDE(v, nv) {
    const long long n = (long long)acc[4 * v + 3];
    if (cls[v] != kUncoloured || n == 0) continue;
    for (int c = 0; c < 3; ++c) {
      c16[3 * v + c] = mean_half_up((long long)acc[4 * v + c], n);
      acc[4 * v + c] = 0;
    }
    acc[4 * v + 3] = 0;
    cls[v] = 3;
    progress[round + 1] = 1;
  }
}

// the sums of the coloured vertices of mesh blockIdx.y: block reduction, one atomic add per block and word
__global__ __launch_bounds__(kThreads) void mesh_mean_kernel(const long long* __restrict__ voff,
                                                             const int* __restrict__ status,
                                                             const int* __restrict__ c16,
                                                             const unsigned char* __restrict__ cls,
                                                             unsigned long long* meshacc) {
  __shared__ unsigned long long part[4];
  const int b = blockIdx.y;
  if (threadIdx.x < 4) part[threadIdx.x] = 0;
  __syncthreads();
  unsigned long long s[4] = {0, 0, 0, 0};
  if (!status[b]) {
    const long long v1 = voff[b + 1];
    for (long long v = voff[b] + (long long)blockIdx.x * kThreads + threadIdx.x; v < v1;
         v += (long long)gridDim.x * kThreads) {
      if (cls[v] == kUncoloured) continue;
      for (int c = 0; c < 3; ++c) s[c] += (unsigned long long)c16[3 * v + c];
      s[3] += 1;
    }
  }
  for (int c = 0; c < 4; ++c) {
    for (int d = 32; d > 0; d >>= 1) s[c] += __shfl_down(s[c], d, 64);
    if ((threadIdx.x & 63) == 0 && s[c]) atomicAdd(&part[c], s[c]);
  }
  __syncthreads();
  if (threadIdx.x < 4 && part[threadIdx.x]) atomicAdd(&meshacc[4 * b + threadIdx.x], part[threadIdx.x]);
}

// class 0 and the bytes
__global__ __launch_bounds__(kThreads) void finish_kernel(const long long* __restrict__ voff, int B, long long nv,
                                                          const int* __restrict__ status,
                                                          const unsigned long long* __restrict__ meshacc,
                                                          const int* __restrict__ c16, unsigned char* __restrict__ cls,
                                                          unsigned char* __restrict__ colours) {
  GRID_STRIDE(v, nv) {
    const int b = mesh_of(voff, B, v);
    int c[3] = {c16[3 * v], c16[3 * v + 1], c16[3 * v + 2]};
    if (cls[v] == kUncoloured) {
      const long long n = status[b] ? 0 : (long long)meshacc[4 * b + 3];
      for (int k = 0; k < 3; ++k) c[k] = n > 0 ? mean_half_up((long long)meshacc[4 * b + k], n) : kGrey16;
      cls[v] = 0;
    }
    for (int k = 0; k < 3; ++k) colours[3 * v + k] = (unsigned char)((c[k] * 255 + 32767) / 65535);
  }
}

// ---- host side -------------------------------------------------------------------------------------------------
struct ColourWs {
  long long *voff, *foff;                          // [B+1] each
  unsigned long long* qcount;                      // [1]    zeroed block starts here
  int* progress;                                   // [kMaxFill + 2]
  unsigned long long* meshacc;                     // [4 B]
  unsigned long long* acc;                         // [4 nv] zeroed block ends behind it
  size_t zero_bytes;
  int* c16;                                        // [3 nv]
  long long* queue;                                // [nf V]
  float* zbuf;                                     // [B V (137 S)^2] (disn_mesh_colour_batch only)
  size_t zbuf_bytes;
  size_t total;
};

ColourWs colour_layout(void* ws, int B, int V, long long nv, long long nf, int S) {
  WsCursor c(ws);
  const size_t b1 = (size_t)B + 1, f = (size_t)(nf > 0 ? nf : 1), v = (size_t)(nv > 0 ? nv : 1);
  ColourWs w;
  w.voff = c.take<long long>(b1); w.foff = c.take<long long>(b1);
  const size_t z0 = c.next();
  w.qcount = c.take<unsigned long long>(1);
  w.progress = c.take<int>(DISN_COLOUR_MAX_FILL + 2);
  w.meshacc = c.take<unsigned long long>(4 * b1);
  w.acc = c.take<unsigned long long>(4 * v);
  w.zero_bytes = c.off - z0;
  w.c16 = c.take<int>(3 * v);
  w.queue = c.take<long long>(f * (size_t)V);
  w.zbuf_bytes = (size_t)B * V * (kImg * S) * (kImg * S) * 4;
  w.zbuf = c.take<float>(w.zbuf_bytes / 4);
  w.total = c.next();
  return w;
}

bool batch_ok(int B, int V, int64_t nv, int64_t nf, int S) {
  return mesh_limits_ok(B, nv, nf) && B <= 65535 && V >= 1 && V <= DISN_COLOUR_MAX_VIEWS &&
         (S == 1 || S == 2 || S == 4);
}

// offsets to the device, the zeroed block, the statuses, the z-buffers of every (mesh, view) into `zbuf`
int zbuffer_run(const ColourWs& w, const float* verts, const int32_t* faces, const int64_t* v_off_host,
                const int64_t* f_off_host, int B, const float* tm, int V, int S, float* zbuf, int32_t* status,
                hipStream_t st) {
  const int64_t nv = v_off_host[B], nf = f_off_host[B];
  MESH_TRY(upload_offsets(w.voff, w.foff, v_off_host, f_off_host, B, st));
  MESH_TRY(hipMemsetAsync(w.qcount, 0, w.zero_bytes, st));
  MESH_TRY(hipMemsetAsync(status, 0, (size_t)B * 4, st));
  MESH_TRY(hipMemsetAsync(zbuf, 0, w.zbuf_bytes, st));
  if (nf > 0) MESH_LAUNCH(validate_faces_kernel, nf, faces, w.voff, w.foff, B, nf, status);
  if (nv > 0) MESH_LAUNCH(validate_verts_kernel, nv, verts, w.voff, B, nv, status);
  if (nf > 0 && nv > 0) {
    const long long items = (long long)nf * V;
    MESH_LAUNCH(raster_kernel, items, verts, faces, w.voff, w.foff, B, items, status, tm, V, S, zbuf, w.qcount, w.queue);
    hipLaunchKernelGGL(raster_big_kernel, dim3(kBigBlocks), dim3(kThreads), 0, st, verts, faces, w.voff, w.foff, B,
                       items, status, tm, V, S, zbuf, w.qcount, w.queue);
    MESH_TRY(hipGetLastError());
  }
  return 0;
}

}  // namespace
}  // namespace disn

using namespace disn;

extern "C" size_t disn_mesh_colour_workspace_bytes(int B, int V, int64_t nv_total, int64_t nf_total, int S) {
  return batch_ok(B, V, nv_total, nf_total, S) ? colour_layout(nullptr, B, V, nv_total, nf_total, S).total : 0;
}

extern "C" int disn_mesh_zbuffer_batch(const float* verts, const int32_t* faces, const int64_t* v_off_host,
                                       const int64_t* f_off_host, int B, const float* trans_mat, int V, int S,
                                       float* zbuf, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  if (!offsets_ok(v_off_host, f_off_host, B) || !trans_mat || !zbuf || !status || !ws) return DISN_E_ARG;
  const int64_t nv = v_off_host[B], nf = f_off_host[B];
  if ((nv > 0 && !verts) || (nf > 0 && !faces)) return DISN_E_ARG;
  if (!batch_ok(B, V, nv, nf, S)) return DISN_E_SHAPE;
  if (ws_bytes < colour_layout(nullptr, B, V, nv, nf, S).total) return DISN_E_WS;
  return zbuffer_run(colour_layout(ws, B, V, nv, nf, S), verts, faces, v_off_host, f_off_host, B, trans_mat, V, S, zbuf,
                     status, (hipStream_t)stream);
}

extern "C" int disn_mesh_colour_batch(const float* verts, const int32_t* faces, const int64_t* v_off_host,
                                      const int64_t* f_off_host, int B, const float* images, const uint8_t* alpha,
                                      const float* trans_mat, int V, int S, float rel_tol, int mirror_axis,
                                      int fill_iters, int bgr, uint8_t* colours, uint8_t* seen, int32_t* status,
                                      void* ws, size_t ws_bytes, void* stream) {
  if (!offsets_ok(v_off_host, f_off_host, B) || !images || !trans_mat || !status || !ws) return DISN_E_ARG;
  const int64_t nv = v_off_host[B], nf = f_off_host[B];
  if ((nv > 0 && (!verts || !colours || !seen)) || (nf > 0 && !faces)) return DISN_E_ARG;
  if (!batch_ok(B, V, nv, nf, S) || mirror_axis < -1 || mirror_axis > 2 || fill_iters < 0 ||
      fill_iters > DISN_COLOUR_MAX_FILL || !(rel_tol >= 0.0f && rel_tol < 1.0f))
    return DISN_E_SHAPE;
  if (ws_bytes < colour_layout(nullptr, B, V, nv, nf, S).total) return DISN_E_WS;
  hipStream_t st = (hipStream_t)stream;
  const ColourWs w = colour_layout(ws, B, V, nv, nf, S);
  const int rc = zbuffer_run(w, verts, faces, v_off_host, f_off_host, B, trans_mat, V, S, w.zbuf, status, st);
  if (rc != 0 || nv == 0) return rc;
  MESH_LAUNCH(vertex_kernel, nv, verts, w.voff, B, nv, status, images, alpha, trans_mat, V, S, rel_tol, mirror_axis,
         bgr ? 1 : 0, w.zbuf, w.c16, seen);
  if (nf > 0 && fill_iters > 0) {
    MESH_TRY(hipMemsetAsync(w.progress, 1, 4, st));             // round 0 always runs (any non-zero word)
    for (int r = 0; r < fill_iters; ++r) {
      MESH_LAUNCH(fill_scatter_kernel, nf, faces, w.voff, w.foff, B, nf, status, w.progress, r, w.c16, seen, w.acc);
      MESH_LAUNCH(fill_apply_kernel, nv, nv, w.progress, r, w.c16, seen, w.acc);
    }
  }
  hipLaunchKernelGGL(mesh_mean_kernel, dim3(kMeanSlices, B), dim3(kThreads), 0, st, w.voff, status, w.c16, seen,
                     w.meshacc);
  MESH_TRY(hipGetLastError());
  MESH_LAUNCH(finish_kernel, nv, w.voff, B, nv, status, w.meshacc, w.c16, seen, colours);
  return 0;
}

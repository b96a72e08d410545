// Forward-mode gradient of pred_sdf with respect to the query point: the non-GEMM launches.
// COMPILED WITH -ffp-contract=off: the projection is elementwise.hip's project_point, rounding for rounding, so a
// point falls into the bilinear cell the forward gather picks for it.
//
// A point travels as FOUR stacked rows, row 4 m = the value a, rows 4 m + 1 .. 4 m + 3 = the tangents da/dx, da/dy,
// da/dz.  A layer z = a W + b is one GEMM over the 4 n rows (no bias, no ReLU: api.hip grad_dense) followed by
//   a' = relu(z + b) on the value row,  t' = t W where z + b > 0, else 0, on the three tangent rows.
//
//   grad_embed       -- fold1/conv1 of both streams (models/sdfnet.py:71-72,173-174): t0 = I3, so the tangent rows
//                       are the rows of w1, masked
//   grad_act         -- bias + ReLU + mask after a GEMM (the global fold2/conv1 with the image's folded bias row)
//   grad_local_seed  -- the folded local fold2/conv1 (disn_fold_local): projection and its Jacobian
//                       (models/model_normalization.py:241-251), the four pmap rows of the point (:172-190), the
//                       value term g(u, v) and the tangent terms dg/du du/dp + dg/dv dv/dp, bias, ReLU, mask
//   grad_head        -- fold2/conv5 of both streams and their sum (models/sdfnet.py:88,186;
//                       models/model_normalization.py:204): four dot products per point
#include "kernels.hpp"

namespace disn {

namespace {

constexpr int kImg = 137;

__device__ __forceinline__ float clamp_px(float v) { return (v != v) ? v : fminf(136.0f, fmaxf(0.0f, v)); }

struct ProjJac {
  float u, v;          // clamped pixel coordinates, elementwise.hip project_point's bits
  float du[3], dv[3];  // d u / d p_k, d v / d p_k; zero for a coordinate whose clamp is active
};

__device__ __forceinline__ ProjJac project_jac(const float* __restrict__ T, float x, float y, float z) {
  float p[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    float a = x * T[0 * 3 + j] + y * T[1 * 3 + j];
    a = a + z * T[2 * 3 + j];
    p[j] = a + T[3 * 3 + j];
  }
  const float ru = p[0] / p[2], rv = p[1] / p[2];
  ProjJac r;
  r.u = clamp_px(ru);
  r.v = clamp_px(rv);
  const bool au = ru > 0.0f && ru < 136.0f, av = rv > 0.0f && rv < 136.0f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    r.du[k] = au ? (T[k * 3 + 0] - ru * T[k * 3 + 2]) / p[2] : 0.0f;
    r.dv[k] = av ? (T[k * 3 + 1] - rv * T[k * 3 + 2]) / p[2] : 0.0f;
  }
  return r;
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, const float4& v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float4 mask4(const float4& z, const float4& t) {
  return make_float4(z.x > 0.f ? t.x : 0.f, z.y > 0.f ? t.y : 0.f, z.z > 0.f ? t.z : 0.f, z.w > 0.f ? t.w : 0.f);
}
__device__ __forceinline__ float4 relu4(const float4& z) {
  return make_float4(fmaxf(z.x, 0.f), fmaxf(z.y, 0.f), fmaxf(z.z, 0.f), fmaxf(z.w, 0.f));
}

inline unsigned blocks_for(int64_t total, int64_t cap = 16384) {
  int64_t b = (total + 255) / 256;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (unsigned)b;
}

}  // namespace

// thread -> (point, 4 channels of one stream): 32 threads per point (16 per stream), as pt_embed_kernel
__global__ __launch_bounds__(256) void grad_embed_kernel(const float* __restrict__ pts, int64_t n,
                                                         const float* __restrict__ g_w1, const float* __restrict__ g_b1,
                                                         const float* __restrict__ l_w1, const float* __restrict__ l_b1,
                                                         float* __restrict__ out_g, float* __restrict__ out_l) {
  const int64_t total = n * 32;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t m = i >> 5;
    const int q = (int)(i & 31);
    const bool local = q >= 16;
    const int c = (q & 15) * 4;
    const float* w = local ? l_w1 : g_w1;
    const float x = pts[m * 3], y = pts[m * 3 + 1], z = pts[m * 3 + 2];
    const float4 w0 = ld4(w + c), w1 = ld4(w + 64 + c), w2 = ld4(w + 128 + c), b4 = ld4((local ? l_b1 : g_b1) + c);
    float4 s;
    s.x = x * w0.x + y * w1.x + z * w2.x + b4.x;
    s.y = x * w0.y + y * w1.y + z * w2.y + b4.y;
    s.z = x * w0.z + y * w1.z + z * w2.z + b4.z;
    s.w = x * w0.w + y * w1.w + z * w2.w + b4.w;
    float* o = (local ? out_l : out_g) + m * 4 * 64 + c;
    st4(o, relu4(s));
    st4(o + 64, mask4(s, w0));
    st4(o + 128, mask4(s, w1));
    st4(o + 192, mask4(s, w2));
  }
}

hipError_t grad_embed_launch(const float* pts, int64_t n, const float* g_w1, const float* g_b1, const float* l_w1,
                             const float* l_b1, float* out_g, float* out_l, hipStream_t st) {
  hipLaunchKernelGGL(grad_embed_kernel, dim3(blocks_for(n * 32)), dim3(256), 0, st, pts, n, g_w1, g_b1, l_w1, l_b1,
                     out_g, out_l);
  return hipGetLastError();
}

// in place on x [4 n][C] (C % 4 == 0): thread -> (point, float4 of the C channels), its four rows
__global__ __launch_bounds__(256) void grad_act_kernel(float* __restrict__ x, int64_t n, int C4,
                                                       const float* __restrict__ bias) {
  const int64_t total = n * C4;
  const int C = C4 * 4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t m = i / C4;
    const int c = (int)(i - m * C4) * 4;
    float* r = x + m * 4 * C + c;
    const float4 a = ld4(r), b4 = ld4(bias + c);
    const float4 s = make_float4(a.x + b4.x, a.y + b4.y, a.z + b4.z, a.w + b4.w);
    st4(r, relu4(s));
    st4(r + C, mask4(s, ld4(r + C)));
    st4(r + 2 * C, mask4(s, ld4(r + 2 * C)));
    st4(r + 3 * C, mask4(s, ld4(r + 3 * C)));
  }
}

hipError_t grad_act_launch(float* x, int64_t n, int C, const float* bias, hipStream_t st) {
  hipLaunchKernelGGL(grad_act_kernel, dim3(blocks_for(n * (C / 4))), dim3(256), 0, st, x, n, C / 4, bias);
  return hipGetLastError();
}

// in place on pre [4 n][512] = the stacked rows times the point rows of the local fold2/conv1: thread -> (point,
// float4 of the 512 outputs); a point's four 2-KiB pmap rows are read by 128 consecutive lanes (gather_fold_kernel's
// access pattern, resampler weights and validity)
__global__ __launch_bounds__(256) void grad_local_seed_kernel(const float* __restrict__ pmap_b,
                                                              const float* __restrict__ trans_mat_b,
                                                              const float* __restrict__ pts, int64_t n,
                                                              float* __restrict__ pre, const float* __restrict__ bias) {
  const int64_t total = n * 128;
  const unsigned lb = xcd_tile(gridDim.x, blockIdx.x);
  for (int64_t i = (int64_t)lb * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t pt = i >> 7;
    const int c = (int)(i & 127) * 4;
    const ProjJac pj = project_jac(trans_mat_b, pts[pt * 3], pts[pt * 3 + 1], pts[pt * 3 + 2]);
    const float x = pj.u, y = pj.v;
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f), gu = g, gv = g;
    const bool ok = x > -1.0f && y > -1.0f && x < (float)kImg && y < (float)kImg;
    if (ok) {
      const float fx = floorf(x), fy = floorf(y);
      const float cx = fx + 1.0f, cy = fy + 1.0f;
      const float dx = cx - x, dy = cy - y;
      const float ax = 1.0f - dx, ay = 1.0f - dy;
      const int ifx = (int)fx, ify = (int)fy, icx = (int)cx, icy = (int)cy;
      const float w_ff = dx * dy, w_cc = ax * ay, w_fc = dx * ay, w_cf = ax * dy;
      const bool xf = ifx >= 0 && ifx < kImg, xc = icx >= 0 && icx < kImg;
      const bool yf = ify >= 0 && ify < kImg, yc = icy >= 0 && icy < kImg;
      const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
      const float* m = pmap_b + c;
      const float4 v_ff = (xf && yf) ? ld4(m + ((size_t)ify * kImg + ifx) * 512) : z4;
      const float4 v_cc = (xc && yc) ? ld4(m + ((size_t)icy * kImg + icx) * 512) : z4;
      const float4 v_fc = (xf && yc) ? ld4(m + ((size_t)icy * kImg + ifx) * 512) : z4;
      const float4 v_cf = (xc && yf) ? ld4(m + ((size_t)ify * kImg + icx) * 512) : z4;
#define DISN_ACC(f)                                          \
  {                                                          \
    float t = w_ff * v_ff.f;                                 \
    t = t + w_cc * v_cc.f;                                   \
    t = t + w_fc * v_fc.f;                                   \
    t = t + w_cf * v_cf.f;                                   \
    g.f = t;                                                 \
    gu.f = dy * (v_cf.f - v_ff.f) + ay * (v_cc.f - v_fc.f);  \
    gv.f = dx * (v_fc.f - v_ff.f) + ax * (v_cc.f - v_cf.f);  \
  }
      DISN_ACC(x) DISN_ACC(y) DISN_ACC(z) DISN_ACC(w)
#undef DISN_ACC
    }
    float* r = pre + pt * 4 * 512 + c;
    const float4 p4 = ld4(r), b4 = ld4(bias + c);
    const float4 s = make_float4((p4.x + g.x) + b4.x, (p4.y + g.y) + b4.y, (p4.z + g.z) + b4.z, (p4.w + g.w) + b4.w);
    st4(r, relu4(s));
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float4 t = ld4(r + (k + 1) * 512);
      const float a = pj.du[k], b = pj.dv[k];
      const float4 o = make_float4(t.x + (gu.x * a + gv.x * b), t.y + (gu.y * a + gv.y * b),
                                   t.z + (gu.z * a + gv.z * b), t.w + (gu.w * a + gv.w * b));
      st4(r + (k + 1) * 512, mask4(s, o));
    }
  }
}

hipError_t grad_local_seed_launch(const float* pmap_b, const float* trans_mat_b, const float* pts, int64_t n,
                                  float* pre, const float* bias, hipStream_t st) {
  hipLaunchKernelGGL(grad_local_seed_kernel, dim3(blocks_for(n * 128)), dim3(256), 0, st, pmap_b, trans_mat_b, pts, n,
                     pre, bias);
  return hipGetLastError();
}

// one wave per stacked row: a lane holds a float4 of each stream's 256 activations (final_dot_kernel's reduction)
__global__ __launch_bounds__(256) void grad_head_kernel(const float* __restrict__ g5, const float* __restrict__ l5,
                                                        int64_t n, const float* __restrict__ g_w6,
                                                        const float* __restrict__ g_b6, const float* __restrict__ l_w6,
                                                        const float* __restrict__ l_b6, float* __restrict__ sdf,
                                                        float* __restrict__ grad) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const float4 wg = ld4(g_w6 + lane * 4), wl = ld4(l_w6 + lane * 4);
  const float bg = g_b6[0], bl = l_b6[0];
  for (int64_t row = wave; row < 4 * n; row += nwaves) {
    const float4 a = ld4(g5 + row * 256 + lane * 4), b = ld4(l5 + row * 256 + lane * 4);
    float vg = (a.x * wg.x + a.y * wg.y) + (a.z * wg.z + a.w * wg.w);
    float vl = (b.x * wl.x + b.y * wl.y) + (b.z * wl.z + b.w * wl.w);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      vg += __shfl_xor(vg, off);
      vl += __shfl_xor(vl, off);
    }
    if (lane == 0) {
      const int64_t m = row >> 2;
      const int r = (int)(row & 3);
      if (r == 0) {
        if (sdf) sdf[m] = (vg + bg) + (vl + bl);
      } else {
        grad[m * 3 + (r - 1)] = vg + vl;
      }
    }
  }
}

hipError_t grad_head_launch(const float* g5, const float* l5, int64_t n, const float* g_w6, const float* g_b6,
                            const float* l_w6, const float* l_b6, float* sdf, float* grad, hipStream_t st) {
  hipLaunchKernelGGL(grad_head_kernel, dim3(blocks_for(n * 4 * 64, 8192)), dim3(256), 0, st, g5, l5, n, g_w6, g_b6,
                     l_w6, l_b6, sdf, grad);
  return hipGetLastError();
}

}  // namespace disn

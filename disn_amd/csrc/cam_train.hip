// Training kernels of the camera network (cam_est/model_cam.py get_loss :124-239, models/posenet.py get_cam_mat
// :91-124): the camera losses with their gradient w.r.t. pred_RT, the head backward down to the VGG embedding, and
// the weight gradients of the 18 cameraprediction/* variables.  Compiled with -ffp-contract=off.
//
// Every reduction runs in a fixed order -- per-thread point loops, LDS trees, one ordered pass over the workgroup
// partials, wave shuffles in a fixed butterfly, batch sums in image order -- and nothing uses float atomics: the
// losses and every head gradient are bitwise repeatable.
//
// Losses (homo = [p, 1], T = pred_RT K^T, sub_3d = homo pred_RT - homo RT):
//   rotpc      = 1/2 sum sub_3d^2 (tf.nn.l2_loss is a scalar: not divided by B or N)
//   rot2d      = 1/2 sum (pred_xy - gt_xy)^2 / 1e4, xy = xyz[:2] / xyz[2] UNclipped
//   rotmatrix  = mean((pred_T - T)^2) over B*4*3
//   rot2d_dist = mean over points of |clip(gt_xy) - clip(pred_xy)|, clip to [0,136]^2; rot3d_dist = mean |sub_3d|
// d(rotpc)/d(pred_RT) = M_b D with M_b = sum_n homo homo^T (4x4) and D = pred_RT - RT: the point pass only
// accumulates M_b.  The 2-D term reaches pred_RT through T: dRT += dT K.
#include "../../include/disn_amd.h"

#include "kernels.hpp"

namespace disn {

namespace {

constexpr int kLossThreads = 256, kLossPpt = 4, kLossChunk = kLossThreads * kLossPpt;
constexpr int kAcc = 25;  // dT[12] | rot2d | M: xx xy xz yy yz zz x y z | rotpc | sum d2 | sum d3

int loss_chunks(int N) { return (N + kLossChunk - 1) / kLossChunk; }

__global__ __launch_bounds__(kLossThreads) void cam_loss_points_kernel(const float* __restrict__ pred_RT,
                                                                       const float* __restrict__ pred_T,
                                                                       const float* __restrict__ pts,
                                                                       const float* __restrict__ RT,
                                                                       const float* __restrict__ T, int N,
                                                                       float* __restrict__ partials) {
  __shared__ float red[kAcc][kLossThreads];
  const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
  float pr[12], rt[12], pt[12], gt[12];
  for (int i = 0; i < 12; ++i) {
    pr[i] = pred_RT[(size_t)b * 12 + i];
    rt[i] = RT[(size_t)b * 12 + i];
    pt[i] = pred_T[(size_t)b * 12 + i];
    gt[i] = T[(size_t)b * 12 + i];
  }
  float acc[kAcc];
  for (int k = 0; k < kAcc; ++k) acc[k] = 0.f;
  for (int j = 0; j < kLossPpt; ++j) {
    const int n = chunk * kLossChunk + j * kLossThreads + tid;
    if (n >= N) break;
    const float* p = pts + ((size_t)b * N + n) * 3;
    const float h[4] = {p[0], p[1], p[2], 1.f};
    float xyz_p[3], xyz_g[3], sq = 0.f;
    for (int c = 0; c < 3; ++c) {
      float a = 0.f, r = 0.f, u = 0.f, v = 0.f;
      for (int q = 0; q < 4; ++q) {
        a += h[q] * pr[q * 3 + c];
        r += h[q] * rt[q * 3 + c];
        u += h[q] * pt[q * 3 + c];
        v += h[q] * gt[q * 3 + c];
      }
      const float s = a - r;
      sq += s * s;
      xyz_p[c] = u;
      xyz_g[c] = v;
    }
    const float px = xyz_p[0] / xyz_p[2], py = xyz_p[1] / xyz_p[2];
    const float gx = xyz_g[0] / xyz_g[2], gy = xyz_g[1] / xyz_g[2];
    const float ex = px - gx, ey = py - gy;
    // d(1/2 |e|^2)/d xyz_p through the division by z
    const float dxyz[3] = {ex / xyz_p[2], ey / xyz_p[2], -(ex * px + ey * py) / xyz_p[2]};
    for (int q = 0; q < 4; ++q)
      for (int c = 0; c < 3; ++c) acc[q * 3 + c] += h[q] * dxyz[c];
    acc[12] += 0.5f * (ex * ex + ey * ey);
    acc[13] += h[0] * h[0]; acc[14] += h[0] * h[1]; acc[15] += h[0] * h[2];
    acc[16] += h[1] * h[1]; acc[17] += h[1] * h[2]; acc[18] += h[2] * h[2];
    acc[19] += h[0]; acc[20] += h[1]; acc[21] += h[2];
    acc[22] += 0.5f * sq;
    const float cgx = fminf(136.f, fmaxf(0.f, gx)), cgy = fminf(136.f, fmaxf(0.f, gy));
    const float cpx = fminf(136.f, fmaxf(0.f, px)), cpy = fminf(136.f, fmaxf(0.f, py));
    const float dx = cgx - cpx, dy = cgy - cpy;
    acc[23] += sqrtf(dx * dx + dy * dy);
    acc[24] += sqrtf(sq);
  }
  for (int k = 0; k < kAcc; ++k) red[k][tid] = acc[k];
  __syncthreads();
  for (int s = kLossThreads / 2; s > 0; s >>= 1) {
    if (tid < s)
      for (int k = 0; k < kAcc; ++k) red[k][tid] += red[k][tid + s];
    __syncthreads();
  }
  if (tid < kAcc) partials[((size_t)b * gridDim.x + chunk) * kAcc + tid] = red[tid][0];
}

// one workgroup: per image the ordered sum over its chunk partials and the 4x4 / 4x3 algebra, then thread 0 sums
// the per-image terms in image order
__global__ __launch_bounds__(256) void cam_loss_finish_kernel(const float* __restrict__ partials, int chunks,
                                                              const float* __restrict__ pred_RT,
                                                              const float* __restrict__ RT,
                                                              const float* __restrict__ pred_T,
                                                              const float* __restrict__ T, CamK K, int B, int N,
                                                              float w3d, float w2d, float wmat,
                                                              const float* __restrict__ reg,
                                                              float* __restrict__ terms, float* __restrict__ losses,
                                                              float* __restrict__ dists, float* __restrict__ dRT) {
  const float inv_n = 1.f / (float)N, mat_scale = 2.f / (float)(B * 12);
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    float A[kAcc];
    for (int k = 0; k < kAcc; ++k) A[k] = 0.f;
    for (int c = 0; c < chunks; ++c)
      for (int k = 0; k < kAcc; ++k) A[k] += partials[((size_t)b * chunks + c) * kAcc + k];
    const float M[4][4] = {{A[13], A[14], A[15], A[19]},
                           {A[14], A[16], A[17], A[20]},
                           {A[15], A[17], A[18], A[21]},
                           {A[19], A[20], A[21], (float)N}};
    float D[12], dT[12], mat = 0.f;
    for (int i = 0; i < 12; ++i) {
      D[i] = pred_RT[(size_t)b * 12 + i] - RT[(size_t)b * 12 + i];
      const float e = pred_T[(size_t)b * 12 + i] - T[(size_t)b * 12 + i];
      mat += e * e;
      dT[i] = w2d * (A[i] * 1e-4f) + wmat * (mat_scale * e);
    }
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 3; ++c) {
        float md = 0.f;
        for (int q = 0; q < 4; ++q) md += M[r][q] * D[q * 3 + c];
        // T[r][j] = sum_c RT[r][c] K[j][c]  =>  dRT[r][c] += sum_j dT[r][j] K[j][c]
        float tk = 0.f;
        for (int j = 0; j < 3; ++j) tk += dT[r * 3 + j] * K.k[j * 3 + c];
        dRT[(size_t)b * 12 + r * 3 + c] = w3d * md + tk;
      }
    const float d2 = A[23] * inv_n, d3 = A[24] * inv_n;
    dists[b] = d2;
    dists[(size_t)B + b] = d3;
    terms[(size_t)b * 5 + 0] = A[22];
    terms[(size_t)b * 5 + 1] = A[12];
    terms[(size_t)b * 5 + 2] = mat;
    terms[(size_t)b * 5 + 3] = d2;
    terms[(size_t)b * 5 + 4] = d3;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int b = 0; b < B; ++b)
      for (int k = 0; k < 5; ++k) s[k] += terms[(size_t)b * 5 + k];
    const float rotpc = s[0], rot2d = s[1] / 10000.f, rotmat = s[2] / (float)(B * 12);
    const float r = reg ? *reg : 0.f;
    losses[0] = rotpc;
    losses[1] = rot2d;
    losses[2] = rotmat;
    losses[3] = s[3] / (float)B;
    losses[4] = s[4] / (float)B;
    losses[5] = r;
    losses[6] = ((w2d * rot2d + w3d * rotpc) + wmat * rotmat) + r;
  }
}

__device__ __forceinline__ void cross3(const float* a, const float* b, float* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// backward of v = w / max(|w|, 1e-8) given v and n = |w|; TF's maximum passes the gradient to |w| on ties
// (n >= 1e-8): dw = (dv - v (v . dv)) / n -- the projected form, so that a direction along v cancels exactly --
// and otherwise (the constant 1e-8) dw = dv / 1e-8
__device__ __forceinline__ void normalize_bwd(const float* v, float n, const float* dv, float* dw) {
  const float m = fmaxf(n, 1e-8f);
  const float vdv = n >= 1e-8f ? v[0] * dv[0] + v[1] * dv[1] + v[2] * dv[2] : 0.f;
  for (int i = 0; i < 3; ++i) dw[i] = (dv[i] - v[i] * vdv) / m;
}

// d(o3) of one image from dRT: pred_RT rows 0..2 = s (x | y | z) (columns), row 3 = t + const
__device__ void gram_schmidt_bwd(const float* o3, const float* dR, float* d) {
  const float s = o3[0];
  const float a[3] = {o3[1], o3[2], o3[3]}, bb[3] = {o3[4], o3[5], o3[6]};
  const float na = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), ma = fmaxf(na, 1e-8f);
  const float x[3] = {a[0] / ma, a[1] / ma, a[2] / ma};
  float w[3], z[3], y[3];
  cross3(x, bb, w);
  const float nw = sqrtf(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]), mw = fmaxf(nw, 1e-8f);
  for (int i = 0; i < 3; ++i) z[i] = w[i] / mw;
  cross3(z, x, y);
  float ds = 0.f, dx[3], dy[3], dz[3];
  for (int i = 0; i < 3; ++i) {
    ds += dR[i * 3 + 0] * x[i] + dR[i * 3 + 1] * y[i] + dR[i * 3 + 2] * z[i];
    dx[i] = s * dR[i * 3 + 0];
    dy[i] = s * dR[i * 3 + 1];
    dz[i] = s * dR[i * 3 + 2];
  }
  // y = z x x:  dz += x x dy,  dx += dy x z
  float t[3];
  cross3(x, dy, t);
  for (int i = 0; i < 3; ++i) dz[i] += t[i];
  cross3(dy, z, t);
  for (int i = 0; i < 3; ++i) dx[i] += t[i];
  // z = n(w), w = x x b:  dx += b x dw,  db = dw x x
  float dw[3], db[3], da[3];
  normalize_bwd(z, nw, dz, dw);
  cross3(bb, dw, t);
  for (int i = 0; i < 3; ++i) dx[i] += t[i];
  cross3(dw, x, db);
  normalize_bwd(x, na, dx, da);
  d[0] = ds;
  for (int i = 0; i < 3; ++i) {
    d[1 + i] = da[i];
    d[4 + i] = db[i];
    d[7 + i] = dR[9 + i];
  }
}

__device__ __forceinline__ float wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

constexpr int kBwdRows = 64;  // rows of a layer's data gradient per workgroup (16 per wave)

// Gram-Schmidt backward + fc3 backward (all 352 rows, cheap) + 64 rows of the fc2 backward; grid (B, 11)
__global__ __launch_bounds__(256) void cam_head_bwd_kernel(const disn_cam_weights_t w, const float* __restrict__ save,
                                                           const float* __restrict__ dRT, float* __restrict__ dsave) {
  __shared__ float d3[10], dh2[352];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* sv = save + (size_t)b * CAM_SAVE_STRIDE;
  float* dsv = dsave + (size_t)b * CAM_SAVE_STRIDE;
  if (tid == 0) {
    float dR[12], d[10];
    for (int i = 0; i < 12; ++i) dR[i] = dRT[(size_t)b * 12 + i];
    gram_schmidt_bwd(sv + CAM_SAVE_O3, dR, d);
    for (int i = 0; i < 10; ++i) {
      d3[i] = d[i];
      if (blockIdx.y == 0) dsv[CAM_SAVE_O3 + i] = d[i];
    }
  }
  __syncthreads();
  for (int n = tid; n < 352; n += 256) {
    const float* W;
    int ld, c0, k;
    if (n < 32) { W = w.s_w3; ld = 1; c0 = 0; k = n; }
    else if (n < 288) { W = w.r_w3; ld = 6; c0 = 1; k = n - 32; }
    else { W = w.t_w3; ld = 3; c0 = 7; k = n - 288; }
    float acc = 0.f;
    for (int c = 0; c < ld; ++c) acc += W[(size_t)k * ld + c] * d3[c0 + c];
    const float g = sv[CAM_SAVE_H2 + n] > 0.f ? acc : 0.f;
    dh2[n] = g;
    if (blockIdx.y == 0) dsv[CAM_SAVE_H2 + n] = g;
  }
  __syncthreads();
  for (int r = wave; r < kBwdRows; r += 4) {
    const int n = blockIdx.y * kBwdRows + r;  // row of h1 (704 = 11 x 64)
    const float* W;
    int ld, c0, k;
    if (n < 64) { W = w.s_w2; ld = 32; c0 = 0; k = n; }
    else if (n < 576) { W = w.r_w2; ld = 256; c0 = 32; k = n - 64; }
    else { W = w.t_w2; ld = 64; c0 = 288; k = n - 576; }
    float acc = 0.f;
    for (int c = lane; c < ld; c += 64) acc += W[(size_t)k * ld + c] * dh2[c0 + c];
    acc = wave_sum(acc);
    if (lane == 0) dsv[n] = sv[n] > 0.f ? acc : 0.f;
  }
}

// fc1 backward: demb[b][k] = sum over the 704 columns of [s_w1 | r_w1 | t_w1][k] * dh1; grid (B, 16)
__global__ __launch_bounds__(256) void cam_emb_bwd_kernel(const disn_cam_weights_t w, const float* __restrict__ dsave,
                                                          float* __restrict__ demb) {
  __shared__ float dh1[704];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < 704; i += 256) dh1[i] = dsave[(size_t)b * CAM_SAVE_STRIDE + i];
  __syncthreads();
  for (int r = wave; r < kBwdRows; r += 4) {
    const int k = blockIdx.y * kBwdRows + r;
    float acc = 0.f;
    for (int c = lane; c < 704; c += 64) {
      float wv;
      if (c < 64) wv = w.s_w1[(size_t)k * 64 + c];
      else if (c < 576) wv = w.r_w1[(size_t)k * 512 + (c - 64)];
      else wv = w.t_w1[(size_t)k * 128 + (c - 576)];
      acc += wv * dh1[c];
    }
    acc = wave_sum(acc);
    if (lane == 0) demb[(size_t)b * 1024 + k] = acc;
  }
}

// the 18 variables: out[k][c] = sum_b a[b][k] g[b][c] (a = 1 for biases), images in order
struct CamWgradJobs {
  float* out[18];
  int a_src[18];  // 0 embedding, 1 saved activations, -1 none (bias)
  int a_off[18], g_off[18], rows[18], cols[18];
  long start[19];
};

__global__ __launch_bounds__(256) void cam_head_wgrad_kernel(const CamWgradJobs J, const float* __restrict__ emb,
                                                             const float* __restrict__ save,
                                                             const float* __restrict__ dsave, int B) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= J.start[18]) return;
  int j = 0;
  while (e >= J.start[j + 1]) ++j;
  const long l = e - J.start[j];
  const int k = (int)(l / J.cols[j]), c = (int)(l % J.cols[j]);
  const float* a = J.a_src[j] == 0 ? emb + k : (J.a_src[j] == 1 ? save + J.a_off[j] + k : nullptr);
  const size_t as = J.a_src[j] == 0 ? 1024 : CAM_SAVE_STRIDE;
  const float* g = dsave + J.g_off[j] + c;
  float acc = 0.f;
  for (int b = 0; b < B; ++b) {
    const float gv = g[(size_t)b * CAM_SAVE_STRIDE];
    acc += a ? a[(size_t)b * as] * gv : gv;
  }
  J.out[j][l] = acc;
}

}  // namespace

size_t cam_loss_ws_floats(int B, int N) { return (size_t)B * loss_chunks(N) * kAcc + (size_t)B * 5; }

hipError_t cam_loss_launch(const float* pred_RT, const float* pred_T, const float* pts, const float* RT,
                           const float* T, const CamK& K, int B, int N, int loss_mode, const float* reg,
                           float* losses, float* dists, float* dRT, float* ws, hipStream_t st) {
  // loss_mode: 0 "3D" rotpc; 1 "2D" rot2d; 2 "3DM" rotpc + 0.3 rotmatrix; 3 (any other) all three
  const float w3d = loss_mode == 1 ? 0.f : 1.f;
  const float w2d = (loss_mode == 1 || loss_mode == 3) ? 1.f : 0.f;
  const float wmat = loss_mode == 2 ? 0.3f : (loss_mode == 3 ? 1.f : 0.f);
  const int chunks = loss_chunks(N);
  float* terms = ws + (size_t)B * chunks * kAcc;
  hipLaunchKernelGGL(cam_loss_points_kernel, dim3(chunks, B), dim3(kLossThreads), 0, st, pred_RT, pred_T, pts, RT,
                     T, N, ws);
  hipLaunchKernelGGL(cam_loss_finish_kernel, dim3(1), dim3(256), 0, st, ws, chunks, pred_RT, RT, pred_T, T, K, B, N,
                     w3d, w2d, wmat, reg, terms, losses, dists, dRT);
  return hipGetLastError();
}

hipError_t cam_head_bwd_launch(const disn_cam_weights_t& w, const float* save, const float* dRT, int B,
                               float* dsave, float* demb, hipStream_t st) {
  hipLaunchKernelGGL(cam_head_bwd_kernel, dim3(B, 704 / kBwdRows), dim3(256), 0, st, w, save, dRT, dsave);
  hipLaunchKernelGGL(cam_emb_bwd_kernel, dim3(B, 1024 / kBwdRows), dim3(256), 0, st, w, dsave, demb);
  return hipGetLastError();
}

hipError_t cam_head_wgrad_launch(const float* emb, const float* save, const float* dsave, int B, const CamGrads& g,
                                 hipStream_t st) {
  // towers (scale, ortho6d, translation): widths of fc1 / fc2 / fc3 and their column offsets in save
  const int n1[3] = {64, 512, 128}, n2[3] = {32, 256, 64}, n3[3] = {1, 6, 3};
  const int o1[3] = {0, 64, 576}, o2[3] = {0, 32, 288}, o3[3] = {0, 1, 7};
  CamWgradJobs J{};
  long at = 0;
  for (int t = 0; t < 3; ++t) {
    const int rows[3] = {1024, n1[t], n2[t]}, cols[3] = {n1[t], n2[t], n3[t]};
    const int aoff[3] = {0, o1[t], CAM_SAVE_H2 + o2[t]};
    const int goff[3] = {o1[t], CAM_SAVE_H2 + o2[t], CAM_SAVE_O3 + o3[t]};
    for (int l = 0; l < 3; ++l)
      for (int isb = 0; isb < 2; ++isb) {
        const int j = t * 6 + l * 2 + isb;
        J.out[j] = g.p[j];
        J.a_src[j] = isb ? -1 : (l == 0 ? 0 : 1);
        J.a_off[j] = aoff[l];
        J.g_off[j] = goff[l];
        J.rows[j] = isb ? 1 : rows[l];
        J.cols[j] = cols[l];
        J.start[j] = at;
        at += (long)J.rows[j] * J.cols[j];
      }
  }
  J.start[18] = at;
  hipLaunchKernelGGL(cam_head_wgrad_kernel, dim3((unsigned)((at + 255) / 256)), dim3(256), 0, st, J, emb, save,
                     dsave, B);
  return hipGetLastError();
}

}  // namespace disn

namespace {
struct CamLossWs {
  float *rot, *trans, *pred_RT, *save, *dsave, *loss_ws;
  size_t total;
};
CamLossWs cam_loss_layout(void* base, int B, int N) {
  char* p = static_cast<char*>(base);
  size_t off = 0;
  auto take = [&](size_t n) {
    off = (off + 255) & ~size_t(255);
    float* r = p ? reinterpret_cast<float*>(p + off) : nullptr;
    off += n * sizeof(float);
    return r;
  };
  CamLossWs t;
  t.rot = take((size_t)B * 9); t.trans = take((size_t)B * 3); t.pred_RT = take((size_t)B * 12);
  t.save = take((size_t)B * disn::CAM_SAVE_STRIDE); t.dsave = take((size_t)B * disn::CAM_SAVE_STRIDE);
  t.loss_ws = take(disn::cam_loss_ws_floats(B, N));
  t.total = (off + 255) & ~size_t(255);
  return t;
}
}  // namespace

extern "C" size_t disn_cam_loss_backward_workspace_bytes(int B, int N) {
  if (B <= 0 || N <= 0 || !disn::fits_int(B, N, 3) || !disn::fits_int(B, DISN_EMBED_DIM)) return 0;
  return cam_loss_layout(nullptr, B, N).total;
}

extern "C" int disn_cam_loss_backward(const disn_cam_weights_t* w, const float* embedding, const float* K_host,
                                      const float* pts, const float* RT, const float* trans_mat, int B, int N,
                                      int loss_mode, float* pred_trans_mat, float* losses, float* dists, float* dRT,
                                      float* demb, float* head_grads, void* ws, size_t ws_bytes, void* stream) {
  if (!w || !embedding || !pts || !RT || !trans_mat || !pred_trans_mat || !losses || !dists || !dRT || !demb ||
      !head_grads || !ws || B <= 0 || N <= 0 || loss_mode < 0 || loss_mode > 3)
    return DISN_E_ARG;
  if (!disn::fits_int(B, N, 3) || !disn::fits_int(B, DISN_EMBED_DIM)) return DISN_E_SHAPE;
  const float* const* wp = reinterpret_cast<const float* const*>(w);
  for (int i = 0; i < 18; ++i)
    if (!wp[i]) return DISN_E_ARG;
  const CamLossWs t = cam_loss_layout(ws, B, N);
  if (ws_bytes < t.total) return DISN_E_WS;
  disn_cam_param_layout_t L;
  disn_cam_param_layout(&L);
  hipStream_t st = (hipStream_t)stream;
  const disn::CamK K = disn::cam_k(K_host);
  hipError_t e = disn::cam_head_launch(*w, embedding, K, B, t.rot, t.trans, t.pred_RT, pred_trans_mat, t.save, st);
  if (e == hipSuccess)
    e = disn::cam_loss_launch(t.pred_RT, pred_trans_mat, pts, RT, trans_mat, K, B, N, loss_mode, nullptr, losses,
                              dists, dRT, t.loss_ws, st);
  if (e == hipSuccess) e = disn::cam_head_bwd_launch(*w, t.save, dRT, B, t.dsave, demb, st);
  if (e == hipSuccess) {
    disn::CamGrads g;
    for (int j = 0; j < 18; ++j) g.p[j] = head_grads + (L.offset[32 + j] - L.offset[32]);
    e = disn::cam_head_wgrad_launch(embedding, t.save, t.dsave, B, g, st);
  }
  return e == hipSuccess ? 0 : (int)e;
}

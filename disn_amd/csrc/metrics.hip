// Point-cloud evaluation metrics of the DISN test scripts (test/test_cd_emd.py, test/test_f_score.py):
// the two custom ops of models/tf_ops, restated for gfx950 (THIS FILE IS COMPILED WITH -ffp-contract=off).
//
// nn_distance: for every point of one cloud the smallest squared distance to the other cloud and the lowest
//   index that attains it, both directions.  d2 = (dx*dx + dy*dy) + dz*dz with d = ref - query, every step an
//   fp32 rounding, nothing contracted: the result is bit-identical to a numpy float32 restatement.  Queries sit
//   in registers (kNnQ per lane), reference points are staged in LDS and read as a wave-wide broadcast.  The
//   reference set is split across workgroups so that the chip fills even for one pair; the splits merge with a
//   64-bit atomicMin on (float_bits(d2) << 32 | idx): for d2 >= 0 that key orders by distance, then by lowest
//   index (the reference kernel's tie rule), whatever the order the workgroups finish in.
//
// approx_match / emd: the GPU schedule of tf_approxmatch_g.cu (levels -4^j, j = 7..-1, then 0; three dependent
//   passes per level), as 30 stream-ordered launches over a workspace that holds remainL/remainR/ratioL/ratioR.
//   Every pass is "owner computes": passes 1 and 3 own points k of xyz1 and loop over xyz2, pass 2 owns points l
//   of xyz2 and loops over xyz1.  A workgroup owns 64 points (one per lane); its S waves split the loop into S
//   contiguous slices and the S partial sums meet in LDS, summed in wave order.  S depends on the loop length
//   only, so every summation order is a function of (n, m): a pair's result never depends on b or on its place
//   in the batch.  No float atomics, no grid barrier.  E = v_exp_f32(d2 * level*log2(e)) (__expf semantics).
//   The fused emd form accumulates w * sqrt(d2) per owner in pass 3 (double across slices and levels) and sums
//   the owners in a fixed tree at the end: no b*m*n match buffer.
#include "kernels.hpp"

namespace disn {

namespace {

constexpr int kNnThreads = 256;
constexpr int kNnQ = 4;                         // queries per lane
constexpr int kNnQBlock = kNnThreads * kNnQ;    // queries per workgroup
constexpr int kNnTile = 1024;                   // reference points per LDS tile (16 KB)
constexpr int kEmdOwners = 64;                  // owners per workgroup = lanes of a wave
constexpr int kEmdMaxWaves = 16;
constexpr int kCostRows = 16;                   // match rows per match_cost workgroup

inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }
inline int cdiv(int a, int b) { return (int)(((long long)a + b - 1) / b); }

struct NnPlan {
  int qblocks, chunk, splits;
};

// split the reference set so that a direction launches ~2048 workgroups (>= 256 reference points each)
NnPlan nn_plan(int b, int nq, int nr) {
  NnPlan p;
  p.qblocks = cdiv(nq, kNnQBlock);
  const long long have = (long long)p.qblocks * b;
  int want = (int)((2048 + have - 1) / have);
  const int most = cdiv(nr, 256);
  if (want > most) want = most;
  if (want < 1) want = 1;
  p.chunk = cdiv(nr, want);
  p.splits = cdiv(nr, p.chunk);
  return p;
}

// waves per emd workgroup: a function of the loop length only (batch invariance)
int emd_waves(int loop_len) {
  int s = 1;
  while (s < kEmdMaxWaves && s * 128 < loop_len) s *= 2;
  return s;
}

struct EmdWs {
  float *remL, *remR, *ratL, *ratR;
  double* costK;   // [b][n] per-owner cost, summed over levels
  size_t total;
};

EmdWs emd_layout(void* ws, int b, int n, int m) {
  char* base = static_cast<char*>(ws);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off = align256(off + bytes);
    return p;
  };
  EmdWs w;
  w.remL = reinterpret_cast<float*>(take((size_t)b * n * 4));
  w.remR = reinterpret_cast<float*>(take((size_t)b * m * 4));
  w.ratL = reinterpret_cast<float*>(take((size_t)b * n * 4));
  w.ratR = reinterpret_cast<float*>(take((size_t)b * m * 4));
  w.costK = reinterpret_cast<double*>(take((size_t)b * n * 8));
  w.total = off;
  return w;
}

// ---------------------------------------------------------------------------------------------------------------
// nearest neighbour
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kNnThreads) void nn_kernel(const float* __restrict__ q, const float* __restrict__ r,
                                                        int nq, int nr, int qblocks, int chunk,
                                                        unsigned long long* __restrict__ keys) {
  __shared__ float4 tile[kNnTile];
  const int pair = blockIdx.y;
  const int qb = blockIdx.x % qblocks, sp = blockIdx.x / qblocks;
  const int r0 = sp * chunk;
  const int r1 = min(nr, r0 + chunk);
  const float* qp = q + (size_t)pair * nq * 3;
  const float* rp = r + (size_t)pair * nr * 3;
  float qx[kNnQ], qy[kNnQ], qz[kNnQ], best[kNnQ];
  int bi[kNnQ];
#pragma unroll
  for (int i = 0; i < kNnQ; ++i) {
    const int j = min(qb * kNnQBlock + i * kNnThreads + (int)threadIdx.x, nq - 1);
    qx[i] = qp[3 * (size_t)j];
    qy[i] = qp[3 * (size_t)j + 1];
    qz[i] = qp[3 * (size_t)j + 2];
    best[i] = __int_as_float(0x7f800000);
    bi[i] = r0;
  }
  for (int t0 = r0; t0 < r1; t0 += kNnTile) {
    const int cnt = min(kNnTile, r1 - t0);
    __syncthreads();
    for (int l = threadIdx.x; l < cnt; l += kNnThreads) {
      const size_t g = 3 * (size_t)(t0 + l);
      tile[l] = make_float4(rp[g], rp[g + 1], rp[g + 2], 0.f);
    }
    __syncthreads();
#pragma unroll 4
    for (int l = 0; l < cnt; ++l) {
      const float4 p = tile[l];
#pragma unroll
      for (int i = 0; i < kNnQ; ++i) {
        const float dx = p.x - qx[i], dy = p.y - qy[i], dz = p.z - qz[i];
        const float d = (dx * dx + dy * dy) + dz * dz;
        if (d < best[i]) {   // strict: the first (lowest) index of the slice keeps a tie
          best[i] = d;
          bi[i] = t0 + l;
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < kNnQ; ++i) {
    const int j = qb * kNnQBlock + i * kNnThreads + (int)threadIdx.x;
    if (j < nq) {
      const unsigned long long key =
          ((unsigned long long)__float_as_uint(best[i]) << 32) | (unsigned long long)(unsigned)bi[i];
      atomicMin(&keys[(size_t)pair * nq + j], key);
    }
  }
}

__global__ __launch_bounds__(256) void nn_unpack_kernel(const unsigned long long* __restrict__ keys, size_t total1,
                                                        size_t total, float* __restrict__ dist1,
                                                        int* __restrict__ idx1, float* __restrict__ dist2,
                                                        int* __restrict__ idx2) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const unsigned long long k = keys[e];
  const float d = __uint_as_float((unsigned)(k >> 32));
  const int i = (int)(unsigned)(k & 0xffffffffu);
  if (e < total1) {
    dist1[e] = d;
    idx1[e] = i;
  } else {
    dist2[e - total1] = d;
    idx2[e - total1] = i;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// approximate match
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void emd_init_kernel(float* __restrict__ remL, float* __restrict__ remR,
                                                       double* __restrict__ costK, size_t bn, size_t bm,
                                                       float multL, float multR) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e < bn) {
    remL[e] = multL;
    costK[e] = 0.0;
  } else if (e < bn + bm) {
    remR[e - bn] = multR;
  }
}

// PASS 1: owners k (xyz1), loop l: ratioL[k] = remainL[k] / (sum_l E remainR[l] + 1e-9)
// PASS 2: owners l (xyz2), loop k: s = remainR[l] sum_k E ratioL[k]; ratioR, remainR
// PASS 3: owners k (xyz1), loop l: w = E ratioL[k] ratioR[l]; match[l][k] += w; remainL[k] -= sum_l w;
//         COST: costK[k] += sum_l w sqrt(d2)
template <int PASS, bool MATCH, bool COST>
__global__ __launch_bounds__(kEmdOwners* kEmdMaxWaves) void emd_pass_kernel(
    const float* __restrict__ xyz1, const float* __restrict__ xyz2, int n, int m, float scale,
    float* __restrict__ remL, float* __restrict__ remR, float* __restrict__ ratL, float* __restrict__ ratR,
    double* __restrict__ costK, float* __restrict__ match, int first) {
  __shared__ float red[kEmdMaxWaves][kEmdOwners];
  __shared__ float cred[COST ? kEmdMaxWaves : 1][kEmdOwners];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int S = blockDim.x >> 6;
  const int pair = blockIdx.y;
  const int no = PASS == 2 ? m : n, nl = PASS == 2 ? n : m;
  const int o = blockIdx.x * kEmdOwners + lane;
  const int oc = min(o, no - 1);
  const float* op = (PASS == 2 ? xyz2 + (size_t)pair * m * 3 : xyz1 + (size_t)pair * n * 3) + 3 * (size_t)oc;
  const float* lp = PASS == 2 ? xyz1 + (size_t)pair * n * 3 : xyz2 + (size_t)pair * m * 3;
  const float* lw = PASS == 1 ? remR + (size_t)pair * m : PASS == 2 ? ratL + (size_t)pair * n : ratR + (size_t)pair * m;
  const float ox = op[0], oy = op[1], oz = op[2];
  const float rl = PASS == 3 ? ratL[(size_t)pair * n + oc] : 0.f;
  const int per = (nl + S - 1) / S;
  const int l0 = wave * per, l1 = min(nl, l0 + per);
  float* mrow = match + (size_t)pair * m * n + o;
  const bool own = o < no;
  float acc = 0.f, cacc = 0.f;
#pragma unroll 8
  for (int l = l0; l < l1; ++l) {   // l is wave-uniform: the loop side arrives by scalar loads
    const float dx = lp[3 * l] - ox, dy = lp[3 * l + 1] - oy, dz = lp[3 * l + 2] - oz;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    const float e = __builtin_amdgcn_exp2f(d2 * scale);
    if (PASS != 3) {
      acc += e * lw[l];
    } else {
      const float w = e * rl * lw[l];
      acc += w;
      if (COST) cacc += w * __builtin_amdgcn_sqrtf(d2);
      if (MATCH && own) {
        float* p = mrow + (size_t)l * n;
        *p = first ? w : *p + w;
      }
    }
  }
  red[wave][lane] = acc;
  if (COST) cred[wave][lane] = cacc;
  __syncthreads();
  if (wave != 0 || !own) return;
  float sum = 0.f;
  for (int s = 0; s < S; ++s) sum += red[s][lane];
  const size_t gi = (size_t)pair * no + o;
  if (PASS == 1) {
    ratL[gi] = remL[gi] / (sum + 1e-9f);
  } else if (PASS == 2) {
    const float rr = remR[gi];
    const float s = rr * sum;
    ratR[gi] = fminf(rr / (s + 1e-9f), 1.0f) * rr;
    remR[gi] = fmaxf(0.0f, rr - s);
  } else {
    remL[gi] = fmaxf(0.0f, remL[gi] - sum);
    if (COST) {
      double c = 0.0;
      for (int s = 0; s < S; ++s) c += (double)cred[s][lane];
      costK[gi] += c;
    }
  }
}

// out[row] = sum of in[row][0..len) in a fixed order (lane-strided partial sums, then a fixed tree)
__global__ __launch_bounds__(256) void sum_rows_kernel(const double* __restrict__ in, int len, float* __restrict__ out) {
  __shared__ double buf[256];
  const double* p = in + (size_t)blockIdx.x * len;
  double acc = 0.0;
  for (int i = threadIdx.x; i < len; i += 256) acc += p[i];
  buf[threadIdx.x] = acc;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) buf[threadIdx.x] += buf[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = (float)buf[0];
}

// part[pair][tile] = sum over rows l of the tile, all k, of sqrt(d2(l, k)) * match[l][k]
__global__ __launch_bounds__(256) void match_cost_kernel(const float* __restrict__ xyz1, const float* __restrict__ xyz2,
                                                         const float* __restrict__ match, int n, int m,
                                                         double* __restrict__ part) {
  __shared__ double buf[256];
  const int pair = blockIdx.y, tiles = gridDim.x;
  const float* x1 = xyz1 + (size_t)pair * n * 3;
  const float* x2 = xyz2 + (size_t)pair * m * 3;
  const float* mt = match + (size_t)pair * m * n;
  const int l0 = blockIdx.x * kCostRows, l1 = min(m, l0 + kCostRows);
  double acc = 0.0;
  for (int l = l0; l < l1; ++l) {
    const float ax = x2[3 * l], ay = x2[3 * l + 1], az = x2[3 * l + 2];
    float a = 0.f;
    for (int k = threadIdx.x; k < n; k += 256) {
      const float dx = ax - x1[3 * k], dy = ay - x1[3 * k + 1], dz = az - x1[3 * k + 2];
      a += __builtin_amdgcn_sqrtf((dx * dx + dy * dy) + dz * dz) * mt[(size_t)l * n + k];
    }
    acc += (double)a;
  }
  buf[threadIdx.x] = acc;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) buf[threadIdx.x] += buf[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[(size_t)pair * tiles + blockIdx.x] = buf[0];
}

template <bool MATCH, bool COST>
hipError_t emd_levels(const float* xyz1, const float* xyz2, int b, int n, int m, const EmdWs& w, float* match,
                      hipStream_t st) {
  // integer division, as the reference op
  const float multL = n >= m ? 1.f : (float)(m / n);
  const float multR = n >= m ? (float)(n / m) : 1.f;
  const size_t bn = (size_t)b * n, bm = (size_t)b * m;
  emd_init_kernel<<<(unsigned)((bn + bm + 255) / 256), 256, 0, st>>>(w.remL, w.remR, w.costK, bn, bm, multL, multR);
  const dim3 gk(cdiv(n, kEmdOwners), b), gl(cdiv(m, kEmdOwners), b);
  const int tk = kEmdOwners * emd_waves(m), tl = kEmdOwners * emd_waves(n);
  const float log2e = 1.44269504088896341f;
  for (int j = 7; j >= -2; --j) {
    const float level = j == -2 ? 0.f : -powf(4.0f, (float)j);
    const float scale = level * log2e;
    emd_pass_kernel<1, MATCH, COST><<<gk, tk, 0, st>>>(xyz1, xyz2, n, m, scale, w.remL, w.remR, w.ratL, w.ratR,
                                                        w.costK, match, 0);
    emd_pass_kernel<2, MATCH, COST><<<gl, tl, 0, st>>>(xyz1, xyz2, n, m, scale, w.remL, w.remR, w.ratL, w.ratR,
                                                        w.costK, match, 0);
    emd_pass_kernel<3, MATCH, COST><<<gk, tk, 0, st>>>(xyz1, xyz2, n, m, scale, w.remL, w.remR, w.ratL, w.ratR,
                                                        w.costK, match, j == 7);
  }
  return hipGetLastError();
}

}  // namespace

static size_t metrics_ws_bytes(int b, int n, int m) {
  const size_t nn = align256((size_t)b * ((size_t)n + m) * 8);
  const size_t emd = emd_layout(nullptr, b, n, m).total;
  const size_t mc = align256((size_t)b * cdiv(m, kCostRows) * 8);
  size_t t = nn > emd ? nn : emd;
  return t > mc ? t : mc;
}

static hipError_t nn_distance_launch(const float* xyz1, const float* xyz2, int b, int n, int m, float* dist1,
                                     int* idx1, float* dist2, int* idx2, void* ws, hipStream_t st) {
  unsigned long long* keys = static_cast<unsigned long long*>(ws);
  const size_t total1 = (size_t)b * n, total = total1 + (size_t)b * m;
  hipError_t e = hipMemsetAsync(keys, 0xff, total * 8, st);
  if (e != hipSuccess) return e;
  const NnPlan p1 = nn_plan(b, n, m), p2 = nn_plan(b, m, n);
  nn_kernel<<<dim3(p1.qblocks * p1.splits, b), kNnThreads, 0, st>>>(xyz1, xyz2, n, m, p1.qblocks, p1.chunk, keys);
  nn_kernel<<<dim3(p2.qblocks * p2.splits, b), kNnThreads, 0, st>>>(xyz2, xyz1, m, n, p2.qblocks, p2.chunk,
                                                                      keys + total1);
  nn_unpack_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(keys, total1, total, dist1, idx1, dist2, idx2);
  return hipGetLastError();
}

static hipError_t approx_match_launch(const float* xyz1, const float* xyz2, int b, int n, int m, float* match,
                                      void* ws, hipStream_t st) {
  return emd_levels<true, false>(xyz1, xyz2, b, n, m, emd_layout(ws, b, n, m), match, st);
}

static hipError_t emd_launch(const float* xyz1, const float* xyz2, int b, int n, int m, float* cost, void* ws,
                             hipStream_t st) {
  const EmdWs w = emd_layout(ws, b, n, m);
  hipError_t e = emd_levels<false, true>(xyz1, xyz2, b, n, m, w, nullptr, st);
  if (e != hipSuccess) return e;
  sum_rows_kernel<<<b, 256, 0, st>>>(w.costK, n, cost);
  return hipGetLastError();
}

static hipError_t match_cost_launch(const float* xyz1, const float* xyz2, const float* match, int b, int n, int m,
                                    float* cost, void* ws, hipStream_t st) {
  double* part = static_cast<double*>(ws);
  const int tiles = cdiv(m, kCostRows);
  match_cost_kernel<<<dim3(tiles, b), 256, 0, st>>>(xyz1, xyz2, match, n, m, part);
  sum_rows_kernel<<<b, 256, 0, st>>>(part, tiles, cost);
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

static int metrics_shape(int b, int n, int m) {
  if (b < 1 || n < 1 || m < 1) return DISN_E_ARG;
  if (b > 65535) return DISN_E_SHAPE;  // one grid row per pair
  if (!fits_int(b, n, 3) || !fits_int(b, m, 3)) return DISN_E_SHAPE;  // xyz1 [b,n,3], xyz2 [b,m,3]
  return 0;
}

size_t disn_metrics_workspace_bytes(int b, int n, int m) {
  // b > 65535 is the entries' DISN_E_SHAPE, not the query's
  return (b < 1 || n < 1 || m < 1 || !fits_int(b, n, 3) || !fits_int(b, m, 3)) ? 0 : metrics_ws_bytes(b, n, m);
}

int disn_nn_distance(const float* xyz1, const float* xyz2, int b, int n, int m, float* dist1, int32_t* idx1,
                     float* dist2, int32_t* idx2, void* ws, size_t ws_bytes, void* stream) {
  if (!xyz1 || !xyz2 || !dist1 || !idx1 || !dist2 || !idx2 || !ws) return DISN_E_ARG;
  if (int rc = metrics_shape(b, n, m)) return rc;
  if (ws_bytes < metrics_ws_bytes(b, n, m)) return DISN_E_WS;
  DISN_TRY(nn_distance_launch(xyz1, xyz2, b, n, m, dist1, idx1, dist2, idx2, ws, (hipStream_t)stream));
  return 0;
}

int disn_approx_match(const float* xyz1, const float* xyz2, int b, int n, int m, float* match, void* ws,
                      size_t ws_bytes, void* stream) {
  if (!xyz1 || !xyz2 || !match || !ws) return DISN_E_ARG;
  if (int rc = metrics_shape(b, n, m)) return rc;
  if (ws_bytes < metrics_ws_bytes(b, n, m)) return DISN_E_WS;
  DISN_TRY(approx_match_launch(xyz1, xyz2, b, n, m, match, ws, (hipStream_t)stream));
  return 0;
}

int disn_match_cost(const float* xyz1, const float* xyz2, const float* match, int b, int n, int m, float* cost,
                    void* ws, size_t ws_bytes, void* stream) {
  if (!xyz1 || !xyz2 || !match || !cost || !ws) return DISN_E_ARG;
  if (int rc = metrics_shape(b, n, m)) return rc;
  if (ws_bytes < metrics_ws_bytes(b, n, m)) return DISN_E_WS;
  DISN_TRY(match_cost_launch(xyz1, xyz2, match, b, n, m, cost, ws, (hipStream_t)stream));
  return 0;
}

int disn_emd(const float* xyz1, const float* xyz2, int b, int n, int m, float* cost, void* ws, size_t ws_bytes,
             void* stream) {
  if (!xyz1 || !xyz2 || !cost || !ws) return DISN_E_ARG;
  if (int rc = metrics_shape(b, n, m)) return rc;
  if (ws_bytes < metrics_ws_bytes(b, n, m)) return DISN_E_WS;
  DISN_TRY(emd_launch(xyz1, xyz2, b, n, m, cost, ws, (hipStream_t)stream));
  return 0;
}

}  // extern "C"

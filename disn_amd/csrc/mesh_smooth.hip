// Taubin lambda|mu smoothing of meshes on the device (include/disn_amd_smooth.h; the rule is disn_amd/postprocess.py
// smooth_arrays, restated here operation by operation): B meshes back to back, as disn_mc_emit_batch,
// disn_mesh_clean_emit_batch and disn_mesh_simplify_emit_batch leave them.  The faces never change.
//
//   build    validate indices and coordinates, status 7 for a coordinate beyond +-1024 -> every face claims the slots of
//            its (up to) three undirected edges, keyed by batch-global vertex ids (lo << 32 | hi), and counts the
//            claim in the slot; the thread that claimed a slot first adds 1 to the degree of both ends -> ONE scan of
//            the degrees: the CSR offsets -> one thread per slot writes each end into the other's row (a cursor per
//            row; the order inside a row is arbitrary, the sums are integers) and marks both ends of an edge counted
//            once as boundary
//   iterate  one kernel per step, one thread per vertex: gather q = rint(x 2^32) over the row in int64, update, cap,
//            range check, write the OTHER position buffer.  No atomic: a range violation is a plain store of the one
//            value 7 to the mesh's status word
//   finish   out_verts = the last buffer, or the INPUT vertices for a mesh with a status
//
// NO KERNEL WAITS FOR ANOTHER WORKGROUP.  The only loop whose trip count depends on other threads is the probe of
// table_claim: at most `mask + 1` steps; a full table raises status 3 (the table has two slots per possible edge).
// NO FLOATING-POINT ATOMIC.  No host synchronisation and no read-back.  A mesh with a status is skipped by every later
// kernel.  Compiled with -ffp-contract=off: the float64 arithmetic rounds as numpy's does.
// (mesh_of, table_claim, the two validators and the host-side helpers are those of mesh_batch.hpp.)
#include "mesh_batch.hpp"

#include "../../include/disn_amd_smooth.h"

namespace disn {
namespace {

enum { ST_RANGE = DISN_SMOOTH_RANGE };         // this stage's own status
constexpr double kFix = 4294967296.0;          // 2^32
constexpr float kRange = 1024.0f;
constexpr unsigned kMaxDegree = 1u << 20;

// status 7 for a mesh with a finite coordinate beyond +-1024 (one that is not finite is validate_verts_kernel's)
__global__ __launch_bounds__(kThreads) void range_kernel(const float* __restrict__ verts,
                                                         const long long* __restrict__ voff, int B, long long nv,
                                                         int* status) {
  GRID_STRIDE(v, nv) {
    bool bad = false;
    for (int k = 0; k < 3; ++k) {
      const float a = fabsf(verts[3 * v + k]);
      bad |= a > kRange && a <= 3.4028234663852886e38f;
    }
    if (bad) atomicMax(&status[mesh_of(voff, B, v)], (int)ST_RANGE);
  }
}

// every face claims its edges; held[slot] = the corner pairs that hold the edge, deg[v] = the distinct edges at v
__global__ __launch_bounds__(kThreads) void edge_claim_kernel(const int* __restrict__ faces,
                                                              const long long* __restrict__ voff,
                                                              const long long* __restrict__ foff, int B, long long nf,
                                                              int* status, unsigned long long* keys,
                                                              unsigned long long mask, unsigned* held, unsigned* deg) {
  GRID_STRIDE(f, nf) {
    const int b = mesh_of(foff, B, f);
    if (status[b]) continue;                                   // so every index below lies in [0, nv_b)
    const long long v0 = voff[b];
    const int c[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
    for (int k = 0; k < 3; ++k) {
      const int i = c[k], j = c[k == 2 ? 0 : k + 1];
      if (i == j) continue;
      const unsigned long long lo = (unsigned long long)(v0 + (i < j ? i : j));
      const unsigned long long hi = (unsigned long long)(v0 + (i < j ? j : i));     // < 2^31: the key is never kEmptyKey
      bool is_new = false;
      const long long s = table_claim(keys, mask, lo << 32 | hi, &is_new);
      if (s < 0) { atomicMax(&status[b], (int)ST_TABLE); continue; }
      atomicAdd(&held[s], 1u);
      if (is_new) {
        atomicAdd(&deg[lo], 1u);
        atomicAdd(&deg[hi], 1u);
      }
    }
  }
}

// status 7 for a mesh with a vertex of more than 2^20 neighbours
__global__ __launch_bounds__(kThreads) void degree_kernel(const long long* __restrict__ voff, int B, long long nv,
                                                          const unsigned* __restrict__ deg, int* status) {
  GRID_STRIDE(v, nv) {
    if (deg[v] > kMaxDegree) atomicMax(&status[mesh_of(voff, B, v)], (int)ST_RANGE);
  }
}

// one thread per slot: each end into the other's row, and the boundary marks (a plain store of the one value 1)
__global__ __launch_bounds__(kThreads) void edge_fill_kernel(const unsigned long long* __restrict__ keys,
                                                             const unsigned* __restrict__ held, long long slots,
                                                             long long nv, const unsigned* __restrict__ deg,
                                                             const unsigned* __restrict__ row, unsigned* cursor,
                                                             unsigned* __restrict__ nbr, unsigned long long nnz,
                                                             unsigned char* boundary) {
  GRID_STRIDE(s, slots) {
    const unsigned long long key = keys[s];
    if (key == kEmptyKey) continue;
    const unsigned end[2] = {(unsigned)(key >> 32), (unsigned)(key & 0xFFFFFFFFull)};
    if ((long long)end[0] >= nv || (long long)end[1] >= nv) continue;     // (every key was made of checked ids)
    for (int k = 0; k < 2; ++k) {
      const unsigned at = atomicAdd(&cursor[end[k]], 1u);
      const unsigned long long e = (unsigned long long)row[end[k]] + at;
      if (at < deg[end[k]] && e < nnz) nbr[e] = end[1 - k];
    }
    if (held[s] == 1u) {
      boundary[end[0]] = 1;
      boundary[end[1]] = 1;
    }
  }
}

__device__ __forceinline__ long long fixed_of(float x) { return (long long)rint((double)x * kFix); }

// step t: dst = the rule's v' from src (for t = 0 the input); an unmovable vertex takes its input bits
__global__ __launch_bounds__(kThreads) void step_kernel(const float* __restrict__ verts, const float* __restrict__ src,
                                                        float* __restrict__ dst, const long long* __restrict__ voff,
                                                        int B, long long nv, int* status,
                                                        const unsigned* __restrict__ deg,
                                                        const unsigned* __restrict__ row,
                                                        const unsigned* __restrict__ nbr, unsigned long long nnz,
                                                        const unsigned char* __restrict__ boundary, int pin, double s,
                                                        const double* __restrict__ cap) {
  GRID_STRIDE(v, nv) {
    const int b = mesh_of(voff, B, v);
    if (status[b]) continue;
    const unsigned d = deg[v];
    if (d == 0 || (pin && boundary[v])) {
      const unsigned* in = reinterpret_cast<const unsigned*>(verts);
      unsigned* out = reinterpret_cast<unsigned*>(dst);
      for (int k = 0; k < 3; ++k) out[3 * v + k] = in[3 * v + k];
      continue;
    }
    long long S[3] = {0, 0, 0};
    const unsigned long long first = row[v];
    for (unsigned k = 0; k < d && first + k < nnz; ++k) {
      const long long j = nbr[first + k];
      if (j >= nv) continue;                                   // (every entry was written from checked ids)
      S[0] += fixed_of(src[3 * j]);
      S[1] += fixed_of(src[3 * j + 1]);
      S[2] += fixed_of(src[3 * j + 2]);
    }
    const double r = cap ? cap[b] : -1.0;
    bool bad = false;
    for (int k = 0; k < 3; ++k) {
      const double x = (double)src[3 * v + k];
      const double m = ((double)S[k] * (1.0 / kFix)) / (double)d;
      double y = x + s * (m - x);
      if (r >= 0.0) {
        const double x0 = (double)verts[3 * v + k];
        y = fmin(fmax(y, x0 - r), x0 + r);
      }
      const float out = (float)y;
      bad |= fabsf(out) > kRange;
      dst[3 * v + k] = out;
    }
    if (bad) status[b] = ST_RANGE;                             // the one value any thread stores here: no atomic
  }
}

__global__ __launch_bounds__(kThreads) void finish_kernel(const float* __restrict__ verts,
                                                          const float* __restrict__ last,
                                                          const long long* __restrict__ voff, int B, long long nv,
                                                          const int* __restrict__ status, float* __restrict__ out) {
  GRID_STRIDE(v, nv) {
    const unsigned* in = reinterpret_cast<const unsigned*>(status[mesh_of(voff, B, v)] ? verts : last);
    for (int k = 0; k < 3; ++k) reinterpret_cast<unsigned*>(out)[3 * v + k] = in[3 * v + k];
  }
}

// ---- host side -------------------------------------------------------------------------------------------------
struct SmoothWs {
  long long *voff, *foff;                          // [B+1] each
  double* cap;                                     // [B]
  unsigned *deg, *cursor;                          // [nv]   zeroed block starts here
  unsigned char* boundary;                         // [nv]
  unsigned* held;                                  // [T]    zeroed block ends behind it
  size_t zero_bytes;
  unsigned long long* keys;                        // [T]
  unsigned long long T;
  unsigned* row;                                   // [nv]   the CSR offsets
  unsigned long long* total;                       // [1]
  unsigned* bsum;
  unsigned* nbr;                                   // [6 nf] two entries per possible edge
  float *pos[2];                                   // [3 nv] each: the steps' two position buffers
  size_t total_bytes;
};

SmoothWs smooth_layout(void* ws, int B, long long nv, long long nf) {
  WsCursor c(ws);
  const size_t b1 = (size_t)B + 1, f = (size_t)(nf > 0 ? nf : 1), v = (size_t)(nv > 0 ? nv : 1);
  SmoothWs w;
  w.voff = c.take<long long>(b1); w.foff = c.take<long long>(b1);
  w.cap = c.take<double>(b1);
  unsigned long long T = 16;
  while (T < 6ull * f) T <<= 1;                    // at most 3 nf edges: at most half full
  w.T = T;
  const size_t z0 = c.next();
  w.deg = c.take<unsigned>(v); w.cursor = c.take<unsigned>(v);
  w.boundary = c.take<unsigned char>(v);
  w.held = c.take<unsigned>(T);
  w.zero_bytes = c.off - z0;
  w.keys = c.take<unsigned long long>(T);
  w.row = c.take<unsigned>(v);
  w.total = c.take<unsigned long long>(1);
  w.bsum = c.take<unsigned>(scan_bsum_items(v));
  w.nbr = c.take<unsigned>(6 * f);
  w.pos[0] = c.take<float>(3 * v); w.pos[1] = c.take<float>(3 * v);
  w.total_bytes = c.next();
  return w;
}

}  // namespace
}  // namespace disn

using namespace disn;

extern "C" size_t disn_mesh_smooth_workspace_bytes(int B, int64_t nv_total, int64_t nf_total) {
  return mesh_limits_ok(B, nv_total, nf_total) ? smooth_layout(nullptr, B, nv_total, nf_total).total_bytes : 0;
}

extern "C" int disn_mesh_smooth_batch(const float* verts, const int32_t* faces, const int64_t* v_off_host,
                                      const int64_t* f_off_host, int B, int iters, double lam, double mu,
                                      int pin_boundary, const double* max_move_host, float* out_verts,
                                      int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  if (!offsets_ok(v_off_host, f_off_host, B) || !status || !ws) return DISN_E_ARG;
  const int64_t nv = v_off_host[B], nf = f_off_host[B];
  if ((nv > 0 && (!verts || !out_verts)) || (nf > 0 && !faces)) return DISN_E_ARG;
  if (iters < 1 || iters > DISN_SMOOTH_MAX_ITERS || !(lam > 0.0 && lam <= 1.0) || !(mu >= -1.5 && mu < 0.0))
    return DISN_E_ARG;
  if (max_move_host)
    for (int b = 0; b < B; ++b)
      if (!(max_move_host[b] < 0.0) && !(max_move_host[b] <= 1.7976931348623157e308)) return DISN_E_ARG;
  if (!mesh_limits_ok(B, nv, nf)) return DISN_E_SHAPE;
  if (ws_bytes < smooth_layout(nullptr, B, nv, nf).total_bytes) return DISN_E_WS;
  hipStream_t st = (hipStream_t)stream;
  const SmoothWs w = smooth_layout(ws, B, nv, nf);
  MESH_TRY(upload_offsets(w.voff, w.foff, v_off_host, f_off_host, B, st));
  if (max_move_host) MESH_TRY(hipMemcpyAsync(w.cap, max_move_host, (size_t)B * 8, hipMemcpyHostToDevice, st));
  MESH_TRY(hipMemsetAsync(status, 0, (size_t)B * 4, st));
  if (nf > 0) MESH_LAUNCH(validate_faces_kernel, nf, faces, w.voff, w.foff, B, nf, status);
  if (nv == 0) return 0;
  MESH_LAUNCH(validate_verts_kernel, nv, verts, w.voff, B, nv, status);
  MESH_LAUNCH(range_kernel, nv, verts, w.voff, B, nv, status);
  MESH_TRY(hipMemsetAsync(w.deg, 0, w.zero_bytes, st));
  const unsigned long long nnz = 6ull * (unsigned long long)(nf > 0 ? nf : 1);
  if (nf > 0) {
    MESH_TRY(hipMemsetAsync(w.keys, 0xFF, w.T * 8, st));
    MESH_LAUNCH(edge_claim_kernel, nf, faces, w.voff, w.foff, B, nf, status, w.keys, w.T - 1, w.held, w.deg);
    MESH_LAUNCH(degree_kernel, nv, w.voff, B, nv, w.deg, status);
  }
  MESH_TRY(exclusive_scan(w.deg, w.row, (size_t)nv, w.bsum, w.total, st));
  if (nf > 0)
    MESH_LAUNCH(edge_fill_kernel, (long long)w.T, w.keys, w.held, (long long)w.T, nv, w.deg, w.row, w.cursor, w.nbr, nnz,
                w.boundary);
  const double* cap = max_move_host ? w.cap : nullptr;
  const float* src = verts;
  for (int t = 0; t < 2 * iters; ++t) {
    float* dst = w.pos[t & 1];
    MESH_LAUNCH(step_kernel, nv, verts, src, dst, w.voff, B, nv, status, w.deg, w.row, w.nbr, nnz, w.boundary,
                pin_boundary ? 1 : 0, (t & 1) ? mu : lam, cap);
    src = dst;
  }
  MESH_LAUNCH(finish_kernel, nv, verts, src, w.voff, B, nv, status, out_verts);
  return 0;
}

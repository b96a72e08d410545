// Mesh simplification by quadric vertex clustering on the device (include/disn_amd_simplify.h; the rule is
// disn_amd/postprocess.py simplify_arrays, restated here operation by operation): B meshes back to back, as
// disn_mc_emit_batch and disn_mesh_clean_emit_batch leave them, each on a lattice of its own.
//
//   count   validate indices and coordinates -> every vertex claims the slot of its (mesh, cell) key and atomicMin's
//           its index into the slot: a cluster's smallest member -> flags at those members, ONE scan: the clusters'
//           numbers through the batch, in the order of their smallest members -> every vertex adds its position in the
//           cell and 1 to its cluster, every face its quadric to each of its distinct clusters -> a face with three
//           distinct clusters claims the slot of its sorted triple and atomicMin's its index -> flags at the smallest
//           face of every triple, one scan -> [B,4] sizes
//   emit    one thread per cluster solves for its position; the surviving faces, vmap and first are written in order
//
// NO KERNEL WAITS FOR ANOTHER WORKGROUP.  The only loop whose trip count depends on other threads is the probe of
// table_claim: an index that advances once per step, at most `mask + 1` steps; a full table raises status 3.
// NO FLOATING-POINT ATOMIC: every real that is summed has magnitude <= 1 and is added as rint(x 2^32) to an int64 with a
// 64-bit integer atomic add, so the sums, and with them every output bit, do not depend on the order of execution.
// Compiled with -ffp-contract=off: the float32 cell and the float64 arithmetic round as numpy's do.
// (mesh_of, the tables, the two validators and the host-side helpers are those of mesh_batch.hpp.)
#include "mesh_batch.hpp"

#include "../../include/disn_amd_simplify.h"

namespace disn {
namespace {

constexpr int kAcc = 14;                       // per cluster: 10 quadric entries, 3 sums of rel, the member count
constexpr unsigned kTripleLimit = 1u << 21;    // cluster numbers a face key holds: 3 x 21 bits (status 5 beyond)
constexpr double kFix = 4294967296.0;          // 2^32
enum { ST_CAPACITY = 5 };

struct Lattice {
  double ox, oy, oz, h;
};

// simplify_arrays' cell: float32, floor, then the clamp (so every finite vertex has a cell)
__device__ __forceinline__ int cell_axis(float v, double origin, float inv_h, int cells) {
  const float c = floorf((v - (float)origin) * inv_h);
  return (int)fminf(fmaxf(c, 0.0f), (float)(cells - 1));
}

struct Cell {
  int x, y, z;
};

__device__ __forceinline__ Cell cell_of(const float* __restrict__ verts, long long gv, const Lattice& L, int cells) {
  const float inv_h = (float)(1.0 / L.h);
  Cell c;
  c.x = cell_axis(verts[3 * gv], L.ox, inv_h, cells);
  c.y = cell_axis(verts[3 * gv + 1], L.oy, inv_h, cells);
  c.z = cell_axis(verts[3 * gv + 2], L.oz, inv_h, cells);
  return c;
}

__device__ __forceinline__ double centre_axis(double origin, int c, double h) { return origin + ((double)c + 0.5) * h; }

// rel = clip((v - centre) / h, -1/2, 1/2) per axis, in float64
__device__ __forceinline__ void rel_of(const float* __restrict__ verts, long long gv, const Lattice& L, int cells,
                                       double r[3]) {
  const Cell c = cell_of(verts, gv, L, cells);
  r[0] = fmin(fmax(((double)verts[3 * gv] - centre_axis(L.ox, c.x, L.h)) / L.h, -0.5), 0.5);
  r[1] = fmin(fmax(((double)verts[3 * gv + 1] - centre_axis(L.oy, c.y, L.h)) / L.h, -0.5), 0.5);
  r[2] = fmin(fmax(((double)verts[3 * gv + 2] - centre_axis(L.oz, c.z, L.h)) / L.h, -0.5), 0.5);
}

__device__ __forceinline__ void add_fixed(long long* acc, double x) {
  atomicAdd(reinterpret_cast<unsigned long long*>(acc), (unsigned long long)(long long)rint(x * kFix));
}

// every vertex claims its (mesh, cell) key -- cell < 2^30, the mesh above it -- and lowers the slot's smallest member
__global__ __launch_bounds__(kThreads) void vertex_claim_kernel(const float* __restrict__ verts,
                                                                const long long* __restrict__ voff, int B,
                                                                long long nv, const Lattice* __restrict__ lat,
                                                                const int* __restrict__ cells, int* status,
                                                                unsigned long long* keys, unsigned long long mask,
                                                                int* vfirst, unsigned* __restrict__ vslot) {
  GRID_STRIDE(v, nv) {
    const int b = mesh_of(voff, B, v);
    vslot[v] = kNone;
    if (status[b]) continue;
    const int n = cells[b];
    const Cell c = cell_of(verts, v, lat[b], n);
    const unsigned long long cell = ((unsigned long long)c.x * n + c.y) * n + c.z;
    const long long s = table_claim(keys, mask, (unsigned long long)b << 30 | cell);
    if (s < 0) { atomicMax(&status[b], (int)ST_TABLE); continue; }
    vslot[v] = (unsigned)s;
    atomicMin(&vfirst[s], (int)v);
  }
}

// a flag at every cluster's smallest member (a mesh with a status has none) and the mesh's number of clusters
__global__ __launch_bounds__(kThreads) void vertex_flag_kernel(const long long* __restrict__ voff, int B, long long nv,
                                                               const int* __restrict__ status,
                                                               const int* __restrict__ vfirst,
                                                               const unsigned* __restrict__ vslot,
                                                               unsigned* __restrict__ vflag,
                                                               unsigned long long* meshcnt) {
  GRID_STRIDE(v, nv) {
    const int b = mesh_of(voff, B, v);
    const bool is_first = !status[b] && vslot[v] != kNone && vfirst[vslot[v]] == (int)v;
    vflag[v] = is_first ? 1u : 0u;
    if (is_first) atomicAdd(&meshcnt[3 * b], 1ull);
  }
}

// cbase[b] = the number of mesh b's first cluster through the batch, cbase[B] = all clusters
__global__ void cluster_base_kernel(const long long* __restrict__ voff, int B, long long nv,
                                    const unsigned* __restrict__ vscan,
                                    const unsigned long long* __restrict__ total, unsigned* __restrict__ cbase) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b > B) return;
  cbase[b] = (b < B && voff[b] < nv) ? vscan[voff[b]] : (unsigned)*total;
}

// vclu[v] = the vertex's cluster (numbered through the batch); its rel and 1 go to the cluster's sums
__global__ __launch_bounds__(kThreads) void vertex_accum_kernel(const float* __restrict__ verts,
                                                                const long long* __restrict__ voff, int B,
                                                                long long nv, const Lattice* __restrict__ lat,
                                                                const int* __restrict__ cells,
                                                                const int* __restrict__ status,
                                                                const int* __restrict__ vfirst,
                                                                const unsigned* __restrict__ vslot,
                                                                const unsigned* __restrict__ vscan,
                                                                unsigned* __restrict__ vclu, long long* acc) {
  GRID_STRIDE(v, nv) {
    const int b = mesh_of(voff, B, v);
    vclu[v] = kNone;
    if (status[b] || vslot[v] == kNone) continue;
    const unsigned c = vscan[vfirst[vslot[v]]];
    vclu[v] = c;
    double r[3];
    rel_of(verts, v, lat[b], cells[b], r);
    long long* a = acc + (size_t)kAcc * c;
    for (int k = 0; k < 3; ++k) add_fixed(a + 10 + k, r[k]);
    atomicAdd(reinterpret_cast<unsigned long long*>(a + 13), 1ull);
  }
}

// a face's quadric, once to each of its distinct clusters; a face with three distinct clusters claims its triple
__global__ __launch_bounds__(kThreads) void face_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                        const long long* __restrict__ voff,
                                                        const long long* __restrict__ foff, int B, long long nf,
                                                        const Lattice* __restrict__ lat, const int* __restrict__ cells,
                                                        int dedup, int* status, const unsigned* __restrict__ vclu,
                                                        long long* acc, unsigned long long* keys,
                                                        unsigned long long mask, int* fmin_,
                                                        unsigned* __restrict__ fslot, unsigned long long* meshcnt) {
  GRID_STRIDE(f, nf) {
    const int b = mesh_of(foff, B, f);
    fslot[f] = kNone;
    if (status[b]) continue;
    long long gv[3];
    unsigned g[3];
    for (int k = 0; k < 3; ++k) {
      gv[k] = voff[b] + faces[3 * f + k];
      g[k] = vclu[gv[k]];
    }
    if (g[0] == kNone || g[1] == kNone || g[2] == kNone) continue;      // (a vertex table that filled: status 3 is set)
    const Lattice L = lat[b];
    double p[3][3];
    for (int k = 0; k < 3; ++k)
      for (int j = 0; j < 3; ++j) p[k][j] = (double)verts[3 * gv[k] + j];
    const double ux = p[1][0] - p[0][0], uy = p[1][1] - p[0][1], uz = p[1][2] - p[0][2];
    const double wx = p[2][0] - p[0][0], wy = p[2][1] - p[0][1], wz = p[2][2] - p[0][2];
    const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
    const double ln = sqrt((nx * nx + ny * ny) + nz * nz);
    if (ln > 0.0 && ln <= 1.7976931348623157e308) {                     // |n| = 0 or not finite: no contribution
      double q[4] = {nx / ln, ny / ln, nz / ln, 0.0};
      const double w = fmin(ln / (L.h * L.h), 1.0);
      for (int k = 0; k < 3; ++k) {
        bool fresh = true;
        for (int j = 0; j < k; ++j) fresh &= g[k] != g[j];
        if (!fresh) continue;
        double r[3];
        rel_of(verts, gv[k], L, cells[b], r);
        q[3] = -((q[0] * r[0] + q[1] * r[1]) + q[2] * r[2]);
        long long* a = acc + (size_t)kAcc * g[k];
        int e = 0;
        for (int i = 0; i < 4; ++i)
          for (int j = i; j < 4; ++j) add_fixed(a + e++, (w * q[i]) * q[j]);
      }
    }
    if (g[0] == g[1] || g[1] == g[2] || g[0] == g[2]) continue;         // collapsed
    atomicAdd(&meshcnt[3 * b + 2], 1ull);
    if (!dedup) { fslot[f] = 0u; continue; }
    unsigned lo = g[0], mid = g[1], hi = g[2], t;
    if (lo > mid) { t = lo; lo = mid; mid = t; }
    if (mid > hi) { t = mid; mid = hi; hi = t; }
    if (lo > mid) { t = lo; lo = mid; mid = t; }
    if (hi >= kTripleLimit) { atomicMax(&status[b], (int)ST_CAPACITY); continue; }
    const long long s = table_claim(keys, mask, (unsigned long long)lo << 42 | (unsigned long long)mid << 21 | hi);
    if (s < 0) { atomicMax(&status[b], (int)ST_TABLE); continue; }
    fslot[f] = (unsigned)s;
    atomicMin(&fmin_[s], (int)f);
  }
}

// a flag at every surviving face and the mesh's number of them
__global__ __launch_bounds__(kThreads) void face_flag_kernel(const long long* __restrict__ foff, int B, long long nf,
                                                             int dedup, const int* __restrict__ status,
                                                             const int* __restrict__ fmin_,
                                                             const unsigned* __restrict__ fslot,
                                                             unsigned* __restrict__ fflag, unsigned long long* meshcnt) {
  GRID_STRIDE(f, nf) {
    const int b = mesh_of(foff, B, f);
    const bool keep = !status[b] && fslot[f] != kNone && (!dedup || fmin_[fslot[f]] == (int)f);
    fflag[f] = keep ? 1u : 0u;
    if (keep) atomicAdd(&meshcnt[3 * b + 1], 1ull);
  }
}

// the sizes, and where each mesh's vertices go in the outputs (B is a handful: one thread)
__global__ void finish_kernel(int B, const int* __restrict__ status, const unsigned long long* __restrict__ meshcnt,
                              long long* __restrict__ vseg, long long* __restrict__ counts) {
  if (blockIdx.x || threadIdx.x) return;
  long long v = 0;
  for (int b = 0; b < B; ++b) {
    const bool ok = status[b] == 0;
    vseg[b] = v;
    counts[4 * b + 0] = ok ? (long long)meshcnt[3 * b] : 0;
    counts[4 * b + 1] = ok ? (long long)meshcnt[3 * b + 1] : 0;
    counts[4 * b + 2] = ok ? (long long)(meshcnt[3 * b + 2] - meshcnt[3 * b + 1]) : 0;
    counts[4 * b + 3] = status[b];
    v += counts[4 * b];
  }
  vseg[B] = v;
}

// ---- emit ----------------------------------------------------------------------------------------------------
// one thread per cluster, at its smallest member: simplify_arrays' _simplify_solve in the same operation order
__global__ __launch_bounds__(kThreads) void solve_kernel(const float* __restrict__ verts,
                                                         const long long* __restrict__ voff, int B, long long nv,
                                                         const Lattice* __restrict__ lat, const int* __restrict__ cells,
                                                         const int* __restrict__ status,
                                                         const unsigned* __restrict__ vflag,
                                                         const unsigned* __restrict__ vclu,
                                                         const unsigned* __restrict__ cbase,
                                                         const long long* __restrict__ vseg,
                                                         const long long* __restrict__ acc, long long n_out,
                                                         float* __restrict__ out_verts, int* __restrict__ first) {
  GRID_STRIDE(v, nv) {
    if (!vflag[v]) continue;
    const int b = mesh_of(voff, B, v);
    if (status[b] || vclu[v] == kNone) continue;
    const long long pos = vseg[b] + ((long long)vclu[v] - (long long)cbase[b]);
    if (pos < 0 || pos >= n_out) continue;                  // (sizes the count did not leave: nothing is written)
    const long long* a = acc + (size_t)kAcc * vclu[v];
    double s[13];
    for (int k = 0; k < 13; ++k) s[k] = (double)a[k] * (1.0 / kFix);
    const double axx = s[0], axy = s[1], axz = s[2], bx = s[3], ayy = s[4], ayz = s[5], by = s[6], azz = s[7], bz = s[8];
    const double n = (double)a[13];
    const double mx = s[10] / n, my = s[11] / n, mz = s[12] / n;
    const double lam = (((axx + ayy) + azz) * 0.0009765625) / 3.0 + 9.094947017729282e-13;
    const double m00 = axx + lam, m11 = ayy + lam, m22 = azz + lam, m01 = axy, m02 = axz, m12 = ayz;
    const double r0 = lam * mx - bx, r1 = lam * my - by, r2 = lam * mz - bz;
    const double c00 = m11 * m22 - m12 * m12;
    const double c01 = m02 * m12 - m01 * m22;
    const double c02 = m01 * m12 - m02 * m11;
    const double c11 = m00 * m22 - m02 * m02;
    const double c12 = m01 * m02 - m00 * m12;
    const double c22 = m00 * m11 - m01 * m01;
    const double det = (m00 * c00 + m01 * c01) + m02 * c02;
    double x0 = ((c00 * r0 + c01 * r1) + c02 * r2) / det;
    double x1 = ((c01 * r0 + c11 * r1) + c12 * r2) / det;
    double x2 = ((c02 * r0 + c12 * r1) + c22 * r2) / det;
    const double big = 1.7976931348623157e308;
    const bool ok = det > 0.0 && fabs(x0) <= big && fabs(x1) <= big && fabs(x2) <= big;
    if (!ok) { x0 = mx; x1 = my; x2 = mz; }
    x0 = fmin(fmax(x0, -0.5), 0.5);
    x1 = fmin(fmax(x1, -0.5), 0.5);
    x2 = fmin(fmax(x2, -0.5), 0.5);
    const Lattice L = lat[b];
    const Cell c = cell_of(verts, v, L, cells[b]);
    out_verts[3 * pos] = (float)(centre_axis(L.ox, c.x, L.h) + L.h * x0);
    out_verts[3 * pos + 1] = (float)(centre_axis(L.oy, c.y, L.h) + L.h * x1);
    out_verts[3 * pos + 2] = (float)(centre_axis(L.oz, c.z, L.h) + L.h * x2);
    first[pos] = (int)(v - voff[b]);
  }
}

__global__ __launch_bounds__(kThreads) void emit_vmap_kernel(const long long* __restrict__ voff, int B, long long nv,
                                                             const int* __restrict__ status,
                                                             const unsigned* __restrict__ vclu,
                                                             const unsigned* __restrict__ cbase,
                                                             int* __restrict__ vmap) {
  GRID_STRIDE(v, nv) {
    const int b = mesh_of(voff, B, v);
    vmap[v] = (status[b] || vclu[v] == kNone) ? -1 : (int)(vclu[v] - cbase[b]);
  }
}

__global__ __launch_bounds__(kThreads) void emit_faces_kernel(const int* __restrict__ faces,
                                                              const long long* __restrict__ voff,
                                                              const long long* __restrict__ foff, int B, long long nf,
                                                              const unsigned* __restrict__ fflag,
                                                              const unsigned* __restrict__ fscan,
                                                              const unsigned* __restrict__ vclu,
                                                              const unsigned* __restrict__ cbase, long long n_out,
                                                              int* __restrict__ out_faces) {
  GRID_STRIDE(f, nf) {
    if (!fflag[f] || (long long)fscan[f] >= n_out) continue;          // (a flagged face passed every check of the count)
    const int b = mesh_of(foff, B, f);
    for (int k = 0; k < 3; ++k)
      out_faces[3 * (size_t)fscan[f] + k] = (int)(vclu[voff[b] + faces[3 * f + k]] - cbase[b]);
  }
}

// ---- host side -------------------------------------------------------------------------------------------------
struct SimplifyWs {
  long long *voff, *foff, *vseg;                   // [B+1] each
  Lattice* lat;                                    // [B]
  int* cells;                                      // [B]
  int* status;                                     // [B]    zeroed block starts here
  unsigned long long* meshcnt;                     // [3B]   clusters, surviving faces, faces with three distinct clusters
  unsigned long long* totals;                      // [2]    all clusters, all surviving faces
  long long* acc;                                  // [14 nv] zeroed block ends behind it
  size_t zero_bytes;
  unsigned* cbase;                                 // [B+1]
  unsigned *vslot, *vflag, *vscan, *vclu;          // [nv]
  unsigned *fslot, *fflag, *fscan;                 // [nf]
  unsigned long long *vkeys, *fkeys;               // [Tv], [Tf]
  int *vfirst, *fmin_;                             // [Tv], [Tf]
  unsigned long long Tv, Tf;
  unsigned* bsum;
  size_t total;
};

SimplifyWs simplify_layout(void* ws, int B, long long nv, long long nf) {
  WsCursor c(ws);
  const size_t b1 = (size_t)B + 1, f = (size_t)(nf > 0 ? nf : 1), v = (size_t)(nv > 0 ? nv : 1);
  SimplifyWs w;
  w.voff = c.take<long long>(b1); w.foff = c.take<long long>(b1); w.vseg = c.take<long long>(b1);
  w.lat = c.take<Lattice>(b1);
  w.cells = c.take<int>(b1);
  const size_t z0 = c.next();
  w.status = c.take<int>(b1);
  w.meshcnt = c.take<unsigned long long>(3 * b1);
  w.totals = c.take<unsigned long long>(2);
  w.acc = c.take<long long>(kAcc * v);
  w.zero_bytes = c.off - z0;
  w.cbase = c.take<unsigned>(b1);
  w.vslot = c.take<unsigned>(v); w.vflag = c.take<unsigned>(v);
  w.vscan = c.take<unsigned>(v); w.vclu = c.take<unsigned>(v);
  w.fslot = c.take<unsigned>(f); w.fflag = c.take<unsigned>(f); w.fscan = c.take<unsigned>(f);
  unsigned long long Tv = 16, Tf = 16;
  while (Tv < 2ull * v) Tv <<= 1;        // one entry per vertex / per face at most: at most half full
  while (Tf < 2ull * f) Tf <<= 1;
  w.Tv = Tv; w.Tf = Tf;
  w.vkeys = c.take<unsigned long long>(Tv); w.vfirst = c.take<int>(Tv);
  w.fkeys = c.take<unsigned long long>(Tf); w.fmin_ = c.take<int>(Tf);
  w.bsum = c.take<unsigned>(scan_bsum_items(f > v ? f : v));
  w.total = c.next();
  return w;
}

}  // namespace
}  // namespace disn

using namespace disn;

extern "C" size_t disn_mesh_simplify_workspace_bytes(int B, int64_t nv_total, int64_t nf_total) {
  return mesh_limits_ok(B, nv_total, nf_total) ? simplify_layout(nullptr, B, nv_total, nf_total).total : 0;
}

extern "C" int disn_mesh_simplify_count_batch(const float* verts, const int32_t* faces, const int64_t* v_off_host,
                                              const int64_t* f_off_host, const double* lattice_host,
                                              const int32_t* cells_host, int B, int dedup, int64_t* counts, void* ws,
                                              size_t ws_bytes, void* stream) {
  if (!offsets_ok(v_off_host, f_off_host, B) || !lattice_host || !cells_host || !counts || !ws) return DISN_E_ARG;
  const int64_t nv = v_off_host[B], nf = f_off_host[B];
  if ((nv > 0 && !verts) || (nf > 0 && !faces)) return DISN_E_ARG;
  if (!mesh_limits_ok(B, nv, nf)) return DISN_E_SHAPE;
  for (int b = 0; b < B; ++b) {
    const double h = lattice_host[4 * (size_t)b + 3];
    const float inv_h = (float)(1.0 / h);          // the cell's factor: positive and finite, as float32 too
    if (cells_host[b] < 1 || cells_host[b] > DISN_SIMPLIFY_MAX_CELLS || !(h > 0.0) || !(inv_h > 0.0f) ||
        !(inv_h <= 3.4028234663852886e38f) || !(h * h <= 1.7976931348623157e308))
      return DISN_E_SHAPE;
    for (int k = 0; k < 3; ++k)
      if (!(fabs(lattice_host[4 * (size_t)b + k]) <= 1.7976931348623157e308)) return DISN_E_SHAPE;
  }
  if (ws_bytes < simplify_layout(nullptr, B, nv, nf).total) return DISN_E_WS;
  hipStream_t st = (hipStream_t)stream;
  const SimplifyWs w = simplify_layout(ws, B, nv, nf);
  static_assert(sizeof(Lattice) == 4 * sizeof(double), "a lattice travels as four doubles");
  MESH_TRY(upload_offsets(w.voff, w.foff, v_off_host, f_off_host, B, st));
  MESH_TRY(hipMemcpyAsync(w.lat, lattice_host, (size_t)B * sizeof(Lattice), hipMemcpyHostToDevice, st));
  MESH_TRY(hipMemcpyAsync(w.cells, cells_host, (size_t)B * 4, hipMemcpyHostToDevice, st));
  MESH_TRY(hipMemsetAsync(w.status, 0, w.zero_bytes, st));
  if (nf > 0) MESH_LAUNCH(validate_faces_kernel, nf, faces, w.voff, w.foff, B, nf, w.status);
  if (nv > 0) {
    MESH_LAUNCH(validate_verts_kernel, nv, verts, w.voff, B, nv, w.status);
    MESH_TRY(hipMemsetAsync(w.vkeys, 0xFF, w.Tv * 8, st));
    MESH_TRY(hipMemsetAsync(w.vfirst, 0x7F, w.Tv * 4, st));
    MESH_LAUNCH(vertex_claim_kernel, nv, verts, w.voff, B, nv, w.lat, w.cells, w.status, w.vkeys, w.Tv - 1, w.vfirst,
           w.vslot);
    MESH_LAUNCH(vertex_flag_kernel, nv, w.voff, B, nv, w.status, w.vfirst, w.vslot, w.vflag, w.meshcnt);
    MESH_TRY(exclusive_scan(w.vflag, w.vscan, (size_t)nv, w.bsum, w.totals, st));
  }
  hipLaunchKernelGGL(cluster_base_kernel, dim3((B + 1 + kThreads - 1) / kThreads), dim3(kThreads), 0, st, w.voff, B,
                     nv, w.vscan, w.totals, w.cbase);
  MESH_TRY(hipGetLastError());
  if (nv > 0)
    MESH_LAUNCH(vertex_accum_kernel, nv, verts, w.voff, B, nv, w.lat, w.cells, w.status, w.vfirst, w.vslot, w.vscan,
           w.vclu, w.acc);
  if (nf > 0) {
    if (dedup) {
      MESH_TRY(hipMemsetAsync(w.fkeys, 0xFF, w.Tf * 8, st));
      MESH_TRY(hipMemsetAsync(w.fmin_, 0x7F, w.Tf * 4, st));
    }
    MESH_LAUNCH(face_kernel, nf, verts, faces, w.voff, w.foff, B, nf, w.lat, w.cells, dedup ? 1 : 0, w.status, w.vclu,
           w.acc, w.fkeys, w.Tf - 1, w.fmin_, w.fslot, w.meshcnt);
    MESH_LAUNCH(face_flag_kernel, nf, w.foff, B, nf, dedup ? 1 : 0, w.status, w.fmin_, w.fslot, w.fflag, w.meshcnt);
    MESH_TRY(exclusive_scan(w.fflag, w.fscan, (size_t)nf, w.bsum, w.totals + 1, st));
  }
  hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(1), 0, st, B, w.status, w.meshcnt, w.vseg,
                     reinterpret_cast<long long*>(counts));
  MESH_TRY(hipGetLastError());
  return 0;
}

extern "C" int disn_mesh_simplify_emit_batch(const float* verts, const int32_t* faces, const int64_t* v_off_host,
                                             const int64_t* f_off_host, int B, const int64_t* sizes_host,
                                             float* out_verts, int32_t* out_faces, int32_t* vmap, int32_t* first,
                                             void* ws, size_t ws_bytes, void* stream) {
  if (!offsets_ok(v_off_host, f_off_host, B) || !sizes_host || !ws) return DISN_E_ARG;
  const int64_t nv = v_off_host[B], nf = f_off_host[B];
  if (!mesh_limits_ok(B, nv, nf)) return DISN_E_SHAPE;
  if (ws_bytes < simplify_layout(nullptr, B, nv, nf).total) return DISN_E_WS;
  hipStream_t st = (hipStream_t)stream;
  const SimplifyWs w = simplify_layout(ws, B, nv, nf);
  // the totals from the sizes the caller read back (the device keeps its own): the outputs hold that much
  long long nvo = 0, nfo = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t* c = sizes_host + 4 * (size_t)b;
    const int64_t nvb = v_off_host[b + 1] - v_off_host[b], nfb = f_off_host[b + 1] - f_off_host[b];
    if (c[0] < 0 || c[0] > nvb || c[1] < 0 || c[1] > nfb || c[2] < 0 || c[2] > nfb) return DISN_E_ARG;
    nvo += c[0];
    nfo += c[1];
  }
  if (nv == 0) return 0;
  if (!verts || !vmap || (nvo > 0 && (!out_verts || !first)) || (nfo > 0 && (!faces || !out_faces)))
    return DISN_E_ARG;
  MESH_LAUNCH(emit_vmap_kernel, nv, w.voff, B, nv, w.status, w.vclu, w.cbase, vmap);
  if (nvo > 0)
    MESH_LAUNCH(solve_kernel, nv, verts, w.voff, B, nv, w.lat, w.cells, w.status, w.vflag, w.vclu, w.cbase, w.vseg, w.acc,
           nvo, out_verts, first);
  if (nfo > 0)
    MESH_LAUNCH(emit_faces_kernel, nf, faces, w.voff, w.foff, B, nf, w.fflag, w.fscan, w.vclu, w.cbase, nfo, out_faces);
  return 0;
}

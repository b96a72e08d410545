// Small-part cleanup of triangle meshes on the device (postprocessing/clean_smallparts.py of the reference, the rule
// restated by disn_amd/postprocess.py clean_arrays): B meshes back to back, as disn_mc_emit_batch leaves them.
//
//   count   validate -> edge table (connectivity 0) or first-face-per-vertex (1) -> union-find over faces (the larger
//           root is always hooked under the smaller, so a root is its component's smallest face) -> roots, ONE
//           scan of the root flags for the ranks -> distinct (component, vertex) pairs through a second table:
//           vertex counts (integers) and float64 coordinate sums -> the keep rule -> [B,5] sizes
//   emit    kept pairs listed in vertex order, kept faces in face order, each stably sorted by the part's rank among
//           its mesh's kept parts (one split pass per bit on exclusive_scan, segmented by mesh; no pass at all when
//           no mesh keeps two parts) -> vertices, vmap, re-indexed faces, kept ids
//
// NO KERNEL WAITS FOR ANOTHER WORKGROUP.  The only loops whose trip count depends on other threads:
//   find_root   follows parent[x] < x, strictly downwards: at most x steps
//   unite       retries only when its CAS found parent[a] already lowered by someone else, and goes on from that
//               lower value; a parent only ever decreases, so the retries of all threads together are bounded
//   claim/find  a probe index that advances once per step, at most `mask + 1` steps; a full table raises status 3
// Everything the emit writes is a function of integers alone; the one order-dependent quantity is the float64
// coordinate sum behind the centroid test (hardware float64 atomic add), DESIGN 4z.  Compiled with -ffp-contract=off.
// (mesh_of, the tables, the face validator and the host-side helpers are those of mesh_batch.hpp.)
#include "mesh_batch.hpp"

#include <vector>

namespace disn {
namespace {

enum { ST_NOTHING_KEPT = 1 };

// (find_root, unite and init_parent_kernel are those of mesh_batch.hpp: mesh_check.hip runs the same union-find)

__device__ __forceinline__ unsigned long long edge_key(const int* __restrict__ faces, long long f, int k,
                                                       long long vbase) {
  const unsigned long long a = (unsigned long long)(vbase + faces[3 * f + k]);
  const unsigned long long c = (unsigned long long)(vbase + faces[3 * f + (k + 1) % 3]);
  return (a < c ? a : c) << 32 | (a < c ? c : a);
}

__global__ __launch_bounds__(kThreads) void edge_insert_kernel(const int* __restrict__ faces,
                                                               const long long* __restrict__ voff,
                                                               const long long* __restrict__ foff, int B, long long nf,
                                                               int* __restrict__ status, unsigned long long* keys,
                                                               unsigned long long mask, int* minface) {
  GRID_STRIDE(f, nf) {
    const int b = mesh_of(foff, B, f);
    if (status[b]) continue;
    for (int k = 0; k < 3; ++k) {
      bool is_new;
      const long long s = table_claim(keys, mask, edge_key(faces, f, k, voff[b]), &is_new);
      if (s < 0) { atomicMax(&status[b], (int)ST_TABLE); break; }
      atomicMin(&minface[s], (int)f);
    }
  }
}

__global__ __launch_bounds__(kThreads) void edge_union_kernel(const int* __restrict__ faces,
                                                              const long long* __restrict__ voff,
                                                              const long long* __restrict__ foff, int B, long long nf,
                                                              const int* __restrict__ status,
                                                              const unsigned long long* __restrict__ keys,
                                                              unsigned long long mask, const int* __restrict__ minface,
                                                              int* parent) {
  GRID_STRIDE(f, nf) {
    const int b = mesh_of(foff, B, f);
    if (status[b]) continue;
    for (int k = 0; k < 3; ++k) {
      const long long s = table_find(keys, mask, edge_key(faces, f, k, voff[b]));
      if (s >= 0) unite(parent, (int)f, minface[s]);
    }
  }
}

__global__ __launch_bounds__(kThreads) void vertex_min_kernel(const int* __restrict__ faces,
                                                              const long long* __restrict__ voff,
                                                              const long long* __restrict__ foff, int B, long long nf,
                                                              const int* __restrict__ status, int* vmin) {
  GRID_STRIDE(f, nf) {
    const int b = mesh_of(foff, B, f);
    if (status[b]) continue;
    for (int k = 0; k < 3; ++k) atomicMin(&vmin[voff[b] + faces[3 * f + k]], (int)f);
  }
}

__global__ __launch_bounds__(kThreads) void vertex_union_kernel(const int* __restrict__ faces,
                                                                const long long* __restrict__ voff,
                                                                const long long* __restrict__ foff, int B,
                                                                long long nf, const int* __restrict__ status,
                                                                const int* __restrict__ vmin, int* parent) {
  GRID_STRIDE(f, nf) {
    const int b = mesh_of(foff, B, f);
    if (status[b]) continue;
    for (int k = 0; k < 3; ++k) unite(parent, (int)f, vmin[voff[b] + faces[3 * f + k]]);
  }
}

// root[f] and the root flags (a mesh with a status has none)
__global__ __launch_bounds__(kThreads) void compress_kernel(const long long* __restrict__ foff, int B, long long nf,
                                                            const int* __restrict__ status, int* parent,
                                                            int* __restrict__ root, unsigned* __restrict__ flag) {
  GRID_STRIDE(f, nf) {
    const int b = mesh_of(foff, B, f);
    const int r = status[b] ? -1 : find_root(parent, (int)f);
    root[f] = r;
    flag[f] = r == (int)f ? 1u : 0u;
  }
}

// cbase[b] = the global id of mesh b's first component, cbase[B] = all components
__global__ void comp_base_kernel(const long long* __restrict__ foff, int B, long long nf,
                                 const unsigned* __restrict__ fscan, const unsigned long long* __restrict__ ncomp_all,
                                 unsigned* __restrict__ cbase, long long* __restrict__ ncomp_out,
                                 const int* __restrict__ status) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b > B) return;
  const unsigned nc = (unsigned)*ncomp_all;
  auto base = [&](int m) { return (m < B && foff[m] < nf) ? fscan[foff[m]] : nc; };
  cbase[b] = base(b);
  if (b < B && ncomp_out) ncomp_out[b] = status[b] ? -(long long)status[b] : (long long)(base(b + 1) - base(b));
}

__global__ __launch_bounds__(kThreads) void label_kernel(const long long* __restrict__ foff, int B, long long nf,
                                                         const int* __restrict__ root,
                                                         const unsigned* __restrict__ fscan,
                                                         const unsigned* __restrict__ cbase,
                                                         unsigned* __restrict__ glabel, int* __restrict__ labels,
                                                         unsigned* cfaces, unsigned* __restrict__ croot) {
  GRID_STRIDE(f, nf) {
    const int r = root[f];
    if (r < 0) {
      glabel[f] = kNone;
      if (labels) labels[f] = -1;
      continue;
    }
    const unsigned gc = fscan[r];
    glabel[f] = gc;
    if (labels) labels[f] = (int)(gc - cbase[mesh_of(foff, B, f)]);
    atomicAdd(&cfaces[gc], 1u);
    if (r == (int)f) croot[gc] = (unsigned)f;
  }
}

// every distinct (component, vertex) pair once: its first claimant counts it, adds its coordinates and marks its
// corner as the pair's representative
__global__ __launch_bounds__(kThreads) void pair_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                        const long long* __restrict__ voff,
                                                        const long long* __restrict__ foff, int B, long long nf,
                                                        int* __restrict__ status,
                                                        const unsigned* __restrict__ glabel, unsigned long long* keys,
                                                        unsigned long long mask, unsigned char* __restrict__ rep,
                                                        unsigned* ccount, double* csum) {
  GRID_STRIDE(q, 3 * nf) {
    const long long f = q / 3;
    const unsigned gc = glabel[f];
    if (gc == kNone) continue;
    const int b = mesh_of(foff, B, f);
    const long long gv = voff[b] + faces[q];
    bool is_new;
    const long long s = table_claim(keys, mask, (unsigned long long)gc << 32 | (unsigned long long)gv, &is_new);
    if (s < 0) { atomicMax(&status[b], (int)ST_TABLE); continue; }
    if (!is_new) continue;
    rep[q] = 1;
    atomicAdd(&ccount[gc], 1u);
    for (int k = 0; k < 3; ++k) unsafeAtomicAdd(&csum[3 * (size_t)gc + k], (double)verts[3 * gv + k]);
  }
}

__global__ __launch_bounds__(kThreads) void biggest_kernel(const long long* __restrict__ foff, int B,
                                                           const unsigned long long* __restrict__ ncomp_all,
                                                           const unsigned* __restrict__ croot,
                                                           const unsigned* __restrict__ ccount, unsigned* biggest,
                                                           long long* __restrict__ comp_verts) {
  GRID_STRIDE(gc, (long long)*ncomp_all) {
    atomicMax(&biggest[mesh_of(foff, B, croot[gc])], ccount[gc]);
    if (comp_verts) comp_verts[gc] = ccount[gc];
  }
}

// clean_smallparts.py:38-54 as clean_arrays states it; gc runs over all nf slots so that keep[] is defined for the scan
__global__ __launch_bounds__(kThreads) void keep_kernel(const long long* __restrict__ foff, int B, long long nf,
                                                        const unsigned long long* __restrict__ ncomp_all,
                                                        const int* __restrict__ status,
                                                        const unsigned* __restrict__ croot,
                                                        const unsigned* __restrict__ ccount,
                                                        const unsigned* __restrict__ cfaces,
                                                        const double* __restrict__ csum,
                                                        const unsigned* __restrict__ biggest, double dist_thresh,
                                                        double num_thresh, unsigned* __restrict__ keep,
                                                        unsigned long long* meshcnt) {
  GRID_STRIDE(gc, nf) {
    unsigned k = 0;
    if (gc < (long long)*ncomp_all) {
      const int b = mesh_of(foff, B, croot[gc]);
      if (!status[b]) {
        const double n = (double)ccount[gc];
        const double cx = csum[3 * gc] / n, cy = csum[3 * gc + 1] / n, cz = csum[3 * gc + 2] / n;
        const double d = sqrt((cx * cx + cy * cy) + cz * cz);
        if (n > (double)biggest[b] * num_thresh && d < dist_thresh) {
          k = 1;
          atomicAdd(&meshcnt[3 * b], 1ull);
          atomicAdd(&meshcnt[3 * b + 1], (unsigned long long)ccount[gc]);
          atomicAdd(&meshcnt[3 * b + 2], (unsigned long long)cfaces[gc]);
        }
      }
    }
    keep[gc] = k;
  }
}

__global__ void finish_kernel(const long long* __restrict__ foff, int B, long long nf,
                              const unsigned* __restrict__ cbase, const unsigned* __restrict__ kscan,
                              const int* __restrict__ status, const unsigned long long* __restrict__ meshcnt,
                              unsigned* __restrict__ kbase, long long* __restrict__ counts) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  kbase[b] = cbase[b] < (unsigned long long)nf ? kscan[cbase[b]] : 0u;
  const long long ncomp = (long long)cbase[b + 1] - (long long)cbase[b];
  int st = status[b];
  const bool ok = st == 0;
  if (ok && foff[b + 1] > foff[b] && meshcnt[3 * b] == 0) st = ST_NOTHING_KEPT;
  counts[5 * b + 0] = ok ? ncomp : 0;
  counts[5 * b + 1] = ok ? (long long)meshcnt[3 * b] : 0;
  counts[5 * b + 2] = ok ? (long long)meshcnt[3 * b + 1] : 0;
  counts[5 * b + 3] = ok ? (long long)meshcnt[3 * b + 2] : 0;
  counts[5 * b + 4] = st;
}

// ---- emit ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool kept_corner(long long q, const unsigned char* __restrict__ rep,
                                            const unsigned* __restrict__ glabel, const unsigned* __restrict__ keep,
                                            unsigned* gc) {
  if (!rep[q]) return false;
  *gc = glabel[q / 3];     // a representative corner's face has a label
  return keep[*gc] != 0;
}

__global__ __launch_bounds__(kThreads) void pair_degree_kernel(const int* __restrict__ faces,
                                                               const long long* __restrict__ voff,
                                                               const long long* __restrict__ foff, int B, long long nf,
                                                               const unsigned char* __restrict__ rep,
                                                               const unsigned* __restrict__ glabel,
                                                               const unsigned* __restrict__ keep, unsigned* kdeg) {
  GRID_STRIDE(q, 3 * nf) {
    unsigned gc;
    if (!kept_corner(q, rep, glabel, keep, &gc)) continue;
    atomicAdd(&kdeg[voff[mesh_of(foff, B, q / 3)] + faces[q]], 1u);
  }
}

// the kept pairs in vertex order (pairs of one vertex belong to different parts: their order among themselves
// does not reach the output); key = the part's rank among its mesh's kept parts, value = the corner
__global__ __launch_bounds__(kThreads) void pair_list_kernel(const int* __restrict__ faces,
                                                             const long long* __restrict__ voff,
                                                             const long long* __restrict__ foff, int B, long long nf,
                                                             const unsigned char* __restrict__ rep,
                                                             const unsigned* __restrict__ glabel,
                                                             const unsigned* __restrict__ keep,
                                                             const unsigned* __restrict__ kscan,
                                                             const unsigned* __restrict__ kbase,
                                                             const unsigned* __restrict__ koff, unsigned* cursor,
                                                             long long n_out, unsigned* __restrict__ key,
                                                             unsigned* __restrict__ val) {
  GRID_STRIDE(q, 3 * nf) {
    unsigned gc;
    if (!kept_corner(q, rep, glabel, keep, &gc)) continue;
    const int b = mesh_of(foff, B, q / 3);
    const long long gv = voff[b] + faces[q];
    const long long pos = (long long)koff[gv] + atomicAdd(&cursor[gv], 1u);
    if (pos >= n_out) continue;
    key[pos] = kscan[gc] - kbase[b];
    val[pos] = (unsigned)q;
  }
}

__global__ __launch_bounds__(kThreads) void face_flag_kernel(long long nf, const unsigned* __restrict__ glabel,
                                                             const unsigned* __restrict__ keep,
                                                             unsigned* __restrict__ flag) {
  GRID_STRIDE(f, nf) flag[f] = (glabel[f] != kNone && keep[glabel[f]]) ? 1u : 0u;
}

__global__ __launch_bounds__(kThreads) void face_list_kernel(const long long* __restrict__ foff, int B, long long nf,
                                                             const unsigned* __restrict__ flag,
                                                             const unsigned* __restrict__ fpos,
                                                             const unsigned* __restrict__ glabel,
                                                             const unsigned* __restrict__ kscan,
                                                             const unsigned* __restrict__ kbase, long long n_out,
                                                             unsigned* __restrict__ key, unsigned* __restrict__ val) {
  GRID_STRIDE(f, nf) {
    if (!flag[f] || (long long)fpos[f] >= n_out) continue;
    key[fpos[f]] = kscan[glabel[f]] - kbase[mesh_of(foff, B, f)];
    val[fpos[f]] = (unsigned)f;
  }
}

// one stable split pass on bit `bit`, segmented by mesh (seg[b] .. seg[b+1] of the list belong to mesh b)
__global__ __launch_bounds__(kThreads) void split_flag_kernel(const unsigned* __restrict__ key, long long n, int bit,
                                                              unsigned* __restrict__ z) {
  GRID_STRIDE(i, n) z[i] = ((key[i] >> bit) & 1u) ? 0u : 1u;
}

__global__ __launch_bounds__(kThreads) void split_scatter_kernel(const unsigned* __restrict__ key,
                                                                 const unsigned* __restrict__ val, long long n,
                                                                 const unsigned* __restrict__ z,
                                                                 const unsigned* __restrict__ zs,
                                                                 const unsigned long long* __restrict__ ztotal,
                                                                 const long long* __restrict__ seg, int B,
                                                                 unsigned* __restrict__ key_out,
                                                                 unsigned* __restrict__ val_out) {
  GRID_STRIDE(i, n) {
    const int b = mesh_of(seg, B, i);
    const long long s = seg[b], e = seg[b + 1];
    const long long z0 = zs[s], z1 = e < n ? (long long)zs[e] : (long long)*ztotal;
    const long long before = (long long)zs[i] - z0;          // zeros of this segment in front of i
    const long long dest = z[i] ? s + before : s + (z1 - z0) + ((i - s) - before);
    if (dest < s || dest >= e) continue;                      // (cannot happen: counts and scan agree)
    key_out[dest] = key[i];
    val_out[dest] = val[i];
  }
}

__global__ __launch_bounds__(kThreads) void emit_verts_kernel(const float* __restrict__ verts,
                                                              const int* __restrict__ faces,
                                                              const long long* __restrict__ voff,
                                                              const long long* __restrict__ foff,
                                                              const long long* __restrict__ vseg, int B, long long nf,
                                                              const unsigned* __restrict__ val, long long n_out,
                                                              const unsigned* __restrict__ glabel,
                                                              const unsigned long long* __restrict__ keys,
                                                              unsigned long long mask, unsigned* __restrict__ newidx,
                                                              float* __restrict__ verts_out,
                                                              int* __restrict__ vmap_out) {
  GRID_STRIDE(i, n_out) {
    const long long q = val[i], f = q / 3;
    if (f >= nf || glabel[f] == kNone) continue;     // (a list the count did not leave: nothing is addressed through it)
    const int b = mesh_of(foff, B, f);
    const int local = faces[q];
    const long long gv = voff[b] + local;
    for (int k = 0; k < 3; ++k) verts_out[3 * i + k] = verts[3 * gv + k];
    vmap_out[i] = local;
    const long long s = table_find(keys, mask, (unsigned long long)glabel[f] << 32 | (unsigned long long)gv);
    if (s >= 0) newidx[s] = (unsigned)(i - vseg[b]);
  }
}

__global__ __launch_bounds__(kThreads) void emit_faces_kernel(const int* __restrict__ faces,
                                                              const long long* __restrict__ voff,
                                                              const long long* __restrict__ foff, int B, long long nf,
                                                              const unsigned* __restrict__ val, long long n_out,
                                                              const unsigned* __restrict__ glabel,
                                                              const unsigned long long* __restrict__ keys,
                                                              unsigned long long mask,
                                                              const unsigned* __restrict__ newidx,
                                                              int* __restrict__ faces_out) {
  GRID_STRIDE(j, n_out) {
    const long long f = val[j];
    if (f >= nf || glabel[f] == kNone) continue;
    const int b = mesh_of(foff, B, f);
    for (int k = 0; k < 3; ++k) {
      const long long gv = voff[b] + faces[3 * f + k];
      const long long s = table_find(keys, mask, (unsigned long long)glabel[f] << 32 | (unsigned long long)gv);
      faces_out[3 * j + k] = s >= 0 ? (int)newidx[s] : -1;
    }
  }
}

__global__ __launch_bounds__(kThreads) void emit_kept_kernel(const long long* __restrict__ foff,
                                                             const long long* __restrict__ kseg, int B,
                                                             const unsigned long long* __restrict__ ncomp_all,
                                                             const unsigned* __restrict__ croot,
                                                             const unsigned* __restrict__ keep,
                                                             const unsigned* __restrict__ kscan,
                                                             const unsigned* __restrict__ kbase,
                                                             const unsigned* __restrict__ cbase, long long n_out,
                                                             int* __restrict__ kept_out) {
  GRID_STRIDE(gc, (long long)*ncomp_all) {
    if (!keep[gc]) continue;
    const int b = mesh_of(foff, B, croot[gc]);
    const long long pos = kseg[b] + (kscan[gc] - kbase[b]);
    if (pos < n_out) kept_out[pos] = (int)(gc - cbase[b]);
  }
}

// where each mesh's kept parts, vertices and faces go in the outputs (B is a handful: one thread)
__global__ void segments_kernel(int B, const unsigned long long* __restrict__ meshcnt, long long* __restrict__ kseg,
                                long long* __restrict__ vseg, long long* __restrict__ fseg) {
  if (blockIdx.x || threadIdx.x) return;
  long long k = 0, v = 0, f = 0;
  for (int b = 0; b < B; ++b) {
    kseg[b] = k; vseg[b] = v; fseg[b] = f;
    k += (long long)meshcnt[3 * b]; v += (long long)meshcnt[3 * b + 1]; f += (long long)meshcnt[3 * b + 2];
  }
  kseg[B] = k; vseg[B] = v; fseg[B] = f;
}

// ---- host side -------------------------------------------------------------------------------------------------
struct CleanWs {
  long long *voff, *foff, *vseg, *fseg, *kseg;     // [B+1] each
  int* status;                                     // [B]    zeroed block starts here
  unsigned* biggest;                               // [B]
  unsigned long long* meshcnt;                     // [3B]   kept parts, their vertices, their faces
  unsigned *ccount, *cfaces;                       // [nf]   per component: distinct vertices, faces
  double* csum;                                    // [3nf]
  unsigned char* rep;                              // [3nf]  zeroed block ends behind it
  size_t zero_bytes;
  unsigned *cbase, *kbase;                         // [B+1], [B]
  int *parent, *root;                              // [nf]
  unsigned *flag, *fscan, *glabel, *croot, *keep, *kscan;   // [nf]
  int* vmin;                                       // [nv]
  unsigned *kdeg, *koff, *cursor;                  // [nv]
  unsigned long long* keys;                        // [T]
  unsigned* slotval;                               // [T]    edge table: smallest face; pair table: new vertex index
  unsigned long long T;
  unsigned *key[2], *val[2], *z, *zs;              // [3nf]  the sort's buffers
  unsigned* bsum;
  unsigned long long* totals;                      // [4]: components, kept parts, scratch, scratch
  size_t total;
};

CleanWs clean_layout(void* ws, int B, long long nv, long long nf) {
  WsCursor c(ws);
  const size_t b1 = (size_t)B + 1, f = (size_t)(nf > 0 ? nf : 1), v = (size_t)(nv > 0 ? nv : 1);
  CleanWs w;
  w.voff = c.take<long long>(b1); w.foff = c.take<long long>(b1);
  w.vseg = c.take<long long>(b1); w.fseg = c.take<long long>(b1); w.kseg = c.take<long long>(b1);
  const size_t z0 = c.next();
  w.status = c.take<int>(b1);
  w.biggest = c.take<unsigned>(b1);
  w.meshcnt = c.take<unsigned long long>(3 * b1);
  w.ccount = c.take<unsigned>(f); w.cfaces = c.take<unsigned>(f);
  w.csum = c.take<double>(3 * f);
  w.rep = c.take<unsigned char>(3 * f);
  w.zero_bytes = c.off - z0;
  w.cbase = c.take<unsigned>(b1); w.kbase = c.take<unsigned>(b1);
  w.parent = c.take<int>(f); w.root = c.take<int>(f);
  w.flag = c.take<unsigned>(f); w.fscan = c.take<unsigned>(f); w.glabel = c.take<unsigned>(f);
  w.croot = c.take<unsigned>(f); w.keep = c.take<unsigned>(f); w.kscan = c.take<unsigned>(f);
  w.vmin = c.take<int>(v);
  w.kdeg = c.take<unsigned>(v); w.koff = c.take<unsigned>(v); w.cursor = c.take<unsigned>(v);
  unsigned long long T = 16;
  while (T < 6ull * f) T <<= 1;          // 3 nf entries at most (edges, then pairs): at most half full
  w.T = T;
  w.keys = c.take<unsigned long long>(T);
  w.slotval = c.take<unsigned>(T);
  for (int i = 0; i < 2; ++i) { w.key[i] = c.take<unsigned>(3 * f); w.val[i] = c.take<unsigned>(3 * f); }
  w.z = c.take<unsigned>(3 * f); w.zs = c.take<unsigned>(3 * f);
  w.bsum = c.take<unsigned>(scan_bsum_items(3 * f > v ? 3 * f : v));
  w.totals = c.take<unsigned long long>(4);
  w.total = c.next();
  return w;
}

// labels (and, with verts, the statistics and the rule); leaves everything disn_mesh_clean_emit_batch reads in ws
int count_run(const float* verts, const int* faces, const int64_t* v_off, const int64_t* f_off, int B, int connectivity,
              double dist_thresh, double num_thresh, int* labels, long long* ncomp, long long* comp_verts,
              long long* counts, void* ws_ptr, hipStream_t st) {
  const long long nv = v_off[B], nf = f_off[B];
  const CleanWs w = clean_layout(ws_ptr, B, nv, nf);
  MESH_TRY(upload_offsets(w.voff, w.foff, v_off, f_off, B, st));
  MESH_TRY(hipMemsetAsync(w.status, 0, w.zero_bytes, st));
  MESH_TRY(hipMemsetAsync(w.totals, 0, 4 * 8, st));
  const int bb = (B + 1 + kThreads - 1) / kThreads;
  if (nf > 0) {
    const unsigned long long mask = w.T - 1;
    MESH_LAUNCH(init_parent_kernel, nf, w.parent, nf);
    MESH_LAUNCH(validate_faces_kernel, nf, faces, w.voff, w.foff, B, nf, w.status);
    MESH_TRY(hipMemsetAsync(w.keys, 0xFF, w.T * 8, st));
    if (connectivity == 0) {
      MESH_TRY(hipMemsetAsync(w.slotval, 0x7F, w.T * 4, st));
      MESH_LAUNCH(edge_insert_kernel, nf, faces, w.voff, w.foff, B, nf, w.status, w.keys, mask, (int*)w.slotval);
      MESH_LAUNCH(edge_union_kernel, nf, faces, w.voff, w.foff, B, nf, w.status, w.keys, mask, (const int*)w.slotval,
             w.parent);
      MESH_TRY(hipMemsetAsync(w.keys, 0xFF, w.T * 8, st));
    } else {
      MESH_TRY(hipMemsetAsync(w.vmin, 0x7F, (size_t)(nv > 0 ? nv : 1) * 4, st));
      MESH_LAUNCH(vertex_min_kernel, nf, faces, w.voff, w.foff, B, nf, w.status, w.vmin);
      MESH_LAUNCH(vertex_union_kernel, nf, faces, w.voff, w.foff, B, nf, w.status, w.vmin, w.parent);
    }
    MESH_LAUNCH(compress_kernel, nf, w.foff, B, nf, w.status, w.parent, w.root, w.flag);
    MESH_TRY(exclusive_scan(w.flag, w.fscan, (size_t)nf, w.bsum, w.totals, st));
  }
  hipLaunchKernelGGL(comp_base_kernel, dim3(bb), dim3(kThreads), 0, st, w.foff, B, nf, w.fscan, w.totals, w.cbase,
                     ncomp, w.status);
  MESH_TRY(hipGetLastError());
  if (nf > 0) {
    MESH_LAUNCH(label_kernel, nf, w.foff, B, nf, w.root, w.fscan, w.cbase, w.glabel, labels, w.cfaces, w.croot);
    if (verts) {
      MESH_LAUNCH(pair_kernel, 3 * nf, verts, faces, w.voff, w.foff, B, nf, w.status, w.glabel, w.keys, w.T - 1, w.rep,
             w.ccount, w.csum);
      MESH_LAUNCH(biggest_kernel, nf, w.foff, B, w.totals, w.croot, w.ccount, w.biggest, comp_verts);
    }
    if (counts) {
      MESH_LAUNCH(keep_kernel, nf, w.foff, B, nf, w.totals, w.status, w.croot, w.ccount, w.cfaces, w.csum, w.biggest,
             dist_thresh, num_thresh, w.keep, w.meshcnt);
      MESH_TRY(exclusive_scan(w.keep, w.kscan, (size_t)nf, w.bsum, w.totals + 1, st));
    }
  }
  if (counts) {
    hipLaunchKernelGGL(finish_kernel, dim3(bb), dim3(kThreads), 0, st, w.foff, B, nf, w.cbase, w.kscan, w.status,
                       w.meshcnt, w.kbase, counts);
    MESH_TRY(hipGetLastError());
  }
  return 0;
}

// `bits` stable split passes over (key, val)[0]; -> the buffer (0 or 1) that holds the result
int sort_run(const CleanWs& w, long long n, int bits, const long long* seg, int B, hipStream_t st, int* where) {
  int cur = 0;
  for (int bit = 0; bit < bits; ++bit, cur ^= 1) {
    MESH_LAUNCH(split_flag_kernel, n, w.key[cur], n, bit, w.z);
    MESH_TRY(exclusive_scan(w.z, w.zs, (size_t)n, w.bsum, w.totals + 2, st));
    MESH_LAUNCH(split_scatter_kernel, n, w.key[cur], w.val[cur], n, w.z, w.zs, w.totals + 2, seg, B, w.key[cur ^ 1],
           w.val[cur ^ 1]);
  }
  *where = cur;
  return 0;
}

}  // namespace
}  // namespace disn

using namespace disn;

extern "C" size_t disn_mesh_clean_workspace_bytes(int B, int64_t nv_total, int64_t nf_total) {
  return mesh_limits_ok(B, nv_total, nf_total) ? clean_layout(nullptr, B, nv_total, nf_total).total : 0;
}

extern "C" int disn_mesh_components_device(const float* verts, const int32_t* faces, const int64_t* v_off_host,
                                           const int64_t* f_off_host, int B, int connectivity, int32_t* labels,
                                           int64_t* ncomp, int64_t* comp_verts, void* ws, size_t ws_bytes,
                                           void* stream) {
  if (!offsets_ok(v_off_host, f_off_host, B) || !ncomp || !ws || (connectivity != 0 && connectivity != 1))
    return DISN_E_ARG;
  const int64_t nv = v_off_host[B], nf = f_off_host[B];
  if (nf > 0 && (!faces || !labels)) return DISN_E_ARG;
  if (comp_verts && nf > 0 && !verts) return DISN_E_ARG;
  if (!mesh_limits_ok(B, nv, nf)) return DISN_E_SHAPE;
  if (ws_bytes < clean_layout(nullptr, B, nv, nf).total) return DISN_E_WS;
  return count_run(comp_verts ? verts : nullptr, faces, v_off_host, f_off_host, B, connectivity, 0.0, 0.0, labels,
                   reinterpret_cast<long long*>(ncomp), reinterpret_cast<long long*>(comp_verts), nullptr, ws,
                   (hipStream_t)stream);
}

extern "C" int disn_mesh_clean_count_batch(const float* verts, const int32_t* faces, const int64_t* v_off_host,
                                           const int64_t* f_off_host, int B, int connectivity, double dist_thresh,
                                           double num_thresh, int64_t* counts, void* ws, size_t ws_bytes,
                                           void* stream) {
  if (!offsets_ok(v_off_host, f_off_host, B) || !counts || !ws || (connectivity != 0 && connectivity != 1))
    return DISN_E_ARG;
  const int64_t nv = v_off_host[B], nf = f_off_host[B];
  if (nf > 0 && (!faces || !verts)) return DISN_E_ARG;
  if (!mesh_limits_ok(B, nv, nf)) return DISN_E_SHAPE;
  if (ws_bytes < clean_layout(nullptr, B, nv, nf).total) return DISN_E_WS;
  return count_run(verts, faces, v_off_host, f_off_host, B, connectivity, dist_thresh, num_thresh, nullptr, nullptr,
                   nullptr, reinterpret_cast<long long*>(counts), ws, (hipStream_t)stream);
}

extern "C" int disn_mesh_clean_emit_batch(const float* verts, const int32_t* faces, const int64_t* v_off_host,
                                          const int64_t* f_off_host, const int64_t* counts_host, int B,
                                          float* verts_out, int32_t* faces_out, int32_t* vmap_out, int32_t* kept_out,
                                          void* ws, size_t ws_bytes, void* stream) {
  if (!offsets_ok(v_off_host, f_off_host, B) || !counts_host || !ws) return DISN_E_ARG;
  const int64_t nv = v_off_host[B], nf = f_off_host[B];
  if (!mesh_limits_ok(B, nv, nf)) return DISN_E_SHAPE;
  if (ws_bytes < clean_layout(nullptr, B, nv, nf).total) return DISN_E_WS;
  hipStream_t st = (hipStream_t)stream;
  const CleanWs w = clean_layout(ws, B, nv, nf);
  // the totals and the longest list of kept parts, from the sizes the caller read back (the device keeps its own)
  std::vector<long long> seg(3 * ((size_t)B + 1), 0);
  long long* kseg = seg.data();
  long long* vseg = kseg + B + 1;
  long long* fseg = vseg + B + 1;
  long long most = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t* c = counts_host + 5 * (size_t)b;
    const int64_t nvb = v_off_host[b + 1] - v_off_host[b], nfb = f_off_host[b + 1] - f_off_host[b];
    if (c[1] < 0 || c[1] > c[0] || c[0] > nfb || c[2] < 0 || c[2] > 3 * nfb || c[3] < 0 || c[3] > nfb || nvb < 0)
      return DISN_E_ARG;
    kseg[b + 1] = kseg[b] + c[1];
    vseg[b + 1] = vseg[b] + c[2];
    fseg[b + 1] = fseg[b] + c[3];
    if (c[1] > most) most = c[1];
  }
  const long long nk = kseg[B], nvo = vseg[B], nfo = fseg[B];
  if (nk == 0 || nvo == 0 || nfo == 0) return 0;
  if (!verts || !faces || !verts_out || !faces_out || !vmap_out || !kept_out) return DISN_E_ARG;
  int bits = 0;
  while ((1ll << bits) < most) ++bits;
  hipLaunchKernelGGL(segments_kernel, dim3(1), dim3(1), 0, st, B, w.meshcnt, w.kseg, w.vseg, w.fseg);
  MESH_TRY(hipGetLastError());
  const unsigned long long mask = w.T - 1;
  int at = 0;
  // vertices
  MESH_TRY(hipMemsetAsync(w.kdeg, 0, (size_t)nv * 4, st));
  MESH_TRY(hipMemsetAsync(w.cursor, 0, (size_t)nv * 4, st));
  MESH_LAUNCH(pair_degree_kernel, 3 * nf, faces, w.voff, w.foff, B, nf, w.rep, w.glabel, w.keep, w.kdeg);
  MESH_TRY(exclusive_scan(w.kdeg, w.koff, (size_t)nv, w.bsum, w.totals + 3, st));
  MESH_LAUNCH(pair_list_kernel, 3 * nf, faces, w.voff, w.foff, B, nf, w.rep, w.glabel, w.keep, w.kscan, w.kbase, w.koff,
         w.cursor, nvo, w.key[0], w.val[0]);
  if (int rc = sort_run(w, nvo, bits, w.vseg, B, st, &at)) return rc;
  MESH_LAUNCH(emit_verts_kernel, nvo, verts, faces, w.voff, w.foff, w.vseg, B, nf, w.val[at], nvo, w.glabel, w.keys, mask,
         w.slotval, verts_out, vmap_out);
  // faces
  MESH_LAUNCH(face_flag_kernel, nf, nf, w.glabel, w.keep, w.flag);
  MESH_TRY(exclusive_scan(w.flag, w.fscan, (size_t)nf, w.bsum, w.totals + 3, st));
  MESH_LAUNCH(face_list_kernel, nf, w.foff, B, nf, w.flag, w.fscan, w.glabel, w.kscan, w.kbase, nfo, w.key[0], w.val[0]);
  if (int rc = sort_run(w, nfo, bits, w.fseg, B, st, &at)) return rc;
  MESH_LAUNCH(emit_faces_kernel, nfo, faces, w.voff, w.foff, B, nf, w.val[at], nfo, w.glabel, w.keys, mask, w.slotval,
         faces_out);
  MESH_LAUNCH(emit_kept_kernel, nf, w.foff, w.kseg, B, w.totals, w.croot, w.keep, w.kscan, w.kbase, w.cbase, nk, kept_out);
  return 0;
}

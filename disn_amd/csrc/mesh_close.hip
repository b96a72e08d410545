// Closing of manifold meshes on the device: consistent orientation and hole filling (include/close/disn_amd_close.h;
// the rule is disn_amd/postprocess.py close_arrays, restated here operation by operation): B meshes back to back, as the
// meshers and the other mesh stages leave them.
//
//   count   validate indices and coordinates; the largest |coordinate| of every mesh -> every face without a repeated
//           index claims its three undirected edges (64-bit keys, table_claim): a slot counts its corner pairs, those
//           that run from the smaller index, and keeps the smallest and the largest pair -> status 16: a repeated
//           index, a slot with three pairs, a vertex on more than two boundary pairs -> orient: a union-find of faces
//           whose word is parent << 1 | parity (one 32-bit CAS links a root under a smaller one, with the parity the
//           edge's relation asks for); a second pass over the regular edges marks the root where the two parities
//           contradict the relation; every face adds itself to its root's n1 / n -> fill: a union-find of vertices
//           over the boundary pairs; every boundary pair adds 1 and its tail's quantised position to its loop's root ->
//           the flags of the filled loops and of their pairs, TWO scans, the centres -> outward: every face and every
//           fill face adds its quantised volume term to its root -> the flips -> [B][9] counts
//   emit    the input vertices and faces in place (a flipped face as (a, c, b)), the centres and the fill faces behind
//           them, each at its scan value; nothing is sorted
//
// NO KERNEL WAITS FOR ANOTHER WORKGROUP.  The loops whose trip count depends on other threads: the probe of the edge
// table (at most `mask + 1` steps; the table has two slots per possible edge, a full one raises status 3), find_parity
// and find_root (strictly downwards), unite and unite_parity (a retry only after ANOTHER thread's link succeeded).
// NO FLOATING-POINT ATOMIC: L, S, n1, n and V are integers, so no sum depends on its order.  Compiled with
// -ffp-contract=off: the volume terms round as numpy's do.
#include "mesh_batch.hpp"

#include "../../include/close/disn_amd_close.h"

namespace disn {
namespace {

enum { NF = DISN_CLOSE_FIELDS, ST_NOT_MANIFOLD = DISN_CLOSE_STATUS_NOT_MANIFOLD };

__device__ __forceinline__ void tally_add(unsigned long long* tally, int b, int field) {
  atomicAdd(&tally[(long long)b * NF + field], 1ull);
}

// the frexp exponent of a finite float given the bits of its magnitude: |x| = m 2^E, 0.5 <= m < 1; 0 for 0
__device__ __forceinline__ int exponent_of(unsigned bits) {
  const int ex = (int)(bits >> 23);
  const unsigned man = bits & 0x7FFFFFu;
  if (ex) return ex - 126;
  return man ? (32 - __clz((int)man)) - 149 : 0;              // a denormal: man 2^-149
}

// ---- validation beyond mesh_batch.hpp ------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void extent_kernel(const float* __restrict__ verts,
                                                          const long long* __restrict__ voff, int B, long long nv,
                                                          unsigned* maxbits) {
  GRID_STRIDE(v, nv) {
    const unsigned m0 = __float_as_uint(verts[3 * v]) & 0x7FFFFFFFu, m1 = __float_as_uint(verts[3 * v + 1]) & 0x7FFFFFFFu,
                   m2 = __float_as_uint(verts[3 * v + 2]) & 0x7FFFFFFFu;
    const unsigned m = m0 > m1 ? (m0 > m2 ? m0 : m2) : (m1 > m2 ? m1 : m2);   // magnitudes order as their bits do
    const int b = mesh_of(voff, B, v);
    if (m > __atomic_load_n(&maxbits[b], __ATOMIC_RELAXED)) atomicMax(&maxbits[b], m);
  }
}

// ---- edges -------------------------------------------------------------------------------------------------------
// corner pair c = 3 f + k runs from index k of face f to index (k+1)%3.  `badidx` is the status word of
// validate_faces_kernel alone: where it is set, no index of the mesh is looked at
__global__ __launch_bounds__(kThreads) void edge_insert_kernel(const int* __restrict__ faces,
                                                               const long long* __restrict__ voff,
                                                               const long long* __restrict__ foff, int B, long long nf,
                                                               const int* __restrict__ badidx, int* status,
                                                               unsigned long long* keys, unsigned long long mask,
                                                               unsigned* held, unsigned* fwd, int* pmin, int* pmax,
                                                               unsigned* __restrict__ eat) {
  GRID_STRIDE(f, nf) {
    const int b = mesh_of(foff, B, f);
    if (badidx[b]) continue;
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if (i0 == i1 || i1 == i2 || i2 == i0) {
      atomicMax(&status[b], (int)ST_NOT_MANIFOLD);
      continue;
    }
    const long long v0 = voff[b];
    const long long g[3] = {v0 + i0, v0 + i1, v0 + i2};
    for (int k = 0; k < 3; ++k) {
      const long long i = g[k], j = g[k == 2 ? 0 : k + 1];
      const int c = (int)(3 * f + k);
      const unsigned long long lo = (unsigned long long)(i < j ? i : j), hi = (unsigned long long)(i < j ? j : i);
      const long long s = table_claim(keys, mask, lo << 32 | hi);           // hi < 2^31: never kEmptyKey
      if (s < 0) { atomicMax(&status[b], (int)ST_TABLE); continue; }
      atomicAdd(&held[s], 1u);
      if (i < j) atomicAdd(&fwd[s], 1u);
      atomicMin(&pmin[s], c);
      atomicMax(&pmax[s], c);
      eat[c] = (unsigned)s;
    }
  }
}

// an edge of three or more pairs: status 16; a boundary pair counts at both its ends
__global__ __launch_bounds__(kThreads) void edge_class_kernel(const int* __restrict__ faces,
                                                              const long long* __restrict__ voff,
                                                              const long long* __restrict__ foff, int B,
                                                              long long corners, const unsigned* __restrict__ eat,
                                                              const unsigned* __restrict__ held, int* status,
                                                              unsigned* vbnd) {
  GRID_STRIDE(c, corners) {
    const unsigned s = eat[c];
    if (s == kNone) continue;                                  // so the mesh's indices are valid
    const long long f = c / 3;
    const int k = (int)(c - 3 * f), b = mesh_of(foff, B, f);
    if (held[s] >= 3u) atomicMax(&status[b], (int)ST_NOT_MANIFOLD);
    if (held[s] == 1u) {
      atomicAdd(&vbnd[voff[b] + faces[c]], 1u);
      atomicAdd(&vbnd[voff[b] + faces[3 * f + (k == 2 ? 0 : k + 1)]], 1u);
    }
  }
}

__global__ __launch_bounds__(kThreads) void vertex_degree_kernel(const long long* __restrict__ voff, int B, long long nv,
                                                                 const unsigned* __restrict__ vbnd, int* status) {
  GRID_STRIDE(v, nv)
    if (vbnd[v] > 2u) atomicMax(&status[mesh_of(voff, B, v)], (int)ST_NOT_MANIFOLD);
}

// from here on a mesh's status is final: one word says whether the mesh takes part
__global__ void merge_status_kernel(int B, const int* __restrict__ badidx, int* __restrict__ status) {
  for (int b = threadIdx.x; b < B; b += blockDim.x)
    if (badidx[b] > status[b]) status[b] = badidx[b];
}

// ---- orient ------------------------------------------------------------------------------------------------------
// a union-find of faces whose word is parent << 1 | parity: the parity of the face against its parent.  A root's word
// is itself << 1.  A word changes ONCE, when its root is linked under a smaller one; a walk sees parents that only
// decrease and parities that never change
struct Found {
  int root;
  unsigned parity;
};

__device__ __forceinline__ Found find_parity(unsigned* word, int x) {
  unsigned parity = 0;
  for (;;) {
    const unsigned w = __atomic_load_n(&word[x], __ATOMIC_RELAXED);
    const int p = (int)(w >> 1);
    if (p == x) return Found{x, parity};
    parity ^= w & 1u;
    x = p;                                                     // p < x
  }
}

// faces a and b are related by `rel`.  The CAS fails only when another thread linked the same root first
__device__ __forceinline__ void unite_parity(unsigned* word, int a, int b, unsigned rel) {
  for (;;) {
    Found x = find_parity(word, a), y = find_parity(word, b);
    if (x.root == y.root) return;
    if (x.root < y.root) { const Found t = x; x = y; y = t; }
    const unsigned self = (unsigned)x.root << 1, want = ((unsigned)y.root << 1) | (x.parity ^ y.parity ^ rel);
    if (atomicCAS(&word[x.root], self, want) == self) return;
  }
}

__global__ __launch_bounds__(kThreads) void init_word_kernel(unsigned* __restrict__ word, long long nf) {
  GRID_STRIDE(f, nf) word[f] = (unsigned)f << 1;
}

// one thread per regular edge, at its smallest pair: `check` == 0 unites, `check` == 1 compares
__global__ __launch_bounds__(kThreads) void face_union_kernel(const long long* __restrict__ foff, int B,
                                                              long long corners, const int* __restrict__ status,
                                                              const unsigned* __restrict__ eat,
                                                              const unsigned* __restrict__ held,
                                                              const unsigned* __restrict__ fwd,
                                                              const int* __restrict__ pmin, const int* __restrict__ pmax,
                                                              unsigned* word, int check, unsigned* twisted) {
  GRID_STRIDE(c, corners) {
    const unsigned s = eat[c];
    if (s == kNone || held[s] != 2u || pmin[s] != (int)c) continue;
    if (status[mesh_of(foff, B, c / 3)]) continue;
    const int f = (int)(c / 3), g = pmax[s] / 3;
    const unsigned rel = fwd[s] != 1u ? 1u : 0u;              // both pairs run the same way
    if (!check) {
      unite_parity(word, f, g, rel);
    } else {
      const Found x = find_parity(word, f), y = find_parity(word, g);
      if ((x.parity ^ y.parity) != rel) twisted[x.root] = 1u;
    }
  }
}

__global__ __launch_bounds__(kThreads) void face_root_kernel(const long long* __restrict__ foff, int B, long long nf,
                                                             const int* __restrict__ status, unsigned* word,
                                                             const unsigned* __restrict__ twisted,
                                                             int* __restrict__ froot, unsigned char* __restrict__ fpar,
                                                             unsigned* n1, unsigned* nall, unsigned long long* tally) {
  GRID_STRIDE(f, nf) {
    const int b = mesh_of(foff, B, f);
    if (status[b]) continue;
    const Found x = find_parity(word, (int)f);
    froot[f] = x.root;
    fpar[f] = (unsigned char)x.parity;
    atomicAdd(&nall[x.root], 1u);
    if (x.parity) atomicAdd(&n1[x.root], 1u);
    if (x.root == (int)f) {
      tally_add(tally, b, DISN_CLOSE_COMPONENTS);
      if (twisted[f]) tally_add(tally, b, DISN_CLOSE_UNORIENTABLE_COMPONENTS);
    }
  }
}

// ---- fill --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void loop_union_kernel(const int* __restrict__ faces,
                                                              const long long* __restrict__ voff,
                                                              const long long* __restrict__ foff, int B,
                                                              long long corners, const int* __restrict__ status,
                                                              const unsigned* __restrict__ eat,
                                                              const unsigned* __restrict__ held, int* vparent) {
  GRID_STRIDE(c, corners) {
    const unsigned s = eat[c];
    if (s == kNone || held[s] != 1u) continue;
    const long long f = c / 3;
    const int k = (int)(c - 3 * f), b = mesh_of(foff, B, f);
    if (status[b]) continue;
    unite(vparent, (int)(voff[b] + faces[c]), (int)(voff[b] + faces[3 * f + (k == 2 ? 0 : k + 1)]));
  }
}

// every boundary pair: its loop, one more pair there, and its tail's position in units of 2^(E-40)
__global__ __launch_bounds__(kThreads) void loop_sum_kernel(const float* __restrict__ verts,
                                                            const int* __restrict__ faces,
                                                            const long long* __restrict__ voff,
                                                            const long long* __restrict__ foff, int B,
                                                            long long corners, const int* __restrict__ status,
                                                            const unsigned* __restrict__ eat,
                                                            const unsigned* __restrict__ held,
                                                            const unsigned* __restrict__ maxbits, int* vparent,
                                                            int* __restrict__ cloop, unsigned* loopL,
                                                            unsigned long long* loopS) {
  GRID_STRIDE(c, corners) {
    const unsigned s = eat[c];
    if (s == kNone || held[s] != 1u) continue;
    const int b = mesh_of(foff, B, c / 3);
    if (status[b]) continue;
    const long long a = voff[b] + faces[c];
    const int r = find_root(vparent, (int)a);
    cloop[c] = r;
    atomicAdd(&loopL[r], 1u);
    const double unit = ldexp(1.0, 40 - exponent_of(maxbits[b]));
    for (int x = 0; x < 3; ++x) {
      const long long q = (long long)rint((double)verts[3 * a + x] * unit);
      atomicAdd(&loopS[3 * (long long)r + x], (unsigned long long)q);
    }
  }
}

__global__ __launch_bounds__(kThreads) void loop_flag_kernel(const long long* __restrict__ voff, int B, long long nv,
                                                             const int* __restrict__ status,
                                                             const unsigned* __restrict__ loopL, long long max_hole,
                                                             unsigned* __restrict__ vfill, unsigned long long* tally) {
  GRID_STRIDE(v, nv) {
    unsigned x = 0;
    const int b = mesh_of(voff, B, v);
    if (!status[b] && loopL[v] > 0u) {                          // a loop's pairs are counted at its smallest vertex
      tally_add(tally, b, DISN_CLOSE_LOOPS);
      x = (long long)loopL[v] <= max_hole ? 1u : 0u;
    }
    vfill[v] = x;
  }
}

// the pairs that get a face; a boundary pair that gets none leaves its component open
__global__ __launch_bounds__(kThreads) void pair_flag_kernel(const long long* __restrict__ foff, int B, long long corners,
                                                             const int* __restrict__ status,
                                                             const unsigned* __restrict__ eat,
                                                             const unsigned* __restrict__ held, int fill, int orient,
                                                             const int* __restrict__ cloop,
                                                             const unsigned* __restrict__ vfill,
                                                             const int* __restrict__ froot, unsigned* still_open,
                                                             unsigned* __restrict__ cfill) {
  GRID_STRIDE(c, corners) {
    unsigned x = 0;
    const unsigned s = eat[c];
    if (s != kNone && held[s] == 1u && !status[mesh_of(foff, B, c / 3)]) {
      if (fill) x = vfill[cloop[c]];
      if (!x && orient) still_open[froot[c / 3]] = 1u;
    }
    cfill[c] = x;
  }
}

__global__ __launch_bounds__(kThreads) void centre_kernel(const long long* __restrict__ voff, int B, long long nv,
                                                          const unsigned* __restrict__ vfill,
                                                          const unsigned* __restrict__ vscan,
                                                          const unsigned* __restrict__ loopL,
                                                          const unsigned long long* __restrict__ loopS,
                                                          const unsigned* __restrict__ maxbits,
                                                          float* __restrict__ centre) {
  GRID_STRIDE(v, nv) {
    if (!vfill[v]) continue;
    const double unit = ldexp(1.0, exponent_of(maxbits[mesh_of(voff, B, v)]) - 40), L = (double)loopL[v];
    for (int x = 0; x < 3; ++x)
      centre[3 * (long long)vscan[v] + x] = (float)((double)(long long)loopS[3 * v + x] / L * unit);
  }
}

// ---- outward -----------------------------------------------------------------------------------------------------
// ((x0 c0 + y0 c1) + z0 c2) / 6, c = p1 x p2, in units of 2^(3E-30)
__device__ __forceinline__ long long volume_term(const double* p0, const double* p1, const double* p2, double unit) {
  const double c0 = p1[1] * p2[2] - p1[2] * p2[1], c1 = p1[2] * p2[0] - p1[0] * p2[2], c2 = p1[0] * p2[1] - p1[1] * p2[0];
  return (long long)rint(((p0[0] * c0 + p0[1] * c1) + p0[2] * c2) / 6.0 * unit);
}

__device__ __forceinline__ unsigned majority(const unsigned* __restrict__ n1, const unsigned* __restrict__ nall, int r) {
  return n1[r] > nall[r] - n1[r] ? 1u : 0u;
}

__global__ __launch_bounds__(kThreads) void volume_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                          const long long* __restrict__ voff,
                                                          const long long* __restrict__ foff, int B, long long nf,
                                                          const int* __restrict__ status,
                                                          const unsigned* __restrict__ maxbits,
                                                          const int* __restrict__ froot,
                                                          const unsigned char* __restrict__ fpar,
                                                          const unsigned* __restrict__ n1,
                                                          const unsigned* __restrict__ nall,
                                                          const unsigned* __restrict__ cfill,
                                                          const int* __restrict__ cloop,
                                                          const unsigned* __restrict__ vscan,
                                                          const float* __restrict__ centre, unsigned long long* vol) {
  GRID_STRIDE(f, nf) {
    const int b = mesh_of(foff, B, f);
    if (status[b]) continue;
    const double unit = ldexp(1.0, 30 - 3 * exponent_of(maxbits[b]));
    double p[3][3];
    for (int k = 0; k < 3; ++k)
      for (int x = 0; x < 3; ++x) p[k][x] = (double)verts[3 * (voff[b] + faces[3 * f + k]) + x];
    const int r = froot[f];
    const bool plus = fpar[f] == majority(n1, nall, r);
    long long sum = volume_term(p[0], p[1], p[2], unit);
    for (int k = 0; k < 3; ++k) {
      if (!cfill[3 * f + k]) continue;                          // the fill face (centre, b, a) of pair a -> b
      double ce[3];
      for (int x = 0; x < 3; ++x) ce[x] = (double)centre[3 * (long long)vscan[cloop[3 * f + k]] + x];
      sum += volume_term(ce, p[k == 2 ? 0 : k + 1], p[k], unit);
    }
    atomicAdd(&vol[r], (unsigned long long)(plus ? sum : -sum));
  }
}

__global__ __launch_bounds__(kThreads) void flip_kernel(const long long* __restrict__ foff, int B, long long nf,
                                                        const int* __restrict__ status, int outward,
                                                        const int* __restrict__ froot,
                                                        const unsigned char* __restrict__ fpar,
                                                        const unsigned* __restrict__ twisted,
                                                        const unsigned* __restrict__ n1,
                                                        const unsigned* __restrict__ nall,
                                                        const unsigned* __restrict__ still_open,
                                                        const unsigned long long* __restrict__ vol,
                                                        unsigned char* __restrict__ fflip, unsigned long long* tally) {
  GRID_STRIDE(f, nf) {
    const int b = mesh_of(foff, B, f);
    if (status[b]) continue;
    const int r = froot[f];
    if (twisted[r]) continue;                                   // not orientable: as it came
    unsigned K = majority(n1, nall, r);
    if (outward && !still_open[r] && (long long)vol[r] < 0) K = 1u - K;
    if (fpar[f] != K) {
      fflip[f] = 1;
      tally_add(tally, b, DISN_CLOSE_FLIPPED_FACES);
    }
  }
}

// ---- numbering ---------------------------------------------------------------------------------------------------
struct MeshBase {
  long long v, c;             // the scan values at the mesh's first vertex and corner
  long long vseg, fseg;       // where its vertices and faces go in the outputs
};

// one thread: B is a handful
__global__ void finish_kernel(const long long* __restrict__ voff, const long long* __restrict__ foff, int B,
                              long long nv, long long nf, const int* __restrict__ status,
                              const unsigned* __restrict__ vscan, const unsigned* __restrict__ cscan,
                              const unsigned long long* __restrict__ totals,
                              const unsigned long long* __restrict__ tally, MeshBase* __restrict__ base,
                              long long* __restrict__ counts) {
  if (blockIdx.x || threadIdx.x) return;
  auto vb = [&](int m) { return (m < B && voff[m] < nv) ? (long long)vscan[voff[m]] : (long long)totals[0]; };
  auto cb = [&](int m) { return (m < B && foff[m] < nf) ? (long long)cscan[3 * foff[m]] : (long long)totals[1]; };
  long long vseg = 0, fseg = 0;
  for (int b = 0; b < B; ++b) {
    const long long centres = vb(b + 1) - vb(b), caps = cb(b + 1) - cb(b);
    base[b] = MeshBase{vb(b), cb(b), vseg, fseg};
    long long* c = counts + (long long)b * NF;
    const bool ok = status[b] == 0;
    for (int k = 0; k < NF; ++k) c[k] = ok ? (long long)tally[(long long)b * NF + k] : 0;
    c[DISN_CLOSE_NV_OUT] = (voff[b + 1] - voff[b]) + centres;
    c[DISN_CLOSE_NF_OUT] = (foff[b + 1] - foff[b]) + caps;
    c[DISN_CLOSE_STATUS] = status[b];
    c[DISN_CLOSE_FILLED_LOOPS] = centres;
    c[DISN_CLOSE_FILL_FACES] = caps;
    vseg += c[DISN_CLOSE_NV_OUT];
    fseg += c[DISN_CLOSE_NF_OUT];
  }
}

// ---- emit --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void emit_verts_kernel(const float* __restrict__ verts,
                                                              const long long* __restrict__ voff, int B, long long nv,
                                                              const unsigned* __restrict__ vfill,
                                                              const unsigned* __restrict__ vscan,
                                                              const float* __restrict__ centre,
                                                              const MeshBase* __restrict__ base, long long n_out,
                                                              float* __restrict__ verts_out, int* __restrict__ vmap_out) {
  GRID_STRIDE(v, nv) {
    const int b = mesh_of(voff, B, v);
    const long long local = v - voff[b], at = base[b].vseg + local;
    if (at >= 0 && at < n_out) {
      for (int x = 0; x < 3; ++x) verts_out[3 * at + x] = verts[3 * v + x];
      vmap_out[at] = (int)local;
    }
    if (!vfill[v]) continue;
    const long long to = base[b].vseg + (voff[b + 1] - voff[b]) + ((long long)vscan[v] - base[b].v);
    if (to < 0 || to >= n_out) continue;                        // (cannot happen: counts and scans agree)
    for (int x = 0; x < 3; ++x) verts_out[3 * to + x] = centre[3 * (long long)vscan[v] + x];
    vmap_out[to] = (int)local;
  }
}

__global__ __launch_bounds__(kThreads) void emit_faces_kernel(const int* __restrict__ faces,
                                                              const long long* __restrict__ voff,
                                                              const long long* __restrict__ foff, int B, long long nf,
                                                              const unsigned char* __restrict__ fflip,
                                                              const unsigned* __restrict__ cfill,
                                                              const unsigned* __restrict__ cscan,
                                                              const int* __restrict__ cloop,
                                                              const unsigned* __restrict__ vscan,
                                                              const MeshBase* __restrict__ base, long long n_out,
                                                              int* __restrict__ faces_out, int* __restrict__ kept_out) {
  GRID_STRIDE(f, nf) {
    const int b = mesh_of(foff, B, f);
    const long long local = f - foff[b], at = base[b].fseg + local;
    const bool flip = fflip[f] != 0;
    const int i[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
    if (at >= 0 && at < n_out) {
      faces_out[3 * at] = i[0];
      faces_out[3 * at + 1] = flip ? i[2] : i[1];
      faces_out[3 * at + 2] = flip ? i[1] : i[2];
      kept_out[at] = (int)local;
    }
    for (int k = 0; k < 3; ++k) {
      const long long c = 3 * f + k;
      if (!cfill[c]) continue;                                  // so the mesh has no status
      const long long to = base[b].fseg + (foff[b + 1] - foff[b]) + ((long long)cscan[c] - base[b].c);
      if (to < 0 || to >= n_out) continue;
      const int a = i[k], e = i[k == 2 ? 0 : k + 1];
      faces_out[3 * to] = (int)((voff[b + 1] - voff[b]) + ((long long)vscan[cloop[c]] - base[b].v));
      faces_out[3 * to + 1] = flip ? a : e;
      faces_out[3 * to + 2] = flip ? e : a;
      kept_out[to] = (int)local;
    }
  }
}

// ---- host side -------------------------------------------------------------------------------------------------
struct CloseWs {
  long long *voff, *foff;                          // [B+1]
  MeshBase* base;                                  // [B]
  // ---- zeroed
  int *status, *badidx;                            // [B]
  unsigned* maxbits;                               // [B]
  unsigned long long* tally;                       // [B][NF]
  unsigned long long* totals;                      // [2]: centres, fill faces
  unsigned *held, *fwd;                            // [Te]
  int* pmax;                                       // [Te]
  unsigned *vbnd, *loopL;                          // [nv]
  unsigned long long* loopS;                       // [nv][3]
  unsigned *n1, *nall, *twisted, *still_open;      // [nf], read at the roots
  unsigned long long* vol;                         // [nf], read at the roots
  unsigned char* fflip;                            // [nf]
  size_t zero_bytes;
  // ---- 0x7F
  int* pmin;                                       // [Te]
  size_t free_bytes;
  // ---- 0xFF: empty keys, kNone
  unsigned long long* keys;                        // [Te]
  unsigned* eat;                                   // [3 nf]: the slot of a corner pair
  size_t none_bytes;
  // ----
  unsigned long long Te;
  unsigned* word;                                  // [nf]
  int* froot;                                      // [nf]
  unsigned char* fpar;                             // [nf]
  int *vparent, *cloop;                            // [nv], [3 nf]
  unsigned *vfill, *vscan, *cfill, *cscan;         // [nv] x 2, [3 nf] x 2
  float* centre;                                   // [nv][3]: at a loop's scan value
  unsigned* bsum;
  size_t total;
};

CloseWs close_layout(void* ws, int B, long long nv, long long nf) {
  WsCursor c(ws);
  const size_t b1 = (size_t)B + 1, f = (size_t)(nf > 0 ? nf : 1), v = (size_t)(nv > 0 ? nv : 1);
  CloseWs w;
  w.Te = table_size(3 * f);
  w.voff = c.take<long long>(b1); w.foff = c.take<long long>(b1);
  w.base = c.take<MeshBase>(b1);
  const size_t z0 = c.next();
  w.status = c.take<int>(b1); w.badidx = c.take<int>(b1);
  w.maxbits = c.take<unsigned>(b1);
  w.tally = c.take<unsigned long long>(NF * b1);
  w.totals = c.take<unsigned long long>(2);
  w.held = c.take<unsigned>(w.Te); w.fwd = c.take<unsigned>(w.Te);
  w.pmax = c.take<int>(w.Te);
  w.vbnd = c.take<unsigned>(v); w.loopL = c.take<unsigned>(v);
  w.loopS = c.take<unsigned long long>(3 * v);
  w.n1 = c.take<unsigned>(f); w.nall = c.take<unsigned>(f); w.twisted = c.take<unsigned>(f);
  w.still_open = c.take<unsigned>(f);
  w.vol = c.take<unsigned long long>(f);
  w.fflip = c.take<unsigned char>(f);
  w.zero_bytes = c.off - z0;
  const size_t f0 = c.next();
  w.pmin = c.take<int>(w.Te);
  w.free_bytes = c.off - f0;
  const size_t n0 = c.next();
  w.keys = c.take<unsigned long long>(w.Te);
  w.eat = c.take<unsigned>(3 * f);
  w.none_bytes = c.off - n0;
  w.word = c.take<unsigned>(f);
  w.froot = c.take<int>(f);
  w.fpar = c.take<unsigned char>(f);
  w.vparent = c.take<int>(v); w.cloop = c.take<int>(3 * f);
  w.vfill = c.take<unsigned>(v); w.vscan = c.take<unsigned>(v);
  w.cfill = c.take<unsigned>(3 * f); w.cscan = c.take<unsigned>(3 * f);
  w.centre = c.take<float>(3 * v);
  w.bsum = c.take<unsigned>(scan_bsum_items(3 * f > v ? 3 * f : v));
  w.total = c.next();
  return w;
}

int count_run(const float* verts, const int* faces, const int64_t* v_off, const int64_t* f_off, int B, int flags,
              long long max_hole, long long* counts, void* ws_ptr, hipStream_t st) {
  const long long nv = v_off[B], nf = f_off[B], corners = 3 * nf;
  const CloseWs w = close_layout(ws_ptr, B, nv, nf);
  const int orient = (flags & DISN_CLOSE_ORIENT) != 0, fill = (flags & DISN_CLOSE_FILL) != 0,
            outward = (flags & DISN_CLOSE_OUTWARD) != 0;
  MESH_TRY(upload_offsets(w.voff, w.foff, v_off, f_off, B, st));
  MESH_TRY(hipMemsetAsync(w.status, 0, w.zero_bytes, st));
  MESH_TRY(hipMemsetAsync(w.pmin, 0x7F, w.free_bytes, st));
  MESH_TRY(hipMemsetAsync(w.keys, 0xFF, w.none_bytes, st));
  if (nf > 0) MESH_LAUNCH(validate_faces_kernel, nf, faces, w.voff, w.foff, B, nf, w.badidx);
  if (nv > 0) {
    MESH_LAUNCH(validate_verts_kernel, nv, verts, w.voff, B, nv, w.status);
    MESH_LAUNCH(extent_kernel, nv, verts, w.voff, B, nv, w.maxbits);
  }
  if (nf > 0) {
    MESH_LAUNCH(edge_insert_kernel, nf, faces, w.voff, w.foff, B, nf, w.badidx, w.status, w.keys, w.Te - 1, w.held, w.fwd,
                w.pmin, w.pmax, w.eat);
    MESH_LAUNCH(edge_class_kernel, corners, faces, w.voff, w.foff, B, corners, w.eat, w.held, w.status, w.vbnd);
  }
  if (nv > 0) MESH_LAUNCH(vertex_degree_kernel, nv, w.voff, B, nv, w.vbnd, w.status);
  hipLaunchKernelGGL(merge_status_kernel, dim3(1), dim3(kThreads), 0, st, B, w.badidx, w.status);
  MESH_TRY(hipGetLastError());
  if (nf > 0 && orient) {
    MESH_LAUNCH(init_word_kernel, nf, w.word, nf);
    for (int check = 0; check < 2; ++check)
      MESH_LAUNCH(face_union_kernel, corners, w.foff, B, corners, w.status, w.eat, w.held, w.fwd, w.pmin, w.pmax, w.word,
                  check, w.twisted);
    MESH_LAUNCH(face_root_kernel, nf, w.foff, B, nf, w.status, w.word, w.twisted, w.froot, w.fpar, w.n1, w.nall, w.tally);
  }
  if (nf > 0 && nv > 0 && fill) {
    MESH_LAUNCH(init_parent_kernel, nv, w.vparent, nv);
    MESH_LAUNCH(loop_union_kernel, corners, faces, w.voff, w.foff, B, corners, w.status, w.eat, w.held, w.vparent);
    MESH_LAUNCH(loop_sum_kernel, corners, verts, faces, w.voff, w.foff, B, corners, w.status, w.eat, w.held, w.maxbits,
                w.vparent, w.cloop, w.loopL, w.loopS);
  }
  if (nv > 0) {
    MESH_LAUNCH(loop_flag_kernel, nv, w.voff, B, nv, w.status, w.loopL, max_hole, w.vfill, w.tally);
    MESH_TRY(exclusive_scan(w.vfill, w.vscan, (size_t)nv, w.bsum, w.totals, st));
  }
  if (nf > 0) {
    MESH_LAUNCH(pair_flag_kernel, corners, w.foff, B, corners, w.status, w.eat, w.held, fill && nv > 0, orient, w.cloop,
                w.vfill, w.froot, w.still_open, w.cfill);
    MESH_TRY(exclusive_scan(w.cfill, w.cscan, (size_t)corners, w.bsum, w.totals + 1, st));
  }
  if (nv > 0 && fill)
    MESH_LAUNCH(centre_kernel, nv, w.voff, B, nv, w.vfill, w.vscan, w.loopL, w.loopS, w.maxbits, w.centre);
  if (nf > 0 && orient) {
    if (outward)
      MESH_LAUNCH(volume_kernel, nf, verts, faces, w.voff, w.foff, B, nf, w.status, w.maxbits, w.froot, w.fpar, w.n1,
                  w.nall, w.cfill, w.cloop, w.vscan, w.centre, w.vol);
    MESH_LAUNCH(flip_kernel, nf, w.foff, B, nf, w.status, outward, w.froot, w.fpar, w.twisted, w.n1, w.nall, w.still_open,
                w.vol, w.fflip, w.tally);
  }
  hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(1), 0, st, w.voff, w.foff, B, nv, nf, w.status, w.vscan, w.cscan,
                     w.totals, w.tally, w.base, counts);
  MESH_TRY(hipGetLastError());
  return 0;
}

bool flags_ok(int flags, int64_t max_hole) {
  if (flags & ~(DISN_CLOSE_ORIENT | DISN_CLOSE_FILL | DISN_CLOSE_OUTWARD)) return false;
  if ((flags & DISN_CLOSE_OUTWARD) && !(flags & DISN_CLOSE_ORIENT)) return false;
  return max_hole >= 0 && max_hole <= DISN_CLOSE_MAX_HOLE;
}

}  // namespace
}  // namespace disn

using namespace disn;

extern "C" size_t disn_mesh_close_workspace_bytes(int B, int64_t nv_total, int64_t nf_total) {
  return mesh_limits_ok(B, nv_total, nf_total) ? close_layout(nullptr, B, nv_total, nf_total).total : 0;
}

extern "C" int disn_mesh_close_count_batch(const float* verts, const int32_t* faces, const int64_t* v_off_host,
                                           const int64_t* f_off_host, int B, int flags, int64_t max_hole,
                                           int64_t* counts, void* ws, size_t ws_bytes, void* stream) {
  static_assert(sizeof(long long) == sizeof(int64_t), "the counts travel as int64");
  if (!offsets_ok(v_off_host, f_off_host, B) || !counts || !ws || !flags_ok(flags, max_hole)) return DISN_E_ARG;
  const int64_t nv = v_off_host[B], nf = f_off_host[B];
  if ((nv > 0 && !verts) || (nf > 0 && !faces)) return DISN_E_ARG;
  if (!mesh_limits_ok(B, nv, nf)) return DISN_E_SHAPE;
  if (ws_bytes < close_layout(nullptr, B, nv, nf).total) return DISN_E_WS;
  return count_run(verts, faces, v_off_host, f_off_host, B, flags, max_hole, reinterpret_cast<long long*>(counts), ws,
                   (hipStream_t)stream);
}

extern "C" int disn_mesh_close_emit_batch(const float* verts, const int32_t* faces, const int64_t* v_off_host,
                                          const int64_t* f_off_host, int B, int flags, int64_t max_hole,
                                          const int64_t* counts_host, float* verts_out, int32_t* faces_out,
                                          int32_t* vmap_out, int32_t* kept_out, void* ws, size_t ws_bytes,
                                          void* stream) {
  if (!offsets_ok(v_off_host, f_off_host, B) || !counts_host || !ws || !flags_ok(flags, max_hole)) return DISN_E_ARG;
  const int64_t nv = v_off_host[B], nf = f_off_host[B];
  if (!mesh_limits_ok(B, nv, nf)) return DISN_E_SHAPE;
  if (ws_bytes < close_layout(nullptr, B, nv, nf).total) return DISN_E_WS;
  long long nvo = 0, nfo = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t* c = counts_host + (size_t)NF * b;
    const int64_t nvb = v_off_host[b + 1] - v_off_host[b], nfb = f_off_host[b + 1] - f_off_host[b];
    // every pair gives at most one face, every filled loop has at least three; a mesh with a status gains nothing
    const int64_t caps = c[DISN_CLOSE_NF_OUT] - nfb, centres = c[DISN_CLOSE_NV_OUT] - nvb;
    const int64_t most = (c[DISN_CLOSE_STATUS] || !(flags & DISN_CLOSE_FILL)) ? 0 : 3 * nfb;
    if (caps < 0 || caps > most || centres < 0 || 3 * centres > caps) return DISN_E_ARG;
    nvo += c[DISN_CLOSE_NV_OUT];
    nfo += c[DISN_CLOSE_NF_OUT];
  }
  if (nvo == 0 && nfo == 0) return 0;
  if ((nvo > 0 && (!verts || !verts_out || !vmap_out)) || (nfo > 0 && (!faces || !faces_out || !kept_out)))
    return DISN_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  const CloseWs w = close_layout(ws, B, nv, nf);
  if (nv > 0)
    MESH_LAUNCH(emit_verts_kernel, nv, verts, w.voff, B, nv, w.vfill, w.vscan, w.centre, w.base, nvo, verts_out, vmap_out);
  if (nf > 0)
    MESH_LAUNCH(emit_faces_kernel, nf, faces, w.voff, w.foff, B, nf, w.fflip, w.cfill, w.cscan, w.cloop, w.vscan, w.base,
                nfo, faces_out, kept_out);
  return 0;
}

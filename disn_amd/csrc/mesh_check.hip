// Topology, orientation and self-intersection checks of meshes on the device (include/check/disn_amd_check.h; the rule
// is disn_amd/postprocess.py check_arrays, restated here operation by operation): B meshes back to back, as the meshers
// and the other mesh stages leave them.  Nothing of a mesh changes.
//
//   topology  validate indices and coordinates -> every face that takes part claims the slots of its three undirected
//             edges, keyed by batch-global vertex ids (lo << 32 | hi); a slot counts its corner pairs, those that run
//             from the smaller index, and keeps the smallest corner at either end -> every face reads its slots back
//             (its flag bits; the corner pair that holds a slot's smallest corner tallies the edge's class) and unites
//             its two corners on every edge with the slot's smallest ones: the corners of one vertex that are joined
//             through shared edges end under one root -> one thread per corner counts the roots at its vertex -> one thread per vertex tallies
//   geometry  one thread per face: cross product, the area and volume terms, the float32 box, the face's extent
//             (quantised, an integer sum) -> per mesh: the cell size, twice the mean extent, and the grid
//   bins      a face that spans at most 8 cells claims each cell's slot, keyed mesh << 32 | cell, and counts itself
//             there; any other goes to the list of large faces -> ONE scan of the slot counts -> the faces are written
//             into their cells' rows -> the work estimate per mesh -> status 8 for a mesh over DISN_CHECK_WORK_FACTOR
//             times its cap
//   pairs     one thread per row entry walks the entries behind it; a pair belongs to the ONE cell that holds the larger
//             of the two boxes' lower corners, so it is met once; a large face walks its whole mesh.  First pass: the
//             exact box test alone, the candidate count -> status 8 above the cap -> second pass, the meshes with status
//             0 only: the six edge-triangle tests.  The rows lie in hash order, so a thread adds what it found to its
//             face's counter and a pass in face order tallies the counters
//   finish    the sums over a fixed tree (slabs of the mesh, 256 strided partial sums, a binary tree, the slabs in
//             order), the face flags, the fields that derive from others and the -1 of an invalid field
//
// NO KERNEL WAITS FOR ANOTHER WORKGROUP.  The loops whose trip count depends on other threads: table_claim's probe (at
// most `mask + 1` steps; a full table raises status 3: the edge table has two slots per possible edge, the cell table
// two per possible entry), find_root (strictly downwards) and unite (mesh_batch.hpp).  Every other loop runs over a row
// or a mesh whose length the work estimate has bounded by the cap.  NO FLOATING-POINT ATOMIC: the integer tallies are
// 64-bit adds, one per wave where the wave lies in one mesh.  No host synchronisation and no read-back.  Compiled with
// -ffp-contract=off: the float64 arithmetic rounds as numpy's does.
#include "mesh_batch.hpp"

#include "../../include/check/disn_amd_check.h"

namespace disn {
namespace {

enum { ST_PAIRS = DISN_CHECK_PAIRS, NF = DISN_CHECK_FIELDS, SLABS = DISN_CHECK_SLABS };
enum : unsigned char { F_PART = 0x80, F_LARGE = 0x40, F_PUBLIC = 0x1F };
constexpr int kMaxSpan = 8;                         // cells a face may be listed in
constexpr int kMaxGrid = 1024;                      // cells per axis: a cell is 3 x 10 bits of its key
constexpr double kExtScale = 1048576.0;             // 2^20: a face extent is summed as an integer of this unit
constexpr double kExtMax = 68719476736.0;           // 2^36: 2^27 faces stay below 2^63

struct Grid {                                       // one mesh's uniform grid
  double lo[3], inv_h;
  int g[3];
};

// a loop every lane of a wave leaves together: `live` is false behind the end
#define WAVE_STRIDE(i, n, live)                                                                              \
  for (long long _b = (long long)blockIdx.x * blockDim.x, i = _b + threadIdx.x; _b < (n);                  \
       _b += (long long)gridDim.x * blockDim.x, i = _b + threadIdx.x)                                        \
    if (const bool live = i < (n); true)

// counts[b][field] += val.  EVERY lane of the wave calls this together (val 0: nothing to add); one atomic per wave
// where all its adding lanes lie in one mesh
__device__ __forceinline__ void wave_add(long long* counts, int b, int field, unsigned long long val) {
  const unsigned long long m = __ballot(val != 0);
  if (!m) return;
  const int leader = __ffsll((long long)m) - 1;
  const int b0 = __shfl(b, leader);
  if (__all(val == 0 || b == b0)) {
    unsigned long long s = val;
    for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
    if ((int)(threadIdx.x & 63) == leader)
      atomicAdd(reinterpret_cast<unsigned long long*>(&counts[(long long)b0 * NF + field]), s);
  } else if (val) {
    atomicAdd(reinterpret_cast<unsigned long long*>(&counts[(long long)b * NF + field]), val);
  }
}

__device__ __forceinline__ bool topo_ok(int st) { return st != ST_INDEX && st != ST_TABLE; }

// float32 <-> a uint32 of the same order (for integer atomicMin / atomicMax)
__device__ __forceinline__ unsigned ordered_of(float x) {
  const unsigned u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float float_of(unsigned o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}

// mbox[b] takes in the box lo .. hi (ordered values).  EVERY lane of the wave calls this together (has false: no box);
// six atomics per wave where all its boxes lie in one mesh
__device__ __forceinline__ void wave_box(unsigned* mbox, int b, bool has, const unsigned* lo, const unsigned* hi) {
  const unsigned long long m = __ballot(has);
  if (!m) return;
  const int leader = __ffsll((long long)m) - 1;
  const int b0 = __shfl(b, leader);
  if (__all(!has || b == b0)) {
    for (int a = 0; a < 3; ++a) {
      unsigned l = has ? lo[a] : 0xFFFFFFFFu, h = has ? hi[a] : 0u;
      for (int o = 32; o; o >>= 1) {
        const unsigned l2 = __shfl_xor(l, o), h2 = __shfl_xor(h, o);
        l = l2 < l ? l2 : l;
        h = h2 > h ? h2 : h;
      }
      if ((int)(threadIdx.x & 63) == leader) {
        atomicMin(&mbox[6 * b0 + a], l);
        atomicMax(&mbox[6 * b0 + 3 + a], h);
      }
    }
  } else if (has) {
    for (int a = 0; a < 3; ++a) {
      atomicMin(&mbox[6 * b + a], lo[a]);
      atomicMax(&mbox[6 * b + 3 + a], hi[a]);
    }
  }
}

__global__ __launch_bounds__(kThreads) void init_kernel(unsigned* __restrict__ mbox, int B) {
  GRID_STRIDE(i, 6ll * B) mbox[i] = (i % 6) < 3 ? 0xFFFFFFFFu : 0u;       // lower corner, upper corner
}

// ---- topology ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void edge_claim_kernel(const int* __restrict__ faces,
                                                              const long long* __restrict__ voff,
                                                              const long long* __restrict__ foff, int B, long long nf,
                                                              int* status, unsigned long long* keys,
                                                              unsigned long long mask, unsigned* held, unsigned* fwd,
                                                              int* rep, unsigned char* ref, unsigned char* fstate,
                                                              long long* counts) {
  WAVE_STRIDE(f, nf, live) {
    const int b = live ? mesh_of(foff, B, f) : 0;
    unsigned long long degenerate = 0;
    if (live && topo_ok(status[b])) {                          // so every index below lies in [0, nv_b)
      const long long v0 = voff[b];
      const int c[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
      if (c[0] == c[1] || c[1] == c[2] || c[2] == c[0]) {
        degenerate = 1;
        fstate[f] = DISN_CHECK_FLAG_DEGENERATE;
      } else {
        fstate[f] = F_PART;
        for (int k = 0; k < 3; ++k) {
          const int k1 = k == 2 ? 0 : k + 1, i = c[k], j = c[k1];
          ref[v0 + i] = 1;
          const bool up = i < j;
          const unsigned long long lo = (unsigned long long)(v0 + (up ? i : j));
          const unsigned long long hi = (unsigned long long)(v0 + (up ? j : i));   // < 2^31: the key is never kEmptyKey
          const long long s = table_claim(keys, mask, lo << 32 | hi);
          if (s < 0) { atomicMax(&status[b], (int)ST_TABLE); continue; }
          atomicAdd(&held[s], 1u);
          if (up) atomicAdd(&fwd[s], 1u);
          atomicMin(&rep[2 * s], (int)(3 * f + (up ? k : k1)));                     // the smallest corner at lo
          atomicMin(&rep[2 * s + 1], (int)(3 * f + (up ? k1 : k)));                 // and at hi
        }
      }
    }
    wave_add(counts, b, DISN_CHECK_INDEX_DEGENERATE_FACES, degenerate);
  }
}

__device__ __forceinline__ unsigned char edge_class(unsigned held, unsigned fwd) {
  return held == 1u ? DISN_CHECK_FLAG_BOUNDARY
       : held >= 3u ? DISN_CHECK_FLAG_NONMANIFOLD
       : (held == 2u && fwd != 1u) ? DISN_CHECK_FLAG_MISORIENTED : 0;
}

// every face that takes part: the flag bits of its edges, and its corners joined with the edges' smallest ones.  The
// corner pair whose lo corner IS the slot's smallest one owns the edge and tallies it: once per edge, from a loop in
// face order, where a wave lies in one mesh (a loop over the hashed slots would meet the meshes at random)
__global__ __launch_bounds__(kThreads) void fan_union_kernel(const int* __restrict__ faces,
                                                             const long long* __restrict__ voff,
                                                             const long long* __restrict__ foff, int B, long long nf,
                                                             const int* __restrict__ status,
                                                             const unsigned long long* __restrict__ keys,
                                                             unsigned long long mask, const unsigned* __restrict__ held,
                                                             const unsigned* __restrict__ fwd,
                                                             const int* __restrict__ rep, long long corners,
                                                             unsigned char* fstate, int* parent, long long* counts) {
  WAVE_STRIDE(f, nf, live) {
    const int b = live ? mesh_of(foff, B, f) : 0;
    unsigned long long own[4] = {0, 0, 0, 0};                  // edges, boundary, non-manifold, misoriented
    if (live && topo_ok(status[b]) && (fstate[f] & F_PART)) {
      const long long v0 = voff[b];
      const int c[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
      unsigned char bits = 0;
      for (int k = 0; k < 3; ++k) {
        const int k1 = k == 2 ? 0 : k + 1, i = c[k], j = c[k1];
        const bool up = i < j;
        const unsigned long long lo = (unsigned long long)(v0 + (up ? i : j));
        const unsigned long long hi = (unsigned long long)(v0 + (up ? j : i));
        const long long s = table_find(keys, mask, lo << 32 | hi);
        if (s < 0) continue;                                   // (a mesh whose claim failed has status 3)
        const unsigned char cls = edge_class(held[s], fwd[s]);
        bits |= cls;
        const int at_lo = (int)(3 * f + (up ? k : k1)), at_hi = (int)(3 * f + (up ? k1 : k));
        const int r0 = rep[2 * s], r1 = rep[2 * s + 1];
        if (r0 == at_lo) {
          own[0] += 1;
          own[1] += cls == DISN_CHECK_FLAG_BOUNDARY;
          own[2] += cls == DISN_CHECK_FLAG_NONMANIFOLD;
          own[3] += cls == DISN_CHECK_FLAG_MISORIENTED;
        }
        if (r0 >= 0 && r0 < corners) unite(parent, at_lo, r0);
        if (r1 >= 0 && r1 < corners) unite(parent, at_hi, r1);
      }
      fstate[f] = F_PART | bits;
    }
    wave_add(counts, b, DISN_CHECK_EDGES, own[0]);
    wave_add(counts, b, DISN_CHECK_BOUNDARY_EDGES, own[1]);
    wave_add(counts, b, DISN_CHECK_NONMANIFOLD_EDGES, own[2]);
    wave_add(counts, b, DISN_CHECK_MISORIENTED_EDGES, own[3]);
  }
}

__global__ __launch_bounds__(kThreads) void fan_count_kernel(const int* __restrict__ faces,
                                                             const long long* __restrict__ voff,
                                                             const long long* __restrict__ foff, int B,
                                                             long long corners, const int* __restrict__ status,
                                                             const unsigned char* __restrict__ fstate, int* parent,
                                                             unsigned* fans) {
  GRID_STRIDE(c, corners) {
    const long long f = c / 3;
    const int b = mesh_of(foff, B, f);
    if (!topo_ok(status[b]) || !(fstate[f] & F_PART)) continue;
    if (find_root(parent, (int)c) == (int)c) atomicAdd(&fans[voff[b] + faces[c]], 1u);
  }
}

__global__ __launch_bounds__(kThreads) void vertex_tally_kernel(const long long* __restrict__ voff, int B, long long nv,
                                                                const int* __restrict__ status,
                                                                const unsigned char* __restrict__ ref,
                                                                const unsigned* __restrict__ fans, long long* counts) {
  WAVE_STRIDE(v, nv, live) {
    const int b = live ? mesh_of(voff, B, v) : 0;
    const bool ok = live && topo_ok(status[b]);
    wave_add(counts, b, DISN_CHECK_UNREFERENCED_VERTICES, ok && !ref[v]);
    wave_add(counts, b, DISN_CHECK_NONMANIFOLD_VERTICES, ok && fans[v] >= 2u);
  }
}

// ---- geometry ----------------------------------------------------------------------------------------------------
struct Tri { double p[3][3]; };

__device__ __forceinline__ Tri load_tri(const float* __restrict__ verts, const int* __restrict__ faces, long long v0,
                                        long long f) {
  Tri t;
  for (int k = 0; k < 3; ++k) {
    const long long v = v0 + faces[3 * f + k];
    for (int a = 0; a < 3; ++a) t.p[k][a] = (double)verts[3 * v + a];
  }
  return t;
}

__global__ __launch_bounds__(kThreads) void face_geometry_kernel(const float* __restrict__ verts,
                                                                 const int* __restrict__ faces,
                                                                 const long long* __restrict__ voff,
                                                                 const long long* __restrict__ foff, int B,
                                                                 long long nf, const int* __restrict__ status,
                                                                 unsigned char* fstate, double* __restrict__ term,
                                                                 float* __restrict__ fbox, unsigned* mbox,
                                                                 unsigned long long* extent, long long* counts) {
  WAVE_STRIDE(f, nf, live) {
    const int b = live ? mesh_of(foff, B, f) : 0;
    unsigned long long flat = 0, ext = 0;
    unsigned blo[3] = {0, 0, 0}, bhi[3] = {0, 0, 0};
    const bool has = live && status[b] == 0 && (fstate[f] & F_PART);
    if (has) {
      const Tri t = load_tri(verts, faces, voff[b], f);
      const double* p0 = t.p[0]; const double* p1 = t.p[1]; const double* p2 = t.p[2];
      const double u[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
      const double w[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
      const double c0 = u[1] * w[2] - u[2] * w[1], c1 = u[2] * w[0] - u[0] * w[2], c2 = u[0] * w[1] - u[1] * w[0];
      if (c0 == 0.0 && c1 == 0.0 && c2 == 0.0) {
        flat = 1;
        fstate[f] |= DISN_CHECK_FLAG_DEGENERATE;
      }
      term[2 * f] = 0.5 * sqrt((c0 * c0 + c1 * c1) + c2 * c2);
      const double d0 = p1[1] * p2[2] - p1[2] * p2[1], d1 = p1[2] * p2[0] - p1[0] * p2[2],
                   d2 = p1[0] * p2[1] - p1[1] * p2[0];
      term[2 * f + 1] = ((p0[0] * d0 + p0[1] * d1) + p0[2] * d2) / 6.0;
      float widest = 0.0f;
      for (int a = 0; a < 3; ++a) {
        const float lo = fminf(fminf((float)p0[a], (float)p1[a]), (float)p2[a]);
        const float hi = fmaxf(fmaxf((float)p0[a], (float)p1[a]), (float)p2[a]);
        fbox[6 * f + a] = lo;
        fbox[6 * f + 3 + a] = hi;
        blo[a] = ordered_of(lo);
        bhi[a] = ordered_of(hi);
        widest = fmaxf(widest, hi - lo);
      }
      ext = (unsigned long long)fmin((double)widest * kExtScale, kExtMax);
    }
    wave_box(mbox, b, has, blo, bhi);
    wave_add(counts, b, DISN_CHECK_ZERO_AREA_FACES, flat);
    wave_add(reinterpret_cast<long long*>(extent), b, 0, ext);       // (a table of one field: see extent_at)
  }
}

// extent is laid out [B][NF] as counts is, field 0: wave_add serves both
__device__ __forceinline__ unsigned long long extent_at(const unsigned long long* extent, int b) {
  return extent[(long long)b * NF];
}

// one thread per mesh: cells of twice the mean face extent over the mesh's box, at most kMaxGrid per axis
__global__ __launch_bounds__(kThreads) void grid_kernel(const long long* __restrict__ foff, int B,
                                                        const int* __restrict__ status,
                                                        const long long* __restrict__ counts,
                                                        const unsigned* __restrict__ mbox,
                                                        const unsigned long long* __restrict__ extent, Grid* grid) {
  GRID_STRIDE(b, B) {
    Grid g;
    for (int a = 0; a < 3; ++a) { g.lo[a] = 0.0; g.g[a] = 1; }
    g.inv_h = 0.0;
    const long long part = foff[b + 1] - foff[b] - counts[b * NF + DISN_CHECK_INDEX_DEGENERATE_FACES];
    const unsigned long long sum = extent_at(extent, (int)b);
    if (status[b] == 0 && part > 0 && sum > 0) {
      const double h = 2.0 * ((double)sum / (double)part) / kExtScale;
      g.inv_h = 1.0 / h;
      for (int a = 0; a < 3; ++a) {
        g.lo[a] = (double)float_of(mbox[6 * b + a]);
        const double cells = floor(((double)float_of(mbox[6 * b + 3 + a]) - g.lo[a]) * g.inv_h) + 1.0;
        g.g[a] = cells >= (double)kMaxGrid ? kMaxGrid : cells >= 1.0 ? (int)cells : 1;
      }
    }
    grid[b] = g;
  }
}

// monotone in x: boxes that overlap on an axis have overlapping cell ranges there
__device__ __forceinline__ int cell_of(const Grid& g, int a, float x) {
  const double c = floor(((double)x - g.lo[a]) * g.inv_h);
  return c >= (double)(g.g[a] - 1) ? g.g[a] - 1 : c >= 0.0 ? (int)c : 0;
}

// ---- bins --------------------------------------------------------------------------------------------------------
// FILL false: count a face in its cells, or list it as large; true: write it into its cells' rows
template <bool FILL>
__global__ __launch_bounds__(kThreads) void bin_kernel(const long long* __restrict__ foff, int B, long long nf,
                                                       int* status, unsigned char* fstate,
                                                       const float* __restrict__ fbox, const Grid* __restrict__ grid,
                                                       unsigned long long* ckeys, unsigned long long cmask,
                                                       unsigned* ccnt, const unsigned* __restrict__ crow,
                                                       unsigned* ccur, unsigned* ent_face, unsigned* ent_slot,
                                                       unsigned long long ent_cap, unsigned* nlarge, unsigned* large,
                                                       unsigned long long* work) {
  WAVE_STRIDE(f, nf, live) {
    const int b = live ? mesh_of(foff, B, f) : 0;
    unsigned long long brute = 0;
    if (live && status[b] == 0 && (fstate[f] & F_PART) && !(FILL && (fstate[f] & F_LARGE))) {
      const Grid g = grid[b];
      int lo[3], hi[3];
      for (int a = 0; a < 3; ++a) {
        lo[a] = cell_of(g, a, fbox[6 * f + a]);
        hi[a] = cell_of(g, a, fbox[6 * f + 3 + a]);
      }
      const long long span = (long long)(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1);
      if (span > kMaxSpan) {                                   // (FILL never comes here: the face is marked)
        if (!FILL) {
          fstate[f] |= F_LARGE;
          const unsigned at = atomicAdd(nlarge, 1u);
          if ((long long)at < nf) large[at] = (unsigned)f;
          brute = (unsigned long long)(foff[b + 1] - foff[b]);
        }
      } else {
        for (int z = lo[2]; z <= hi[2]; ++z)
          for (int y = lo[1]; y <= hi[1]; ++y)
            for (int x = lo[0]; x <= hi[0]; ++x) {
              const unsigned long long key = (unsigned long long)b << 32 | (unsigned)(x | y << 10 | z << 20);
              if (!FILL) {
                const long long s = table_claim(ckeys, cmask, key);
                if (s < 0) { atomicMax(&status[b], (int)ST_TABLE); continue; }
                atomicAdd(&ccnt[s], 1u);
              } else {
                const long long s = table_find(ckeys, cmask, key);
                if (s < 0) continue;
                const unsigned long long e = (unsigned long long)crow[s] + atomicAdd(&ccur[s], 1u);
                if (e < ent_cap) {
                  ent_face[e] = (unsigned)f;
                  ent_slot[e] = (unsigned)s;
                }
              }
            }
      }
    }
    if (!FILL) wave_add(reinterpret_cast<long long*>(work), b, 0, brute);
  }
}

// the work of the pair passes: n (n - 1) / 2 per cell (the large faces' nf_b each are in already)
__global__ __launch_bounds__(kThreads) void work_kernel(const unsigned long long* __restrict__ ckeys,
                                                        const unsigned* __restrict__ ccnt, long long slots, int B,
                                                        unsigned long long* work) {
  WAVE_STRIDE(s, slots, live) {
    const unsigned long long key = live ? ckeys[s] : kEmptyKey;
    const bool cell = key != kEmptyKey && (long long)(key >> 32) < B;
    const unsigned long long n = cell ? ccnt[s] : 0;
    wave_add(reinterpret_cast<long long*>(work), cell ? (int)(key >> 32) : 0, 0, n * (n - (n ? 1 : 0)) / 2);
  }
}

// status 8 before the candidates are counted (PASS 0: the work estimate) and before the narrow phase (PASS 1: the count)
template <int PASS>
__global__ __launch_bounds__(kThreads) void cap_kernel(int B, const long long* __restrict__ cap,
                                                       const unsigned long long* __restrict__ work,
                                                       const long long* __restrict__ counts, int* status,
                                                       unsigned char* tripped) {
  GRID_STRIDE(b, B) {
    if (status[b] != 0) continue;
    const unsigned long long limit = (unsigned long long)cap[b];
    if (PASS == 0) {
      const unsigned long long w = work[b * NF];
      if (limit < (1ull << 59) && w > DISN_CHECK_WORK_FACTOR * limit + 4096) {      // (a larger cap never trips)
        status[b] = ST_PAIRS;
        tripped[b] = 1;
      }
    } else if ((unsigned long long)counts[b * NF + DISN_CHECK_CANDIDATE_PAIRS] > limit) {
      status[b] = ST_PAIRS;
    }
  }
}

// ---- pairs -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool boxes_meet(const float* __restrict__ fbox, long long f, long long g) {
  bool meet = true;
  for (int a = 0; a < 3; ++a)
    meet &= fbox[6 * f + a] <= fbox[6 * g + 3 + a] && fbox[6 * g + a] <= fbox[6 * f + 3 + a];
  return meet;
}

__device__ __forceinline__ double orient(const double* a, const double* b, const double* c, const double* d) {
  const double u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
  const double v[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  const double w[3] = {d[0] - a[0], d[1] - a[1], d[2] - a[2]};
  return (u[0] * (v[1] * w[2] - v[2] * w[1]) - u[1] * (v[0] * w[2] - v[2] * w[0])) + u[2] * (v[0] * w[1] - v[1] * w[0]);
}

// an edge of P goes through the inside of T
__device__ __forceinline__ bool pierces(const Tri& P, const Tri& T) {
  const double* a = T.p[0]; const double* b = T.p[1]; const double* c = T.p[2];
  bool hit = false;
  for (int k = 0; k < 3; ++k) {
    const double* p = P.p[k];
    const double* q = P.p[k == 2 ? 0 : k + 1];
    const bool across = orient(a, b, c, p) * orient(a, b, c, q) < 0.0;
    const double s1 = orient(p, q, a, b), s2 = orient(p, q, b, c), s3 = orient(p, q, c, a);
    hit |= across && ((s1 > 0.0 && s2 > 0.0 && s3 > 0.0) || (s1 < 0.0 && s2 < 0.0 && s3 < 0.0));
  }
  return hit;
}

// the pair (f, g), boxes known to meet: NARROW false -> a candidate; true -> the rule, and the marks
template <bool NARROW>
__device__ __forceinline__ unsigned pair_test(const float* __restrict__ verts, const int* __restrict__ faces,
                                                        long long v0, const Tri& tf, long long f, long long g,
                                                        unsigned char* imark) {
  if (!NARROW) return 1;
  const Tri tg = load_tri(verts, faces, v0, g);
  if (!(pierces(tf, tg) || pierces(tg, tf))) return 0;
  imark[f] = 1;                                                // the one value any thread stores here
  imark[g] = 1;
  return 1;
}

// one thread per row entry: the entries behind it in the row, each pair in the one cell that owns it
template <bool NARROW>
__global__ __launch_bounds__(kThreads) void cell_pairs_kernel(const float* __restrict__ verts,
                                                              const int* __restrict__ faces,
                                                              const long long* __restrict__ voff, int B,
                                                              const int* __restrict__ status,
                                                              const float* __restrict__ fbox,
                                                              const Grid* __restrict__ grid,
                                                              const unsigned long long* __restrict__ ckeys,
                                                              const unsigned* __restrict__ ccnt,
                                                              const unsigned* __restrict__ crow, long long slots,
                                                              const unsigned* __restrict__ ent_face,
                                                              const unsigned* __restrict__ ent_slot,
                                                              const unsigned long long* __restrict__ total,
                                                              unsigned long long ent_cap, long long nf,
                                                              unsigned char* imark, unsigned* pcount) {
  const unsigned long long n_ent = *total < ent_cap ? *total : ent_cap;
  GRID_STRIDE(e, (long long)n_ent) {
    const long long s = ent_slot[e];
    if (s < slots) {
      const unsigned long long key = ckeys[s];
      const int b = (int)(key >> 32);
      const long long f = ent_face[e];
      if (key != kEmptyKey && b < B && status[b] == 0 && f < nf) {
        unsigned found = 0;
        const Grid g = grid[b];
        const int cell[3] = {(int)(key & 1023), (int)(key >> 10 & 1023), (int)(key >> 20 & 1023)};
        int flo[3];
        for (int a = 0; a < 3; ++a) flo[a] = cell_of(g, a, fbox[6 * f + a]);
        Tri tf;
        if (NARROW) tf = load_tri(verts, faces, voff[b], f);
        unsigned long long end = (unsigned long long)crow[s] + ccnt[s];
        if (end > n_ent) end = n_ent;
        for (unsigned long long e2 = (unsigned long long)e + 1; e2 < end; ++e2) {
          const long long h = ent_face[e2];
          if (h >= nf || h == f || !boxes_meet(fbox, f, h)) continue;
          bool owner = true;
          for (int a = 0; a < 3; ++a) {
            const int hlo = cell_of(g, a, fbox[6 * h + a]);
            owner &= (flo[a] > hlo ? flo[a] : hlo) == cell[a];
          }
          if (owner) found += pair_test<NARROW>(verts, faces, voff[b], tf, f, h, imark);
        }
        if (found) atomicAdd(&pcount[f], found);               // the rows lie in hash order: the tally is per face
      }
    }
  }
}

// one thread per large face: every face of its mesh that is not large, and the large ones behind it
template <bool NARROW>
__global__ __launch_bounds__(kThreads) void large_pairs_kernel(const float* __restrict__ verts,
                                                               const int* __restrict__ faces,
                                                               const long long* __restrict__ voff,
                                                               const long long* __restrict__ foff, int B, long long nf,
                                                               const int* __restrict__ status,
                                                               const unsigned char* __restrict__ fstate,
                                                               const float* __restrict__ fbox,
                                                               const unsigned* __restrict__ nlarge,
                                                               const unsigned* __restrict__ large,
                                                               unsigned char* imark, unsigned* pcount) {
  const long long n = (long long)*nlarge < nf ? (long long)*nlarge : nf;
  GRID_STRIDE(i, n) {
    const long long f = large[i];
    if (f < nf) {
      const int b = mesh_of(foff, B, f);
      if (status[b] == 0) {
        unsigned found = 0;
        Tri tf;
        if (NARROW) tf = load_tri(verts, faces, voff[b], f);
        for (long long h = foff[b]; h < foff[b + 1]; ++h) {
          const unsigned char st = fstate[h];
          if (h == f || !(st & F_PART) || ((st & F_LARGE) && h < f) || !boxes_meet(fbox, f, h)) continue;
          found += pair_test<NARROW>(verts, faces, voff[b], tf, f, h, imark);
        }
        if (found) atomicAdd(&pcount[f], found);
      }
    }
  }
}

// the pairs found at every face, in face order: one 64-bit add per wave
__global__ __launch_bounds__(kThreads) void pair_tally_kernel(const long long* __restrict__ foff, int B, long long nf,
                                                              const unsigned* __restrict__ pcount, int field,
                                                              long long* counts) {
  WAVE_STRIDE(f, nf, live) {
    wave_add(counts, live ? mesh_of(foff, B, f) : 0, field, live ? pcount[f] : 0u);
  }
}

// ---- finish ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void face_finish_kernel(const long long* __restrict__ foff, int B, long long nf,
                                                               const int* __restrict__ status,
                                                               const unsigned char* __restrict__ fstate,
                                                               const unsigned char* __restrict__ imark,
                                                               unsigned char* face_flags, long long* counts) {
  WAVE_STRIDE(f, nf, live) {
    const int b = live ? mesh_of(foff, B, f) : 0;
    const int st = live ? status[b] : (int)ST_INDEX;
    const bool hit = st == 0 && imark[f];
    if (live && face_flags)
      face_flags[f] = topo_ok(st) ? (unsigned char)((fstate[f] & F_PUBLIC) | (hit ? DISN_CHECK_FLAG_INTERSECTS : 0)) : 0;
    wave_add(counts, b, DISN_CHECK_INTERSECTING_FACES, hit);
  }
}

// block b SLABS + s: slab s of mesh b, both terms; thread t adds the slab's faces t, t + 256, .. then a binary tree
__global__ __launch_bounds__(kThreads) void slab_sum_kernel(const long long* __restrict__ foff,
                                                            const double* __restrict__ term,
                                                            double* __restrict__ partial) {
  __shared__ double tree[2][kThreads];
  const int s = blockIdx.x % SLABS, b = blockIdx.x / SLABS, t = threadIdx.x;
  const long long n = foff[b + 1] - foff[b];
  const long long lo = foff[b] + s * n / SLABS, hi = foff[b] + (s + 1) * n / SLABS;
  double a = 0.0, v = 0.0;
  for (long long f = lo + t; f < hi; f += kThreads) {
    a += term[2 * f];
    v += term[2 * f + 1];
  }
  tree[0][t] = a;
  tree[1][t] = v;
  __syncthreads();
  for (int o = kThreads / 2; o; o >>= 1) {
    if (t < o) {
      tree[0][t] += tree[0][t + o];
      tree[1][t] += tree[1][t + o];
    }
    __syncthreads();
  }
  if (t == 0) {
    partial[2 * ((long long)b * SLABS + s)] = tree[0][0];
    partial[2 * ((long long)b * SLABS + s) + 1] = tree[1][0];
  }
}

// one thread per mesh: the slabs in order, the derived fields, -1 for what the status makes invalid
__global__ __launch_bounds__(kThreads) void mesh_finish_kernel(const long long* __restrict__ voff,
                                                               const long long* __restrict__ foff, int B,
                                                               const int* __restrict__ status,
                                                               const unsigned char* __restrict__ tripped,
                                                               const double* __restrict__ partial, long long* counts,
                                                               double* sums) {
  GRID_STRIDE(b, B) {
    long long* c = counts + b * NF;
    const long long nv = voff[b + 1] - voff[b], nf = foff[b + 1] - foff[b];
    const int st = status[b];
    c[DISN_CHECK_NV] = nv;
    c[DISN_CHECK_NF] = nf;
    c[DISN_CHECK_EULER] = (nv - c[DISN_CHECK_UNREFERENCED_VERTICES]) - c[DISN_CHECK_EDGES] +
                          (nf - c[DISN_CHECK_INDEX_DEGENERATE_FACES]);
    double a = 0.0, v = 0.0;
    for (int s = 0; s < SLABS; ++s) {
      a += partial[2 * (b * SLABS + s)];
      v += partial[2 * (b * SLABS + s) + 1];
    }
    const bool geometry = st == 0 || st == ST_PAIRS;
    sums[2 * b] = geometry ? a : 0.0;
    sums[2 * b + 1] = geometry ? v : 0.0;
    if (!topo_ok(st))
      for (int k = DISN_CHECK_UNREFERENCED_VERTICES; k <= DISN_CHECK_EULER; ++k) c[k] = -1;
    if (!geometry) c[DISN_CHECK_ZERO_AREA_FACES] = -1;
    if (!geometry || tripped[b]) c[DISN_CHECK_CANDIDATE_PAIRS] = -1;
    if (st != 0) c[DISN_CHECK_INTERSECTING_PAIRS] = c[DISN_CHECK_INTERSECTING_FACES] = -1;
  }
}

// ---- host side -------------------------------------------------------------------------------------------------
struct CheckWs {
  long long *voff, *foff, *cap;                    // [B+1], [B+1], [B]
  Grid* grid;                                      // [B]
  unsigned* mbox;                                  // [B][6]
  double* partial;                                 // [B][SLABS][2]
  // ---- one zeroed block
  unsigned long long *extent, *work;               // [B][NF] each, field 0 (the layout wave_add serves)
  unsigned char* tripped;                          // [B]
  unsigned *nlarge;                                // [1]
  unsigned char *ref;                              // [nv]
  unsigned* fans;                                  // [nv]
  unsigned char *fstate, *imark;                   // [nf]
  unsigned *pcount, *icount;                       // [nf] the candidate and the intersecting pairs found at a face
  double* term;                                    // [nf][2]
  unsigned *held, *fwd;                            // [T]
  unsigned *ccnt, *ccur;                           // [Tc]
  size_t zero_bytes;
  // ----
  unsigned long long *keys, *ckeys;                // [T], [Tc]
  unsigned long long T, Tc, ent_cap;
  int* rep;                                        // [T][2]
  int* parent;                                     // [3 nf]
  float* fbox;                                     // [nf][6]
  unsigned *crow, *bsum;                           // [Tc]
  unsigned long long* total;                       // [1]
  unsigned *ent_face, *ent_slot;                   // [8 nf]
  unsigned* large;                                 // [nf]
  size_t total_bytes;
};

CheckWs check_layout(void* ws, int B, long long nv, long long nf) {
  WsCursor c(ws);
  const size_t b1 = (size_t)B + 1, f = (size_t)(nf > 0 ? nf : 1), v = (size_t)(nv > 0 ? nv : 1);
  CheckWs w;
  w.voff = c.take<long long>(b1); w.foff = c.take<long long>(b1); w.cap = c.take<long long>(b1);
  w.grid = c.take<Grid>(b1);
  w.mbox = c.take<unsigned>(6 * b1);
  w.partial = c.take<double>(2 * SLABS * b1);
  unsigned long long T = 16, Tc = 16;
  while (T < 6ull * f) T <<= 1;                    // at most 3 nf edges: at most half full
  while (Tc < 2ull * kMaxSpan * f) Tc <<= 1;       // at most 8 nf entries: at most half full
  w.T = T; w.Tc = Tc; w.ent_cap = (unsigned long long)kMaxSpan * f;
  const size_t z0 = c.next();
  w.extent = c.take<unsigned long long>(NF * b1); w.work = c.take<unsigned long long>(NF * b1);
  w.tripped = c.take<unsigned char>(b1);
  w.nlarge = c.take<unsigned>(1);
  w.ref = c.take<unsigned char>(v);
  w.fans = c.take<unsigned>(v);
  w.fstate = c.take<unsigned char>(f); w.imark = c.take<unsigned char>(f);
  w.pcount = c.take<unsigned>(f); w.icount = c.take<unsigned>(f);
  w.term = c.take<double>(2 * f);
  w.held = c.take<unsigned>(T); w.fwd = c.take<unsigned>(T);
  w.ccnt = c.take<unsigned>(Tc); w.ccur = c.take<unsigned>(Tc);
  w.zero_bytes = c.off - z0;
  w.keys = c.take<unsigned long long>(T); w.ckeys = c.take<unsigned long long>(Tc);
  w.rep = c.take<int>(2 * T);
  w.parent = c.take<int>(3 * f);
  w.fbox = c.take<float>(6 * f);
  w.crow = c.take<unsigned>(Tc);
  w.bsum = c.take<unsigned>(scan_bsum_items(Tc));
  w.total = c.take<unsigned long long>(1);
  w.ent_face = c.take<unsigned>(w.ent_cap); w.ent_slot = c.take<unsigned>(w.ent_cap);
  w.large = c.take<unsigned>(f);
  w.total_bytes = c.next();
  return w;
}

inline bool check_limits_ok(int B, int64_t nv, int64_t nf) {
  return mesh_limits_ok(B, nv, nf) && nf <= DISN_CHECK_MAX_FACES;
}

}  // namespace
}  // namespace disn

using namespace disn;

extern "C" size_t disn_mesh_check_workspace_bytes(int B, int64_t nv_total, int64_t nf_total, int64_t max_pairs_total) {
  if (!check_limits_ok(B, nv_total, nf_total) || max_pairs_total < 0) return 0;
  return check_layout(nullptr, B, nv_total, nf_total).total_bytes;
}

extern "C" int disn_mesh_check_batch(const float* verts, const int32_t* faces, const int64_t* v_off_host,
                                     const int64_t* f_off_host, int B, const int64_t* max_pairs_host, int64_t* counts,
                                     double* sums, uint8_t* face_flags, int32_t* status, void* ws, size_t ws_bytes,
                                     void* stream) {
  static_assert(sizeof(long long) == sizeof(int64_t), "the counts travel as int64");
  if (!offsets_ok(v_off_host, f_off_host, B) || !max_pairs_host || !counts || !sums || !status || !ws) return DISN_E_ARG;
  const int64_t nv = v_off_host[B], nf = f_off_host[B];
  if ((nv > 0 && !verts) || (nf > 0 && !faces)) return DISN_E_ARG;
  for (int b = 0; b < B; ++b)
    if (max_pairs_host[b] < 0) return DISN_E_ARG;
  if (!check_limits_ok(B, nv, nf)) return DISN_E_SHAPE;
  if (ws_bytes < check_layout(nullptr, B, nv, nf).total_bytes) return DISN_E_WS;
  hipStream_t st = (hipStream_t)stream;
  const CheckWs w = check_layout(ws, B, nv, nf);
  long long* cnt = reinterpret_cast<long long*>(counts);
  MESH_TRY(upload_offsets(w.voff, w.foff, v_off_host, f_off_host, B, st));
  MESH_TRY(hipMemcpyAsync(w.cap, max_pairs_host, (size_t)B * 8, hipMemcpyHostToDevice, st));
  MESH_TRY(hipMemsetAsync(status, 0, (size_t)B * 4, st));
  MESH_TRY(hipMemsetAsync(counts, 0, (size_t)B * NF * 8, st));
  MESH_TRY(hipMemsetAsync(w.extent, 0, w.zero_bytes, st));
  MESH_TRY(hipMemsetAsync(w.partial, 0, (size_t)B * SLABS * 16, st));
  MESH_LAUNCH(init_kernel, 6ll * B, w.mbox, B);
  if (nf > 0) {
    const long long corners = 3 * nf;
    MESH_LAUNCH(validate_faces_kernel, nf, faces, w.voff, w.foff, B, nf, status);
    if (nv > 0) MESH_LAUNCH(validate_verts_kernel, nv, verts, w.voff, B, nv, status);
    // topology
    MESH_TRY(hipMemsetAsync(w.keys, 0xFF, w.T * 8, st));
    MESH_TRY(hipMemsetAsync(w.rep, 0x7F, w.T * 8, st));          // above every corner: 3 nf <= 3 2^27
    MESH_LAUNCH(init_parent_kernel, corners, w.parent, corners);
    MESH_LAUNCH(edge_claim_kernel, nf, faces, w.voff, w.foff, B, nf, status, w.keys, w.T - 1, w.held, w.fwd, w.rep,
                w.ref, w.fstate, cnt);
    MESH_LAUNCH(fan_union_kernel, nf, faces, w.voff, w.foff, B, nf, status, w.keys, w.T - 1, w.held, w.fwd, w.rep,
                corners, w.fstate, w.parent, cnt);
    MESH_LAUNCH(fan_count_kernel, corners, faces, w.voff, w.foff, B, corners, status, w.fstate, w.parent, w.fans);
  } else if (nv > 0) {
    MESH_LAUNCH(validate_verts_kernel, nv, verts, w.voff, B, nv, status);
  }
  if (nv > 0) MESH_LAUNCH(vertex_tally_kernel, nv, w.voff, B, nv, status, w.ref, w.fans, cnt);
  if (nf > 0) {
    // geometry and bins
    MESH_LAUNCH(face_geometry_kernel, nf, verts, faces, w.voff, w.foff, B, nf, status, w.fstate, w.term, w.fbox, w.mbox,
                w.extent, cnt);
    MESH_LAUNCH(grid_kernel, B, w.foff, B, status, cnt, w.mbox, w.extent, w.grid);
    MESH_TRY(hipMemsetAsync(w.ckeys, 0xFF, w.Tc * 8, st));
    MESH_LAUNCH(bin_kernel<false>, nf, w.foff, B, nf, status, w.fstate, w.fbox, w.grid, w.ckeys, w.Tc - 1, w.ccnt,
                w.crow, w.ccur, w.ent_face, w.ent_slot, w.ent_cap, w.nlarge, w.large, w.work);
    MESH_TRY(exclusive_scan(w.ccnt, w.crow, (size_t)w.Tc, w.bsum, w.total, st));
    MESH_LAUNCH(bin_kernel<true>, nf, w.foff, B, nf, status, w.fstate, w.fbox, w.grid, w.ckeys, w.Tc - 1, w.ccnt,
                w.crow, w.ccur, w.ent_face, w.ent_slot, w.ent_cap, w.nlarge, w.large, w.work);
    MESH_LAUNCH(work_kernel, (long long)w.Tc, w.ckeys, w.ccnt, (long long)w.Tc, B, w.work);
    MESH_LAUNCH(cap_kernel<0>, B, B, w.cap, w.work, cnt, status, w.tripped);
    // pairs: the candidates of every mesh still in order, then the rule for those within their cap
    const long long ents = (long long)w.ent_cap;
    MESH_LAUNCH(cell_pairs_kernel<false>, ents, verts, faces, w.voff, B, status, w.fbox, w.grid, w.ckeys, w.ccnt, w.crow,
                (long long)w.Tc, w.ent_face, w.ent_slot, w.total, w.ent_cap, nf, w.imark, w.pcount);
    MESH_LAUNCH(large_pairs_kernel<false>, nf, verts, faces, w.voff, w.foff, B, nf, status, w.fstate, w.fbox, w.nlarge,
                w.large, w.imark, w.pcount);
    MESH_LAUNCH(pair_tally_kernel, nf, w.foff, B, nf, w.pcount, DISN_CHECK_CANDIDATE_PAIRS, cnt);
    MESH_LAUNCH(cap_kernel<1>, B, B, w.cap, w.work, cnt, status, w.tripped);
    MESH_LAUNCH(cell_pairs_kernel<true>, ents, verts, faces, w.voff, B, status, w.fbox, w.grid, w.ckeys, w.ccnt, w.crow,
                (long long)w.Tc, w.ent_face, w.ent_slot, w.total, w.ent_cap, nf, w.imark, w.icount);
    MESH_LAUNCH(large_pairs_kernel<true>, nf, verts, faces, w.voff, w.foff, B, nf, status, w.fstate, w.fbox, w.nlarge,
                w.large, w.imark, w.icount);
    MESH_LAUNCH(pair_tally_kernel, nf, w.foff, B, nf, w.icount, DISN_CHECK_INTERSECTING_PAIRS, cnt);
    MESH_LAUNCH(face_finish_kernel, nf, w.foff, B, nf, status, w.fstate, w.imark, face_flags, cnt);
    hipLaunchKernelGGL(slab_sum_kernel, dim3((unsigned)B * SLABS), dim3(kThreads), 0, st, w.foff, w.term, w.partial);
    MESH_TRY(hipGetLastError());
  }
  MESH_LAUNCH(mesh_finish_kernel, B, w.voff, w.foff, B, status, w.tripped, w.partial, cnt, sums);
  return 0;
}

// Repair of meshes to a manifold on the device (include/repair/disn_amd_repair.h; the rule is disn_amd/postprocess.py
// repair_arrays, restated here operation by operation): B meshes back to back, as the meshers and the other mesh stages
// leave them.
//
//   count   validate indices and coordinates -> weld: every vertex claims the slot of its POSITION (96 bits and the
//           mesh; the slot holds the smallest vertex seen, a probe compares the positions themselves) -> drop: every
//           face without a repeated welded index claims the slot of its sorted TRIPLE (the slot holds the smallest face
//           and, by atomicOr, the orientations seen) -> the survivors claim their three undirected edges (64-bit keys,
//           table_claim): a slot counts its corner pairs and keeps the smallest and the largest -> the pairs of the
//           singular edges are gathered into rows (the counts in the slots, ONE scan, fill) -> one thread per singular
//           edge sorts its row (<= 16 corner pairs, local memory) and evaluates the rank rule; partner[] holds every
//           pair's partner pair -> union over corners, the pinch pass (one thread per stitched edge), init_parent,
//           union again -> the roots; the flags of the referenced vertices, the kept faces and the further classes;
//           three scans -> [B][12] counts
//   emit    the referenced vertices in vertex order, the further classes in corner order, the kept faces in face order:
//           each element's place is its scan value; nothing is sorted
//
// NO KERNEL WAITS FOR ANOTHER WORKGROUP.  The loops whose trip count depends on other threads: the probes of the three
// tables (at most `mask + 1` steps each; a full table raises status 3: the position table has two slots per vertex, the
// triple table two per face, the edge table two per possible edge), find_root (strictly downwards) and unite
// (mesh_batch.hpp).  The loops of the rank rule and of the pinch pass run over a row of at most DISN_REPAIR_MAX_FAN
// entries.  NO FLOATING-POINT ATOMIC.  Everything written is a function of integers and of the signs of the float64
// determinants below.  Compiled with -ffp-contract=off: they round as numpy's do.
#include "mesh_batch.hpp"

#include "../../include/repair/disn_amd_repair.h"

namespace disn {
namespace {

enum { NF = DISN_REPAIR_FIELDS, MAXFAN = DISN_REPAIR_MAX_FAN };
constexpr int kFree = 0x7F7F7F7F;                   // a slot of an element table, a vertex without a corner (memset 0x7F)
enum : unsigned char { E_STITCHED = 1, E_PINCHED = 2 };

__device__ __forceinline__ void tally_add(unsigned long long* tally, int b, int field) {
  atomicAdd(&tally[(long long)b * NF + field], 1ull);
}

// ---- weld --------------------------------------------------------------------------------------------------------
// the bits of x + 0.0f for a finite x: -0 becomes +0, nothing else changes
__device__ __forceinline__ unsigned coord_bits(float x) {
  const unsigned u = __float_as_uint(x);
  return u == 0x80000000u ? 0u : u;
}

__device__ __forceinline__ bool same_position(const float* __restrict__ verts, long long v, long long w) {
  return coord_bits(verts[3 * v]) == coord_bits(verts[3 * w]) && coord_bits(verts[3 * v + 1]) == coord_bits(verts[3 * w + 1]) &&
         coord_bits(verts[3 * v + 2]) == coord_bits(verts[3 * w + 2]);
}

__device__ __forceinline__ unsigned long long position_hash(const float* __restrict__ verts, long long v, int b) {
  const unsigned long long xy = (unsigned long long)coord_bits(verts[3 * v]) << 32 | coord_bits(verts[3 * v + 1]);
  return mix64(mix64(xy) ^ ((unsigned long long)b << 32 | coord_bits(verts[3 * v + 2])));
}

// every vertex into the slot of its position: the slot keeps the smallest vertex of the group.  A slot never becomes
// free again, and every vertex it ever holds has the one position, so the comparison does not depend on when it is made
__global__ __launch_bounds__(kThreads) void weld_insert_kernel(const float* __restrict__ verts,
                                                               const long long* __restrict__ voff, int B, long long nv,
                                                               int* status, int* vslot, unsigned long long mask,
                                                               unsigned* __restrict__ vat) {
  GRID_STRIDE(v, nv) {
    const int b = mesh_of(voff, B, v);
    if (status[b]) continue;
    unsigned long long h = position_hash(verts, v, b) & mask;
    bool done = false;
    for (unsigned long long probe = 0; probe <= mask && !done; ++probe) {
      int cur = __atomic_load_n(&vslot[h], __ATOMIC_RELAXED);
      if (cur == kFree) {
        cur = atomicCAS(&vslot[h], kFree, (int)v);
        if (cur == kFree) cur = (int)v;
      }
      if ((long long)cur >= voff[b] && (long long)cur < voff[b + 1] && same_position(verts, cur, v)) {
        atomicMin(&vslot[h], (int)v);
        vat[v] = (unsigned)h;
        done = true;
      } else {
        h = (h + 1) & mask;
      }
    }
    if (!done) atomicMax(&status[b], (int)ST_TABLE);
  }
}

// rep[v]: the batch-global vertex v stands for
__global__ __launch_bounds__(kThreads) void weld_rep_kernel(const long long* __restrict__ voff, int B, long long nv,
                                                            const int* __restrict__ status, int weld,
                                                            const int* __restrict__ vslot,
                                                            const unsigned* __restrict__ vat, int* __restrict__ rep,
                                                            unsigned long long* tally) {
  GRID_STRIDE(v, nv) {
    int r = (int)v;
    if (weld) {
      const int b = mesh_of(voff, B, v);
      if (!status[b] && vat[v] != kNone) {
        const int s = vslot[vat[v]];
        if ((long long)s >= voff[b] && s < r) {
          r = s;
          tally_add(tally, b, DISN_REPAIR_WELDED_VERTICES);
        }
      }
    }
    rep[v] = r;
  }
}

// ---- drop --------------------------------------------------------------------------------------------------------
struct Triple {
  int g[3];           // the welded batch-global indices in face order
  int s[3];           // sorted
  bool repeated, even;
};

__device__ __forceinline__ Triple triple_of(const int* __restrict__ faces, const int* __restrict__ rep, long long v0,
                                            long long f) {
  Triple t;
  for (int k = 0; k < 3; ++k) t.g[k] = rep[v0 + faces[3 * f + k]];
  t.repeated = t.g[0] == t.g[1] || t.g[1] == t.g[2] || t.g[2] == t.g[0];
  t.even = ((t.g[0] < t.g[1]) + (t.g[1] < t.g[2]) + (t.g[2] < t.g[0])) == 2;
  int a = t.g[0], b = t.g[1], c = t.g[2], x;
  if (a > b) { x = a; a = b; b = x; }
  if (b > c) { x = b; b = c; c = x; }
  if (a > b) { x = a; a = b; b = x; }
  t.s[0] = a; t.s[1] = b; t.s[2] = c;
  return t;
}

// every face without a repeated index into the slot of its sorted triple: the smallest face, the orientations seen
__global__ __launch_bounds__(kThreads) void face_insert_kernel(const int* __restrict__ faces,
                                                               const long long* __restrict__ voff,
                                                               const long long* __restrict__ foff, int B, long long nf,
                                                               int* status, const int* __restrict__ rep, int* tslot,
                                                               unsigned* tbits, unsigned long long mask,
                                                               unsigned* __restrict__ fat, unsigned long long* tally) {
  GRID_STRIDE(f, nf) {
    const int b = mesh_of(foff, B, f);
    if (status[b]) continue;                                   // so every index below lies in [0, nv_b)
    const Triple t = triple_of(faces, rep, voff[b], f);
    if (t.repeated) {
      tally_add(tally, b, DISN_REPAIR_REPEATED_FACES);
      continue;
    }
    unsigned long long h = mix64(mix64((unsigned long long)t.s[0] << 32 | (unsigned)t.s[1]) ^ (unsigned)t.s[2]) & mask;
    bool done = false;
    for (unsigned long long probe = 0; probe <= mask && !done; ++probe) {
      int cur = __atomic_load_n(&tslot[h], __ATOMIC_RELAXED);
      if (cur == kFree) {
        cur = atomicCAS(&tslot[h], kFree, (int)f);
        if (cur == kFree) cur = (int)f;
      }
      bool same = cur == (int)f;
      if (!same && (long long)cur >= foff[b] && (long long)cur < foff[b + 1]) {      // (global indices: one mesh only)
        const Triple u = triple_of(faces, rep, voff[b], cur);
        same = !u.repeated && u.s[0] == t.s[0] && u.s[1] == t.s[1] && u.s[2] == t.s[2];
      }
      if (same) {
        atomicMin(&tslot[h], (int)f);
        atomicOr(&tbits[h], t.even ? 1u : 2u);
        fat[f] = (unsigned)h;
        done = true;
      } else {
        h = (h + 1) & mask;
      }
    }
    if (!done) atomicMax(&status[b], (int)ST_TABLE);
  }
}

__global__ __launch_bounds__(kThreads) void face_class_kernel(const long long* __restrict__ foff, int B, long long nf,
                                                              const int* __restrict__ status,
                                                              const int* __restrict__ tslot,
                                                              const unsigned* __restrict__ tbits,
                                                              const unsigned* __restrict__ fat,
                                                              unsigned char* __restrict__ keep,
                                                              unsigned long long* tally) {
  GRID_STRIDE(f, nf) {
    const int b = mesh_of(foff, B, f);
    if (status[b] || fat[f] == kNone) continue;
    const unsigned h = fat[f];
    if (tbits[h] == 3u) tally_add(tally, b, DISN_REPAIR_PILLOW_FACES);
    else if (tslot[h] != (int)f) tally_add(tally, b, DISN_REPAIR_DUPLICATE_FACES);
    else keep[f] = 1;
  }
}

// ---- edges -------------------------------------------------------------------------------------------------------
// corner pair c = 3 f + k runs from index k of face f to index (k+1)%3
__global__ __launch_bounds__(kThreads) void edge_insert_kernel(const int* __restrict__ faces,
                                                               const long long* __restrict__ voff,
                                                               const long long* __restrict__ foff, int B, long long nf,
                                                               int* status, const int* __restrict__ rep,
                                                               const unsigned char* __restrict__ keep,
                                                               unsigned long long* keys, unsigned long long mask,
                                                               unsigned* held, int* pmin, int* pmax,
                                                               unsigned* __restrict__ eat, int* first) {
  GRID_STRIDE(f, nf) {
    const int b = mesh_of(foff, B, f);
    if (status[b] || !keep[f]) continue;
    const Triple t = triple_of(faces, rep, voff[b], f);
    for (int k = 0; k < 3; ++k) {
      const int i = t.g[k], j = t.g[k == 2 ? 0 : k + 1], c = (int)(3 * f + k);
      atomicMin(&first[i], c);
      const unsigned long long lo = (unsigned long long)(i < j ? i : j), hi = (unsigned long long)(i < j ? j : i);
      const long long s = table_claim(keys, mask, lo << 32 | hi);           // hi < 2^31: never kEmptyKey
      if (s < 0) { atomicMax(&status[b], (int)ST_TABLE); continue; }
      atomicAdd(&held[s], 1u);
      atomicMin(&pmin[s], c);
      atomicMax(&pmax[s], c);
      eat[c] = (unsigned)s;
    }
  }
}

__global__ __launch_bounds__(kThreads) void row_count_kernel(const unsigned* __restrict__ held, long long slots,
                                                             unsigned* __restrict__ rowcnt) {
  GRID_STRIDE(s, slots) rowcnt[s] = held[s] >= 3u ? held[s] : 0u;
}

// the partner of every pair on a regular edge; the pairs of the singular edges into their rows
__global__ __launch_bounds__(kThreads) void row_fill_kernel(long long corners, const unsigned* __restrict__ eat,
                                                            const unsigned* __restrict__ held,
                                                            const int* __restrict__ pmin, const int* __restrict__ pmax,
                                                            const unsigned* __restrict__ rowoff, unsigned* rowcur,
                                                            unsigned* __restrict__ ent, int* __restrict__ partner) {
  GRID_STRIDE(c, corners) {
    const unsigned s = eat[c];
    if (s == kNone) continue;
    if (held[s] == 2u) {
      partner[c] = pmin[s] == (int)c ? pmax[s] : pmin[s];
    } else if (held[s] >= 3u) {
      const long long at = (long long)rowoff[s] + atomicAdd(&rowcur[s], 1u);
      if (at < corners) ent[at] = (unsigned)c;
    }
  }
}

// ---- the angular rule ----------------------------------------------------------------------------------------------
__device__ __forceinline__ void cross3(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ double det3(const double* a, const double* b, const double* c) {
  return (a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0])) + a[2] * (b[0] * c[1] - b[1] * c[0]);
}

// the row of slot s, ascending; false when it is not a row the rule may read
__device__ __forceinline__ bool load_row(const unsigned* __restrict__ ent, long long corners, unsigned off, int k,
                                         const unsigned char* __restrict__ keep, int* c) {
  if ((long long)off + k > corners) return false;
  for (int m = 0; m < k; ++m) {
    const unsigned x = ent[off + m];
    if ((long long)x >= corners || !keep[x / 3]) return false;
    int at = m;
    for (; at > 0 && c[at - 1] > (int)x; --at) c[at] = c[at - 1];           // insertion: k <= MAXFAN
    c[at] = (int)x;
  }
  return true;
}

// one thread per singular edge
__global__ __launch_bounds__(kThreads) void stitch_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                          const long long* __restrict__ voff,
                                                          const long long* __restrict__ foff, int B, long long corners,
                                                          const int* __restrict__ status, const int* __restrict__ rep,
                                                          const unsigned char* __restrict__ keep,
                                                          const unsigned long long* __restrict__ keys, long long slots,
                                                          const unsigned* __restrict__ held,
                                                          const unsigned* __restrict__ rowoff,
                                                          const unsigned* __restrict__ ent, int stitch,
                                                          int* __restrict__ partner, unsigned char* __restrict__ estate,
                                                          unsigned long long* tally) {
  GRID_STRIDE(s, slots) {
    if (held[s] < 3u) continue;
    const unsigned long long key = keys[s];
    const long long lo = (long long)(key >> 32), hi = (long long)(key & 0xFFFFFFFFull);
    const int b = mesh_of(voff, B, lo);
    if (status[b]) continue;
    tally_add(tally, b, DISN_REPAIR_SINGULAR_EDGES);
    const int k = (int)held[s];
    if (!stitch || (k & 1) || held[s] > (unsigned)MAXFAN) continue;
    int c[MAXFAN];
    if (!load_row(ent, corners, rowoff[s], k, keep, c)) continue;
    const long long v0 = voff[b];
    double e[3], d[MAXFAN][3];
    bool fwd[MAXFAN];
    for (int a = 0; a < 3; ++a) e[a] = (double)verts[3 * hi + a] - (double)verts[3 * lo + a];
    for (int m = 0; m < k; ++m) {
      const long long f = c[m] / 3;
      const int kk = c[m] % 3;
      const long long from = rep[v0 + faces[3 * f + kk]], opp = rep[v0 + faces[3 * f + (kk + 2) % 3]];
      fwd[m] = from == lo;
      for (int a = 0; a < 3; ++a) d[m][a] = (double)verts[3 * opp + a] - (double)verts[3 * lo + a];
    }
    double er[3];
    cross3(e, d[0], er);
    int half[MAXFAN], at[MAXFAN];
    bool ok = true;
    half[0] = 0;
    for (int m = 1; m < k && ok; ++m) {
      double ed[3];
      cross3(e, d[m], ed);
      const double sm = det3(e, d[0], d[m]), cm = dot3(er, ed);
      if (sm > 0.0 || (sm == 0.0 && cm > 0.0)) half[m] = 0;
      else if (sm < 0.0 || (sm == 0.0 && cm < 0.0)) half[m] = 1;
      else ok = false;
    }
    if (!ok) continue;
    for (int m = 0; m < k; ++m) at[m] = -1;
    at[0] = 0;                                                  // the reference: rank 0
    for (int m = 1; m < k && ok; ++m) {
      int before = 1;
      for (int n = 1; n < k; ++n)
        if (n != m && (half[n] < half[m] || (half[n] == half[m] && det3(e, d[n], d[m]) > 0.0))) ++before;
      if (before >= k || at[before] >= 0) ok = false;           // no permutation
      else at[before] = m;
    }
    for (int q = 0; q < k && ok; ++q) ok = fwd[at[q]] != fwd[at[q + 1 == k ? 0 : q + 1]];
    if (!ok) continue;
    for (int q = 0; q < k; ++q) {
      if (fwd[at[q]]) continue;
      const int m = at[q], n = at[q + 1 == k ? 0 : q + 1];
      partner[c[m]] = c[n];
      partner[c[n]] = c[m];
    }
    estate[s] = E_STITCHED;
    tally_add(tally, b, DISN_REPAIR_STITCHED_EDGES);
  }
}

// ---- split -------------------------------------------------------------------------------------------------------
// the corners of pair c at the smaller and at the larger welded index of its edge
__device__ __forceinline__ void pair_ends(const int* __restrict__ faces, const int* __restrict__ rep, long long v0,
                                          int c, int* at_lo, int* at_hi) {
  const int f = c / 3, k = c % 3, k1 = k == 2 ? 0 : k + 1;
  const bool up = rep[v0 + faces[3 * f + k]] < rep[v0 + faces[3 * f + k1]];
  *at_lo = 3 * f + (up ? k : k1);
  *at_hi = 3 * f + (up ? k1 : k);
}

__global__ __launch_bounds__(kThreads) void corner_union_kernel(const int* __restrict__ faces,
                                                                const long long* __restrict__ voff,
                                                                const long long* __restrict__ foff, int B,
                                                                long long corners, const int* __restrict__ rep,
                                                                const int* __restrict__ partner, int* parent) {
  GRID_STRIDE(c, corners) {
    const int p = partner[c];
    if (p <= (int)c || (long long)p >= corners) continue;       // each pair of partners once
    const long long v0 = voff[mesh_of(foff, B, c / 3)];
    int a0, a1, b0, b1;
    pair_ends(faces, rep, v0, (int)c, &a0, &a1);
    pair_ends(faces, rep, v0, p, &b0, &b1);
    unite(parent, a0, b0);
    unite(parent, a1, b1);
  }
}

// one thread per stitched edge: two of its pairs with one (class at lo, class at hi) -> the edge is cut
__global__ __launch_bounds__(kThreads) void pinch_kernel(const int* __restrict__ faces,
                                                         const long long* __restrict__ voff, int B, long long corners,
                                                         const int* __restrict__ rep,
                                                         const unsigned char* __restrict__ keep,
                                                         const unsigned long long* __restrict__ keys, long long slots,
                                                         const unsigned* __restrict__ held,
                                                         const unsigned* __restrict__ rowoff,
                                                         const unsigned* __restrict__ ent, int* parent,
                                                         int* __restrict__ partner, unsigned char* __restrict__ estate,
                                                         unsigned long long* tally) {
  GRID_STRIDE(s, slots) {
    if (estate[s] != E_STITCHED) continue;
    const int k = (int)held[s];
    if (k > MAXFAN) continue;
    int c[MAXFAN];
    if (!load_row(ent, corners, rowoff[s], k, keep, c)) continue;
    const long long lo = (long long)(keys[s] >> 32);
    const int b = mesh_of(voff, B, lo);
    const long long v0 = voff[b];
    int sig[MAXFAN][2], n = 0;
    for (int m = 0; m < k; ++m) {
      int a0, a1;
      pair_ends(faces, rep, v0, c[m], &a0, &a1);
      if (a0 == c[m]) continue;                                 // runs lo -> hi: its partner speaks for the pair
      sig[n][0] = find_root(parent, a0);
      sig[n][1] = find_root(parent, a1);
      ++n;
    }
    bool pinched = false;
    for (int i = 0; i < n; ++i)
      for (int j = i + 1; j < n; ++j) pinched |= sig[i][0] == sig[j][0] && sig[i][1] == sig[j][1];
    if (!pinched) continue;
    for (int m = 0; m < k; ++m) partner[c[m]] = -1;
    estate[s] = E_PINCHED;
    tally_add(tally, b, DISN_REPAIR_PINCHED_EDGES);
  }
}

// ---- numbering ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void root_kernel(long long corners, const unsigned char* __restrict__ keep,
                                                        int* parent, int* __restrict__ croot) {
  GRID_STRIDE(c, corners) croot[c] = keep[c / 3] ? find_root(parent, (int)c) : -1;
}

// a mesh with a status keeps every vertex and every face, and gains nothing
__global__ __launch_bounds__(kThreads) void vertex_flag_kernel(const long long* __restrict__ voff, int B, long long nv,
                                                               const int* __restrict__ status,
                                                               const int* __restrict__ first,
                                                               unsigned* __restrict__ vref) {
  GRID_STRIDE(v, nv) vref[v] = (status[mesh_of(voff, B, v)] || first[v] != kFree) ? 1u : 0u;
}

__global__ __launch_bounds__(kThreads) void face_flag_kernel(const int* __restrict__ faces,
                                                             const long long* __restrict__ voff,
                                                             const long long* __restrict__ foff, int B, long long nf,
                                                             const int* __restrict__ status,
                                                             const int* __restrict__ rep,
                                                             const unsigned char* __restrict__ keep,
                                                             const int* __restrict__ first,
                                                             const int* __restrict__ croot,
                                                             unsigned* __restrict__ fkeep, unsigned* __restrict__ extra) {
  GRID_STRIDE(f, nf) {
    const int b = mesh_of(foff, B, f);
    const bool bad = status[b] != 0;
    fkeep[f] = (bad || keep[f]) ? 1u : 0u;
    for (int k = 0; k < 3; ++k) {
      const long long c = 3 * f + k;
      unsigned x = 0;
      if (!bad && keep[f] && croot[c] == (int)c) {
        const int head = first[rep[voff[b] + faces[c]]];        // the vertex's smallest corner: of a kept face
        x = croot[head] != (int)c ? 1u : 0u;
      }
      extra[c] = x;
    }
  }
}

struct MeshBase {
  long long v, f, x;          // the scan values at the mesh's first vertex, face and corner
  long long nref;             // its referenced vertices
  long long vseg, fseg;       // where its vertices and faces go in the outputs
};

// one thread: B is a handful
__global__ void finish_kernel(const long long* __restrict__ voff, const long long* __restrict__ foff, int B,
                              long long nv, long long nf, const int* __restrict__ status,
                              const unsigned* __restrict__ vscan, const unsigned* __restrict__ fscan,
                              const unsigned* __restrict__ xscan, const unsigned long long* __restrict__ totals,
                              const unsigned long long* __restrict__ tally, MeshBase* __restrict__ base,
                              long long* __restrict__ counts) {
  if (blockIdx.x || threadIdx.x) return;
  auto vb = [&](int m) { return (m < B && voff[m] < nv) ? (long long)vscan[voff[m]] : (long long)totals[0]; };
  auto fb = [&](int m) { return (m < B && foff[m] < nf) ? (long long)fscan[foff[m]] : (long long)totals[1]; };
  auto xb = [&](int m) { return (m < B && foff[m] < nf) ? (long long)xscan[3 * foff[m]] : (long long)totals[2]; };
  long long vseg = 0, fseg = 0;
  for (int b = 0; b < B; ++b) {
    const long long nref = vb(b + 1) - vb(b), nkeep = fb(b + 1) - fb(b), nextra = xb(b + 1) - xb(b);
    base[b] = MeshBase{vb(b), fb(b), xb(b), nref, vseg, fseg};
    long long* c = counts + (long long)b * NF;
    const bool ok = status[b] == 0;
    for (int k = 0; k < NF; ++k) c[k] = ok ? (long long)tally[(long long)b * NF + k] : 0;
    c[DISN_REPAIR_NV_OUT] = nref + nextra;
    c[DISN_REPAIR_NF_OUT] = nkeep;
    c[DISN_REPAIR_STATUS] = status[b];
    c[DISN_REPAIR_ADDED_VERTICES] = nextra;
    c[DISN_REPAIR_DROPPED_VERTICES] = (voff[b + 1] - voff[b]) - nref;
    vseg += nref + nextra;
    fseg += nkeep;
  }
}

// ---- emit --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void emit_verts_kernel(const float* __restrict__ verts,
                                                              const long long* __restrict__ voff, int B, long long nv,
                                                              const unsigned* __restrict__ vref,
                                                              const unsigned* __restrict__ vscan,
                                                              const MeshBase* __restrict__ base, long long n_out,
                                                              float* __restrict__ verts_out, int* __restrict__ vmap_out) {
  GRID_STRIDE(v, nv) {
    if (!vref[v]) continue;
    const int b = mesh_of(voff, B, v);
    const long long at = base[b].vseg + ((long long)vscan[v] - base[b].v);
    if (at < 0 || at >= n_out) continue;                        // (cannot happen: counts and scans agree)
    for (int a = 0; a < 3; ++a) verts_out[3 * at + a] = verts[3 * v + a];
    vmap_out[at] = (int)(v - voff[b]);
  }
}

__global__ __launch_bounds__(kThreads) void emit_extra_kernel(const float* __restrict__ verts,
                                                              const int* __restrict__ faces,
                                                              const long long* __restrict__ voff,
                                                              const long long* __restrict__ foff, int B,
                                                              long long corners, const int* __restrict__ rep,
                                                              const unsigned* __restrict__ extra,
                                                              const unsigned* __restrict__ xscan,
                                                              const MeshBase* __restrict__ base, long long n_out,
                                                              float* __restrict__ verts_out, int* __restrict__ vmap_out) {
  GRID_STRIDE(c, corners) {
    if (!extra[c]) continue;                                    // so the face is kept and its mesh has no status
    const int b = mesh_of(foff, B, c / 3);
    const long long v = rep[voff[b] + faces[c]];
    const long long at = base[b].vseg + base[b].nref + ((long long)xscan[c] - base[b].x);
    if (at < 0 || at >= n_out) continue;
    for (int a = 0; a < 3; ++a) verts_out[3 * at + a] = verts[3 * v + a];
    vmap_out[at] = (int)(v - voff[b]);
  }
}

__global__ __launch_bounds__(kThreads) void emit_faces_kernel(const int* __restrict__ faces,
                                                              const long long* __restrict__ voff,
                                                              const long long* __restrict__ foff, int B, long long nf,
                                                              const int* __restrict__ status,
                                                              const int* __restrict__ rep, const int* __restrict__ first,
                                                              const int* __restrict__ croot,
                                                              const unsigned* __restrict__ fkeep,
                                                              const unsigned* __restrict__ fscan,
                                                              const unsigned* __restrict__ vscan,
                                                              const unsigned* __restrict__ xscan,
                                                              const MeshBase* __restrict__ base, long long n_out,
                                                              int* __restrict__ faces_out, int* __restrict__ kept_out) {
  GRID_STRIDE(f, nf) {
    if (!fkeep[f]) continue;
    const int b = mesh_of(foff, B, f);
    const long long at = base[b].fseg + ((long long)fscan[f] - base[b].f);
    if (at < 0 || at >= n_out) continue;
    kept_out[at] = (int)(f - foff[b]);
    for (int k = 0; k < 3; ++k) {
      const long long c = 3 * f + k;
      int idx = faces[c];                                       // a mesh with a status: as it came
      if (!status[b]) {
        const long long v = rep[voff[b] + faces[c]];
        const int r = croot[c];
        idx = croot[first[v]] == r ? (int)((long long)vscan[v] - base[b].v)
                                   : (int)(base[b].nref + ((long long)xscan[r] - base[b].x));
      }
      faces_out[3 * at + k] = idx;
    }
  }
}

// ---- host side -------------------------------------------------------------------------------------------------
struct RepairWs {
  long long *voff, *foff;                          // [B+1]
  MeshBase* base;                                  // [B]
  // ---- zeroed
  int* status;                                     // [B]
  unsigned long long* tally;                       // [B][NF]
  unsigned long long* totals;                      // [4]: referenced vertices, kept faces, further classes, row entries
  unsigned char* keep;                             // [nf]
  unsigned *held, *rowcur;                         // [Te]
  int* pmax;                                       // [Te]
  unsigned char* estate;                           // [Te]
  unsigned* tbits;                                 // [Tf]
  size_t zero_bytes;
  // ---- 0x7F: free slots, no corner yet
  int *vslot, *tslot, *pmin, *first;               // [Tv], [Tf], [Te], [nv]
  size_t free_bytes;
  // ---- 0xFF: empty keys, kNone, no partner
  unsigned long long* keys;                        // [Te]
  unsigned *vat, *fat, *eat;                       // [nv], [nf], [3 nf]: the slot of a vertex, a face, a corner pair
  int* partner;                                    // [3 nf]
  size_t none_bytes;
  // ----
  unsigned long long Tv, Tf, Te;
  int *rep, *parent, *croot;                       // [nv], [3 nf], [3 nf]
  unsigned *rowcnt, *rowoff, *ent;                 // [Te], [Te], [3 nf]
  unsigned *vref, *vscan, *fkeep, *fscan, *extra, *xscan;   // [nv] x 2, [nf] x 2, [3 nf] x 2
  unsigned* bsum;
  size_t total;
};

RepairWs repair_layout(void* ws, int B, long long nv, long long nf) {
  WsCursor c(ws);
  const size_t b1 = (size_t)B + 1, f = (size_t)(nf > 0 ? nf : 1), v = (size_t)(nv > 0 ? nv : 1);
  RepairWs w;
  w.Tv = table_size(v); w.Tf = table_size(f); w.Te = table_size(3 * f);
  w.voff = c.take<long long>(b1); w.foff = c.take<long long>(b1);
  w.base = c.take<MeshBase>(b1);
  const size_t z0 = c.next();
  w.status = c.take<int>(b1);
  w.tally = c.take<unsigned long long>(NF * b1);
  w.totals = c.take<unsigned long long>(4);
  w.keep = c.take<unsigned char>(f);
  w.held = c.take<unsigned>(w.Te); w.rowcur = c.take<unsigned>(w.Te);
  w.pmax = c.take<int>(w.Te);
  w.estate = c.take<unsigned char>(w.Te);
  w.tbits = c.take<unsigned>(w.Tf);
  w.zero_bytes = c.off - z0;
  const size_t f0 = c.next();
  w.vslot = c.take<int>(w.Tv); w.tslot = c.take<int>(w.Tf); w.pmin = c.take<int>(w.Te); w.first = c.take<int>(v);
  w.free_bytes = c.off - f0;
  const size_t n0 = c.next();
  w.keys = c.take<unsigned long long>(w.Te);
  w.vat = c.take<unsigned>(v); w.fat = c.take<unsigned>(f); w.eat = c.take<unsigned>(3 * f);
  w.partner = c.take<int>(3 * f);
  w.none_bytes = c.off - n0;
  w.rep = c.take<int>(v); w.parent = c.take<int>(3 * f); w.croot = c.take<int>(3 * f);
  w.rowcnt = c.take<unsigned>(w.Te); w.rowoff = c.take<unsigned>(w.Te); w.ent = c.take<unsigned>(3 * f);
  w.vref = c.take<unsigned>(v); w.vscan = c.take<unsigned>(v);
  w.fkeep = c.take<unsigned>(f); w.fscan = c.take<unsigned>(f);
  w.extra = c.take<unsigned>(3 * f); w.xscan = c.take<unsigned>(3 * f);
  const size_t longest = (size_t)w.Te > v ? (size_t)w.Te : v;
  w.bsum = c.take<unsigned>(scan_bsum_items(longest));
  w.total = c.next();
  return w;
}

int count_run(const float* verts, const int* faces, const int64_t* v_off, const int64_t* f_off, int B, int flags,
              long long* counts, void* ws_ptr, hipStream_t st) {
  const long long nv = v_off[B], nf = f_off[B], corners = 3 * nf;
  const RepairWs w = repair_layout(ws_ptr, B, nv, nf);
  const int weld = (flags & DISN_REPAIR_WELD) != 0, stitch = (flags & DISN_REPAIR_STITCH) != 0;
  MESH_TRY(upload_offsets(w.voff, w.foff, v_off, f_off, B, st));
  MESH_TRY(hipMemsetAsync(w.status, 0, w.zero_bytes, st));
  MESH_TRY(hipMemsetAsync(w.vslot, 0x7F, w.free_bytes, st));
  MESH_TRY(hipMemsetAsync(w.keys, 0xFF, w.none_bytes, st));
  if (nf > 0) MESH_LAUNCH(validate_faces_kernel, nf, faces, w.voff, w.foff, B, nf, w.status);
  if (nv > 0) {
    MESH_LAUNCH(validate_verts_kernel, nv, verts, w.voff, B, nv, w.status);
    if (weld) MESH_LAUNCH(weld_insert_kernel, nv, verts, w.voff, B, nv, w.status, w.vslot, w.Tv - 1, w.vat);
    MESH_LAUNCH(weld_rep_kernel, nv, w.voff, B, nv, w.status, weld, w.vslot, w.vat, w.rep, w.tally);
  }
  if (nf > 0) {
    const long long slots = (long long)w.Te;
    MESH_LAUNCH(face_insert_kernel, nf, faces, w.voff, w.foff, B, nf, w.status, w.rep, w.tslot, w.tbits, w.Tf - 1, w.fat,
                w.tally);
    MESH_LAUNCH(face_class_kernel, nf, w.foff, B, nf, w.status, w.tslot, w.tbits, w.fat, w.keep, w.tally);
    MESH_LAUNCH(edge_insert_kernel, nf, faces, w.voff, w.foff, B, nf, w.status, w.rep, w.keep, w.keys, w.Te - 1, w.held,
                w.pmin, w.pmax, w.eat, w.first);
    MESH_LAUNCH(row_count_kernel, slots, w.held, slots, w.rowcnt);
    MESH_TRY(exclusive_scan(w.rowcnt, w.rowoff, (size_t)slots, w.bsum, w.totals + 3, st));
    MESH_LAUNCH(row_fill_kernel, corners, corners, w.eat, w.held, w.pmin, w.pmax, w.rowoff, w.rowcur, w.ent, w.partner);
    MESH_LAUNCH(stitch_kernel, slots, verts, faces, w.voff, w.foff, B, corners, w.status, w.rep, w.keep, w.keys, slots,
                w.held, w.rowoff, w.ent, stitch, w.partner, w.estate, w.tally);
    MESH_LAUNCH(init_parent_kernel, corners, w.parent, corners);
    MESH_LAUNCH(corner_union_kernel, corners, faces, w.voff, w.foff, B, corners, w.rep, w.partner, w.parent);
    MESH_LAUNCH(pinch_kernel, slots, faces, w.voff, B, corners, w.rep, w.keep, w.keys, slots, w.held, w.rowoff, w.ent,
                w.parent, w.partner, w.estate, w.tally);
    MESH_LAUNCH(init_parent_kernel, corners, w.parent, corners);
    MESH_LAUNCH(corner_union_kernel, corners, faces, w.voff, w.foff, B, corners, w.rep, w.partner, w.parent);
    MESH_LAUNCH(root_kernel, corners, corners, w.keep, w.parent, w.croot);
    MESH_LAUNCH(face_flag_kernel, nf, faces, w.voff, w.foff, B, nf, w.status, w.rep, w.keep, w.first, w.croot, w.fkeep,
                w.extra);
    MESH_TRY(exclusive_scan(w.fkeep, w.fscan, (size_t)nf, w.bsum, w.totals + 1, st));
    MESH_TRY(exclusive_scan(w.extra, w.xscan, (size_t)corners, w.bsum, w.totals + 2, st));
  }
  if (nv > 0) {
    MESH_LAUNCH(vertex_flag_kernel, nv, w.voff, B, nv, w.status, w.first, w.vref);
    MESH_TRY(exclusive_scan(w.vref, w.vscan, (size_t)nv, w.bsum, w.totals, st));
  }
  hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(1), 0, st, w.voff, w.foff, B, nv, nf, w.status, w.vscan, w.fscan,
                     w.xscan, w.totals, w.tally, w.base, counts);
  MESH_TRY(hipGetLastError());
  return 0;
}

bool flags_ok(int flags) { return (flags & ~(DISN_REPAIR_WELD | DISN_REPAIR_STITCH)) == 0; }

}  // namespace
}  // namespace disn

using namespace disn;

extern "C" size_t disn_mesh_repair_workspace_bytes(int B, int64_t nv_total, int64_t nf_total) {
  return mesh_limits_ok(B, nv_total, nf_total) ? repair_layout(nullptr, B, nv_total, nf_total).total : 0;
}

extern "C" int disn_mesh_repair_count_batch(const float* verts, const int32_t* faces, const int64_t* v_off_host,
                                            const int64_t* f_off_host, int B, int flags, int64_t* counts, void* ws,
                                            size_t ws_bytes, void* stream) {
  static_assert(sizeof(long long) == sizeof(int64_t), "the counts travel as int64");
  if (!offsets_ok(v_off_host, f_off_host, B) || !counts || !ws || !flags_ok(flags)) return DISN_E_ARG;
  const int64_t nv = v_off_host[B], nf = f_off_host[B];
  if ((nv > 0 && !verts) || (nf > 0 && !faces)) return DISN_E_ARG;
  if (!mesh_limits_ok(B, nv, nf)) return DISN_E_SHAPE;
  if (ws_bytes < repair_layout(nullptr, B, nv, nf).total) return DISN_E_WS;
  return count_run(verts, faces, v_off_host, f_off_host, B, flags, reinterpret_cast<long long*>(counts), ws,
                   (hipStream_t)stream);
}

extern "C" int disn_mesh_repair_emit_batch(const float* verts, const int32_t* faces, const int64_t* v_off_host,
                                           const int64_t* f_off_host, int B, int flags, const int64_t* counts_host,
                                           float* verts_out, int32_t* faces_out, int32_t* vmap_out, int32_t* kept_out,
                                           void* ws, size_t ws_bytes, void* stream) {
  if (!offsets_ok(v_off_host, f_off_host, B) || !counts_host || !ws || !flags_ok(flags)) return DISN_E_ARG;
  const int64_t nv = v_off_host[B], nf = f_off_host[B];
  if (!mesh_limits_ok(B, nv, nf)) return DISN_E_SHAPE;
  if (ws_bytes < repair_layout(nullptr, B, nv, nf).total) return DISN_E_WS;
  long long nvo = 0, nfo = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t* c = counts_host + (size_t)NF * b;
    const int64_t nvb = v_off_host[b + 1] - v_off_host[b], nfb = f_off_host[b + 1] - f_off_host[b];
    const int64_t most = c[DISN_REPAIR_STATUS] ? nvb : 3 * c[DISN_REPAIR_NF_OUT];     // nv_out <= 3 nf_out
    if (c[DISN_REPAIR_NF_OUT] < 0 || c[DISN_REPAIR_NF_OUT] > nfb || c[DISN_REPAIR_NV_OUT] < 0 ||
        c[DISN_REPAIR_NV_OUT] > most)
      return DISN_E_ARG;
    nvo += c[DISN_REPAIR_NV_OUT];
    nfo += c[DISN_REPAIR_NF_OUT];
  }
  if (nvo == 0 && nfo == 0) return 0;
  if ((nvo > 0 && (!verts || !verts_out || !vmap_out)) || (nfo > 0 && (!faces || !faces_out || !kept_out)))
    return DISN_E_ARG;
  if (nvo > 0 && nf > 0 && !faces) return DISN_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  const RepairWs w = repair_layout(ws, B, nv, nf);
  const long long corners = 3 * nf;
  if (nvo > 0) {
    MESH_LAUNCH(emit_verts_kernel, nv, verts, w.voff, B, nv, w.vref, w.vscan, w.base, nvo, verts_out, vmap_out);
    if (nf > 0)
      MESH_LAUNCH(emit_extra_kernel, corners, verts, faces, w.voff, w.foff, B, corners, w.rep, w.extra, w.xscan, w.base,
                  nvo, verts_out, vmap_out);
  }
  if (nfo > 0)
    MESH_LAUNCH(emit_faces_kernel, nf, faces, w.voff, w.foff, B, nf, w.status, w.rep, w.first, w.croot, w.fkeep, w.fscan,
                w.vscan, w.xscan, w.base, nfo, faces_out, kept_out);
  return 0;
}

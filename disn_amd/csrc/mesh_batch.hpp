// The building blocks of the stages that work on "B meshes back to back, with host offsets" (mesh_clean.hip,
// mesh_simplify.hip, mesh_colour.hip, mesh_sample.hip, mesh_smooth.hip, mesh_check.hip, mesh_repair.hip, mesh_close.hip; DESIGN 4z states each block's contract).  Everything has internal linkage: each
// translation unit that includes this keeps its own copy, and no kernel is launched across translation units.  FOR
// THOSE FILES ONLY: the compiler emits a __global__ function whether or not the file launches it, so the workspace
// cursor (WsCursor, scan_bsum_items), which marching_cubes.hip and grid_band.hip use as well, lives in kernels.hpp.
#pragma once

#include "kernels.hpp"

namespace disn {
namespace {

constexpr unsigned long long kEmptyKey = ~0ull;
constexpr unsigned kNone = 0xFFFFFFFFu;
constexpr int kThreads = 256;
// a mesh's status word, part of the C ABI (include/); a stage's own further values stay in its file
enum { ST_INDEX = 2, ST_TABLE = 3, ST_FINITE = 4 };

#define GRID_STRIDE(i, n) \
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (long long)gridDim.x * blockDim.x)

// the mesh of flat element i: the largest b with off[b] <= i (empty meshes are stepped over)
__device__ __forceinline__ int mesh_of(const long long* __restrict__ off, int B, long long i) {
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27; x *= 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

// the slot of `key`, claiming an empty one (*is_new, where asked for: this call claimed it); -1 when `mask + 1`
// probes found neither (table full).  The tables are sized to run at most half full.
__device__ __forceinline__ long long table_claim(unsigned long long* keys, unsigned long long mask,
                                                 unsigned long long key, bool* is_new = nullptr) {
  unsigned long long h = mix64(key) & mask;
  for (unsigned long long probe = 0; probe <= mask; ++probe) {
    const unsigned long long prev = atomicCAS(&keys[h], kEmptyKey, key);
    if (prev == kEmptyKey || prev == key) {
      if (is_new) *is_new = prev == kEmptyKey;
      return (long long)h;
    }
    h = (h + 1) & mask;
  }
  return -1;
}

// the slot of `key` in a table no one writes any more; -1 when it is not there
__device__ __forceinline__ long long table_find(const unsigned long long* __restrict__ keys, unsigned long long mask,
                                                unsigned long long key) {
  unsigned long long h = mix64(key) & mask;
  for (unsigned long long probe = 0; probe <= mask; ++probe) {
    const unsigned long long k = keys[h];
    if (k == key) return (long long)h;
    if (k == kEmptyKey) return -1;
    h = (h + 1) & mask;
  }
  return -1;
}

// a union-find whose parents only decrease (parent[x] <= x, set to x by init_parent_kernel).  find_root follows
// parent[x] < x strictly downwards: at most x steps.  unite retries only when its CAS found parent[a] already lowered by
// someone else, and goes on from that lower value, so the retries of all threads together are bounded.
__device__ __forceinline__ int find_root(int* parent, int x) {
  int p;
  while ((p = __atomic_load_n(&parent[x], __ATOMIC_RELAXED)) != x) x = p;   // p < x
  return x;
}

__device__ __forceinline__ void unite(int* parent, int a, int b) {
  for (;;) {
    a = find_root(parent, a);
    b = find_root(parent, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicCAS(&parent[a], a, b);   // hook the larger root under the smaller
    if (old == a) return;
    a = old;                                       // someone lowered parent[a] first: go on from there
  }
}

__global__ __launch_bounds__(kThreads) void init_parent_kernel(int* __restrict__ parent, long long nf) {
  GRID_STRIDE(f, nf) parent[f] = (int)f;
}

// status 2 for a mesh with an index outside [0, nv_b): the ONLY kernel that looks at an index before it is checked
__global__ __launch_bounds__(kThreads) void validate_faces_kernel(const int* __restrict__ faces,
                                                                  const long long* __restrict__ voff,
                                                                  const long long* __restrict__ foff, int B,
                                                                  long long nf, int* status) {
  GRID_STRIDE(f, nf) {
    const int b = mesh_of(foff, B, f);
    const long long nvb = voff[b + 1] - voff[b];
    bool bad = false;
    for (int k = 0; k < 3; ++k) {
      const int i = faces[3 * f + k];
      bad |= i < 0 || (long long)i >= nvb;
    }
    if (bad) atomicMax(&status[b], (int)ST_INDEX);
  }
}

// status 4 for a mesh with a coordinate that is not finite (mesh_clean.hip has no such check and carries this unlaunched)
__global__ __launch_bounds__(kThreads) void validate_verts_kernel(const float* __restrict__ verts,
                                                                  const long long* __restrict__ voff, int B,
                                                                  long long nv, int* status) {
  GRID_STRIDE(v, nv) {
    const float s = (verts[3 * v] - verts[3 * v]) + (verts[3 * v + 1] - verts[3 * v + 1]) +
                    (verts[3 * v + 2] - verts[3 * v + 2]);          // 0 for finite coordinates, NaN otherwise
    if (!(s == 0.0f)) atomicMax(&status[mesh_of(voff, B, v)], (int)ST_FINITE);
  }
}

// ---- host side -------------------------------------------------------------------------------------------------
inline int blocks_for(long long n) {
  long long b = (n + kThreads - 1) / kThreads;
  if (b > 16384) b = 16384;
  return (int)(b < 1 ? 1 : b);
}

// the slots of a table of `entries` keys or elements: a power of two, at most half full
inline unsigned long long table_size(size_t entries) {
  unsigned long long T = 16;
  while (T < 2ull * entries) T <<= 1;
  return T;
}

// inside a function that returns the hipError_t as an int and has the stream in `st`
#define MESH_TRY(expr)                    \
  do {                                    \
    hipError_t _e = (expr);               \
    if (_e != hipSuccess) return (int)_e; \
  } while (0)
#define MESH_LAUNCH(kernel, n, ...)                                                               \
  do {                                                                                            \
    hipLaunchKernelGGL(kernel, dim3(blocks_for(n)), dim3(kThreads), 0, st, __VA_ARGS__);          \
    MESH_TRY(hipGetLastError());                                                                  \
  } while (0)

// the offsets a caller hands in: ascending from 0
inline bool offsets_ok(const int64_t* v_off, const int64_t* f_off, int B) {
  if (!v_off || !f_off || B < 1 || v_off[0] != 0 || f_off[0] != 0) return false;
  for (int b = 0; b < B; ++b)
    if (v_off[b + 1] < v_off[b] || f_off[b + 1] < f_off[b]) return false;
  return true;
}
// what the kernels' index arithmetic holds: vertex ids and 3 nf corners are int32
inline bool mesh_limits_ok(int B, int64_t nv, int64_t nf) {
  return B >= 1 && nv >= 0 && nf >= 0 && nf <= INT32_MAX / 3 && nv <= INT32_MAX;
}

inline hipError_t upload_offsets(long long* voff, long long* foff, const int64_t* v_off_host,
                                 const int64_t* f_off_host, int B, hipStream_t st) {
  static_assert(sizeof(long long) == sizeof(int64_t), "offsets travel as int64");
  const size_t bytes = ((size_t)B + 1) * 8;
  const hipError_t e = hipMemcpyAsync(voff, v_off_host, bytes, hipMemcpyHostToDevice, st);
  return e != hipSuccess ? e : hipMemcpyAsync(foff, f_off_host, bytes, hipMemcpyHostToDevice, st);
}

}  // namespace
}  // namespace disn

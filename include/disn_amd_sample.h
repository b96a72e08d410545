/*
 * disn_amd_sample.h -- area-weighted surface samples of device meshes, with the face normal and the face of every
 * sample: the fourth header of libdisn_amd.so.  Conventions, error codes and DISN_ABI_VERSION are those of disn_amd.h,
 * which this header includes and leaves as it is; the entries below are additions to the same library.
 *
 * B meshes back to back as disn_mc_emit_batch, disn_mesh_clean_emit_batch and disn_mesh_simplify_emit_batch leave them:
 * verts [sum nv][3], faces [sum nf][3] int32 with indices LOCAL to their mesh, v_off_host / f_off_host [B+1] int64
 * ascending from 0; limits as disn_mesh_clean_*: sum nf <= INT32_MAX/3, sum nv <= INT32_MAX; 1 <= n <= 2^20 samples per
 * mesh (disn_mesh_sample_workspace_bytes is 0 beyond them).  seeds_host [B] uint64: one seed per mesh.
 *
 * THE RULE is metrics.sample_surface_arrays (disn_amd/metrics.py), restated operation by operation.  The choice of the
 * face is integer arithmetic and float64 + - x / only (mesh_sample.hip is compiled without contraction): no step rests
 * on the rounding of a library sqrt or on the order of a sum.
 *   weight    corners a, b, c as float64; e1 = b - a, e2 = c - a; N = e1 x e2 = (e1.y e2.z - e1.z e2.y,
 *             e1.z e2.x - e1.x e2.z, e1.x e2.y - e1.y e2.x); s = (N.x^2 + N.y^2) + N.z^2; smax the largest s of the mesh
 *             (unsigned integer atomic max of the bits of the non-negative double: independent of the order);
 *             q = isqrt(floor((s / smax) 2^62)), the exact integer square root, in [0, 2^31].  A degenerate face, and
 *             one of less than about 2^-31 of the largest area, has q = 0 and is never drawn.
 *   cum       the inclusive sum of q in uint64 (<= nf 2^31 < 2^63; an integer sum: one flat scan over the call's faces,
 *             a mesh subtracts its base); total = cum of the mesh's last face
 *   words     r(i, k) = mix64(seed + 0x9E3779B97F4A7C15 (2 i + k + 1)) mod 2^64, k in {0, 1}, for sample i (SplitMix64;
 *             mix64: x ^= x >> 30, x *= 0xbf58476d1ce4e5b9, x ^= x >> 27, x *= 0x94d049bb133111eb, x ^ (x >> 31)):
 *             a mesh's samples depend on its seed and on itself, never on its companions, its place, B or n
 *   face      target = (r(i,0) total) >> 64 (128-bit product); the first face with cum > target
 *   point     u1 = (r(i,1) >> 40) 2^-24, u2 = ((r(i,1) >> 16) & 0xFFFFFF) 2^-24, t = sqrtf(u1), float32:
 *             p = ((1 - t) A + (t (1 - u2)) B) + (t u2) C
 *   normal    N / sqrt(s) in float64, rounded to float32: the face normal of corners a, b, c in that order
 *
 *   disn_mesh_sample_batch  points [B][n][3] float32, normals [B][n][3] float32 or NULL, face_idx [B][n] int32 (local
 *       to the mesh) or NULL, status [B] int32 (device).
 *   status: 0 ok; 2 a face index outside [0, nv_b) (the first kernel compares every index with its mesh's size, every
 *       later one skips that mesh: nothing is addressed through an unchecked index); 4 a vertex coordinate that is
 *       not finite; 6 (DISN_SAMPLE_NO_AREA) nothing to sample: no faces, or smax == 0.  A mesh with a status gets
 *       zeros in all three outputs and leaves its neighbours as they are.
 * No kernel waits for another workgroup; the scan is three passes (blocks, block sums, add), no look-back; every loop
 * is bounded (the grid stride; the block sums of one call; 32 steps of the binary search); there is no floating-point
 * atomic; no host synchronisation and no read-back.  The host arrays must stay valid until the stream has passed the
 * call.
 */
#ifndef DISN_AMD_SAMPLE_H
#define DISN_AMD_SAMPLE_H

#include "disn_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DISN_SAMPLE_MAX_N 1048576
#define DISN_SAMPLE_NO_AREA 6

size_t disn_mesh_sample_workspace_bytes(int B, int64_t nv_total, int64_t nf_total, int n);
int disn_mesh_sample_batch(const float* verts, const int32_t* faces, const int64_t* v_off_host,
                           const int64_t* f_off_host, int B, const uint64_t* seeds_host, int n, float* points,
                           float* normals, int32_t* face_idx, int32_t* status, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DISN_AMD_SAMPLE_H */

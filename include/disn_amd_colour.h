/*
 * disn_amd_colour.h -- vertex colours of reconstructed meshes from their input views, and depth maps of device meshes
 * without a BVH: the third header of libdisn_amd.so.  Conventions, error codes and DISN_ABI_VERSION are those of
 * disn_amd.h, which this header includes and leaves as it is; the entries below are additions to the same library.
 *
 * B meshes back to back as disn_mc_emit_batch, disn_mesh_clean_emit_batch and disn_mesh_simplify_emit_batch leave them:
 * verts [sum nv][3], faces [sum nf][3] int32 with indices LOCAL to their mesh, v_off_host / f_off_host [B+1] int64
 * ascending from 0; limits as disn_mesh_clean_*: sum nf <= INT32_MAX/3, sum nv <= INT32_MAX; 1 <= V <= 256 views per
 * mesh, S in {1, 2, 4} (disn_mesh_colour_workspace_bytes is 0 beyond them).  Every mesh has V views: trans_mat
 * [B][V][4][3] float32 (device) with [p, 1] . trans_mat = (u w, v w, w), pixel centres at integer (u, v) of a 137 x 137
 * image, w the camera-space depth.
 *
 * THE RULE is postprocess.zbuffer_arrays / postprocess.colour_arrays (disn_amd/postprocess.py), restated operation by
 * operation in float32 and integers (mesh_colour.hip is compiled without contraction):
 *   z-buffer  per view [137 S][137 S] of q = 1/w, larger is nearer, 0 empty; sub-pixel (i, j) at [j][i] covers
 *             [i, i+1) x [j, j+1) of x = (u + 1/2) S, y = (v + 1/2) S.  A triangle with a vertex at w <= 0, of zero
 *             screen area or without a finite gradient of q is skipped; coverage is conservative (edge functions at
 *             the centre raised by (|a| + |b|) / 2); the value is the plane of q at the centre, clamped to the vertices'
 *             [min q, max q], THEN lowered by |dq/dx| + |dq/dy|, floored at FLT_MIN; the buffer keeps the maximum
 *             (unsigned integer atomic max of the bits: independent of the order)
 *   seen      w > 0, sub-pixel inside, 1/w >= (1 - rel_tol) zbuf, alpha > 0 at the nearest pixel when alpha is given
 *   colour    bilinear samples as rint(c 65535); integer means that round half up over the seeing views (class 1),
 *             over the views that see the reflection in the plane mirror_axis (0, 1, 2; -1: none) ON the surface,
 *             1/w <= (1 + 32 rel_tol) zbuf (class 2), over coloured face neighbours in up to fill_iters rounds
 *             (class 3), over the mesh (class 0, mid grey 128 when nothing is coloured)
 *
 *   disn_mesh_zbuffer_batch  zbuf [B][V][137 S][137 S] float32 and status [B] int32 (device).
 *   disn_mesh_colour_batch   images [B][V][137][137][3] float32 in [0,1], alpha [B][V][137][137] uint8 or NULL (device);
 *       bgr != 0: the images are in B G R order, colours are written R G B.  0 <= fill_iters <= 4096, 0 <= rel_tol < 1.
 *       colours [sum nv][3] uint8, seen [sum nv] uint8 (the class), status [B] int32 (device).
 *   status: 0 ok; 2 a face index outside [0, nv_b) (the first kernel compares every index with its mesh's size, every
 *       later one skips that mesh: nothing is addressed through an unchecked index); 4 a vertex coordinate that is
 *       not finite.  A mesh with a status gets mid grey and class 0 (an all-empty z-buffer) and leaves its neighbours
 *       as they are.  An empty mesh is a no-op.
 *   disn_write_obj_colours   host: "v x y z r g b" with r, g, b = c / 255 in four decimals; with normals "vn" lines
 *       and "f a//a b//b c//c" as disn_write_obj_normals.  disn_read_obj_verts and disn_read_obj_mesh stop after
 *       three numbers on a "v" line: they read these files as they read plain ones.
 * No kernel waits for another workgroup; every loop is bounded (a large triangle's wave walks its clipped bounding
 * box, at most (137 S)^2 sub-pixels); there is no floating-point atomic; no host synchronisation: a device word lets
 * the fill rounds after the last useful one return at once.  The host arrays must stay valid until the stream has
 * passed the call.
 */
#ifndef DISN_AMD_COLOUR_H
#define DISN_AMD_COLOUR_H

#include "disn_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DISN_COLOUR_IMG 137
#define DISN_COLOUR_MAX_VIEWS 256
#define DISN_COLOUR_MAX_FILL 4096

size_t disn_mesh_colour_workspace_bytes(int B, int V, int64_t nv_total, int64_t nf_total, int S);
int disn_mesh_zbuffer_batch(const float* verts, const int32_t* faces, const int64_t* v_off_host,
                            const int64_t* f_off_host, int B, const float* trans_mat, int V, int S, float* zbuf,
                            int32_t* status, void* ws, size_t ws_bytes, void* stream);
int disn_mesh_colour_batch(const float* verts, const int32_t* faces, const int64_t* v_off_host,
                           const int64_t* f_off_host, int B, const float* images, const uint8_t* alpha,
                           const float* trans_mat, int V, int S, float rel_tol, int mirror_axis, int fill_iters, int bgr,
                           uint8_t* colours, uint8_t* seen, int32_t* status, void* ws, size_t ws_bytes, void* stream);
int disn_write_obj_colours(const char* path, const float* verts, int64_t nv, const uint8_t* colours,
                           const float* normals, const int32_t* faces, int64_t nf);

#ifdef __cplusplus
}
#endif

#endif /* DISN_AMD_COLOUR_H */

"""float32 numpy restatement of csrc/render.hip, a plain loop over all triangles, written from the rule in the
kernel's header and DESIGN §4u: the same operations in the same order, so hits, depth and the colour bytes are
compared bit for bit.  Also the tripod mesh and the vertex/mask check the tests share."""
import numpy as np

import mesh_sdf_reference as R

f32 = np.float32


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def trace(org, dirs, tris, chunk=4096):
    """nearest hit of rays org [3] + t * dirs [n,3] among tris [m,3,3] (float32) -> (t [n] float32, inf for a miss;
    face [n] int64, -1 for a miss); equal t goes to the lowest face"""
    n = len(dirs)
    t_out = np.full(n, np.inf, f32)
    f_out = np.full(n, -1, np.int64)
    a = tris[None, :, 0]
    e1, e2 = tris[None, :, 1] - a, tris[None, :, 2] - a
    tv = (org[None, None, :] - a).astype(f32)
    q = _cross(tv, e1)
    e2q = _dot(e2, q)
    with np.errstate(all="ignore"):
        for s in range(0, n, chunk):
            d = dirs[s:s + chunk, None, :]
            p = _cross(d, e2)
            det = _dot(e1, p)
            u = _dot(tv, p) / det
            v = _dot(d, q) / det
            t = e2q / det
            ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= f32(1)) & (t > 0)
            t = np.where(ok, t, f32(np.inf)).astype(f32)
            best = t.min(axis=1)
            face = np.argmax(t == best[:, None], axis=1)      # the first (lowest) face at the minimum
            hit = np.isfinite(best)
            t_out[s:s + chunk] = best
            f_out[s:s + chunk] = np.where(hit, face, -1)
    return t_out, f_out


def render(verts, faces, cams, W, H, S, albedo=None, ambient=0.3):
    """-> (rgba uint8 [V,H,W,4], depth float32 [V,H,W], face int32 [V,H,W]) as disn_render_views writes them"""
    tris = np.asarray(verts, f32)[np.asarray(faces, np.int64)]
    nrm = _cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0])
    nn = np.sqrt(_dot(nrm, nrm))
    alb = np.full((len(tris), 3), f32(0.8), f32) if albedo is None else np.asarray(albedo, f32)
    cams = np.asarray(cams, f32).reshape(-1, 12)
    V = len(cams)
    rgba = np.zeros((V, H, W, 4), np.uint8)
    depth = np.zeros((V, H, W), f32)
    face = np.full((V, H, W), -1, np.int32)
    amb, fs = f32(ambient), f32(S)
    ii, jj = np.meshgrid(np.arange(H, dtype=f32), np.arange(W, dtype=f32), indexing="ij")
    for v in range(V):
        org, d0, dx, dy = cams[v, 0:3], cams[v, 3:6], cams[v, 6:9], cams[v, 9:12]
        sums = np.zeros((H, W, 3), f32)
        hits = np.zeros((H, W), np.int64)
        best_t = np.full((H, W), np.inf, f32)
        best_f = np.full((H, W), -1, np.int64)
        for sy in range(S):
            y = ii + (f32(sy) + f32(0.5)) / fs
            for sx in range(S):
                x = jj + (f32(sx) + f32(0.5)) / fs
                d = ((d0 + x[..., None] * dx) + y[..., None] * dy).astype(f32)
                t, f = trace(org, d.reshape(-1, 3), tris)
                t, f = t.reshape(H, W), f.reshape(H, W)
                hit = f >= 0
                fi = np.where(hit, f, 0)
                with np.errstate(all="ignore"):
                    den = nn[fi] * np.sqrt(_dot(d, d))
                    c = np.where(den > 0, np.minimum(np.abs(_dot(nrm[fi], d)) / den, f32(1)), f32(0)).astype(f32)
                shade = amb + (f32(1) - amb) * c
                col = shade[..., None] * alb[fi]
                sums = np.where(hit[..., None], sums + col, sums).astype(f32)
                hits += hit
                nearer = hit & (t < best_t)
                best_t = np.where(nearer, t, best_t)
                best_f = np.where(nearer, f, best_f)
        any_hit = hits > 0
        nh = np.maximum(hits, 1).astype(f32)
        col = np.minimum(np.floor(sums / nh[..., None] * f32(255) + f32(0.5)), f32(255))
        al = np.floor(f32(255) * nh / (fs * fs) + f32(0.5))
        rgba[v, ..., :3] = np.where(any_hit[..., None], col, 0).astype(np.uint8)
        rgba[v, ..., 3] = np.where(any_hit, al, 0).astype(np.uint8)
        depth[v] = np.where(any_hit, best_t, f32(0))
        face[v] = best_f
    return rgba, depth, face


# ---- shared fixtures ---------------------------------------------------------------------------------------------
TRIPOD = ((1, 0.10, (0.55, 0.0, 0.0)), (1, 0.16, (0.0, 0.45, 0.0)), (1, 0.22, (0.0, 0.0, 0.35)),
          (1, 0.06, (0.0, 0.0, 0.0)))
# az, el, distance ratio, W, H, S
TRIPOD_VIEWS = ((30.0, 27.0, 0.8, 137, 137, 1), (200.0, 25.0, 0.7, 37, 29, 3), (0.0, 0.0, 0.9, 33, 33, 1),
                (123.0, 30.0, 0.95, 137, 137, 2))


def tripod():
    """four icospheres, asymmetric under every flip and transposition of the image"""
    vs, fs, base = [], [], 0
    for level, radius, centre in TRIPOD:
        v, f = R.icosphere(level, radius)
        vs.append((v + np.asarray(centre, f32)).astype(f32))
        fs.append(f + base)
        base += len(v)
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32)


def unit_cube():
    """[0,1]^3, 12 triangles: three faces lie in the coordinate planes, which hold the axes"""
    return R.box([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])


def project(points, trans_mat):
    """get_img_points without the integer cast: float64 [n,2] (x, y)"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    xyz = np.concatenate([p, np.ones((len(p), 1))], -1) @ np.asarray(trans_mat, np.float64)
    return xyz[:, :2] / xyz[:, 2:3]


def dilate3(mask):
    m = np.pad(mask, 1)
    out = np.zeros_like(mask)
    for dy in range(3):
        for dx in range(3):
            out |= m[dy:dy + mask.shape[0], dx:dx + mask.shape[1]]
    return out


def vertex_mask_check(points, trans_mat, alpha):
    """-> (fraction of points inside the image, fraction of those on the 3x3-dilated alpha > 0 mask); the pixel
    of an image point is its integer part, as get_img_points casts"""
    H, W = alpha.shape
    xy = project(points, trans_mat)
    inside = (xy[:, 0] >= 0) & (xy[:, 0] < W) & (xy[:, 1] >= 0) & (xy[:, 1] < H)
    px = xy[inside].astype(np.int32)
    mask = dilate3(alpha > 0)
    on = mask[px[:, 1], px[:, 0]]
    return inside.mean(), (on.mean() if len(on) else 0.0)


def convex_hull(xy):
    """Andrew's monotone chain -> the hull's corners counter-clockwise, float64 [k,2]"""
    pts = sorted(map(tuple, np.asarray(xy, np.float64)))

    def half(seq):
        out = []
        for p in seq:
            while len(out) >= 2 and ((out[-1][0] - out[-2][0]) * (p[1] - out[-2][1])
                                     - (out[-1][1] - out[-2][1]) * (p[0] - out[-2][0])) <= 0:
                out.pop()
            out.append(p)
        return out[:-1]
    return np.asarray(half(pts) + half(pts[::-1]))


def outside_hull(hull, xy):
    """how far each point lies outside the convex polygon (0 inside), float64 [n]"""
    a, b = hull, np.roll(hull, -1, axis=0)
    e = b - a
    nrm = np.stack([e[:, 1], -e[:, 0]], 1) / np.linalg.norm(e, axis=1, keepdims=True)     # outward for CCW
    d = np.einsum("nkc,kc->nk", np.asarray(xy, np.float64)[:, None, :] - a[None], nrm)
    return np.maximum(d.max(axis=1), 0.0)

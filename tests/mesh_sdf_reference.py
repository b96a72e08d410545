"""numpy restatements of mesh-to-SDF preprocessing (disn_amd/mesh_sdf.py, disn_amd/preprocess.py), written from
the rules in csrc/mesh_sdf.hip and DESIGN §4p:

tri_d2 / udf   float32, the kernel's operation order: Ericson's region-based closest point with guarded divisions
               (in the face region n . (p - a) == 0 gives 0: a point on the face has u == 0) and the three-edge fall-back, the minimum with the edges for slivers, dot = (ax*bx + ay*by) + az*bz, d2 = (dx*dx + dy*dy) + dz*dz, one
               sqrt of the minimum.  Bit-identical to the kernel.
crossing_bits  float64 edge/triangle crossing from the float32 inputs, same operation order as the kernel.
flood          the sign rule on given u and crossing arrays: far flood of {u >= tau} from the box boundary
               (6-connected), then `steps` Jacobi band steps through uncrossed edges.
Also mesh generators for the tests (icosphere, torus, boxes) and a parser of the BVH image.
"""
from collections import deque

import numpy as np

f32 = np.float32


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _d2(p, q):
    d = p - q
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _safe_div(n, d):
    ok = d > 0
    return np.where(ok, n / np.where(ok, d, f32(1)), f32(0)).astype(f32)


def _seg_d2(p, a, b):
    ab = b - a
    den = _dot(ab, ab)
    t = _safe_div(_dot(p - a, ab), den)
    t = np.minimum(np.maximum(t, f32(0)), f32(1))
    return _d2(p, a + t[..., None] * ab)


def tri_d2(p, tris):
    """p [n,3], tris [m,3,3] float32 -> d2 [n,m] float32"""
    p = np.asarray(p, f32)[:, None, :]
    t = np.asarray(tris, f32)[None]
    a, b, c = t[..., 0, :], t[..., 1, :], t[..., 2, :]
    with np.errstate(all="ignore"):
        ab, ac = b - a, c - a
        ap = p - a
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = p - b
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = p - c
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e1, e2 = d4 - d3, d5 - d6
        s = (va + vb) + vc
        n = np.stack([ab[..., 1] * ac[..., 2] - ab[..., 2] * ac[..., 1], ab[..., 2] * ac[..., 0] - ab[..., 0] * ac[..., 2],
                      ab[..., 0] * ac[..., 1] - ab[..., 1] * ac[..., 0]], -1)
        in_plane = np.broadcast_to(_dot(n, ap) == 0, s.shape)
        cases = [
            ((d1 <= 0) & (d2 <= 0), lambda: _d2(p, a)),
            ((d3 >= 0) & (d4 <= d3), lambda: _d2(p, b)),
            ((vc <= 0) & (d1 >= 0) & (d3 <= 0), lambda: _d2(p, a + _safe_div(d1, d1 - d3)[..., None] * ab)),
            ((d6 >= 0) & (d5 <= d6), lambda: _d2(p, c)),
            ((vb <= 0) & (d2 >= 0) & (d6 <= 0), lambda: _d2(p, a + _safe_div(d2, d2 - d6)[..., None] * ac)),
            ((va <= 0) & (e1 >= 0) & (e2 >= 0), lambda: _d2(p, b + _safe_div(e1, e1 + e2)[..., None] * (c - b))),
            ((va >= 0) & (vb >= 0) & (vc >= 0) & (s > 0),
             lambda: np.where(in_plane, f32(0), _d2(p, (a + (vb / s)[..., None] * ab) + (vc / s)[..., None] * ac))),
        ]
        edges = np.minimum(np.minimum(_seg_d2(p, a, b), _seg_d2(p, b, c)), _seg_d2(p, c, a))
        out = edges
        done = np.zeros(out.shape, bool)
        for cond, val in cases:
            take = cond & ~done
            if take.any():
                out = np.where(take, val(), out)
            done |= cond
        sliver = ~(_dot(n, n) > f32(2.0 ** -20) * (_dot(ab, ab) * _dot(ac, ac)))
        out = np.where(sliver, np.minimum(out, edges), out)
    return out.astype(f32)


def udf(points, verts, faces, chunk=256):
    """unsigned distance of points [n,3] to the mesh, float32 [n] (bit-identical to disn_mesh_udf_*)"""
    pts = np.asarray(points, f32).reshape(-1, 3)
    tris = np.asarray(verts, f32)[np.asarray(faces, np.int64)]
    step = max(1, min(chunk, (1 << 22) // max(1, len(tris))))
    out = np.empty(len(pts), f32)
    for s in range(0, len(pts), step):
        out[s:s + step] = np.sqrt(tri_d2(pts[s:s + step], tris).min(axis=1))
    return out


def udf_f64(points, verts, faces, chunk=1024):
    """float64 distance (projection + edge distances), for accuracy checks and for telling nodes on the surface"""
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    if len(pts) > chunk:
        return np.concatenate([udf_f64(pts[s:s + chunk], verts, faces, chunk) for s in range(0, len(pts), chunk)])
    p = pts[:, None, :]
    t = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)][None]
    a, b, c = t[..., 0, :], t[..., 1, :], t[..., 2, :]

    def seg(a, b):
        ab = b - a
        tt = np.clip(np.sum((p - a) * ab, -1) / np.maximum(np.sum(ab * ab, -1), 1e-300), 0, 1)
        return np.sum((p - (a + tt[..., None] * ab)) ** 2, -1)
    n = np.cross(b - a, c - a)
    nn = np.sum(n * n, -1)
    dist_plane = np.sum((p - a) * n, -1)
    q = p - (dist_plane / np.maximum(nn, 1e-300))[..., None] * n
    inside = np.ones(q.shape[:-1], bool)
    for u, v in ((a, b), (b, c), (c, a)):
        inside &= np.sum(np.cross(v - u, q - u) * n, -1) >= 0
    d_in = np.where(nn > 0, dist_plane ** 2 / np.maximum(nn, 1e-300), np.inf)
    d = np.minimum(np.minimum(seg(a, b), seg(b, c)), seg(c, a))
    d = np.where(inside & (nn > 0), np.minimum(d, d_in), d)
    return np.sqrt(d.min(axis=1))


def grid_points(axes):
    zz, yy, xx = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.stack([xx, yy, zz], -1).reshape(-1, 3).astype(f32)


# ---- sign ---------------------------------------------------------------------------------------------------------
def crossing_bits(axes, u, tau, verts, faces):
    """uint8 [nz,ny,nx]: bit a set when the edge from the node to its +a neighbour crosses a triangle; tested where
    one end is a band node (u < tau), the kernel's rule"""
    nx, ny, nz = (len(a) for a in axes)
    u = np.asarray(u, f32).reshape(nz, ny, nx)
    tris = np.asarray(verts, f32)[np.asarray(faces, np.int64)].astype(np.float64)   # [m,3,3]
    bits = np.zeros((nz, ny, nx), np.uint8)
    band = u < f32(tau)
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        sl0 = [slice(None)] * 3
        sl1 = [slice(None)] * 3
        zyx = 2 - a
        sl0[zyx] = slice(0, -1)
        sl1[zyx] = slice(1, None)
        test = np.zeros_like(band)
        test[tuple(sl0)] = band[tuple(sl0)] | band[tuple(sl1)]
        iz, iy, ix = np.nonzero(test)
        if len(iz) == 0:
            continue
        idx = np.stack([ix, iy, iz], 1)
        x0 = np.asarray(axes[a], f32)[idx[:, a]].astype(np.float64)
        x1 = np.asarray(axes[a], f32)[idx[:, a] + 1].astype(np.float64)
        sb = np.asarray(axes[b], f32)[idx[:, b]].astype(np.float64)[:, None]
        sc = np.asarray(axes[c], f32)[idx[:, c]].astype(np.float64)[:, None]
        P, Q, R = tris[None, :, 0], tris[None, :, 1], tris[None, :, 2]
        hitany = np.zeros(len(iz), bool)
        step = max(1, (1 << 21) // max(1, len(tris)))
        for s in range(0, len(iz), step):
            e = slice(s, s + step)
            pb, pc = P[..., b] - sb[e], P[..., c] - sc[e]
            qb, qc = Q[..., b] - sb[e], Q[..., c] - sc[e]
            rb, rc = R[..., b] - sb[e], R[..., c] - sc[e]
            wp = qb * rc - qc * rb
            wq = rb * pc - rc * pb
            wr = pb * qc - pc * qb
            area = (wp + wq) + wr
            hit = (area != 0) & (((wp >= 0) & (wq >= 0) & (wr >= 0)) | ((wp <= 0) & (wq <= 0) & (wr <= 0)))
            with np.errstate(all="ignore"):
                x = ((wp * P[..., a] + wq * Q[..., a]) + wr * R[..., a]) / np.where(area != 0, area, 1.0)
            lo, hi = np.minimum(x0[e], x1[e])[:, None], np.maximum(x0[e], x1[e])[:, None]
            hitany[e] = (hit & (lo <= x) & (x <= hi)).any(1)
        bits[iz[hitany], iy[hitany], ix[hitany]] |= np.uint8(1 << a)
    return bits


def flood(u, bits, tau, steps):
    """the sign rule on u [nz,ny,nx] and crossing bits [nz,ny,nx] -> outside bool [nz,ny,nx]"""
    u = np.asarray(u, f32)
    nz, ny, nx = u.shape
    far = u >= f32(tau)
    out = np.zeros(u.shape, bool)
    q = deque()
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                if far[z, y, x] and (x in (0, nx - 1) or y in (0, ny - 1) or z in (0, nz - 1)):
                    out[z, y, x] = True
                    q.append((z, y, x))
    while q:
        z, y, x = q.popleft()
        for dz, dy, dx in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
            j = (z + dz, y + dy, x + dx)
            if 0 <= j[0] < nz and 0 <= j[1] < ny and 0 <= j[2] < nx and far[j] and not out[j]:
                out[j] = True
                q.append(j)
    band = ~far
    for _ in range(steps):
        nxt = out.copy()
        for ax, bit in ((2, 1), (1, 2), (0, 4)):   # numpy axis of x, y, z
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[ax], hi[ax] = slice(0, -1), slice(1, None)
            lo, hi = tuple(lo), tuple(hi)
            open_edge = (bits[lo] & bit) == 0
            nxt[lo] |= band[lo] & out[hi] & open_edge     # from the + neighbour
            nxt[hi] |= band[hi] & out[lo] & open_edge     # from the - neighbour
        out = nxt
    return out


def signed(u, outside, offset=0.0):
    u = np.asarray(u, f32)
    return (np.where(outside, u, -u) - f32(offset)).astype(f32)


# ---- BVH image (csrc/mesh_bvh.hpp) ------------------------------------------------------------------------------
def parse_bvh(img, nf):
    hdr = np.frombuffer(img[:16].tobytes(), np.int32)
    n_nodes = int(hdr[1])
    raw = np.frombuffer(img[16:16 + 32 * n_nodes].tobytes(), np.float32).reshape(n_nodes, 8)
    ints = raw.view(np.int32)
    off = (16 + 2 * nf * 32 + 15) & ~15
    tris = np.frombuffer(img[off:off + 36 * nf].tobytes(), np.float32).reshape(nf, 3, 3)
    return {"magic": int(hdr[0]), "n_nodes": n_nodes, "n_tris": int(hdr[2]), "lo": raw[:, 0:3], "hi": raw[:, 4:7],
            "escape": ints[:, 3], "leaf": ints[:, 7], "tris": tris}


# ---- sampling -----------------------------------------------------------------------------------------------------
def sample_surface(verts, faces, count, rng):
    """area-weighted surface samples, written out step by step (trimesh.sample.sample_surface)"""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    area = np.linalg.norm(np.cross(b - a, c - a), axis=1) / 2.0
    cum = np.cumsum(area)
    pick = rng.random(count) * cum[-1]
    fi = np.searchsorted(cum, pick)
    r = rng.random((count, 2))
    out = np.empty((count, 3))
    for k in range(count):
        s, t = r[k]
        if s + t > 1.0:
            s, t = abs(s - 1.0), abs(t - 1.0)
        i = fi[k]
        out[k] = a[i] + ((b[i] - a[i]) * s + (c[i] - a[i]) * t)
    return out


def sample_sdf(num_sample, bandwidth, iso_val, params, values, sdf_res, rng):
    """the reference's sample_sdf in numpy with rng.integers for np.random.randint"""
    percentages = [[-1. * bandwidth, -1. * bandwidth * 0.30, int(num_sample * 0.25)],
                   [-1. * bandwidth * 0.30, 0, int(num_sample * 0.25)],
                   [0, bandwidth * 0.30, int(num_sample * 0.25)],
                   [bandwidth * 0.30, bandwidth, int(num_sample * 0.25)]]
    p = np.asarray(params, f32).astype(np.float64)
    x, y, z = (np.linspace(p[a], p[a + 3], num=sdf_res + 1).astype(f32) for a in range(3))
    vals = np.asarray(values, f32).ravel()
    dis = vals - iso_val
    rows = np.zeros((0, 4), f32)
    for i in range(4):
        ind = np.argwhere((dis >= percentages[i][0]) & (dis < percentages[i][1]))
        if len(ind) < percentages[i][2]:
            if i < 3:
                percentages[i + 1][2] += percentages[i][2] - len(ind)
            percentages[i][2] = len(ind)
        if len(ind) == 0:
            continue
        ch = ind[rng.integers(len(ind), size=percentages[i][2])]
        xi, yi, zi = ch % (sdf_res + 1), (ch // (sdf_res + 1)) % (sdf_res + 1), ch // (sdf_res + 1) ** 2
        rows = np.concatenate((rows, np.concatenate((x[xi], y[yi], z[zi], vals[ch]), -1)), 0)
    return rows.astype(f32), [q[2] for q in percentages]


# ---- test meshes ---------------------------------------------------------------------------------------------------
def icosphere(level=2, radius=1.0):
    t = (1.0 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        cache, nf = {}, []

        def mid(i, j):
            k = (min(i, j), max(i, j))
            if k not in cache:
                m = (v[i] + v[j]) / 2
                v.append(m / np.linalg.norm(m))
                cache[k] = len(v) - 1
            return cache[k]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.asarray(v) * radius).astype(f32), np.asarray(f, np.int32)


def torus(R=0.6, r=0.25, nu=32, nv=16):
    us, vs = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing="ij")
    v = np.stack([(R + r * np.cos(vs)) * np.cos(us), (R + r * np.cos(vs)) * np.sin(us), r * np.sin(vs)], -1)
    f = []
    for i in range(nu):
        for j in range(nv):
            a, b = i * nv + j, ((i + 1) % nu) * nv + j
            c, d = ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
            f += [(a, b, c), (a, c, d)]
    return v.reshape(-1, 3).astype(f32), np.asarray(f, np.int32)


def box(lo, hi, open_face=None):
    """axis-aligned box, two triangles per face; open_face = "+x" etc. leaves that face out"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[lo[0] if i & 1 == 0 else hi[0], lo[1] if i & 2 == 0 else hi[1], lo[2] if i & 4 == 0 else hi[2]]
                  for i in range(8)], f32)
    faces = {"-x": (0, 2, 6, 4), "+x": (1, 5, 7, 3), "-y": (0, 4, 5, 1), "+y": (2, 3, 7, 6),
             "-z": (0, 1, 3, 2), "+z": (4, 6, 7, 5)}
    f = []
    for k, (a, b, c, d) in faces.items():
        if k != open_face:
            f += [(a, b, c), (a, c, d)]
    return v, np.asarray(f, np.int32)


def box_with_hole(lo, hi, hole):
    """closed box whose +z face has a square hole of side `hole` at its centre (faces tessellated on a 3x3 grid of
    the +z face: the centre cell is the hole)"""
    v, f = box(lo, hi, open_face="+z")
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    cx, cy = (lo[0] + hi[0]) / 2, (lo[1] + hi[1]) / 2
    xs = [lo[0], cx - hole / 2, cx + hole / 2, hi[0]]
    ys = [lo[1], cy - hole / 2, cy + hole / 2, hi[1]]
    base = len(v)
    verts = [(x, y, hi[2]) for y in ys for x in xs]
    faces = list(map(tuple, f))
    for j in range(3):
        for i in range(3):
            if i == 1 and j == 1:
                continue
            a = base + j * 4 + i
            faces += [(a, a + 1, a + 5), (a, a + 5, a + 4)]
    return np.concatenate([v, np.asarray(verts, f32)]).astype(f32), np.asarray(faces, np.int32)


def inside_exact(points, kind, **kw):
    p = np.asarray(points, np.float64)
    if kind == "box":
        lo, hi = np.asarray(kw["lo"]), np.asarray(kw["hi"])
        return np.all((p > lo) & (p < hi), axis=1)
    raise ValueError(kind)


def winding(points, verts, faces, chunk=2048):
    """generalised winding number (float64 solid angles, van Oosterom-Strackee) of a closed oriented mesh"""
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    if len(pts) > chunk:
        return np.concatenate([winding(pts[s:s + chunk], verts, faces, chunk) for s in range(0, len(pts), chunk)])
    p = pts[:, None, :]
    t = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)][None]
    a, b, c = t[..., 0, :] - p, t[..., 1, :] - p, t[..., 2, :] - p
    la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (a, b, c))
    num = np.sum(a * np.cross(b, c), -1)
    den = la * lb * lc + np.sum(a * b, -1) * lc + np.sum(b * c, -1) * la + np.sum(c * a, -1) * lb
    return (2 * np.arctan2(num, den)).sum(1) / (4 * np.pi)

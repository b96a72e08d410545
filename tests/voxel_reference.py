"""numpy restatement of csrc/voxel.hip and of the component labelling of csrc/mesh_host.cpp (checker only).

Voxel key k is the closed box of centre k*h and half side h/2, h = float32(2)/float32(dim).  ``axis_terms`` is the
13-axis separating-axis test in the kernel's operation order (float32, one rounding per operation: numpy never
contracts a*b - c*d) with a float64 twin; ``surface_voxels`` tests every candidate key of every triangle by brute
force over a range wider than the kernel's; the corner map is the reference's literal expression on explicit
float64 corners; the fill is scipy.ndimage.binary_fill_holes.
"""
import numpy as np


def cell_size(dim, dt=np.float32):
    return dt(np.float32(2.0) / np.float32(dim))


def key_range(dim):
    """-> (kmin, nkeys): the keys whose corners (k -+ 0.5) * (2/dim) all have 0 <= (c + 1.1) / 2.4 * dim < dim"""
    ks = np.arange(-3 * dim, 3 * dim + 1)
    ok = np.ones(ks.size, bool)
    for s in (-0.5, 0.5):
        val = ((ks + s) * (2.0 / dim) + 1.1) / 2.4 * dim
        ok &= (val >= 0) & (val < dim)
    good = ks[ok]
    assert good.size and good[-1] - good[0] + 1 == good.size
    return int(good[0]), int(good.size)


def axis_terms(tri, c, hh, dt=np.float32):
    """tri [..., 3, 3] (vertex, xyz), c [..., 3] box centres (broadcast against tri's leading axes), hh the half
    side -> (lo, hi, r), each [13, ...]: the extreme projections of the translated triangle and the box radius on
    every axis.  Axis a separates when lo[a] > r[a] or hi[a] < -r[a]."""
    tri = np.asarray(tri, dt)
    c = np.asarray(c, dt)
    hh = dt(hh)
    v = tri - c[..., None, :]                                   # [..., vertex, xyz]
    e = (tri[..., 1, :] - tri[..., 0, :], tri[..., 2, :] - tri[..., 1, :], tri[..., 0, :] - tri[..., 2, :])
    shape = v.shape[:-2]
    lo, hi, r = [], [], []

    def add(q, rad):
        lo.append(q.min(-1))
        hi.append(q.max(-1))
        r.append(np.broadcast_to(np.asarray(rad, dt), shape))

    for a in range(3):
        add(v[..., :, a], hh)
    vx, vy, vz = v[..., :, 0], v[..., :, 1], v[..., :, 2]
    for ed in e:
        ex, ey, ez = ed[..., 0:1], ed[..., 1:2], ed[..., 2:3]
        add(ez * vy - ey * vz, ((np.abs(ez) + np.abs(ey)) * hh)[..., 0])
        add(ex * vz - ez * vx, ((np.abs(ex) + np.abs(ez)) * hh)[..., 0])
        add(ey * vx - ex * vy, ((np.abs(ey) + np.abs(ex)) * hh)[..., 0])
    e0, e1 = e[0], e[1]
    nx = e0[..., 1] * e1[..., 2] - e0[..., 2] * e1[..., 1]
    ny = e0[..., 2] * e1[..., 0] - e0[..., 0] * e1[..., 2]
    nz = e0[..., 0] * e1[..., 1] - e0[..., 1] * e1[..., 0]
    s = (nx * v[..., 0, 0] + ny * v[..., 0, 1]) + nz * v[..., 0, 2]
    rad = ((np.abs(nx) + np.abs(ny)) + np.abs(nz)) * hh
    s = np.broadcast_to(s, shape)
    lo.append(s)
    hi.append(s)
    r.append(np.broadcast_to(rad, shape))
    out = np.stack(lo), np.stack(hi), np.stack(r)
    assert all(o.dtype == dt for o in out)
    return out


def overlap(tri, keys, dim, dt=np.float32):
    """tri [..., 3, 3] float32, keys [..., 3] integers -> bool [...]: the triangle overlaps the voxel"""
    h = cell_size(dim, dt)
    c = np.asarray(keys).astype(dt) * h
    lo, hi, r = axis_terms(tri, c, h * dt(0.5), dt)
    return ~((lo > r) | (hi < -r)).any(0)


def borderline(tri, keys, dim, eps=1e-7):
    """some axis of the float64 test has |min - r| or |max + r| below eps (absolute, axes not normalised)"""
    h = cell_size(dim, np.float64)
    c = np.asarray(keys).astype(np.float64) * h
    lo, hi, r = axis_terms(tri, c, h * 0.5, np.float64)
    return ((np.abs(lo - r) < eps) | (np.abs(hi + r) < eps)).any(0)


def surface_voxels(verts, faces, dim, dt=np.float32):
    """-> (dense bool [n, n, n] indexed [x, y, z] over the key range, overflow): every key of a candidate range one
    key wider on each side than the keys the triangle's bounding box touches is tested.  overflow: some point of some triangle lies outside the
    key range (an overlap on the sentinel layer around it, or a vertex beyond that layer or not finite)."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    kmin, n = key_range(dim)
    dense = np.zeros((n + 2, n + 2, n + 2), bool)               # with the sentinel layer: index = k - (kmin - 1)
    overflow = False
    if faces.shape[0] == 0:
        return dense[1:-1, 1:-1, 1:-1].copy(), overflow
    tri = verts[faces]                                          # [T, 3, 3]
    h64 = float(cell_size(dim, np.float64))
    mn, mx = tri.min(1).astype(np.float64), tri.max(1).astype(np.float64)
    bad = ~np.isfinite(tri).all((1, 2)) | (mn < (kmin - 1.5) * h64).any(1) | (mx > (kmin + n + 0.5) * h64).any(1)
    overflow = bool(bad.any())
    tri, mn, mx = tri[~bad], mn[~bad], mx[~bad]
    lo = np.clip(np.floor(mn / h64 - 0.5).astype(np.int64) - 1, kmin - 1, kmin + n)
    hi = np.clip(np.ceil(mx / h64 + 0.5).astype(np.int64) + 1, kmin - 1, kmin + n)
    ext = hi - lo + 1
    done = np.zeros(tri.shape[0], bool)
    for side, batch in ((6, 4096), (8, 2048), (12, 512)):       # triangles of similar extent share a block of keys
        idx = np.nonzero(~done & (ext <= side).all(1))[0]
        done[idx] = True
        off = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)
        for s in range(0, idx.size, batch):
            j = idx[s:s + batch]
            keys = lo[j][:, None, :] + off[None]                # [B, side^3, 3]
            ok = (off[None] < ext[j][:, None, :]).all(-1)
            hit = overlap(tri[j][:, None], keys, dim, dt) & ok
            k = keys[hit] - (kmin - 1)
            dense[k[:, 0], k[:, 1], k[:, 2]] = True
    small = done
    for j in np.nonzero(~small)[0]:
        ax = [np.arange(lo[j, a], hi[j, a] + 1) for a in range(3)]
        for z0 in range(0, ax[2].size, 16):                     # slabs keep the temporaries small
            keys = np.stack(np.meshgrid(ax[0], ax[1], ax[2][z0:z0 + 16], indexing="ij"), -1).reshape(-1, 3)
            k = keys[overlap(tri[j], keys, dim, dt)] - (kmin - 1)
            dense[k[:, 0], k[:, 1], k[:, 2]] = True
    inner = dense[1:-1, 1:-1, 1:-1].copy()
    overflow = overflow or bool(dense.sum() != inner.sum())
    return inner, overflow


def index_grid(dense, dim):
    """the reference's array (test_iou.py: ind = ((grid.mesh.vertices + 1.1) / 2.4 * dim).astype(int);
    v[ind[:, 0], ind[:, 1], ind[:, 2]] = 1) from the eight corners (k -+ 0.5) * (2/dim) of every occupied voxel,
    as explicit float64 vertices"""
    kmin, n = key_range(dim)
    assert dense.shape == (n, n, n)
    k = np.argwhere(dense) + kmin
    sgn = np.array([[a, b, c] for a in (-0.5, 0.5) for b in (-0.5, 0.5) for c in (-0.5, 0.5)])
    vertices = ((k[:, None, :] + sgn[None]) * (2.0 / dim)).reshape(-1, 3)
    ind = ((vertices + 1.1) / 2.4 * dim).astype(int)
    v = np.zeros([dim, dim, dim])
    v[ind[:, 0], ind[:, 1], ind[:, 2]] = 1
    return v.astype(bool)


def fill(dense):
    from scipy import ndimage
    return ndimage.binary_fill_holes(np.pad(dense, 1))[1:-1, 1:-1, 1:-1]


def iou_counts(gt, pred):
    return int(np.logical_and(gt, pred).sum()), int(np.logical_or(gt, pred).sum())


def grids(verts, faces, dim, mode):
    """the grid that ``mode`` counts on -> (bool array, overflow)"""
    s, ovf = surface_voxels(verts, faces, dim)
    return (index_grid(s, dim) if mode == "reference" else fill(s)), ovf


def components(faces, nv, connectivity="face"):
    """pure-Python union-find -> (labels [nf], count): triangles joined through shared edges (unordered vertex
    pairs) or shared vertices; a component's id is the rank of its smallest triangle index"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    nf = faces.shape[0]
    parent = list(range(nf))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    seen = {}
    for t in range(nf):
        a, b, c = (int(x) for x in faces[t])
        assert 0 <= min(a, b, c) and max(a, b, c) < nv
        items = (a, b, c) if connectivity == "vertex" else (tuple(sorted((a, b))), tuple(sorted((b, c))),
                                                           tuple(sorted((c, a))))
        for it in items:
            if it in seen:
                ra, rb = find(seen[it]), find(t)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
            else:
                seen[it] = t
    ids, labels = {}, np.empty(nf, np.int32)
    for t in range(nf):
        labels[t] = ids.setdefault(find(t), len(ids))
    return labels, len(ids)


def cube(half):
    """an axis-aligned cube of half side ``half`` about the origin: 8 vertices, 12 triangles"""
    a = np.float32(half)
    v = np.array([[x, y, z] for z in (-a, a) for y in (-a, a) for x in (-a, a)], np.float32)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 7, 5], [4, 6, 7], [0, 5, 1], [0, 4, 5], [2, 3, 7], [2, 7, 6],
                  [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)
    return v, f


def icosphere(radius, level, centre=(0.0, 0.0, 0.0)):
    """a subdivided icosahedron -> (verts float32 [nv, 3], faces int32 [nf, 3]): a closed, edge-connected surface"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius + np.array(centre)).astype(np.float32), np.array(f, np.int32)

"""Meshes, cameras and pictures of the vertex-colour tests (test_mesh_colour_host.py, test_gpu_mesh_colour.py).  Plain
module, numpy only.  Everything is small: the largest mesh is the 256 x 128 sphere (33 k vertices)."""
import functools

import numpy as np

IMG = 137
FOCAL, DIST = 150.0, 2.0


def pinhole(focal=FOCAL, dist=DIST, rot_y=0.0, cx=68.0, cy=68.0):
    """trans_mat [4,3] float32 with [p, 1] . T = (u w, v w, w): the object turned by ``rot_y`` about its y axis, then a
    camera at distance ``dist`` on the -z axis that looks along +z, principal point (cx, cy)"""
    c, s = np.cos(rot_y), np.sin(rot_y)
    R = np.array([[c, 0.0, -s], [0.0, 1.0, 0.0], [s, 0.0, c]])          # rows: where x, y, z of the object go
    K = np.array([[focal, 0.0, 0.0], [0.0, focal, 0.0], [cx, cy, 1.0]])   # rows: camera x, y, z -> (u w, v w, w)
    T = np.zeros((4, 3))
    T[:3] = R @ K
    T[3] = np.array([0.0, 0.0, dist]) @ K
    return T.astype(np.float32)


def camera_centre(T):
    """the object-frame point that projects to w = 0 on every ray: -tt M^-1"""
    T = np.asarray(T, np.float64)
    return -T[3] @ np.linalg.inv(T[:3])


def project(v, T):
    p = np.asarray(v, np.float64) @ np.asarray(T, np.float64)[:3] + np.asarray(T, np.float64)[3]
    return p[:, 0] / p[:, 2], p[:, 1] / p[:, 2], p[:, 2]


def uv_sphere(nu, nv, r=0.4):
    """a closed UV sphere about the y axis: nu segments around, nv from pole to pole; outward winding"""
    verts = [[0.0, r, 0.0]]
    for j in range(1, nv):
        t = np.pi * j / nv
        for i in range(nu):
            p = 2.0 * np.pi * i / nu
            verts.append([r * np.sin(t) * np.cos(p), r * np.cos(t), r * np.sin(t) * np.sin(p)])
    verts.append([0.0, -r, 0.0])
    ring = lambda j, i: 1 + (j - 1) * nu + i % nu
    faces = []
    for i in range(nu):
        faces.append([0, ring(1, i + 1), ring(1, i)])
        faces.append([len(verts) - 1, ring(nv - 1, i), ring(nv - 1, i + 1)])
    for j in range(1, nv - 1):
        for i in range(nu):
            a, b, c, d = ring(j, i), ring(j, i + 1), ring(j + 1, i), ring(j + 1, i + 1)
            faces += [[a, b, d], [a, d, c]]
    return np.asarray(verts, np.float32), np.asarray(faces, np.int32)


def square(cells, half, z, x0=0.0, y0=0.0):
    """a square of cells x cells cells (two triangles each) in the plane z, centre (x0, y0), half side ``half``"""
    t = np.linspace(-half, half, cells + 1)
    X, Y = np.meshgrid(t + x0, t + y0)
    v = np.stack([X.reshape(-1), Y.reshape(-1), np.full(X.size, z)], 1)
    idx = lambda j, i: j * (cells + 1) + i
    f = []
    for j in range(cells):
        for i in range(cells):
            f += [[idx(j, i), idx(j, i + 1), idx(j + 1, i + 1)], [idx(j, i), idx(j + 1, i + 1), idx(j + 1, i)]]
    return np.asarray(v, np.float32), np.asarray(f, np.int32)


def join(*meshes):
    vs, fs, base = [], [], 0
    for v, f in meshes:
        vs.append(v)
        fs.append(f + base)
        base += v.shape[0]
    return np.concatenate(vs).astype(np.float32), np.concatenate(fs).astype(np.int32)


FRONT_HALF, BACK_HALF, FRONT_Z, BACK_Z = 0.15, 0.4, -0.2, 0.2          # depths 1.8 and 2.2 from the camera


def occluder(back_cells):
    """a 10 x 10-cell square at depth 1.8 in front of a ``back_cells``-cell square at depth 2.2, one mesh; -> (verts,
    faces, number of front vertices)"""
    front, back = square(10, FRONT_HALF, FRONT_Z), square(back_cells, BACK_HALF, BACK_Z)
    v, f = join(front, back)
    return v, f, front[0].shape[0]


def occluder_truth(v, n_front, T):
    """-> (visible bool [nv] as the geometry says, distance in image pixels of every vertex's projection from the front
    square's projected outline)"""
    u, w_, _ = project(v, T)
    corners = np.array([[-FRONT_HALF, -FRONT_HALF, FRONT_Z], [FRONT_HALF, FRONT_HALF, FRONT_Z]])
    cu, cv, _ = project(corners, T)
    dx = np.maximum(np.maximum(cu[0] - u, u - cu[1]), 0.0)
    dy = np.maximum(np.maximum(cv[0] - w_, w_ - cv[1]), 0.0)
    inside = (u > cu[0]) & (u < cu[1]) & (w_ > cv[0]) & (w_ < cv[1])
    d_in = np.minimum(np.minimum(u - cu[0], cu[1] - u), np.minimum(w_ - cv[0], cv[1] - w_))
    dist = np.where(inside, d_in, np.sqrt(dx * dx + dy * dy))
    visible = ~inside
    visible[:n_front] = True
    return visible, dist


def ramp_image(cu=(0.002, 0.001, 0.003), cv=(0.001, 0.004, 0.002), c0=(0.1, 0.2, 0.05)):
    """[137,137,3] float32: channel c = c0 + cu u + cv v, an affine ramp in the pixel (u, v) = (column, row)"""
    vv, uu = np.meshgrid(np.arange(IMG, dtype=np.float64), np.arange(IMG, dtype=np.float64), indexing="ij")
    return np.stack([c0[k] + cu[k] * uu + cv[k] * vv for k in range(3)], 2).astype(np.float32)


def ramp_value(u, v, cu=(0.002, 0.001, 0.003), cv=(0.001, 0.004, 0.002), c0=(0.1, 0.2, 0.05)):
    return np.stack([c0[k] + cu[k] * np.asarray(u) + cv[k] * np.asarray(v) for k in range(3)], 1)


def noise_image(seed):
    return np.random.default_rng(seed).random((IMG, IMG, 3), dtype=np.float32)


def flat_image(rgb):
    return np.broadcast_to(np.asarray(rgb, np.float32), (IMG, IMG, 3)).copy()


def full_quad():
    """two triangles that fill the image at depth 2 (and reach beyond it): the large-face path"""
    v = np.array([[-1.2, -1.2, 0.0], [1.2, -1.2, 0.0], [1.2, 1.2, 0.0], [-1.2, 1.2, 0.0]], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def mixed():
    """large and tiny faces in one mesh: the image-filling quad behind a 64 x 32 sphere and a 3-cell square"""
    q = full_quad()
    q = (q[0] + np.array([0.0, 0.0, 0.6], np.float32), q[1])
    return join(q, uv_sphere(64, 32, 0.3), square(3, 0.5, -0.5, 0.1, -0.05))


def strip(n):
    """a strip of n quads along x in the plane z = 0, from x = 0: vertex 2 i, 2 i + 1 at x = i d"""
    d = 0.01
    v = np.array([[i * d, y, 0.0] for i in range(n + 1) for y in (0.0, d)], np.float32)
    f = []
    for i in range(n):
        a, b, c, e = 2 * i, 2 * i + 1, 2 * i + 2, 2 * i + 3
        f += [[a, c, e], [a, e, b]]
    return v, np.asarray(f, np.int32)


VIEWS2 = (pinhole(), pinhole(rot_y=np.pi / 2))


@functools.lru_cache(maxsize=None)
def device_cases():
    """name -> (verts, faces, images [V,137,137,3], trans_mats [V,4,3], alpha or None, keyword arguments)"""
    two = np.stack(VIEWS2)
    img2 = np.stack([noise_image(1), noise_image(2)])
    one, img1 = two[:1], img2[:1]
    alpha = (np.random.default_rng(5).random((2, IMG, IMG)) > 0.3).astype(np.uint8) * 255
    occ40, occ160 = occluder(40), occluder(160)
    return {
        "sphere 16x8": (*uv_sphere(16, 8), img2, two, None, {}),
        "sphere 64x32": (*uv_sphere(64, 32), img2, two, None, {}),
        "sphere 256x128 one view": (*uv_sphere(256, 128), img1, one, None, {}),
        "occluder 40": (occ40[0], occ40[1], img1, one, None, {}),
        "occluder 160": (occ160[0], occ160[1], img1, one, None, {}),
        "quad": (*full_quad(), img1, one, None, {}),
        "mixed": (*mixed(), img2, two, None, {}),
        "mixed S1": (*mixed(), img2, two, None, {"S": 1}),
        "mixed S4": (*mixed(), img2, two, None, {"S": 4}),
        "sphere alpha mirror": (*uv_sphere(64, 32), img2, two, alpha, {"mirror_axis": 2, "bgr": False}),
        "sphere one view mirror": (*uv_sphere(32, 16), img1, one, None, {"mirror_axis": 2, "fill_iters": 3}),
        "strip short fill": (*strip(40), img1, np.stack([pinhole(cx=-29.2)]), None, {"fill_iters": 5}),
    }


@functools.lru_cache(maxsize=None)
def host_colour(name):
    from disn_amd import postprocess
    v, f, img, T, alpha, kw = device_cases()[name]
    return postprocess.colour_arrays(v, f, img, T, alpha=alpha, **kw)


@functools.lru_cache(maxsize=None)
def host_zbuffer(name):
    from disn_amd import postprocess
    v, f, img, T, alpha, kw = device_cases()[name]
    return postprocess.zbuffer_arrays(v, f, T, kw.get("S", 2))

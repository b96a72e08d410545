"""Meshes for the tests of the Taubin smoothing (``postprocess.smooth_arrays``, the specification, and mesh_smooth.hip,
its device restatement): each is the smallest that reaches one way the rule or the kernels can go wrong.  Everything is
computed once, shared between the tests and never modified."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_simplify_fixtures as SF  # noqa: E402

cached = SF.cached
MF = SF.MF
RADIUS = 0.4
DENORMAL = np.float32(1e-41)


def _icosphere(subdivisions):
    """an icosahedron subdivided and projected onto the unit sphere -> (verts float64 [nv,3], faces int32 [nf,3]),
    outward orientation"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, out = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    return np.stack(v), np.asarray(f, np.int32)


def sphere():
    """the icosahedron subdivided 3 times on radius 0.4: 642 vertices, 1280 faces, closed"""
    def make():
        v, f = _icosphere(3)
        return (RADIUS * v).astype(np.float32), f
    return cached("smooth sphere", make)


def noisy():
    """``sphere`` with normal noise of sigma 0.01 along the radius"""
    def make():
        v, f = _icosphere(3)
        r = RADIUS + np.random.default_rng(7).normal(0, 0.01, (642, 1))
        return (r * v).astype(np.float32), f
    return cached("smooth noisy", make)


def patch(n=9):
    """an open n x n sheet with bumps: 4 (n - 1) boundary vertices, the others inside"""
    def make():
        x, y = np.meshgrid(np.linspace(-0.4, 0.4, n), np.linspace(-0.4, 0.4, n), indexing="ij")
        z = 0.05 * np.sin(7.0 * x) * np.cos(5.0 * y) + 0.02 * np.random.default_rng(3).normal(size=x.shape)
        v = np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(np.float32)
        idx = np.arange(n * n).reshape(n, n)
        a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel()
        return v, np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)]).astype(np.int32)
    return cached(("smooth patch", n), make)


def patch_boundary(n=9):
    idx = np.arange(n * n).reshape(n, n)
    edge = np.zeros((n, n), bool)
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
    return edge.ravel()


MESSY_ISOLATED, MESSY_PINNED, MESSY_FREE = 10, (0, 2, 6, 7, 8, 9), (1, 3, 4, 5)


def messy():
    """an octahedron (vertices 0..5, closed) with one face twice, a wing (0, 2, 6) that makes {0, 2} an edge of THREE
    faces and 0, 2, 6 boundary vertices, a face (6, 6, 4) -- the pair (6, 6) counts for nothing, {4, 6} is held twice --
    a separate open triangle 7 8 9 whose (pinned) vertices carry a -0.0 and denormal coordinates, and the isolated
    vertex 10 with a -0.0 and a denormal too"""
    v = np.array([[0.5, 0.01, 0], [-0.5, 0, 0.02], [0, 0.45, 0], [0.03, -0.5, 0], [0, 0.02, 0.55], [0.01, 0, -0.5],
                  [0.6, 0.6, 0.1], [-0.0, 0.8, 0.8], [0.9, DENORMAL, 0.8], [0.8, 0.9, -DENORMAL],
                  [-0.0, DENORMAL, 0.25]], np.float32)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5], [1, 3, 4],
                  [0, 2, 6], [6, 6, 4], [7, 8, 9]], np.int32)
    return v, f


def empty():
    return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)


MC_R = 16                                          # 17^3 grids
MC_BOX = np.array([-0.5, -0.5, -0.5, 0.5, 0.5, 0.5], np.float64)


def mc_fields():
    """two analytic fields on the 17^3 grid of MC_BOX -> float32 [2, 17^3] in the mesher's flat (iz, iy, ix) order: a
    sphere inside the box, and a box that sticks out of the grid on +x, so its mesh is open and its boundary lies on
    the face x = 0.5 of the grid box"""
    def make():
        t = np.linspace(-0.5, 0.5, MC_R + 1)
        z, y, x = np.meshgrid(t, t, t, indexing="ij")
        ball = np.sqrt((x - 0.013) ** 2 + (y + 0.021) ** 2 + (z - 0.007) ** 2) - 0.333
        q = np.stack([np.abs(x - 0.4) - 0.31, np.abs(y - 0.02) - 0.27, np.abs(z + 0.01) - 0.23])
        cut = np.sqrt((np.maximum(q, 0) ** 2).sum(0)) + np.minimum(q.max(0), 0)
        return np.stack([ball.reshape(-1), cut.reshape(-1)]).astype(np.float32)
    return cached("smooth mc fields", make)


def host_cases():
    return {"sphere": sphere(), "noisy": noisy(), "patch": patch(), "messy": messy(), "empty": empty()}


def host_smooth(name, iters, pin, cap, mesh=None):
    """``smooth_arrays`` of a named mesh, computed once per parameter set"""
    def make():
        from disn_amd import postprocess
        v, f = host_cases()[name] if mesh is None else mesh
        return postprocess.smooth_arrays(v, f, iters=iters, pin_boundary=bool(pin), max_move=cap)
    return cached(("host_smooth", name, iters, int(pin), cap), make)


def permuted(v, f, seed=1):
    """the same mesh with its faces in another order and every face's corners rotated"""
    rng = np.random.default_rng(seed)
    g = f[rng.permutation(len(f))]
    turn = rng.integers(0, 3, len(g))
    return v, np.stack([g[np.arange(len(g)), (turn + k) % 3] for k in range(3)], 1).astype(np.int32)


def spike():
    """every coordinate within +-1024 at input, but a step throws the hub beyond it: the hub at x = 1000 over four rim
    vertices at x = -1000 (closed below by two more faces, so all five move).  With lam = 1 the first step swaps the
    sides (hub -> -1000, rim -> -500 and -333), and the mu = -1.5 step sends the hub to -1000 - 1.5 (-417 + 1000) = -1875"""
    v = np.array([[1000, 0, 0], [-1000, 1, 0], [-1000, 0, 1], [-1000, -1, 0], [-1000, 0, -1]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1], [1, 3, 2], [1, 4, 3]], np.int32)
    return v, f


SPIKE_KW = {"iters": 1, "lam": 1.0, "mu": -1.5}


def signed_volume(v, f):
    p = np.asarray(v, np.float64)
    return float(np.einsum("ij,ij->i", p[f[:, 0]], np.cross(p[f[:, 1]], p[f[:, 2]])).sum() / 6.0)


def radial_rms(v, radius=RADIUS):
    r = np.linalg.norm(np.asarray(v, np.float64), axis=1)
    return float(np.sqrt(np.mean((r - radius) ** 2)))

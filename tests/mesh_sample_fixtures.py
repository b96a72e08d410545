"""Meshes for the tests of the surface sampler (``metrics.sample_surface_arrays``, the specification, and
mesh_sample.hip, its device restatement): each is the smallest that reaches one way the rule or the kernels can go
wrong.  Everything is computed once, shared between the tests and never modified."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_simplify_fixtures as SF  # noqa: E402

cached = SF.cached
N_BATCH = 1000                                     # no multiple of the block of 256
BATCH_SEEDS = (11, 0xFFFFFFFFFFFFFFFF, 3, 2 ** 63 + 5, 12345678901234567)


def two_triangles():
    """areas 0.5 and 1.5: |N|^2 = 1 and 9, weights isqrt(floor(2^62 / 9)) = 715827882 and 2^31"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [3, 0, 0], [0, 0, 1]], np.float32)
    return v, np.array([[0, 1, 2], [0, 3, 4]], np.int32)


def with_undrawable_faces():
    """the two triangles, a face of one vertex three times and a face with a repeated corner: faces 1 and 3 have no area"""
    v = np.concatenate([two_triangles()[0], [[5, 5, 5]]]).astype(np.float32)
    return v, np.array([[0, 1, 2], [5, 5, 5], [0, 3, 4], [1, 1, 2]], np.int32)


def uneven_square():
    """the unit square in z = 0 on a 40 x 40 lattice whose lines crowd towards 0: 3042 triangles of very uneven area"""
    def make():
        xs = np.sort(np.random.default_rng(0).random(40)) ** 2
        xs[0], xs[-1] = 0.0, 1.0
        X, Y = np.meshgrid(xs, xs, indexing="ij")
        v = np.stack([X.ravel(), Y.ravel(), np.zeros(X.size)], 1).astype(np.float32)
        idx = np.arange(1600).reshape(40, 40)
        a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel()
        return v, np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)]).astype(np.int32)
    return cached("uneven_square", make)


def empty():
    return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)


def all_degenerate():
    """four faces, none with an area: collinear corners, a repeated corner, one vertex three times"""
    v = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [-1, 0.5, 0.25]], np.float32)
    return v, np.array([[0, 1, 2], [3, 3, 0], [2, 2, 2], [2, 1, 0]], np.int32)


def soup(nf=70000, seed=5):
    """nf separate triangles in [-1,1]^3 whose side lengths span 2^20, so their areas span 2^40: it crosses 17 scan
    blocks of 4096 faces, and the faces of less than about 2^-31 of the largest area quantise to weight 0"""
    def make():
        rng = np.random.default_rng(seed)
        scale = 2.0 ** (-20.0 * rng.random(nf))
        scale[[7, nf // 2]] = 1.0, 2.0 ** -20
        centre = rng.uniform(-0.5, 0.5, (nf, 1, 3))
        v = (centre + 0.5 * scale[:, None, None] * rng.uniform(-1.0, 1.0, (nf, 3, 3))).astype(np.float32)
        return v.reshape(-1, 3), np.arange(3 * nf, dtype=np.int32).reshape(-1, 3)
    return cached(("soup", nf, seed), make)


def batch():
    """the B = 5 call of the device tests: two triangles, an empty mesh in the middle, the box of the simplification's
    tests (about 10^4 faces), a mesh of degenerate faces, the soup"""
    return [two_triangles(), empty(), SF.box_mesh(32), all_degenerate(), soup()]


def host_rule(b, n=N_BATCH, seed=None):
    """``sample_surface_arrays`` of mesh b of ``batch()`` with its seed, computed once"""
    def make():
        from disn_amd import metrics
        v, f = batch()[b]
        return metrics.sample_surface_arrays(v, f, n, BATCH_SEEDS[b] if seed is None else seed)
    return cached(("host_rule", b, n, seed), make)


def nn_brute(a, b):
    """float64 brute force of nn_distance for one pair [n,3], [m,3] -> (d1, i1, d2, i2), lowest index on ties"""
    d = ((np.asarray(a, np.float64)[:, None] - np.asarray(b, np.float64)[None]) ** 2).sum(-1)
    return d.min(1), d.argmin(1), d.min(0), d.argmin(0)

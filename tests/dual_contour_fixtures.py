"""Fields for the dual-contouring tests (tests/test_dual_contour_host.py, tests/test_gpu_dual_contour.py): plain
module, no test.  Every fixture returns (vol float32 [(R+1)^3] in .dist order, box float64 [6], iso, normals_at) where
normals_at(points float32 [ne,3]) -> float32 [ne,3] gives the field's normals at Hermite points."""
from __future__ import annotations

import numpy as np

UNIT = np.array([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0])
SKEW = np.array([-1.0, -0.8, -0.9, 1.0, 0.9, 1.1])        # a non-cubic box: three different cell sizes


def grid(box, R):
    """float32 coordinates [n,n,n,3] indexed [iz,iy,ix] of the (R+1)^3 grid (numpy.linspace in float64, cast)"""
    ax = [np.linspace(box[a], box[a + 3], num=R + 1).astype(np.float32) for a in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x, y, z], -1)


def sphere(R=9, box=SKEW, radius=0.6, iso=0.05, centre=(0.03, -0.02, 0.01)):
    c = np.asarray(centre, np.float64)
    g = grid(box, R).astype(np.float64)
    vol = (np.linalg.norm(g - c, axis=-1) - radius).astype(np.float32).reshape(-1)

    def normals_at(points):
        d = np.asarray(points, np.float64) - c
        return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return vol, np.asarray(box, np.float64), iso, normals_at


def plane(R=6, normal=(0.3, -0.5, 0.8), offset=0.11):
    nrm = np.asarray(normal, np.float64)
    vol = (grid(UNIT, R).astype(np.float64) @ nrm - offset).astype(np.float32).reshape(-1)
    return vol, UNIT.copy(), 0.0, lambda points: np.tile(nrm.astype(np.float32), (len(points), 1))


CUBE_H, CUBE_C = 0.625, 0.25


def cube(R=8, h=CUBE_H):
    """f = max_k |p_k| - h on [-1,1]^3: at R = 8, h = 0.625 the faces lie exactly midway between grid planes, every value
    is dyadic and every crossing has t = 1/2 exactly; the normals are the face axes"""
    vol = (np.abs(grid(UNIT, R)).max(-1) - np.float32(h)).astype(np.float32).reshape(-1)

    def normals_at(points):
        p = np.asarray(points, np.float64)
        k = np.abs(p).argmax(1)
        out = np.zeros_like(p)
        out[np.arange(len(p)), k] = np.sign(p[np.arange(len(p)), k])
        return out.astype(np.float32)
    return vol, UNIT.copy(), 0.0, normals_at


def noise(R=5, seed=7, box=SKEW):
    """seeded noise: ambiguous cells, cells with many sheets, both diagonals; the normals are random, of any length, and
    every seventh row is NaN, every eleventh zero, every thirteenth infinite"""
    rng = np.random.RandomState(seed)
    vol = rng.standard_normal((R + 1) ** 3).astype(np.float32)

    def normals_at(points):
        r = np.random.RandomState(seed + 1)
        g = (r.standard_normal((len(points), 3)) * np.exp(r.uniform(-3, 3, (len(points), 1)))).astype(np.float32)
        g[::7] = np.nan
        g[3::11] = 0.0
        g[5::13, 1] = np.inf
        return g
    return vol, np.asarray(box, np.float64), 0.0, normals_at


def mesh(fixture, reg=2.0 ** -10):
    """(points, normals, verts, faces) of a fixture by the host specification"""
    from disn_amd import isosurface
    vol, box, iso, normals_at = fixture
    pts = isosurface.hermite_points_arrays(vol, box, iso)
    nrm = normals_at(pts)
    v, f = isosurface.dual_contour_arrays(vol, box, iso, nrm, reg)
    return pts, nrm, v, f


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a

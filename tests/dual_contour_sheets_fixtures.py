"""Fields and mesh-topology helpers for the per-sheet dual-contouring tests (tests/test_dual_contour_sheets_host.py,
tests/test_gpu_dual_contour_sheets.py): plain module, no test.  The fields follow ``dual_contour_fixtures``: (vol
float32 [(R+1)^3] in .dist order, box float64 [6], iso, normals_at); all are float32 with iso 0."""
from __future__ import annotations

import numpy as np

import dual_contour_fixtures as F

DISC_N = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])


def _numeric_normals(field):
    """normals_at of an analytic field f(p [m,3] float64): central differences of step 2^-12, not normalised"""
    def normals_at(points):
        p = np.asarray(points, np.float64)
        h = 2.0 ** -12
        g = np.stack([(field(p + h * np.eye(3)[k]) - field(p - h * np.eye(3)[k])) / (2 * h) for k in range(3)], 1)
        return g.astype(np.float32)
    return normals_at


def disc(w, R=12):
    """a thin oblique disc, f = max(|n.p - 0.11| - w, |p| - 0.7) in the unit box: at R = 12 a cell is 1/6 wide, so
    w = 0.03 .. 0.06 is 0.36 .. 0.72 of a cell thick and many cells hold both of its sheets"""
    def field(p):
        return np.maximum(np.abs(p @ DISC_N - 0.11) - w, np.linalg.norm(p, axis=-1) - 0.7)
    vol = field(F.grid(F.UNIT, R).astype(np.float64)).astype(np.float32).reshape(-1)
    return vol, F.UNIT.copy(), 0.0, _numeric_normals(field)


def two_spheres(gap=0.05, R=12, radius=0.4):
    """two spheres of radius 0.4 whose surfaces are ``gap`` apart along DISC_N: two parts closer than a cell"""
    c = (radius + gap / 2) * DISC_N

    def field(p):
        return np.minimum(np.linalg.norm(p - c, axis=-1), np.linalg.norm(p + c, axis=-1)) - radius
    vol = field(F.grid(F.UNIT, R).astype(np.float64)).astype(np.float32).reshape(-1)
    return vol, F.UNIT.copy(), 0.0, _numeric_normals(field)


def checker(R):
    """vol = +1 / -1 by the parity of ix + iy + iz: every grid edge is cut and every cell has four loops"""
    i = np.arange(R + 1)
    par = (i[:, None, None] + i[None, :, None] + i[None, None, :]) % 2
    vol = np.where(par == 0, 1.0, -1.0).astype(np.float32).reshape(-1)
    return vol, F.UNIT.copy(), 0.0, lambda points: np.ones((len(points), 3), np.float32)


def mesh(fixture, reg=2.0 ** -10):
    """(points, normals, verts, faces) of a fixture by the per-sheet host specification"""
    from disn_amd import isosurface
    vol, box, iso, normals_at = fixture
    pts = isosurface.hermite_points_arrays(vol, box, iso)
    nrm = normals_at(pts)
    v, f = isosurface.dual_contour_sheets_arrays(vol, box, iso, nrm, reg)
    return pts, nrm, v, f


# ---- topology of an indexed triangle mesh --------------------------------------------------------------------------
def edge_counts(faces, nv):
    """-> (undirected edges [m,2] sorted pairs, their face counts [m], the largest count of one DIRECTED edge)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    if not len(e):
        return np.zeros((0, 2), np.int64), np.zeros(0, np.int64), 0
    _, dcount = np.unique(e[:, 0] * nv + e[:, 1], return_counts=True)
    und, ucount = np.unique(np.sort(e, 1), axis=0, return_counts=True)
    return und, ucount, int(dcount.max())


def components(faces, nv):
    """the number of connected components among the vertices that a face uses"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    parent = np.arange(nv)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for a, b in np.concatenate([f[:, [0, 1]], f[:, [1, 2]]]):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return len({find(v) for v in np.unique(f)})


def topology(verts, faces):
    """{components, euler (V - E + F over the used vertices), over (edges with more than 2 faces), directed (the most
    often one directed edge occurs), repeats (faces that repeat an index)}"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    und, ucount, dmax = edge_counts(f, len(verts))
    used = len(np.unique(f))
    rep = int(((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).sum())
    return {"components": components(f, len(verts)), "euler": used - len(und) + len(f), "over": int((ucount > 2).sum()),
            "directed": dmax, "repeats": rep}

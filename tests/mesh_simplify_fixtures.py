"""Meshes and measures for the tests of the mesh simplification (``postprocess.simplify_arrays``, the specification,
and mesh_simplify.hip, its device restatement).  The meshes themselves are those of mesh_clean_fixtures.py; here are
the lattices they are clustered on, the box field of DESIGN 4za and the two measures taken on it."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_clean_fixtures as MF  # noqa: E402,F401

UNIT = np.array([-1, -1, -1, 1, 1, 1], np.float64)
SOUP_BOX = np.array([-0.3, -0.3, -0.3, 0.3, 0.3, 0.3], np.float64)
BOX_HALF = np.array([0.43, 0.37, 0.51])
BOX_CENTRE = np.array([0.03, -0.02, 0.01])
_CACHE = {}


def cached(key, make):
    """computed once, shared between the tests, never modified"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def quad():
    """a unit quad in the plane z = 0.1 on the lattice of [0,2]^3 with two cells per axis: vertices 0, 3 in cell
    (0,0,0), 1, 2 in cell (1,0,0) -> two clusters, both faces collapse"""
    v = np.array([[0.5, 0.25, 0.1], [1.5, 0.25, 0.1], [1.5, 0.75, 0.1], [0.5, 0.75, 0.1]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    return v, f, np.array([0, 0, 0, 2, 2, 2], np.float64), 2


def box_field(R=32):
    """the signed distance of the box (BOX_HALF, BOX_CENTRE) on the (R+1)^3 grid of [-1,1]^3 -> (vol, sdf_params)"""
    ax = np.linspace(-1.0, 1.0, R + 1)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    q = np.abs(np.stack([x, y, z], -1) - BOX_CENTRE) - BOX_HALF
    d = np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(-1), 0.0)
    return d.astype(np.float32), UNIT.copy()


def box_mesh(R=32):
    """marching cubes (the CPU oracle) of ``box_field``"""
    def make():
        from oracle import mc_oracle as M
        vol, box = box_field(R)
        v, f = M.marching_cubes(vol, box, 0.0)
        return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    return cached(("box_mesh", R), make)


def box_surface_distance(p):
    """|signed distance| of points to the true box surface, float64"""
    q = np.abs(np.asarray(p, np.float64) - BOX_CENTRE) - BOX_HALF
    return np.abs(np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(-1), 0.0))


def volume(v, f):
    """signed volume of a closed oriented mesh, float64 (the sign follows the orientation)"""
    p = np.asarray(v, np.float64)
    a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def device_cases():
    """name -> (verts, faces, box, cells): what the device is compared with ``simplify_arrays`` on"""
    def make():
        from oracle import mc_oracle as M
        cases = {"fans": MF.fans() + (UNIT, 16)}
        for nv, nf in MF.SOUPS:
            cases["soup %d %d" % (nv, nf)] = MF.soup(nv, nf) + (SOUP_BOX, 4)
        cases["strip"] = MF.strip() + (SOUP_BOX, 64)
        cases["crowd"] = MF.crowd() + (SOUP_BOX, 16)
        cases["box"] = box_mesh(32) + (UNIT, 8)
        vol, box = MF.field_grid(16)
        mv, mf = M.marching_cubes(vol, box, 0.0)
        cases["field_grid"] = (np.ascontiguousarray(mv, np.float32), np.ascontiguousarray(mf, np.int32), box, 8)
        return cases
    return cached("device_cases", make)


def host_simplify(name, dedup=True):
    """``simplify_arrays`` of a device case, computed once"""
    def make():
        from disn_amd import postprocess
        v, f, box, cells = device_cases()[name]
        return postprocess.simplify_arrays(v, f, box, cells, dedup)
    return cached(("host", name, dedup), make)


BATCH_BOXES = (UNIT, np.array([-0.7, -0.4, -0.4, 0.7, 0.4, 0.4], np.float64), UNIT,
               np.array([-0.3, -0.3, -0.3, 0.3, 0.3, 0.3], np.float64), np.array([-0.1, -0.1, 0.0, 0.4, 0.4, 0.4], np.float64))
BATCH_CELLS = (16, 12, 5, 16, 3)

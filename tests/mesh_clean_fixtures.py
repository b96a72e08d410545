"""Meshes for the tests of the device small-part cleanup (mesh_clean.hip) and their host reference: the host path
``postprocess.separate_mesh`` / ``postprocess.clean_arrays``.  Every fixture keeps each part's centroid distance at
least 1e-6 away from ``dist_thresh`` and each vertex count different from ``biggest * num_thresh`` (``assert_margins``,
checked through the host functions before a comparison): the device sums a part's coordinates in float64 in an
order of its own, so only there could a keep decision differ."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from voxel_reference import components, icosphere  # noqa: E402,F401

DEFAULT = (0.5, 0.3)


def fans():
    """two fans meeting in vertex 0, vertex 7 referenced by nothing (the fixture of test_voxel_host.py)"""
    v = np.array([[0, 0, 0], [0.1, 0, 0], [0.1, 0.1, 0], [0, 0.1, 0], [-0.1, 0, 0], [-0.1, -0.1, 0], [0, -0.1, 0],
                  [0.4, 0.4, 0.4]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3], [0, 4, 5], [0, 5, 6]], np.int32)
    return v, f


SOUPS = ((40, 30), (300, 150), (2000, 1500), (50, 400), (50, 4000))


def soup(nv, nf, seed=5):
    """random index triples: repeated vertices, edges shared by many triangles, duplicate triangles"""
    rng = np.random.default_rng(seed + nv + nf)
    f = rng.integers(0, nv, (nf, 3)).astype(np.int32)
    f[::7, 1] = f[::7, 0]
    v = rng.uniform(-0.3, 0.3, (nv, 3)).astype(np.float32)
    return v, f


def strip(n=4096, seed=3):
    """a strip of n triangles (i, i+1, i+2) in shuffled face order: one component, long hooking chains"""
    x = np.arange(n + 2, dtype=np.float32)
    v = np.stack([x / np.float32(n + 2) * np.float32(0.6) - np.float32(0.3), (x % 2) * np.float32(0.05),
                  np.zeros_like(x)], 1).astype(np.float32)
    f = np.stack([np.arange(n), np.arange(n) + 1, np.arange(n) + 2], 1).astype(np.int32)
    return v, f[np.random.default_rng(seed).permutation(n)]


def crowd(n=5000, seed=9):
    """n isolated triangles IN FRONT OF one icosphere of 162 vertices: n + 1 components over several scan blocks"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-0.2, 0.2, (n, 1, 3))
    tv = (c + rng.uniform(-0.01, 0.01, (n, 3, 3))).astype(np.float32).reshape(-1, 3)
    tf = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    sv, sf = icosphere(0.3, 2)
    return np.concatenate([tv, sv]), np.concatenate([tf, sf + 3 * n]).astype(np.int32)


def two_spheres():
    """42 vertices at 0.6 from the origin in front of 162 about it (test_voxel_host.py)"""
    v0, f0 = icosphere(0.3, 2)
    v1, f1 = icosphere(0.05, 1, (0.6, 0.0, 0.0))
    return np.concatenate([v1, v0]), np.concatenate([f1, f0 + v1.shape[0]]).astype(np.int32)


# (shift of the vertices, dist_thresh, num_thresh) -> kept: the four cases of the host test
RULE_CASES = ((0.0, 0.5, 0.3, [1]), (0.0, 0.5, 0.2, [1]), (0.0, 0.7, 0.2, [0, 1]), (2.0, 0.5, 0.3, None))


def empty():
    return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)


def batch_of_five():
    return [fans(), two_spheres(), empty(), crowd(), fans()]


def field_grid(R=16, k=0):
    """the union of three spheres on an (R+1)^3 grid of [-1,1]^3: radius 0.3 at the origin, 0.08 at distance 0.25 (a
    bump on the first), 0.2 at distance 0.7 on the other side (a far part); ``k`` = 0, 1, 2: the axis of the offsets -> (vol, box)"""
    ax = np.linspace(-1.0, 1.0, R + 1)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    p = np.stack([x, y, z], -1)
    e = np.roll(np.array([1.0, 0.0, 0.0]), k)
    d = np.minimum(np.minimum(np.linalg.norm(p, axis=-1) - 0.3, np.linalg.norm(p - 0.25 * e, axis=-1) - 0.08),
                   np.linalg.norm(p + 0.7 * e, axis=-1) - 0.2)
    return d.astype(np.float32), np.array([-1, -1, -1, 1, 1, 1], np.float64)


def part_distances(v, f, connectivity="face"):
    """host: (counts, centroid distance of every part)"""
    from disn_amd import postprocess
    labels, counts = postprocess.separate_mesh(v, f, connectivity)
    order = np.argsort(labels, kind="stable")
    bounds = np.searchsorted(labels[order], np.arange(counts.size + 1))
    d = np.empty(counts.size)
    for c in range(counts.size):
        used = np.unique(f[order[bounds[c]:bounds[c + 1]]])
        d[c] = np.sqrt(np.sum(np.square(v[used].astype(np.float64).mean(0))))
    return counts, d


def assert_margins(v, f, dist_thresh, num_thresh, connectivity="face"):
    """the condition on the inputs: no part within 1e-6 of dist_thresh, no count equal to biggest * num_thresh"""
    if f.shape[0] == 0:
        return
    counts, d = part_distances(v, f, connectivity)
    assert (np.abs(d - dist_thresh) >= 1e-6).all(), "a part's centroid lies within 1e-6 of dist_thresh"
    assert (counts.astype(np.float64) != counts.max() * num_thresh).all(), "a count equals biggest * num_thresh"


def host_clean(v, f, dist_thresh=0.5, num_thresh=0.3, connectivity="face"):
    """``clean_arrays`` -> (verts, faces, kept); None where nothing is kept; the empty mesh stays empty"""
    from disn_amd import postprocess
    if f.shape[0] == 0:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), []
    assert_margins(v, f, dist_thresh, num_thresh, connectivity)
    try:
        return postprocess.clean_arrays(v, f, dist_thresh, num_thresh, connectivity)
    except ValueError as e:
        assert "no part is kept" in str(e)
        return None

"""Small meshes for the mesh checks (postprocess.check_arrays, mesh_check.hip), on dyadic coordinates so that every
determinant is exact, each with the fields it must give written out by hand.  No test lives here.

``FIXTURES``: name -> (verts float32 [nv,3], faces int32 [nf,3], expected): ``expected`` holds every count of
postprocess.CHECK_FIELDS and the status; ``volume`` and ``area`` where they are exact in float64 whatever the order of
the sum.
"""
import numpy as np

_TET = [[0, 0, 0], [4, 0, 0], [0, 4, 0], [0, 0, 4]]
_TET_FACES = [[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]]          # outward
# the cube [0,2]^3, vertex x + 2 y + 4 z, outward; the last two faces are the top
_CUBE = [[2 * (i & 1), 2 * (i >> 1 & 1), 2 * (i >> 2 & 1)] for i in range(8)]
_CUBE_FACES = [[0, 2, 3], [0, 3, 1], [0, 1, 5], [0, 5, 4], [2, 7, 3], [2, 6, 7], [0, 4, 6], [0, 6, 2], [1, 3, 7],
               [1, 7, 5], [4, 5, 7], [4, 7, 6]]


def _mesh(verts, faces):
    return np.asarray(verts, np.float32).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3)


def _fields(nv, nf, **kw):
    out = dict(status=0, nv=nv, nf=nf, unreferenced_vertices=0, index_degenerate_faces=0, edges=0, boundary_edges=0,
               nonmanifold_edges=0, misoriented_edges=0, nonmanifold_vertices=0, euler=0, zero_area_faces=0,
               candidate_pairs=0, intersecting_pairs=0, intersecting_faces=0)
    out.update(kw)
    return out


def _remap(faces, table):
    return [[table[i] for i in f] for f in faces]


FIXTURES = {}
# closed, oriented, chi = 2; every two faces share an edge, so all 6 pairs are candidates; volume 4^3 / 6
FIXTURES["tetrahedron"] = _mesh(_TET, _TET_FACES) + (
    _fields(4, 4, edges=6, euler=2, candidate_pairs=6, volume=64.0 / 6.0),)
# the closed cube: 12 + 6 diagonals; two faces' boxes miss each other only when they lie in opposite sides: 3 x 4
# (its volume terms are sixths, each rounded: the sum is 8 only up to rounding, so none is stated)
FIXTURES["cube"] = _mesh(_CUBE, _CUBE_FACES) + (
    _fields(8, 12, edges=18, euler=2, candidate_pairs=66 - 12, area=24.0),)
# without its top: a disc, the 4 top edges on the boundary, the top's diagonal gone; 45 pairs less 2 x 4 opposite ones
FIXTURES["cube_open"] = _mesh(_CUBE, _CUBE_FACES[:10]) + (
    _fields(8, 10, edges=17, boundary_edges=4, euler=1, candidate_pairs=45 - 8, area=20.0),)
# face 2 turned over: its three edges run the same way in both their faces
FIXTURES["tetrahedron_flipped_face"] = _mesh(_TET, _TET_FACES[:2] + [[1, 3, 2]] + _TET_FACES[3:]) + (
    _fields(4, 4, edges=6, misoriented_edges=3, euler=2, candidate_pairs=6),)
# a second tetrahedron standing on the apex of the first (one index): a bow-tie vertex.  The boxes of the two solids
# meet in the plane z = 4: the 3 faces at the apex of the first against ALL 4 faces of the second, whose boxes all
# start at z = 4 over [0,4] x [0,4] or a side of it
FIXTURES["two_tetrahedra_at_a_vertex"] = _mesh(
    _TET + [[4, 0, 4], [0, 4, 4], [0, 0, 8]], _TET_FACES + _remap(_TET_FACES, {0: 3, 1: 4, 2: 5, 3: 6})) + (
    _fields(7, 8, edges=12, nonmanifold_vertices=1, euler=3, candidate_pairs=6 + 6 + 12),)
# a second tetrahedron mirrored in y and in z on the edge {0, 1}: that edge has 4 faces, every corner at 0 and at 1 is
# related through it.  Boxes: each solid's 6 pairs; across, [0,4]x[0,4]x[0,4] faces against [0,4]x[-4,0]x[-4,0] ones
# meet on y = 0 = z: all 16 pairs touch there, as every face of either solid reaches the x axis or the origin
FIXTURES["two_tetrahedra_on_an_edge"] = _mesh(
    _TET + [[0, -4, 0], [0, 0, -4]], _TET_FACES + _remap(_TET_FACES, {0: 0, 1: 1, 2: 4, 3: 5})) + (
    _fields(6, 8, edges=11, nonmanifold_edges=1, euler=3, candidate_pairs=6 + 6 + 16),)
FIXTURES["three_triangles_on_an_edge"] = _mesh(
    _TET + [[0, -4, 0]], [[0, 1, 2], [0, 1, 3], [0, 1, 4]]) + (
    _fields(5, 3, edges=7, boundary_edges=6, nonmanifold_edges=1, euler=1, candidate_pairs=3),)
# the second tetrahedron shifted by (1/2, 1/2, 1/2): its origin corner lies inside the first, its other three
# corners outside, so its three faces at that corner each cut the slanted face of the first and nothing else: 3 pairs
# over 4 faces.  The slanted face of the second lies beyond the first: only its box reaches that of the first's
FIXTURES["two_tetrahedra_interpenetrating"] = _mesh(
    _TET + [[x + 0.5, y + 0.5, z + 0.5] for x, y, z in _TET], _TET_FACES + [[i + 4 for i in f] for f in _TET_FACES]) + (
    _fields(8, 8, edges=12, euler=4, candidate_pairs=6 + 6 + 4, intersecting_pairs=3, intersecting_faces=4,
            volume=128.0 / 6.0),)
# the second tetrahedron shifted by (4, 0, 0), its own vertices: the solids touch in the point (4,0,0).  Across: the 3
# faces of the first at (4,0,0) against all 4 faces of the second, whose boxes all start at x = 4
FIXTURES["two_tetrahedra_touching"] = _mesh(
    _TET + [[x + 4, y, z] for x, y, z in _TET], _TET_FACES + [[i + 4 for i in f] for f in _TET_FACES]) + (
    _fields(8, 8, edges=12, euler=4, candidate_pairs=6 + 6 + 12, volume=128.0 / 6.0),)
FIXTURES["coplanar_overlap"] = _mesh(
    [[0, 0, 0], [4, 0, 0], [0, 4, 0], [1, 1, 0], [5, 1, 0], [1, 5, 0]], [[0, 1, 2], [3, 4, 5]]) + (
    _fields(6, 2, edges=6, boundary_edges=6, euler=2, candidate_pairs=1, area=16.0, volume=0.0),)
# two triangles with one common index, the opposite edge of the second goes through the first at (1,1,0)
FIXTURES["fold_over_at_a_vertex"] = _mesh(
    [[0, 0, 0], [4, 0, 0], [0, 4, 0], [1, 1, -1], [1, 1, 1]], [[0, 1, 2], [0, 3, 4]]) + (
    _fields(5, 2, edges=6, boundary_edges=6, nonmanifold_vertices=1, euler=1, candidate_pairs=1, intersecting_pairs=1,
            intersecting_faces=2),)
# a face with a repeated index beside the tetrahedron: counted, and no further part
FIXTURES["repeated_index"] = _mesh(_TET, _TET_FACES + [[0, 0, 1]]) + (
    _fields(4, 5, index_degenerate_faces=1, edges=6, euler=2, candidate_pairs=6, volume=64.0 / 6.0),)
FIXTURES["zero_area_face"] = _mesh([[0, 0, 0], [2, 0, 0], [4, 0, 0]], [[0, 1, 2]]) + (
    _fields(3, 1, edges=3, boundary_edges=3, euler=1, zero_area_faces=1, area=0.0, volume=0.0),)
FIXTURES["unreferenced_vertex"] = _mesh(_TET + [[8, 8, 8]], _TET_FACES) + (
    _fields(5, 4, unreferenced_vertices=1, edges=6, euler=2, candidate_pairs=6, volume=64.0 / 6.0),)
FIXTURES["single_triangle"] = _mesh(_TET[:3], [[0, 1, 2]]) + (
    _fields(3, 1, edges=3, boundary_edges=3, euler=1, area=8.0, volume=0.0),)
FIXTURES["empty"] = _mesh([], []) + (_fields(0, 0, area=0.0, volume=0.0),)
# 64 copies of one triangle, each with vertices of its own: one common box, 64 63 / 2 candidate pairs, all coplanar
STACK = 64
FIXTURES["stack"] = _mesh(_TET[:3] * STACK, [[3 * k, 3 * k + 1, 3 * k + 2] for k in range(STACK)]) + (
    _fields(3 * STACK, STACK, edges=3 * STACK, boundary_edges=3 * STACK, euler=STACK, candidate_pairs=2016,
            area=8.0 * STACK, volume=0.0),)

COUNT_KEYS = tuple(k for k in FIXTURES["empty"][2] if k not in ("area", "volume"))


def noise(R: int, seed: int) -> np.ndarray:
    """white noise on an (R+1)^3 grid, positive on the border: marching cubes of it is closed (the volume of
    tests/test_marching_cubes.py's _noise)"""
    v = np.random.default_rng(seed).standard_normal((R + 1,) * 3).astype(np.float32)
    v[0] = v[-1] = 1
    v[:, 0] = v[:, -1] = 1
    v[:, :, 0] = v[:, :, -1] = 1
    return v


def brute_force(verts, faces):
    """an independent restatement of the counts over ALL pairs, one pair at a time where check_arrays sweeps:
    -> (candidate_pairs, intersecting_pairs, intersecting_faces) of a mesh whose faces all take part"""
    v = np.asarray(verts, np.float32)
    f = np.asarray(faces, np.int64)
    p32 = v[f]
    lo, hi = p32.min(axis=1), p32.max(axis=1)
    p = p32.astype(np.float64)

    def det(a, b, c, d):
        m = np.stack([b - a, c - a, d - a], axis=-2)              # rows u, v, w; cofactors along the first row
        u, v_, w = m[..., 0, :], m[..., 1, :], m[..., 2, :]
        return (u[..., 0] * (v_[..., 1] * w[..., 2] - v_[..., 2] * w[..., 1])
                - u[..., 1] * (v_[..., 0] * w[..., 2] - v_[..., 2] * w[..., 0])
                + u[..., 2] * (v_[..., 0] * w[..., 1] - v_[..., 1] * w[..., 0]))

    def through(P, T):
        hit = np.zeros(len(P), bool)
        for k in range(3):
            e0, e1 = P[:, k], P[:, (k + 1) % 3]
            side = det(T[:, 0], T[:, 1], T[:, 2], e0) * det(T[:, 0], T[:, 1], T[:, 2], e1)
            s = np.stack([det(e0, e1, T[:, i], T[:, (i + 1) % 3]) for i in range(3)])
            hit |= (side < 0) & ((s > 0).all(axis=0) | (s < 0).all(axis=0))
        return hit

    cand = pairs = 0
    touched = np.zeros(len(f), bool)
    for i in range(len(f) - 1):
        j = np.arange(i + 1, len(f))
        j = j[((lo[j] <= hi[i]) & (lo[i] <= hi[j])).all(axis=1)]
        cand += j.size
        if j.size:
            Pi = np.broadcast_to(p[i], (j.size, 3, 3))
            hit = through(Pi, p[j]) | through(p[j], Pi)
            pairs += int(hit.sum())
            touched[j[hit]] = True
            touched[i] |= bool(hit.any())
    return cand, pairs, int(touched.sum())

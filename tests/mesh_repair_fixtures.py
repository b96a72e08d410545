"""Small meshes for the mesh repair (postprocess.repair_arrays, mesh_repair.hip), on dyadic coordinates so that every
determinant of the angular rule is exact, each with what the repair must give written out by hand.  No test lives here.

``FIXTURES``: name -> (verts float32 [nv,3], faces int32 [nf,3], (faces' [nf',3], vmap [nv'], kept [nf'], report)); the
output positions are ``verts[vmap]`` bit for bit (a gather), so they are not written out again.  The repair runs with its
defaults (weld and stitch).  Corner 3 f + k is index k of input face f: a vertex keeps the class of its smallest corner,
every further class becomes a new vertex, in the order of the classes' smallest corners.
"""
import numpy as np

import mesh_check_fixtures as X
from mesh_check_fixtures import _TET, _TET_FACES, _mesh, _remap

_FLIPPED = [[a, c, b] for a, b, c in _TET_FACES]                  # [[0,1,2],[0,3,1],[1,3,2],[0,2,3]]: inside out


def report(nv, nf, nv_out, nf_out, **kw):
    out = dict(status=0, nv=nv, nf=nf, nv_out=nv_out, nf_out=nf_out, welded_vertices=0, repeated_faces=0,
               duplicate_faces=0, pillow_faces=0, singular_edges=0, stitched_edges=0, pinched_edges=0, added_vertices=0,
               dropped_vertices=0)
    out.update(kw)
    return out


def _want(faces, vmap, kept, rep):
    return (np.asarray(faces, np.int32).reshape(-1, 3), np.asarray(vmap, np.int32).reshape(-1),
            np.asarray(kept, np.int32).reshape(-1), rep)


FIXTURES = {}
# the bow-tie: vertex 3 has the fan of the first solid (its smallest corner, 5, lies there) and that of the second,
# which becomes vertex 7, a copy of 3
FIXTURES["two_tetrahedra_at_a_vertex"] = X.FIXTURES["two_tetrahedra_at_a_vertex"][:2] + (_want(
    _TET_FACES + [[7, 5, 4], [7, 4, 6], [4, 5, 6], [7, 6, 5]], [0, 1, 2, 3, 4, 5, 6, 3], range(8),
    report(7, 8, 8, 8, added_vertices=1)),)
# edge {0,1} = the x axis, e = (4,0,0); its faces 0 (1 -> 0, opposite (0,4,0): the reference, rank 0), 1 (0 -> 1,
# (0,0,4): s > 0, rank 1), 4 (1 -> 0, (0,-4,0): s = 0, c < 0, half 1, rank 2), 5 (0 -> 1, (0,0,-4): s < 0, rank 3).  The
# directions alternate; the faces that run 1 -> 0 take the next rank: (0, 1) and (4, 5), each solid with itself.  The
# second solid's corners at 0 and at 1 (smallest: 12 and 14) become the vertices 6 and 7: two closed tetrahedra
FIXTURES["two_tetrahedra_on_an_edge"] = X.FIXTURES["two_tetrahedra_on_an_edge"][:2] + (_want(
    _TET_FACES + [[6, 4, 7], [6, 7, 5], [7, 4, 5], [6, 5, 4]], [0, 1, 2, 3, 4, 5, 0, 1], range(8),
    report(6, 8, 8, 8, singular_edges=1, stitched_edges=1, added_vertices=2)),)
# three faces: k is odd, the edge is cut; no other edge has a partner, so every corner is a class of its own
FIXTURES["three_triangles_on_an_edge"] = X.FIXTURES["three_triangles_on_an_edge"][:2] + (_want(
    [[0, 1, 2], [5, 6, 3], [7, 8, 4]], [0, 1, 2, 3, 4, 0, 1, 0, 1], range(3),
    report(5, 3, 9, 3, singular_edges=1, added_vertices=4)),)
# vertex 4 = (4,0,0) is welded into vertex 1, which then is a bow-tie and is split again: the second solid's fan
# (smallest corner 12) becomes the last vertex, a copy of 1; the vertices 5, 6, 7 move up by one
FIXTURES["two_tetrahedra_touching"] = X.FIXTURES["two_tetrahedra_touching"][:2] + (_want(
    _TET_FACES + [[7, 5, 4], [7, 4, 6], [4, 5, 6], [7, 6, 5]], [0, 1, 2, 3, 5, 6, 7, 1], range(8),
    report(8, 8, 8, 8, welded_vertices=1, dropped_vertices=1, added_vertices=1)),)
FIXTURES["repeated_index"] = X.FIXTURES["repeated_index"][:2] + (_want(
    _TET_FACES, range(4), range(4), report(4, 5, 4, 4, repeated_faces=1)),)
FIXTURES["unreferenced_vertex"] = X.FIXTURES["unreferenced_vertex"][:2] + (_want(
    _TET_FACES, range(4), range(4), report(5, 4, 4, 4, dropped_vertices=1)),)
# faces 0 and 1 hold the triple {0,1,2} in both orientations: both go, vertex 2 with them
FIXTURES["pillow"] = _mesh(_TET, [[0, 1, 2], [0, 2, 1], [0, 1, 3]]) + (_want(
    [[0, 1, 2]], [0, 1, 3], [2], report(4, 3, 3, 1, pillow_faces=2, dropped_vertices=1)),)
# face 1 is face 0 again, the same way round: it goes.  Faces 0 and 2 hold edge {0,1} from the same end: misoriented,
# but regular, so they are partners and stay joined
FIXTURES["duplicate_face"] = _mesh(_TET, [[0, 1, 2], [1, 2, 0], [0, 1, 3]]) + (_want(
    [[0, 1, 2], [0, 1, 3]], range(4), [0, 2], report(4, 3, 4, 2, duplicate_faces=1)),)
# vertex 3 = (-0, 0, -0) is vertex 0
FIXTURES["plus_minus_zero"] = _mesh([[0, 0, 0], [4, 0, 0], [0, 4, 0], [-0.0, 0, -0.0], [0, 0, 4]],
                                    [[0, 1, 2], [3, 4, 1]]) + (_want(
    [[0, 1, 2], [0, 3, 1]], [0, 1, 2, 4], range(2), report(5, 2, 4, 2, welded_vertices=1, dropped_vertices=1)),)
# four faces on edge {0,1} in the plane z = 0, opposite (0,4,0) (the reference), (4,4,0) (s = 0, c > 0: half 0, rank 1),
# (0,-4,0) and (4,-4,0) (s = 0, c < 0: half 1, and det(e, d_m, d_n) = 0 both ways: both have rank 2).  A tie: cut
FIXTURES["coplanar_four_face_edge"] = _mesh(
    [[0, 0, 0], [4, 0, 0], [0, 4, 0], [4, 4, 0], [0, -4, 0], [4, -4, 0]],
    [[0, 1, 2], [1, 0, 3], [1, 0, 4], [0, 1, 5]]) + (_want(
        [[0, 1, 2], [6, 7, 3], [8, 9, 4], [10, 11, 5]], [0, 1, 2, 3, 4, 5, 1, 0, 1, 0, 0, 1], range(4),
        report(6, 4, 12, 4, singular_edges=1, added_vertices=6)),)
# 18 faces around edge {0,1}, alternately 0 -> 1 and 1 -> 0, at 18 distinct angles: over the cap of 16, cut.  Face m > 0
# gets the copies 18 + 2 m and 19 + 2 m for its first and its second index
_RING = [[2, 4, 0], [2, 4, 1], [2, 4, 2], [2, 4, 4], [2, 2, 4], [2, 1, 4], [2, 0, 4], [2, -1, 4], [2, -2, 4], [2, -4, 4],
         [2, -4, 2], [2, -4, 1], [2, -4, 0], [2, -4, -1], [2, -4, -4], [2, 0, -4], [2, 4, -4], [2, 4, -1]]
FIXTURES["fan_of_18"] = _mesh(
    [[0, 0, 0], [4, 0, 0]] + _RING, [[0, 1, 2 + m] if m % 2 == 0 else [1, 0, 2 + m] for m in range(18)]) + (_want(
        [[0, 1, 2]] + [[18 + 2 * m, 19 + 2 * m, 2 + m] for m in range(1, 18)],
        list(range(20)) + [i for m in range(1, 18) for i in ((0, 1) if m % 2 == 0 else (1, 0))], range(18),
        report(20, 18, 54, 18, singular_edges=1, added_vertices=34)),)
# the two tetrahedra on an edge turned inside out: the same ranks (0, 1, 4, 5), the directions reversed, so the faces
# that run 1 -> 0 are 1 and 5 and the pairs are (1, 4) and (5, 0): the material lies BETWEEN the two cavities.  Through
# those pairs and the regular edges {0,2}, {0,3}, {0,4}, {0,5} all six corners at vertex 0 are one class -- the link of
# 0 becomes ONE closed curve that passes the edge twice -- and likewise at vertex 1: both pairs have the signature
# (corner 0, corner 1).  Pinched: the edge is cut, and each cavity closes over copies of its own
FIXTURES["pinched_edge"] = _mesh(
    _TET + [[0, -4, 0], [0, 0, -4]], _FLIPPED + _remap(_FLIPPED, {0: 0, 1: 1, 2: 4, 3: 5})) + (_want(
        _FLIPPED + [[6, 7, 4], [6, 5, 7], [7, 5, 4], [6, 4, 5]], [0, 1, 2, 3, 4, 5, 0, 1], range(8),
        report(6, 8, 8, 8, singular_edges=1, stitched_edges=1, pinched_edges=1, added_vertices=2)),)
FIXTURES["empty"] = _mesh([], []) + (_want([], [], [], report(0, 0, 0, 0)),)
# a status: the mesh as it came
FIXTURES["index_out_of_range"] = _mesh(_TET, _TET_FACES[:3] + [[0, 3, 4]]) + (_want(
    _TET_FACES[:3] + [[0, 3, 4]], range(4), range(4), report(4, 4, 4, 4, status=2)),)
FIXTURES["not_finite"] = _mesh([[0, 0, 0], [4, 0, 0], [0, float("inf"), 0], [0, 0, 4]], _TET_FACES) + (_want(
    _TET_FACES, range(4), range(4), report(4, 4, 4, 4, status=4)),)


def same_bits(a, b) -> bool:
    """two float32 arrays of one shape with the same bits (an infinity or a -0 included)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def noise_meshes():
    """name -> (verts, faces): per-cell and per-sheet dual contouring of noise(12, seed), seeds 0 and 1, box [-1,1]^3,
    iso 0, grid normals, and their ``simplify_arrays(cells=6)`` outputs; computed once"""
    if not _NOISE:
        from disn_amd import isosurface, postprocess
        box = np.array([-1, -1, -1, 1, 1, 1], np.float64)
        for seed in (0, 1):
            vol = X.noise(12, seed).reshape(-1)
            normals = isosurface.grid_normals_arrays(vol, box, 0.0)
            for name, fn in (("dc", isosurface.dual_contour_arrays), ("dcs", isosurface.dual_contour_sheets_arrays)):
                v, f = fn(vol, box, 0.0, normals)
                _NOISE["%s%d" % (name, seed)] = (v, f)
                _NOISE["%s%d_simplified" % (name, seed)] = postprocess.simplify_arrays(v, f, box, 6)[:2]
    return _NOISE


_NOISE = {}
_REPAIRED = {}


def repaired(name, weld=True, stitch=True):
    """``repair_arrays`` of a fixture or a noise mesh, computed once per (name, flags) and shared: do not change it"""
    key = (name, weld, stitch)
    if key not in _REPAIRED:
        from disn_amd import postprocess
        v, f = (FIXTURES[name] if name in FIXTURES else noise_meshes()[name])[:2]
        _REPAIRED[key] = postprocess.repair_arrays(v, f, weld, stitch)
    return _REPAIRED[key]

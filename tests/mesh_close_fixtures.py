"""Small meshes for the mesh closing (postprocess.close_arrays, mesh_close.hip), on dyadic coordinates whose loop sums
divide by the loop length, so that every centre is exact, each with what the closing must give written out by hand.  No
test lives here.

``FIXTURES``: name -> (verts float32 [nv,3], faces int32 [nf,3], cases); ``cases``: [(keywords of ``close_arrays``,
(faces' [nf',3], centres float32 [n,3], vmap [nv'], kept [nf'], report))].  The output positions are the input's, then
the centres.  Corner 3 f + k is the pair from index k to index (k+1)%3 of input face f; the fill faces stand in the
order of their pairs' corners, the centres in the order of their loops' smallest vertices.
"""
import numpy as np

import mesh_check_fixtures as X
import mesh_repair_fixtures as RX
from mesh_check_fixtures import _CUBE, _CUBE_FACES, _TET_FACES, _mesh

_TET6 = [[0, 0, 0], [6, 0, 0], [0, 6, 0], [0, 0, 6]]


def report(nv, nf, nv_out, nf_out, **kw):
    out = dict(status=0, nv=nv, nf=nf, nv_out=nv_out, nf_out=nf_out, components=0, unorientable_components=0,
               flipped_faces=0, loops=0, filled_loops=0, fill_faces=0)
    out.update(kw)
    return out


def _want(faces, centres, vmap, kept, rep):
    return (np.asarray(faces, np.int32).reshape(-1, 3), np.asarray(centres, np.float32).reshape(-1, 3),
            np.asarray(vmap, np.int32).reshape(-1), np.asarray(kept, np.int32).reshape(-1), rep)


def _unchanged(verts, faces, **kw):
    nv, nf = len(verts), len(faces)
    return _want(faces, [], range(nv), range(nf), report(nv, nf, nv, nf, **kw))


def _turned(faces, which=None):
    return [[a, c, b] if which is None or k in which else [a, b, c] for k, (a, b, c) in enumerate(faces)]


DEFAULT, OUTWARD = {}, {"outward": True}
NO_FILL, NO_ORIENT, NEITHER = {"fill": False}, {"orient": False}, {"orient": False, "fill": False}
FIXTURES = {}

# the face (0, 3, 2) is missing: its edges are the pairs 0 -> 2 (corner 0), 3 -> 0 (corner 5), 2 -> 3 (corner 7); the
# tails 0, 3, 2 add up to (0, 6, 6): the centre (0, 2, 2) is vertex 4
_f = _TET_FACES[:3]
FIXTURES["tetrahedron_missing_a_face"] = _mesh(_TET6, _f) + ([
    (DEFAULT, _want(_f + [[4, 2, 0], [4, 0, 3], [4, 3, 2]], [[0, 2, 2]], [0, 1, 2, 3, 0], [0, 1, 2, 0, 1, 2],
                    report(4, 3, 5, 6, components=1, loops=1, filled_loops=1, fill_faces=3))),
    (NO_FILL, _unchanged(_TET6, _f, components=1)),
    (NO_ORIENT, _want(_f + [[4, 2, 0], [4, 0, 3], [4, 3, 2]], [[0, 2, 2]], [0, 1, 2, 3, 0], [0, 1, 2, 0, 1, 2],
                      report(4, 3, 5, 6, loops=1, filled_loops=1, fill_faces=3))),
    (NEITHER, _unchanged(_TET6, _f)),
    ({"max_hole": 2}, _unchanged(_TET6, _f, components=1, loops=1)),
    ({"max_hole": 3, "outward": True}, _want(
        _f + [[4, 2, 0], [4, 0, 3], [4, 3, 2]], [[0, 2, 2]], [0, 1, 2, 3, 0], [0, 1, 2, 0, 1, 2],
        report(4, 3, 5, 6, components=1, loops=1, filled_loops=1, fill_faces=3)))],)

# the cube without its top, side face 2 = (0, 1, 5) turned over: parity 1 against nine of parity 0, so it is flipped
# back.  The top's edges are the pairs 5 -> 4 (corner 10, face 3), 6 -> 7 (16, face 5), 4 -> 6 (19, face 6) and 7 -> 5
# (28, face 9), none of the flipped face; the tails 5, 6, 4, 7 add up to (4, 4, 8): the centre (1, 1, 2) is vertex 8
_f = _turned(_CUBE_FACES[:10], {2})
_caps = [[8, 4, 5], [8, 7, 6], [8, 6, 4], [8, 5, 7]]
FIXTURES["cube_missing_its_top_one_side_flipped"] = _mesh(_CUBE, _f) + ([
    (DEFAULT, _want(_CUBE_FACES[:10] + _caps, [[1, 1, 2]], list(range(8)) + [4], list(range(10)) + [3, 5, 6, 9],
                    report(8, 10, 9, 14, components=1, flipped_faces=1, loops=1, filled_loops=1, fill_faces=4))),
    (OUTWARD, _want(_CUBE_FACES[:10] + _caps, [[1, 1, 2]], list(range(8)) + [4], list(range(10)) + [3, 5, 6, 9],
                    report(8, 10, 9, 14, components=1, flipped_faces=1, loops=1, filled_loops=1, fill_faces=4))),
    (NO_ORIENT, _want(_f + _caps, [[1, 1, 2]], list(range(8)) + [4], list(range(10)) + [3, 5, 6, 9],
                      report(8, 10, 9, 14, loops=1, filled_loops=1, fill_faces=4))),
    (NO_FILL, _want(_CUBE_FACES[:10], [], range(8), range(10), report(8, 10, 8, 10, components=1, flipped_faces=1)))],)

# a triangular tube, open at both ends, ONE component with two loops.  The first boundary pair in corner order, 4 -> 3
# (corner 1), belongs to the top loop {3, 4, 5}, yet the bottom loop {0, 1, 2} has the smaller id: its centre
# (2, 2, 0) is vertex 6, the top's (2, 2, 6) vertex 7.  The other pairs: 0 -> 1 (3), 1 -> 2 (6), 5 -> 4 (10), 2 -> 0
# (12), 3 -> 5 (16)
_PRISM = [[0, 0, 0], [6, 0, 0], [0, 6, 0], [0, 0, 6], [6, 0, 6], [0, 6, 6]]
_f = [[0, 4, 3], [0, 1, 4], [1, 2, 5], [1, 5, 4], [2, 0, 3], [2, 3, 5]]
FIXTURES["open_prism"] = _mesh(_PRISM, _f) + ([
    (DEFAULT, _want(_f + [[7, 3, 4], [6, 1, 0], [6, 2, 1], [7, 4, 5], [6, 0, 2], [7, 5, 3]], [[2, 2, 0], [2, 2, 6]],
                    [0, 1, 2, 3, 4, 5, 0, 3], list(range(6)) * 2,
                    report(6, 6, 8, 12, components=1, loops=2, filled_loops=2, fill_faces=6)))],)

# one triangle closes to a flat solid of 4 vertices and 4 faces; its volume is 0, which is not below 0
_TRI = [[0, 0, 0], [6, 0, 0], [0, 6, 0]]
_w = _want([[0, 1, 2], [3, 1, 0], [3, 2, 1], [3, 0, 2]], [[2, 2, 0]], [0, 1, 2, 0], [0, 0, 0, 0],
           report(3, 1, 4, 4, components=1, loops=1, filled_loops=1, fill_faces=3))
FIXTURES["single_triangle"] = _mesh(_TRI, [[0, 1, 2]]) + ([(DEFAULT, _w), (OUTWARD, _w)],)

# both faces hold the edge {0, 1} as 0 -> 1: related by 1, n0 = n1 = 1, a tie: the root, face 0, stays and face 1
# becomes (0, 3, 1).  The boundary pairs 1 -> 2 (corner 1), 2 -> 0 (2), 1 -> 3 (4), 3 -> 0 (5): one loop {0, 1, 2, 3}
# of length 4; the tails IN THE INPUT'S ORIENTATION are 1, 2, 1, 3 and add up to (8, 0, 8): the centre (2, 0, 2).  The
# pairs of the flipped face give (c, a, b)
_BOOK = [[0, 0, 0], [4, 0, 4], [0, 4, 0], [0, -4, 0]]
FIXTURES["two_triangles_the_same_way"] = _mesh(_BOOK, [[0, 1, 2], [0, 1, 3]]) + ([
    (DEFAULT, _want([[0, 1, 2], [0, 3, 1], [4, 2, 1], [4, 0, 2], [4, 1, 3], [4, 3, 0]], [[2, 0, 2]], [0, 1, 2, 3, 0],
                    [0, 1, 0, 0, 1, 1],
                    report(4, 2, 5, 6, components=1, flipped_faces=1, loops=1, filled_loops=1, fill_faces=4))),
    (NO_ORIENT, _want([[0, 1, 2], [0, 1, 3], [4, 2, 1], [4, 0, 2], [4, 3, 1], [4, 0, 3]], [[2, 0, 2]], [0, 1, 2, 3, 0],
                      [0, 1, 0, 0, 1, 1], report(4, 2, 5, 6, loops=1, filled_loops=1, fill_faces=4)))],)

# the Moebius band of 5 faces (i, i+1, i+2) mod 5: every edge {i, i+1} is held the same way by the faces i-1 and i, an
# odd cycle of relations 1: not orientable, nothing is flipped.  The pairs i+2 -> i (corner 3 i + 2) are ONE loop
# 2 -> 0 -> 3 -> 1 -> 4 -> 2 of length 5; the five vertices add up to (10, 10, 15): the centre (2, 2, 3)
_BAND = [[0, 0, 0], [5, 0, 0], [5, 5, 5], [0, 5, 5], [0, 0, 5]]
_f = [[i, (i + 1) % 5, (i + 2) % 5] for i in range(5)]
_w = _want(_f + [[5, i, (i + 2) % 5] for i in range(5)], [[2, 2, 3]], [0, 1, 2, 3, 4, 0], list(range(5)) * 2,
           report(5, 5, 6, 10, components=1, unorientable_components=1, loops=1, filled_loops=1, fill_faces=5))
FIXTURES["moebius_band"] = _mesh(_BAND, _f) + ([(DEFAULT, _w), (OUTWARD, _w)],)

# the cube [0,8]^3 facing outwards around a tetrahedral cavity that faces inwards: both consistent, nothing to do --
# unless ``outward`` is asked for, which turns the cavity's four faces over (documented as wrong for cavities)
_v = [[4 * x for x in p] for p in _CUBE] + [[1, 1, 1], [3, 1, 1], [1, 3, 1], [1, 1, 3]]
_in = [[i + 8 for i in f] for f in _TET_FACES]
FIXTURES["cavity_in_a_cube"] = _mesh(_v, _CUBE_FACES + _turned(_in)) + ([
    (DEFAULT, _unchanged(_v, _CUBE_FACES + _turned(_in), components=2)),
    (OUTWARD, _want(_CUBE_FACES + _in, [], range(12), range(16), report(12, 16, 12, 16, components=2, flipped_faces=4)))],)

# a pentagonal bipyramid, 10 faces, the first six turned over: against the root (face 0) they have parity 0, the four
# good ones parity 1, and the majority wins: the good ones are flipped and the solid faces inwards.  ``outward`` finds
# the volume negative and turns the six instead
_v = [[4, 0, 0], [1, 4, 0], [-3, 2, 0], [-3, -2, 0], [1, -4, 0], [0, 0, 4], [0, 0, -4]]
_good = [[i, (i + 1) % 5, 5] for i in range(5)] + [[(i + 1) % 5, i, 6] for i in range(5)]
FIXTURES["sixty_percent_flipped"] = _mesh(_v, _turned(_good, range(6))) + ([
    (DEFAULT, _want(_turned(_good), [], range(7), range(10), report(7, 10, 7, 10, components=1, flipped_faces=4))),
    (OUTWARD, _want(_good, [], range(7), range(10), report(7, 10, 7, 10, components=1, flipped_faces=6)))],)

# a cone over a rim of 300 integer points, symmetric about the axis (point i + 150 = -point i: the rim adds up to 0
# and the centre is the origin), the apex above: more boundary pairs than one workgroup has threads.  The sides face
# outwards, so the volume of the closed cone is positive
RIM = 300
_half = np.rint(1000.0 * np.stack([np.cos(np.arange(RIM // 2) * 2 * np.pi / RIM),
                                   np.sin(np.arange(RIM // 2) * 2 * np.pi / RIM), np.zeros(RIM // 2)], axis=1))
_v = np.concatenate([_half, -_half, [[0, 0, 700]]])
_f = [[i, (i + 1) % RIM, RIM] for i in range(RIM)]
_lid = [[RIM + 1, (i + 1) % RIM, i] for i in range(RIM)]
_closed = dict(components=1, loops=1, filled_loops=1, fill_faces=RIM)
_vm, _kp = list(range(RIM + 1)) + [0], list(range(RIM)) * 2
FIXTURES["cone"] = _mesh(_v, _f) + ([
    (DEFAULT, _want(_f + _lid, [[0, 0, 0]], _vm, _kp, report(RIM + 1, RIM, RIM + 2, 2 * RIM, **_closed))),
    (OUTWARD, _want(_f + _lid, [[0, 0, 0]], _vm, _kp, report(RIM + 1, RIM, RIM + 2, 2 * RIM, **_closed))),
    (NO_FILL, _unchanged(_v, _f, components=1)),
    (NO_ORIENT, _want(_f + _lid, [[0, 0, 0]], _vm, _kp,
                      report(RIM + 1, RIM, RIM + 2, 2 * RIM, loops=1, filled_loops=1, fill_faces=RIM))),
    (NEITHER, _unchanged(_v, _f)),
    ({"max_hole": RIM}, _want(_f + _lid, [[0, 0, 0]], _vm, _kp, report(RIM + 1, RIM, RIM + 2, 2 * RIM, **_closed)))],)
# the same cone inside out: consistent, so only ``outward`` turns it -- every face, and the lid is made to match --
# and not while its loop is over ``max_hole`` and stays open
FIXTURES["cone_inside_out"] = _mesh(_v, _turned(_f)) + ([
    (DEFAULT, _want(_turned(_f) + _turned(_lid), [[0, 0, 0]], _vm, _kp,
                    report(RIM + 1, RIM, RIM + 2, 2 * RIM, **_closed))),
    (OUTWARD, _want(_f + _lid, [[0, 0, 0]], _vm, _kp,
                    report(RIM + 1, RIM, RIM + 2, 2 * RIM, flipped_faces=RIM, **_closed))),
    ({"max_hole": RIM - 1, "outward": True}, _unchanged(_v, _turned(_f), components=1, loops=1))],)

# status 16: vertex 0 on four boundary edges; an edge of three faces; a face with a repeated index
for _name, _src in (("fold_over_at_a_vertex", X), ("three_triangles_on_an_edge", X), ("repeated_index", X)):
    _v, _f = _src.FIXTURES[_name][:2]
    FIXTURES[_name] = (_v, _f, [(DEFAULT, _unchanged(_v, _f, status=16)), (NEITHER, _unchanged(_v, _f, status=16))])
for _name, _status in (("index_out_of_range", 2), ("not_finite", 4)):
    _v, _f = RX.FIXTURES[_name][:2]
    FIXTURES[_name] = (_v, _f, [(DEFAULT, _unchanged(_v, _f, status=_status))])
FIXTURES["empty"] = _mesh([], []) + ([(DEFAULT, _unchanged([], [])), (OUTWARD, _unchanged([], []))],)

CASES = [(name, k) for name, m in FIXTURES.items() for k in range(len(m[2]))]
same_bits = RX.same_bits
noise_meshes = RX.noise_meshes
NOISE = ["dc0", "dcs0", "dc1", "dcs1", "dc0_simplified", "dcs0_simplified", "dc1_simplified", "dcs1_simplified"]
_CLOSED = {}


def closed(name, case=0, **kw):
    """``close_arrays`` of a fixture's case, or (``kw``) of a repaired noise mesh, computed once and shared: do not
    change it"""
    key = (name, case, tuple(sorted(kw.items())))
    if key not in _CLOSED:
        from disn_amd import postprocess
        if name in FIXTURES:
            v, f, cases = FIXTURES[name]
            _CLOSED[key] = postprocess.close_arrays(v, f, **cases[case][0])
        else:
            _CLOSED[key] = postprocess.close_arrays(*RX.repaired(name)[:2], **kw)
    return _CLOSED[key]

"""Exact dyadic-lattice fixtures for the geometry kernels' tie rules, with references in Python ``int`` and
``fractions.Fraction`` only.

Every geometry module is specified by a written rule that says what happens at equality.  The float32 restatements
(tests/*_reference.py) were written by the same hand as the kernels, and random inputs never land on an equality.
This module is a second, independent statement of each rule: it imports no restatement, no part of the library, and
does no float arithmetic (numpy only packs arrays).  Each fixture builder checks its own bit budget: coordinates are
integers times a stated power of two, small enough that every product and sum that the rule forms fits the 24-bit
significand of float32, so the kernels' float32 arithmetic is exact on them and a comparison at equality is decided
by the written rule alone.

A *strict mutant* of a rule swaps the closed comparison of one named clause for its open twin (``strict`` is the set
of clause names to swap); tests/test_geometry_lattice_host.py asserts how many items each mutant moves: a fixture
that a mutant does not move does not test that clause.

Users: tests/test_geometry_lattice_host.py (CPU: restatement == integer rule, reach of every clause) and
tests/test_gpu_geometry_lattice.py (device == integer rule, bit for bit).
"""
import math
import random
from fractions import Fraction

import numpy as np

BITS = 24      # float32 significand


def _fits(*values):
    """every integer magnitude is below 2^24: a float32 holds it, and a dyadic multiple of it, exactly"""
    return all(abs(int(v)) < (1 << BITS) for v in values)


def _scaled_f32(ints, den):
    """integers / den (a power of two) as float32, packed without arithmetic on floats: Fraction -> float is exact"""
    assert den & (den - 1) == 0
    a = np.asarray(ints, dtype=object)
    out = np.empty(a.shape, np.float32)
    flat = out.reshape(-1)
    for i, v in enumerate(a.reshape(-1)):
        assert _fits(v)
        flat[i] = float(Fraction(int(v), den))
    return out


# =====================================================================================================================
# 1. voxel.hip surface voxels.  Unit = 1/dim: h = 2 units, voxel key k is the CLOSED box of centre 2k and
# half side 1 per axis, so box faces are the odd integers.  13 separating axes; an axis separates when
# min > r || max < -r ("touching is overlap").
# =====================================================================================================================
VOXEL_CLAUSES = ("box", "edge", "plane")


def voxel_key_range(dim):
    """-> (kmin, nkeys): the keys whose corners c = (k -+ 1/2) * 2/dim all have 0 <= (c + 1.1) / 2.4 * dim < dim"""
    good = []
    for k in range(-3 * dim, 3 * dim + 1):
        ok = True
        for s in (-1, 1):
            c = Fraction(2 * k + s, dim)
            val = (c + Fraction(11, 10)) / Fraction(24, 10) * dim
            ok = ok and 0 <= val < dim
        if ok:
            good.append(k)
    assert good and good[-1] - good[0] + 1 == len(good)
    return good[0], len(good)


def _sep(q, r, strict):
    if strict:
        return min(q) >= r or max(q) <= -r
    return min(q) > r or max(q) < -r


def voxel_overlap(tri, key, strict=()):
    """tri: three integer points (units of 1/dim), key: integer voxel key -> the triangle overlaps the closed box"""
    v = [[p[a] - 2 * key[a] for a in range(3)] for p in tri]
    for a in range(3):
        if _sep([v[i][a] for i in range(3)], 1, "box" in strict):
            return False
    e = [[tri[(i + 1) % 3][a] - tri[i][a] for a in range(3)] for i in range(3)]
    for ex, ey, ez in e:
        if _sep([ez * p[1] - ey * p[2] for p in v], abs(ez) + abs(ey), "edge" in strict):
            return False
        if _sep([ex * p[2] - ez * p[0] for p in v], abs(ex) + abs(ez), "edge" in strict):
            return False
        if _sep([ey * p[0] - ex * p[1] for p in v], abs(ey) + abs(ex), "edge" in strict):
            return False
    n = (e[0][1] * e[1][2] - e[0][2] * e[1][1], e[0][2] * e[1][0] - e[0][0] * e[1][2],
         e[0][0] * e[1][1] - e[0][1] * e[1][0])
    s = n[0] * v[0][0] + n[1] * v[0][1] + n[2] * v[0][2]
    return not _sep([s], abs(n[0]) + abs(n[1]) + abs(n[2]), "plane" in strict)


def voxel_candidates(tri):
    """per axis the keys whose closed box meets the triangle's closed bounding interval: |2k - x| <= 1 for some x in
    [min, max].  (The box axes of the rule, hoisted; a strict mutant is tested on the same keys.)"""
    out = []
    for a in range(3):
        mn, mx = min(p[a] for p in tri), max(p[a] for p in tri)
        out.append(range(-((1 - mn) // 2), (mx + 1) // 2 + 1))      # ceil((mn - 1) / 2) .. floor((mx + 1) / 2)
    return out


def voxel_surface(tris, dim, strict=()):
    """-> (set of occupied (kx, ky, kz), overflow): overflow when some triangle overlaps a key outside the key range"""
    kmin, n = voxel_key_range(dim)
    cells, overflow = set(), False
    for tri in tris:
        rx, ry, rz = voxel_candidates(tri)
        for kx in rx:
            for ky in ry:
                for kz in rz:
                    if (kx, ky, kz) not in cells and voxel_overlap(tri, (kx, ky, kz), strict):
                        if all(kmin <= k < kmin + n for k in (kx, ky, kz)):
                            cells.add((kx, ky, kz))
                        else:
                            overflow = True
    return cells, overflow


def voxel_dense(cells, dim):
    """the occupied keys as the bool [n, n, n] array indexed [x, y, z] over the key range"""
    kmin, n = voxel_key_range(dim)
    dense = np.zeros((n, n, n), bool)
    for kx, ky, kz in cells:
        dense[kx - kmin, ky - kmin, kz - kmin] = True
    return dense


def voxel_candidate_cells(tri):
    rx, ry, rz = voxel_candidates(tri)
    return len(rx) * len(ry) * len(rz)


def voxel_fixture(dim, ties=True):
    """-> dict(tris: integer triangles in units of 1/dim, verts float32 [3T, 3], faces int32 [T, 3], groups).
    ``ties=False`` keeps the random lattice triangles only."""
    assert dim in (16, 32)
    kmin, n = voxel_key_range(dim)
    lo, hi = 2 * kmin - 1, 2 * (kmin + n - 1) + 1            # the extreme box faces of the key range
    rng = random.Random(1000 + dim)
    groups = {}

    def odd(a, b):
        return 2 * rng.randrange((a - 1) // 2 + 1, (b - 1) // 2 + 1) + 1

    rand = []
    for _ in range(96):
        c = [rng.randrange(lo + 5, hi - 4) for _ in range(3)]
        rand.append([[c[a] + rng.randrange(-3, 4) for a in range(3)] for _ in range(3)])
    groups["random"] = rand
    if ties:
        plane = []                                           # a triangle lying in a box-face plane (odd coordinate)
        for i in range(64):
            a = i % 3
            c = [rng.randrange(lo + 5, hi - 4) for _ in range(3)]
            t = [[c[b] + rng.randrange(-3, 4) for b in range(3)] for _ in range(3)]
            w = odd(lo + 2, hi - 2)
            for p in t:
                p[a] = w
            plane.append(t)
        groups["in a face plane"] = plane
        corner = []                                          # all three vertices on one box corner: eight voxels touch
        for _ in range(8):
            p = [odd(lo + 2, hi - 2) for _ in range(3)]
            corner.append([list(p), list(p), list(p)])
        groups["point on a corner"] = corner
        edge = []                                            # a segment along a box edge (two odd coordinates)
        for i in range(12):
            a = i % 3
            p, q = [odd(lo + 2, hi - 2) for _ in range(3)], None
            p[a] = rng.randrange(lo + 3, hi - 8)
            q = list(p)
            q[a] = p[a] + rng.randrange(1, 6)
            edge.append([p, q, list(q if i & 1 else p)])
        groups["segment on an edge"] = edge
        face = []                                            # degenerate faces with every vertex on a box face
        for i in range(12):
            a = i % 3
            p = [2 * rng.randrange((lo + 3) // 2, (hi - 3) // 2) for _ in range(3)]
            p[a] = odd(lo + 2, hi - 2)
            q = list(p)
            q[(a + 1) % 3] += 2 * rng.randrange(0, 3)
            face.append([p, q, list(p)])
        groups["degenerate on a face"] = face
        # voxel_big_kernel: its queue (> 64 candidate cells: a triangle in the face plane z = 1) and its multi-chunk
        # path (> 256: one across the grid, one across the grid in the same face plane)
        groups["queue"] = [[[-3, -5, 1], [3, -3, 1], [-1, 5, 1]]]
        groups["multi-chunk"] = [[[lo + 2, lo + 4, -1], [hi - 2, lo + 2, 1], [1, hi - 2, 5]],
                                 [[lo + 2, lo + 4, 1], [hi - 2, lo + 2, 1], [1, hi - 2, 1]]]
    tris = [t for g in groups.values() for t in g]
    if ties:
        assert 64 < voxel_candidate_cells(groups["queue"][0]) <= 256
        assert all(voxel_candidate_cells(t) > 256 for t in groups["multi-chunk"])
    flat = [p for t in tris for p in t]
    # bit budget: |v| <= M, |e| <= E; an edge axis forms 2*E*M, the normal 2*E*E, the plane 3*(2*E*E)*M
    M = max(abs(x) for p in flat for x in p) + 2 * (max(abs(kmin - 1), abs(kmin + n)) + 1)
    E = max(abs(t[(i + 1) % 3][a] - t[i][a]) for t in tris for i in range(3) for a in range(3))
    assert _fits(2 * E * M, 6 * E * E * M), (E, M)
    assert all(lo <= x <= hi for p in flat for x in p)
    verts = _scaled_f32(flat, dim)
    faces = np.arange(3 * len(tris), dtype=np.int32).reshape(-1, 3)
    return {"tris": tris, "verts": verts, "faces": faces, "groups": groups, "dim": dim}


def voxel_sentinel_triangle(dim):
    """a triangle wholly inside the box of sentinel key kmin - 1 (x axis) whose only contact with the key range is
    one vertex on the face it shares with key kmin: by the closed rule it overlaps kmin - 1, which raises the flag"""
    kmin, _ = voxel_key_range(dim)
    tri = [[2 * kmin - 1, 0, 0], [2 * kmin - 2, 1, 0], [2 * kmin - 2, 0, 1]]
    assert voxel_overlap(tri, (kmin - 1, 0, 0)) and voxel_overlap(tri, (kmin, 0, 0))
    assert not voxel_overlap(tri, (kmin, 0, 0), strict=("box",))
    return tri, _scaled_f32(tri, dim), np.arange(3, dtype=np.int32).reshape(1, 3)


# =====================================================================================================================
# 5. marching_cubes.hip.  A node is inside when v < iso; a grid edge is cut when its ends differ; the
# vertex sits at c0 + t*(c1 - c0), t = (iso - v0) / (v1 - v0).  Labels -1 / 0 / +1 stand for below / EQUAL / above
# iso: with the value sets {-1, -0.0, +0.0, 1} (iso 0) and {0, 1/2, 1} (iso 1/2) t is 0, 1/2 or 1, so a vertex of an
# edge with v0 == iso sits on its node.  The case tables are an argument (tools/gen_mc_tables.py builds them; this
# module imports nothing of the project).
# =====================================================================================================================
MC_CLAUSES = ("inside",)
MC_VALUES = {0: {-1: Fraction(-1), 0: Fraction(0), 1: Fraction(1)},            # keyed by 2 * iso
             1: {-1: Fraction(0), 0: Fraction(1, 2), 1: Fraction(1)}}
MC_PITCH = 3        # an isolated cell: nodes 3i+1 and 3i+2 per axis, an outside layer at 3i and 3i+3
MC_SIDE = 19        # 19^3 = 6859 slots >= 3^8 = 6561 labelings
MC_H_DEN = 4        # node spacing 1/4, the box starts at 1: every coordinate is a positive multiple of 1/8


def mc_labelings():
    """all 3^8 labelings of a cell's corners, corner c of the table order taking digit c (base 3) - 1"""
    out = []
    for i in range(3 ** 8):
        lab, k = [], i
        for _ in range(8):
            lab.append(k % 3 - 1)
            k //= 3
        out.append(tuple(lab))
    return out


def mc_single_volume(corners):
    """-> labels [n, n, n] int8 indexed [iz, iy, ix]: labeling number i in slot i of a 19^3 arrangement of isolated
    cells, everything else outside (+1).  ``corners``: the table's corner offsets [8][3] (dx, dy, dz)."""
    n = MC_PITCH * MC_SIDE + 1
    lab = np.ones((n, n, n), np.int8)
    for i, cell in enumerate(mc_labelings()):
        sx, sy, sz = i % MC_SIDE, (i // MC_SIDE) % MC_SIDE, i // (MC_SIDE * MC_SIDE)
        for c in range(8):
            dx, dy, dz = (int(v) for v in corners[c])
            lab[MC_PITCH * sz + 1 + dz, MC_PITCH * sy + 1 + dy, MC_PITCH * sx + 1 + dx] = cell[c]
    return lab


def mc_batch_volumes(corners):
    """-> labels [3^8, 3, 3, 3]: one R = 2 grid per labeling, the cell at nodes {0, 1}^3, node 2 outside"""
    cells = mc_labelings()
    lab = np.ones((len(cells), 3, 3, 3), np.int8)
    for i, cell in enumerate(cells):
        for c in range(8):
            dx, dy, dz = (int(v) for v in corners[c])
            lab[i, dz, dy, dx] = cell[c]
    return lab


def mc_values_f32(labels, iso2):
    """labels -> the float32 volume; at iso 0 the EQUAL label is +0.0 on even nodes and -0.0 on odd ones"""
    vals = MC_VALUES[iso2]
    out = np.empty(labels.shape, np.float32)
    for lab in (-1, 0, 1):
        out[labels == lab] = float(vals[lab])
    if iso2 == 0:
        idx = np.indices(labels.shape[-3:]).sum(0) & 1
        neg = np.empty(1, np.float32)
        neg.view(np.uint32)[0] = 0x80000000
        out[(labels == 0) & (idx == 1)] = neg[0]
    return out


def mc_params(res):
    """the grid box: 1 .. 1 + res/4 per axis (node spacing 1/4 exactly, in float32 and in float64)"""
    return [1.0, 1.0, 1.0] + [float(Fraction(MC_H_DEN + res, MC_H_DEN))] * 3


def mc_reference(labels, iso2, ntri, tri, edge_geom, strict=()):
    """labels [n, n, n] ([iz, iy, ix]) -> (verts: integer triples in units of 1/8, faces: index triples), in the
    kernels' order: vertex id = rank of the cut edge in the flat order 3*p + axis, p = (iz*n + iy)*n + ix; faces by
    cell in flat order over (n-1)^3, triangles in table order."""
    n = labels.shape[0]
    lab = labels.tolist()
    vals = MC_VALUES[iso2]
    iso = Fraction(iso2, 2)
    if "inside" in strict:
        inside = [[[vals[v] <= iso for v in row] for row in pl] for pl in lab]
    else:
        inside = [[[vals[v] < iso for v in row] for row in pl] for pl in lab]
    near = set()                                  # nodes with an inside node among themselves and their + neighbours
    for iz in range(n):
        for iy in range(n):
            row = inside[iz][iy]
            for ix in range(n):
                if row[ix]:
                    for dz in (0, -1):
                        for dy in (0, -1):
                            for dx in (0, -1):
                                if iz + dz >= 0 and iy + dy >= 0 and ix + dx >= 0:
                                    near.add(((iz + dz) * n + iy + dy) * n + ix + dx)
    step = ((0, 0, 1), (0, 1, 0), (1, 0, 0))       # (dz, dy, dx) of axis x, y, z
    vid, verts = {}, []
    for p in sorted(near):
        iz, iy, ix = p // (n * n), (p // n) % n, p % n
        for a in range(3):
            jz, jy, jx = iz + step[a][0], iy + step[a][1], ix + step[a][2]
            if max(jz, jy, jx) >= n or inside[iz][iy][ix] == inside[jz][jy][jx]:
                continue
            v0, v1 = vals[lab[iz][iy][ix]], vals[lab[jz][jy][jx]]
            t = (iso - v0) / (v1 - v0)
            assert t in (0, Fraction(1, 2), 1) or strict
            pos = [2 * (MC_H_DEN + ix), 2 * (MC_H_DEN + iy), 2 * (MC_H_DEN + iz)]      # units of 1/8
            t2 = 2 * t
            assert t2.denominator == 1
            pos[a] += int(t2)
            vid[3 * p + a] = len(verts)
            verts.append(tuple(pos))
    faces = []
    R = n - 1
    for p in sorted(near):
        iz, iy, ix = p // (n * n), (p // n) % n, p % n
        if max(iz, iy, ix) >= R:
            continue
        mask = 0
        for c, (dx, dy, dz) in enumerate(MC_CORNERS):
            mask |= int(inside[iz + dz][iy + dy][ix + dx]) << c
        for k in range(int(ntri[mask])):
            f = []
            for j in range(3):
                dx, dy, dz, a = (int(v) for v in edge_geom[int(tri[mask][3 * k + j])])
                f.append(vid[3 * (((iz + dz) * n + iy + dy) * n + ix + dx) + a])
            faces.append(tuple(f))
    return verts, faces


# the corner numbering of the classic table (bit c of the mask is corner c): checked against the table's own in the tests
MC_CORNERS = ((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1))


def mc_pack(verts, faces):
    v = _scaled_f32(verts, 8).reshape(-1, 3) if verts else np.zeros((0, 3), np.float32)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    return v, f


# =====================================================================================================================
# 2. mesh_sdf.hip.  The grid is [-1, 1]^3 with res cells per axis; coordinates here are integers in
# units of 1/(2*res) (a quarter cell) measured from the box's low corner, so node i sits at 4*i and the world
# coordinate is -1 + c / (2*res).  Unsigned distance: the exact rational d^2 to the closed triangle.  Sign: far nodes
# (u >= tau) of components touching the box boundary are outside; then `steps` Jacobi steps in which a band node
# (u < tau) becomes outside when a 6-neighbour is outside and "the closed edge crosses no closed triangle":
# in the plane across the edge, w_p, w_q, w_r all >= 0 or all <= 0 with area != 0 (area == 0: ignored), and the
# crossing coordinate x in [x0, x1].
# =====================================================================================================================
SDF_CLAUSES = ("triangle", "edge")
SDF_NODE = 4        # lattice units per grid cell
# the fixtures whose unsigned distance is compared with float32(sqrt(rational d^2)) bit for bit, at most 2 % of the nodes
# excepted: their faces all lie in coordinate planes, so the foot of every perpendicular is a lattice point.  An
# octahedron's face normal has |n|^2 = 3 * 2^k, a divisor that is no power of two: the octahedra serve the sign pass
# only (their distance is held to the module's 1e-6 bar, as everywhere)
SDF_AXIS_ALIGNED = ("box", "thin box", "box off the nodes", "sheet")


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _seg_d2(p, a, b):
    ab, ap = _sub(b, a), _sub(p, a)
    den, num = _dot(ab, ab), _dot(ap, ab)
    if den == 0 or num <= 0:
        return Fraction(_dot(ap, ap))
    if num >= den:
        bp = _sub(p, b)
        return Fraction(_dot(bp, bp))
    return Fraction(_dot(ap, ap) * den - num * num, den)


def point_tri_d2(p, tri):
    """the exact squared distance of an integer point to a closed triangle: the least of the three edge distances
    and, where the foot of the perpendicular lies in the closed triangle, the distance to the plane"""
    a, b, c = tri
    best = min(_seg_d2(p, a, b), _seg_d2(p, b, c), _seg_d2(p, c, a))
    n = _cross(_sub(b, a), _sub(c, a))
    nn = _dot(n, n)
    if nn:
        inside = all(_dot(_cross(_sub(v, u), _sub(p, u)), n) >= 0 for u, v in ((a, b), (b, c), (c, a)))
        if inside:
            best = min(best, Fraction(_dot(n, _sub(p, a)) ** 2, nn))
    return best


def sqrt_to_f32(q):
    """the float32 nearest sqrt(q) (ties to even) for a rational q >= 0, as an exact Fraction; integers only"""
    q = Fraction(q)
    if q == 0:
        return Fraction(0)
    e = 0                                           # scale so that 2^23 <= sqrt(q) * 2^e < 2^24
    while q * 4 ** e < 1 << 46:
        e += 1
    while q * 4 ** e >= 1 << 48:
        e -= 1
    s = q * 4 ** e if e >= 0 else q / 4 ** (-e)
    m = math.isqrt(s.numerator // s.denominator)
    assert (1 << 23) <= m < (1 << 24)
    half = Fraction(2 * m + 1, 2) ** 2               # (m + 1/2)^2 against s
    if s > half or (s == half and m & 1):
        m += 1
    return Fraction(m) * Fraction(2) ** (-e)


def sdf_nodes(res):
    """node coordinates in flat order (iz, iy, ix), x fastest"""
    n = res + 1
    return [(SDF_NODE * ix, SDF_NODE * iy, SDF_NODE * iz) for iz in range(n) for iy in range(n) for ix in range(n)]


def sdf_d2(points, tris):
    return [min(point_tri_d2(p, t) for t in tris) for p in points]


def edge_crosses(tris, a, x0, x1, sb, sc, strict=()):
    """does the grid edge along axis a from x0 to x1 (x0 < x1) at (sb, sc) on axes b = (a+1)%3, c = (a+2)%3 cross a
    triangle?  -> (crosses, clauses): clauses is the set of ways a crossing was met at equality"""
    b, c = (a + 1) % 3, (a + 2) % 3
    for P, Q, R in tris:
        pb, pc, qb, qc, rb, rc = P[b] - sb, P[c] - sc, Q[b] - sb, Q[c] - sc, R[b] - sb, R[c] - sc
        wp, wq, wr = qb * rc - qc * rb, rb * pc - rc * pb, pb * qc - pc * qb
        area = wp + wq + wr
        if area == 0:
            continue
        if "triangle" in strict:
            hit = (wp > 0 and wq > 0 and wr > 0) or (wp < 0 and wq < 0 and wr < 0)
        else:
            hit = (wp >= 0 and wq >= 0 and wr >= 0) or (wp <= 0 and wq <= 0 and wr <= 0)
        if not hit:
            continue
        x = Fraction(wp * P[a] + wq * Q[a] + wr * R[a], area)
        if (x0 < x < x1) if "edge" in strict else (x0 <= x <= x1):
            return True
    return False


def sdf_sign(res, tris, d2, tau2, steps, strict=()):
    """-> outside: list of bool in flat node order.  d2: exact squared distances at the nodes, tau2 = tau^2 in
    lattice units"""
    n = res + 1
    N = n * n * n
    far = [d >= tau2 for d in d2]
    out = [False] * N
    stride = (1, n, n * n)

    def idx(i):
        return (i % n, (i // n) % n, i // (n * n))

    stack = []
    for i in range(N):
        if far[i] and any(v in (0, n - 1) for v in idx(i)):
            out[i] = True
            stack.append(i)
    while stack:
        i = stack.pop()
        id3 = idx(i)
        for a in range(3):
            for s in (-1, 1):
                if 0 <= id3[a] + s < n:
                    j = i + s * stride[a]
                    if far[j] and not out[j]:
                        out[j] = True
                        stack.append(j)
    cache = {}

    def crosses(i, a):                                # the edge from node i to its +a neighbour
        if (i, a) not in cache:
            id3 = idx(i)
            b, c = (a + 1) % 3, (a + 2) % 3
            cache[(i, a)] = edge_crosses(tris, a, SDF_NODE * id3[a], SDF_NODE * (id3[a] + 1), SDF_NODE * id3[b],
                                         SDF_NODE * id3[c], strict)
        return cache[(i, a)]

    for _ in range(steps):
        nxt = list(out)
        for i in range(N):
            if out[i] or far[i]:
                continue
            id3 = idx(i)
            for a in range(3):
                if id3[a] > 0 and out[i - stride[a]] and not crosses(i - stride[a], a):
                    nxt[i] = True
                if id3[a] < n - 1 and out[i + stride[a]] and not crosses(i, a):
                    nxt[i] = True
        out = nxt
    return out


def _box_tris(lo, hi):
    """an axis-aligned box, two triangles per face"""
    v = [tuple(lo[a] if not (i >> a) & 1 else hi[a] for a in range(3)) for i in range(8)]
    quads = ((0, 2, 6, 4), (1, 5, 7, 3), (0, 4, 5, 1), (2, 3, 7, 6), (0, 1, 3, 2), (4, 6, 7, 5))
    return [t for a, b, c, d in quads for t in ((v[a], v[b], v[c]), (v[a], v[c], v[d]))]


def _octa_tris(c, r):
    px, mx = (c[0] + r, c[1], c[2]), (c[0] - r, c[1], c[2])
    py, my = (c[0], c[1] + r, c[2]), (c[0], c[1] - r, c[2])
    pz, mz = (c[0], c[1], c[2] + r), (c[0], c[1], c[2] - r)
    return [(px, py, pz), (py, mx, pz), (mx, my, pz), (my, px, pz), (py, px, mz), (mx, py, mz), (my, mx, mz),
            (px, my, mz)]


def sdf_fixtures(res):
    """-> {name: dict(tris, kind)}: meshes in lattice units (node i at 4*i).  kind "box": a closed box on node planes
    (ground truth: outside == not in the closed box, given as lo / hi); the others hit one crossing clause each."""
    assert res in (8, 16)
    k = res // 8
    N = SDF_NODE
    fx = {}
    lo, hi = (N * 2 * k, N * 3 * k, N * 2 * k), (N * 6 * k, N * 6 * k, N * (5 * k + (k - 1)))
    fx["box"] = {"tris": _box_tris(lo, hi), "lo": lo, "hi": hi}
    # a small box whose interior holds one layer of nodes, at distance exactly h = tau from two faces (u >= tau is far)
    lo2, hi2 = (N * 1, N * 1, N * 1), (N * 3, N * (res - 1), N * 4)
    fx["thin box"] = {"tris": _box_tris(lo2, hi2), "lo": lo2, "hi": hi2}
    # half a cell off the node planes in z: its corners lie inside grid edges along z (a triangle vertex on a grid edge)
    # and the diagonals of its two z faces, each shared by two triangles, cut grid edges along z in two
    lo3, hi3 = (N * 2 * k, N * 2 * k, N * 2 * k + 2), (N * 5 * k, N * 6 * k, N * 5 * k + 2)
    fx["box off the nodes"] = {"tris": _box_tris(lo3, hi3), "lo": lo3, "hi": hi3}
    c = N * (res // 2)
    # half a cell off the node planes in z: the equatorial vertices lie inside grid edges along z (a triangle vertex
    # on a grid edge), and the equator's mesh edges, shared by an upper and a lower triangle, cut grid edges in two
    fx["octahedron off the nodes"] = {"tris": _octa_tris((c, c, c + 2), 2 * N)}
    # vertices on nodes, mesh edges through nodes: every contact is at a grid edge's end
    fx["octahedron on the nodes"] = {"tris": _octa_tris((c, c, c), 2 * N)}
    # a square sheet in a node plane: grid edges that end on it, and grid edges that lie in its plane (area 0)
    s0, s1, z = N * 1, N * (res - 1), N * (res // 2)
    fx["sheet"] = {"tris": [((s0, s0, z), (s1, s0, z), (s1, s1, z)), ((s0, s0, z), (s1, s1, z), (s0, s1, z))],
                   "sheet": (s0, s1, z)}
    for f in fx.values():
        flat = [x for t in f["tris"] for p in t for x in p]
        assert all(0 <= x <= N * res for x in flat)
        # bit budget of the float32 distance: differences < 2^7, dot products of two < 2^16, products of two dot
        # products < 2^32 are NOT all exact in float32: bit equality is claimed only where the restatement agrees
        # (tests cap the rest); the float64 crossing test forms |w| < 2^15 and |w * x| < 2^23: exact
        assert _fits(3 * (2 * N * res) ** 2 * N * res)
    return fx


def sdf_world(points, res):
    """lattice points -> float32 world coordinates -1 + c / (2*res)"""
    den = 2 * res
    return _scaled_f32([[x - den for x in p] for p in points], den)


def sdf_mesh_arrays(tris, res):
    verts = sdf_world([p for t in tris for p in t], res)
    return verts, np.arange(3 * len(tris), dtype=np.int32).reshape(-1, 3)


# =====================================================================================================================
# 3. render.hip.  Moeller-Trumbore, two-sided: det = e1 . (dir x e2) (0: skipped), u = tv . p / det,
# v = dir . q / det, t = e2 . q / det; a hit when u >= 0, v >= 0, u + v <= 1, t > 0; the nearest hit wins and equal t
# goes to the lowest file-order face.  The camera org (0, 0, -4), d0 (-1/2, -1/2, 1), dx (1/16, 0, 0), dy (0, 1/16, 0)
# sends the sample rays of a 16 x 16 image through the 1/8 lattice (S = 1) or the 1/16 lattice (S = 2) of the plane
# z = 0, at t = 4 exactly.  A second camera, d0 (-15/32, -15/32, 1), gives pixel column 7 dir.x == 0 and pixel row 7
# dir.y == 0 at S = 1: those rays lie in the planes x = 0 and y = 0 through the origin of the rays, the containment
# branch of the BVH walk's slab test, and the scene "axis" puts triangle edges, hence leaf and inner box faces, on
# both planes.  Vertices are integers in units of 1/8, directions in units of 1/64.
# =====================================================================================================================
RENDER_CLAUSES = ("u", "v", "u+v", "tie")
RENDER_CAM = (0.0, 0.0, -4.0, -0.5, -0.5, 1.0, 0.0625, 0.0, 0.0, 0.0, 0.0625, 0.0)
RENDER_CAM_AXIS = (0.0, 0.0, -4.0, -0.46875, -0.46875, 1.0, 0.0625, 0.0, 0.0, 0.0, 0.0625, 0.0)
RENDER_SCENES = ("corners 7/8", "dyadic", "axis")
RENDER_SIZE = 16
_RA, _RD = 8, 64                     # vertex units 1/8, direction units 1/64
_RORG = (0, 0, -4 * _RA)


def render_camera(kind):
    """-> (the 12 camera floats, d0.x = d0.y as a Fraction) of a scene"""
    return (RENDER_CAM_AXIS, Fraction(-15, 32)) if kind == "axis" else (RENDER_CAM, Fraction(-1, 2))


def render_dir(i, j, sy, sx, S, d0=Fraction(-1, 2)):
    """the direction of sample (sy, sx) of pixel (row i, col j) in units of 1/64: x = j + (sx + 1/2)/S"""
    x = Fraction(j) + Fraction(2 * sx + 1, 2 * S)
    y = Fraction(i) + Fraction(2 * sy + 1, 2 * S)
    d = (d0 + x / 16, d0 + y / 16, Fraction(1))
    out = tuple(v * _RD for v in d)
    assert all(v.denominator == 1 for v in out)
    return tuple(int(v) for v in out)


def render_trace(d, tris, strict=()):
    """-> (t as a Fraction or None, face or -1, dyadic): the exact hit of the ray org + t*d.  ``dyadic`` is False
    when some triangle meets the ray at u + v == 1 with a det that is no power of two: float32 rounds u and v there,
    so the kernel's decision on that ray is reported, not asserted (u == 0 and v == 0 are exact for any det: 0 / det)."""
    best_t, best_f, dyadic = None, -1, True
    for f, (a, b, c) in enumerate(tris):
        e1, e2 = _sub(b, a), _sub(c, a)
        p = _cross(d, e2)
        det = _dot(e1, p)
        if det == 0:
            continue
        s = 1 if det > 0 else -1
        tv = _sub(_RORG, a)
        un = _dot(tv, p) * s
        q = _cross(tv, e1)
        vn = _dot(d, q) * s
        tn = _dot(e2, q) * s
        ad = det * s
        pow2 = ad & (ad - 1) == 0
        assert _fits(un, vn, tn, ad)                 # bit budget: every numerator and det is a float32 integer
        if un >= 0 and vn >= 0 and tn > 0 and un + vn == ad and not pow2:
            dyadic = False
        ok_u = un > 0 if "u" in strict else un >= 0
        ok_v = vn > 0 if "v" in strict else vn >= 0
        ok_w = un + vn < ad if "u+v" in strict else un + vn <= ad
        if not (ok_u and ok_v and ok_w and tn > 0):
            continue
        t = Fraction(tn * _RD, ad * _RA)
        if best_t is None or t < best_t or (t == best_t and "tie" in strict):
            best_t, best_f = t, f                    # ("tie" mutant: equal t goes to the LAST face)
    return best_t, best_f, dyadic


def _square(x0, x1, y0, y1, z, flip=False):
    """two triangles split along the diagonal, each with its first vertex at a right-angle corner: the outer edges
    are u == 0 and v == 0, the shared diagonal is u + v == 1"""
    a, b, c, d = (x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)
    return [(b, c, a), (d, a, c)] if not flip else [(b, a, c), (d, c, a)]


def render_scene(kind):
    """-> triangles in file order (integer vertices, units of 1/8).
    "corners 7/8": the split square with corners +-7/8 at t = 4 (det 49/16: its diagonal is reported only);
    "dyadic": the split square [-7/8, 9/8]^2 (side 2, det 4): outer edges, vertices and the diagonal are all asserted.
    "axis" (for the camera with dir.x == 0 in column 7 and dir.y == 0 in row 7): four split unit squares that meet
    on the lines x = 0 and y = 0 of the plane z = 0, and behind them, at t = 8, a triangle with an edge on x = 0.
    All: 48 filler triangles first in the file (legs 1/2 at t = 12, so the tree has several leaves and leaf order is
    not file order), a triangle seen edge-on by pixel column 8 in front of everything, a square at t = 8 behind, and
    duplicates of the front square's faces at the end of the file."""
    assert kind in RENDER_SCENES
    rng = random.Random(7)
    tris = []
    for _ in range(48):
        x, y = 4 * rng.randrange(-14, 14) + 1, 4 * rng.randrange(-14, 14) + 1      # legs 1/2 on the 1/8 lattice
        tris.append(((x, y, 64), (x + 4, y, 64), (x, y + 4, 64)))
    # pixel column 8 has dir.x = 1/32: its rays lie in the plane x = (z + 4) / 32, and so does this triangle, which
    # reaches past the front square in y and stands before the square at t = 8: det == 0, so it is never seen
    tris.append(((1, -12, 0), (1, 12, 0), (2, 0, 32)))
    if kind == "axis":
        front = (_square(-8, 0, -8, 0, 0) + _square(0, 8, -8, 0, 0) + _square(-8, 0, 0, 8, 0) + _square(0, 8, 0, 8, 0))
        tris.append(((0, -32, 32), (0, 32, 32), (8, 0, 32)))       # its edge a-b (v == 0) lies in x = 0; det 8
    else:
        front = _square(-7, 7, -7, 7, 0) if kind == "corners 7/8" else _square(-7, 9, -7, 9, 0)
    tris += front
    tris += _square(-18, 14, -18, 14, 32, flip=True)       # t = 8: side 4, det 16; hit points on the 1/4 lattice
    tris += [front[0], (front[1][1], front[1][2], front[1][0])]      # duplicates; the second with rotated vertices
    return tris


def render_edge_on_face():
    """the file-order index of the triangle seen edge-on (it follows the 48 fillers)"""
    return 48


def render_pack(tris):
    verts = _scaled_f32([p for t in tris for p in t], _RA)
    return verts, np.arange(3 * len(tris), dtype=np.int32).reshape(-1, 3)


def render_expected(tris, S, strict=(), d0=Fraction(-1, 2)):
    """-> per pixel (face, depth Fraction or None, hits, dyadic) in row-major order: face / depth of the first
    sample with the smallest t, hits = samples that hit, dyadic = every sample of the pixel is"""
    out = []
    n = RENDER_SIZE
    for i in range(n):
        for j in range(n):
            hits, bt, bf, ok = 0, None, -1, True
            for sy in range(S):
                for sx in range(S):
                    t, f, dy = render_trace(render_dir(i, j, sy, sx, S, d0), tris, strict)
                    ok = ok and dy
                    if f < 0:
                        continue
                    hits += 1
                    if bt is None or t < bt:
                        bt, bf = t, f
            out.append((bf, bt, hits, ok))
    return out


# =====================================================================================================================
# 6. grid_band.hip selection and fill.  A coarse cell (stride s) with corner minimum lo and maximum hi
# is active when lo - t < iso && hi + t >= iso, t = margin * (hi - lo): with margin 0, lo == iso is INACTIVE however
# large hi is, and hi == iso is ACTIVE when lo < iso.  Then `rounds` rounds of 26-neighbour dilation clipped at the
# box.  The fill gives every point outside the closed boxes of the active cells the trilinear interpolant of its
# coarse cell's corners, t = k/s.  Field values are integers in units of 1/4; iso likewise; margin is 0 or 1/2.
# =====================================================================================================================
BAND_CLAUSES = ("lo", "hi")
BAND_R = 8
BAND_VALUE_DEN = 4
# (values the field draws from, iso), in units of 1/4
BAND_FIELDS = (((0, 1, 2, 3), 0), ((-3, -2, -1, 0), 0), ((-1, 0, 1), 0), ((1, 2, 3), 0), ((-3, -2, -1), 0),
               ((0, 1, 2, 3, 4), 2), ((2,), 2), ((0, 0, 0, 0, 0, 0, 0, -1, 4), 0), ((-4, 0, 0, 0, 0, 0, 0, 0, 1), 0))


def band_fields():
    """-> [(field: nested list [9][9][9] of integers indexed [iz][iy][ix], iso)]"""
    n = BAND_R + 1
    out = []
    for k, (vals, iso) in enumerate(BAND_FIELDS):
        rng = random.Random(50 + k)
        out.append(([[[rng.choice(vals) for _ in range(n)] for _ in range(n)] for _ in range(n)], iso))
    return out


def band_cell_rule(field, s, iso, margin, strict=()):
    C = BAND_R // s
    margin = Fraction(margin)
    out = [[[False] * C for _ in range(C)] for _ in range(C)]
    for cz in range(C):
        for cy in range(C):
            for cx in range(C):
                c = [field[(cz + dz) * s][(cy + dy) * s][(cx + dx) * s] for dz in (0, 1) for dy in (0, 1)
                     for dx in (0, 1)]
                lo, hi = min(c), max(c)
                t = margin * (hi - lo)
                assert (4 * t).denominator == 1        # margin 1/2 of a difference of quarter units: exact in float32
                a = lo - t <= iso if "lo" in strict else lo - t < iso
                b = hi + t > iso if "hi" in strict else hi + t >= iso
                out[cz][cy][cx] = a and b
    return out


def band_dilate(mask, rounds):
    C = len(mask)
    for _ in range(rounds):
        out = [[[False] * C for _ in range(C)] for _ in range(C)]
        for z in range(C):
            for y in range(C):
                for x in range(C):
                    out[z][y][x] = any(mask[z + dz][y + dy][x + dx] for dz in (-1, 0, 1) for dy in (-1, 0, 1)
                                       for dx in (-1, 0, 1)
                                       if 0 <= z + dz < C and 0 <= y + dy < C and 0 <= x + dx < C)
        mask = out
    return mask


def band_evaluated(mask, s):
    """the set of flat fine indices that are evaluated: the coarse lattice and the closed boxes of the active cells"""
    n, C = BAND_R + 1, len(mask)
    ev = set()
    for z in range(n):
        for y in range(n):
            for x in range(n):
                if z % s == 0 and y % s == 0 and x % s == 0:
                    ev.add((z * n + y) * n + x)
    for cz in range(C):
        for cy in range(C):
            for cx in range(C):
                if mask[cz][cy][cx]:
                    for z in range(cz * s, cz * s + s + 1):
                        for y in range(cy * s, cy * s + s + 1):
                            for x in range(cx * s, cx * s + s + 1):
                                ev.add((z * n + y) * n + x)
    return ev


def band_points(mask, s):
    """the evaluated points that are not on the coarse lattice, ascending"""
    n = BAND_R + 1
    return sorted(i for i in band_evaluated(mask, s)
                  if not ((i % n) % s == 0 and ((i // n) % n) % s == 0 and (i // (n * n)) % s == 0))


def band_fill(field, mask, s):
    """-> the filled grid as exact Fractions (units of 1/4) in flat order; asserts that the clamp to the corners'
    range is a no-op"""
    n, C = BAND_R + 1, BAND_R // s
    ev = band_evaluated(mask, s)
    out = []
    for z in range(n):
        for y in range(n):
            for x in range(n):
                if (z * n + y) * n + x in ev:
                    out.append(Fraction(field[z][y][x]))
                    continue
                c = [min(i // s, C - 1) for i in (z, y, x)]
                t = [Fraction(i - ci * s, s) for i, ci in zip((z, y, x), c)]
                v = [[[field[(c[0] + dz) * s][(c[1] + dy) * s][(c[2] + dx) * s] for dx in (0, 1)] for dy in (0, 1)]
                     for dz in (0, 1)]
                xs = [[(1 - t[2]) * v[dz][dy][0] + t[2] * v[dz][dy][1] for dy in (0, 1)] for dz in (0, 1)]
                ys = [(1 - t[1]) * xs[dz][0] + t[1] * xs[dz][1] for dz in (0, 1)]
                r = (1 - t[0]) * ys[0] + t[0] * ys[1]
                flat = [w for a in v for b in a for w in b]
                assert min(flat) <= r <= max(flat)
                out.append(r)
    return out


def band_pack_field(field):
    return _scaled_f32(field, BAND_VALUE_DEN).reshape(-1)


def band_pack_fill(values):
    den = BAND_VALUE_DEN * 64
    ints = [v * 64 for v in values]
    assert all(v.denominator == 1 for v in ints)
    return _scaled_f32([int(v) for v in ints], den)


# =====================================================================================================================
# 7. mesh_simplify.hip cell assignment.  Per axis: cell = clamp(floor(fl(v - origin) * (1/h)), 0,
# cells - 1), fl = one float32 rounding.  On the box [-1, 1]^3 with 8 cells h = 1/4 and 1/h = 4 are exact, so the only
# rounding is that of v + 1, which is exact for -1 <= v <= -1/2 (Sterbenz): there two vertices either side of a border
# by one ulp separate, and a vertex exactly on a border goes to the upper cell.  Further up one ulp below a border
# may round onto it: the reference models fl() exactly, in integers.
# =====================================================================================================================
SIMPLIFY_CLAUSES = ("border",)
SIMPLIFY_CELLS = 8
SIMPLIFY_BOX = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)


def round_to_f32(q):
    """the float32 nearest the rational q (ties to even, normal range), as an exact Fraction"""
    q = Fraction(q)
    if q == 0:
        return q
    s, a = (1 if q > 0 else -1), abs(q)
    e = 0
    while a * Fraction(2) ** e < 1 << 23:
        e += 1
    while a * Fraction(2) ** e >= 1 << 24:
        e -= 1
    x = a * Fraction(2) ** e
    m = x.numerator // x.denominator
    r = x - m
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and m & 1):
        m += 1
    return s * Fraction(m) * Fraction(2) ** (-e)


def _f32_neighbours(value):
    """-> (the float32 below, value, the float32 above) by stepping the bit pattern"""
    a = np.array([value], np.float32)
    bits = int(a.view(np.uint32)[0])
    out = []
    for step in (-1, 0, 1):
        if value == 0.0 and step:
            b = 1 if step > 0 else 0x80000001
        else:
            b = bits + step if value > 0 else bits - step
        out.append(np.array([b], np.uint32).view(np.float32)[0])
    return out


def simplify_vertices():
    """-> float32 [nv, 3]: on every axis every cell border -1 + k/4 (k = 0..8; k = 8 is the box's maximum face) with
    its two float32 neighbours, and points beyond the box, the other two axes at one of two mid-cell positions"""
    specials = []
    for k in range(SIMPLIFY_CELLS + 1):
        specials += _f32_neighbours(float(Fraction(k - 4, 4)))
    specials += [np.float32(-1.5), np.float32(1.5), np.float32(-1.0625), np.float32(1.0625)]
    rows = []
    for rest in ((float(Fraction(-5, 8)), float(Fraction(3, 8))), (float(Fraction(1, 8)), float(Fraction(-7, 8)))):
        for a in range(3):
            for s in specials:
                p = [rest[0], rest[1]]
                p.insert(a, s)
                rows.append(p)
    return np.asarray(rows, np.float32)


def simplify_cell(v, strict=()):
    """v: one float32 coordinate -> its cell on the lattice of SIMPLIFY_BOX with SIMPLIFY_CELLS cells"""
    x = round_to_f32(Fraction(float(v)) + 1) * 4            # Fraction(float) is exact
    c = -((-x.numerator) // x.denominator) - 1 if "border" in strict else x.numerator // x.denominator
    return min(max(c, 0), SIMPLIFY_CELLS - 1)


def simplify_cells(verts, strict=()):
    return [tuple(simplify_cell(x, strict) for x in p) for p in verts.tolist()]


def simplify_vmap(cells):
    """clusters numbered by their smallest member -> (vmap, first)"""
    ids, vmap, first = {}, [], []
    for i, c in enumerate(cells):
        if c not in ids:
            ids[c] = len(ids)
            first.append(i)
        vmap.append(ids[c])
    return vmap, first


# =====================================================================================================================
# 4. mesh_colour.hip z-buffer and seen test.  The exact lattice camera of tests/resample_lattice.py with
# a third row: [p, 1] . T = (64 px + 68 w, 64 py + 68 w, w), w = 1 + pz, so a fronto-parallel triangle at pz in
# {0, 1, 3} has w in {1, 2, 4}, q = 1/w exact, a zero plane gradient and a zero bias.  A vertex goes to the sub-pixel
# position x = (u + 1/2) S; sub-pixel i covers [i, i+1).  Positions here are given as xs = u + 1/2 (the S = 1
# sub-pixel coordinate) in quarter units: integers 4 * xs.
# =====================================================================================================================
COLOUR_CLAUSES = ("edge", "depth", "floor")
COLOUR_CAMERA = ((64.0, 0.0, 0.0), (0.0, 64.0, 0.0), (68.0, 68.0, 1.0), (68.0, 68.0, 1.0))
COLOUR_IMG = 137


def _floor(q):
    q = Fraction(q)
    return q.numerator // q.denominator


def _upper_cell(q, strict):
    """the sub-pixel of coordinate q: [i, i+1) holds it -- floor; the strict twin (i, i+1] gives ceil - 1"""
    return -_floor(-q) - 1 if "floor" in strict else _floor(q)


def _rect(x0, x1, y0, y1, w):
    return [((x0, y0, w), (x1, y0, w), (x1, y1, w)), ((x0, y0, w), (x1, y1, w), (x0, y1, w))]


def colour_fixture():
    """-> triangles of (4 xs, 4 ys, w) vertices, none shared between triangles"""
    def tri(x, y, leg, w):
        return ((4 * x, 4 * y, w), (4 * (x + leg), 4 * y, w), (4 * x, 4 * (y + leg), w))

    t = [tri(20, 20, 20, 2),            # the queue path: a bounding box of 21 x 21 sub-pixels, edges on sub-pixel lines
         tri(50, 20, 6, 2),             # the thread path: 7 x 7 = 49 sub-pixels
         tri(24, 24, 4, 4),             # behind the first: hidden
         tri(10, 60, 60, 4),            # a large triangle at the back, partly hidden
         tri(0, 100, 6, 2),             # x = 0 is inside the image
         tri(131, 100, 6, 2),           # x = 137 S is outside
         tri(-3, 80, 6, 2),             # x < 0
         tri(100, 131, 6, 1), tri(100, 0, 6, 1)]
    # occluders one layer nearer (w = 1) that only TOUCH the sub-pixel line of a vertex of the triangles above
    t += [tuple((4 * x, 4 * y, 1) for x, y, _ in r) for r in
          (_rect(36, 40, 16, 24, 0) + _rect(14, 19, 36, 44, 0) + _rect(57, 61, 17, 20, 0) + _rect(50, 53, 27, 30, 0))]
    # small triangles at w = 2 and w = 4 with vertices on and off the sub-pixel lines, under and beside occluders
    rng = random.Random(4)
    for k in range(16):
        x, y = 70 + 8 * (k % 4), 20 + 8 * (k // 4)
        off = (0, 1, 2, 3)[k % 4]
        t.append(tuple((4 * x + off + 4 * dx, 4 * y + off + 4 * dy, 2 if k & 1 else 4)
                       for dx, dy in ((0, 0), (rng.randrange(2, 6), 0), (0, rng.randrange(2, 6)))))
        if k % 3 == 0:
            t += [tuple((4 * a, 4 * b, 1) for a, b, _ in r) for r in _rect(x - 2, x, y - 2, y + 3, 0)]
        if k % 3 == 1:
            t += [tuple((4 * a, 4 * b, 1) for a, b, _ in r) for r in _rect(x + 1, x + 3, y - 1, y, 0)]
    for S in (1, 2):                                # the raster paths: more than 64 sub-pixels goes to the queue
        assert colour_box_subpixels(t[0], S) > 64 >= colour_box_subpixels(t[1], 1)
    assert colour_box_subpixels(t[1], 2) > 64      # (at S = 2 the 6-pixel triangle is queued too: 13 x 13)
    assert any(colour_box_subpixels(tr, 2) <= 64 for tr in t)
    for tr in t:
        for x4, y4, w in tr:
            assert w in (1, 2, 4) and _fits((x4 - 274) * w * 64)       # px = (4 xs - 2 - 272) w / 256, exact
    return t


def colour_box_subpixels(tr, S):
    """the sub-pixels of a triangle's bounding box floor(min) .. floor(max) at S samples per pixel (unclipped)"""
    n = 1
    for a in (0, 1):
        c = [Fraction(p[a] * S, 4) for p in tr]
        n *= _floor(max(c)) - _floor(min(c)) + 1
    return n


def colour_pack(tris):
    """-> (verts float32 [3T, 3], faces int32 [T, 3]): px = (u - 68) w / 64 with u = xs - 1/2, pz = w - 1"""
    rows = [((x4 - 274) * w, (y4 - 274) * w, 256 * (w - 1)) for tr in tris for x4, y4, w in tr]
    return _scaled_f32(rows, 256), np.arange(3 * len(tris), dtype=np.int32).reshape(-1, 3)


def colour_zbuffer(tris, S, strict=()):
    """-> {(j, i): q}: the z-buffer of the written rule, exact.  Coverage: the sub-pixels of the bounding box
    floor(min) .. floor(max), clipped to the image, whose three edge functions at the centre, oriented by the sign of
    the area and raised by (|a| + |b|) / 2, are >= 0; the value is the plane of q at the centre clamped to the
    vertices' range, lowered by |gx| + |gy|; the buffer keeps the maximum."""
    N = COLOUR_IMG * S
    zb = {}
    for tr in tris:
        X = [Fraction(x4 * S, 4) for x4, _, _ in tr]
        Y = [Fraction(y4 * S, 4) for _, y4, _ in tr]
        Q = [Fraction(1, w) for _, _, w in tr]
        area = (X[1] - X[0]) * (Y[2] - Y[0]) - (X[2] - X[0]) * (Y[1] - Y[0])
        if area == 0:
            continue
        dq1, dq2 = Q[1] - Q[0], Q[2] - Q[0]
        gx = (dq1 * (Y[2] - Y[0]) - dq2 * (Y[1] - Y[0])) / area
        gy = (dq2 * (X[1] - X[0]) - dq1 * (X[2] - X[0])) / area
        assert gx == 0 and gy == 0                      # fronto-parallel: where bit equality is claimed
        i0, i1 = _floor(min(X)), _upper_cell(max(X), strict)
        j0, j1 = _floor(min(Y)), _upper_cell(max(Y), strict)
        if i1 < 0 or i0 > N - 1 or j1 < 0 or j0 > N - 1:
            continue
        s = 1 if area > 0 else -1
        edges = [(s * (Y[a] - Y[b]), s * (X[b] - X[a]), X[a], Y[a]) for a, b in ((1, 2), (2, 0), (0, 1))]
        for i in range(max(i0, 0), min(i1, N - 1) + 1):
            for j in range(max(j0, 0), min(j1, N - 1) + 1):
                cx, cy = Fraction(2 * i + 1, 2), Fraction(2 * j + 1, 2)
                inside = True
                for a, b, ex, ey in edges:
                    e = a * (cx - ex) + b * (cy - ey) + (abs(a) + abs(b)) / 2
                    inside = inside and (e > 0 if "edge" in strict else e >= 0)
                if not inside:
                    continue
                val = Q[0] + gx * (cx - X[0]) + gy * (cy - Y[0])
                val = min(max(val, min(Q)), max(Q)) - (abs(gx) + abs(gy))
                if val > zb.get((j, i), 0):
                    zb[(j, i)] = val
    return zb


def colour_seen(tris, zb, S, tol, strict=()):
    """-> the class byte of every vertex (1 seen, 0 not; no mirror, no fill): w > 0, the sub-pixel [i, i+1) of x inside
    the image, 1/w >= (1 - tol) zbuf there"""
    N = COLOUR_IMG * S
    out = []
    for tr in tris:
        for x4, y4, w in tr:
            i, j = _upper_cell(Fraction(x4 * S, 4), strict), _upper_cell(Fraction(y4 * S, 4), strict)
            if not (0 <= i <= N - 1 and 0 <= j <= N - 1):
                out.append(0)
                continue
            z, q = zb.get((j, i), 0), Fraction(1, w)
            bound = (1 - Fraction(tol)) * z
            out.append(int(q > bound if "depth" in strict else q >= bound))
    return out


def colour_zbuffer_f32(zb, S):
    N = COLOUR_IMG * S
    out = np.zeros((N, N), np.float32)
    for (j, i), q in zb.items():
        out[j, i] = float(q)                            # 1, 1/2, 1/4: exact
    return out

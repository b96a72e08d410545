"""Per-sheet dual contouring, host side: the loop table of tools/gen_mc_loops.py against an independent derivation, the
specification ``isosurface.dual_contour_sheets_arrays`` checked by properties (equal to ``dual_contour_arrays`` where
every cell has one loop, manifold with marching cubes' components and Euler characteristic on thin plates and close
parts, nothing but the documented limit elsewhere, the counts of a checkerboard, rows that only count in the mean), the
argument checks of the five C entries of include/dc/disn_amd_dc_sheets.h, the header itself, and the drivers' flags and
paths.  No GPU: the device's bits are compared in tests/test_gpu_dual_contour_sheets.py."""
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import abi_table
import dual_contour_fixtures as F
import dual_contour_sheets_fixtures as S
from oracle import mc_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REG = 2.0 ** -10


def iso_mod():
    from disn_amd import isosurface
    return isosurface


def loops_mod():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_mc_loops
    finally:
        sys.path.pop(0)
    return gen_mc_loops


def cases_of(vol, iso=0.0):
    """per cell [R^3] in flat (iz,iy,ix) order: the marching-cubes case, stated on its own"""
    n = round(vol.size ** (1.0 / 3.0))
    R = n - 1
    ins = vol.reshape(n, n, n) < np.float32(iso)
    case = np.zeros((R, R, R), np.int64)
    for i, (dx, dy, dz) in enumerate(O.gen.CORNERS.astype(int)):
        case += ins[dz:dz + R, dy:dy + R, dx:dx + R].astype(np.int64) << i
    return case.reshape(-1)


def tables():
    from disn_amd import mc_loops
    return np.asarray(mc_loops.MC_NLOOP), np.asarray(mc_loops.MC_LOOP)


# ------------------------------------------------------------------ 1. the loop table
def _loops_face_by_face(mask):
    """the loops of a case WITHOUT its triangles: the cut edges paired face by face by the rule of
    gen_mc_tables.case_triangles (two cut edges of a face are joined; on a face with four, the two edges at every
    inside corner), the components of that pairing numbered by their smallest edge"""
    g = O.gen
    inside = [(mask >> i) & 1 for i in range(8)]
    parent = list(range(12))

    def find(a):
        while parent[a] != a:
            a = parent[a]
        return a

    def link(a, b):
        a, b = find(a), find(b)
        parent[max(a, b)] = min(a, b)

    for f in g.FACES:
        es = [g.EDGE_OF[frozenset((f[k], f[(k + 1) % 4]))] for k in range(4)]
        cut = [k for k in range(4) if inside[f[k]] != inside[f[(k + 1) % 4]]]
        assert len(cut) in (0, 2, 4)
        if len(cut) == 2:
            link(es[cut[0]], es[cut[1]])
        elif len(cut) == 4:
            for k in range(4):
                if inside[f[k]]:
                    link(es[(k - 1) % 4], es[k])
    cut_edges = [e for e, (a, b) in enumerate(g.EDGES) if inside[a] != inside[b]]
    roots = sorted({find(e) for e in cut_edges})
    return [roots.index(find(e)) if e in cut_edges else -1 for e in range(12)], len(roots)


def test_the_generated_files_are_the_generators_output():
    gen = loops_mod()
    for path, text in gen.targets():
        assert open(path).read() == text(), path
    nloop, loop = gen.build_loops()
    tn, tl = tables()
    assert np.array_equal(tn, nloop) and np.array_equal(tl, loop)
    header = open(os.path.join(ROOT, "disn_amd", "csrc", "mc_loops.h")).read()
    assert "kMcNloop[256]" in header and "signed char kMcLoop[256][12]" in header


def test_the_loop_table_is_the_face_by_face_pairing():
    nloop, loop = tables()
    assert nloop.shape == (256,) and loop.shape == (256, 12)
    assert np.bincount(nloop).tolist() == [2, 162, 82, 8, 2]
    sizes = np.bincount([int((loop[m] == k).sum()) for m in range(256) for k in range(nloop[m])])
    assert {i: int(c) for i, c in enumerate(sizes) if c} == {3: 144, 4: 66, 5: 72, 6: 52, 7: 24}
    for m in range(256):
        want, n = _loops_face_by_face(m)
        assert n == nloop[m] and want == loop[m].tolist(), m
        for e, (a, b) in enumerate(O.gen.EDGES):            # a loop id if and only if the edge's ends differ
            assert (loop[m, e] >= 0) == (((m >> a) & 1) != ((m >> b) & 1)), (m, e)
        ids = sorted(set(loop[m][loop[m] >= 0].tolist()))
        assert ids == list(range(nloop[m]))
        first = [int(np.nonzero(loop[m] == k)[0][0]) for k in ids]
        assert first == sorted(first)                        # numbered by their smallest cube-edge id


def test_the_quad_edge_table():
    from disn_amd import mc_loops
    m = iso_mod()
    assert m.DCS_QUAD_EDGES == mc_loops.MC_QUAD_EDGE == tuple(tuple(r) for r in loops_mod().quad_edges())
    assert "kMcQuadEdge[3][4] = {%s};" % ",".join("{%s}" % ",".join(map(str, r)) for r in m.DCS_QUAD_EDGES) in open(
        os.path.join(ROOT, "disn_amd", "csrc", "mc_loops.h")).read()
    # stated on its own: cell q_k at offset (du, dv) sees the grid edge as the cube edge whose two end corners are the
    # grid edge's ends, in the cell's own corner coordinates
    corners = [tuple(int(v) for v in c) for c in O.gen.CORNERS]
    for a in range(3):
        u, v = (a + 1) % 3, (a + 2) % 3
        for k, (du, dv) in enumerate(((-1, -1), (0, -1), (0, 0), (-1, 0))):
            lo, hi = [0, 0, 0], [0, 0, 0]
            lo[u] = hi[u] = -du
            lo[v] = hi[v] = -dv
            hi[a] = 1
            e = O.gen.EDGE_OF[frozenset((corners.index(tuple(lo)), corners.index(tuple(hi))))]
            assert m.DCS_QUAD_EDGES[a][k] == e, (a, k)


# ------------------------------------------------------------------ 2. one-loop grids
@pytest.mark.parametrize("fixture", [F.sphere(9, F.SKEW), F.cube(8), F.plane(6)], ids=["sphere9", "cube8", "plane6"])
def test_a_grid_of_one_loop_cells_is_dual_contouring_bit_for_bit(fixture):
    vol, box, iso, nat = fixture
    assert tables()[0][cases_of(vol, iso)].max() == 1          # no cell has two loops
    pts = iso_mod().hermite_points_arrays(vol, box, iso)
    nrm = nat(pts)
    v, f = iso_mod().dual_contour_arrays(vol, box, iso, nrm, REG)
    sv, sf = iso_mod().dual_contour_sheets_arrays(vol, box, iso, nrm, REG)
    assert len(v) > 50 and len(f) > 100
    assert sv.dtype == np.float32 and sf.dtype == np.int32 and sv.shape == v.shape and sf.shape == f.shape
    assert np.array_equal(F.bits(sv), F.bits(v)) and np.array_equal(sf, f)


# ------------------------------------------------------------------ 3. manifold where dual contouring welds
THIN = {"disc0.03": (lambda: S.disc(0.03), 17, 34), "disc0.05": (lambda: S.disc(0.05), 15, 30),
        "disc0.06": (lambda: S.disc(0.06), 8, 16), "two_spheres": (lambda: S.two_spheres(0.05), 2, 4)}


@pytest.mark.parametrize("name", sorted(THIN))
def test_thin_parts_stay_manifold_and_apart(name):
    make, comps, euler = THIN[name]
    fx = make()
    vol, box, iso, _ = fx
    assert vol.dtype == np.float32 and vol.size == 13 ** 3 and iso == 0.0
    mv, mf = O.marching_cubes(vol.reshape(13, 13, 13), box, iso)
    mc = S.topology(mv, mf)
    _, _, v, f = S.mesh(fx)
    t = S.topology(v, f)
    _, _, dv, df = F.mesh(fx)
    dc = S.topology(dv, df)
    print(name, "mc", mc, "per sheet", t, "per cell", dc)
    assert t["over"] == 0                                     # every undirected edge has at most 2 faces
    assert t["directed"] == 1                                 # no directed edge occurs twice
    assert t["repeats"] == 0                                  # no face repeats an index
    assert (t["components"], t["euler"]) == (mc["components"], mc["euler"])
    assert (mc["components"], mc["euler"]) == (comps, euler)  # the figures of the prototype
    assert dc["over"] >= 1 and dc["components"] < t["components"]
    assert int(f.min()) == 0 and int(f.max()) == len(v) - 1 and len(f) == len(df)


# ------------------------------------------------------------------ 4. the limit that remains
def _limit_edges(fx):
    """-> (edges with more than 2 faces, how many of them are the documented kind, multi-loop cells, those of them with
    no vertex on such an edge)"""
    vol, box, iso, _ = fx
    n = round(vol.size ** (1.0 / 3.0))
    R = n - 1
    nloop, loop = tables()
    case = cases_of(vol)
    base = np.cumsum(nloop[case]) - nloop[case]
    _, _, v, f = S.mesh(fx)
    und, count, _ = S.edge_counts(f, len(v))
    over = und[count > 2]
    edges = [tuple(e) for e in O.gen.edge_geometry()]
    documented, touched = 0, set()
    for a, b in over:
        # the cell of a vertex: the one whose ids base .. base + loops - 1 hold it
        ca = int(np.nonzero((base <= a) & (base + nloop[case] > a))[0][0])
        cb = int(np.nonzero((base <= b) & (base + nloop[case] > b))[0][0])
        touched.update((ca, cb))
        la, lb = int(a - base[ca]), int(b - base[cb])
        pa = np.array([ca % R, (ca // R) % R, ca // (R * R)])
        pb = np.array([cb % R, (cb // R) % R, cb // (R * R)])
        d = pb - pa
        if np.abs(d).sum() != 1:
            continue                                          # not two face neighbours
        k = int(np.nonzero(d)[0][0])
        if d[k] < 0:
            ca, cb, la, lb = cb, ca, lb, la                   # ca is the lower cell: the face is its upper face on axis k
        fa = [e for e, g in enumerate(edges) if g[3] != k and g[k] == 1]
        fb = [e for e, g in enumerate(edges) if g[3] != k and g[k] == 0]
        assert len(fa) == 4 and len(fb) == 4
        # all four edges of the shared face cut (ambiguous) and, in both cells, on the one loop whose vertex this is
        if (loop[case[ca]][fa] == la).all() and (loop[case[cb]][fb] == lb).all():
            documented += 1
    multi = np.nonzero(nloop[case] > 1)[0]
    return len(over), documented, len(multi), len(set(multi.tolist()) - touched)


def test_every_edge_with_more_than_two_faces_is_the_documented_limit():
    grids = {"noise8 seed %d" % s: F.noise(8, seed=s) for s in (7, 8, 9)}
    grids["disc0.08"] = S.disc(0.08)
    some, spared = 0, 0
    for name, fx in grids.items():
        over, documented, multi, clear = _limit_edges(fx)
        print("%s: %d edges with more than 2 faces, %d of the documented kind; %d multi-loop cells, %d of them on none"
              % (name, over, documented, multi, clear))
        assert documented == over, name                       # the documented limit and nothing else
        some += over > 0
        spared += clear > 0
    # not vacuous: a grid has such an edge, and a grid has a multi-loop cell that lies on none
    assert some >= 1 and spared >= 1


# ------------------------------------------------------------------ 5. the checkerboard
@pytest.mark.parametrize("R,want", [(1, (12, 4, 0)), (2, (54, 32, 12))])
def test_checker_counts(R, want):
    fx = S.checker(R)
    assert (tables()[0][cases_of(fx[0])] == 4).all()          # every cell has four loops
    pts, _, v, f = S.mesh(fx)
    assert (len(pts), len(v), len(f)) == want == (3 * R * (R + 1) ** 2, 4 * R ** 3, 6 * R * (R - 1) ** 2)
    if len(f):
        assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 0] != f[:, 2]).all()
        assert 0 <= f.min() and f.max() < len(v)


# ------------------------------------------------------------------ 6. rows that only count in the mean, per loop
def test_a_row_without_a_usable_normal_changes_nothing_but_its_loops_mean():
    m = iso_mod()
    vol, box, iso, nat = F.noise(5)
    pts = m.hermite_points_arrays(vol, box, iso)
    nrm = nat(pts)
    bad = ~np.isfinite(nrm).all(1) | (nrm == 0).all(1)
    assert np.isnan(nrm).any() and np.isinf(nrm).any() and (nrm == 0).all(1).any() and 0 < bad.sum() < len(nrm) // 2
    v, f = m.dual_contour_sheets_arrays(vol, box, iso, nrm, REG)
    for fill in (np.nan, np.inf, 0.0):                        # one kind: the same bits whichever stands in a bad row
        other = nrm.copy()
        other[bad] = fill
        v2, f2 = m.dual_contour_sheets_arrays(vol, box, iso, other, REG)
        assert np.array_equal(F.bits(v), F.bits(v2)) and np.array_equal(f, f2), fill
    # per (cell, loop), an independent statement: numpy.linalg on the loop's usable rows, the mean over the loop's rows
    nloop, loop = tables()
    case = cases_of(vol)
    assert (nloop[case] > 1).sum() >= 10
    E = m._DcEdges(vol, box, iso)
    n, R = E.n, E.R
    k, checked, bad_in_multi = 0, 0, 0
    for c in range(R ** 3):
        cx, cy, cz = c % R, (c // R) % R, c // (R * R)
        corner = np.array([E.ax[0][cx], E.ax[1][cy], E.ax[2][cz]], np.float64)
        hi = np.array([E.ax[0][cx + 1], E.ax[1][cy + 1], E.ax[2][cz + 1]], np.float64) - corner
        for l in range(nloop[case[c]]):
            rows = [int(E.eidx[3 * (((cz + dz) * n + cy + dy) * n + cx + dx) + a])
                    for e, (dx, dy, dz, a) in enumerate(m.DC_CUBE_EDGES) if loop[case[c]][e] == l]
            assert 3 <= len(rows) <= 7
            d = pts[rows].astype(np.float64) - corner
            g = nrm[rows].astype(np.float64)
            with np.errstate(all="ignore"):
                s = (g * g).sum(1)
            good = np.isfinite(s) & (s > 0)
            bad_in_multi += int(nloop[case[c]] > 1 and not good.all())
            gh = g[good] / np.sqrt(s[good])[:, None]
            A = gh.T @ gh
            b = -(gh * (gh * d[good]).sum(1)[:, None]).sum(0)
            mean = d.mean(0)
            lam = REG * np.trace(A) / 3 + 2.0 ** -40
            x = np.linalg.solve(A + lam * np.eye(3), lam * mean - b)
            got = v[k].astype(np.float64)
            if (x > 1e-4).all() and (x < hi - 1e-4).all():
                assert np.abs(corner + x - got).max() <= 1e-5, (c, l)
                checked += 1
            assert (got >= corner - 1e-6).all() and (got <= corner + hi + 1e-6).all()       # clipped to the cell
            k += 1
    assert k == len(v) and checked >= 10 and bad_in_multi >= 3
    # a grid whose rows all lack a normal: every vertex at its LOOP's mean
    v0, _ = m.dual_contour_sheets_arrays(vol, box, iso, np.zeros_like(pts), REG)
    k = 0
    for c in range(R ** 3):
        cx, cy, cz = c % R, (c // R) % R, c // (R * R)
        corner = np.array([E.ax[0][cx], E.ax[1][cy], E.ax[2][cz]], np.float64)
        for l in range(nloop[case[c]]):
            rows = [int(E.eidx[3 * (((cz + dz) * n + cy + dy) * n + cx + dx) + a])
                    for e, (dx, dy, dz, a) in enumerate(m.DC_CUBE_EDGES) if loop[case[c]][e] == l]
            assert np.abs(pts[rows].astype(np.float64).mean(0) - v0[k]).max() <= 1e-6
            k += 1


def test_degenerate_grids_and_arguments():
    m = iso_mod()
    for R in (1, 3):
        for value in (1.0, -1.0):
            vol = np.full((R + 1) ** 3, value, np.float32)
            v, f = m.dual_contour_sheets_arrays(vol, F.UNIT, 0.0, np.zeros((0, 3), np.float32))
            assert v.shape == (0, 3) and f.shape == (0, 3) and v.dtype == np.float32 and f.dtype == np.int32
    vol = np.array([-1, 1, 1, 1, 1, 1, 1, 1], np.float32)
    with pytest.raises(ValueError):
        m.dual_contour_sheets_arrays(vol, F.UNIT, 0.0, np.zeros((3, 3), np.float32), reg=0.0)
    with pytest.raises(ValueError):
        m.dual_contour_sheets_arrays(vol, F.UNIT, 0.0, np.zeros((2, 3), np.float32))


# ------------------------------------------------------------------ 7. argument checks, header, flags
ENTRIES = ("disn_dcs_count_batch", "disn_dcs_points_batch", "disn_dcs_grid_normals_batch", "disn_dcs_emit_batch")
NEW = ("disn_dcs_workspace_bytes",) + ENTRIES


def _parse_header():
    path = os.path.join(ROOT, "include", "dc", "disn_amd_dc_sheets.h")
    text = abi_table.strip_comments(open(path).read())
    text = "\n".join(l for l in text.split("\n") if not l.lstrip().startswith("#"))
    out = []
    for ret, name, params in re.findall(r"([\w\s\*]+?)\b(disn_\w+)\s*\(([^)]*)\)\s*;", text):
        out.append(abi_table.Proto(" ".join(ret.split()), name, [abi_table.parse_param(p) for p in params.split(",")],
                                   "dc/disn_amd_dc_sheets.h"))
    return out


def _case(name, h, box):
    """the smallest legal call as {parameter: value}, in the prototype's order; device pointers are abi_table.FAKE"""
    need = h.disn_dcs_workspace_bytes(1, 4)
    fake = abi_table.FAKE
    a = {"sdf": fake}
    if name != "disn_dcs_count_batch":
        a["sdf_params_host"] = box.ctypes.data
    a.update(B=1, R=4, iso=0.0)
    if name == "disn_dcs_count_batch":
        a["counts"] = fake
    elif name == "disn_dcs_points_batch":
        a["points"] = fake
    elif name == "disn_dcs_grid_normals_batch":
        a["normals"] = fake
    else:
        a.update(points=fake, normals=fake, reg=REG, verts=fake, faces=fake)
    a.update(ws=fake, ws_bytes=need, stream=None)
    return a


@pytest.mark.parametrize("name", ENTRIES)
def test_every_entry_refuses_bad_arguments_on_the_host(name):
    """the table of test_dual_contour_host.py for the disn_dcs_* entries, and the limit 4 B R^3 < 2^32: every refused
    call returns its negative code; the device pointers are never mapped and there may be no device at all"""
    from disn_amd import _lib
    h = _lib.lib()
    box = np.array([-1, -1, -1, 1, 1, 1], np.float64)
    fn = getattr(h, name)
    base = _case(name, h, box)
    protos = [p for p in _parse_header() if p.name == name]
    assert [pn for _, pn in protos[0].params] == list(base)
    dc = [p for p in abi_table.strip_comments(open(os.path.join(ROOT, "include", "dc", "disn_amd_dc.h")).read()).split(";")
          if name.replace("disn_dcs_", "disn_dc_") + "(" in p]
    mine = [p for p in abi_table.strip_comments(open(os.path.join(ROOT, "include", "dc", "disn_amd_dc_sheets.h")).read()
                                                ).split(";") if name + "(" in p]
    assert len(dc) == 1 and len(mine) == 1                    # the argument list of its disn_dc_* twin
    assert "".join(dc[0].split()).replace("disn_dc_", "disn_dcs_") == "".join(mine[0].split())

    def call(**kw):
        return fn(*dict(base, **kw).values())

    pointers = [k for k in base if k not in ("B", "R", "iso", "reg", "ws_bytes", "stream")]
    assert len(pointers) >= 3
    for p in pointers:
        assert call(**{p: None}) == abi_table.E_ARG, p
    for size in ("B", "R"):
        for bad in (0, -1):
            assert call(**{size: bad}) == abi_table.E_ARG, (size, bad)
    if "reg" in base:
        for bad in (0.0, 1.5, float("nan"), -REG, float("inf")):
            assert call(reg=bad) == abi_table.E_ARG, bad
        assert call(reg=1.0, ws_bytes=base["ws_bytes"] - 1) == abi_table.E_WS       # 1 itself is legal
    assert call(ws_bytes=base["ws_bytes"] - 1) == abi_table.E_WS
    assert call(ws_bytes=0) == abi_table.E_WS
    assert call(R=1291, ws_bytes=1 << 62) == abi_table.E_SHAPE
    assert call(R=1290, B=2, ws_bytes=1 << 62) == abi_table.E_SHAPE
    assert call(B=abi_table.INT_MAX, R=4, ws_bytes=1 << 62) == abi_table.E_SHAPE    # refused before a box is read
    # 4 B R^3 < 2^32: R = 1024 is 2^32 exactly, which the edge slots alone (3 * 1025^3) would still allow
    assert call(R=1024, ws_bytes=1 << 62) == abi_table.E_SHAPE
    assert call(R=1023, ws_bytes=0) == abi_table.E_WS
    assert call(R=512, B=8, ws_bytes=1 << 62) == abi_table.E_SHAPE
    assert call(R=512, B=7, ws_bytes=0) == abi_table.E_WS


def test_the_workspace_query_is_zero_beyond_the_limits():
    from disn_amd import _lib
    h = _lib.lib()
    q, dc = h.disn_dcs_workspace_bytes, h.disn_dc_workspace_bytes
    for B, R in ((0, 4), (-1, 4), (1, 0), (1, -1), (0, 0), (1, 1291), (2, 1290), (abi_table.INT_MAX, 4),
                 (1, abi_table.INT_MAX), (abi_table.INT_MAX, abi_table.INT_MAX)):
        assert q(B, R) == 0, (B, R)
    for B, R in ((1, 1), (1, 4), (2, 4), (1, 9), (1, 1000), (1, 1023), (7, 512), (3, 700), (43690, 9)):
        assert q(B, R) == dc(B, R) > 0, (B, R)                # the same workspace inside both limits
    for B, R in ((1, 1024), (1, 1125), (8, 512), (2, 813), (43690, 31)):
        assert 4 * B * R ** 3 >= 1 << 32 and 3 * B * (R + 1) ** 3 < 1 << 32
        assert q(B, R) == 0 and dc(B, R) > 0, (B, R)          # the loop ranks are what refuses
    for B, R in ((1, 1023), (2, 812), (7, 512)):
        assert 4 * B * R ** 3 < 1 << 32 and q(B, R) > 0, (B, R)


def test_the_header_declares_exactly_the_seventh_table():
    from disn_amd import _lib
    protos = {p.name: p for p in _parse_header()}
    assert set(protos) == set(_lib.SIGNATURES_DCS) == set(NEW)
    for name, p in protos.items():
        res, args = _lib.SIGNATURES_DCS[name]
        assert abi_table.c_class(p.ret) == abi_table.binding_class(res), name
        assert len(p.params) == len(args), name
        for (ctype, pname), a in zip(p.params, args):
            assert abi_table.c_class(ctype) == abi_table.binding_class(a), (name, pname)
        twin = _lib.SIGNATURES_DC[name.replace("disn_dcs_", "disn_dc_")]
        assert (res, args) == twin, name
    for t in abi_table.binding_tables() + (_lib.SIGNATURES_DC,):
        assert not set(t) & set(_lib.SIGNATURES_DCS)
    assert len(glob.glob(os.path.join(ROOT, "include", "*.h"))) == 5            # the five headers stay five
    assert sorted(os.listdir(os.path.join(ROOT, "include", "dc"))) == ["disn_amd_dc.h", "disn_amd_dc_sheets.h"]
    assert _lib.ABI_VERSION == 10
    h = _lib.lib()
    for name in NEW:
        assert getattr(h, name).argtypes == _lib.SIGNATURES_DCS[name][1]          # lib() binds the seventh table too


def test_the_header_compiles_as_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "dc/disn_amd_dc_sheets.h"\n'
                   "int main(void) {\n"
                   "  size_t (*ws)(int, int) = disn_dcs_workspace_bytes;\n"
                   "  int (*count)(const float*, int, int, float, uint64_t*, void*, size_t, void*) = disn_dcs_count_batch;\n"
                   "  int (*points)(const float*, const double*, int, int, float, float*, void*, size_t, void*)\n"
                   "      = disn_dcs_points_batch;\n"
                   "  int (*emit)(const float*, const double*, int, int, float, const float*, const float*, double, float*,\n"
                   "              int32_t*, void*, size_t, void*) = disn_dcs_emit_batch;\n"
                   "  int (*cell)(const float*, const double*, int, int, float, const float*, const float*, double, float*,\n"
                   "              int32_t*, void*, size_t, void*) = disn_dc_emit_batch;      /* the sixth header comes along */\n"
                   "  return ws == 0 || count == 0 || points == 0 || emit == 0 || cell == 0 || DISN_ABI_VERSION != 10;\n"
                   "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I",
                        os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_build_lists_the_source_without_contraction_and_the_headers():
    from disn_amd.csrc import build
    csrc = os.path.join(ROOT, "disn_amd", "csrc")
    assert build.SOURCES["dual_contour.hip"] == ["-ffp-contract=off"] == build.SOURCES["marching_cubes.hip"]
    for gone in ("dual_contour_sheets.hip", "dual_contour_common.hpp"):
        assert gone not in build.SOURCES and gone not in build.HEADERS and not os.path.exists(os.path.join(csrc, gone))
    for hdr in ("disn_amd_dc.h", "disn_amd_dc_sheets.h"):
        assert any(h.endswith(os.path.join("include", "dc", hdr)) for h in build.HEADERS)
    assert "grid_mesh.hpp" in build.HEADERS and "mc_loops.h" in build.HEADERS
    # the bodies the meshers share have ONE definition over all of csrc (comments stripped): the axis value, the case of
    # a cell from its eight corners, the edge-point kernel, the grid-normals kernel, the quadric, the quad's split and the
    # 32-box kernel-argument struct
    files = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.hpp")))
    text = {os.path.basename(f): abi_table.strip_comments(open(f).read()) for f in files}
    once = {r"\bfloat\s+grid_coord\s*\(": "grid_mesh.hpp",
            r"\bint\s+grid_cell_case\s*\(": "grid_mesh.hpp",
            r"\?\s*128u?\s*:\s*0u?\s*;": "grid_mesh.hpp",                  # the bit of the eighth corner
            r"\bvoid\s+grid_points_batch_kernel\s*\(": "grid_mesh.hpp",
            r"\bvoid\s+dc_grid_normals_batch_kernel\s*\(": "dual_contour.hip",
            r"\bstruct\s+DcQuadric\b": "dual_contour.hip",
            r"\bvoid\s+dc_quad_faces\s*\(": "dual_contour.hip",
            r"\bstruct\s+\w+\s*\{\s*\w+\s+\w+\[kMcBatchBoxes\]\s*;\s*\}": "grid_mesh.hpp"}
    for pattern, home in once.items():
        assert [name for name, t in text.items() for _ in re.findall(pattern, t)] == [home], pattern
    for old in ("mc_verts_batch_kernel", "dc_points_batch_kernel", "mc_edge_vertex", "dc_edge(", "McBoxes", "DcBoxes"):
        assert not [name for name, t in text.items() if old in t], old
    assert "atomic" not in text["dual_contour.hip"].lower()
    users = sorted(name for name, t in text.items() if name.endswith(".hip") and '#include "grid_mesh.hpp"' in t)
    assert users == ["dual_contour.hip", "marching_cubes.hip"]
    for rule in ("<DcPerCell>", "<DcPerSheet>"):                                  # both families in the one unit
        assert rule in text["dual_contour.hip"]


def test_flags_and_paths():
    from disn_amd import create_sdf, demo
    base = ["--test_lst_dir", "lists"]
    a = create_sdf.parser().parse_args(base + ["--mesher", "dcs"])
    assert create_sdf.dc_from_flags(a) == {"normals": "network", "reg": REG, "sheets": True}
    a = create_sdf.parser().parse_args(base + ["--mesher", "dcs", "--dc_normals", "grid", "--dc_reg", "0.25"])
    assert create_sdf.dc_from_flags(a) == {"normals": "grid", "reg": 0.25, "sheets": True}
    d = demo.parser().parse_args(["--img", "x.png", "--mesher", "dcs", "--dc_reg", "0.5"])
    assert create_sdf.dc_from_flags(d) == {"normals": "network", "reg": 0.5, "sheets": True}
    # dc and mc are what they were
    assert create_sdf.dc_from_flags(create_sdf.parser().parse_args(base + ["--mesher", "dc"])) == {
        "normals": "network", "reg": REG}
    assert create_sdf.dc_from_flags(create_sdf.parser().parse_args(base)) is None
    for bad in (["--dc_reg", "0.5"], ["--dc_normals", "grid"], ["--mesher", "mc", "--dc_reg", "0.5"],
                ["--mesher", "dcs", "--dc_reg", "0"], ["--mesher", "dcs", "--dc_reg", "1.5"],
                ["--mesher", "dcs", "--dc_reg", "nan"]):
        with pytest.raises(ValueError):
            create_sdf.dc_from_flags(create_sdf.parser().parse_args(base + bad))
    with pytest.raises(SystemExit):
        create_sdf.parser().parse_args(base + ["--mesher", "tetra"])
    with pytest.raises(ValueError):
        create_sdf.dc_args("tetra")
    # a checked dict may be handed on with its own mesher, not with another
    checked = create_sdf.dc_args("dcs", 0.25)
    assert checked == {"normals": "network", "reg": 0.25, "sheets": True} == create_sdf.dc_args("dcs", checked)
    with pytest.raises(ValueError):
        create_sdf.dc_args("dc", checked)
    with pytest.raises(ValueError):
        create_sdf.dc_args("dcs", {"sheets": False})
    with pytest.raises(ValueError):
        create_sdf.dc_args("dcs", {"loops": 1})
    # the paths: _dcs in the position _dc takes
    old = create_sdf.result_obj_path("log", 64, 0.0)
    assert create_sdf.result_obj_path("log", 64, 0.0, mesher="dcs") == old + "_dcs"
    assert create_sdf.result_obj_path("log", 64, 0.0, mesher="dc") == old + "_dc"
    full = dict(cam_est=True, fuse=(3, "max"), clean=True, simplify=32, colour=True, smooth=4)
    assert create_sdf.result_obj_path("log", 64, 0.003, mesher="dcs", **full) == os.path.join(
        "log", "test_objs", "camest_fuse3max_65_0.003_dcs_comb_t4_s32_col")

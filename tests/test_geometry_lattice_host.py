"""What the exact dyadic lattices of tests/geometry_lattice.py reach, asserted on the CPU: for every geometry module
(a) the committed float32 restatement equals the integer / Fraction statement of the written rule on the fixture, with
no tolerance, and (b) a strict mutant of the integer rule -- one named closed comparison swapped for its open twin --
moves at least MIN_ITEMS items per clause (a quarter of the occupied cells for the voxeliser).  The kernels of
tests/test_gpu_geometry_lattice.py are only as well tested at equality as these counts are large; none may be relaxed
to make a fixture smaller.  Every test prints its counts."""
from fractions import Fraction

import numpy as np
import pytest

import geometry_lattice as L
import grid_band_reference as BR
import mesh_sdf_reference as SR
import render_reference as RR
import voxel_reference as VR
from disn_amd import postprocess
from oracle import mc_oracle as MO

MIN_ITEMS = 32
F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. voxel.hip ---------------------------------------------------------------------------------------------------
VOXEL_TIE_GROUPS = ("in a face plane", "point on a corner", "segment on an edge", "degenerate on a face", "queue",
                    "multi-chunk")


@pytest.mark.parametrize("dim", [16, 32])
def test_voxel_restatement_equals_the_integer_rule_and_ties_decide(dim):
    fx = L.voxel_fixture(dim)
    assert L.voxel_key_range(dim) == VR.key_range(dim)
    cells, overflow = L.voxel_surface(fx["tris"], dim)
    ref, ref_overflow = VR.surface_voxels(fx["verts"], fx["faces"], dim)
    assert not overflow and not ref_overflow
    assert np.array_equal(L.voxel_dense(cells, dim), ref)
    moved = {}
    for clause in L.VOXEL_CLAUSES:
        moved[clause] = len(cells ^ L.voxel_surface(fx["tris"], dim, strict=(clause,))[0])
    open_cells = L.voxel_surface(fx["tris"], dim, strict=L.VOXEL_CLAUSES)[0]
    share = len(cells - open_cells) / len(cells)
    print("voxel dim %d: %d triangles, %d occupied cells; strict mutants move %s; 'touching does not count' keeps %d "
          "(%.0f %% of the cells are decided by a tie)" % (dim, len(fx["tris"]), len(cells), moved, len(open_cells),
                                                           100 * share))
    assert open_cells <= cells and share >= 0.25
    assert all(n >= MIN_ITEMS for n in moved.values())
    # every tie group on its own: the queue and multi-chunk triangles and the degenerate faces carry ties themselves
    for name in VOXEL_TIE_GROUPS:
        own = L.voxel_surface(fx["groups"][name], dim)[0]
        kept = L.voxel_surface(fx["groups"][name], dim, strict=L.VOXEL_CLAUSES)[0]
        print("  %-22s %4d cells, %4d decided by a tie" % (name, len(own), len(own - kept)))
        assert len(own - kept) >= MIN_ITEMS
    for name in ("point on a corner", "segment on an edge", "degenerate on a face"):
        assert not L.voxel_surface(fx["groups"][name], dim, strict=L.VOXEL_CLAUSES)[0]    # nothing but ties


def test_voxel_sentinel_triangle_overflows_in_both_statements():
    for dim in (16, 32):
        tri, verts, faces = L.voxel_sentinel_triangle(dim)
        cells, overflow = L.voxel_surface([tri], dim)
        assert overflow and len(cells) >= 1
        assert VR.surface_voxels(verts, faces, dim)[1]
        assert not L.voxel_surface([tri], dim, strict=("box",))[0]     # the open twin sees nothing in the key range


# ---- 2. mesh_sdf.hip ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[8, 16])
def sdf_world(request):
    """res -> per fixture the exact d^2, the rule's sign and the mutants' signs; computed once, never modified"""
    res = request.param
    nodes = L.sdf_nodes(res)
    out = {}
    for name, f in L.sdf_fixtures(res).items():
        d2 = L.sdf_d2(nodes, f["tris"])
        out[name] = {"fx": f, "d2": d2, "sign": L.sdf_sign(res, f["tris"], d2, L.SDF_NODE ** 2, 3),
                     "mutants": {c: L.sdf_sign(res, f["tris"], d2, L.SDF_NODE ** 2, 3, strict=(c,))
                                 for c in L.SDF_CLAUSES}}
    return res, nodes, out


def test_sdf_restatement_equals_the_rational_rule(sdf_world):
    res, nodes, world = sdf_world
    axes = [np.linspace(-1.0, 1.0, res + 1).astype(F32)] * 3
    pts = L.sdf_world(nodes, res)
    assert np.array_equal(pts, SR.grid_points(axes))
    n, den = res + 1, 2 * res
    tau = F32(2.0 / res)
    moved = dict.fromkeys(L.SDF_CLAUSES, 0)
    for name, w in world.items():
        verts, faces = L.sdf_mesh_arrays(w["fx"]["tris"], res)
        u = SR.udf(pts, verts, faces)
        on = np.array([d == 0 for d in w["d2"]])
        assert (u[on] == 0).all()
        assert np.abs(u.astype(np.float64) - np.array([float(d) for d in w["d2"]]) ** 0.5 / den).max() <= 1e-6
        differ = "sign pass only"
        if name in L.SDF_AXIS_ALIGNED:               # the bit comparison, and its cap, on every fixture it is made on
            exact = np.array([float(L.sqrt_to_f32(d / den ** 2)) for d in w["d2"]], F32)
            same = _bits(u) == _bits(exact)
            assert 1 - same.mean() <= 0.02
            differ = "%d udf bits differ from the rational" % int((~same).sum())
        bits = SR.crossing_bits(axes, u.reshape(n, n, n), tau, verts, faces)
        want = SR.flood(u.reshape(n, n, n), bits, tau, 3).reshape(-1)
        assert np.array_equal(want, np.array(w["sign"])), name
        here = {c: sum(a != b for a, b in zip(w["sign"], m)) for c, m in w["mutants"].items()}
        for c in here:
            moved[c] += here[c]
        print("sdf res %d %-26s %d nodes, %d on the surface, %s, inside %d, mutants move %s"
              % (res, name, len(nodes), int(on.sum()), differ, len(nodes) - sum(w["sign"]), here))
    print("sdf res %d: mutants move %s nodes over the fixtures" % (res, moved))
    assert all(v >= MIN_ITEMS for v in moved.values())


def test_sdf_sign_ground_truth(sdf_world):
    res, nodes, world = sdf_world
    for name in ("box", "thin box", "box off the nodes"):
        f = world[name]["fx"]
        outside = [not all(f["lo"][a] <= p[a] <= f["hi"][a] for a in range(3)) for p in nodes]
        assert outside == world[name]["sign"]                      # every node, the surface nodes included
        assert sum(1 for d in world[name]["d2"] if d == 0) >= MIN_ITEMS
    # the octahedra: inside exactly where |x| + |y| + |z| <= r about the centre (closed)
    c = L.SDF_NODE * (res // 2)
    for name, cz in (("octahedron off the nodes", c + 2), ("octahedron on the nodes", c)):
        outside = [abs(p[0] - c) + abs(p[1] - c) + abs(p[2] - cz) > 2 * L.SDF_NODE for p in nodes]
        assert outside == world[name]["sign"], name
    # the sheet: an open surface has no inside.  Every node off the sheet is outside; on it, grid edges that end on the
    # sheet are crossed, but the grid edges lying IN its plane are not (area 0: ignored), so the rim leaks inward one
    # ring per band step: after 3 steps the nodes more than 3 rings from the rim remain inside
    s0, s1, z = world["sheet"]["fx"]["sheet"]
    for p, o in zip(nodes, world["sheet"]["sign"]):
        on = p[2] == z and s0 <= p[0] <= s1 and s0 <= p[1] <= s1
        ring = min(p[0] - s0, s1 - p[0], p[1] - s0, s1 - p[1]) // L.SDF_NODE if on else -1
        assert o == (not on or ring < 3), p


# ---- 3. render.hip --------------------------------------------------------------------------------------------------
def test_render_restatement_equals_the_integer_classification():
    moved = dict.fromkeys(L.RENDER_CLAUSES, 0)
    n = L.RENDER_SIZE
    for kind in L.RENDER_SCENES:
        cam, d0 = L.render_camera(kind)
        cam = np.asarray(cam, F32)
        tris = L.render_scene(kind)
        verts, faces = L.render_pack(tris)
        for S in (1, 2):
            exp = L.render_expected(tris, S, d0=d0)
            rgba, depth, face = RR.render(verts, faces, cam, n, n, S)
            ok = np.array([e[3] for e in exp]).reshape(n, n)
            want_f = np.array([e[0] for e in exp]).reshape(n, n)
            want_d = np.array([float(e[1]) if e[1] is not None else 0.0 for e in exp], F32).reshape(n, n)
            want_a = np.array([(2 * 255 * e[2] + S * S) // (2 * S * S) for e in exp]).reshape(n, n)
            assert np.array_equal(face[0][ok], want_f[ok]) and np.array_equal(_bits(depth[0])[ok], _bits(want_d)[ok])
            assert np.array_equal(rgba[0, ..., 3][ok], want_a[ok])
            assert set(np.unique(want_d[ok])) <= {0.0, 4.0, 8.0, 12.0}
            assert kind == "axis" or (want_f != L.render_edge_on_face()).all()            # det == 0: never seen
            here = {}
            for c in L.RENDER_CLAUSES:
                mut = L.render_expected(tris, S, strict=(c,), d0=d0)
                here[c] = sum(1 for a, b in zip(exp, mut) if a[3] and a[:3] != b[:3])
                moved[c] += here[c]
            print("render %-11s S=%d: %d pixels, %d asserted, %d on a non-dyadic edge (reported only); mutants move %s"
                  % (kind, S, n * n, int(ok.sum()), int((~ok).sum()), here))
            assert (kind == "dyadic") <= bool(ok.all())
            if kind == "axis" and S == 1:
                # column 7 has dir.x == 0 and row 7 dir.y == 0: rays in the planes x = 0 and y = 0, where the four
                # squares meet (the lowest face wins) and, behind them, the edge of the lone triangle lies
                assert all(L.render_dir(i, 7, 0, 0, 1, d0)[0] == 0 and L.render_dir(7, i, 0, 0, 1, d0)[1] == 0
                           for i in range(n))
                assert ok[:, 7].all() and ok[7, :].all()
                assert (want_f[3:12, 7] >= 0).all() and (want_f[7, 3:12] >= 0).all()
                assert (want_f[[0, 1, 2, 12, 13, 14, 15], 7] == 49).all()
    print("render: mutants move %s pixels over the scenes" % moved)
    assert all(v >= MIN_ITEMS for v in moved.values())


# ---- 4. mesh_colour.hip ---------------------------------------------------------------------------------------------
def test_colour_specification_equals_the_fraction_rule():
    tris = L.colour_fixture()
    verts, faces = L.colour_pack(tris)
    T = np.asarray(L.COLOUR_CAMERA, F32)[None]
    img = np.zeros((1, 137, 137, 3), F32)
    moved = dict.fromkeys(L.COLOUR_CLAUSES, 0)
    for S in (1, 2):
        zb = L.colour_zbuffer(tris, S)
        assert np.array_equal(_bits(postprocess.zbuffer_arrays(verts, faces, T, S)[0]), _bits(L.colour_zbuffer_f32(zb, S)))
        for tol in (0.0, float(F32(1e-3))):
            seen = L.colour_seen(tris, zb, S, tol)
            cls = postprocess.colour_arrays(verts, faces, img, T, S=S, rel_tol=tol, fill_iters=0)[1]
            assert np.array_equal(cls, np.array(seen, np.uint8))
        base = L.colour_seen(tris, zb, S, 0)
        for c in L.COLOUR_CLAUSES:
            z2 = L.colour_zbuffer(tris, S, (c,))
            s2 = L.colour_seen(tris, z2, S, 0, (c,))
            sub = sum(1 for k in set(zb) | set(z2) if zb.get(k) != z2.get(k))
            vert = sum(a != b for a, b in zip(base, s2))
            moved[c] += sub + vert
            print("colour S=%d %-5s: %d covered sub-pixels, %d vertices (%d seen); the mutant moves %d sub-pixels and %d "
                  "vertices" % (S, c, len(zb), len(base), sum(base), sub, vert))
    assert all(v >= MIN_ITEMS for v in moved.values())
    # x = 0 is inside the image, x = 137 S outside
    seen = L.colour_seen(tris, L.colour_zbuffer(tris, 1), 1, 0)
    assert seen[3 * 4] == 1 and seen[3 * 5 + 1] == 0 and seen[3 * 6] == 0


# ---- 5. marching_cubes.hip ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mc_tables():
    ntri, tri, _ = MO.gen.build_tables()
    assert np.array_equal(MO.gen.CORNERS.astype(int), np.array(L.MC_CORNERS))
    return ntri, tri, MO.gen.edge_geometry()


@pytest.mark.parametrize("iso2", [0, 1])
def test_mc_oracle_equals_the_integer_rule_on_all_labelings(mc_tables, iso2):
    ntri, tri, eg = mc_tables
    lab = L.mc_single_volume(L.MC_CORNERS)
    vol = L.mc_values_f32(lab, iso2)
    if iso2 == 0:
        assert (np.signbit(vol) & (vol == 0)).any() and (~np.signbit(vol) & (vol == 0)).any()    # both zeros
    verts, faces = L.mc_pack(*L.mc_reference(lab, iso2, ntri, tri, eg))
    ov, of = MO.marching_cubes(vol, L.mc_params(lab.shape[0] - 1), iso2 / 2.0)
    assert np.array_equal(_bits(ov), _bits(verts)) and np.array_equal(of, faces)
    assert MO.mesh_is_closed_and_oriented(faces) == (True, 0)
    zero_area = int((np.cross(verts[faces[:, 1]] - verts[faces[:, 0]], verts[faces[:, 2]] - verts[faces[:, 0]]) == 0)
                    .all(1).sum())
    mv, mf = L.mc_reference(lab, iso2, ntri, tri, eg, strict=("inside",))
    cells = L.mc_labelings()
    # the labelings whose mesh the mutant changes: each as its own R = 2 grid, rule against mutant
    moved = 0
    for one in L.mc_batch_volumes(L.MC_CORNERS):
        moved += L.mc_reference(one, iso2, ntri, tri, eg) != L.mc_reference(one, iso2, ntri, tri, eg, strict=("inside",))
    print("marching cubes iso %g: %d labelings, %d vertices, %d faces (%d of zero area, counted); the mutant v <= iso "
          "changes the mesh of %d labelings (%d vertices, %d faces)" % (iso2 / 2.0, len(cells), len(verts), len(faces), zero_area,
                                                            moved, len(mv), len(mf)))
    assert zero_area >= MIN_ITEMS and moved >= MIN_ITEMS and (len(mv), len(mf)) != (len(verts), len(faces))


def test_mc_batch_grids_equal_the_oracle(mc_tables):
    ntri, tri, eg = mc_tables
    labs = L.mc_batch_volumes(L.MC_CORNERS)
    for i in range(0, len(labs), 37):
        for iso2 in (0, 1):
            verts, faces = L.mc_pack(*L.mc_reference(labs[i], iso2, ntri, tri, eg))
            ov, of = MO.marching_cubes(L.mc_values_f32(labs[i], iso2), L.mc_params(2), iso2 / 2.0)
            assert np.array_equal(_bits(ov), _bits(verts)) and np.array_equal(of, faces)


# ---- 6. grid_band.hip -----------------------------------------------------------------------------------------------
def test_band_restatement_equals_the_fraction_rule():
    moved, cells = {}, 0
    for field, iso in L.band_fields():
        vol = L.band_pack_field(field)
        for s in (2, 4):
            for margin in (Fraction(0), Fraction(1, 2)):
                base = L.band_cell_rule(field, s, iso, margin)
                ref = BR.cell_rule(vol, L.BAND_R, s, iso / 4.0, float(margin))
                assert np.array_equal(np.array(base), ref)
                cells += ref.size
                for c in L.BAND_CLAUSES:
                    m = np.array(L.band_cell_rule(field, s, iso, margin, strict=(c,)))
                    moved[c, float(margin)] = moved.get((c, float(margin)), 0) + int((m != ref).sum())
                for rounds in (0, 1, 2):
                    mask = L.band_dilate(base, rounds)
                    assert np.array_equal(np.array(mask), BR.dilate(ref, rounds))
                    assert np.array_equal(L.band_points(mask, s), np.nonzero(BR.band_mask(np.array(mask), L.BAND_R, s))[0])
                    fill = L.band_pack_fill(L.band_fill(field, mask, s))
                    assert np.array_equal(_bits(fill), _bits(BR.fill(vol, np.array(mask), L.BAND_R, s)))
    print("grid band: %d cell decisions; mutants move %s" % (cells, moved))
    assert all(v >= MIN_ITEMS for v in moved.values())
    # lo == iso with hi > iso is inactive, hi == iso with lo < iso is active (margin 0)
    n = L.BAND_R + 1
    flat = [[[0] * n for _ in range(n)] for _ in range(n)]
    up = [[[2 if x == 0 else 0 for x in range(n)] for _ in range(n)] for _ in range(n)]
    down = [[[-2 if x == 0 else 0 for x in range(n)] for _ in range(n)] for _ in range(n)]
    assert not np.array(L.band_cell_rule(flat, 4, 0, 0)).any() and not np.array(L.band_cell_rule(up, 4, 0, 0)).any()
    assert np.array(L.band_cell_rule(down, 4, 0, 0))[:, :, 0].all()
    assert not np.array(L.band_cell_rule(down, 4, 0, 0))[:, :, 1:].any()


# ---- 7. mesh_simplify.hip -------------------------------------------------------------------------------------------
def test_simplify_specification_equals_the_integer_cells():
    verts = L.simplify_vertices()
    cells = L.simplify_cells(verts)
    origin, h = postprocess.simplify_lattice(L.SIMPLIFY_BOX, L.SIMPLIFY_CELLS)
    assert np.array_equal(postprocess._simplify_cells(verts, origin, h, L.SIMPLIFY_CELLS), np.array(cells))
    faces = np.stack([np.arange(len(verts) - 2), np.arange(1, len(verts) - 1), np.arange(2, len(verts))], 1).astype(np.int32)
    _, _, vmap, first = postprocess.simplify_arrays(verts, faces, L.SIMPLIFY_BOX, L.SIMPLIFY_CELLS)
    want_vmap, want_first = L.simplify_vmap(cells)
    assert np.array_equal(vmap, want_vmap) and np.array_equal(first, want_first)
    moved = sum(a != b for a, b in zip(cells, L.simplify_cells(verts, strict=("border",))))
    print("simplify: %d vertices, %d clusters; the mutant 'a border vertex goes to the lower cell' moves %d vertices"
          % (len(verts), len(want_first), moved))
    assert moved >= MIN_ITEMS
    # on the border: the upper cell; the maximum face: clamped; one ulp either side of a border in [-1, -1/2] separates
    below, on, above = L._f32_neighbours(-0.75)
    assert [L.simplify_cell(v) for v in (below, on, above)] == [0, 1, 1]
    assert L.simplify_cell(F32(1.0)) == L.SIMPLIFY_CELLS - 1 and L.simplify_cell(F32(1.5)) == L.SIMPLIFY_CELLS - 1
    assert L.simplify_cell(F32(-1.5)) == 0 and L.simplify_cell(L._f32_neighbours(-1.0)[0]) == 0

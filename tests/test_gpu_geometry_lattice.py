"""The geometry kernels at equality: every kernel whose written rule says what happens on a tie, run on the exact dyadic
lattices of tests/geometry_lattice.py and compared, bit for bit, with that module's integer / Fraction statement of the
rule -- not with the float32 restatements, which share a hand with the kernels.  tests/test_geometry_lattice_host.py
asserts on the CPU that the restatements agree with the integer rules and how many items a strict mutant of each
clause moves.  One ``LATTICE`` line per kernel path: the items compared."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import geometry_lattice as L
import voxel_reference as VR
from oracle import mc_oracle as MO

pytestmark = pytest.mark.gpu

F32 = np.float32


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def line(kernel, what):
    print("\nLATTICE %s: %s" % (kernel, what))


# ---- 1. voxel.hip ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [16, 32])
def test_voxel_surface_fill_and_index_grid(dim):
    from disn_amd import voxel
    fx = L.voxel_fixture(dim)
    cells, overflow = L.voxel_surface(fx["tris"], dim)
    assert not overflow
    want = L.voxel_dense(cells, dim)
    vox = voxel.surface_voxels(dev(fx["verts"]), dev(fx["faces"], np.int32), dim)
    got = voxel.to_dense(vox)
    assert (vox.kmin, vox.n) == L.voxel_key_range(dim)
    tie = len(cells - L.voxel_surface(fx["tris"], dim, strict=L.VOXEL_CLAUSES)[0])
    line("voxel_tri_kernel + voxel_big_kernel dim %d" % dim, "%d triangles, %d occupied cells (%d decided by a tie), %d "
         "differ" % (len(fx["tris"]), len(cells), tie, int((got != want).sum())))
    assert np.array_equal(got, want), np.argwhere(got != want)[:8].tolist()
    # each group alone as well: a group's ties are not covered by another group's cells
    for name, group in fx["groups"].items():
        own = L.voxel_dense(L.voxel_surface(group, dim)[0], dim)
        verts = L._scaled_f32([p for t in group for p in t], dim)
        faces = np.arange(3 * len(group), dtype=np.int32).reshape(-1, 3)
        one = voxel.to_dense(voxel.surface_voxels(dev(verts), dev(faces, np.int32), dim))
        assert np.array_equal(one, own), (name, int((one != own).sum()))
    assert np.array_equal(voxel.to_dense(voxel.fill(vox)), VR.fill(want))
    assert np.array_equal(voxel.to_dense(voxel.index_grid(vox)), VR.index_grid(want, dim))


@pytest.mark.parametrize("dim", [16, 32])
def test_voxel_touching_the_sentinel_key_raises(dim):
    from disn_amd import voxel
    tri, verts, faces = L.voxel_sentinel_triangle(dim)
    assert L.voxel_surface([tri], dim)[1]
    with pytest.raises(ValueError, match="key range"):
        voxel.surface_voxels(dev(verts), dev(faces, np.int32), dim)


# ---- 2. mesh_sdf.hip ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[8, 16])
def sdf_world(request):
    res = request.param
    nodes = L.sdf_nodes(res)
    out = {}
    for name, f in L.sdf_fixtures(res).items():
        d2 = L.sdf_d2(nodes, f["tris"])
        out[name] = (f, d2, L.sdf_sign(res, f["tris"], d2, L.SDF_NODE ** 2, 3))
    return res, nodes, out


def test_sdf_unsigned_distance_and_sign(sdf_world):
    """u on the axis-aligned fixtures: bits of float32(sqrt(rational d^2)) wherever the restatement has them, at no
    more than 2 % of the nodes otherwise, and those within the module's 1e-6; 0 on the surface.  The octahedra (a
    divisor 3 * 2^k in every face projection) serve the sign pass: their u is held to 1e-6 and to 0 on the surface.
    sign: the rational crossing rule plus the flood at EVERY node; sdf = -+u - offset, so -0.0 - offset on a box."""
    from disn_amd import mesh_sdf
    import mesh_sdf_reference as SR
    res, nodes, world = sdf_world
    den, n = 2 * res, res + 1
    axes = mesh_sdf.grid_axes(F32([-1, -1, -1, 1, 1, 1]), res)
    pts = L.sdf_world(nodes, res)
    tau, steps = mesh_sdf.seal_params(axes, 1.0)
    assert Fraction(tau) ** 2 * den ** 2 == L.SDF_NODE ** 2 and steps == 3
    for name, (f, d2, sign) in world.items():
        verts, faces = L.sdf_mesh_arrays(f["tris"], res)
        m = mesh_sdf.MeshBvh(verts, faces)
        exact = np.array([float(L.sqrt_to_f32(d / den ** 2)) for d in d2], F32)
        exact64 = np.array([float(d) for d in d2]) ** 0.5 / den
        on = np.array([d == 0 for d in d2])
        restated = bits(SR.udf(pts, verts, faces)) == bits(exact)
        u_grid = None
        for entry in ("grid", "points"):
            for brute in (False, True):
                if entry == "grid":
                    u = host(mesh_sdf.unsigned_distance_grid(m, None, axes, brute=brute))
                    u_grid = u if not brute else u_grid
                else:
                    u = host(mesh_sdf.unsigned_distance(m, None, dev(pts), brute=brute))
                assert np.abs(u.astype(np.float64) - exact64).max() <= 1e-6
                assert (u[on] == 0).all(), int((u[on] != 0).sum())
                if name not in L.SDF_AXIS_ALIGNED:
                    continue
                same = bits(u) == bits(exact)
                print("udf res %d %-26s %-6s brute=%d: %d nodes, %d differ from the rational (restatement: %d), worst "
                      "%.3g" % (res, name, entry, brute, len(nodes), int((~same).sum()), int((~restated).sum()),
                                np.abs(u - exact64).max()))
                assert same[restated].all()
                assert (~same).mean() <= 0.02
        for offset in (0.0, 0.015625):
            sdf, out = mesh_sdf.sign_grid(m, None, axes, dev(u_grid), tau, steps, offset)
            out, sdf = host(out).astype(bool), host(sdf)
            assert np.array_equal(out, np.array(sign)), (name, int((out != np.array(sign)).sum()))
            assert np.array_equal(bits(sdf), bits(np.where(out, u_grid, -u_grid) - F32(offset)))
            if "lo" in f:                                  # a closed box: every surface node is inside
                assert not out[on].any() and (bits(sdf[on]) == bits(F32(-0.0) - F32(offset))).all()
        if "lo" in f:
            truth = [not all(f["lo"][a] <= p[a] <= f["hi"][a] for a in range(3)) for p in nodes]
            assert truth == sign
        line("udf_grid_kernel, udf_points_kernel, sign pass res %d %s" % (res, name),
             "%d nodes, %d on the surface (u == 0), %d inside, 0 differ"
             % (len(nodes), int(on.sum()), len(nodes) - sum(sign)))


def test_sdf_points_on_vertices_edges_and_faces():
    """lattice points that are no grid nodes: triangle vertices, edge midpoints and face points of the box"""
    from disn_amd import mesh_sdf
    res = 16
    f = L.sdf_fixtures(res)["box"]
    pts = set()
    for a, b, c in f["tris"]:
        pts |= {a, b, c, tuple((x + y) // 2 for x, y in zip(a, b)), tuple((x + y) // 2 for x, y in zip(b, c)),
                tuple((2 * x + y + z) // 4 for x, y, z in zip(a, b, c))}
    pts = sorted(p for p in pts if any(L.point_tri_d2(p, t) == 0 for t in f["tris"]))
    assert len(pts) >= 32
    verts, faces = L.sdf_mesh_arrays(f["tris"], res)
    m = mesh_sdf.MeshBvh(verts, faces)
    for brute in (False, True):
        u = host(mesh_sdf.unsigned_distance(m, None, dev(L.sdf_world(pts, res)), brute=brute))
        assert (u == 0).all(), int((u != 0).sum())
    line("udf_points_kernel", "%d points on vertices, edges and faces: u == 0" % len(pts))


# ---- 3. render.hip --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", L.RENDER_SCENES)
def test_render_face_depth_and_alpha(kind):
    from disn_amd import mesh_sdf, render
    tris = L.render_scene(kind)
    verts, faces = L.render_pack(tris)
    m = mesh_sdf.MeshBvh(verts, faces)
    assert not np.array_equal(m.order_host, np.arange(len(tris)))            # leaf order is not file order
    if kind == "axis":                           # tree boxes have faces on the planes x = 0 and y = 0 of the rays
        import mesh_sdf_reference as SR
        bvh = SR.parse_bvh(m.host, len(tris))
        for a in (0, 1):
            assert (np.abs(bvh["lo"][:, a]) < 1e-4).any() or (np.abs(bvh["hi"][:, a]) < 1e-4).any()
    n = L.RENDER_SIZE
    cam, d0 = L.render_camera(kind)
    cam = np.asarray(cam, F32)[None]
    for S in (1, 2):
        exp = L.render_expected(tris, S, d0=d0)
        ok = np.array([e[3] for e in exp]).reshape(n, n)
        want_f = np.array([e[0] for e in exp]).reshape(n, n)
        want_d = np.array([float(e[1]) if e[1] is not None else 0.0 for e in exp], F32).reshape(n, n)
        want_a = np.array([(2 * 255 * e[2] + S * S) // (2 * S * S) for e in exp]).reshape(n, n)
        for brute in (False, True):
            out = render.render_views(m, None, size=(n, n), samples=S, brute=brute, want=("rgba", "depth", "face"),
                                      cams=cam)
            face, depth, alpha = host(out["face"])[0], host(out["depth"])[0], host(out["rgba"])[0, ..., 3]
            off = (face != want_f) & ~ok
            line("render_views_kernel %s S=%d brute=%d" % (kind, S, brute),
                 "%d pixels, %d asserted, %d on a non-dyadic edge reported only (%d of them differ from the exact "
                 "classification)" % (n * n, int(ok.sum()), int((~ok).sum()), int(off.sum())))
            assert np.array_equal(face[ok], want_f[ok]), np.argwhere((face != want_f) & ok)[:8].tolist()
            assert np.array_equal(bits(depth)[ok], bits(want_d)[ok])
            assert np.array_equal(alpha[ok], want_a[ok])


# ---- 4. mesh_colour.hip ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2])
def test_colour_zbuffer_and_seen(S):
    from disn_amd import postprocess
    tris = L.colour_fixture()
    verts, faces = L.colour_pack(tris)
    T = np.asarray(L.COLOUR_CAMERA, F32)[None, None]
    zb = L.colour_zbuffer(tris, S)
    mesh = (dev(verts), dev(faces, np.int32))
    got = host(postprocess.zbuffer_meshes_device([mesh], T, views_per_mesh=1, S=S))[0, 0]
    want = L.colour_zbuffer_f32(zb, S)
    line("raster_kernel + raster_big_kernel S=%d" % S, "%d triangles, %d covered sub-pixels of %d, %d differ"
         % (len(tris), len(zb), want.size, int((bits(got) != bits(want)).sum())))
    assert np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:8].tolist()
    img = torch.zeros((1, 1, 137, 137, 3), dtype=torch.float32, device="cuda")
    for tol in (0.0, 1e-3):
        seen = np.array(L.colour_seen(tris, zb, S, float(F32(tol))), np.uint8)
        _, cls = postprocess.colour_meshes_device([mesh], img, T, views_per_mesh=1, S=S, rel_tol=tol, fill_iters=0)
        cls = host(cls[0])
        line("vertex_kernel S=%d rel_tol=%g" % (S, tol), "%d vertices, %d seen, %d differ"
             % (len(seen), int(seen.sum()), int((cls != seen).sum())))
        assert np.array_equal(cls, seen), np.nonzero(cls != seen)[0][:8].tolist()


# ---- 5. marching_cubes.hip ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mc_tables():
    ntri, tri, _ = MO.gen.build_tables()
    assert np.array_equal(MO.gen.CORNERS.astype(int), np.array(L.MC_CORNERS))
    return ntri, tri, MO.gen.edge_geometry()


@pytest.mark.parametrize("iso2", [0, 1])
def test_mc_all_labelings_in_one_volume(mc_tables, iso2):
    from disn_amd import isosurface
    ntri, tri, eg = mc_tables
    lab = L.mc_single_volume(L.MC_CORNERS)
    res = lab.shape[0] - 1
    vol = L.mc_values_f32(lab, iso2)
    want_v, want_f = L.mc_pack(*L.mc_reference(lab, iso2, ntri, tri, eg))
    v, f = isosurface.marching_cubes(dev(vol).reshape(-1), L.mc_params(res), res, iso2 / 2.0)
    v, f = host(v), host(f)
    line("mc_flags_kernel, mc_verts_kernel, mc_faces_kernel iso %g" % (iso2 / 2.0),
         "%d labelings, %d vertices, %d faces" % (3 ** 8, len(want_v), len(want_f)))
    assert np.array_equal(f, want_f) and np.array_equal(bits(v), bits(want_v))
    ov, of = MO.marching_cubes(vol, L.mc_params(res), iso2 / 2.0)
    assert np.array_equal(of, f) and np.array_equal(bits(ov), bits(v))
    assert MO.mesh_is_closed_and_oriented(f) == (True, 0)


@pytest.mark.parametrize("iso2", [0, 1])
def test_mc_all_labelings_as_a_batch(mc_tables, iso2):
    from disn_amd import isosurface
    ntri, tri, eg = mc_tables
    labs = L.mc_batch_volumes(L.MC_CORNERS)
    B = len(labs)
    vols = np.stack([L.mc_values_f32(x, iso2) for x in labs])
    meshes = isosurface.marching_cubes_batch(dev(vols).reshape(B, -1), [L.mc_params(2)] * B, 2, iso2 / 2.0)
    assert len(meshes) == B
    all_v = host(torch.cat([v for v, _ in meshes]))              # one copy each: the pairs are views of two tensors
    all_f = host(torch.cat([f for _, f in meshes]))
    nv = nf = 0
    for i, (v, f) in enumerate(meshes):
        want_v, want_f = L.mc_pack(*L.mc_reference(labs[i], iso2, ntri, tri, eg))
        assert (len(v), len(f)) == (len(want_v), len(want_f)), i
        assert np.array_equal(all_f[nf:nf + len(f)], want_f), i
        assert np.array_equal(bits(all_v[nv:nv + len(v)]), bits(want_v)), i
        nv, nf = nv + len(want_v), nf + len(want_f)
    line("mc_flags_batch_kernel, mc_verts_batch_kernel, mc_faces_batch_kernel iso %g" % (iso2 / 2.0),
         "%d grids of R = 2, %d vertices, %d faces" % (B, nv, nf))


# ---- 6. grid_band.hip -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [2, 4])
def test_band_selection_and_fill(s):
    from disn_amd import ops
    R, cells = L.BAND_R, 0
    for field, iso in L.band_fields():
        vol = L.band_pack_field(field)
        for margin in (Fraction(0), Fraction(1, 2)):
            base = L.band_cell_rule(field, s, iso, margin)
            for rounds in (0, 1, 2):
                want = L.band_dilate(base, rounds)
                grid = dev(vol)
                mask, idx, counts = ops.grid_band_select(grid, R, s, iso / 4.0, float(margin), rounds)
                nband, ncell = (int(v) for v in counts.tolist())
                tag = (iso, s, margin, rounds)
                assert np.array_equal(host(mask).reshape((R // s,) * 3), np.array(want, np.int32)), tag
                pts = L.band_points(want, s)
                assert ncell == int(np.array(want).sum()) and nband == len(pts), tag
                assert np.array_equal(host(idx[:nband]), np.array(pts, host(idx).dtype)), tag
                ops.grid_band_fill(grid, R, s, mask)
                assert np.array_equal(bits(host(grid)), bits(L.band_pack_fill(L.band_fill(field, want, s)))), tag
                cells += (R // s) ** 3
    line("band_cell_rule_kernel, band_dilate_kernel, band_compact_kernel, band_fill_kernel stride %d" % s,
         "%d cell decisions, point lists and fills: 0 differ" % cells)


# ---- 7. mesh_simplify.hip -------------------------------------------------------------------------------------------
def test_simplify_cells_on_borders():
    from disn_amd import postprocess
    verts = L.simplify_vertices()
    faces = np.stack([np.arange(len(verts) - 2), np.arange(1, len(verts) - 1), np.arange(2, len(verts))], 1).astype(np.int32)
    cells = L.simplify_cells(verts)
    want_vmap, want_first = L.simplify_vmap(cells)
    hv, hf, hmap, hfirst = postprocess.simplify_arrays(verts, faces, L.SIMPLIFY_BOX, L.SIMPLIFY_CELLS)
    v, f, vmap, first = postprocess.simplify_arrays_device(dev(verts), dev(faces, np.int32), L.SIMPLIFY_BOX,
                                                           L.SIMPLIFY_CELLS)
    line("vertex_claim_kernel .. emit_faces_kernel", "%d vertices on and beside cell borders, %d clusters"
         % (len(verts), len(want_first)))
    assert np.array_equal(host(vmap), np.array(want_vmap, np.int32)) and np.array_equal(host(first), want_first)
    assert np.array_equal(host(vmap), hmap) and np.array_equal(host(first), hfirst)
    assert np.array_equal(host(f), hf) and np.array_equal(bits(host(v)), bits(hv))

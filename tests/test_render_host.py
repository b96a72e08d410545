"""CPU tests of view rendering's host side (disn_amd/render.py, disn_amd/create_img_h5.py): the camera matrices
against the reference's recorded ones, the ray construction against the stored camera through the numpy restatement
of the ray caster, and the default mode of the driver on a small synthetic tree.  (-m "not gpu")"""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_sdf_reference as R  # noqa: E402
import render_reference as RR  # noqa: E402

from disn_amd import render  # noqa: E402

IDENT = np.float32([0, 0, 0, 1])


@pytest.fixture(scope="module")
def pins():
    return np.load(os.path.join(ROOT, "tests", "golden", "view_pins.npz"))


# ---- (a) camera math ---------------------------------------------------------------------------------------------
def test_view_matrices_match_the_reference_pins(pins):
    """within 2 float32 ulp of each matrix's largest entry: only the association of the float64 products may differ"""
    names = ("K", "RT", "trans_mat", "regress_mat", "obj_rot_mat")
    for n, norm in enumerate(pins["norm_params"]):
        for i, row in enumerate(pins["rows"]):
            got = dict(zip(names, render.view_matrices(row, norm)))
            for k in names:
                want = pins[k][n, i]
                assert got[k].shape == want.shape
                ulp = float(np.spacing(np.float32(np.abs(want).max())))
                err = np.abs(np.asarray(got[k], np.float64) - want.astype(np.float64)).max()
                assert err <= 2 * ulp, (k, n, i, err / ulp)
    assert render.view_matrices(pins["rows"][0], IDENT)[4].dtype == np.float32
    assert np.abs(render.get_rotate_matrix(-np.pi / 2) - pins["rot_mat"]).max() <= 1e-15


def test_regress_mat_times_K_is_trans_mat(pins):
    """the reference's own self-check (get_img): regress_mat . K^T = trans_mat"""
    for norm in pins["norm_params"]:
        for row in pins["rows"]:
            K, _, trans_mat, regress_mat, _ = render.view_matrices(row, norm)
            back = np.dot(regress_mat.astype(np.float32), np.transpose(K.astype(np.float32)))
            assert np.abs(back - trans_mat).max() <= 4 * np.spacing(np.float32(np.abs(trans_mat).max()))


def test_random_view_params_ranges_and_seed():
    a = render.random_view_params(np.random.default_rng([0, 3]), 24)
    b = render.random_view_params(np.random.default_rng([0, 3]), 24)
    assert a.shape == (24, 5) and np.array_equal(a, b)
    assert (a[:, 0] >= 0).all() and (a[:, 0] < 360).all() and (a[:, 1] >= 25).all() and (a[:, 1] <= 30).all()
    assert not a[:, 2].any() and (a[:, 3] >= 0.65).all() and (a[:, 3] <= 0.95).all() and (a[:, 4] == 25).all()
    c = render.random_view_params(np.random.default_rng(0), 4, el=(0, 10), dist=(1.0, 1.0), tilt=2.0)
    assert (c[:, 1] <= 10).all() and (c[:, 3] == 1.0).all() and (c[:, 2] == 2.0).all()


# ---- (b) the restated ray caster ties ray_cameras to the stored camera ---------------------------------------------
@pytest.fixture(scope="module")
def tripod_renders():
    v, f = RR.tripod()
    out = []
    for az, el, d, W, H, S in RR.TRIPOD_VIEWS:
        row = [az, el, 0.0, d, 25.0]
        rgba, _, _ = RR.render(v, f, render.ray_cameras([row], W, H), W, H, S)
        out.append((render.view_matrices(row, IDENT, W, H)[2], rgba[0, ..., 3]))
    return v, out


def test_tripod_vertices_land_on_the_mask(tripod_renders):
    v, views = tripod_renders
    for trans_mat, alpha in views:
        inside, on = RR.vertex_mask_check(v, trans_mat, alpha)
        assert inside >= 0.9 and on == 1.0, (inside, on)


def test_tripod_check_rejects_flipped_and_transposed_images(tripod_renders):
    v, views = tripod_renders
    for trans_mat, alpha in views:
        wrong = [alpha[::-1], alpha[:, ::-1]] + ([alpha.T] if alpha.shape[0] == alpha.shape[1] else [])
        for img in wrong:
            assert RR.vertex_mask_check(v, trans_mat, img)[1] < 1.0


def test_hit_pixels_lie_inside_the_projected_hull():
    """a convex mesh at S = 1: a pixel is hit only if its centre is inside the hull of the projected vertices"""
    v, f = R.icosphere(1, 0.4)
    v = (v + np.float32([0.1, -0.05, 0.2])).astype(np.float32)
    for az, el, d, W, H in ((30.0, 27.0, 0.8, 137, 137), (200.0, 25.0, 0.7, 37, 29), (0.0, 0.0, 0.9, 33, 33)):
        row = [az, el, 0.0, d, 25.0]
        rgba, depth, face = RR.render(v, f, render.ray_cameras([row], W, H), W, H, 1)
        hull = RR.convex_hull(RR.project(v, render.view_matrices(row, IDENT, W, H)[2]))
        ii, jj = np.nonzero(rgba[0, ..., 3])
        assert len(ii) > 20 and (rgba[0, ..., 3][ii, jj] == 255).all()
        assert RR.outside_hull(hull, np.stack([jj + 0.5, ii + 0.5], 1)).max() <= 1e-3
        assert ((depth[0] > 0) == (face[0] >= 0)).all() and ((face[0] >= 0) == (rgba[0, ..., 3] > 0)).all()


# ---- (c) the default mode of the driver ------------------------------------------------------------------------------
def _tree(tmp_path, n_views=3):
    from PIL import Image
    from disn_amd import data_sdf
    cat, objs = "03001627", ["objA", "objB"]
    rng = np.random.default_rng(4)
    lst = tmp_path / "lst"
    lst.mkdir()
    (lst / (cat + "_test.lst")).write_text(objs[0] + "\n")
    (lst / (cat + "_train.lst")).write_text(objs[1] + "\n")
    dirs = {k: str(tmp_path / k) for k in ("mesh_dir", "norm_mesh_dir", "sdf_dir", "rendered_dir", "renderedh5_dir")}
    pngs, rows = {}, {}
    for k, obj in enumerate(objs):
        d = tmp_path / "rendered_dir" / cat / obj / "rendering"
        d.mkdir(parents=True)
        rows[obj] = render.random_view_params(rng, n_views)
        rows[obj][:, 2] = k * 1.5
        np.savetxt(d / "rendering_metadata.txt", rows[obj])
        (d / "renderings.txt").write_text("".join("%02d.png\n" % i for i in range(n_views)))
        for i in range(n_views):
            pngs[obj, i] = rng.integers(0, 256, (137, 137, 4), dtype=np.uint8)
            Image.fromarray(pngs[obj, i]).save(d / ("%02d.png" % i))
        smp = rng.uniform(-0.5, 0.5, (200, 4)).astype(np.float32)
        data_sdf.save_sample(dirs["sdf_dir"], cat, obj, np.zeros((1, 3), np.float32), smp,
                             np.float32([0.01 * k, -0.02, 0.03, 0.5 + 0.1 * k]), np.float32([-1, -1, -1, 1, 1, 1]))
    info = {"lst_dir": str(lst), "cats": {"chair": cat}, "all_cats": ["chair"], "raw_dirs_v1": dirs}
    (tmp_path / "info.json").write_text(json.dumps(info))
    return cat, objs, dirs, pngs, rows


def test_default_mode_writes_view_files_the_loaders_read(tmp_path):
    from disn_amd import create_img_h5, data_cam, data_sdf
    cat, objs, dirs, pngs, rows = _tree(tmp_path)
    stats = create_img_h5.main(["--info", str(tmp_path / "info.json")])
    assert stats == {"objects": 2, "rendered": 0, "written": 6}
    for obj in objs:
        d = os.path.join(dirs["renderedh5_dir"], cat, obj)
        assert sorted(os.listdir(d)) == ["00.npz", "01.npz", "02.npz"]
        norm = np.load(os.path.join(dirs["sdf_dir"], cat, obj, "ori_sample.npz"))["norm_params"]
        for i in range(3):
            z = np.load(os.path.join(d, "%02d.npz" % i))
            assert sorted(z.files) == ["K", "RT", "img_arr", "obj_rot_mat", "regress_mat", "trans_mat"]
            assert z["img_arr"].dtype == np.uint8 and z["img_arr"].shape == (137, 137, 4)
            assert np.array_equal(z["img_arr"], pngs[obj, i][:, :, [2, 1, 0, 3]])          # BGRA
            shapes = {"K": (3, 3), "RT": (3, 4), "trans_mat": (4, 3), "regress_mat": (4, 3), "obj_rot_mat": (3, 3)}
            for k, s in shapes.items():
                assert z[k].dtype == np.float32 and z[k].shape == s
            want = render.view_matrices(np.loadtxt(os.path.join(
                dirs["rendered_dir"], cat, obj, "rendering", "rendering_metadata.txt"))[i], norm)
            assert np.array_equal(z["trans_mat"], want[2].astype(np.float32))
            assert np.array_equal(z["obj_rot_mat"], want[4])
    # a second run finds every view and writes nothing
    before = {p: os.stat(os.path.join(dirs["renderedh5_dir"], cat, objs[0], p)).st_mtime_ns for p in os.listdir(d)}
    assert create_img_h5.main(["--info", str(tmp_path / "info.json"), "--category", "chair"])["written"] == 0
    assert before == {p: os.stat(os.path.join(dirs["renderedh5_dir"], cat, objs[0], p)).st_mtime_ns for p in before}
    # an unreadable view file is written again
    with open(os.path.join(dirs["renderedh5_dir"], cat, objs[1], "01.npz"), "wb") as f:
        f.write(b"not a zip")
    assert create_img_h5.main(["--info", str(tmp_path / "info.json")])["written"] == 1
    # both loaders return a batch from the result
    flags = SimpleNamespace(num_points=16, num_sample_points=64, batch_size=2, img_h=137, img_w=137, max_epoch=1)
    info = {"rendered_dir": dirs["renderedh5_dir"], "sdf_dir": dirs["sdf_dir"]}
    listinfo = [(cat, objs[0], 2), (cat, objs[1], 0)]
    b = data_sdf.Pt_sdf_img(flags, listinfo=listinfo, info=info, shuffle=False, seed=0).get_batch(0)
    assert b["img"].shape == (2, 137, 137, 3) and b["trans_mat"].shape == (2, 4, 3)
    assert np.array_equal(b["img"][0], pngs[objs[0], 2][:, :, [2, 1, 0]].astype(np.float32) / np.float32(255))
    c = data_cam.Pt_sdf_img_cam(flags, listinfo=listinfo, info=info, shuffle=False, seed=0).get_batch(0)
    assert c["img"].shape == (2, 137, 137, 4) and c["RT"].shape == (2, 4, 3) and np.isfinite(c["RT"]).all()
    z = np.load(os.path.join(dirs["renderedh5_dir"], cat, objs[1], "00.npz"))
    assert np.array_equal(c["RT"][1], z["regress_mat"]) and np.array_equal(c["trans_mat"][1], z["trans_mat"])


def test_read_obj_albedo_follows_the_fan_triangulation(tmp_path):
    from disn_amd import mesh_sdf
    (tmp_path / "m.mtl").write_text("newmtl red\nKa 0 0 0\nKd 0.9 0.1 0.2\nnewmtl blue\nKd 0.1 0.2 0.7\n")
    (tmp_path / "model.obj").write_text(
        "mtllib m.mtl\n"
        "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nv 0 0 1\nv 1 0 1\nv 1 1 1\nv 0 1 1\n"
        "f 1 2 3\n"                      # before any usemtl: grey
        "usemtl red\nf 1 2 3 4\nf 5/1 6/2 7/3 8/4\n"
        "usemtl blue\nf 1 2 6 5 8\n"     # a pentagon: three triangles
        "usemtl missing\nf 2 3 7\n")
    v, f = mesh_sdf.read_obj_mesh(str(tmp_path / "model.obj"))
    alb = render.read_obj_albedo(str(tmp_path / "model.obj"), len(f))
    assert alb.shape == (len(f), 3) == (9, 3) and alb.dtype == np.float32
    want = [[0.8] * 3] + [[0.9, 0.1, 0.2]] * 4 + [[0.1, 0.2, 0.7]] * 3 + [[0.8] * 3]
    assert np.array_equal(alb, np.float32(want))
    with pytest.raises(AssertionError):
        render.read_obj_albedo(str(tmp_path / "model.obj"), len(f) + 1)
    (tmp_path / "plain.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    assert np.array_equal(render.read_obj_albedo(str(tmp_path / "plain.obj"), 1), np.float32([[0.8] * 3]))


# ---- host entries of the library -----------------------------------------------------------------------------------
def test_bvh_order_entry_leaves_the_image_unchanged():
    from disn_amd import _lib, mesh_sdf
    rng = np.random.default_rng(2)
    v = rng.uniform(-1, 1, (90, 3)).astype(np.float32)
    f = rng.integers(0, 90, (257, 3)).astype(np.int32)
    img, order = mesh_sdf.build_bvh_host_order(v, f)
    h = _lib.lib()
    plain = np.empty(h.disn_mesh_bvh_bytes(len(f)), np.uint8)
    assert h.disn_mesh_bvh_build(v.ctypes.data, len(v), f.ctypes.data, len(f), plain.ctypes.data, plain.nbytes) == 0
    assert np.array_equal(img, plain) and np.array_equal(mesh_sdf.build_bvh_host(v, f), plain)
    assert order.dtype == np.int32 and np.array_equal(np.sort(order), np.arange(len(f)))
    assert np.array_equal(R.parse_bvh(img, len(f))["tris"], v[f[order].astype(np.int64)])


def test_render_views_argument_validation_without_gpu():
    """<0 for invalid arguments, checked before any launch"""
    from disn_amd import _lib
    h = _lib.lib()

    def call(bvh=1, nf=12, order=1, albedo=None, cams=1, V=1, H=8, W=8, S=1, ambient=0.3, rgba=1, face=None):
        return h.disn_render_views(bvh, nf, order, albedo, cams, V, H, W, S, ambient, 0, rgba, None, face, None)
    assert call(bvh=None) == -1 and call(cams=None) == -1 and call(rgba=None) == -1 and call(nf=0) == -1
    assert call(S=0) == -1 and call(V=0) == -1 and call(ambient=1.5) == -1 and call(ambient=float("nan")) == -1
    assert call(order=None, albedo=1) == -1 and call(order=None, face=1) == -1
    assert call(S=5) == -2 and call(H=1025) == -2 and call(W=1025) == -2 and call(nf=(1 << 27) + 1) == -2

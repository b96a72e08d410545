"""GPU tests of view rendering (csrc/render.hip via disn_amd/render.py and disn_amd/create_img_h5.py): the BVH walk
against brute force and both against the float32 numpy restatement, bit for bit; the rendered mask against the
stored camera; and preprocess -> create_img_h5 --render on a sphere into a tree the loader reads."""
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

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

IDENT = np.float32([0, 0, 0, 1])


def _soup(seed, n):
    """the triangle soup of test_gpu_mesh_sdf.py: a duplicated, a degenerate and a nearly collinear triangle"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-0.8, 0.8, (3 * n, 3)).astype(np.float32)
    f = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    f[n - 1] = f[n - 2]
    v[1] = v[0]
    v[5] = v[3] + np.float32(0.5) * (v[4] - v[3])
    return v, f


def meshes():
    return {"icosphere": R.icosphere(2, 0.7), "torus": R.torus(), "soup": _soup(3, 300), "cube": RR.unit_cube()}


def cameras_33():
    """V = 3 at W = H = 33: an ordinary view; az 0 / el 0 (with S = 1 the centre ray runs along an axis and the
    centre row and column lie in coordinate planes, which hold three faces of the cube); and a camera placed by hand
    inside the icosphere, so every pixel hits a back face"""
    from disn_amd import render
    cams = render.ray_cameras([[30.0, 27.0, 0.0, 0.8, 25.0], [0.0, 0.0, 0.0, 0.9, 25.0],
                               [200.0, 25.0, 0.0, 0.7, 25.0]], 33, 33)
    cams[2, 0:3] = np.float32([0.1, 0.05, -0.02])
    return cams


def cameras_37x29():
    from disn_amd import render
    return render.ray_cameras([[123.0, 30.0, 0.0, 0.95, 25.0], [310.0, 26.0, 4.0, 0.65, 25.0]], 37, 29)


def camera_far():
    """the ordinary camera moved far behind itself and turned round: nothing is hit"""
    from disn_amd import render
    cams = render.ray_cameras([[30.0, 27.0, 0.0, 0.8, 25.0]], 33, 33)
    cams[0, 0:3] = cams[0, 0:3] * np.float32(8.0)
    cams[0, 3:12] = -cams[0, 3:12]
    return cams


CASES = (("v3", cameras_33, 33, 33, 1), ("s3", cameras_37x29, 37, 29, 3), ("far", camera_far, 33, 33, 2))


def _gpu(mesh, cams, W, H, S, brute, albedo=None, ambient=0.3):
    from disn_amd import render
    out = render.render_views(mesh, None, None, size=(W, H), samples=S, albedo=albedo, ambient=ambient, brute=brute,
                              want=("rgba", "depth", "face"), cams=cams)
    return tuple(out[k].cpu().numpy() for k in ("rgba", "depth", "face"))


_REF = {}


def _reference(name, case):
    """the restatement's result, computed once per (mesh, case) and shared"""
    if (name, case) not in _REF:
        v, f = meshes()[name]
        _, cams, W, H, S = [c for c in CASES if c[0] == case][0]
        _REF[name, case] = RR.render(v, f, cams(), W, H, S)
        for a in _REF[name, case]:
            a.setflags(write=False)
    return _REF[name, case]


# ---- (d) BVH == brute == restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c[0] for c in CASES])
@pytest.mark.parametrize("name", ["icosphere", "torus", "soup", "cube"])
def test_bvh_equals_brute_equals_restatement(name, case):
    from disn_amd import mesh_sdf
    v, f = meshes()[name]
    _, cams, W, H, S = [c for c in CASES if c[0] == case][0]
    m = mesh_sdf.MeshBvh(v, f)
    rgba, depth, face = _gpu(m, cams(), W, H, S, brute=False)
    rgba_b, depth_b, face_b = _gpu(m, cams(), W, H, S, brute=True)
    assert np.array_equal(face, face_b) and np.array_equal(depth, depth_b) and np.array_equal(rgba, rgba_b)
    want_rgba, want_depth, want_face = _reference(name, case)
    assert np.array_equal(face, want_face), int((face != want_face).sum())
    assert np.array_equal(depth, want_depth), np.abs(depth - want_depth).max()
    assert np.array_equal(rgba, want_rgba), int(np.abs(rgba.astype(int) - want_rgba.astype(int)).max())
    hit = face >= 0
    assert np.array_equal(hit, depth > 0) and np.array_equal(hit, rgba[..., 3] > 0)
    if case == "far":
        assert not hit.any() and not rgba.any()
    elif case == "v3":
        assert hit[0].any() and hit[1].any()
        if name == "icosphere":
            assert not hit[0].all() and hit[2].all()  # from inside: a back face behind every pixel
        if name == "soup":
            n = len(f)
            assert not (face == n - 1).any()          # the duplicate's tie goes to the lower face


def test_albedo_colours_are_those_of_face():
    from disn_amd import mesh_sdf
    rng = np.random.default_rng(11)
    for name in ("icosphere", "soup"):
        v, f = meshes()[name]
        albedo = rng.uniform(0.05, 1.0, (len(f), 3)).astype(np.float32)
        m = mesh_sdf.MeshBvh(v, f)
        cams = cameras_33()
        # ambient 1: shade = 1 + 0 * c = 1, so at S = 1 the colour byte is the face's albedo rounded
        rgba, _, face = _gpu(m, cams, 33, 33, 1, brute=False, albedo=albedo, ambient=1.0)
        hit = face >= 0
        want = np.floor(albedo[face[hit]] * np.float32(255) + np.float32(0.5)).astype(np.uint8)
        assert hit.any() and np.array_equal(rgba[hit][:, :3], want) and (rgba[hit][:, 3] == 255).all()
        # shaded and supersampled: the restatement, and brute force
        cams2 = cameras_37x29()
        got = _gpu(m, cams2, 37, 29, 3, brute=False, albedo=albedo)
        for a, b in zip(got, _gpu(m, cams2, 37, 29, 3, brute=True, albedo=albedo)):
            assert np.array_equal(a, b)
        for a, b in zip(got, RR.render(v, f, cams2, 37, 29, 3, albedo=albedo)):
            assert np.array_equal(a, b)


def test_argument_checks():
    from disn_amd import mesh_sdf, render
    from disn_amd._lib import DisnError
    v, f = RR.unit_cube()
    m = mesh_sdf.MeshBvh(v, f)
    with pytest.raises(DisnError):
        render.render_views(m, None, None, size=(33, 33), samples=5, cams=cameras_33())
    with pytest.raises(DisnError):
        render.render_views(m, None, None, size=(1025, 33), samples=1, cams=cameras_33())
    with pytest.raises(ValueError):
        render.render_views(m, None, None, size=(33, 33), albedo=np.ones((5, 3), np.float32), cams=cameras_33())


# ---- (e) the rendered mask against the stored camera ---------------------------------------------------------------------
def test_tripod_vertices_land_on_the_device_mask():
    from disn_amd import mesh_sdf, render
    v, f = RR.tripod()
    m = mesh_sdf.MeshBvh(v, f)
    for az, el, d, W, H, S in RR.TRIPOD_VIEWS:
        row = [az, el, 0.0, d, 25.0]
        alpha = render.render_views(m, None, [row], size=(W, H), samples=S)["rgba"][0, ..., 3].cpu().numpy()
        trans_mat = render.view_matrices(row, IDENT, W, H)[2]
        inside, on = RR.vertex_mask_check(v, trans_mat, alpha)
        assert inside >= 0.9 and on == 1.0, (inside, on)
        for img in (alpha[::-1], alpha[:, ::-1]):
            assert RR.vertex_mask_check(v, trans_mat, img)[1] < 1.0


# ---- (f) end to end --------------------------------------------------------------------------------------------------
def _snapshot(root):
    out = {}
    for d, _, files in os.walk(root):
        for fn in files:
            p = os.path.join(d, fn)
            out[p] = os.stat(p).st_mtime_ns
    return out


def test_end_to_end_preprocess_render_load(tmp_path):
    from PIL import Image
    from disn_amd import create_img_h5, data_sdf, isosurface, preprocess
    cat, obj = "03001627", "sphere0"
    v, f = R.icosphere(3, 0.4)                      # the cameras (distance >= 0.65 * 1.75) stay outside it
    v = (v + np.float32([0.05, -0.03, 0.02])).astype(np.float32)
    (tmp_path / "mesh" / cat / obj).mkdir(parents=True)
    isosurface.write_obj(str(tmp_path / "mesh" / cat / obj / "model.obj"), v, f)
    (tmp_path / "lst").mkdir()
    (tmp_path / "lst" / (cat + "_test.lst")).write_text(obj + "\n")
    (tmp_path / "lst" / (cat + "_train.lst")).write_text("")
    dirs = {k: str(tmp_path / k) for k in ("norm_mesh_dir", "sdf_dir", "rendered_dir", "renderedh5_dir")}
    dirs["mesh_dir"] = str(tmp_path / "mesh")
    info = {"lst_dir": str(tmp_path / "lst"), "cats": {"chair": cat}, "all_cats": ["chair"], "raw_dirs_v1": dirs}
    (tmp_path / "info.json").write_text(json.dumps(info))
    preprocess.main(["--info", str(tmp_path / "info.json"), "--category", "chair", "--res", "64"])
    args = ["--info", str(tmp_path / "info.json"), "--render", "--views", "3", "--samples", "2"]
    assert create_img_h5.main(args) == {"objects": 1, "rendered": 3, "written": 3}
    rdir = tmp_path / "rendered_dir" / cat / obj / "rendering"
    assert sorted(os.listdir(rdir)) == ["00.png", "01.png", "02.png", "rendering_metadata.txt", "renderings.txt"]
    assert (rdir / "renderings.txt").read_text().split() == ["00.png", "01.png", "02.png"]
    meta = np.loadtxt(rdir / "rendering_metadata.txt")
    assert meta.shape == (3, 5) and (meta[:, 4] == 25).all()
    assert sorted(os.listdir(tmp_path / "renderedh5_dir" / cat / obj)) == ["00.npz", "01.npz", "02.npz"]
    # a second run writes nothing
    before = (_snapshot(dirs["rendered_dir"]), _snapshot(dirs["renderedh5_dir"]))
    assert create_img_h5.main(args) == {"objects": 1, "rendered": 0, "written": 0}
    assert before == (_snapshot(dirs["rendered_dir"]), _snapshot(dirs["renderedh5_dir"]))
    # the loader's batch: its camera puts the inside samples on the object's pixels
    flags = SimpleNamespace(num_points=16, num_sample_points=2048, batch_size=1, img_h=137, img_w=137, max_epoch=1)
    for num in range(3):
        loader = data_sdf.Pt_sdf_img(flags, listinfo=[(cat, obj, num)], shuffle=False, seed=0,
                                     info={"rendered_dir": dirs["renderedh5_dir"], "sdf_dir": dirs["sdf_dir"]})
        b = loader.get_batch(0)
        z = np.load(tmp_path / "renderedh5_dir" / cat / obj / ("%02d.npz" % num))
        png = np.asarray(Image.open(rdir / ("%02d.png" % num)))
        assert png.shape == (137, 137, 4) and np.array_equal(z["img_arr"], png[:, :, [2, 1, 0, 3]])
        assert np.array_equal(b["img"][0], z["img_arr"][:, :, :3].astype(np.float32) / np.float32(255))
        pts = b["sdf_pt"][0][b["sdf_val"][0, :, 0] < 0]
        assert len(pts) > 100
        inside, on = RR.vertex_mask_check(pts, b["trans_mat"][0], z["img_arr"][:, :, 3])
        assert inside == 1.0 and on == 1.0, (num, inside, on)
        assert 0.05 < (z["img_arr"][:, :, 3] > 0).mean() < 0.9

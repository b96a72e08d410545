"""GPU tests of mesh-to-SDF preprocessing (csrc/mesh_sdf.hip via disn_amd/mesh_sdf.py and disn_amd/preprocess.py):
unsigned distance bit for bit against the float32 restatement and brute force, the sign against the restated rule
and exact inside tests, and the whole preprocessing of a sphere mesh into a tree that the loader and the
evaluation driver read."""
import json
import os
import shutil
import subprocess
import sys
import time
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_sdf_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _soup(seed, n):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-0.8, 0.8, (3 * n, 3)).astype(np.float32)
    f = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    f[n - 1] = f[n - 2]                # duplicated
    v[1] = v[0]                        # degenerate: two equal vertices
    v[5] = v[3] + np.float32(0.5) * (v[4] - v[3])   # nearly collinear
    return v, f


def _meshes():
    v, f = R.icosphere(2, 0.7)
    t, tf = R.torus()
    s, sf = _soup(3, 300)
    return {"icosphere": (v, f), "torus": (t, tf), "soup": (s, sf)}


@pytest.mark.parametrize("name", ["icosphere", "torus", "soup"])
def test_udf_grid_is_bit_exact(name):
    from disn_amd import mesh_sdf
    v, f = _meshes()[name]
    res = 32 if name != "soup" else 16
    axes = mesh_sdf.grid_axes(np.float32([-1, -1, -1, 1, 1, 1]), res)
    m = mesh_sdf.MeshBvh(v, f)
    u = mesh_sdf.unsigned_distance_grid(m, None, axes).cpu().numpy()
    ub = mesh_sdf.unsigned_distance_grid(m, None, axes, brute=True).cpu().numpy()
    ref = R.udf(R.grid_points(axes), v, f)
    assert np.array_equal(u, ub)
    assert np.array_equal(u, ref), np.abs(u - ref).max()


def test_udf_points_bit_exact_and_accurate():
    from disn_amd import mesh_sdf
    rng = np.random.default_rng(0)
    for name, (v, f) in _meshes().items():
        pts = rng.uniform(-1, 1, (3000, 3)).astype(np.float32)
        pts[:100] = v[f[:100, 0]]                     # on vertices
        pts[100:200] = (v[f[:100]].mean(1)).astype(np.float32)   # on faces
        m = mesh_sdf.MeshBvh(v, f)
        u = mesh_sdf.unsigned_distance(m, None, _dev(pts)).cpu().numpy()
        ub = mesh_sdf.unsigned_distance(m, None, _dev(pts), brute=True).cpu().numpy()
        assert np.array_equal(u, ub), name
        assert np.array_equal(u, R.udf(pts, v, f)), name
        err = np.abs(u.astype(np.float64) - R.udf_f64(pts, v, f)).max()
        assert err <= 1e-6, (name, err)


def test_udf_adversarial_near_equidistant():
    """queries at the centre of a fine icosphere: every triangle nearly equidistant, the pruning margin decides"""
    from disn_amd import mesh_sdf
    v, f = R.icosphere(4, 0.5)                        # 5120 triangles
    rng = np.random.default_rng(1)
    pts = (rng.standard_normal((4096, 3)) * 1e-4).astype(np.float32)
    pts[0] = 0
    m = mesh_sdf.MeshBvh(v, f)
    u = mesh_sdf.unsigned_distance(m, None, _dev(pts)).cpu().numpy()
    ub = mesh_sdf.unsigned_distance(m, None, _dev(pts), brute=True).cpu().numpy()
    assert np.array_equal(u, ub)
    assert np.array_equal(u[:256], R.udf(pts[:256], v, f))


def _sign(v, f, res, box=(-1, -1, -1, 1, 1, 1), seal=1.0, offset=0.0):
    from disn_amd import mesh_sdf
    axes = mesh_sdf.grid_axes(np.float32(box), res)
    tau, steps = mesh_sdf.seal_params(axes, seal)
    m = mesh_sdf.MeshBvh(v, f)
    u = mesh_sdf.unsigned_distance_grid(m, None, axes)
    sdf, out = mesh_sdf.sign_grid(m, None, axes, u, tau, steps, offset)
    n = res + 1
    return (axes, tau, steps, u.cpu().numpy().reshape(n, n, n), sdf.cpu().numpy().reshape(n, n, n),
            out.cpu().numpy().reshape(n, n, n).astype(bool))


@pytest.mark.parametrize("name", ["icosphere", "torus", "soup"])
def test_sign_equals_restated_rule(name):
    v, f = _meshes()[name]
    axes, tau, steps, u, sdf, out = _sign(v, f, 24, offset=0.01)
    bits = R.crossing_bits(axes, u, tau, v, f)
    want = R.flood(u, bits, tau, steps)
    assert np.array_equal(out, want)
    assert np.array_equal(sdf, R.signed(u, want, 0.01))


def _check_closed(v, f, res, inside):
    axes, tau, steps, u, sdf, out = _sign(v, f, res)
    pts = R.grid_points(axes).reshape(u.shape + (3,))
    # nodes off the surface (float64 distance > 0; a node on a face may carry an fp32 u of ~1e-8)
    pos = (R.udf_f64(pts.reshape(-1, 3), v, f) > 0).reshape(u.shape)
    assert np.array_equal(out[pos], ~inside(pts[pos])), int((out[pos] == inside(pts[pos])).sum())
    assert (sdf[pos] < 0).any() and (sdf[pos] > 0).any()


def test_sign_closed_meshes_match_exact_inside():
    v, f = R.icosphere(2, 0.7)
    _check_closed(v, f, 32, lambda p: np.abs(R.winding(p, v, f)) > 0.5)
    t, tf = R.torus()
    _check_closed(t, tf, 32, lambda p: np.abs(R.winding(p, t, tf)) > 0.5)
    # faces on node planes (dyadic box, h = 1/8): nodes on the faces have u = 0
    b, bf = R.box([-0.5, -0.25, -0.5], [0.5, 0.5, 0.375])
    _check_closed(b, bf, 16, lambda p: R.inside_exact(p, "box", lo=[-0.5, -0.25, -0.5], hi=[0.5, 0.5, 0.375]))


def test_open_box_has_an_outside_interior():
    v, f = R.box([-0.5, -0.5, -0.5], [0.5, 0.5, 0.5], open_face="+x")
    axes, tau, steps, u, sdf, out = _sign(v, f, 32)
    pts = R.grid_points(axes).reshape(u.shape + (3,))
    interior = np.all(np.abs(pts) < 0.4, axis=-1)
    assert interior.sum() > 100 and out[interior].all() and (sdf[interior] > 0).all()


def test_box_with_narrow_hole_stays_inside():
    v, f = R.box_with_hole([-0.5, -0.5, -0.5], [0.5, 0.5, 0.5], 0.05)
    axes, tau, steps, u, sdf, out = _sign(v, f, 32)
    assert 0.05 < tau
    pts = R.grid_points(axes).reshape(u.shape + (3,))
    interior = np.all(np.abs(pts) < 0.45, axis=-1) & (pts[..., 2] < 0.2)
    assert interior.sum() > 100 and not out[interior].any() and (sdf[interior] < 0).all()
    # the same box with a hole wider than the band: the flood enters
    v2, f2 = R.box_with_hole([-0.5, -0.5, -0.5], [0.5, 0.5, 0.5], 0.5)
    out2 = _sign(v2, f2, 32)[5]
    assert out2[interior].all()


def test_flipped_soup_equals_oriented_twin():
    t, tf = R.torus()
    rng = np.random.default_rng(5)
    flip = rng.random(len(tf)) < 0.5
    tf2 = tf.copy()
    tf2[flip] = tf2[flip][:, [0, 2, 1]]
    tf2 = tf2[rng.permutation(len(tf2))]
    a = _sign(t, tf, 32)
    b = _sign(t, tf2, 32)
    assert np.array_equal(a[5], b[5])
    assert np.abs(a[4] - b[4]).max() <= 1e-6


def _tree(tmp_path, mesh, cat="03001627", obj="sphere0"):
    v, f = mesh
    mesh_dir = tmp_path / "mesh"
    (mesh_dir / cat / obj).mkdir(parents=True)
    from disn_amd import isosurface
    isosurface.write_obj(str(mesh_dir / cat / obj / "model.obj"), v, f)
    lst = tmp_path / "lst"
    lst.mkdir()
    (lst / (cat + "_test.lst")).write_text(obj + "\n")
    (lst / (cat + "_train.lst")).write_text("")
    info = {"lst_dir": str(lst), "cats": {"chair": cat}, "all_cats": ["chair"],
            "raw_dirs_v1": {"mesh_dir": str(mesh_dir), "norm_mesh_dir": str(tmp_path / "norm"),
                            "sdf_dir": str(tmp_path / "sdf")}}
    (tmp_path / "info.json").write_text(json.dumps(info))
    return info


def test_end_to_end_sphere(tmp_path):
    from disn_amd import data_sdf, isosurface, metrics, preprocess
    cat, obj = "03001627", "sphere0"
    v, f = R.icosphere(3, 2.0)
    v = (v + np.float32(0.25)).astype(np.float32)
    info = _tree(tmp_path, (v, f), cat, obj)
    t0 = time.perf_counter()
    preprocess.main(["--info", str(tmp_path / "info.json"), "--category", "chair", "--res", "64"])
    print("one object at res 64: %.3f s" % (time.perf_counter() - t0))
    npz = tmp_path / "sdf" / cat / obj / "ori_sample.npz"
    z = np.load(npz)
    rows = z["pc_sdf_sample"]
    assert rows.shape == (32768, 4) and rows.dtype == np.float32
    assert z["pc_sdf_original"].shape == (1, 3) and not z["pc_sdf_original"].any()
    assert z["norm_params"].shape == (4,) and z["sdf_params"].shape == (6,)
    # the bins of the reference rule on the same grid
    norm_obj = str(tmp_path / "norm" / cat / obj / "pc_norm.obj")
    grid = preprocess.create_one_sdf(64, 1.2, None, norm_obj)
    _, counts = R.sample_sdf(32768, 0.1, 0.003, grid["param"], grid["value"].cpu().numpy(), 64,
                             np.random.default_rng(0))
    dis = rows[:, 3] - np.float32(0.003)
    b = [np.float32(x) for x in (-0.1, -0.1 * 0.3, 0, 0.1 * 0.3, 0.1)]
    got = [int(((dis >= b[i]) & (dis < b[i + 1])).sum()) for i in range(4)]
    assert got == counts and sum(got) == 32768
    # values against the sphere's analytic field: the normalised sphere has radius ~1 about the origin
    r = np.linalg.norm(rows[:, :3].astype(np.float64), axis=1)
    assert np.abs(rows[:, 3] - (r - 1.0)).max() < 0.03
    # the loader reads it
    flags = SimpleNamespace(num_points=16, num_sample_points=64, batch_size=1, img_h=137, img_w=137, max_epoch=1)
    loader = data_sdf.Pt_sdf_img(flags, listinfo=[(cat, obj, 0)], info={"rendered_dir": str(tmp_path / "r"),
                                                                       "sdf_dir": info["raw_dirs_v1"]["sdf_dir"]})
    ori, _, spt, sval, npar, spar = loader.get_sdf_h5(loader.get_sdf_h5_filenm(cat, obj), cat, obj)
    assert spt.shape == (32768, 3) and sval.shape == (32768,) and np.array_equal(spar, z["sdf_params"])
    # isosurf.obj against the normalised input surface
    iso = str(tmp_path / "norm" / cat / obj / "isosurf.obj")
    iv = isosurface.read_obj_verts(iso)
    nv, nf = isosurface.read_obj(norm_obj)
    surf = preprocess.sample_surface(nv, nf, 8192, np.random.default_rng(0)).astype(np.float32)
    d1, _, d2, _ = metrics.nn_distance(_dev(iv[None]), _dev(surf[None]))
    cd = float(d1.mean() + d2.mean())
    print("isosurf.obj vs pc_norm.obj Chamfer (squared, sum of means): %.3g" % cd)
    assert cd < 1e-3
    # the evaluation driver on the produced tree: a copy of isosurf.obj as the prediction of view 0
    cal = tmp_path / "cal" / cat
    cal.mkdir(parents=True)
    shutil.copy(iso, cal / ("%s_%s_00.obj" % (cat, obj)))
    r = subprocess.run([sys.executable, "-m", "disn_amd.evaluate", "cd_emd", "--cal_dir", str(tmp_path / "cal"),
                        "--gt_dir", info["raw_dirs_v1"]["norm_mesh_dir"], "--test_lst_dir", info["lst_dir"],
                        "--category", "chair", "--view_num", "1", "--num_sample_points", str(len(iv))],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("cat_nm:")][0]
    cf = float(line.split("avg_cf:")[1].split(",")[0])
    print(line)
    assert 0 <= cf < 0.5     # both sides sample the same vertices independently: close to, not exactly, 0


def test_scale_res256_100k_triangles():
    from disn_amd import mesh_sdf
    v, f = R.torus(nu=400, nv=128)
    assert len(f) >= 100000
    mesh_sdf.sdf_grid(v, f, 32)                        # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sdf, params = mesh_sdf.sdf_grid(v, f, 256)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("sdf_grid res 256, %d triangles: %.3f s" % (len(f), dt))
    assert sdf.numel() == 257 ** 3 and torch.isfinite(sdf).all()
    assert dt < 120

"""CPU tests of the vertex colours: ``postprocess.zbuffer_arrays`` / ``colour_arrays``, the host functions that ARE the
specification of mesh_colour.hip, checked against geometry; the coloured .obj; ``--colour`` of ``create_sdf``
and ``demo``; the third header of the C ABI.  Bars used below, all the issue's:
  * spheres: no vertex with |cos(normal, view ray)| >= 0.3 is misclassified at S = 2;
  * occluder: every vertex farther than 1.5 image pixels from the front square's projected outline is classified as the
    geometry says, and that band holds at most 15 % of the vertices;
  * ramp: a seen vertex has the ramp's value at its projection to +- 1 of 255 (bilinear interpolation of an affine
    picture is exact up to float32 rounding; the two roundings to integers add less than one step).
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_colour_fixtures as CF  # noqa: E402
import mesh_simplify_fixtures as SF  # noqa: E402
import reconstruct_fixtures as RF  # noqa: E402
from disn_amd import create_sdf as cs  # noqa: E402
from disn_amd import postprocess as P  # noqa: E402

MF = SF.MF
NEW = ("disn_mesh_colour_workspace_bytes", "disn_mesh_zbuffer_batch", "disn_mesh_colour_batch",
       "disn_write_obj_colours")
T0 = CF.pinhole()


@pytest.fixture(scope="module", autouse=True)
def _built():
    from disn_amd.csrc import build
    build.build()


def _c16(rgb):
    return np.rint(np.asarray(rgb, np.float32) * np.float32(65535.0)).astype(np.int64)


def _c8(c16):
    return (np.asarray(c16, np.int64) * 255 + 32767) // 65535


# ------------------------------------------------------------------ visibility against geometry
@pytest.mark.parametrize("nu,nv", [(16, 8), (64, 32), (256, 128)])
def test_sphere_vertices_are_classified_as_their_normals_say(nu, nv):
    v, f = CF.uv_sphere(nu, nv)
    _, cls = P.colour_arrays(v, f, CF.ramp_image()[None], T0[None], S=2)
    normal = v / np.linalg.norm(v, axis=1, keepdims=True)
    ray = CF.camera_centre(T0)[None] - v
    cos = (normal * (ray / np.linalg.norm(ray, axis=1, keepdims=True))).sum(1)
    wrong = (cls == P.CLASS_SEEN) != (cos > 0)
    worst = np.abs(cos[wrong]).max() if wrong.any() else 0.0
    print("sphere %d x %d: %d of %d vertices differ from the sign of cos, the worst at |cos| = %.3f"
          % (nu, nv, wrong.sum(), len(v), worst))
    assert worst < 0.3
    assert (cls[cos > 0.3] == P.CLASS_SEEN).all() and (cls[cos < -0.3] != P.CLASS_SEEN).all()


@pytest.mark.parametrize("cells", [40, 160])
def test_occluder_hides_what_lies_behind_it(cells):
    v, f, n_front = CF.occluder(cells)
    col, cls = P.colour_arrays(v, f, CF.ramp_image()[None], T0[None], bgr=False)
    visible, dist = CF.occluder_truth(v, n_front, T0)
    band = dist <= 1.5
    wrong = (cls == P.CLASS_SEEN) != visible
    print("occluder %d: %.1f %% of the vertices in the band, %d wrong inside it, the farthest wrong one at %.2f px"
          % (cells, 100 * band.mean(), (wrong & band).sum(), dist[wrong].max() if wrong.any() else 0.0))
    assert band.mean() <= 0.15
    assert not (wrong & ~band).any()
    # every seen vertex has the ramp's value at its projection
    u, w_, _ = CF.project(v, T0)
    seen = cls == P.CLASS_SEEN
    want = CF.ramp_value(u, w_) * 255.0
    assert np.abs(col[seen].astype(np.float64) - want[seen]).max() <= 1.0
    if cells == 40:
        # the hidden part is filled from its rim: class 3, inside the range of the coloured vertices it was filled from
        hidden = ~visible & ~band
        assert hidden.sum() > 100 and (cls[hidden] == P.CLASS_FILL).all()
        filled = cls == P.CLASS_FILL
        touches = np.zeros(len(v), bool)
        for k in range(3):
            for m in range(3):
                sel = filled[f[:, k]] & seen[f[:, m]]
                touches[f[sel, m]] = True
        assert touches.any()
        lo, hi = col[touches].min(0), col[touches].max(0)
        assert (col[filled] >= lo).all() and (col[filled] <= hi).all()


# ------------------------------------------------------------------ the means of two views, the fallback, the channels
def _islands():
    """four tiny triangles: at x = -0.6 (view 0 only), 1.2 (view 1 only), 0.6 (both), -1.5 (neither); view 1 is view 0
    with its principal point moved 100 pixels to the left"""
    tri = np.array([[0.0, 0.0, 0.0], [0.01, 0.0, 0.0], [0.0, 0.01, 0.0]], np.float32)
    v = np.concatenate([tri + np.array([x, 0.0, 0.0], np.float32) for x in (-0.6, 1.2, 0.6, -1.5)])
    f = np.arange(12, dtype=np.int32).reshape(4, 3)
    return v, f, np.stack([CF.pinhole(), CF.pinhole(cx=-32.0)])


def test_two_views_take_the_stated_means_and_the_rest_the_mesh_mean():
    v, f, T = _islands()
    a, b = (0.2, 0.4, 0.6), (0.8, 0.45, 0.1)
    img = np.stack([CF.flat_image(a), CF.flat_image(b)])
    col, cls = P.colour_arrays(v, f, img, T, bgr=False)
    assert cls.tolist() == [1] * 9 + [0] * 3
    ca, cb = _c16(a), _c16(b)
    both = (2 * (ca + cb) + 2) // 4                                    # two views, rounded half up
    assert (col[0:3] == _c8(ca)).all() and (col[3:6] == _c8(cb)).all() and (col[6:9] == _c8(both)).all()
    mean = (2 * (3 * ca + 3 * cb + 3 * both) + 9) // 18                 # the nine coloured vertices of the mesh
    assert (col[9:12] == _c8(mean)).all()
    # cv2 order: channels 0 and 2 change places, nothing else moves
    swapped, cls2 = P.colour_arrays(v, f, img, T, bgr=True)
    assert np.array_equal(swapped, col[:, ::-1]) and np.array_equal(cls2, cls)
    assert P.colour_arrays(v, f, img, T)[0].tolist() == swapped.tolist()            # the default
    # nothing coloured at all: mid grey
    grey, cls3 = P.colour_arrays(v[9:], f[:1], img, T)
    assert (grey == 128).all() and (cls3 == 0).all()


def test_a_chain_longer_than_fill_iters_ends_in_the_fallback():
    """the strip's columns i >= 39 project into the image (u = -29.2 + 0.75 i >= -0.5), a round fills one column"""
    v, f = CF.strip(40)
    T = np.stack([CF.pinhole(cx=-29.2)])
    col, cls = P.colour_arrays(v, f, CF.noise_image(3)[None], T, fill_iters=5)
    column = np.arange(len(v)) // 2
    assert (cls[column >= 39] == 1).all() and (cls[(column >= 34) & (column < 39)] == 3).all()
    assert (cls[column < 34] == 0).all()
    assert (cls[column < 39] != 1).all()                               # a vertex that projects outside is unseen
    _, all_filled = P.colour_arrays(v, f, CF.noise_image(3)[None], T, fill_iters=64)
    assert (all_filled[column < 39] == 3).all()
    _, none = P.colour_arrays(v, f, CF.noise_image(3)[None], T, fill_iters=0)
    assert (none[column < 39] == 0).all()


def test_mirror_colours_the_far_side():
    v, f = CF.uv_sphere(32, 16)
    img = CF.noise_image(4)[None]
    plain, cls_plain = P.colour_arrays(v, f, img, T0[None])
    mirrored, cls_mirror = P.colour_arrays(v, f, img, T0[None], mirror_axis=2)
    normal = v / np.linalg.norm(v, axis=1, keepdims=True)
    r = v * np.array([1.0, 1.0, -1.0], np.float32)
    ray = CF.camera_centre(T0)[None] - r
    cos_r = (normal * np.array([1.0, 1.0, -1.0]) * (ray / np.linalg.norm(ray, axis=1, keepdims=True))).sum(1)
    far = (v[:, 2] > 0.1) & (cos_r > 0.3)                   # unseen itself, its reflection plainly seen
    assert far.sum() > 50
    assert (cls_mirror[far] == P.CLASS_MIRROR).all() and (cls_plain[far] == P.CLASS_FILL).all()
    same = cls_plain == P.CLASS_SEEN
    assert np.array_equal(cls_mirror[same], cls_plain[same]) and np.array_equal(mirrored[same], plain[same])
    # a reflected vertex has the colour of the picture at its reflection's projection
    u, w_, _ = CF.project(r, T0)
    near = P._sample16(img[0], u.astype(np.float32), w_.astype(np.float32), True)
    assert np.abs(mirrored[far].astype(np.int64) - _c8(near[far])).max() <= 1


def test_alpha_hides_the_background():
    v, f = CF.uv_sphere(32, 16)
    alpha = np.zeros((1, CF.IMG, CF.IMG), np.uint8)
    alpha[:, :, 68:] = 255                                             # columns u >= 68 are foreground
    _, cls = P.colour_arrays(v, f, CF.noise_image(4)[None], T0[None], alpha=alpha)
    _, cls_plain = P.colour_arrays(v, f, CF.noise_image(4)[None], T0[None])
    u, _, _ = CF.project(v, T0)
    left = np.rint(u) < 68
    assert (cls[left] != 1).all() and (cls_plain[left] == 1).any()
    assert np.array_equal(cls[~left] == 1, cls_plain[~left] == 1)


# ------------------------------------------------------------------ skips, clipping, statuses
def test_skipped_and_clipped_triangles():
    v, f = CF.square(4, 0.3, 0.0)
    base = P.zbuffer_arrays(v, f, T0[None])
    assert base.shape == (1, 274, 274) and base.dtype == np.float32 and (base > 0).sum() > 1000
    assert np.abs(base[base > 0] - 0.5).max() < 1e-3                   # 1 / w at depth 2, the bias of a flat plane is 0
    # a triangle over the whole image with one vertex behind the camera (w = -1), and three collinear vertices
    extra = np.array([[-5, -5, -0.5], [5, -5, -0.5], [0, 5, -3.0], [-1, -1, -0.4], [0, 0, -0.4], [1, 1, -0.4]], np.float32)
    v2 = np.concatenate([v, extra])
    f2 = np.concatenate([f, np.array([[25, 26, 27], [28, 29, 30]], np.int32)])
    assert np.array_equal(P.zbuffer_arrays(v2, f2, T0[None]).view(np.uint32), base.view(np.uint32))
    # partly outside the image: clipped to it, every sub-pixel covered
    quad = P.zbuffer_arrays(*CF.full_quad(), T0[None], S=1)
    assert quad.shape == (1, 137, 137) and (quad > 0).all()
    # an empty mesh, and S outside 1, 2, 4
    assert not P.zbuffer_arrays(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), T0[None]).any()
    col, cls = P.colour_arrays(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), CF.ramp_image()[None], T0[None])
    assert col.shape == (0, 3) and cls.shape == (0,)
    with pytest.raises(ValueError, match="S must be"):
        P.zbuffer_arrays(v, f, T0[None], S=3)


def test_bad_meshes_raise():
    v, f = CF.square(2, 0.3, 0.0)
    bad_f = f.copy()
    bad_f[1, 2] = len(v)
    bad_v = v.copy()
    bad_v[3, 1] = np.nan
    for fn, args in ((P.zbuffer_arrays, (T0[None],)), (P.colour_arrays, (CF.ramp_image()[None], T0[None]))):
        with pytest.raises(ValueError, match="face index out of range"):
            fn(v, bad_f, *args)
        with pytest.raises(ValueError, match="not finite"):
            fn(bad_v, f, *args)
    for kw in ({"mirror_axis": 3}, {"fill_iters": -1}, {"rel_tol": 1.5}, {"S": 8}):
        with pytest.raises(ValueError):
            P.colour_arrays(v, f, CF.ramp_image()[None], T0[None], **kw)


# ------------------------------------------------------------------ the coloured .obj
def test_coloured_obj_round_trip(tmp_path):
    from disn_amd import isosurface, mesh_sdf
    v, f = CF.uv_sphere(16, 8)
    rng = np.random.default_rng(2)
    col = rng.integers(0, 256, size=v.shape, dtype=np.uint8)
    col[:3] = [[0, 0, 0], [255, 255, 255], [1, 128, 254]]
    normals = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    plain, plain_n = str(tmp_path / "plain.obj"), str(tmp_path / "plain_n.obj")
    isosurface.write_obj(plain, v, f)
    isosurface.write_obj(plain_n, v, f, normals)
    for name, n, ref in (("c.obj", None, plain), ("cn.obj", normals, plain_n)):
        path = str(tmp_path / name)
        isosurface.write_obj(path, v, f, n, colours=col)
        assert np.array_equal(isosurface.read_obj_colours(path), col)
        for line, ref_line, c in zip(open(path), open(ref), col):     # the vertex lines: the plain ones + four decimals
            assert line.split()[:4] == ref_line.split() and line.split()[4:] == ["%.4f" % (x / 255.0) for x in c]
        rest = lambda p: [l for l in open(p) if not l.startswith("v ")]
        assert rest(path) == rest(ref)
        for reader in (isosurface.read_obj, mesh_sdf.read_obj_mesh):
            gv, gf = reader(path)
            wv, wf = reader(ref)
            assert np.array_equal(gv, wv) and np.array_equal(gf, wf) and np.array_equal(gv, v)
        assert np.array_equal(isosurface.read_obj_verts(path), isosurface.read_obj_verts(ref))
    with pytest.raises(ValueError, match="without colour"):
        isosurface.read_obj_colours(plain)
    with pytest.raises(ValueError, match="colours must be uint8"):
        isosurface.write_obj(str(tmp_path / "x.obj"), v, f, colours=col.astype(np.float32))
    # without colours the calls take the paths they took: same bytes through either spelling
    again = str(tmp_path / "again.obj")
    isosurface.write_obj(again, v, f, None, None)
    assert open(again, "rb").read() == open(plain, "rb").read()


# ------------------------------------------------------------------ flags, tree, driver
def test_colour_flags_and_tree_name(tmp_path):
    from disn_amd import demo
    base = ["--test_lst_dir", "lists"]
    a = cs.parser().parse_args(base)
    assert a.colour is False and cs.colour_from_flags(a) is None and cs.colour_args(None) is None
    assert cs.colour_args(False) is None
    for flag in ("--colour", "--color"):
        a = cs.parser().parse_args(base + [flag])
        assert cs.colour_from_flags(a) == cs.COLOUR_DEFAULTS == cs.colour_args(True) and cs.check_flags(a) is None
        d = demo.parser().parse_args(["--img", "x.png", flag, "--colour_mirror", "x"])
        assert cs.colour_from_flags(d)["mirror_axis"] == 0
    a = cs.parser().parse_args(base + ["--colour", "--colour_mirror", "z", "--fuse_views", "2", "--view_num", "4"])
    assert cs.colour_from_flags(a)["mirror_axis"] == 2 and cs.check_flags(a) == (2, "max")
    assert cs.colour_args({"mirror_axis": 1, "S": 4})["S"] == 4
    for bad in ({"mirror_axis": "w"}, {"mirror_axis": 3}, {"S": 3}, {"fill_iters": -2}, {"rel_tol": 2.0}, {"shade": 1}):
        with pytest.raises(ValueError):
            cs.colour_args(bad)
    j = os.path.join
    assert cs.result_obj_path("log", 64, 0.0, colour=True) == j("log", "test_objs", "65_0.0_col")
    assert cs.result_obj_path("log", 64, 0.0, clean=True, colour=True) == j("log", "test_objs", "65_0.0_comb_col")
    assert cs.result_obj_path("log", 64, 0.0, simplify=8, colour=True) == j("log", "test_objs", "65_0.0_s8_col")
    assert cs.result_obj_path("log", 64, 0.0, True, (3, "mean"), clean=True, simplify=7, colour=True) == \
        j("log", "test_objs", "camest_fuse3mean_65_0.0_comb_s7_col")
    assert cs.result_obj_path("log", 64, 0.0, clean=True, simplify=7) == j("log", "test_objs", "65_0.0_comb_s7")

    def boom(*a, **k):
        raise AssertionError("device work was reached")

    for bad in (["--colour", "--colour_mirror", "w"], ["--colour", "--colour_mirror", "3"], ["--colour_mirror", "x"]):
        with pytest.raises(ValueError, match="--colour"):
            cs.main(["--test_lst_dir", str(tmp_path / "none"), "--log_dir", str(tmp_path / "log")] + bad,
                    reconstruct_fn=boom)
        with pytest.raises(ValueError, match="--colour"):
            demo.main(["--img", str(tmp_path / "missing.png")] + bad)               # never opened
    assert not os.path.exists(str(tmp_path / "log"))


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_driver_writes_the_col_tree(tmp_path):
    from disn_amd import isosurface
    view_num, seed = 3, 4
    entries = RF.expected_entries(seed, view_num)
    sdf_dir, rendered_dir = RF.build_dataset(str(tmp_path / "data"), entries, n_samples=32)
    lst_dir, log_dir = str(tmp_path / "lst"), str(tmp_path / "log")
    RF.write_lists(lst_dir)
    argv = ["--log_dir", log_dir, "--test_lst_dir", lst_dir, "--sdf_dir", sdf_dir, "--rendered_dir", rendered_dir,
            "--category", "chair,car", "--view_num", str(view_num), "--sdf_res", "8", "--seed", str(seed),
            "--batch_size", "5"]
    v, f = MF.fans()
    col = np.arange(3 * len(v), dtype=np.uint8).reshape(-1, 3) * 9
    normals = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (len(v), 1))
    none = np.zeros((0, 3), np.uint8)

    def fake(extras, empty_extras):
        n = [0]

        def run(imgs, trans_mats, sdf_params):
            out = [MF.empty() + empty_extras if (n[0] + b) == 2 else (v, f) + extras for b in range(imgs.shape[0])]
            n[0] += imgs.shape[0]
            return out
        return run

    plain = cs.main(argv, reconstruct_fn=fake((), ()))
    assert plain == {"written": 12, "skipped": 0, "empty": 1, "out_dir": os.path.join(log_dir, "test_objs", "9_0.0")}
    ref = str(tmp_path / "ref.obj")
    isosurface.write_obj(ref, v, f)
    for rel in _tree(plain["out_dir"]):                                # without the flag: the bytes of the plain writer
        data = open(os.path.join(plain["out_dir"], rel), "rb").read()
        assert data == open(ref, "rb").read() or len(data) == 0
    results = {}
    for flag in ("--colour", "--color"):
        res = cs.main(argv + [flag], reconstruct_fn=fake((col,), (none,)))
        assert res == {"written": 12, "skipped": 0, "empty": 1, "coloured": 11,
                       "out_dir": os.path.join(log_dir, "test_objs", "9_0.0_col")}
        assert _tree(res["out_dir"]) == _tree(plain["out_dir"])
        results[flag] = {rel: open(os.path.join(res["out_dir"], rel), "rb").read() for rel in _tree(res["out_dir"])}
        for rel in _tree(res["out_dir"]):
            path = os.path.join(res["out_dir"], rel)
            lines = [l.split() for l in open(path) if l.startswith("v ")]
            assert all(len(l) == 7 for l in lines)
            if lines:
                assert np.array_equal(isosurface.read_obj_colours(path), col)
                assert np.array_equal(isosurface.read_obj(path)[0], v)
    assert results["--colour"] == results["--color"]
    with_normals = fake((normals, col), (none.astype(np.float32), none))
    res = cs.main(argv + ["--colour", "--normals", "--simplify", "4", "--clean", "all"],
                  reconstruct_fn=lambda i, t, s, select: (with_normals(i, t, s), [False] * i.shape[0]))
    assert res["out_dir"] == os.path.join(log_dir, "test_objs", "9_0.0_comb_s4_col") and res["coloured"] == 11
    for rel in _tree(res["out_dir"]):
        lines = open(os.path.join(res["out_dir"], rel)).read().splitlines()
        assert sum(l.startswith("vn ") for l in lines) in (0, len(v))
        assert all(len(l.split()) == 7 for l in lines if l.startswith("v "))


def test_colour_group_picks_the_meshes_with_vertices(monkeypatch):
    calls = []

    def fake(meshes, imgs, tm, views_per_mesh=1, alpha=None, **kw):
        calls.append((len(meshes), tuple(imgs.shape), tm.shape, views_per_mesh, alpha, kw))
        return [torch.full((m[0].shape[0], 3), 7, dtype=torch.uint8) for m in meshes], None

    import torch
    monkeypatch.setattr(P, "colour_meshes_device", fake)
    t = lambda m: tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in m)
    meshes = [t(MF.fans()), t(MF.empty()), t(MF.fans()) + (torch.zeros(8, 3),)]
    imgs, tm = np.zeros((6, 137, 137, 3), np.float32), np.zeros((6, 4, 3), np.float32)
    out = cs.colour_group(meshes, cs.colour_args(True), imgs, tm, 2)
    assert calls == [(2, (2, 2, 137, 137, 3), (2, 2, 4, 3), 2, None, cs.COLOUR_DEFAULTS)]
    assert [len(m) for m in out] == [3, 3, 4] and out[1][2].shape == (0, 3) and out[1][2].dtype == torch.uint8
    assert (out[0][2] == 7).all() and out[2][2] is meshes[2][2] and out[2][0] is meshes[2][0]
    assert cs.colour_group(meshes, None, imgs, tm, 2) == meshes and len(calls) == 1


# ------------------------------------------------------------------ the third header
def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return re.findall(r"\b(disn_[a-z0-9_]+)\s*\(", text)


def test_third_header_equals_the_third_table_and_the_others_stay():
    from disn_amd import _lib
    assert _declared("disn_amd_colour.h") == list(NEW) == list(_lib.SIGNATURES_COLOUR)
    assert not set(NEW) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_SIMPLIFY))
    assert set(_declared("disn_amd.h")) == set(_lib.SIGNATURES)
    assert _declared("disn_amd_simplify.h") == list(_lib.SIGNATURES_SIMPLIFY)
    header = open(os.path.join(ROOT, "include", "disn_amd.h")).read()
    assert re.search(r"#define DISN_ABI_VERSION 10\b", header) and "zbuffer" not in header
    assert not any(name in header for name in NEW) and "disn_mesh_colour" not in header
    assert _lib.ABI_VERSION == 10 and _lib.lib().disn_abi_version() == 10
    h = _lib.lib()
    for name in NEW:
        fn = getattr(h, name)
        assert fn.restype is _lib.SIGNATURES_COLOUR[name][0] and list(fn.argtypes) == _lib.SIGNATURES_COLOUR[name][1]
    ws = h.disn_mesh_colour_workspace_bytes
    assert ws(24, 1, 100000, 200000, 2) > 24 * 274 * 274 * 4 and ws(1, 1, 0, 0, 1) > 0
    assert ws(1, 2, 10, 10, 4) > ws(1, 1, 10, 10, 4) > ws(1, 1, 10, 10, 2)
    for bad in ((0, 1, 10, 10, 2), (1, 0, 10, 10, 2), (1, 257, 10, 10, 2), (1, 1, 10, 10, 3), (1, 1, 2 ** 31, 10, 2),
                (1, 1, 10, (2 ** 31 - 1) // 3 + 1, 2), (1, 1, -1, 10, 2)):
        assert ws(*bad) == 0, bad
    # argument checks that need no device
    off, bad_off = np.zeros(2, np.int64), np.array([0, -1], np.int64)
    o = off.ctypes.data
    assert h.disn_mesh_zbuffer_batch(None, None, o, o, 1, None, 1, 2, None, None, None, 0, None) == -1
    assert h.disn_mesh_zbuffer_batch(None, None, bad_off.ctypes.data, o, 1, 1, 1, 2, 1, 1, 1, 1 << 30, None) == -1
    assert h.disn_mesh_zbuffer_batch(None, None, o, o, 1, 1, 1, 3, 1, 1, 1, 1 << 30, None) == -2
    assert h.disn_mesh_zbuffer_batch(None, None, o, o, 1, 1, 1, 2, 1, 1, 1, 16, None) == -3
    assert h.disn_mesh_colour_batch(None, None, o, o, 1, None, None, 1, 1, 2, 1e-3, -1, 32, 1, None, None, 1, 1, 1 << 30,
                                    None) == -1
    for S, tol, axis, fill in ((3, 1e-3, -1, 32), (2, 1.0, -1, 32), (2, -0.1, -1, 32), (2, 1e-3, 3, 32),
                               (2, 1e-3, -2, 32), (2, 1e-3, -1, -1), (2, 1e-3, -1, 4097)):
        assert h.disn_mesh_colour_batch(None, None, o, o, 1, 1, None, 1, 1, S, tol, axis, fill, 1, None, None, 1, 1,
                                        1 << 30, None) == -2
    assert h.disn_mesh_colour_batch(None, None, o, o, 1, 1, None, 1, 1, 2, 1e-3, -1, 32, 1, None, None, 1, 1, 16,
                                    None) == -3
    assert h.disn_write_obj_colours(b"/nonexistent/dir/x.obj", None, 0, None, None, None, 0) == -1


def test_third_header_compiles_as_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "disn_amd_colour.h"\n'
                   "int main(void) {\n"
                   "  size_t (*ws)(int, int, int64_t, int64_t, int) = disn_mesh_colour_workspace_bytes;\n"
                   "  int (*wr)(const char*, const float*, int64_t, const uint8_t*, const float*, const int32_t*,\n"
                   "            int64_t) = disn_write_obj_colours;\n"
                   "  return ws == 0 || wr == 0 || DISN_ABI_VERSION != 10 || DISN_COLOUR_IMG != 137;\n"
                   "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I",
                        os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

"""Host side of multi-view reconstruction: the numpy reference against the single-view oracle, the inputs of the
kernel test, the ``--fuse_views`` flag rules, the run grouping and the output path of ``disn_amd.create_sdf``, and the
C ABI names -- no device needed."""
import os
import re

import numpy as np
import pytest

import multiview_reference as MR
import reconstruct_fixtures as RF
from disn_amd import create_sdf as cs
from oracle import disn_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ("disn_gather_taps_pool", "disn_pool_embedding", "disn_query_views_workspace_bytes", "disn_query_views",
             "disn_query_grid_views_workspace_bytes", "disn_query_grid_views")


@pytest.fixture(scope="module")
def two_views():
    """signed taps of the true shapes for two views, their up-sampled maps, two cameras and the kernel test's points"""
    rng = np.random.default_rng(21)
    taps = [rng.standard_normal((2, hw, hw, ch), dtype=np.float32) for hw, ch in ((224, 64), (112, 128), (56, 256),
                                                                                 (28, 512), (14, 512))]
    return MR.view_maps(taps), MR.kernel_cameras()[:2], MR.kernel_points()[0]


@pytest.mark.parametrize("pool", ["max", "mean"])
def test_one_view_is_the_oracles_gather(two_views, pool):
    maps, cams, pts = two_views
    want = O.gather_point_feat(maps[1], O.get_img_points(pts[None], cams[1:2]))[0, :, 0, :]
    assert np.abs(want).max() > 0
    assert np.array_equal(MR.gather_pool(maps[1:2], cams[1:2], pts, pool), want)      # 1.0 * f == f


def test_mean_with_weights_1_0_is_view_0_and_max_is_the_maximum(two_views):
    maps, cams, pts = two_views
    f = MR.gather_views(maps, cams, pts)
    assert np.array_equal(MR.gather_pool(maps, cams, pts, "mean", [1.0, 0.0]), f[0])
    assert np.array_equal(MR.gather_pool(maps, cams, pts, "max"), np.maximum(f[0], f[1]))
    half = MR.gather_pool(maps, cams, pts, "mean")
    assert np.array_equal(half, (np.float32(0.5) * f[0] + np.float32(0.5) * f[1]).astype(np.float32))
    assert (f < 0).any() and not np.array_equal(f[0], f[1])


def test_kernel_inputs_hit_the_cases_they_are_meant_to():
    pts, idx = MR.kernel_points()
    cams = MR.kernel_cameras()
    assert pts.shape == (70, 3) and pts.dtype == np.float32
    xy = np.stack([O.get_img_points(pts[None], cams[v:v + 1])[0] for v in range(3)])
    for v, i in enumerate(idx["integer"]):                     # exactly on an interior pixel of view v
        assert np.array_equal(xy[v, i], np.floor(xy[v, i])) and (xy[v, i] > 0).all() and (xy[v, i] < 136).all()
    for i in idx["clamp"]:                                      # on the clamp in view 0 only
        assert ((xy[0, i] == 0) | (xy[0, i] == 136)).any()
        assert ((xy[1:, i] > 0) & (xy[1:, i] < 136)).all()
    bad = O.get_img_points(pts[None], MR.kernel_cameras(nan_view=1)[1:2])[0]
    assert np.isnan(bad[idx["origin"][0]]).all() and np.isnan(bad).any(axis=1).sum() == 1
    assert np.isfinite(xy).all()


def test_pool_views_rules():
    x = np.array([[1.0, -2.0, 3.0], [0.5, -1.0, 7.0], [-4.0, -3.0, 0.1]], np.float32)
    assert np.array_equal(MR.pool_views(x, "max"), [1.0, -1.0, 7.0])                  # signed: the plain maximum
    w = np.array([0.7, 0.2, 0.1], np.float32)
    want = ((w[0] * x[0]).astype(np.float32) + w[1] * x[1]).astype(np.float32)
    want = (want + w[2] * x[2]).astype(np.float32)
    assert np.array_equal(MR.pool_views(x, "mean", w), want)
    assert MR.default_weights(3)[0] == np.float32(1.0) / np.float32(3.0)
    with pytest.raises(ValueError):
        MR.pool_views(x, "sum")


def test_pool_check_rejects_before_device_work():
    from disn_amd import ops
    assert ops.pool_check("max", 1) == 0 and ops.pool_check("mean", 24, [0.0] * 24) == 1
    for pool, views, weights in (("sum", 2, None), ("max", 0, None), ("max", 25, None), ("mean", 2, [1.0])):
        with pytest.raises(ValueError):
            ops.pool_check(pool, views, weights)


def test_new_names_are_declared_and_bound():
    from disn_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "disn_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(disn_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_NAMES:
        assert name in declared and name in _lib.SIGNATURES, name
    assert re.search(r"#define\s+DISN_ABI_VERSION\s+10\b", hdr) and _lib.ABI_VERSION == 10
    assert re.search(r"#define\s+DISN_POOL_MAX\s+0\b", hdr) and re.search(r"#define\s+DISN_POOL_MEAN\s+1\b", hdr)
    assert re.search(r"#define\s+DISN_MAX_VIEWS\s+24\b", hdr)


# ---- the driver ---------------------------------------------------------------------------------------------------
def test_fuse_args_and_output_path():
    assert cs.fuse_args(0) is None and cs.fuse_args(None) is None
    assert cs.fuse_args(3, "mean") == (3, "mean") and cs.fuse_args(24) == (24, "max")
    for fuse, pool in ((1, "max"), (25, "max"), (-2, "max"), (2, "sum")):
        with pytest.raises(ValueError):
            cs.fuse_args(fuse, pool)
    assert cs.result_obj_path("L", 64, 0.0, fuse=(2, "max")) == os.path.join("L", "test_objs", "fuse2max_65_0.0")
    assert cs.result_obj_path("L", 16, 0.01, cam_est=True, fuse=(3, "mean")) == os.path.join(
        "L", "test_objs", "camest_fuse3mean_17_0.01")
    assert cs.result_obj_path("L", 64, 0.0) == os.path.join("L", "test_objs", "65_0.0")


def test_fuse_runs():
    e = [("c", "o%d" % (i // 4), v) for i, v in enumerate([1, 5, 9, 20, 0, 2, 3, 4])]
    runs = cs.fuse_runs(e, 2)
    assert [len(r) for r in runs] == [2, 2, 2, 2] and runs[1] == [("c", "o0", 9), ("c", "o0", 20)]
    assert [r[0][2] for r in cs.fuse_runs(e, 4)] == [1, 0]
    with pytest.raises(ValueError):
        cs.fuse_runs(e[:7], 2)
    with pytest.raises(ValueError, match="two objects"):
        cs.fuse_runs(e[2:6] + e[:2] + e[6:], 4)[0]


@pytest.mark.parametrize("extra,match", [
    (["--fuse_views", "1"], "normal path"),
    (["--fuse_views", "2", "--view_num", "3"], "view_num"),
    (["--fuse_views", "2", "--view_num", "4", "--batch_size", "3"], "batch_size"),
    (["--fuse_views", "2", "--view_num", "4", "--band", "2"], "--band"),
    (["--fuse_views", "2", "--view_num", "4", "--refine", "1"], "--refine"),
    (["--fuse_views", "2", "--view_num", "4", "--normals"], "--normals"),
    (["--fuse_views", "25", "--view_num", "24"], "2..24"),
])
def test_fuse_flag_errors_come_before_any_work(tmp_path, extra, match):
    with pytest.raises(ValueError, match=match):
        cs.main(["--test_lst_dir", str(tmp_path), "--log_dir", str(tmp_path), "--sdf_res", "8"] + extra)
    assert not os.path.exists(str(tmp_path / "test_objs"))


def test_multi_view_flag_still_raises(tmp_path):
    with pytest.raises(NotImplementedError, match="out of scope"):
        cs.main(["--test_lst_dir", str(tmp_path), "--log_dir", str(tmp_path), "--multi_view", "--fuse_views", "2"])


def _tetra(k):
    t = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    v = np.concatenate([t / np.float32(3.0) + np.float32(k + 0.1 * j) for j in range(3)])
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    return v, np.concatenate([f + 4 * j for j in range(3)]).astype(np.int32)


def test_main_fuses_runs_of_views(tmp_path):
    """4 objects x 4 views, --fuse_views 2: groups of --batch_size views hold whole runs, one mesh per run, named
    after the run's first view, in the fused directory; --skip_existing works on runs"""
    from disn_amd import isosurface
    view_num, seed = 4, 4
    entries = RF.expected_entries(seed, view_num)
    sdf_dir, rendered_dir = RF.build_dataset(str(tmp_path / "data"), entries, n_samples=32)
    lst_dir, log_dir = str(tmp_path / "lst"), str(tmp_path / "log")
    RF.write_lists(lst_dir)
    argv = ["--log_dir", log_dir, "--test_lst_dir", lst_dir, "--sdf_dir", sdf_dir, "--rendered_dir", rendered_dir,
            "--category", "chair,car", "--view_num", str(view_num), "--sdf_res", "8", "--seed", str(seed),
            "--fuse_views", "2", "--fuse_pool", "mean"]
    calls = []

    def fake(imgs, trans_mats, sdf_params):
        assert imgs.shape[0] % 2 == 0 and trans_mats.shape == (imgs.shape[0], 4, 3)
        assert np.array_equal(sdf_params[0::2], sdf_params[1::2])             # a run's views share the object's box
        base = sum(calls) // 2
        calls.append(imgs.shape[0])
        return [_tetra(base + r) for r in range(imgs.shape[0] // 2)]

    res = cs.main(argv + ["--batch_size", "6"], reconstruct_fn=fake)
    assert calls == [6, 6, 4]
    out_dir = os.path.join(log_dir, "test_objs", "fuse2mean_9_0.0")
    assert res == {"written": 8, "skipped": 0, "empty": 0, "out_dir": out_dir}
    heads = entries[0::2]
    for k, e in enumerate(heads):
        v, f = isosurface.read_obj(cs.obj_path(out_dir, *e))
        assert np.array_equal(v, _tetra(k)[0]) and np.array_equal(f, _tetra(k)[1])
    assert len([f for _, _, fs in os.walk(out_dir) for f in fs]) == 8          # nothing under the other views' names
    os.remove(cs.obj_path(out_dir, *heads[5]))
    calls.clear()
    res = cs.main(argv + ["--skip_existing"], reconstruct_fn=fake)
    assert calls == [2] and res["written"] == 1 and res["skipped"] == 14
    assert os.path.isfile(cs.obj_path(out_dir, *heads[5]))

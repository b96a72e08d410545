"""CPU tests of the device small-part cleanup's host side: the --clean flags of ``create_sdf`` and ``demo``, the
result directory, the routing of the listed categories through an injected ``reconstruct_fn``, the C ABI (version,
binding table, header), and the fixtures' condition on the inputs (tests/mesh_clean_fixtures.py)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_clean_fixtures as MF  # noqa: E402
import reconstruct_fixtures as RF  # noqa: E402
from disn_amd import create_sdf as cs  # noqa: E402

NEW = ("disn_mesh_clean_workspace_bytes", "disn_mesh_components_device", "disn_mesh_clean_count_batch",
       "disn_mesh_clean_emit_batch")


@pytest.fixture(scope="module", autouse=True)
def _built():
    from disn_amd.csrc import build
    build.build()


# ------------------------------------------------------------------ flags
def test_clean_flags_parse():
    from disn_amd import demo, evaluate
    base = ["--test_lst_dir", "lists"]
    a = cs.parser().parse_args(base)
    assert a.clean is None and cs.clean_cats_from_flags(a) is None
    a = cs.parser().parse_args(base + ["--clean", "clean"])
    assert cs.clean_cats_from_flags(a) == ((0.5, 0.3, "face"), set(evaluate.CATS_CLEAN.values()))
    a = cs.parser().parse_args(base + ["--clean", "all", "--clean_dist_thresh", "0.7", "--clean_num_thresh", "0.2",
                                       "--clean_connectivity", "vertex"])
    assert cs.clean_cats_from_flags(a) == ((0.7, 0.2, "vertex"), set(evaluate.CATS_ALL.values()))
    a = cs.parser().parse_args(base + ["--clean", "chair,car"])
    assert cs.clean_cats_from_flags(a)[1] == {"03001627", "02958343"}
    d = demo.parser().parse_args(["--img", "x.png"])
    assert d.clean is False and cs.clean_from_flags(d, d.clean) is None
    d = demo.parser().parse_args(["--img", "x.png", "--clean", "--clean_num_thresh", "0.1"])
    assert cs.clean_from_flags(d, d.clean) == (0.5, 0.1, "face")
    # --clean composes with the other mesh options
    a = cs.parser().parse_args(base + ["--clean", "clean", "--band", "4", "--refine", "2", "--normals"])
    assert cs.check_flags(a) is None
    a = cs.parser().parse_args(base + ["--clean", "clean", "--fuse_views", "2", "--view_num", "4"])
    assert cs.check_flags(a) == (2, "max")
    assert cs.clean_args(None) is None and cs.clean_args((1, 0, "face")) == (1.0, 0.0, "face")


def test_clean_flag_errors_come_before_any_work(tmp_path):
    from disn_amd import demo
    base = ["--test_lst_dir", str(tmp_path / "none"), "--log_dir", str(tmp_path / "log")]

    def boom(*a):
        raise AssertionError("device work was reached")

    for extra, match in ((["--clean", "teapot"], "unknown category"),
                         (["--clean", "chair,teapot"], "unknown category"),
                         (["--clean", "all", "--clean_dist_thresh", "-0.1"], "--clean_dist_thresh"),
                         (["--clean", "all", "--clean_num_thresh", "-1"], "--clean_num_thresh"),
                         (["--clean", "all", "--clean_connectivity", "auto"], "--clean_connectivity"),
                         (["--clean_dist_thresh", "0.5"], "needs --clean"),
                         (["--clean_num_thresh", "0.3"], "needs --clean"),
                         (["--clean_connectivity", "face"], "needs --clean")):
        with pytest.raises(ValueError, match=match):
            cs.main(base + extra, reconstruct_fn=boom)
    assert not os.path.exists(str(tmp_path / "log"))
    img = str(tmp_path / "missing.png")                             # never opened: the flags are checked first
    with pytest.raises(ValueError, match="needs --clean"):
        demo.main(["--img", img, "--clean_num_thresh", "0.3"])
    with pytest.raises(ValueError, match="--clean_dist_thresh"):
        demo.main(["--img", img, "--clean", "--clean_dist_thresh", "-1"])
    with pytest.raises(ValueError, match="--clean_connectivity"):
        demo.main(["--img", img, "--clean", "--clean_connectivity", "edge"])


def test_result_obj_path_with_and_without_clean():
    j = os.path.join
    assert cs.result_obj_path("log", 64, 0.0) == j("log", "test_objs", "65_0.0")
    assert cs.result_obj_path("log", 64, 0.0, True) == j("log", "test_objs", "camest_65_0.0")
    assert cs.result_obj_path("log", 16, 0.003, False, (2, "max")) == j("log", "test_objs", "fuse2max_17_0.003")
    assert cs.result_obj_path("log", 64, 0.0, clean=False) == j("log", "test_objs", "65_0.0")
    assert cs.result_obj_path("log", 64, 0.0, clean=True) == j("log", "test_objs", "65_0.0_comb")
    assert cs.result_obj_path("log", 64, 0.0, True, (3, "mean"), clean=True) == \
        j("log", "test_objs", "camest_fuse3mean_65_0.0_comb")


# ------------------------------------------------------------------ the driver around an injected reconstruct_fn
def _tetra(k):
    t = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    return t / np.float32(3.0) + np.float32(k), f


def test_only_listed_categories_are_routed_to_cleaning(tmp_path):
    from disn_amd import isosurface
    view_num, seed = 3, 4
    entries = RF.expected_entries(seed, view_num)                   # chairs (03001627), then cars (02958343)
    sdf_dir, rendered_dir = RF.build_dataset(str(tmp_path / "data"), entries, n_samples=32)
    lst_dir, log_dir = str(tmp_path / "lst"), str(tmp_path / "log")
    RF.write_lists(lst_dir)
    argv = ["--log_dir", log_dir, "--test_lst_dir", lst_dir, "--sdf_dir", sdf_dir, "--rendered_dir", rendered_dir,
            "--category", "chair,car", "--view_num", str(view_num), "--sdf_res", "8", "--seed", str(seed),
            "--batch_size", "5"]
    seen = []

    def fake(imgs, trans_mats, sdf_params, select):
        base = len(seen)
        assert len(select) == imgs.shape[0]
        seen.extend(select)
        # a "cleaned" mesh is marked by a shift of 100; of every second selected mesh nothing is kept
        left = [bool(s) and (base + b) % 2 == 1 for b, s in enumerate(select)]
        meshes = []
        for b, s in enumerate(select):
            v, f = _tetra(base + b)
            meshes.append((v + np.float32(100.0) if s and not left[b] else v, f))
        return meshes, left

    res = cs.main(argv + ["--clean", "car"], reconstruct_fn=fake)
    assert seen == [e[0] == "02958343" for e in entries]            # a group of 5 mixes the categories
    assert seen[4:7] == [False, False, True]
    out_dir = os.path.join(log_dir, "test_objs", "9_0.0_comb")
    n_left = sum(1 for k, s in enumerate(seen) if s and k % 2 == 1)
    assert n_left == 3
    assert res == {"written": 12, "skipped": 0, "empty": 0, "unclean": n_left, "out_dir": out_dir}
    for k, e in enumerate(entries):
        v, _ = isosurface.read_obj(cs.obj_path(out_dir, *e))
        shift = 100.0 if seen[k] and k % 2 == 0 else 0.0
        assert np.array_equal(v, _tetra(k)[0] + np.float32(shift)), k
    log = open(os.path.join(log_dir, "log_test.txt")).read()
    assert log.count("UNCLEAN") == n_left
    # without --clean: the three-argument call, the old directory, no "unclean" key
    res = cs.main(argv, reconstruct_fn=lambda i, t, s: [_tetra(b) for b in range(i.shape[0])])
    assert res == {"written": 12, "skipped": 0, "empty": 0, "out_dir": os.path.join(log_dir, "test_objs", "9_0.0")}


def test_clean_group_selects_and_marks(monkeypatch):
    from disn_amd import postprocess
    calls = []

    def fake(meshes, dist_thresh, num_thresh, connectivity, strict=True):
        calls.append((len(meshes), dist_thresh, num_thresh, connectivity, strict))
        return [None if k == 1 else (m[0] + 1, m[1]) for k, m in enumerate(meshes)], [None] * len(meshes)

    monkeypatch.setattr(postprocess, "clean_meshes_device", fake)
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    meshes = [_tetra(0), _tetra(1), empty, _tetra(3), _tetra(4)]
    out, unclean = cs.clean_group(meshes, (0.5, 0.3, "face"), [True, False, True, True, True], strict=False)
    assert calls == [(3, 0.5, 0.3, "face", False)]                  # meshes 0, 3, 4: 1 is not listed, 2 has no triangle
    assert unclean == [False, False, False, True, False]
    assert np.array_equal(out[0][0], meshes[0][0] + 1) and np.array_equal(out[4][0], meshes[4][0] + 1)
    assert out[1] is meshes[1] and out[2] is meshes[2] and out[3] is meshes[3]
    out, unclean = cs.clean_group(meshes, None)
    assert len(calls) == 1 and out == meshes and not any(unclean)


# ------------------------------------------------------------------ the C ABI
def test_abi_stays_10_and_the_new_symbols_are_bound_and_declared():
    from disn_amd import _lib
    assert _lib.ABI_VERSION == 10 and _lib.lib().disn_abi_version() == 10
    header = open(os.path.join(ROOT, "include", "disn_amd.h")).read()
    assert re.search(r"#define DISN_ABI_VERSION 10\b", header)
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
        assert re.search(r"\b%s\(" % name, header), name
    assert list(_lib.SIGNATURES)[-4:] == list(NEW)                   # appended, like every later entry
    h = _lib.lib()
    assert h.disn_mesh_clean_workspace_bytes(24, 100000, 200000) > 0
    assert h.disn_mesh_clean_workspace_bytes(1, 0, 0) > 0           # an empty batch is a supported one
    assert h.disn_mesh_clean_workspace_bytes(0, 10, 10) == 0
    assert h.disn_mesh_clean_workspace_bytes(1, 10, (2 ** 31 - 1) // 3 + 1) == 0
    assert h.disn_mesh_clean_workspace_bytes(1, 2 ** 31, 10) == 0
    # argument checks that need no device
    off = np.zeros(2, np.int64)
    assert h.disn_mesh_clean_count_batch(None, None, off.ctypes.data, off.ctypes.data, 1, 2, 0.5, 0.3, None, None, 0,
                                         None) == -1
    bad = np.array([0, -1], np.int64)
    assert h.disn_mesh_clean_emit_batch(None, None, bad.ctypes.data, off.ctypes.data, off.ctypes.data, 1, None, None,
                                        None, None, None, 0, None) == -1


def test_header_still_compiles_as_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "disn_amd.h"\n'
                   "int main(void) {\n"
                   "  size_t (*ws)(int, int64_t, int64_t) = disn_mesh_clean_workspace_bytes;\n"
                   "  int (*count)(const float*, const int32_t*, const int64_t*, const int64_t*, int, int, double, double,\n"
                   "               int64_t*, void*, size_t, void*) = disn_mesh_clean_count_batch;\n"
                   "  return ws == 0 || count == 0;\n"
                   "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I",
                        os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------ the condition on the inputs
def test_fixtures_keep_their_distance_from_the_thresholds():
    """what tests/test_gpu_mesh_clean.py compares bit for bit: every part's centroid distance at least 1e-6 from
    dist_thresh, every count different from biggest * num_thresh (host functions only)"""
    from oracle import mc_oracle as M
    for conn in ("face", "vertex"):
        MF.assert_margins(*MF.fans(), 0.5, 0.3, conn)
    for num in (0.0, 0.3):
        MF.assert_margins(*MF.crowd(), 0.5, num)
        for v, f in MF.batch_of_five():
            MF.assert_margins(v, f, 0.5, num)
    v, f = MF.two_spheres()
    for shift, dist, num, expect in MF.RULE_CASES:
        got = MF.host_clean(v + np.float32(shift), f, dist, num)
        assert (got is None) == (expect is None) and (got is None or got[2] == expect)
    counts, d = MF.part_distances(*MF.crowd())
    assert counts.size == 5001 and counts.max() == 162 and (d < 0.5 - 1e-6).all()
    assert MF.part_distances(*MF.strip())[0].tolist() == [4098]
    for k in range(3):                                              # the marching-cubes meshes, on the CPU oracle
        vol, box = MF.field_grid(16, k)
        mv, mf = M.marching_cubes(vol, box, 0.0)
        counts, d = MF.part_distances(mv, mf)
        assert counts.size >= 2 and (d > 0.5 + 1e-6).sum() >= 1 and (d < 0.5 - 1e-6).sum() >= 1, (k, counts, d)
        MF.assert_margins(mv, mf, 0.5, 0.3)
        assert len(MF.host_clean(mv, mf)[2]) < counts.size

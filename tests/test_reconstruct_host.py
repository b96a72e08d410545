"""Host side of the reconstruction drivers (``disn_amd.create_sdf``, ``disn_amd.demo``): the sample list, groups,
shards, ``--skip_existing``, output paths, flag checks, the checkpoint rule, the demo image reader and the writer
pool -- no device needed (``main`` takes the device work as a callable)."""
import os
import random

import numpy as np
import pytest

import reconstruct_fixtures as RF
from disn_amd import create_sdf as cs
from disn_amd.evaluate import CATS_ALL


def _lists(tmp_path, objs):
    d = str(tmp_path / "lst")
    os.makedirs(d, exist_ok=True)
    for cat_id, names in objs.items():
        with open(os.path.join(d, cat_id + "_test.lst"), "w") as f:
            f.write("\n".join(names) + "\n")
    return d


def test_sample_list_order_views_and_seed(tmp_path):
    objs = {"02958343": ["c1", "c2"], "03001627": ["a1", "a2", "a3"], "04530566": ["w1"]}
    d = _lists(tmp_path, objs)
    cats = {nm: CATS_ALL[nm] for nm in ("car", "chair", "watercraft")}      # dict order must not matter
    got = cs.sample_list(cats, d, view_num=5, seed=7)
    rng = random.Random(7)
    want = []
    for cat_id, names in (("04530566", ["w1"]), ("03001627", ["a1", "a2", "a3"]), ("02958343", ["c1", "c2"])):
        for o in names:                                    # CATS_ALL order: watercraft, ..., chair, ..., car
            want += [(cat_id, o, v) for v in sorted(rng.sample(range(24), 5))]
    assert got == want and len(got) == 30
    assert got == cs.sample_list(dict(reversed(list(cats.items()))), d, view_num=5, seed=7)
    assert got == cs.sample_list(cats, d, view_num=5, seed=7)               # a seed reproduces the choice
    assert got != cs.sample_list(cats, d, view_num=5, seed=8)
    full = cs.sample_list(cats, d, view_num=24, seed=3)
    assert len(full) == 6 * 24
    for k in range(6):
        assert [v for _, _, v in full[24 * k:24 * k + 24]] == list(range(24))
    with pytest.raises(ValueError):
        cs.sample_list(cats, d, view_num=25)
    assert got == RF.expected_entries(7, 5, cats=(("watercraft", "04530566"), ("chair", "03001627"),
                                                  ("car", "02958343")), objs=objs)


def test_groups_keep_the_tail():
    e = [("c", "o%d" % (i // 3), i % 3) for i in range(10)]
    g = cs.groups(e, 4)
    assert [len(x) for x in g] == [4, 4, 2]
    assert [x for grp in g for x in grp] == e
    assert cs.groups(e, 10) == [e] and cs.groups(e, 24) == [e] and cs.groups([], 4) == []
    assert [len(x) for x in cs.groups(e, 1)] == [1] * 10
    with pytest.raises(ValueError):
        cs.groups(e, 0)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_shards_partition_objects(tmp_path, n):
    objs = {"03001627": ["o%d" % i for i in range(4)], "02958343": ["p%d" % i for i in range(3)]}   # 7 objects
    d = _lists(tmp_path, objs)
    cats = {"chair": CATS_ALL["chair"], "car": CATS_ALL["car"]}
    whole = cs.sample_list(cats, d, view_num=3, seed=1)
    parts = [cs.sample_list(cats, d, view_num=3, seed=1, num_shards=n, shard_id=i) for i in range(n)]
    assert sorted(x for p in parts for x in p) == sorted(whole)             # exhaustive, same views
    assert sum(len(p) for p in parts) == len(whole) == 21                   # disjoint
    for p in parts:
        per_obj = {}
        for c, o, v in p:
            per_obj.setdefault((c, o), []).append(v)
        assert all(len(v) == 3 for v in per_obj.values())                   # an object's views stay together
    owners = [{(c, o) for c, o, _ in p} for p in parts]
    assert sum(len(s) for s in owners) == 7
    with pytest.raises(ValueError):
        cs.sample_list(cats, d, view_num=3, num_shards=n, shard_id=n)


def test_skip_existing_uses_the_200_byte_rule(tmp_path):
    out = str(tmp_path / "out")
    e = [("03001627", "a", 0), ("03001627", "a", 1), ("03001627", "a", 2), ("03001627", "b", 5)]
    for ent, size in zip(e, (201, 200, 0)):
        p = cs.obj_path(out, *ent)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "wb") as f:
            f.write(b"v" * size)
    assert cs.pending(e, out) == e[1:]                                      # > 200 bytes: done; 200, 0, missing: to do
    assert cs.MIN_OBJ_BYTES == 200


def test_output_paths():
    assert cs.result_obj_path("L", 64, 0.0) == os.path.join("L", "test_objs", "65_0.0")
    assert cs.result_obj_path("L", 64, 0.0, cam_est=True) == os.path.join("L", "test_objs", "camest_65_0.0")
    assert cs.result_obj_path("L", 256, 0.003) == os.path.join("L", "test_objs", "257_0.003")
    assert cs.obj_path("D", "03001627", "abc", 3) == os.path.join("D", "03001627", "03001627_abc_03.obj")
    assert cs.parser().parse_args(["--test_lst_dir", "x"]).batch_size is None   # -> view_num


@pytest.mark.parametrize("flag", ["--binary", "--threedcnn", "--img_feat_onestream", "--multi_view", "--alpha"])
def test_unsupported_flags_raise(tmp_path, flag):
    with pytest.raises(NotImplementedError, match="out of scope"):
        cs.main(["--test_lst_dir", str(tmp_path), "--log_dir", str(tmp_path), flag])
    assert not os.path.exists(str(tmp_path / "test_objs"))


def test_writers_bound(tmp_path):
    with pytest.raises(ValueError):
        cs.main(["--test_lst_dir", str(tmp_path), "--log_dir", str(tmp_path), "--writers", "17"])


def test_missing_checkpoint_raises_before_device_work(tmp_path, monkeypatch):
    import disn_amd.engine as engine
    d = _lists(tmp_path, {"03001627": ["a"]})

    def no_engine(*a, **k):
        raise AssertionError("the engine was built before the checkpoint was checked")
    monkeypatch.setattr(engine, "SdfEngine", no_engine)
    log_dir = str(tmp_path / "ckpt")
    with pytest.raises(FileNotFoundError, match="--random_init"):
        cs.main(["--test_lst_dir", d, "--log_dir", log_dir, "--category", "chair", "--view_num", "2"])
    os.makedirs(log_dir)
    with pytest.raises(FileNotFoundError, match="--random_init"):
        cs.main(["--test_lst_dir", d, "--log_dir", log_dir, "--category", "chair", "--view_num", "2"])
    from disn_amd import demo
    from PIL import Image
    png = str(tmp_path / "v.png")
    Image.fromarray(np.zeros((137, 137, 4), np.uint8), "RGBA").save(png)
    with pytest.raises(FileNotFoundError, match="--random_init"):
        demo.main(["--img", png, "--log_dir", log_dir, "--out", str(tmp_path / "o.obj")])


def test_demo_image_reader_equals_the_oracle(tmp_path):
    from PIL import Image
    from disn_amd import demo
    from oracle import disn_oracle as O
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, size=(137, 137, 4), dtype=np.uint8)
    png = str(tmp_path / "view.png")
    Image.fromarray(a, "RGBA").save(png)
    got = demo.read_image(png)
    assert got.dtype == np.float32 and got.shape == (1, 137, 137, 3)
    assert np.array_equal(got, O.load_demo_image(png))
    assert np.array_equal(got[0], a[:, :, [2, 1, 0]].astype(np.float32) / np.float32(255.0))
    assert np.array_equal(demo.DEMO_TRANS_MAT, O.DEMO_TRANS_MAT)


def _driver_inputs(tmp_path, view_num=3, seed=4):
    entries = RF.expected_entries(seed, view_num)
    sdf_dir, rendered_dir = RF.build_dataset(str(tmp_path / "data"), entries, n_samples=32)
    lst_dir = str(tmp_path / "lst")
    RF.write_lists(lst_dir)
    log_dir = str(tmp_path / "log")
    argv = ["--log_dir", log_dir, "--test_lst_dir", lst_dir, "--sdf_dir", sdf_dir, "--rendered_dir", rendered_dir,
            "--category", "chair,car", "--view_num", str(view_num), "--sdf_res", "8", "--seed", str(seed)]
    return entries, argv, log_dir


def _tetra(k):
    """three tetrahedra with float32 coordinates that need all nine digits (a file of more than 200 bytes)"""
    t = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    v = np.concatenate([t / np.float32(3.0) + np.float32(k + 0.1 * j) for j in range(3)])
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    return v, np.concatenate([f + 4 * j for j in range(3)]).astype(np.int32)


def test_main_with_injected_reconstruct(tmp_path):
    """the driver around the device work: groups (with the tail), loader batches, paths, empty meshes, the log"""
    from disn_amd import isosurface
    entries, argv, log_dir = _driver_inputs(tmp_path)
    calls = []

    def fake(imgs, trans_mats, sdf_params):
        assert imgs.shape[1:] == (137, 137, 3) and trans_mats.shape[1:] == (4, 3) and sdf_params.shape[1:] == (6,)
        assert imgs.dtype == np.float32 and 0.0 <= imgs.min() and imgs.max() <= 1.0
        base = sum(calls)
        calls.append(imgs.shape[0])
        return [(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)) if base + b == 7 else _tetra(base + b)
                for b in range(imgs.shape[0])]

    res = cs.main(argv + ["--batch_size", "5"], reconstruct_fn=fake)
    assert calls == [5, 5, 2]                                               # the tail group is kept
    out_dir = os.path.join(log_dir, "test_objs", "9_0.0")
    assert res == {"written": 12, "skipped": 0, "empty": 1, "out_dir": out_dir}
    for k, e in enumerate(entries):
        p = cs.obj_path(out_dir, *e)
        v, f = isosurface.read_obj(p)
        if k == 7:
            assert os.stat(p).st_size == 0                                  # an empty mesh is written, not skipped
        else:
            assert np.array_equal(v, _tetra(k)[0]) and np.array_equal(f, _tetra(k)[1])
    log = open(os.path.join(log_dir, "log_test.txt")).read()
    assert "EMPTY" in log and "12 written (1 empty)" in log
    calls.clear()
    res = cs.main(argv + ["--batch_size", "5", "--skip_existing"], reconstruct_fn=fake)
    assert calls == [1] and res["written"] == 1 and res["skipped"] == 11    # only the empty one (0 bytes) is redone
    res = cs.main(argv + ["--cam_est", "--num_shards", "2", "--shard_id", "1"], reconstruct_fn=fake)
    assert res["out_dir"] == os.path.join(log_dir, "test_objs", "camest_9_0.0") and res["written"] == 6


def test_writer_exception_fails_the_run(tmp_path, monkeypatch):
    from disn_amd import isosurface
    entries, argv, log_dir = _driver_inputs(tmp_path)
    real = isosurface.write_obj
    bad = cs.obj_path(os.path.join(log_dir, "test_objs", "9_0.0"), *entries[-1])      # in the LAST group

    def write_obj(path, verts, faces):
        if path == bad:
            raise OSError("disk full: %s" % path)
        real(path, verts, faces)
    monkeypatch.setattr(isosurface, "write_obj", write_obj)
    with pytest.raises(OSError, match="disk full"):
        cs.main(argv, reconstruct_fn=lambda i, t, s: [_tetra(b) for b in range(i.shape[0])])
    assert len([f for _, _, fs in os.walk(os.path.join(log_dir, "test_objs")) for f in fs]) == 11
    # ... and in a group that is not the last
    bad = cs.obj_path(os.path.join(log_dir, "test_objs", "9_0.0"), *entries[0])
    with pytest.raises(OSError, match="disk full"):
        cs.main(argv, reconstruct_fn=lambda i, t, s: [_tetra(b) for b in range(i.shape[0])])


def test_mc_batch_fixtures_have_surfaces():
    """the grids of tests/test_gpu_reconstruct.py, on the CPU oracle: every non-empty fixture has triangles at both
    iso levels, the empty one none, and the 'last plane' sphere has cut edges ON the planes ix = R and iz = R"""
    from oracle import mc_oracle as M
    fx = RF.mc_batch_grids(20)
    assert [f[3] for f in fx] == [False, False, True, False, False, False]
    for iso in (0.0, 0.07):
        for name, vol, box, empty in fx:
            v, f = M.marching_cubes(vol, box, iso)
            assert (len(f) == 0) == empty and (len(v) == 0) == empty, (name, iso)
    name, vol, box, _ = fx[4]
    v, _ = M.marching_cubes(vol, box, 0.0)
    assert np.any(v[:, 0] == np.float32(box[3])) and np.any(v[:, 2] == np.float32(box[5]))


def test_batch_workspace_bytes_bounds():
    """host-only entry: 0 for an unsupported batch"""
    from disn_amd._lib import ABI_VERSION, lib
    h = lib()
    assert ABI_VERSION == 10 and h.disn_abi_version() == 10
    assert h.disn_mc_batch_workspace_bytes(0, 64) == 0 and h.disn_mc_batch_workspace_bytes(-1, 64) == 0
    assert h.disn_mc_batch_workspace_bytes(1, 0) == 0 and h.disn_mc_batch_workspace_bytes(1, 1291) == 0
    per = 3 * 65 ** 3
    big = -(-(1 << 32) // per)
    assert h.disn_mc_batch_workspace_bytes(big, 64) == 0 and h.disn_mc_batch_workspace_bytes(big - 1, 64) > 0
    assert h.disn_mc_batch_workspace_bytes(24, 64) >= 24 * (2 * per + 2 * 64 ** 3) * 4

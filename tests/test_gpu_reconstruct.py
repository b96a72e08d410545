"""Batched meshing (disn_mc_count_batch / disn_mc_emit_batch), ``create_sdf.reconstruct`` and the drivers built on
them (``python -m disn_amd.create_sdf``, ``python -m disn_amd.demo``, ``python -m disn_amd.evaluate sdf_acc``) on
the device.  Meshes are compared bit for bit: with the CPU oracle, with the single-grid kernels, and -- for the
drivers -- with ``reconstruct`` on the same inputs, regrouped by the documented rule."""
import os
import shutil

import numpy as np
import pytest
import torch

import reconstruct_fixtures as RF
from oracle import disn_oracle as O
from oracle import mc_oracle as M

pytestmark = pytest.mark.gpu


def _host(mesh):
    return mesh[0].cpu().numpy(), mesh[1].cpu().numpy()


def _same(a, b):
    return a[0].shape == b[0].shape and a[1].shape == b[1].shape and np.array_equal(a[1], b[1]) \
        and np.array_equal(a[0], b[0])


def _stack(vols):
    return torch.from_numpy(np.stack([v.reshape(-1) for v in vols])).cuda()


# ------------------------------------------------------------------ 1. batched meshing, bit exact
@pytest.mark.parametrize("iso", [0.0, 0.07])
def test_batch_equals_oracle_and_single_grid(iso):
    from disn_amd import isosurface
    R = 20
    fx = RF.mc_batch_grids(R)
    sdf, boxes = _stack([f[1] for f in fx]), np.asarray([f[2] for f in fx], np.float64)
    got = isosurface.marching_cubes_batch(sdf, boxes, R, iso)
    assert len(got) == 6
    for b, (name, vol, box, empty) in enumerate(fx):
        vr, fr = M.marching_cubes(vol, box, iso)
        single = _host(isosurface.marching_cubes(sdf[b], box, R, iso))
        mine = _host(got[b])
        assert (len(fr) == 0) == empty, name                       # every non-empty fixture HAS a surface
        assert mine[0].dtype == np.float32 and mine[1].dtype == np.int32
        assert _same(mine, (vr, fr)), "%s (grid %d, iso %g) differs from the oracle" % (name, b, iso)
        assert _same(mine, single), "%s (grid %d, iso %g) differs from the single-grid kernels" % (name, b, iso)
        if empty:
            assert mine[0].shape == (0, 3) and mine[1].shape == (0, 3)
    # B = 1: every grid alone through the batch entry
    for b in (1, 2, 4):
        one = _host(isosurface.marching_cubes_batch(sdf[b:b + 1], boxes[b:b + 1], R, iso)[0])
        assert _same(one, _host(got[b]))


def test_batch_r64_b24_equals_single_grid():
    """the production shape: 24 views at --sdf_res 64"""
    from disn_amd import isosurface
    R, B = 64, 24
    vols = [RF.noise(R, 100 + b) if b % 3 == 0 else RF.sphere(R, 0.3 + 0.02 * b, (0.02 * b - 0.2, 0.1, -0.01 * b))
            for b in range(B)]
    vols[5] = np.ones((R + 1,) * 3, np.float32)
    boxes = np.asarray([[-1.0, -1.0 - 0.01 * b, -1.0, 1.0 + 0.02 * b, 1.0, 1.0] for b in range(B)], np.float64)
    sdf = _stack(vols)
    got = isosurface.marching_cubes_batch(sdf, boxes, R, 0.01)
    nonempty = 0
    for b in range(B):
        single = _host(isosurface.marching_cubes(sdf[b], boxes[b], R, 0.01))
        assert _same(_host(got[b]), single), "grid %d" % b
        nonempty += len(single[1]) > 0
    assert len(got[5][0]) == 0 and len(got[5][1]) == 0 and nonempty == B - 1


def test_batch_of_33_grids_crosses_the_32_box_launch_in_all_three_meshers():
    """The boxes of a batch travel as kernel arguments, 32 grids per launch: 33 grids with 33 different boxes put one
    grid into a second launch of the edge-point, grid-normals and vertex kernels.  Every grid bit for bit the host
    specification's, and grids 31, 32 and 0 the same grid meshed alone."""
    import dual_contour_fixtures as F
    from disn_amd import isosurface
    R, B = 3, 33
    fx = [F.noise(R, seed=b, box=F.UNIT * (0.5 + 0.01 * b)) for b in range(B)]
    sdf, boxes = _stack([f[0] for f in fx]), np.asarray([f[1] for f in fx], np.float64)
    mc = isosurface.marching_cubes_batch(sdf, boxes, R, 0.0)
    dc = isosurface.dual_contour_batch(sdf, boxes, R, 0.0, None)
    dcs = isosurface.dual_contour_batch(sdf, boxes, R, 0.0, None, sheets=True)
    assert len(mc) == len(dc) == len(dcs) == B
    for b, (vol, box, iso, _) in enumerate(fx):
        nrm = isosurface.grid_normals_arrays(vol, box, iso)
        want = {"mc": M.marching_cubes(vol.reshape((R + 1,) * 3), box, iso),
                "dc": isosurface.dual_contour_arrays(vol, box, iso, nrm),
                "dcs": isosurface.dual_contour_sheets_arrays(vol, box, iso, nrm)}
        # no case can drop out silently: every grid has a surface under every mesher, and cells of several sheets
        assert len(nrm) >= 59 and all(len(v) and len(f) for v, f in want.values()), b
        assert len(want["mc"][0]) == len(nrm) and len(want["dc"][0]) != len(want["dcs"][0]), b
        for name, got in (("mc", mc[b]), ("dc", dc[b]), ("dcs", dcs[b])):
            assert _same(_host(got), want[name]), "%s: grid %d differs from the host specification" % (name, b)
    for b in (31, 32, 0):
        one = slice(b, b + 1)
        assert _same(_host(isosurface.marching_cubes_batch(sdf[one], boxes[one], R, 0.0)[0]), _host(mc[b])), b
        assert _same(_host(isosurface.marching_cubes(sdf[b], boxes[b], R, 0.0)), _host(mc[b])), b
        assert _same(_host(isosurface.dual_contour(sdf[b], boxes[b], R, 0.0)), _host(dc[b])), b
        assert _same(_host(isosurface.dual_contour(sdf[b], boxes[b], R, 0.0, sheets=True)), _host(dcs[b])), b


# ------------------------------------------------------------------ 2. workspace bounds, split batches
def test_workspace_bounds_and_split():
    from disn_amd import isosurface
    from disn_amd._lib import lib
    h = lib()
    assert h.disn_mc_batch_workspace_bytes(0, 20) == 0
    assert h.disn_mc_batch_workspace_bytes(1, 0) == 0
    per = 3 * 65 ** 3
    big = -(-(1 << 32) // per)                                     # the first B with B*3*65^3 >= 2^32
    assert big * per >= 1 << 32 > (big - 1) * per
    assert h.disn_mc_batch_workspace_bytes(big, 64) == 0
    assert h.disn_mc_batch_workspace_bytes(big - 1, 64) > 0
    assert h.disn_mc_batch_workspace_bytes(1, 20) >= h.disn_mc_workspace_bytes(20)
    R = 20
    fx = RF.mc_batch_grids(R)
    sdf, boxes = _stack([f[1] for f in fx]), np.asarray([f[2] for f in fx], np.float64)
    whole = isosurface.marching_cubes_batch(sdf, boxes, R, 0.0)
    for grids_per_round in (1, 2, 4):                              # 6 grids in rounds of 1, 2 and 4 + 2
        part = isosurface.marching_cubes_batch(sdf, boxes, R, 0.0,
                                               max_edge_slots=grids_per_round * 3 * (R + 1) ** 3 + 1)
        assert len(part) == 6
        for b in range(6):
            assert _same(_host(part[b]), _host(whole[b])), (grids_per_round, b)
    with pytest.raises(ValueError):
        isosurface.marching_cubes_batch(sdf, boxes, R, 0.0, max_edge_slots=3 * (R + 1) ** 3)    # not one grid fits
    with pytest.raises(ValueError):
        isosurface.marching_cubes_batch(sdf, boxes[:5], R, 0.0)


# ------------------------------------------------------------------ 3. reconstruct == the existing path
def _five_views():
    feed = O.synth_inputs(21, 5, 8)
    imgs = feed["imgs"] * np.array([1.0, 0.5, 0.75, 0.25, 0.9], np.float32).reshape(5, 1, 1, 1)
    tms = np.stack([O.DEMO_TRANS_MAT[0]] + [O.synth_trans_mat(30.0 + 50.0 * k, 25.0, 0.8) for k in range(4)]
                   ).astype(np.float32)
    boxes = np.asarray([[-1.0, -1.0, -1.0, 1.0, 1.0 + 0.05 * b, 1.0] for b in range(5)], np.float32)
    return imgs, tms, boxes


def test_reconstruct_equals_create_sdf_then_marching_cubes():
    from disn_amd import create_sdf as cs, isosurface
    from disn_amd.engine import SdfEngine
    from disn_amd.weights import WeightStore
    eng = SdfEngine(WeightStore.random_init(0, mode="he"))
    imgs, tms, boxes = _five_views()                               # 5 images: the batched kernel forms
    R = 16
    grids = cs.create_sdf(eng, imgs, tms, boxes, R)
    iso = float(grids[0].median())                                 # a level that image 0's grid crosses
    want = [_host(isosurface.marching_cubes(grids[b], boxes[b].astype(np.float64), R, iso)) for b in range(5)]
    got = cs.reconstruct(eng, imgs, tms, boxes, R, iso)
    assert len(got) == 5
    for b in range(5):
        assert _same(_host(got[b]), want[b]), "image %d" % b
    nonempty = sum(len(w[1]) > 0 for w in want)
    print("\n[reconstruct] iso %.6g, triangles per image %s" % (iso, [len(w[1]) for w in want]))
    assert len(want[0][1]) > 0 and nonempty >= 3


def _same_bits(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape
                                    and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))
                                    for x, y in zip(a, b))


def test_every_stage_at_once_equals_the_stage_functions_one_after_another(tmp_path):
    """``reconstruct_select`` and ``reconstruct_fused_select`` with every stage on, bit for bit the public stage
    functions called in the order documented at ``create_sdf._mesh_stages`` on the same grids"""
    from disn_amd import create_sdf as cs, isosurface
    from disn_amd.engine import SdfEngine
    from disn_amd.weights import WeightStore
    cats, objs = (("chair", "03001627"),), {"03001627": ["obj_a", "obj_b"]}
    entries = RF.expected_entries(4, 2, cats, objs)
    assert len(entries) == 4                                       # two objects, two views each: two runs of fuse=2
    batch = cs.load_group(entries, *RF.build_dataset(str(tmp_path / "data"), entries))
    imgs, tms, R, band = batch["img"], batch["trans_mat"], 8, (4, 0.5, 1)
    sp = np.asarray(batch["sdf_params"], np.float64).reshape(4, 6)
    eng = SdfEngine(WeightStore.random_init(3))
    iso = float(cs.create_sdf(eng, imgs, tms, sp, R)[0].median())
    on = {"clean": (3.0, 0.0, "face"), "strict": False, "simplify": 4, "smooth": 2, "colour": True, "mesher": "dcs"}
    dc, smooth, colour = cs.dc_args("dcs"), cs.smooth_args(2), cs.colour_args(True)

    def stages(meshes, boxes, refine, views_per_mesh, cams):
        meshes, unclean = cs.clean_group(meshes, on["clean"], None, strict=False)
        meshes = cs.smooth_group(cs.simplify_group(meshes, on["simplify"], boxes), smooth, boxes, R)
        if refine:
            meshes = [isosurface.refine_mesh(eng, enc, b, tms, v, f, boxes[b], R, iso, 1)
                      for b, (v, f) in enumerate(meshes)]
        return cs.colour_group(meshes, colour, imgs, cams, views_per_mesh), unclean

    got, got_unclean = cs.reconstruct_select(eng, imgs, tms, sp, R, iso, refine=1, normals=True, band=band, **on)
    enc = eng.encode(imgs)
    grids = cs.create_sdf(eng, imgs, tms, sp, R, band=band, iso=iso)
    want, want_unclean = stages(cs.mesh_group(grids, sp, R, iso, dc, eng, enc, tms), sp, True, 1, tms)
    print("\n[pipeline] iso %.6g, triangles per view %s" % (iso, [len(m[1]) for m in want]))
    assert len(got) == 4 and any(len(m[1]) for m in want) and got_unclean == want_unclean
    for b in range(4):
        assert len(got[b]) == 4 and _same_bits(got[b], want[b]), "view %d" % b

    got, got_unclean = cs.reconstruct_fused_select(eng, imgs, tms, sp, R, iso, fuse=2, **on)
    grids = torch.stack([eng.query_grid_views(enc, (2 * r, 2), tms[2 * r:2 * r + 2], sp[2 * r], R, "max")
                         for r in range(2)])
    want, want_unclean = stages(cs.mesh_group(grids, sp[::2], R, iso, dc), sp[::2], False, 2, tms)
    print("[pipeline] fused: triangles per run %s" % [len(m[1]) for m in want])
    assert len(got) == 2 and any(len(m[1]) for m in want) and got_unclean == want_unclean
    for r in range(2):
        assert len(got[r]) == 3 and _same_bits(got[r], want[r]), "run %d" % r


# ------------------------------------------------------------------ 4. the command line, end to end
def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


SEED, VIEW_NUM = 4, 3


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """2 categories x 2 objects x 3 views, two list files, a He-mode checkpoint and an engine restored from it"""
    from disn_amd.engine import SdfEngine
    from disn_amd.weights import WeightStore
    root = tmp_path_factory.mktemp("reconstruct")
    entries = RF.expected_entries(SEED, VIEW_NUM)
    assert len(entries) == 12
    sdf_dir, rendered_dir = RF.build_dataset(str(root / "data"), entries)
    lst_dir = str(root / "lst")
    RF.write_lists(lst_dir)
    log_dir = str(root / "ckpt")
    os.makedirs(log_dir)
    WeightStore.random_init(2, mode="he").save_tf(os.path.join(log_dir, "model.ckpt"))
    store = WeightStore.restore_latest(log_dir)
    return {"entries": entries, "sdf_dir": sdf_dir, "rendered_dir": rendered_dir, "lst_dir": lst_dir,
            "log_dir": log_dir, "store": store, "engine": SdfEngine(store)}


def test_create_sdf_command_line(world, tmp_path):
    from disn_amd import create_sdf as cs, isosurface
    seed, view_num, R = SEED, VIEW_NUM, 16
    entries, sdf_dir, rendered_dir = world["entries"], world["sdf_dir"], world["rendered_dir"]
    lst_dir, log_dir, eng = world["lst_dir"], world["log_dir"], world["engine"]
    first = cs.load_group(entries[:view_num], sdf_dir, rendered_dir)
    iso = float(cs.create_sdf(eng, first["img"], first["trans_mat"], first["sdf_params"], R)[0].median())
    base = ["--log_dir", log_dir, "--test_lst_dir", lst_dir, "--sdf_dir", sdf_dir, "--rendered_dir", rendered_dir,
            "--category", "chair,car", "--view_num", str(view_num), "--sdf_res", str(R), "--iso", repr(iso),
            "--seed", str(seed)]
    res = cs.main(base)
    out_dir = os.path.join(log_dir, "test_objs", "17_" + str(iso))
    assert res["out_dir"] == out_dir and res["written"] == 12 and res["skipped"] == 0
    expect = sorted(os.path.join(c, "%s_%s_%02d.obj" % (c, o, v)) for c, o, v in entries)
    assert _tree(out_dir) == expect                                # every expected path, and nothing else
    assert os.path.isfile(os.path.join(log_dir, "log_test.txt"))
    # the bytes: write_obj of reconstruct on the same groups (consecutive runs of batch_size = view_num entries)
    want, nonempty = {}, 0
    for g0 in range(0, len(entries), view_num):
        group = entries[g0:g0 + view_num]
        batch = cs.load_group(group, sdf_dir, rendered_dir)
        assert batch["view_id"] == [v for _, _, v in group]
        meshes = cs.reconstruct(eng, batch["img"], batch["trans_mat"], batch["sdf_params"], R, iso)
        for (c, o, v), (verts, faces) in zip(group, meshes):
            p = str(tmp_path / "want" / ("%s_%s_%02d.obj" % (c, o, v)))
            isosurface.write_obj(p, verts, faces)
            want[os.path.join(c, "%s_%s_%02d.obj" % (c, o, v))] = open(p, "rb").read()
            nonempty += len(faces) > 0
    assert nonempty >= 3 and res["empty"] == 12 - nonempty
    for rel in expect:
        assert open(os.path.join(out_dir, rel), "rb").read() == want[rel], rel
    # --skip_existing: files above 200 bytes are left alone (an empty mesh's file is not above 200 bytes: redone)
    small = [rel for rel in expect if len(want[rel]) <= 200]
    stamp = {rel: os.stat(os.path.join(out_dir, rel)).st_mtime_ns for rel in expect}
    res2 = cs.main(base + ["--skip_existing"])
    assert res2["written"] == len(small) and res2["skipped"] == 12 - len(small)
    assert all(os.stat(os.path.join(out_dir, rel)).st_mtime_ns == stamp[rel] for rel in expect if rel not in small)
    # two shards together: the same files with the same bytes
    shutil.rmtree(out_dir)
    r0 = cs.main(base + ["--num_shards", "2", "--shard_id", "0"])
    part0 = _tree(out_dir)
    r1 = cs.main(base + ["--num_shards", "2", "--shard_id", "1"])
    assert r0["written"] == 6 and r1["written"] == 6 and len(part0) == 6
    assert _tree(out_dir) == expect
    for rel in expect:
        assert open(os.path.join(out_dir, rel), "rb").read() == want[rel], rel


# ------------------------------------------------------------------ 5. the demo
def _demo_png(path, seed=8):
    from PIL import Image
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, size=(137, 137, 4), dtype=np.uint8)
    Image.fromarray(a, "RGBA").save(path)
    return a


def test_demo_with_the_given_camera(tmp_path):
    from disn_amd import create_sdf as cs, demo, isosurface
    from disn_amd.engine import SdfEngine
    from disn_amd.weights import WeightStore
    png = str(tmp_path / "view.png")
    a = _demo_png(png)
    img = (a[:, :, [2, 1, 0]].astype(np.float32) / np.float32(255.0))[None]
    assert np.array_equal(demo.read_image(png), img)
    eng = SdfEngine(WeightStore.random_init(3))
    R = 16
    iso = float(cs.create_sdf(eng, img, O.DEMO_TRANS_MAT, [[-1, -1, -1, 1, 1, 1]], R)[0].median())
    out = str(tmp_path / "mesh" / "demo.obj")
    res = demo.main(["--img", png, "--log_dir", str(tmp_path / "none"), "--random_init", "3", "--sdf_res", str(R),
                     "--iso", repr(iso), "--out", out])
    assert np.array_equal(res["trans_mat"], O.DEMO_TRANS_MAT)
    verts, faces = cs.reconstruct(eng, img, O.DEMO_TRANS_MAT, [[-1, -1, -1, 1, 1, 1]], R, iso)[0]
    assert len(faces) > 0 and res["faces"] == len(faces) and res["verts"] == len(verts)
    want = str(tmp_path / "want.obj")
    isosurface.write_obj(want, verts, faces)
    assert open(out, "rb").read() == open(want, "rb").read()
    with pytest.raises(FileNotFoundError):
        demo.main(["--img", png, "--log_dir", str(tmp_path / "none"), "--out", out])


def test_demo_with_the_estimated_camera(tmp_path):
    from disn_amd import create_sdf as cs, demo, isosurface, tf_checkpoint as tfc, train_cam
    from disn_amd.engine import SdfEngine
    from disn_amd.posenet import CameraEstimator
    from disn_amd.weights import WeightStore
    png = str(tmp_path / "view.png")
    _demo_png(png, 9)
    img = demo.read_image(png)
    cam_dir = str(tmp_path / "cam")
    os.makedirs(cam_dir)
    tfc.save_checkpoint(os.path.join(cam_dir, "latest.ckpt"), train_cam.random_init(5))
    tfc.write_checkpoint_state(cam_dir, "latest.ckpt")
    store_c, head = demo.restore_camera(cam_dir, None)
    tm = CameraEstimator(store_c, head).get_model(img)["pred_trans_mat"]
    assert tuple(tm.shape) == (1, 4, 3) and not np.allclose(tm.cpu().numpy(), O.DEMO_TRANS_MAT)
    eng = SdfEngine(WeightStore.random_init(3))
    R = 16
    iso = float(cs.create_sdf(eng, img, tm, [[-1, -1, -1, 1, 1, 1]], R)[0].median())
    out = str(tmp_path / "demo_cam.obj")
    res = demo.main(["--img", png, "--log_dir", str(tmp_path / "none"), "--random_init", "3", "--cam_est",
                     "--cam_log_dir", cam_dir, "--sdf_res", str(R), "--iso", repr(iso), "--out", out])
    assert np.array_equal(res["trans_mat"], tm.cpu().numpy())
    verts, faces = cs.reconstruct(eng, img, tm, [[-1, -1, -1, 1, 1, 1]], R, iso)[0]
    assert len(faces) > 0
    want = str(tmp_path / "want.obj")
    isosurface.write_obj(want, verts, faces)
    assert open(out, "rb").read() == open(want, "rb").read()


# ------------------------------------------------------------------ 6. sdf_acc
def test_sdf_acc_against_the_float64_oracle(world):
    """``evaluate sdf_acc`` on the tiny dataset, N = 256 points per view, 3 batches of 4 views, against the float64
    oracle forward and the loss definition of models/model_normalization.py:278-299.  Tolerances from the project's
    1e-5 bar on pred_sdf (not measured): sdf_loss_realvalue = mean|gt - pred/10| moves by at most 1e-5/10 = 1e-6;
    sdf_loss = 1000 * mean(|10 gt - pred| * mask), mask <= 4, by at most 1000 * 4 * 1e-5 = 0.04; accuracy can differ
    only at points whose sign the bar leaves open: k/(B N), k = #points with oracle |pred_sdf| <= 1e-5."""
    from disn_amd import create_sdf as cs, evaluate
    N, B = 256, 4
    W = world["store"].arrays
    res = evaluate.main(["sdf_acc", "--log_dir", world["log_dir"], "--test_lst_dir", world["lst_dir"],
                         "--sdf_dir", world["sdf_dir"], "--rendered_dir", world["rendered_dir"],
                         "--category", "chair,car", "--view_num", str(VIEW_NUM), "--seed", str(SEED),
                         "--batch_size", str(B), "--num_sample_points", str(N)])
    assert res["batches"].shape == (3, 5)
    reg = sum(1e-5 * 0.5 * float(np.sum(np.asarray(v, np.float64) ** 2)) for k, v in W.items() if k.endswith("/weights"))
    k_total = n_total = 0
    for got, entries in ((res, world["entries"]),):
        rows, slack = [], []
        for gi, g0 in enumerate(range(0, len(entries), B)):
            group = entries[g0:g0 + B]
            batch = cs.load_group(group, world["sdf_dir"], world["rendered_dir"], False, N, False, SEED + gi)
            feed = {"imgs": batch["img"], "sample_pc": batch["sdf_pt"], "sample_pc_rot": batch["sdf_pt_rot"],
                    "trans_mat": batch["trans_mat"]}
            pred = np.asarray(O.get_model(feed, W, dtype=np.float64)["pred_sdf"], np.float64)
            gt = (batch["sdf_val"] - 0.003).astype(np.float32).astype(np.float64)
            mask = np.where(gt <= np.float64(np.float32(0.01)), 4.0, 1.0)
            rows.append([np.mean((gt > 0) == (pred > 0)), np.mean(np.abs(gt - pred / 10.0)),
                         1000.0 * np.mean(np.abs(gt * 10.0 - pred) * mask)])
            k = int((np.abs(pred) <= 1e-5).sum())
            slack.append(k / pred.size)
            k_total += k
            n_total += pred.size
        want = np.mean(np.asarray(rows), axis=0)
        print("\n[sdf_acc] got %s\n          f64 %s  (accuracy slack %.3g)" % (
            [got[n] for n in evaluate.SDF_ACC_NAMES], want.tolist(), float(np.mean(slack))))
        assert abs(got["sdf_loss_realvalue"] - want[1]) <= 1e-6
        assert abs(got["sdf_loss"] - want[2]) <= 0.04
        assert abs(got["accuracy"] - want[0]) <= float(np.mean(slack)) + 1e-7       # (+ float32 rounding of a mean)
        assert abs(got["regularization"] - reg) <= 1e-6 * reg
        assert abs(got["overall_loss"] - (got["sdf_loss"] + got["regularization"])) <= 1e-5 * got["overall_loss"]
        assert 0.0 < want[0] < 1.0                                                  # both signs occur: a real check
    assert n_total == 12 * N and k_total <= 0.01 * n_total

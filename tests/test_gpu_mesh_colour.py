"""Vertex colours on the device (mesh_colour.hip: disn_mesh_zbuffer_batch / disn_mesh_colour_batch;
``postprocess.zbuffer_meshes_device`` / ``colour_meshes_device`` / ``colour_arrays_device``) and the drivers' ``--colour``.
The reference of every comparison is the host rule, ``postprocess.zbuffer_arrays`` / ``colour_arrays``: the depth maps are
compared in every bit and the colours and classes in every byte, with no vertex left out -- the float32 operations are
restated in the host's order without contraction, the maximum is an integer maximum of the bits, every sum an integer sum
(DESIGN 4zb)."""
import os

import numpy as np
import pytest
import torch

import mesh_colour_fixtures as CF
from guarded_alloc import guarded

pytestmark = pytest.mark.gpu


def _dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _bytes_equal(got_c, got_s, want, what):
    gc, gs = got_c.cpu().numpy(), got_s.cpu().numpy()
    assert gc.dtype == np.uint8 and gs.dtype == np.uint8 and gc.shape == want[0].shape and gs.shape == want[1].shape, what
    bad = np.nonzero(gs != want[1])[0]
    assert bad.size == 0, "%s: %d of %d classes differ, first %d: device %d host %d" % (
        what, bad.size, gs.size, bad[0], gs[bad[0]], want[1][bad[0]])
    bad = np.nonzero((gc != want[0]).any(1))[0]
    assert bad.size == 0, "%s: %d of %d colours differ, first %d: device %s host %s" % (
        what, bad.size, gs.size, bad[0], gc[bad[0]], want[0][bad[0]])


def _bits_equal(got, want, what):
    g = got.cpu().numpy()
    assert g.dtype == np.float32 and g.shape == want.shape, what
    bad = np.nonzero(g.view(np.uint32).reshape(-1) != want.view(np.uint32).reshape(-1))[0]
    assert bad.size == 0, "%s: %d of %d depth values differ in their bits, first at %d: device %r host %r" % (
        what, bad.size, g.size, bad[0], g.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


# ------------------------------------------------------------------ 1. the device against the specification
@pytest.mark.parametrize("name", list(CF.device_cases()))
def test_device_equals_the_rule(name):
    from disn_amd import postprocess
    v, f, img, T, alpha, kw = CF.device_cases()[name]
    dv, df, dimg = _dev(v, f, img)
    zb = postprocess.zbuffer_meshes_device([(dv, df)], T[None], views_per_mesh=T.shape[0], S=kw.get("S", 2))
    _bits_equal(zb[0], CF.host_zbuffer(name), name)
    dalpha = None if alpha is None else _dev(alpha)[0]
    col, seen = postprocess.colour_arrays_device(dv, df, dimg, T, alpha=dalpha, **kw)
    want = CF.host_colour(name)
    _bytes_equal(col, seen, want, name)
    if name == "quad":                                                 # two faces, both over the per-thread box
        assert (CF.host_zbuffer(name) > 0).all()
    if name.startswith("mixed"):
        assert len(np.unique(want[1])) >= 2


# ------------------------------------------------------------------ 2. a batch equals every mesh alone
def _batch():
    """an empty mesh, one triangle, a face index out of range (its own nv: the next mesh's first vertex), a NaN
    coordinate, and two ordinary meshes, each with its own pair of cameras"""
    sq = CF.square(3, 0.3, 0.0)
    bad_f = sq[1].copy()
    bad_f[2, 1] = len(sq[0])
    bad_v = sq[0].copy()
    bad_v[5, 0] = np.nan
    tri = (np.array([[-0.3, -0.2, 0.1], [0.3, -0.2, 0.0], [0.0, 0.3, -0.1]], np.float32), np.array([[0, 1, 2]], np.int32))
    meshes = [(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)), tri, (sq[0], bad_f), (bad_v, sq[1]),
              CF.uv_sphere(24, 12), CF.occluder(12)[:2]]
    cams = np.stack([np.stack([CF.pinhole(rot_y=0.3 * b), CF.pinhole(rot_y=0.3 * b + 2.0, cx=60.0)]) for b in range(6)])
    imgs = np.stack([np.stack([CF.noise_image(10 + 2 * b), CF.noise_image(11 + 2 * b)]) for b in range(6)])
    return meshes, cams, imgs, [0, 0, 2, 4, 0, 0]


def test_batch_equals_every_mesh_alone():
    from disn_amd import postprocess
    meshes, cams, imgs, statuses = _batch()
    dev = [_dev(v, f) for v, f in meshes]
    dimg = _dev(imgs)[0]
    kw = {"mirror_axis": 0, "fill_iters": 8}
    cs_, ss, st = postprocess.colour_meshes_device(dev, dimg, cams, views_per_mesh=2, strict=False, **kw)
    zb, zst = postprocess.zbuffer_meshes_device(dev, cams, views_per_mesh=2, strict=False)
    assert st.tolist() == statuses and zst.tolist() == statuses
    for b, (v, f) in enumerate(meshes):
        if statuses[b]:
            assert (cs_[b] == 128).all() and (ss[b] == 0).all() and cs_[b].shape == (len(v), 3)
            assert not zb[b].any()
            continue
        want = postprocess.colour_arrays(v, f, imgs[b], cams[b], **kw)
        _bytes_equal(cs_[b], ss[b], want, "mesh %d" % b)
        _bits_equal(zb[b], postprocess.zbuffer_arrays(v, f, cams[b]), "mesh %d" % b)
        if len(v):
            alone_c, alone_s = postprocess.colour_arrays_device(*dev[b], dimg[b], cams[b], **kw)
            assert torch.equal(alone_c, cs_[b]) and torch.equal(alone_s, ss[b])
    assert cs_[0].shape == (0, 3) and ss[0].shape == (0,)
    with pytest.raises(ValueError, match="mesh 2: face index out of range"):
        postprocess.colour_meshes_device(dev, dimg, cams, views_per_mesh=2)
    with pytest.raises(ValueError, match="mesh 1: a vertex coordinate is not finite"):
        postprocess.zbuffer_meshes_device([dev[1], dev[3]], cams[[1, 3]], views_per_mesh=2)
    with pytest.raises(TypeError):
        postprocess.colour_meshes_device([meshes[1]], dimg[1], cams[1], views_per_mesh=2)   # host arrays: no CPU fallback
    with pytest.raises(TypeError):
        postprocess.colour_meshes_device([dev[1]], imgs[1], cams[1], views_per_mesh=2)
    assert postprocess.colour_meshes_device([], dimg, cams) == ([], [])


# ------------------------------------------------------------------ 3. the memory contract of the two device entries
def _contract_scenario(g):
    from disn_amd import postprocess
    meshes, cams, imgs, statuses = _batch()
    alpha = (np.random.default_rng(6).random((6, 2, CF.IMG, CF.IMG)) > 0.2).astype(np.uint8)
    dev = [(g.put(v) if len(v) else torch.from_numpy(v).cuda(), g.put(f) if len(f) else torch.from_numpy(f).cuda())
           for v, f in meshes]
    kw = {"mirror_axis": 2, "fill_iters": 4, "S": 4}
    cs_, ss, st = postprocess.colour_meshes_device(dev, g.put(imgs), cams, views_per_mesh=2, alpha=g.put(alpha),
                                                   strict=False, **kw)
    zb, zst = postprocess.zbuffer_meshes_device(dev, cams, views_per_mesh=2, S=1, strict=False)
    out = {"status": st, "zstatus": zst, "zbuf": zb.cpu().numpy()}
    for b in range(len(meshes)):
        out["c%d" % b], out["s%d" % b] = cs_[b].cpu().numpy(), ss[b].cpu().numpy()

    def verify(r):
        assert r["status"].tolist() == statuses and r["zstatus"].tolist() == statuses
        for b, (v, f) in enumerate(meshes):
            if statuses[b]:
                assert (r["c%d" % b] == 128).all() and (r["s%d" % b] == 0).all() and not r["zbuf"][b].any()
                continue
            want = postprocess.colour_arrays(v, f, imgs[b], cams[b], alpha=alpha[b], **kw)
            assert np.array_equal(r["c%d" % b], want[0]) and np.array_equal(r["s%d" % b], want[1]), b
            assert np.array_equal(r["zbuf"][b].view(np.uint32), postprocess.zbuffer_arrays(v, f, cams[b], 1).view(np.uint32))
    return out, verify


# the device entries of include/disn_amd_colour.h (tests/test_guarded_alloc_host.py reads this tuple)
NEW = ("disn_mesh_colour_workspace_bytes", "disn_mesh_zbuffer_batch", "disn_mesh_colour_batch")


def test_memory_contract_of_the_colour_entries():
    """in the manner of test_gpu_mesh_simplify.py: every buffer the wrappers hand over (the workspace too) lies between
    guard bands and starts out poisoned; guards intact, const inputs unchanged, runs A and B bit-identical, both device
    entries really called"""
    results, verify = {}, None
    for variant in ("A", "B"):
        with guarded(variant) as g:
            with g.recording() as called:
                out, check_reference = _contract_scenario(g)
            g.check()
        missing = sorted(set(NEW) - set(called))
        assert set(NEW) <= set(called), "variant %s: the scenario never called %s" % (variant, missing)
        results[variant] = out
        verify = verify or check_reference
    a, b = results["A"], results["B"]
    assert sorted(a) == sorted(b)
    differ = [k for k in a if not (a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes())]
    assert not differ, "results depend on what the buffers held before, or on memory outside them: %s" % differ
    verify(a)


def test_a_workspace_one_byte_short_is_refused_without_a_launch():
    from disn_amd import ops
    from disn_amd._lib import lib
    h = lib()
    v, f = CF.uv_sphere(16, 8)
    dv, df, dimg, dtm = _dev(v, f, CF.noise_image(1)[None], CF.pinhole()[None])
    v_off, f_off = np.array([0, len(v)], np.int64), np.array([0, len(f)], np.int64)
    need = h.disn_mesh_colour_workspace_bytes(1, 1, len(v), len(f), 2)
    ws = torch.full((need,), 9, dtype=torch.uint8, device="cuda")
    col = torch.full((len(v), 3), 7, dtype=torch.uint8, device="cuda")
    seen = torch.full((len(v),), 7, dtype=torch.uint8, device="cuda")
    status = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    zbuf = torch.full((1, 1, 274, 274), 7.0, device="cuda")
    colour = lambda nbytes: h.disn_mesh_colour_batch(
        dv.data_ptr(), df.data_ptr(), v_off.ctypes.data, f_off.ctypes.data, 1, dimg.data_ptr(), None, dtm.data_ptr(), 1, 2,
        1e-3, -1, 32, 1, col.data_ptr(), seen.data_ptr(), status.data_ptr(), ws.data_ptr(), nbytes, ops._stream())
    depth = lambda nbytes: h.disn_mesh_zbuffer_batch(
        dv.data_ptr(), df.data_ptr(), v_off.ctypes.data, f_off.ctypes.data, 1, dtm.data_ptr(), 1, 2, zbuf.data_ptr(),
        status.data_ptr(), ws.data_ptr(), nbytes, ops._stream())
    assert colour(need - 1) == -3 and depth(need - 1) == -3
    torch.cuda.synchronize()
    assert (col == 7).all() and (seen == 7).all() and (status == -7).all() and (zbuf == 7.0).all() and (ws == 9).all()
    assert colour(need) == 0 and depth(need) == 0
    torch.cuda.synchronize()
    assert status.item() == 0 and (seen != 7).all()


# ------------------------------------------------------------------ 4. the pipeline
def _engine_and_groups(tmp_path, view_num, R):
    import reconstruct_fixtures as RF
    from disn_amd import create_sdf as cs
    from disn_amd.engine import SdfEngine
    from disn_amd.weights import WeightStore
    cats = (("chair", "03001627"), ("car", "02958343"))
    objs = {"03001627": ["obj_a"], "02958343": ["obj_c"]}
    seed = 4
    entries = RF.expected_entries(seed, view_num, cats, objs)
    sdf_dir, rendered_dir = RF.build_dataset(str(tmp_path / "data"), entries)
    lst_dir, log_dir = str(tmp_path / "lst"), str(tmp_path / "ckpt")
    RF.write_lists(lst_dir, cats, objs)
    eng = SdfEngine(WeightStore.random_init(3))
    groups = [cs.load_group(entries[i:i + view_num], sdf_dir, rendered_dir) for i in range(0, len(entries), view_num)]
    iso = float(cs.create_sdf(eng, groups[0]["img"], groups[0]["trans_mat"], groups[0]["sdf_params"], R)[0].median())
    base = ["--log_dir", log_dir, "--random_init", "3", "--test_lst_dir", lst_dir, "--sdf_dir", sdf_dir,
            "--rendered_dir", rendered_dir, "--category", "chair,car", "--view_num", str(view_num), "--sdf_res", str(R),
            "--iso", repr(iso), "--seed", str(seed)]
    return eng, entries, groups, iso, base


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_reconstruct_colour_leaves_the_meshes_and_equals_the_rule(tmp_path):
    from disn_amd import create_sdf as cs, isosurface, postprocess
    view_num, R = 3, 8
    eng, entries, groups, iso, base = _engine_and_groups(tmp_path, view_num, R)
    batch = groups[0]
    img, tm = np.asarray(batch["img"], np.float32), np.asarray(batch["trans_mat"], np.float32).reshape(-1, 4, 3)
    args = (batch["img"], batch["trans_mat"], batch["sdf_params"], R, iso)
    coloured = 0
    for kw in ({}, {"refine": 2, "normals": True},
               {"clean": (0.5, 0.3, "face"), "simplify": 4, "refine": 1, "normals": True, "band": (2, 0.5, 1)}):
        plain = cs.reconstruct_select(eng, *args, strict=False, **kw)[0]
        both = cs.reconstruct_select(eng, *args, strict=False, colour=True, **kw)[0]
        assert len(plain) == len(both) == view_num
        for b in range(view_num):
            assert len(both[b]) == len(plain[b]) + 1 and both[b][-1].dtype == torch.uint8
            for x, y in zip(plain[b], both[b]):
                assert x.dtype == y.dtype and torch.equal(x.view(torch.int32), y.view(torch.int32))
            v, f = both[b][0].cpu().numpy(), both[b][1].cpu().numpy()
            want = postprocess.colour_arrays(v, f, img[b:b + 1], tm[b:b + 1])
            assert np.array_equal(both[b][-1].cpu().numpy(), want[0]), (kw, b)
            coloured += len(v) > 0 and len(np.unique(want[0], axis=0)) > 1
    assert coloured >= 3, "the fixture's meshes are coloured at all"
    # fused: one mesh of the three views, coloured from all of them
    plain = cs.reconstruct_fused(eng, *args, fuse=3)
    fused = cs.reconstruct_fused(eng, *args, fuse=3, colour={"mirror_axis": "x"})
    assert len(fused) == 1 and len(fused[0]) == 3
    assert torch.equal(fused[0][0].view(torch.int32), plain[0][0].view(torch.int32)) and torch.equal(fused[0][1], plain[0][1])
    v, f = fused[0][0].cpu().numpy(), fused[0][1].cpu().numpy()
    want = postprocess.colour_arrays(v, f, img, tm, mirror_axis=0)
    assert len(v) > 0 and np.array_equal(fused[0][2].cpu().numpy(), want[0])
    first_only = postprocess.colour_arrays(v, f, img[:1], tm[:1], mirror_axis=0)
    assert (want[0] != first_only[0]).any(), "the other two views reach the colours"

    # the driver: the _col tree holds the returned colours and scores as the plain tree does
    res = cs.main(base + ["--colour"])
    assert res["out_dir"] == cs.result_obj_path(base[1], R, iso) + "_col" and res["written"] == len(entries)
    assert res["coloured"] == res["written"] - res["empty"]
    ref = cs.main(base)
    assert _tree(ref["out_dir"]) == _tree(res["out_dir"])
    for gi, group in enumerate(groups):
        meshes = cs.reconstruct(eng, group["img"], group["trans_mat"], group["sdf_params"], R, iso, colour=True)
        for b, e in enumerate(entries[gi * view_num:(gi + 1) * view_num]):
            path = cs.obj_path(res["out_dir"], *e)
            if len(meshes[b][0]):
                assert np.array_equal(isosurface.read_obj_colours(path), meshes[b][2].cpu().numpy())
            assert np.array_equal(isosurface.read_obj_verts(path), isosurface.read_obj_verts(cs.obj_path(ref["out_dir"], *e)))


def test_demo_colour_writes_the_returned_colours(tmp_path):
    from PIL import Image
    from disn_amd import create_sdf as cs, demo, isosurface, postprocess
    from disn_amd.engine import SdfEngine
    from disn_amd.weights import WeightStore
    from oracle import disn_oracle as O
    png = str(tmp_path / "view.png")
    rgba = np.random.default_rng(8).integers(0, 256, size=(137, 137, 4), dtype=np.uint8)
    rgba[:, :40, 3] = 0                                                # a background band
    Image.fromarray(rgba, "RGBA").save(png)
    img = demo.read_image(png)
    eng = SdfEngine(WeightStore.random_init(3))
    R, box = 16, [[-1, -1, -1, 1, 1, 1]]
    iso = float(cs.create_sdf(eng, img, O.DEMO_TRANS_MAT, box, R)[0].median())
    args = ["--img", png, "--log_dir", str(tmp_path / "none"), "--random_init", "3", "--sdf_res", str(R),
            "--iso", repr(iso)]
    plain = demo.main(args + ["--out", str(tmp_path / "plain.obj")])
    col = demo.main(args + ["--out", str(tmp_path / "col.obj"), "--color", "--normals"])
    assert col["coloured"] is True and "coloured" not in plain and col["verts"] == plain["verts"] > 0
    assert np.array_equal(isosurface.read_obj_colours(col["out"]), col["colours"])
    verts, faces = cs.reconstruct(eng, img, O.DEMO_TRANS_MAT, box, R, iso)[0]
    want = postprocess.colour_arrays(verts, faces, img, np.asarray(O.DEMO_TRANS_MAT, np.float32).reshape(1, 4, 3),
                                     alpha=demo.read_alpha(png)[None])
    assert np.array_equal(col["colours"], want[0]) and len(np.unique(want[1])) >= 2
    assert np.array_equal(isosurface.read_obj_verts(col["out"]), isosurface.read_obj_verts(plain["out"]))
    assert sum(l.startswith("vn ") for l in open(col["out"])) == col["verts"]


def test_a_coloured_tree_scores_as_the_plain_one(tmp_path):
    from disn_amd import evaluate, isosurface
    cat, objs = "03001627", ["objA", "objB"]
    rng = np.random.default_rng(9)
    for j, obj in enumerate(objs):
        v, f = CF.uv_sphere(24, 12, 0.4 + 0.05 * j)
        isosurface.write_obj(str(tmp_path / "gt" / cat / obj / "isosurf.obj"), v, f)
        for view in range(3):
            pv, pf = CF.uv_sphere(16, 8, 0.38 + 0.02 * view + 0.05 * j)
            name = "%s_%s_%02d.obj" % (cat, obj, view)
            isosurface.write_obj(str(tmp_path / "plain" / cat / name), pv, pf)
            isosurface.write_obj(str(tmp_path / "plain_col" / cat / name), pv, pf,
                                 colours=rng.integers(0, 256, size=pv.shape, dtype=np.uint8))
    (tmp_path / "lst").mkdir()
    (tmp_path / "lst" / (cat + "_test.lst")).write_text("\n".join(objs) + "\n")
    run = lambda tree: evaluate.main(["cd_emd", "--cal_dir", str(tmp_path / tree), "--gt_dir", str(tmp_path / "gt"),
                                      "--test_lst_dir", str(tmp_path / "lst"), "--category", "chair", "--view_num", "3",
                                      "--num_sample_points", "512", "--seed", "7"])[cat]

    def numbers(x):
        if isinstance(x, dict):
            return {k: numbers(val) for k, val in x.items() if k != "views"}
        if isinstance(x, (list, tuple)):
            return [numbers(val) for val in x]
        return np.asarray(x).tolist() if not isinstance(x, str) else None

    a, b = run("plain"), run("plain_col")
    assert numbers(a) == numbers(b) and numbers(a)

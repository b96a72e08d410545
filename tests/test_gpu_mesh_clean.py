"""Small-part cleanup on the device (mesh_clean.hip: disn_mesh_components_device, disn_mesh_clean_count_batch,
disn_mesh_clean_emit_batch; ``postprocess.separate_mesh_device`` / ``clean_meshes_device`` / ``clean_arrays_device``)
and the drivers' ``--clean``.  The reference of every comparison is the host path (``separate_mesh``, ``clean_arrays``,
for labels also the pure-Python ``voxel_reference.components``); everything is compared bit for bit, under the
condition on the inputs that ``mesh_clean_fixtures.assert_margins`` checks first."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mesh_clean_fixtures as MF

pytestmark = pytest.mark.gpu


def _dev(v, f, *rest):
    return (torch.from_numpy(np.ascontiguousarray(v)).cuda(), torch.from_numpy(np.ascontiguousarray(f)).cuda()) + \
        tuple(torch.from_numpy(np.ascontiguousarray(r)).cuda() for r in rest)


def _equal_to_host(got, kept, want, what=""):
    """one mesh of ``clean_meshes_device`` against ``host_clean``'s triple"""
    assert want is not None, what
    gv, gf = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert gv.dtype == np.float32 and gf.dtype == np.int32
    assert gv.shape == want[0].shape and gf.shape == want[1].shape, what
    assert np.array_equal(gv.view(np.uint32), np.ascontiguousarray(want[0]).view(np.uint32)), what
    assert np.array_equal(gf, want[1]), what
    assert kept.cpu().tolist() == list(want[2]), what


def _labels_equal(v, f, connectivity):
    from disn_amd import postprocess
    labels, counts = postprocess.separate_mesh_device(*_dev(v, f), connectivity)
    hl, hc = postprocess.separate_mesh(v, f, connectivity)
    assert labels.dtype == torch.int32 and counts.dtype == torch.int64
    assert np.array_equal(labels.cpu().numpy(), hl) and np.array_equal(counts.cpu().numpy(), hc)
    ref, n = MF.components(f, v.shape[0], connectivity)
    assert np.array_equal(hl, ref) and hc.size == n
    return hl, hc


# ------------------------------------------------------------------ 1. two fans and an unreferenced vertex
def test_fans_meeting_in_one_vertex_and_an_unreferenced_vertex():
    from disn_amd import postprocess
    v, f = MF.fans()
    labels, counts = _labels_equal(v, f, "face")
    assert labels.tolist() == [0, 0, 1, 1] and counts.tolist() == [4, 4]
    labels, counts = _labels_equal(v, f, "vertex")
    assert labels.tolist() == [0, 0, 0, 0] and counts.tolist() == [7]
    for conn in ("face", "vertex"):
        want = MF.host_clean(v, f, 0.5, 0.3, conn)
        cv, cf, kept = postprocess.clean_arrays_device(*_dev(v, f), connectivity=conn)
        assert kept == want[2] and np.array_equal(cv.cpu().numpy(), want[0]) and np.array_equal(cf.cpu().numpy(), want[1])
    cv, cf, kept = postprocess.clean_arrays_device(*_dev(v, f))
    assert kept == [0, 1] and np.array_equal(cv.cpu().numpy(), v[[0, 1, 2, 3, 0, 4, 5, 6]])    # 0 twice, 7 dropped
    assert cf.cpu().tolist() == [[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]]
    with pytest.raises(ValueError):
        postprocess.separate_mesh_device(*_dev(v, f), "auto")
    with pytest.raises(ValueError, match="no triangles"):
        postprocess.clean_arrays_device(*_dev(v, np.zeros((0, 3), np.int32)))
    labels, counts = postprocess.separate_mesh_device(*_dev(v, np.zeros((0, 3), np.int32)))
    assert labels.numel() == 0 and counts.numel() == 0


# ------------------------------------------------------------------ 2. non-manifold soups
@pytest.mark.parametrize("connectivity", ["face", "vertex"])
def test_soups_label_like_the_host(connectivity):
    for nv, nf in MF.SOUPS:
        _labels_equal(*MF.soup(nv, nf), connectivity)


# ------------------------------------------------------------------ 3. hooking depth and compression
@pytest.mark.parametrize("connectivity", ["face", "vertex"])
def test_shuffled_strip_is_one_component(connectivity):
    v, f = MF.strip(4096)
    labels, counts = _labels_equal(v, f, connectivity)
    assert counts.tolist() == [4098] and not labels.any()


# ------------------------------------------------------------------ 4. thousands of components
@pytest.mark.parametrize("num_thresh,nkept", [(0.0, 5001), (0.3, 1)])
def test_crowd_of_isolated_triangles_in_front_of_a_sphere(num_thresh, nkept):
    from disn_amd import postprocess
    v, f = MF.crowd(5000)
    want = MF.host_clean(v, f, 0.5, num_thresh)
    assert len(want[2]) == nkept
    cleaned, kept = postprocess.clean_meshes_device([_dev(v, f)], 0.5, num_thresh)
    _equal_to_host(cleaned[0], kept[0], want)
    _labels_equal(v, f, "face")


# ------------------------------------------------------------------ 5. the keep rule
def test_two_spheres_and_the_keep_rule():
    from disn_amd import postprocess
    v, f = MF.two_spheres()
    for shift, dist, num, expect in MF.RULE_CASES:
        vs = v + np.float32(shift)
        want = MF.host_clean(vs, f, dist, num)
        if expect is None:
            assert want is None
            with pytest.raises(ValueError, match="no part is kept"):
                postprocess.clean_arrays_device(*_dev(vs, f), dist_thresh=dist, num_thresh=num)
            cleaned, kept = postprocess.clean_meshes_device([_dev(vs, f)], dist, num, strict=False)
            assert cleaned == [None] and kept[0].numel() == 0
            sizes = _raw(([(vs, f)]), dist, num)[0]
            assert sizes.tolist() == [[2, 0, 0, 0, 1]]
            continue
        assert want[2] == expect
        cleaned, kept = postprocess.clean_meshes_device([_dev(vs, f)], dist, num)
        _equal_to_host(cleaned[0], kept[0], want, str((shift, dist, num)))


# ------------------------------------------------------------------ 6. / 10. a batch, twice
def _batch_results(dist, num):
    from disn_amd import postprocess
    return postprocess.clean_meshes_device([_dev(v, f) for v, f in MF.batch_of_five()], dist, num)


@pytest.mark.parametrize("num_thresh", [0.0, 0.3])
def test_batch_of_five_equals_every_mesh_alone_and_repeats(num_thresh):
    from disn_amd import postprocess
    meshes = MF.batch_of_five()
    cleaned, kept = _batch_results(0.5, num_thresh)
    again, kept_again = _batch_results(0.5, num_thresh)
    assert len(cleaned) == 5
    for b, (v, f) in enumerate(meshes):
        want = MF.host_clean(v, f, 0.5, num_thresh)
        _equal_to_host(cleaned[b], kept[b], want, "mesh %d" % b)
        alone, kept_alone = postprocess.clean_meshes_device([_dev(v, f)], 0.5, num_thresh)
        for other, ids in ((alone[0], kept_alone[0]), (again[b], kept_again[b])):
            assert torch.equal(other[0].view(torch.int32), cleaned[b][0].view(torch.int32))
            assert torch.equal(other[1], cleaned[b][1]) and torch.equal(ids, kept[b])
    assert cleaned[2][0].shape == (0, 3) and cleaned[2][1].shape == (0, 3) and kept[2].numel() == 0


# ------------------------------------------------------------------ 7. the project's own marching cubes
def test_meshes_of_the_batched_marching_cubes_with_carried_arrays():
    from disn_amd import isosurface, postprocess
    R = 16
    grids = [MF.field_grid(R, k) for k in range(3)]
    sdf = torch.from_numpy(np.stack([g[0].reshape(-1) for g in grids])).cuda()
    boxes = np.stack([g[1] for g in grids])
    meshes = isosurface.marching_cubes_batch(sdf, boxes, R, 0.0)
    carried = [(v, f, torch.arange(v.shape[0], device=v.device, dtype=torch.float32)[:, None].repeat(1, 3))
               for v, f in meshes]
    cleaned, kept = postprocess.clean_meshes_device(carried)
    for b, (v, f) in enumerate(meshes):
        hv, hf = v.cpu().numpy(), f.cpu().numpy()
        counts, _ = MF.part_distances(hv, hf)
        assert counts.size >= 2, "grid %d: the far sphere is a part of its own" % b
        want = MF.host_clean(hv, hf)
        assert len(want[2]) < counts.size
        _equal_to_host(cleaned[b], kept[b], want, "grid %d" % b)
        src = cleaned[b][2].cpu().numpy()
        assert src.shape == want[0].shape and (src[:, 0] == src[:, 1]).all() and (src[:, 0] == src[:, 2]).all()
        assert np.array_equal(hv[src[:, 0].astype(np.int64)], want[0])           # the array rode along the vertex map
        labels, _ = postprocess.separate_mesh(hv, hf)
        assert np.array_equal(src[:, 0].astype(np.int64),
                              np.concatenate([np.unique(hf[labels == c]) for c in want[2]]))


# ------------------------------------------------------------------ 8. an out-of-range index that cannot fault
def _raw(meshes, dist=0.5, num=0.3, conn=0):
    """the C entries on host meshes -> (sizes [B,5], per mesh (verts, faces, vmap) or None where nothing is emitted)"""
    from disn_amd import ops
    from disn_amd._lib import check, lib
    h = lib()
    v_off = np.zeros(len(meshes) + 1, np.int64)
    f_off = np.zeros(len(meshes) + 1, np.int64)
    v_off[1:] = np.cumsum([m[0].shape[0] for m in meshes])
    f_off[1:] = np.cumsum([m[1].shape[0] for m in meshes])
    v, f = _dev(np.concatenate([m[0] for m in meshes]), np.concatenate([m[1] for m in meshes]))
    B = len(meshes)
    ws = torch.empty(h.disn_mesh_clean_workspace_bytes(B, int(v_off[-1]), int(f_off[-1])), dtype=torch.uint8,
                     device="cuda")
    counts = torch.zeros((B, 5), dtype=torch.int64, device="cuda")
    st = ops._stream()
    check("count", h.disn_mesh_clean_count_batch(v.data_ptr(), f.data_ptr(), v_off.ctypes.data, f_off.ctypes.data, B,
                                                 conn, dist, num, counts.data_ptr(), ws.data_ptr(), ws.numel(), st))
    sizes = np.ascontiguousarray(counts.cpu().numpy())
    nk, nv, nf = (int(sizes[:, c].sum()) for c in (1, 2, 3))
    ov = torch.full((nv, 3), 7.0, dtype=torch.float32, device="cuda")
    of = torch.full((nf, 3), -7, dtype=torch.int32, device="cuda")
    vm = torch.full((nv,), -7, dtype=torch.int32, device="cuda")
    ko = torch.full((nk,), -7, dtype=torch.int32, device="cuda")
    check("emit", h.disn_mesh_clean_emit_batch(v.data_ptr(), f.data_ptr(), v_off.ctypes.data, f_off.ctypes.data,
                                               sizes.ctypes.data, B, ov.data_ptr(), of.data_ptr(), vm.data_ptr(),
                                               ko.data_ptr(), ws.data_ptr(), ws.numel(), st))
    out, v0, f0 = [], 0, 0
    for b in range(B):
        nvb, nfb = int(sizes[b, 2]), int(sizes[b, 3])
        out.append((ov[v0:v0 + nvb].cpu().numpy(), of[f0:f0 + nfb].cpu().numpy(), vm[v0:v0 + nvb].cpu().numpy()))
        v0, f0 = v0 + nvb, f0 + nfb
    return sizes, out


def test_an_index_equal_to_the_mesh_size_gives_status_2_and_leaves_the_next_mesh_alone():
    """the first mesh's bad index equals its own nv: that slot exists in the shared vertex buffer (the second mesh's
    first vertex), so nothing here could read outside an allocation"""
    from disn_amd import postprocess
    v0, f0 = MF.fans()
    f0 = f0.copy()
    f0[2, 1] = v0.shape[0]
    v1, f1 = MF.icosphere(0.3, 1)
    sizes, out = _raw([(v0, f0), (v1, f1)])
    assert sizes[0].tolist() == [0, 0, 0, 0, 2]
    assert sizes[1].tolist() == [1, 1, 42, f1.shape[0], 0]
    want = MF.host_clean(v1, f1)
    assert np.array_equal(out[1][0], want[0]) and np.array_equal(out[1][1], want[1])
    assert np.array_equal(out[1][2], np.arange(42))
    with pytest.raises(ValueError, match="out of range"):
        postprocess.clean_meshes_device([_dev(v0, f0), _dev(v1, f1)])
    with pytest.raises(ValueError, match="out of range"):
        postprocess.clean_arrays_device(*_dev(v0, f0))
    with pytest.raises(ValueError, match="out of range"):
        postprocess.separate_mesh_device(*_dev(v0, f0))
    from disn_amd._lib import lib
    assert lib().disn_mesh_clean_workspace_bytes(1, 10, (2 ** 31 - 1) // 3 + 1) == 0
    assert lib().disn_mesh_clean_workspace_bytes(1, 2 ** 31, 10) == 0
    assert lib().disn_mesh_clean_workspace_bytes(0, 10, 10) == 0


# ------------------------------------------------------------------ 9. the drivers
def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_create_sdf_clean_equals_the_two_step_route(tmp_path):
    import reconstruct_fixtures as RF
    from disn_amd import create_sdf as cs, evaluate, mesh_sdf, postprocess
    from disn_amd.engine import SdfEngine
    from disn_amd.weights import WeightStore
    cats = (("chair", "03001627"), ("car", "02958343"))
    objs = {"03001627": ["obj_a"], "02958343": ["obj_c"]}
    seed, view_num, R = 4, 2, 16
    entries = RF.expected_entries(seed, view_num, cats, objs)
    assert len(entries) == 4
    sdf_dir, rendered_dir = RF.build_dataset(str(tmp_path / "data"), entries)
    lst_dir, log_dir = str(tmp_path / "lst"), str(tmp_path / "ckpt")
    RF.write_lists(lst_dir, cats, objs)
    eng = SdfEngine(WeightStore.random_init(3))
    first = cs.load_group(entries[:view_num], sdf_dir, rendered_dir)
    iso = float(cs.create_sdf(eng, first["img"], first["trans_mat"], first["sdf_params"], R)[0].median())
    base = ["--log_dir", log_dir, "--random_init", "3", "--test_lst_dir", lst_dir, "--sdf_dir", sdf_dir,
            "--rendered_dir", rendered_dir, "--category", "chair,car", "--view_num", str(view_num), "--sdf_res", str(R),
            "--iso", repr(iso), "--seed", str(seed)]
    plain = cs.main(base)
    res = cs.main(base + ["--clean", "all"])
    assert res["out_dir"] == plain["out_dir"] + "_comb" and res["written"] == 4
    assert _tree(res["out_dir"]) == _tree(plain["out_dir"])
    # the two-step route on the plain files, mesh by mesh (where nothing is kept the file stays as it is)
    unclean = cleaned = 0
    for rel in _tree(plain["out_dir"]):
        src, two_step = os.path.join(plain["out_dir"], rel), str(tmp_path / "two_step" / rel)
        v, f = mesh_sdf.read_obj_mesh(src)
        want = open(src, "rb").read()
        if f.shape[0]:
            MF.assert_margins(v, f, 0.5, 0.3)
            os.makedirs(os.path.dirname(two_step), exist_ok=True)
            try:
                postprocess.clean_single_mesh(src, two_step, out=open(os.devnull, "w"))
                want = open(two_step, "rb").read()
                cleaned += 1
            except ValueError as e:
                assert "no part is kept" in str(e)
                unclean += 1
        assert open(os.path.join(res["out_dir"], rel), "rb").read() == want, rel
    assert res["unclean"] == unclean and cleaned + unclean + res["empty"] == 4 and cleaned + unclean >= 2
    # only the listed categories: the chairs as the plain run wrote them, the cars as above
    part = cs.main(base + ["--clean", "car", "--clean_dist_thresh", "0.5"])
    for rel in _tree(plain["out_dir"]):
        other = plain["out_dir"] if rel.startswith("03001627") else res["out_dir"]
        assert open(os.path.join(part["out_dir"], rel), "rb").read() == open(os.path.join(other, rel), "rb").read()
    # nothing is ever kept within distance 0: every mesh with triangles is written as it is and counted
    none = cs.main(base + ["--clean", "all", "--clean_dist_thresh", "0"])
    assert none["unclean"] == 4 - none["empty"] and none["empty"] == plain["empty"]
    for rel in _tree(plain["out_dir"]):
        assert open(os.path.join(none["out_dir"], rel), "rb").read() == open(os.path.join(plain["out_dir"], rel), "rb").read()
    # with refinement and normals: one vn line per vertex, faces within range, never more vertices than cleaned
    rn = cs.main(base + ["--clean", "all", "--refine", "1", "--normals"])
    for rel in _tree(rn["out_dir"]):
        lines = open(os.path.join(rn["out_dir"], rel)).read().splitlines()
        nv, nvn = sum(l.startswith("v ") for l in lines), sum(l.startswith("vn ") for l in lines)
        ids = [int(t.split("/")[0]) for l in lines if l.startswith("f ") for t in l.split()[1:]]
        ref = open(os.path.join(res["out_dir"], rel)).read().splitlines()
        assert nv == nvn == sum(l.startswith("v ") for l in ref)
        assert len(ids) == 3 * sum(l.startswith("f ") for l in ref)
        assert not ids or (min(ids) >= 1 and max(ids) <= nv)
    assert evaluate.CATS_CLEAN                                         # (the word --clean clean stands for)


def test_demo_clean(tmp_path):
    from PIL import Image
    from disn_amd import create_sdf as cs, demo, isosurface
    from disn_amd.engine import SdfEngine
    from disn_amd.weights import WeightStore
    from oracle import disn_oracle as O
    png = str(tmp_path / "view.png")
    Image.fromarray(np.random.default_rng(8).integers(0, 256, size=(137, 137, 4), dtype=np.uint8), "RGBA").save(png)
    img = demo.read_image(png)
    eng = SdfEngine(WeightStore.random_init(3))
    R, box = 16, [[-1, -1, -1, 1, 1, 1]]
    iso = float(cs.create_sdf(eng, img, O.DEMO_TRANS_MAT, box, R)[0].median())
    verts, faces = cs.reconstruct(eng, img, O.DEMO_TRANS_MAT, box, R, iso)[0]
    hv, hf = verts.cpu().numpy(), faces.cpu().numpy()
    out = str(tmp_path / "demo.obj")
    args = ["--img", png, "--log_dir", str(tmp_path / "none"), "--random_init", "3", "--sdf_res", str(R),
            "--iso", repr(iso), "--out", out, "--clean"]
    want = MF.host_clean(hv, hf, 0.5, 0.3)
    if want is None:                                                   # (this image's largest part lies far out)
        with pytest.raises(ValueError, match="no part is kept"):
            demo.main(args)
        want = MF.host_clean(hv, hf, 3.0, 0.3)
        args += ["--clean_dist_thresh", "3.0"]
    res = demo.main(args)
    assert res["verts"] == want[0].shape[0] and res["faces"] == want[1].shape[0]
    ref = str(tmp_path / "want.obj")
    isosurface.write_obj(ref, want[0], want[1])
    assert open(out, "rb").read() == open(ref, "rb").read()
    got = cs.reconstruct(eng, img, O.DEMO_TRANS_MAT, box, R, iso, clean=(3.0, 0.3, "face"))[0]
    w3 = MF.host_clean(hv, hf, 3.0, 0.3)
    assert np.array_equal(got[0].cpu().numpy(), w3[0]) and np.array_equal(got[1].cpu().numpy(), w3[1])

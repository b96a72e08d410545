"""Mesh simplification on the device (mesh_simplify.hip: disn_mesh_simplify_count_batch / _emit_batch;
``postprocess.simplify_meshes_device`` / ``simplify_arrays_device``) and the drivers' ``--simplify``.  The reference of
every comparison is the host function ``postprocess.simplify_arrays``, the specification: the integers (faces, vmap,
first) AND the position bits are compared for equality -- every sum is an integer sum, and the float64 operations of
the solve are restated in the host's order."""
import os

import numpy as np
import pytest
import torch

import mesh_simplify_fixtures as SF
from guarded_alloc import guarded

MF = SF.MF
pytestmark = pytest.mark.gpu


def _dev(v, f, *rest):
    return (torch.from_numpy(np.ascontiguousarray(v)).cuda(), torch.from_numpy(np.ascontiguousarray(f)).cuda()) + \
        tuple(torch.from_numpy(np.ascontiguousarray(r)).cuda() for r in rest)


def _equal_to_host(got, maps, want, what=""):
    """one mesh of ``simplify_meshes_device`` against ``simplify_arrays``' quadruple"""
    gv, gf, vmap, first = (t.cpu().numpy() for t in (got[0], got[1], maps[0], maps[1]))
    assert gv.dtype == np.float32 and gf.dtype == np.int32 and vmap.dtype == np.int32 and first.dtype == np.int32
    assert np.array_equal(vmap, want[2]), what
    assert np.array_equal(first, want[3]), what
    assert gf.shape == want[1].shape and np.array_equal(gf, want[1]), what
    assert gv.shape == want[0].shape, what
    differ = np.nonzero((gv.view(np.uint32) != np.ascontiguousarray(want[0]).view(np.uint32)).any(1))[0]
    assert differ.size == 0, "%s: %d of %d positions differ in their bits, first %s device %r host %r" % (
        what, differ.size, gv.shape[0], differ[:1], gv[differ[:1]], want[0][differ[:1]])


# ------------------------------------------------------------------ 1. the device against the specification
@pytest.mark.parametrize("name", ["fans", "soup 40 30", "soup 300 150", "soup 2000 1500", "soup 50 400",
                                  "soup 50 4000", "strip", "crowd", "box", "field_grid"])
def test_device_equals_simplify_arrays(name):
    from disn_amd import postprocess
    v, f, box, cells = SF.device_cases()[name]
    want = SF.host_simplify(name)
    simplified, maps = postprocess.simplify_meshes_device([_dev(v, f)], [box], cells)
    _equal_to_host(simplified[0], maps[0], want, name)
    if name == "crowd":
        assert v.shape[0] == 15162 and want[0].shape[0] > 1000          # vertices and clusters over several scan blocks
    if name in ("soup 50 4000", "fans"):
        nd = SF.host_simplify(name, dedup=False)
        qv, qf, vmap, first = postprocess.simplify_arrays_device(*_dev(v, f), box, cells, dedup=False)
        _equal_to_host((qv, qf), (vmap, first), nd, name + " without dedup")
        assert nd[1].shape[0] > want[1].shape[0] or name == "fans"


# ------------------------------------------------------------------ 2. a batch, each mesh on its own lattice, twice
def test_batch_of_five_equals_every_mesh_alone_and_repeats():
    from disn_amd import postprocess
    meshes = MF.batch_of_five()
    boxes, cells = np.stack(SF.BATCH_BOXES), list(SF.BATCH_CELLS)
    run = lambda: postprocess.simplify_meshes_device([_dev(v, f) for v, f in meshes], boxes, cells)
    simplified, maps = run()
    again, maps_again = run()
    assert len(simplified) == 5
    for b, (v, f) in enumerate(meshes):
        want = postprocess.simplify_arrays(v, f, boxes[b], cells[b])
        _equal_to_host(simplified[b], maps[b], want, "mesh %d" % b)
        alone, maps_alone = postprocess.simplify_meshes_device([_dev(v, f)], boxes[b:b + 1], cells[b])
        for other, m in ((alone[0], maps_alone[0]), (again[b], maps_again[b])):
            assert torch.equal(other[0].view(torch.int32), simplified[b][0].view(torch.int32)), b
            assert torch.equal(other[1], simplified[b][1]) and torch.equal(m[0], maps[b][0]) and torch.equal(m[1], maps[b][1])
    assert simplified[2][0].shape == (0, 3) and simplified[2][1].shape == (0, 3)         # the empty mesh stays empty
    assert maps[2][0].numel() == 0 and maps[2][1].numel() == 0
    assert postprocess.simplify_meshes_device([], np.zeros((0, 6)), 4) == ([], [])


# ------------------------------------------------------------------ 3. the project's own marching cubes, in place
def test_meshes_of_the_batched_marching_cubes_with_carried_arrays():
    from disn_amd import isosurface, postprocess
    R = 16
    grids = [MF.field_grid(R, k) for k in range(3)]
    sdf = torch.from_numpy(np.stack([g[0].reshape(-1) for g in grids])).cuda()
    boxes = np.stack([g[1] for g in grids])
    meshes = isosurface.marching_cubes_batch(sdf, boxes, R, 0.0)
    whole, off = postprocess._pack([m[0] for m in meshes], torch.float32, "verts")
    assert whole.data_ptr() == meshes[0][0].data_ptr(), "the views are taken in place"
    carried = [(v, f, torch.arange(v.shape[0], device=v.device, dtype=torch.float32)[:, None].repeat(1, 3))
               for v, f in meshes]
    simplified, maps = postprocess.simplify_meshes_device(carried, boxes, 8)
    for b, (v, f) in enumerate(meshes):
        hv, hf = v.cpu().numpy(), f.cpu().numpy()
        want = postprocess.simplify_arrays(hv, hf, boxes[b], 8)
        assert 0 < want[1].shape[0] < hf.shape[0] // 2
        _equal_to_host(simplified[b], maps[b], want, "grid %d" % b)
        src = simplified[b][2].cpu().numpy()
        assert src.shape == want[0].shape and (src[:, 0] == src[:, 1]).all() and (src[:, 0] == src[:, 2]).all()
        assert np.array_equal(src[:, 0].astype(np.int64), want[3])       # the array rode along `first`


# ------------------------------------------------------------------ 4. statuses that cannot fault
def _raw(meshes, boxes, cells, dedup=1):
    """the C entries on host meshes -> (sizes [B,4], per mesh (verts, faces, vmap, first))"""
    from disn_amd import ops, postprocess
    from disn_amd._lib import check, lib
    h = lib()
    B = len(meshes)
    v_off, f_off = np.zeros(B + 1, np.int64), np.zeros(B + 1, np.int64)
    v_off[1:] = np.cumsum([m[0].shape[0] for m in meshes])
    f_off[1:] = np.cumsum([m[1].shape[0] for m in meshes])
    v, f = _dev(np.concatenate([m[0] for m in meshes]), np.concatenate([m[1] for m in meshes]))
    lattice = np.array([np.append(*postprocess.simplify_lattice(boxes[b], cells[b])) for b in range(B)], np.float64)
    cells_h = np.asarray(cells, np.int32)
    ws = torch.empty(h.disn_mesh_simplify_workspace_bytes(B, int(v_off[-1]), int(f_off[-1])), dtype=torch.uint8,
                     device="cuda")
    counts = torch.full((B, 4), -7, dtype=torch.int64, device="cuda")
    st = ops._stream()
    check("count", h.disn_mesh_simplify_count_batch(v.data_ptr(), f.data_ptr(), v_off.ctypes.data, f_off.ctypes.data,
                                                    lattice.ctypes.data, cells_h.ctypes.data, B, dedup,
                                                    counts.data_ptr(), ws.data_ptr(), ws.numel(), st))
    sizes = np.ascontiguousarray(counts.cpu().numpy())
    nv, nf = int(sizes[:, 0].sum()), int(sizes[:, 1].sum())
    ov = torch.full((nv, 3), 7.0, dtype=torch.float32, device="cuda")
    of = torch.full((nf, 3), -7, dtype=torch.int32, device="cuda")
    vm = torch.full((int(v_off[-1]),), -7, dtype=torch.int32, device="cuda")
    fi = torch.full((nv,), -7, dtype=torch.int32, device="cuda")
    check("emit", h.disn_mesh_simplify_emit_batch(v.data_ptr(), f.data_ptr(), v_off.ctypes.data, f_off.ctypes.data, B,
                                                  sizes.ctypes.data, ov.data_ptr(), of.data_ptr(), vm.data_ptr(),
                                                  fi.data_ptr(), ws.data_ptr(), ws.numel(), st))
    out, v0, f0 = [], 0, 0
    for b in range(B):
        nvb, nfb = int(sizes[b, 0]), int(sizes[b, 1])
        out.append((ov[v0:v0 + nvb].cpu().numpy(), of[f0:f0 + nfb].cpu().numpy(),
                    vm[int(v_off[b]):int(v_off[b + 1])].cpu().numpy(), fi[v0:v0 + nvb].cpu().numpy()))
        v0, f0 = v0 + nvb, f0 + nfb
    return sizes, out


def _same(got, want):
    return (np.array_equal(got[0].view(np.uint32), np.ascontiguousarray(want[0]).view(np.uint32))
            and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]))


def test_a_bad_mesh_gets_its_status_and_leaves_its_neighbours_alone():
    """status 2: the bad index equals its mesh's own nv -- with the bad mesh first that slot exists in the shared vertex
    buffer (the next mesh's first vertex), and no kernel addresses anything through an index of a mesh with a status;
    status 4: one NaN coordinate.  Nothing here could read outside an allocation."""
    from disn_amd import postprocess
    v0, f0 = MF.fans()
    bad_f = f0.copy()
    bad_f[2, 1] = v0.shape[0]
    bad_v = v0.copy()
    bad_v[3, 2] = np.nan
    v1, f1 = (np.ascontiguousarray(a, d) for a, d in zip(MF.icosphere(0.3, 1), (np.float32, np.int32)))
    boxes, cells = [SF.UNIT, SF.UNIT, SF.UNIT], [16, 6, 16]
    want0 = postprocess.simplify_arrays(v0, f0, SF.UNIT, 16)
    want1 = postprocess.simplify_arrays(v1, f1, SF.UNIT, 6)
    dropped1 = postprocess.simplify_arrays(v1, f1, SF.UNIT, 6, dedup=False)[1].shape[0] - want1[1].shape[0]
    for bad, status in (((v0, bad_f), 2), ((bad_v, f0), 4)):
        for order in ((0, 1, 2), (1, 2, 0)):                       # the bad mesh first, and last
            trio = [bad, (v1, f1), (v0, f0)]
            sizes, out = _raw([trio[k] for k in order], [boxes[k] for k in order], [cells[k] for k in order])
            at = {k: i for i, k in enumerate(order)}
            assert sizes[at[0]].tolist() == [0, 0, 0, status]
            assert (out[at[0]][2] == -1).all() and out[at[0]][0].shape == (0, 3) and out[at[0]][1].shape == (0, 3)
            assert sizes[at[1]].tolist() == [want1[0].shape[0], want1[1].shape[0], dropped1, 0]
            assert sizes[at[2]].tolist() == [want0[0].shape[0], want0[1].shape[0], 0, 0]
            assert _same(out[at[1]], want1) and _same(out[at[2]], want0)
    with pytest.raises(ValueError, match="mesh 0: face index out of range"):
        postprocess.simplify_meshes_device([_dev(v0, bad_f), _dev(v1, f1)], [SF.UNIT, SF.UNIT], 8)
    with pytest.raises(ValueError, match="mesh 1: a vertex coordinate is not finite"):
        postprocess.simplify_meshes_device([_dev(v1, f1), _dev(bad_v, f0)], [SF.UNIT, SF.UNIT], 8)
    with pytest.raises(ValueError, match="^face index out of range"):
        postprocess.simplify_arrays_device(*_dev(v0, bad_f), SF.UNIT, 8)
    with pytest.raises(ValueError, match="1..1024"):
        postprocess.simplify_arrays_device(*_dev(v0, f0), SF.UNIT, 0)
    with pytest.raises(TypeError):
        postprocess.simplify_meshes_device([(v0, f0)], [SF.UNIT], 8)             # host arrays: no CPU fallback


# ------------------------------------------------------------------ 5. the memory contract of the three entries
def _contract_scenario(g):
    from disn_amd import postprocess
    out = {}
    ico = MF.icosphere(0.4, 1)
    meshes = [MF.fans(), (np.zeros((3, 3), np.float32), np.zeros((0, 3), np.int32)),
              (np.ascontiguousarray(ico[0], np.float32), np.ascontiguousarray(ico[1], np.int32)), MF.soup(50, 400)]
    boxes, cells = [SF.UNIT, SF.UNIT, SF.UNIT, SF.SOUP_BOX], [16, 4, 5, 4]
    dev = [(g.put(v), g.put(f) if len(f) else torch.from_numpy(f).cuda()) for v, f in meshes]
    simplified, maps = postprocess.simplify_meshes_device(dev, boxes, cells)
    for k in range(len(meshes)):
        out["v%d" % k], out["f%d" % k] = simplified[k][0].cpu().numpy(), simplified[k][1].cpu().numpy()
        out["vmap%d" % k], out["first%d" % k] = maps[k][0].cpu().numpy(), maps[k][1].cpu().numpy()
    v, f = meshes[3]
    one = postprocess.simplify_arrays_device(g.put(v), g.put(f), boxes[3], cells[3], dedup=False)
    for key, t in zip(("v", "f", "vmap", "first"), one):
        out["nodedup " + key] = t.cpu().numpy()

    def verify(r):
        for k, (v, f) in enumerate(meshes):
            want = postprocess.simplify_arrays(v, f, boxes[k], cells[k])
            assert _same((r["v%d" % k], r["f%d" % k], r["vmap%d" % k], r["first%d" % k]), want), k
        want = postprocess.simplify_arrays(*meshes[3], boxes[3], cells[3], dedup=False)
        assert _same(tuple(r["nodedup " + key] for key in ("v", "f", "vmap", "first")), want)
        assert r["f3"].shape[0] < r["nodedup f"].shape[0]
    return out, verify


# the entries of include/disn_amd_simplify.h (tests/test_guarded_alloc_host.py reads this tuple)
NEW = ("disn_mesh_simplify_workspace_bytes", "disn_mesh_simplify_count_batch", "disn_mesh_simplify_emit_batch")


def test_memory_contract_of_the_simplify_entries():
    """in the manner of test_gpu_memory_contract.py: every buffer the wrapper hands over (the workspace too) lies
    between guard bands and starts out poisoned; guards intact, const inputs unchanged, runs A and B bit-identical
    (no tolerance: there is no float atomic), every entry really called"""
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


# ------------------------------------------------------------------ 6. the drivers
def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_create_sdf_simplify_equals_reconstruct_then_simplify(tmp_path):
    import reconstruct_fixtures as RF
    from disn_amd import create_sdf as cs, isosurface, postprocess
    from disn_amd.engine import SdfEngine
    from disn_amd.weights import WeightStore
    cats = (("chair", "03001627"), ("car", "02958343"))
    objs = {"03001627": ["obj_a"], "02958343": ["obj_c"]}
    seed, view_num, R, cells = 4, 2, 8, 4
    entries = RF.expected_entries(seed, view_num, cats, objs)
    assert len(entries) == 4
    sdf_dir, rendered_dir = RF.build_dataset(str(tmp_path / "data"), entries)
    lst_dir, log_dir = str(tmp_path / "lst"), str(tmp_path / "ckpt")
    RF.write_lists(lst_dir, cats, objs)
    eng = SdfEngine(WeightStore.random_init(3))
    groups = [cs.load_group(entries[i:i + view_num], sdf_dir, rendered_dir) for i in range(0, 4, view_num)]
    iso = float(cs.create_sdf(eng, groups[0]["img"], groups[0]["trans_mat"], groups[0]["sdf_params"], R)[0].median())
    base = ["--log_dir", log_dir, "--random_init", "3", "--test_lst_dir", lst_dir, "--sdf_dir", sdf_dir,
            "--rendered_dir", rendered_dir, "--category", "chair,car", "--view_num", str(view_num), "--sdf_res", str(R),
            "--iso", repr(iso), "--seed", str(seed)]
    res = cs.main(base + ["--simplify", str(cells)])
    assert res["out_dir"] == cs.result_obj_path(log_dir, R, iso) + "_s4" and res["written"] == 4
    assert res["simplified"] == 4 - res["empty"] and "unclean" not in res
    smaller = 0
    for gi, batch in enumerate(groups):
        args = (batch["img"], batch["trans_mat"], batch["sdf_params"], R, iso)
        plain = cs.reconstruct(eng, *args)
        boxes = np.asarray(batch["sdf_params"], np.float64).reshape(-1, 6)
        have = [b for b, m in enumerate(plain) if len(m[1])]
        two_step = list(plain)
        for b, m in zip(have, postprocess.simplify_meshes_device([plain[b] for b in have], boxes[have], cells)[0]):
            two_step[b] = m
        one_call = cs.reconstruct(eng, *args, simplify=cells)
        for b, e in enumerate(entries[gi * view_num:(gi + 1) * view_num]):
            assert torch.equal(one_call[b][0], two_step[b][0]) and torch.equal(one_call[b][1], two_step[b][1])
            ref = str(tmp_path / "want.obj")
            isosurface.write_obj(ref, two_step[b][0], two_step[b][1])
            assert open(cs.obj_path(res["out_dir"], *e), "rb").read() == open(ref, "rb").read(), e
            smaller += len(two_step[b][1]) < len(plain[b][1])
            if len(plain[b][1]):                                       # the host rule on the device's own mesh
                want = postprocess.simplify_arrays(plain[b][0], plain[b][1], boxes[b], cells)
                assert np.array_equal(two_step[b][0].cpu().numpy().view(np.uint32), want[0].view(np.uint32))
                assert np.array_equal(two_step[b][1].cpu().numpy(), want[1])
        # refinement behind the simplification: same faces, no vertex further from the level set than before
        enc = eng.encode(batch["img"])
        refined = cs.reconstruct(eng, *args, refine=2, simplify=cells)
        for b in range(len(plain)):
            assert torch.equal(refined[b][1], one_call[b][1]) and refined[b][0].shape == one_call[b][0].shape
            if not len(one_call[b][0]):
                continue
            r0 = eng.refine_vertices(enc, b, batch["trans_mat"], one_call[b][0], iso=iso, iters=0)[2].cpu().numpy()
            r1 = eng.refine_vertices(enc, b, batch["trans_mat"], refined[b][0], iso=iso, iters=0)[2].cpu().numpy()
            print("group %d view %d: %d vertices, |pred/10 - iso| median %.3g -> %.3g, max %.3g -> %.3g"
                  % (gi, b, len(r0), np.median(r0) / 10, np.median(r1) / 10, r0.max() / 10, r1.max() / 10))
            assert (r1 <= r0).all() and r1.max() <= r0.max()
    assert smaller >= 2, "the fixture's meshes are simplified at all"
    # with the cleanup, the refinement and the normals: the _comb_s4 tree, one vn line per vertex, faces within range
    rn = cs.main(base + ["--simplify", str(cells), "--clean", "all", "--refine", "2", "--normals"])
    assert rn["out_dir"] == cs.result_obj_path(log_dir, R, iso) + "_comb_s4" and rn["written"] == 4
    assert rn["simplified"] == 4 - rn["empty"] and "unclean" in rn
    assert _tree(rn["out_dir"]) == _tree(res["out_dir"])
    for rel in _tree(rn["out_dir"]):
        lines = open(os.path.join(rn["out_dir"], rel)).read().splitlines()
        nv, nvn = sum(l.startswith("v ") for l in lines), sum(l.startswith("vn ") for l in lines)
        ids = [int(t.split("/")[0]) for l in lines if l.startswith("f ") for t in l.split()[1:]]
        assert nv == nvn and (not ids or (min(ids) >= 1 and max(ids) <= nv))
        plain_nv = sum(l.startswith("v ") for l in open(os.path.join(res["out_dir"], rel)))
        assert nv <= plain_nv                                          # cleaned first: never more clusters


def test_demo_simplify_writes_a_smaller_file(tmp_path):
    from PIL import Image
    from disn_amd import create_sdf as cs, demo, isosurface, postprocess
    from disn_amd.engine import SdfEngine
    from disn_amd.weights import WeightStore
    from oracle import disn_oracle as O
    png = str(tmp_path / "view.png")
    Image.fromarray(np.random.default_rng(8).integers(0, 256, size=(137, 137, 4), dtype=np.uint8), "RGBA").save(png)
    img = demo.read_image(png)
    eng = SdfEngine(WeightStore.random_init(3))
    R, box = 16, [[-1, -1, -1, 1, 1, 1]]
    iso = float(cs.create_sdf(eng, img, O.DEMO_TRANS_MAT, box, R)[0].median())
    args = ["--img", png, "--log_dir", str(tmp_path / "none"), "--random_init", "3", "--sdf_res", str(R),
            "--iso", repr(iso)]
    plain = demo.main(args + ["--out", str(tmp_path / "plain.obj")])
    small = demo.main(args + ["--out", str(tmp_path / "small.obj"), "--simplify", "8"])
    assert 0 < small["faces"] < plain["faces"] and 0 < small["verts"] < plain["verts"]
    assert os.path.getsize(small["out"]) < os.path.getsize(plain["out"])
    verts, faces = cs.reconstruct(eng, img, O.DEMO_TRANS_MAT, box, R, iso)[0]
    want = postprocess.simplify_arrays(verts, faces, box[0], 8)
    ref = str(tmp_path / "want.obj")
    isosurface.write_obj(ref, want[0], want[1])
    assert open(small["out"], "rb").read() == open(ref, "rb").read()

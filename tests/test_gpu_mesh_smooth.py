"""Taubin smoothing on the device (mesh_smooth.hip: disn_mesh_smooth_batch; ``postprocess.smooth_meshes_device`` /
``smooth_arrays_device``) and the drivers' ``--smooth``.  The reference of every comparison is the host function
``postprocess.smooth_arrays``, the specification: the position BITS are compared for equality, with no tolerance -- every
sum is an integer sum, and the float64 operations of a step are + - x / in the host's order."""
import os

import numpy as np
import pytest
import torch

import mesh_smooth_fixtures as XF
from guarded_alloc import guarded

pytestmark = pytest.mark.gpu

CASES = ["sphere", "noisy", "patch", "messy", "empty", "mc_sphere", "mc_cut"]


def _dev(v, f, *rest):
    return (torch.from_numpy(np.ascontiguousarray(v)).cuda(), torch.from_numpy(np.ascontiguousarray(f)).cuda()) + \
        tuple(torch.from_numpy(np.ascontiguousarray(r)).cuda() for r in rest)


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _mc_device():
    """the two 17^3 meshes as the batched mesher leaves them: device views of one allocation, computed once"""
    def make():
        from disn_amd import isosurface
        sdf = torch.from_numpy(XF.mc_fields()).cuda()
        return isosurface.marching_cubes_batch(sdf, np.stack([XF.MC_BOX, XF.MC_BOX]), XF.MC_R, 0.0)
    return XF.cached("smooth mc device", make)


def _case(name):
    """-> (verts, faces) on the host"""
    if name.startswith("mc_"):
        v, f = _mc_device()[0 if name == "mc_sphere" else 1]
        return XF.cached(("smooth mc host", name), lambda: (v.cpu().numpy(), f.cpu().numpy()))
    return XF.host_cases()[name]


def _want(name, iters, pin, cap):
    return XF.host_smooth(name, iters, pin, cap, mesh=_case(name))


def _assert_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, what
    differ = np.nonzero((g != w).any(1))[0]
    assert differ.size == 0, "%s: %d of %d positions differ in their bits, first %s device %r host %r" % (
        what, differ.size, g.shape[0], differ[:1], np.asarray(got.cpu())[differ[:1]], want[differ[:1]])


# ------------------------------------------------------------------ 1. the device against the specification
@pytest.mark.parametrize("cap", [None, 0.01])
@pytest.mark.parametrize("pin", [0, 1])
@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("name", CASES)
def test_device_equals_smooth_arrays(name, iters, pin, cap):
    from disn_amd import postprocess
    v, f = _case(name)
    want = _want(name, iters, pin, cap)
    out, status = postprocess.smooth_meshes_device([_dev(v, f)], iters=iters, pin_boundary=bool(pin), max_move=cap)
    assert status.tolist() == [0] and status.dtype == np.int32
    assert out[0][0].dtype == torch.float32 and out[0][1].dtype == torch.int32
    assert np.array_equal(out[0][1].cpu().numpy(), f)                      # the faces as they were given
    _assert_bits(out[0][0], want, "%s iters %d pin %d cap %r" % (name, iters, pin, cap))
    if name != "empty":
        assert (_bits(want) != _bits(v)).any() and len(v) > 0              # something moved at all
        one = postprocess.smooth_arrays_device(*_dev(v, f), iters=iters, pin_boundary=bool(pin), max_move=cap)
        _assert_bits(one, want, name + " (one mesh)")
    if name.startswith("mc_"):
        assert len(f) > 300


# ------------------------------------------------------------------ 2. a batch, every mesh alone, twice, permuted
def test_batch_equals_every_mesh_alone_and_repeats():
    from disn_amd import postprocess
    names = ["noisy", "messy", "empty", "patch", "mc_cut"]
    meshes = [_case(n) for n in names]
    caps = [0.01, 0.02, 0.5, 0.003, 0.01]
    kw = {"iters": 3, "pin_boundary": True}
    run = lambda ms, cs: postprocess.smooth_meshes_device([_dev(v, f) for v, f in ms], max_move=cs, **kw)
    out, status = run(meshes, caps)
    again, status_again = run(meshes, caps)
    assert status.tolist() == [0] * 5 == status_again.tolist() and len(out) == 5
    assert out[2][0].shape == (0, 3) and out[2][1].shape == (0, 3)          # the empty mesh stays empty
    for b, (v, f) in enumerate(meshes):
        want = postprocess.smooth_arrays(v, f, max_move=caps[b], **kw)
        _assert_bits(out[b][0], want, "mesh %d in the batch" % b)
        _assert_bits(again[b][0], want, "mesh %d in the second call" % b)
        alone, _ = run([(v, f)], caps[b])
        _assert_bits(alone[0][0], want, "mesh %d alone" % b)
    # at any position: the batch reversed, the empty mesh no longer in the middle
    order = [4, 2, 0, 3, 1]
    moved, _ = run([meshes[k] for k in order], [caps[k] for k in order])
    for at, k in enumerate(order):
        assert np.array_equal(_bits(moved[at][0]), _bits(out[k][0])), (at, k)
    # face-permuted copies: the same bits
    perm, _ = run([XF.permuted(v, f, 3) if len(f) else (v, f) for v, f in meshes], caps)
    for b in range(5):
        assert np.array_equal(_bits(perm[b][0]), _bits(out[b][0])), b
    assert postprocess.smooth_meshes_device([])[0] == []
    # further arrays ride along untouched
    v, f = meshes[0]
    extra = torch.arange(len(v), device="cuda", dtype=torch.float32)
    carried, _ = postprocess.smooth_meshes_device([_dev(v, f) + (extra,)], max_move=caps[0], **kw)
    assert carried[0][2] is extra and np.array_equal(_bits(carried[0][0]), _bits(out[0][0]))


# ------------------------------------------------------------------ 3. statuses that cannot fault
def test_a_bad_mesh_gets_its_status_and_leaves_its_neighbours_alone():
    """status 2: the bad index equals its mesh's own nv -- with a mesh behind it that slot exists in the shared vertex
    buffer, and no kernel addresses anything through an index of a mesh with a status; status 4: one NaN coordinate;
    status 7: a coordinate of 2000, and the spike whose second step leaves +-1024.  Nothing here could read outside an
    allocation: the first kernel compares every index before anything dereferences it."""
    from disn_amd import postprocess
    v, f = XF.messy()
    bad_f = f.copy()
    bad_f[3, 1] = len(v)
    nan = v.copy()
    nan[4, 1] = np.nan
    far = v.copy()
    far[1, 2] = 2000.0
    good = [XF.patch(), XF.noisy()]
    kw = dict(XF.SPIKE_KW, pin_boundary=True)
    meshes = [(v, bad_f), good[0], (nan, f), (far, f), good[1], XF.spike(), (v, f)]
    want_status = [2, 0, 4, 7, 0, 7, 0]
    assert [postprocess.smooth_arrays_status(mv, mf, **kw)[1] for mv, mf in meshes] == want_status
    for order in (list(range(7)), [6, 5, 4, 3, 2, 1, 0]):
        out, status = postprocess.smooth_meshes_device([_dev(*meshes[k]) for k in order], strict=False, **kw)
        assert status.tolist() == [want_status[k] for k in order]
        for at, k in enumerate(order):
            mv, mf = meshes[k]
            if want_status[k]:
                assert np.array_equal(_bits(out[at][0]), _bits(mv)), "a mesh with a status keeps its input vertices"
            else:
                alone, _ = postprocess.smooth_meshes_device([_dev(mv, mf)], **kw)
                assert np.array_equal(_bits(out[at][0]), _bits(alone[0][0]))
                _assert_bits(out[at][0], postprocess.smooth_arrays(mv, mf, **kw), "good mesh %d" % k)
    with pytest.raises(ValueError, match="mesh 0: face index out of range"):
        postprocess.smooth_meshes_device([_dev(v, bad_f), _dev(*good[0])], **kw)
    with pytest.raises(ValueError, match="mesh 1: a vertex coordinate is not finite"):
        postprocess.smooth_meshes_device([_dev(*good[0]), _dev(nan, f)], **kw)
    with pytest.raises(ValueError, match="mesh 2: a coordinate leaves"):
        postprocess.smooth_meshes_device([_dev(*good[0]), _dev(v, f), _dev(*XF.spike())], **kw)
    with pytest.raises(ValueError, match="^a coordinate leaves"):
        postprocess.smooth_arrays_device(*_dev(far, f))
    with pytest.raises(ValueError, match="iters"):
        postprocess.smooth_arrays_device(*_dev(v, f), iters=0)
    with pytest.raises(ValueError, match="max_move"):
        postprocess.smooth_meshes_device([_dev(v, f)], max_move=[0.1, 0.2])
    with pytest.raises(TypeError):
        postprocess.smooth_meshes_device([(v, f)])                          # host arrays: no CPU fallback


# ------------------------------------------------------------------ 4. the memory contract of the two entries
def _raw(v, f, v_off, f_off, cap, out, status, ws, ws_bytes, iters=2, pin=1):
    from disn_amd import _lib, ops
    rc = _lib.lib().disn_mesh_smooth_batch(v.data_ptr(), f.data_ptr(), v_off.ctypes.data, f_off.ctypes.data,
                                           len(v_off) - 1, iters, 0.5, -0.53, pin, None if cap is None else cap.ctypes.data,
                                           out.data_ptr(), status.data_ptr(), ws.data_ptr(), ws_bytes, ops._stream())
    torch.cuda.synchronize()
    return rc


def test_memory_contract_of_the_smooth_entries():
    """every buffer the wrapper hands over (the workspace too, exactly as large as disn_mesh_smooth_workspace_bytes
    says) lies between guard bands and starts out poisoned; guards intact, const inputs unchanged, runs A and B
    bit-identical and equal to the rule; one byte less of workspace: DISN_E_WS and nothing written"""
    from disn_amd import _lib, postprocess
    names = ["noisy", "messy", "patch", "mc_sphere"]
    parts = [_case(n) for n in names]
    caps = [0.01, 0.02, 0.003, 0.01]
    results = {}
    for variant in ("A", "B"):
        with guarded(variant) as g:
            with g.recording() as called:
                # one guarded allocation sliced into views: the call reads the frozen inputs in place
                verts, faces = g.put(np.concatenate([m[0] for m in parts])), g.put(np.concatenate([m[1] for m in parts]))
                v_off = np.cumsum([0] + [len(m[0]) for m in parts]).astype(np.int64)
                f_off = np.cumsum([0] + [len(m[1]) for m in parts]).astype(np.int64)
                views = [(verts[v_off[k]:v_off[k + 1]], faces[f_off[k]:f_off[k + 1]]) for k in range(len(parts))]
                assert postprocess._pack([m[0] for m in views], torch.float32, "verts")[0].data_ptr() == verts.data_ptr()
                out, status = postprocess.smooth_meshes_device(views, iters=2, max_move=caps)
                # a batch with an empty mesh and a bad one (a concatenated copy of guarded inputs)
                v, f = XF.messy()
                bad_f = f.copy()
                bad_f[0, 0] = -1
                mixed = [(g.put(v), g.put(f)), _dev(*XF.empty()), (g.put(v), g.put(bad_f)), (g.put(parts[2][0]), g.put(parts[2][1]))]
                mixed_out, mixed_status = postprocess.smooth_meshes_device(mixed, iters=2, pin_boundary=False, strict=False)
                # the entry itself with one byte less than it asks for
                need = _lib.lib().disn_mesh_smooth_workspace_bytes(len(parts), int(v_off[-1]), int(f_off[-1]))
                ws = torch.empty(need, dtype=torch.uint8, device="cuda")
                o2 = torch.empty((int(v_off[-1]), 3), dtype=torch.float32, device="cuda")
                s2 = torch.empty(len(parts), dtype=torch.int32, device="cuda")
                before = [t.clone() for t in (ws, o2.view(torch.uint8), s2.view(torch.uint8))]
                cap = np.asarray(caps, np.float64)
                assert _raw(verts, faces, v_off, f_off, cap, o2, s2, ws, need - 1) == -3
                for t, b in zip((ws, o2.view(torch.uint8), s2.view(torch.uint8)), before):
                    assert torch.equal(t, b), "a refused call writes nothing"
                assert _raw(verts, faces, v_off, f_off, cap, o2, s2, ws, need) == 0
            g.check()
            assert set(NEW) <= set(called)
            assert len(g.records) >= 5
            assert status.tolist() == [0] * 4 and mixed_status.tolist() == [0, 0, 2, 0] and s2.cpu().tolist() == [0] * 4
            results[variant] = [o[0].cpu().numpy() for o in out] + [o[0].cpu().numpy() for o in mixed_out] + [o2.cpu().numpy()]
    a, b = results["A"], results["B"]
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), "results depend on what the buffers held before"
    for k, (v, f) in enumerate(parts):
        _assert_bits(torch.from_numpy(a[k]), postprocess.smooth_arrays(v, f, iters=2, max_move=caps[k]), names[k])
    v, f = XF.messy()
    _assert_bits(torch.from_numpy(a[4]), postprocess.smooth_arrays(v, f, iters=2, pin_boundary=False), "messy, free")
    assert a[5].shape == (0, 3) and np.array_equal(_bits(a[6]), _bits(v))   # the bad mesh: its input
    _assert_bits(torch.from_numpy(a[7]), postprocess.smooth_arrays(*parts[2], iters=2, pin_boundary=False), "patch, free")
    assert np.array_equal(_bits(a[8]), _bits(np.concatenate(a[:4])))


NEW = ("disn_mesh_smooth_workspace_bytes", "disn_mesh_smooth_batch")


# ------------------------------------------------------------------ 5. the project's own marching cubes, in place
def test_meshes_of_the_batched_marching_cubes():
    from disn_amd import postprocess
    meshes = _mc_device()
    whole, off = postprocess._pack([m[0] for m in meshes], torch.float32, "verts")
    assert whole.data_ptr() == meshes[0][0].data_ptr(), "the views are taken in place"
    cell = 1.0 / XF.MC_R
    out, status = postprocess.smooth_meshes_device(meshes, iters=3, max_move=0.5 * cell)
    assert status.tolist() == [0, 0]
    for b, name in enumerate(("mc_sphere", "mc_cut")):
        v, f = _case(name)
        want = postprocess.smooth_arrays(v, f, iters=3, max_move=0.5 * cell)
        _assert_bits(out[b][0], want, name)
        assert torch.equal(out[b][1], meshes[b][1])
        boundary = postprocess.smooth_graph(f, len(v))[2]
        moved = (_bits(want) != _bits(v)).any(1)
        if name == "mc_sphere":
            assert not boundary.any() and moved.mean() > 0.9                # closed: everything is free
        else:
            got = out[b][0].cpu().numpy()
            assert 16 < boundary.sum() < len(v) // 2 and moved[~boundary].mean() > 0.9
            assert np.array_equal(_bits(got)[boundary], _bits(v)[boundary])
            assert (np.abs(v[boundary, 0] - 0.5) <= 1e-6).all() and (np.abs(got[boundary, 0] - 0.5) <= 1e-6).all()
            assert (v[:, 0] <= 0.5 + 1e-6).all()                            # the mesh ends on the face x = 0.5 of the grid box


# ------------------------------------------------------------------ 6. the drivers
def test_create_sdf_smooth_equals_reconstruct_then_smooth(tmp_path):
    import reconstruct_fixtures as RF
    from disn_amd import create_sdf as cs, isosurface, postprocess
    from disn_amd.engine import SdfEngine
    from disn_amd.weights import WeightStore
    cats = (("chair", "03001627"),)
    objs = {"03001627": ["obj_a"]}
    seed, view_num, R, iters, cells = 4, 2, 16, 3, 6
    entries = RF.expected_entries(seed, view_num, cats, objs)
    assert len(entries) == 2
    sdf_dir, rendered_dir = RF.build_dataset(str(tmp_path / "data"), entries)
    lst_dir, log_dir = str(tmp_path / "lst"), str(tmp_path / "ckpt")
    RF.write_lists(lst_dir, cats, objs)
    eng = SdfEngine(WeightStore.random_init(3))
    batch = cs.load_group(entries, sdf_dir, rendered_dir)
    iso = float(cs.create_sdf(eng, batch["img"], batch["trans_mat"], batch["sdf_params"], R)[0].median())
    args = (batch["img"], batch["trans_mat"], batch["sdf_params"], R, iso)
    boxes = np.asarray(batch["sdf_params"], np.float64).reshape(-1, 6)
    cap = 0.5 * (boxes[:, 3:] - boxes[:, :3]).max(1) / R
    plain = cs.reconstruct(eng, *args)
    for m, p in zip(cs.reconstruct(eng, *args, smooth=None), plain):        # without it: the bits of today
        assert torch.equal(m[0].view(torch.int32), p[0].view(torch.int32)) and torch.equal(m[1], p[1])
    smoothed = cs.reconstruct(eng, *args, smooth=iters)
    moved = 0
    for b in range(len(plain)):
        assert torch.equal(smoothed[b][1], plain[b][1])                     # the faces of the unsmoothed run
        if not len(plain[b][1]):
            assert torch.equal(smoothed[b][0], plain[b][0])
            continue
        v, f = plain[b][0].cpu().numpy(), plain[b][1].cpu().numpy()
        _assert_bits(smoothed[b][0], postprocess.smooth_arrays(v, f, iters=iters, max_move=float(cap[b])), "view %d" % b)
        moved += int((_bits(smoothed[b][0]) != _bits(v)).any())
    assert moved >= 1, "the fixture's meshes are smoothed at all"
    # simplify -> smooth -> refine, against the stages run one by one
    chain = cs.reconstruct(eng, *args, refine=1, simplify=cells, smooth={"iters": iters, "pin_boundary": False})
    enc = eng.encode(batch["img"])
    simplified = cs.reconstruct(eng, *args, simplify=cells)
    for b in range(len(plain)):
        sv, sf = simplified[b]
        assert torch.equal(chain[b][1], sf)
        if not len(sf):
            continue
        want = postprocess.smooth_arrays(sv.cpu().numpy(), sf.cpu().numpy(), iters=iters, pin_boundary=False,
                                         max_move=float(cap[b]))
        step = isosurface.refine_mesh(eng, enc, b, batch["trans_mat"], torch.from_numpy(want).cuda(), sf, boxes[b], R, iso, 1)
        assert torch.equal(chain[b][0].view(torch.int32), step[0].view(torch.int32)), b
    # the driver: its own tree, the same bytes as the two-step route
    base = ["--log_dir", log_dir, "--random_init", "3", "--test_lst_dir", lst_dir, "--sdf_dir", sdf_dir,
            "--rendered_dir", rendered_dir, "--category", "chair", "--view_num", str(view_num), "--sdf_res", str(R),
            "--iso", repr(iso), "--seed", str(seed)]
    res = cs.main(base + ["--smooth", str(iters)])
    assert res["out_dir"] == cs.result_obj_path(log_dir, R, iso) + "_t3" and res["written"] == 2
    assert res["smoothed"] == 2 - res["empty"]
    for b, e in enumerate(entries):
        ref = str(tmp_path / "want.obj")
        isosurface.write_obj(ref, smoothed[b][0], smoothed[b][1])
        assert open(cs.obj_path(res["out_dir"], *e), "rb").read() == open(ref, "rb").read(), e


def test_demo_smooth_writes_the_same_faces(tmp_path):
    from PIL import Image
    from disn_amd import create_sdf as cs, demo
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
    smooth = demo.main(args + ["--out", str(tmp_path / "smooth.obj"), "--smooth", "3"])
    assert smooth["faces"] == plain["faces"] > 0 and smooth["verts"] == plain["verts"] > 0
    lines = {k: open(r["out"]).read().splitlines() for k, r in (("plain", plain), ("smooth", smooth))}
    pick = lambda k, tag: [l for l in lines[k] if l.startswith(tag)]
    assert pick("plain", "f ") == pick("smooth", "f ") and len(pick("plain", "f ")) == plain["faces"]
    assert len(pick("plain", "v ")) == len(pick("smooth", "v ")) == plain["verts"]
    assert pick("plain", "v ") != pick("smooth", "v ")

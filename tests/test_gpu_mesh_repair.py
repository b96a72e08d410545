"""The mesh repair on the device (mesh_repair.hip: disn_mesh_repair_count_batch / disn_mesh_repair_emit_batch;
``postprocess.repair_meshes_device`` / ``repair_arrays_device``).  The reference of every comparison is the host function
``postprocess.repair_arrays``, the specification: the faces, the vertex map, the kept faces and the report are compared
for equality, the positions bit for bit (they are a gather)."""
import numpy as np
import pytest
import torch

import mesh_check_fixtures as X
import mesh_repair_fixtures as RX
from guarded_alloc import guarded

pytestmark = pytest.mark.gpu

_CACHE = {}


def _dev(v, f):
    return (torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda().reshape(-1, 3),
            torch.from_numpy(np.ascontiguousarray(f, np.int32)).cuda().reshape(-1, 3))


def _assert_same(got, want, what):
    """got: (verts', faces', vmap, kept, report) of the device; want: that of ``repair_arrays``"""
    assert got[4] == want[4], "%s: report device %r host %r" % (what, got[4], want[4])
    for k, name in enumerate(("verts", "faces", "vmap", "kept")):
        g = got[k].cpu().numpy()
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (what, name, g.shape, want[k].shape)
        same = RX.same_bits(g, want[k]) if k == 0 else np.array_equal(g, want[k])
        assert same, "%s: %s differ" % (what, name)


# ------------------------------------------------------------------ 1. every fixture, the noise meshes
@pytest.mark.parametrize("name", list(RX.FIXTURES))
def test_fixture_equals_repair_arrays_and_the_hand_values(name):
    from disn_amd import postprocess
    v, f, (faces, vmap, kept, report) = RX.FIXTURES[name]
    got = postprocess.repair_arrays_device(*_dev(v, f), strict=False)
    _assert_same(got, RX.repaired(name), name)
    assert got[4] == report and np.array_equal(got[1].cpu().numpy(), faces) and np.array_equal(got[2].cpu().numpy(), vmap)


@pytest.mark.parametrize("name", ["dc0", "dcs0", "dc1", "dcs1", "dc0_simplified", "dcs1_simplified"])
def test_noise_mesh_equals_repair_arrays(name):
    from disn_amd import postprocess
    v, f = RX.noise_meshes()[name]
    for kw in ({}, {"stitch": False}) if name in ("dc0", "dcs1") else ({},):
        got = postprocess.repair_arrays_device(*_dev(v, f), **kw)
        _assert_same(got, RX.repaired(name, **kw), "%s %s" % (name, kw))
    print(name, got[4])
    check = postprocess.check_arrays_device(got[0], got[1], max_pairs=0)
    assert check["manifold"] and check["index_degenerate_faces"] == 0 and check["unreferenced_vertices"] == 0


# ------------------------------------------------------------------ 2. a mesh's result does not depend on its batch
def test_batch_of_five_with_an_empty_and_a_bad_mesh_in_the_middle():
    """status 2: the bad index equals its mesh's own nv -- a slot that exists in the shared vertex buffer, and no kernel
    addresses anything through an index of a mesh with that status"""
    from disn_amd import postprocess
    names = ["dc0", "empty", "index_out_of_range", "pinched_edge", "dcs1_simplified"]
    meshes = [(RX.FIXTURES[n] if n in RX.FIXTURES else RX.noise_meshes()[n])[:2] for n in names]
    repaired, reports = postprocess.repair_meshes_device([_dev(*m) for m in meshes], strict=False)
    assert [r["status"] for r in reports] == [0, 0, 2, 0, 0] and len(repaired[1][0]) == 0
    for n, m, r, rep in zip(names, meshes, repaired, reports):
        assert len(r) == 4
        _assert_same(r + (rep,), RX.repaired(n), "%s in the batch" % n)
        alone = postprocess.repair_arrays_device(*_dev(*m), strict=False)
        assert alone[4] == rep and all(torch.equal(a, b) for a, b in zip(alone[:4], r)), n
    with pytest.raises(ValueError, match="mesh 2: face index out of range"):
        postprocess.repair_meshes_device([_dev(*m) for m in meshes])
    with pytest.raises(ValueError, match="^a vertex coordinate is not finite"):
        postprocess.repair_arrays_device(*_dev(*RX.FIXTURES["not_finite"][:2]))
    with pytest.raises(TypeError):
        postprocess.repair_meshes_device([meshes[0]])                        # host arrays: no CPU fallback
    assert postprocess.repair_meshes_device([]) == ([], [])


def test_further_arrays_follow_the_vertex_map():
    from disn_amd import postprocess
    v, f = RX.FIXTURES["two_tetrahedra_touching"][:2]
    dv, df = _dev(v, f)
    extra = torch.arange(len(v) * 2, dtype=torch.float32, device="cuda").reshape(-1, 2)
    (got,), _ = postprocess.repair_meshes_device([(dv, df, extra)])
    assert len(got) == 5 and torch.equal(got[2], extra[got[3].long()]) and got[3].tolist() == [0, 1, 2, 3, 5, 6, 7, 1]


def test_marching_cubes_of_noise_is_returned_unchanged():
    from disn_amd import isosurface, postprocess
    sdf = torch.from_numpy(X.noise(12, 0).reshape(1, -1)).cuda()
    v, f = isosurface.marching_cubes_batch(sdf, np.asarray([[-1, -1, -1, 1, 1, 1]], np.float64), 12, 0.0)[0]
    v2, f2, vmap, kept, report = postprocess.repair_arrays_device(v, f, weld=False)
    assert len(f) == 4696 and torch.equal(v2, v) and torch.equal(f2, f)
    assert torch.equal(vmap, torch.arange(len(v), dtype=torch.int32, device="cuda"))
    assert torch.equal(kept, torch.arange(len(f), dtype=torch.int32, device="cuda"))
    assert all(report[k] == 0 for k in postprocess.REPAIR_FIELDS if k not in ("nv_out", "nf_out"))
    assert (report["nv_out"], report["nf_out"]) == (len(v), len(f))


# ------------------------------------------------------------------ 3. the stage in the pipeline
def _group():
    if "group" not in _CACHE:
        from disn_amd import create_sdf as cs
        from disn_amd.engine import SdfEngine
        from disn_amd.weights import WeightStore
        from oracle import disn_oracle as O
        eng = SdfEngine(WeightStore.random_init(3))
        img = np.random.default_rng(5).random((2, 137, 137, 3)).astype(np.float32)
        tm = np.concatenate([O.DEMO_TRANS_MAT, O.DEMO_TRANS_MAT]).astype(np.float32)
        box = np.asarray([[-1, -1, -1, 1, 1, 1]] * 2, np.float64)
        iso = float(cs.create_sdf(eng, img, tm, box, 16)[0].median())
        _CACHE["group"] = (eng, img, tm, box, iso)
    return _CACHE["group"]


def test_reconstruct_with_repair():
    from disn_amd import create_sdf as cs, postprocess
    eng, img, tm, box, iso = _group()
    plain = cs.reconstruct(eng, img, tm, box, 16, iso, mesher="dc")
    log = []
    repaired = cs.reconstruct(eng, img, tm, box, 16, iso, mesher="dc", repair=True, repair_log=log)
    assert len(repaired) == 2 == len(log) and sum(len(m[1]) for m in plain) > 100
    wants = [postprocess.repair_arrays(m[0], m[1]) for m in plain]
    for b, (m, want) in enumerate(zip(repaired, wants)):
        assert len(m) == 2 and log[b] == want[4]
        assert RX.same_bits(m[0].cpu().numpy(), want[0]) and np.array_equal(m[1].cpu().numpy(), want[1]), b
        print("dc mesh", b, want[4])
    for c in postprocess.check_meshes_device(repaired, max_pairs=0):
        assert c["nonmanifold_edges"] == c["nonmanifold_vertices"] == 0
        assert c["index_degenerate_faces"] == c["unreferenced_vertices"] == 0
    # the normals follow their vertices
    with_n = cs.reconstruct(eng, img, tm, box, 16, iso, mesher="dc", normals=True)
    rep_n = cs.reconstruct(eng, img, tm, box, 16, iso, mesher="dc", normals=True, repair=True)
    for b, (m, r) in enumerate(zip(with_n, rep_n)):
        want = postprocess.repair_arrays(m[0], m[1])
        assert len(r) == 3 and RX.same_bits(r[0].cpu().numpy(), want[0]) and np.array_equal(r[1].cpu().numpy(), want[1])
        assert torch.equal(r[2], m[2][torch.from_numpy(want[2]).cuda().long()]), b
    # the colours are those of the repaired mesh; vertices and faces those of the call without them
    coloured = cs.reconstruct(eng, img, tm, box, 16, iso, mesher="dc", repair={"stitch": True}, colour=True)
    direct = cs.colour_group(repaired, cs.colour_args(True), img, tm)
    for m, r, d in zip(coloured, repaired, direct):
        assert len(m) == 3 and torch.equal(m[0], r[0]) and torch.equal(m[1], r[1])
        assert m[2].dtype == torch.uint8 and m[2].shape == (len(r[0]), 3) and torch.equal(m[2], d[2])


# ------------------------------------------------------------------ 4. the entries' checks and their memory contract
NEW = ("disn_mesh_repair_workspace_bytes", "disn_mesh_repair_count_batch", "disn_mesh_repair_emit_batch")


def test_memory_contract_of_the_repair_entries():
    """counts, the four outputs (each 5 rows longer than nv_out / nf_out) and a workspace of exactly
    disn_mesh_repair_workspace_bytes lie between guard bands and start out poisoned; guards intact, const inputs
    unchanged, the rows beyond nv_out / nf_out still poison, runs A and B bit-identical; null pointers, B < 1, bad offsets:
    DISN_E_ARG; one byte less of workspace: DISN_E_WS; and a refused call writes nothing"""
    from disn_amd import _lib, ops, postprocess
    names = ["two_tetrahedra_touching", "empty", "pillow", "dc1", "not_finite", "fan_of_18"]
    parts = [(RX.FIXTURES[n] if n in RX.FIXTURES else RX.noise_meshes()[n])[:2] for n in names]
    B, K, pad = len(parts), len(postprocess.REPAIR_FIELDS), 5
    results = {}
    for variant in ("A", "B"):
        with guarded(variant) as g:
            with g.recording() as called:
                h = _lib.lib()
                verts = g.put(np.concatenate([np.asarray(m[0], np.float32).reshape(-1, 3) for m in parts]))
                faces = g.put(np.concatenate([np.asarray(m[1], np.int32).reshape(-1, 3) for m in parts]))
                v_off = np.cumsum([0] + [len(m[0]) for m in parts]).astype(np.int64)
                f_off = np.cumsum([0] + [len(m[1]) for m in parts]).astype(np.int64)
                views = [(verts[v_off[k]:v_off[k + 1]], faces[f_off[k]:f_off[k + 1]]) for k in range(B)]
                wrapped = postprocess.repair_meshes_device(views, strict=False)
                need = h.disn_mesh_repair_workspace_bytes(B, int(v_off[-1]), int(f_off[-1]))
                ws = torch.empty(need, dtype=torch.uint8, device="cuda")
                counts = torch.empty((B, K), dtype=torch.int64, device="cuda")
                sizes = np.asarray([[r[k] for k in postprocess.REPAIR_FIELDS] for r in wrapped[1]], np.int64)
                nvo, nfo = int(sizes[:, 0].sum()), int(sizes[:, 1].sum())
                out_v = torch.empty((nvo + pad, 3), dtype=torch.float32, device="cuda")
                out_f = torch.empty((nfo + pad, 3), dtype=torch.int32, device="cuda")
                vmap = torch.empty(nvo + pad, dtype=torch.int32, device="cuda")
                kept = torch.empty(nfo + pad, dtype=torch.int32, device="cuda")
                outs = (ws, counts, out_v, out_f, vmap, kept)
                before = [t.clone() for t in outs]

                def count(ws_bytes=need, **over):
                    a = dict(verts=verts.data_ptr(), faces=faces.data_ptr(), v_off=v_off.ctypes.data,
                             f_off=f_off.ctypes.data, B=B, counts=counts.data_ptr(), ws=ws.data_ptr())
                    a.update(over)
                    rc = h.disn_mesh_repair_count_batch(a["verts"], a["faces"], a["v_off"], a["f_off"], a["B"], 3,
                                                        a["counts"], a["ws"], ws_bytes, ops._stream())
                    torch.cuda.synchronize()
                    return rc

                def emit(ws_bytes=need, **over):
                    a = dict(verts=verts.data_ptr(), faces=faces.data_ptr(), v_off=v_off.ctypes.data,
                             f_off=f_off.ctypes.data, B=B, sizes=sizes.ctypes.data, out_v=out_v.data_ptr(),
                             out_f=out_f.data_ptr(), vmap=vmap.data_ptr(), kept=kept.data_ptr(), ws=ws.data_ptr())
                    a.update(over)
                    rc = h.disn_mesh_repair_emit_batch(a["verts"], a["faces"], a["v_off"], a["f_off"], a["B"], 3,
                                                       a["sizes"], a["out_v"], a["out_f"], a["vmap"], a["kept"], a["ws"],
                                                       ws_bytes, ops._stream())
                    torch.cuda.synchronize()
                    return rc
                descending = np.asarray(v_off[::-1], np.int64).copy()
                for call, pointers in ((count, ("verts", "faces", "v_off", "f_off", "counts", "ws")),
                                       (emit, ("verts", "faces", "v_off", "f_off", "sizes", "out_v", "out_f", "vmap",
                                               "kept", "ws"))):
                    for name in pointers:
                        assert call(**{name: None}) == -1, (call.__name__, name)
                    assert call(B=0) == -1 and call(v_off=descending.ctypes.data) == -1
                    assert call(ws_bytes=need - 1) == -3
                for t, b in zip(outs, before):
                    assert torch.equal(t.view(torch.uint8), b.view(torch.uint8)), "a refused call writes nothing"
                assert count() == 0
                assert np.array_equal(counts.cpu().numpy(), sizes)
                assert emit() == 0
                for t, b, n in ((out_v, before[2], nvo), (out_f, before[3], nfo), (vmap, before[4], nvo),
                                (kept, before[5], nfo)):
                    assert torch.equal(t[n:].view(torch.uint8), b[n:].view(torch.uint8)), "written beyond the sizes"
            g.check()
            assert set(NEW) <= set(called)
            results[variant] = (wrapped[1], [[x.cpu().numpy() for x in m] for m in wrapped[0]], counts.cpu().numpy(),
                                out_v[:nvo].cpu().numpy(), out_f[:nfo].cpu().numpy(), vmap[:nvo].cpu().numpy(),
                                kept[:nfo].cpu().numpy())
    a, b = results["A"], results["B"]
    assert a[0] == b[0], "results depend on what the buffers held before"
    for k in range(2, 7):
        assert a[k].tobytes() == b[k].tobytes()
    v0 = f0 = 0
    for k, n in enumerate(names):
        want = RX.repaired(n)
        assert a[0][k] == want[4], n
        for x, y, w in zip(a[1][k], b[1][k], want[:4]):
            assert x.tobytes() == y.tobytes() == np.ascontiguousarray(w).tobytes(), n
        nv, nf = len(want[2]), len(want[3])
        assert a[3][v0:v0 + nv].tobytes() == want[0].tobytes() and np.array_equal(a[4][f0:f0 + nf], want[1])
        assert np.array_equal(a[5][v0:v0 + nv], want[2]) and np.array_equal(a[6][f0:f0 + nf], want[3])
        v0, f0 = v0 + nv, f0 + nf
    assert a[0][4]["status"] == 4 and (v0, f0) == (len(a[3]), len(a[4]))

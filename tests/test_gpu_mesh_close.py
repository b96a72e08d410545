"""The mesh closing on the device (mesh_close.hip: disn_mesh_close_count_batch / disn_mesh_close_emit_batch;
``postprocess.close_meshes_device`` / ``close_arrays_device``).  The reference of every comparison is the host function
``postprocess.close_arrays``, the specification: the faces, the vertex map, the kept faces and the report are compared
for equality, the positions bit for bit (the centres are integers divided once)."""
import numpy as np
import pytest
import torch

import mesh_close_fixtures as CX
from guarded_alloc import guarded

pytestmark = pytest.mark.gpu

_CACHE = {}
COMBOS = [{}, {"outward": True}, {"fill": False}, {"orient": False}, {"orient": False, "fill": False}, {"max_hole": 5},
          {"max_hole": 5, "outward": True}]


def _dev(v, f):
    return (torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda().reshape(-1, 3),
            torch.from_numpy(np.ascontiguousarray(f, np.int32)).cuda().reshape(-1, 3))


def _assert_same(got, want, what):
    """got: (verts', faces', vmap, kept, report) of the device; want: that of ``close_arrays``"""
    assert got[4] == want[4], "%s: report device %r host %r" % (what, got[4], want[4])
    for k, name in enumerate(("verts", "faces", "vmap", "kept")):
        g = got[k].cpu().numpy()
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (what, name, g.shape, want[k].shape)
        same = CX.same_bits(g, want[k]) if k == 0 else np.array_equal(g, want[k])
        assert same, "%s: %s differ" % (what, name)


# ------------------------------------------------------------------ 1. every fixture, the noise meshes
@pytest.mark.parametrize("name,case", CX.CASES)
def test_fixture_equals_close_arrays_and_the_hand_values(name, case):
    from disn_amd import postprocess
    v, f, cases = CX.FIXTURES[name]
    kw, (faces, centres, vmap, kept, report) = cases[case]
    got = postprocess.close_arrays_device(*_dev(v, f), strict=False, **kw)
    _assert_same(got, CX.closed(name, case), "%s %s" % (name, kw))
    assert got[4] == report and np.array_equal(got[1].cpu().numpy(), faces) and np.array_equal(got[2].cpu().numpy(), vmap)
    assert CX.same_bits(got[0].cpu().numpy()[len(v):], centres)


@pytest.mark.parametrize("name", CX.NOISE)
def test_noise_mesh_equals_close_arrays_and_is_closed_and_oriented(name):
    from disn_amd import postprocess
    v, f = CX.RX.repaired(name)[:2]
    before = postprocess.check_arrays(v, f, max_pairs=0)
    got = postprocess.close_arrays_device(*_dev(v, f))
    _assert_same(got, CX.closed(name), name)
    print(name, got[4])
    check = postprocess.check_arrays_device(got[0], got[1], max_pairs=0)
    assert check["boundary_edges"] == 0 and check["nonmanifold_edges"] == 0 and got[4]["unorientable_components"] == 0
    assert check["misoriented_edges"] == 0 and check["nonmanifold_vertices"] == before["nonmanifold_vertices"]


@pytest.mark.parametrize("kw", COMBOS, ids=lambda kw: "-".join("%s=%s" % i for i in sorted(kw.items())) or "default")
def test_every_flag_combination_on_a_noise_mesh(kw):
    from disn_amd import postprocess
    v, f = CX.RX.repaired("dcs1_simplified")[:2]
    got = postprocess.close_arrays_device(*_dev(v, f), **kw)
    _assert_same(got, CX.closed("dcs1_simplified", **kw), "dcs1_simplified %s" % kw)
    # the mesh turned inside out face by face for every second face: a component's majority is no longer the input's
    mixed = np.asarray(f).copy()
    mixed[::2] = mixed[::2][:, (0, 2, 1)]
    _assert_same(postprocess.close_arrays_device(*_dev(v, mixed), **kw), postprocess.close_arrays(v, mixed, **kw),
                 "dcs1_simplified, every second face turned, %s" % kw)


# ------------------------------------------------------------------ 2. a mesh's result does not depend on its batch
def test_one_batch_of_all_the_fixtures():
    """the empty mesh and the meshes with a status stand in the middle; status 2: the bad index equals its mesh's own
    nv -- a slot that exists in the shared vertex buffer, and no kernel addresses anything through it"""
    from disn_amd import postprocess
    plain = [n for n in CX.FIXTURES if CX.FIXTURES[n][2][0][1][4]["status"] == 0 and n != "empty"]
    other = [n for n in CX.FIXTURES if n not in plain]
    names = plain[:len(plain) // 2] + other + plain[len(plain) // 2:]
    assert len(names) == len(CX.FIXTURES) and "empty" in other and len(other) == 6
    meshes = [CX.FIXTURES[n][:2] for n in names]
    closed, reports = postprocess.close_meshes_device([_dev(*m) for m in meshes], strict=False)
    assert sorted(r["status"] for r in reports) == [0] * (len(names) - 5) + [2, 4, 16, 16, 16]
    for n, m, r, rep in zip(names, meshes, closed, reports):
        assert len(r) == 4
        _assert_same(r + (rep,), CX.closed(n, 0), "%s in the batch" % n)
    first_bad = min(names.index(n) for n in other if n != "empty")
    with pytest.raises(ValueError, match="mesh %d: " % first_bad):
        postprocess.close_meshes_device([_dev(*m) for m in meshes])
    with pytest.raises(ValueError, match="^not manifold"):
        postprocess.close_arrays_device(*_dev(*CX.FIXTURES["fold_over_at_a_vertex"][:2]))
    with pytest.raises(ValueError, match="^a vertex coordinate is not finite"):
        postprocess.close_arrays_device(*_dev(*CX.FIXTURES["not_finite"][:2]))
    with pytest.raises(ValueError, match="outward needs orient"):
        postprocess.close_meshes_device([_dev(*meshes[0])], orient=False, outward=True)
    with pytest.raises(ValueError, match="max_hole"):
        postprocess.close_meshes_device([_dev(*meshes[0])], max_hole=(1 << 22) + 1)
    with pytest.raises(TypeError):
        postprocess.close_meshes_device([meshes[0]])                         # host arrays: no CPU fallback
    assert postprocess.close_meshes_device([]) == ([], [])


def test_further_arrays_follow_the_vertex_map():
    from disn_amd import postprocess
    v, f = CX.FIXTURES["open_prism"][:2]
    dv, df = _dev(v, f)
    extra = torch.arange(len(v) * 2, dtype=torch.float32, device="cuda").reshape(-1, 2)
    (got,), _ = postprocess.close_meshes_device([(dv, df, extra)])
    assert len(got) == 5 and got[3].tolist() == [0, 1, 2, 3, 4, 5, 0, 3] and torch.equal(got[2], extra[got[3].long()])


def test_closing_the_result_again_changes_nothing():
    from disn_amd import postprocess
    v, f = CX.closed("dc0_simplified")[:2]
    v2, f2, vmap, kept, report = postprocess.close_arrays_device(*_dev(v, f))
    assert CX.same_bits(v2.cpu().numpy(), v) and np.array_equal(f2.cpu().numpy(), f)
    assert report["flipped_faces"] == report["loops"] == 0 and (report["nv_out"], report["nf_out"]) == (len(v), len(f))
    assert torch.equal(vmap, torch.arange(len(v), dtype=torch.int32, device="cuda"))
    assert torch.equal(kept, torch.arange(len(f), dtype=torch.int32, device="cuda"))


# ------------------------------------------------------------------ 3. the stage in the pipeline
def test_reconstruct_with_close():
    from disn_amd import create_sdf as cs, postprocess
    from disn_amd.engine import SdfEngine
    from disn_amd.weights import WeightStore
    from oracle import disn_oracle as O
    eng = SdfEngine(WeightStore.random_init(3))
    img = np.random.default_rng(5).random((2, 137, 137, 3)).astype(np.float32)
    tm = np.concatenate([O.DEMO_TRANS_MAT, O.DEMO_TRANS_MAT]).astype(np.float32)
    box = np.asarray([[-1, -1, -1, 1, 1, 1]] * 2, np.float64)
    iso = float(cs.create_sdf(eng, img, tm, box, 16)[0].median())
    repaired = cs.reconstruct(eng, img, tm, box, 16, iso, mesher="dc", repair=True)
    log = []
    closed = cs.reconstruct(eng, img, tm, box, 16, iso, mesher="dc", repair=True, close=True, close_log=log)
    assert len(closed) == 2 == len(log) and sum(len(m[1]) for m in repaired) > 100
    for b, (m, r) in enumerate(zip(closed, repaired)):
        want = postprocess.close_arrays(r[0], r[1])
        assert len(m) == 2 and log[b] == want[4]
        assert CX.same_bits(m[0].cpu().numpy(), want[0]) and np.array_equal(m[1].cpu().numpy(), want[1]), b
        print("dc mesh", b, want[4])
    for c, rep in zip(postprocess.check_meshes_device(closed, max_pairs=0), log):
        assert c["closed"] and c["manifold"] and rep["unorientable_components"] == 0 and c["oriented"]
    # the normals follow the vertex map: a centre takes those of its loop's smallest vertex
    rep_n = cs.reconstruct(eng, img, tm, box, 16, iso, mesher="dc", normals=True, repair=True)
    cls_n = cs.reconstruct(eng, img, tm, box, 16, iso, mesher="dc", normals=True, repair=True, close={"outward": False})
    for b, (m, r) in enumerate(zip(rep_n, cls_n)):
        want = postprocess.close_arrays(m[0], m[1])
        assert len(r) == 3 and CX.same_bits(r[0].cpu().numpy(), want[0]) and np.array_equal(r[1].cpu().numpy(), want[1])
        assert torch.equal(r[2], m[2][torch.from_numpy(want[2]).cuda().long()]), b


# ------------------------------------------------------------------ 4. the entries' checks and their memory contract
NEW = ("disn_mesh_close_workspace_bytes", "disn_mesh_close_count_batch", "disn_mesh_close_emit_batch")


def test_memory_contract_of_the_close_entries():
    """counts, the four outputs (each 5 rows longer than nv_out / nf_out) and a workspace of exactly
    disn_mesh_close_workspace_bytes lie between guard bands and start out poisoned; guards intact, const inputs
    unchanged, the rows beyond nv_out / nf_out still poison, runs A and B bit-identical; null pointers, B < 1, bad
    offsets: DISN_E_ARG; one byte less of workspace: DISN_E_WS; and a refused call writes nothing"""
    from disn_amd import _lib, ops, postprocess
    names = ["cube_missing_its_top_one_side_flipped", "empty", "moebius_band", "dc1_simplified", "not_finite",
             "three_triangles_on_an_edge", "cone_inside_out"]
    parts = [(CX.FIXTURES[n] if n in CX.FIXTURES else CX.RX.repaired(n))[:2] for n in names]
    flags, cap = postprocess.close_flags(True, True, True, None)
    B, K, pad = len(parts), len(postprocess.CLOSE_FIELDS), 5
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
                wrapped = postprocess.close_meshes_device(views, outward=True, strict=False)
                need = h.disn_mesh_close_workspace_bytes(B, int(v_off[-1]), int(f_off[-1]))
                ws = torch.empty(need, dtype=torch.uint8, device="cuda")
                counts = torch.empty((B, K), dtype=torch.int64, device="cuda")
                sizes = np.asarray([[r[k] for k in postprocess.CLOSE_FIELDS] for r in wrapped[1]], np.int64)
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
                    rc = h.disn_mesh_close_count_batch(a["verts"], a["faces"], a["v_off"], a["f_off"], a["B"], flags, cap,
                                                       a["counts"], a["ws"], ws_bytes, ops._stream())
                    torch.cuda.synchronize()
                    return rc

                def emit(ws_bytes=need, **over):
                    a = dict(verts=verts.data_ptr(), faces=faces.data_ptr(), v_off=v_off.ctypes.data,
                             f_off=f_off.ctypes.data, B=B, sizes=sizes.ctypes.data, out_v=out_v.data_ptr(),
                             out_f=out_f.data_ptr(), vmap=vmap.data_ptr(), kept=kept.data_ptr(), ws=ws.data_ptr())
                    a.update(over)
                    rc = h.disn_mesh_close_emit_batch(a["verts"], a["faces"], a["v_off"], a["f_off"], a["B"], flags, cap,
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
    for k, (n, m) in enumerate(zip(names, parts)):
        want = postprocess.close_arrays(m[0], m[1], outward=True)
        assert a[0][k] == want[4], n
        for x, y, w in zip(a[1][k], b[1][k], want[:4]):
            assert x.tobytes() == y.tobytes() == np.ascontiguousarray(w).tobytes(), n
        nv, nf = len(want[2]), len(want[3])
        assert a[3][v0:v0 + nv].tobytes() == want[0].tobytes() and np.array_equal(a[4][f0:f0 + nf], want[1])
        assert np.array_equal(a[5][v0:v0 + nv], want[2]) and np.array_equal(a[6][f0:f0 + nf], want[3])
        v0, f0 = v0 + nv, f0 + nf
    assert [r["status"] for r in a[0]] == [0, 0, 0, 0, 4, 16, 0] and (v0, f0) == (len(a[3]), len(a[4]))
    assert a[0][6]["flipped_faces"] == CX.RIM and a[0][2]["unorientable_components"] == 1

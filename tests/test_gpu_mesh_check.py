"""The mesh checks on the device (mesh_check.hip: disn_mesh_check_batch; ``postprocess.check_meshes_device`` /
``check_arrays_device``).  The reference of every comparison is the host function ``postprocess.check_arrays``, the
specification: status and counts are compared for equality; ``area`` and ``volume`` are sums whose order is the
implementation's, so they are compared within nf 2^-52 sum|term| -- n - 1 additions, each off by at most 2^-53 of a
partial sum that never exceeds sum|term|, on either side."""
import numpy as np
import pytest
import torch

import mesh_check_fixtures as X
from guarded_alloc import guarded

pytestmark = pytest.mark.gpu

NAMES = list(X.FIXTURES)
_CACHE = {}


def _dev(v, f):
    return (torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda().reshape(-1, 3),
            torch.from_numpy(np.ascontiguousarray(f, np.int32)).cuda().reshape(-1, 3))


def _want(key, v, f, cap=None):
    """check_arrays and check_face_flags of a mesh, computed once per key"""
    from disn_amd import postprocess
    if (key, cap) not in _CACHE:
        _CACHE[(key, cap)] = postprocess._check(v, f, cap)
    return _CACHE[(key, cap)]


def _sum_bounds(v, f):
    """nf 2^-52 sum|term| for the area and the volume of a mesh whose indices are valid and coordinates finite"""
    f = np.asarray(f, np.int64).reshape(-1, 3)
    if not len(f):
        return 0.0, 0.0
    p = np.asarray(v, np.float32).astype(np.float64)[f]
    area = 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    vol = np.abs(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2]))) / 6.0
    scale = len(f) * 2.0 ** -52
    return scale * float(area.sum()) * (1 + 1e-9), scale * float(vol.sum()) * (1 + 1e-9)


def _assert_same(got, got_flags, v, f, want, want_flags, what):
    for k in ("status",) + tuple(X.COUNT_KEYS[1:]) + ("closed", "manifold", "oriented", "watertight"):
        assert got[k] == want[k], "%s: %s device %r host %r" % (what, k, got[k], want[k])
    if want["status"] in (0, 8):
        for k, bound in zip(("area", "volume"), _sum_bounds(v, f)):
            print("%s: %s device %r host %r bound %.3g" % (what, k, got[k], want[k], bound))
            assert abs(got[k] - want[k]) <= bound, (what, k, got[k], want[k], bound)
    else:
        assert got["area"] == 0.0 and got["volume"] == 0.0
    if got_flags is not None:
        assert got_flags.dtype == torch.uint8
        assert np.array_equal(got_flags.cpu().numpy(), want_flags), what


# ------------------------------------------------------------------ 1. every fixture, alone and in one batch
@pytest.mark.parametrize("name", NAMES)
def test_fixture_alone_equals_check_arrays_and_the_hand_values(name):
    from disn_amd import postprocess
    v, f, hand = X.FIXTURES[name]
    want, want_flags = _want(name, v, f)
    got, flags = postprocess.check_arrays_device(*_dev(v, f), face_flags=True)
    _assert_same(got, flags, v, f, want, want_flags, name)
    for k in X.COUNT_KEYS:
        assert got[k] == hand[k], (name, k)


def test_all_fixtures_in_one_batch_with_the_empty_mesh_in_the_middle():
    from disn_amd import postprocess
    order = [n for n in NAMES if n != "empty"]
    order.insert(len(order) // 2, "empty")
    got, flags = postprocess.check_meshes_device([_dev(*X.FIXTURES[n][:2]) for n in order], face_flags=True)
    assert len(got) == len(order) and flags[order.index("empty")].shape == (0,)
    for b, n in enumerate(order):
        v, f, _ = X.FIXTURES[n]
        _assert_same(got[b], flags[b], v, f, *_want(n, v, f), what="%s in the batch" % n)
    assert postprocess.check_meshes_device([]) == []


# ------------------------------------------------------------------ 2. a mesh's result does not depend on its batch
def _noise_host(R):
    from oracle import mc_oracle
    if ("noise", R) not in _CACHE:
        _CACHE[("noise", R)] = mc_oracle.marching_cubes(X.noise(R, 0), [-1, -1, -1, 1, 1, 1], 0.0)
    v, f = _CACHE[("noise", R)]
    return np.asarray(v, np.float32), np.asarray(f, np.int32)


def test_alone_or_among_33_and_twice_the_same_bits():
    from disn_amd import postprocess
    v, f = _noise_host(8)                                                   # 1 192 faces: several blocks
    small = [X.FIXTURES[NAMES[k % len(NAMES)]][:2] for k in range(32)]
    batch = small[:16] + [(v, f)] + small[16:]
    assert len(batch) == 33
    alone = postprocess.check_arrays_device(*_dev(v, f), face_flags=True)
    first = postprocess.check_meshes_device([_dev(*m) for m in batch], face_flags=True)
    again = postprocess.check_meshes_device([_dev(*m) for m in batch], face_flags=True)
    bits = lambda r: np.asarray([r["area"], r["volume"]], np.float64).tobytes()
    assert first[0][16] == alone[0] and bits(first[0][16]) == bits(alone[0])
    assert torch.equal(first[1][16], alone[1])
    for b in range(33):
        assert first[0][b] == again[0][b] and bits(first[0][b]) == bits(again[0][b]), b
        assert torch.equal(first[1][b], again[1][b])
    _assert_same(alone[0], alone[1], v, f, *_want("noise8", v, f), what="noise 8")


def test_meshes_of_255_256_and_257_faces_back_to_back():
    """the block boundary of mesh_of: each mesh the first n faces of the noise mesh, over all its vertices"""
    from disn_amd import postprocess
    v, f = _noise_host(8)
    sizes = [255, 256, 257]
    got, flags = postprocess.check_meshes_device([_dev(v, f[:n]) for n in sizes], face_flags=True)
    for b, n in enumerate(sizes):
        _assert_same(got[b], flags[b], v, f[:n], *_want(("head", n), v, f[:n]), what="%d faces" % n)
        assert got[b]["nf"] == n and got[b]["boundary_edges"] > 0 and got[b]["unreferenced_vertices"] > 0


# ------------------------------------------------------------------ 3. the project's own marching cubes of noise
@pytest.mark.parametrize("R", [12, 20])
def test_noise_mesh_of_the_batched_marching_cubes(R):
    from disn_amd import isosurface, postprocess
    sdf = torch.from_numpy(X.noise(R, 0).reshape(1, -1)).cuda()
    mesh = isosurface.marching_cubes_batch(sdf, np.asarray([[-1, -1, -1, 1, 1, 1]], np.float64), R, 0.0)[0]
    v, f = mesh[0].cpu().numpy(), mesh[1].cpu().numpy()
    want, want_flags = _want(("mc noise", R), v, f)
    got, flags = postprocess.check_arrays_device(mesh[0], mesh[1], face_flags=True)
    _assert_same(got, flags, v, f, want, want_flags, "noise %d" % R)
    assert got["status"] == 0 and got["closed"] and got["oriented"] and got["candidate_pairs"] > 10 * len(f)
    if R == 12:
        assert (got["nf"], got["candidate_pairs"]) == (4696, 54168)


# ------------------------------------------------------------------ 4. statuses that cannot fault
def test_bad_index_nan_and_capped_stack_among_clean_meshes():
    """status 2: the bad index equals its mesh's own nv -- a slot that exists in the shared vertex buffer, and no kernel
    addresses anything through an index of a mesh with that status; status 4: one NaN coordinate; status 8: the stack
    with a cap one below its 2016 candidate pairs"""
    from disn_amd import postprocess
    tv, tf, _ = X.FIXTURES["two_tetrahedra_interpenetrating"]
    sv, sf, _ = X.FIXTURES["stack"]
    cv, cf, _ = X.FIXTURES["cube_open"]
    bad_f = tf.copy()
    bad_f[3, 1] = len(tv)
    nan = tv.copy()
    nan[5, 1] = np.nan
    meshes = [(cv, cf), (tv, bad_f), (tv, tf), (nan, tf), (cv, cf), (sv, sf), (tv, tf)]
    caps = [None, None, None, None, None, 2015, None]
    default = lambda m: postprocess.check_max_pairs(None, len(m[1]))
    cap_list = [default(m) if c is None else c for m, c in zip(meshes, caps)]
    got, flags = postprocess.check_meshes_device([_dev(*m) for m in meshes], max_pairs=cap_list, face_flags=True,
                                                 strict=False)
    assert [g["status"] for g in got] == [0, 2, 0, 4, 0, 8, 0]
    for b, (m, c) in enumerate(zip(meshes, cap_list)):
        want, want_flags = postprocess._check(m[0], m[1], c)
        _assert_same(got[b], flags[b], m[0], m[1], want, want_flags, "mesh %d" % b)
    assert got[5]["candidate_pairs"] == 2016 and got[5]["intersecting_pairs"] == -1 and got[5]["edges"] == 192
    assert got[1]["nv"] == 8 and got[1]["nf"] == 8 and got[1]["edges"] == -1
    assert got[3]["edges"] == 12 and got[3]["candidate_pairs"] == -1
    with pytest.raises(ValueError, match="mesh 1: face index out of range"):
        postprocess.check_meshes_device([_dev(cv, cf), _dev(tv, bad_f)])
    with pytest.raises(ValueError, match="^a vertex coordinate is not finite"):
        postprocess.check_arrays_device(*_dev(nan, tf))
    assert postprocess.check_arrays_device(*_dev(sv, sf), max_pairs=2015)["status"] == 8      # strict: 8 never raises
    with pytest.raises(TypeError):
        postprocess.check_meshes_device([(tv, tf)])                         # host arrays: no CPU fallback


# ------------------------------------------------------------------ 5. the memory contract of the two entries
NEW = ("disn_mesh_check_workspace_bytes", "disn_mesh_check_batch")


def test_memory_contract_of_the_check_entries():
    """counts, sums, status, face_flags and a workspace of exactly disn_mesh_check_workspace_bytes lie between guard
    bands and start out poisoned; guards intact, const inputs unchanged, runs A and B bit-identical; one byte less of
    workspace: DISN_E_WS and nothing written"""
    from disn_amd import _lib, ops, postprocess
    names = ["two_tetrahedra_interpenetrating", "empty", "cube_open", "stack", "fold_over_at_a_vertex"]
    parts = [X.FIXTURES[n][:2] for n in names] + [_noise_host(8)]
    B = len(parts)
    results = {}
    for variant in ("A", "B"):
        with guarded(variant) as g:
            with g.recording() as called:
                verts, faces = g.put(np.concatenate([m[0] for m in parts])), g.put(np.concatenate([m[1] for m in parts]))
                v_off = np.cumsum([0] + [len(m[0]) for m in parts]).astype(np.int64)
                f_off = np.cumsum([0] + [len(m[1]) for m in parts]).astype(np.int64)
                views = [(verts[v_off[k]:v_off[k + 1]], faces[f_off[k]:f_off[k + 1]]) for k in range(B)]
                got, flags = postprocess.check_meshes_device(views, face_flags=True)
                caps = np.asarray([postprocess.check_max_pairs(None, len(m[1])) for m in parts], np.int64)
                need = _lib.lib().disn_mesh_check_workspace_bytes(B, int(v_off[-1]), int(f_off[-1]), int(caps.sum()))
                ws = torch.empty(need, dtype=torch.uint8, device="cuda")
                counts = torch.empty((B, len(postprocess.CHECK_FIELDS)), dtype=torch.int64, device="cuda")
                sums = torch.empty((B, 2), dtype=torch.float64, device="cuda")
                status = torch.empty(B, dtype=torch.int32, device="cuda")
                fl = torch.empty(int(f_off[-1]), dtype=torch.uint8, device="cuda")
                outs = (ws, counts, sums, status, fl)
                before = [t.clone() for t in outs]

                def raw(ws_bytes):
                    rc = _lib.lib().disn_mesh_check_batch(
                        verts.data_ptr(), faces.data_ptr(), v_off.ctypes.data, f_off.ctypes.data, B, caps.ctypes.data,
                        counts.data_ptr(), sums.data_ptr(), fl.data_ptr(), status.data_ptr(), ws.data_ptr(), ws_bytes,
                        ops._stream())
                    torch.cuda.synchronize()
                    return rc
                assert raw(need - 1) == -3
                for t, b in zip(outs, before):
                    assert torch.equal(t.view(torch.uint8), b.view(torch.uint8)), "a refused call writes nothing"
                assert raw(need) == 0
            g.check()
            assert set(NEW) <= set(called)
            results[variant] = (got, [x.cpu().numpy() for x in flags], counts.cpu().numpy(), sums.cpu().numpy(),
                                status.cpu().numpy(), fl.cpu().numpy())
    a, b = results["A"], results["B"]
    assert a[0] == b[0], "results depend on what the buffers held before"
    for x, y in zip(a[1], b[1]):
        assert np.array_equal(x, y)
    for k in range(2, 6):
        assert a[k].tobytes() == b[k].tobytes()
    for k, (v, f) in enumerate(parts):
        want, want_flags = _want(("contract", k), v, f)
        _assert_same(a[0][k], torch.from_numpy(a[1][k]), v, f, want, want_flags, "part %d" % k)
        assert a[2][k].tolist() == [want[n] for n in postprocess.CHECK_FIELDS]
    assert a[4].tolist() == [0] * B and np.array_equal(a[5], np.concatenate(a[1]))
    assert a[3].tobytes() == np.asarray([[r["area"], r["volume"]] for r in a[0]], np.float64).tobytes()


# ------------------------------------------------------------------ 6. the meshes of the three meshers
@pytest.mark.parametrize("mesher", ["mc", "dc", "dcs"])
def test_group_through_reconstruct(mesher):
    import reconstruct_fixtures as RF
    from disn_amd import create_sdf as cs, postprocess
    if "group" not in _CACHE:
        from disn_amd.engine import SdfEngine
        from disn_amd.weights import WeightStore
        eng = SdfEngine(WeightStore.random_init(3))
        rng = np.random.default_rng(5)
        img = rng.random((2, 137, 137, 3)).astype(np.float32)
        from oracle import disn_oracle as O
        tm = np.concatenate([O.DEMO_TRANS_MAT, O.DEMO_TRANS_MAT]).astype(np.float32)
        box = np.asarray([[-1, -1, -1, 1, 1, 1]] * 2, np.float64)
        iso = float(cs.create_sdf(eng, img, tm, box, 16)[0].median())
        _CACHE["group"] = (eng, img, tm, box, iso)
    eng, img, tm, box, iso = _CACHE["group"]
    meshes = cs.reconstruct(eng, img, tm, box, 16, iso, mesher=mesher)
    assert len(meshes) == 2 and sum(len(m[1]) for m in meshes) > 100
    got, flags = postprocess.check_meshes_device(meshes, face_flags=True, strict=False)
    for b, m in enumerate(meshes):
        v, f = m[0].cpu().numpy(), m[1].cpu().numpy()
        want, want_flags = postprocess._check(v, f)
        _assert_same(got[b], flags[b], v, f, want, want_flags, "%s mesh %d" % (mesher, b))
        print(mesher, b, got[b])

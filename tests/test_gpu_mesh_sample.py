"""GPU tests of the surface sampler (mesh_sample.hip, include/disn_amd_sample.h) against its specification,
``metrics.sample_surface_arrays``: the face of every sample and the statuses exactly, points and normals to the derived
bar; independence from the companions of a call and from n; the memory contract; the scores end to end.

The bar for points and normals: at most 8 float32 roundings with weights in [0, 1] (three products, two sums, the
weights' own three), each below 2^-24 max|coordinate|, so below 4.8e-7 max|coordinate| -- 1e-6 max|coordinate| is
asserted.  Bitwise equality is what the construction promises (no contraction, correctly rounded sqrtf and float64
division and square root); the first test prints how many values differ in any bit.

End to end on the box (2332 faces) and its simplification on 16 cells (566 faces), n = 2048, the expected values (the
host rule with a float64 brute-force nearest neighbour gives them too): Chamfer-L1 on surface samples 0.02298 (the mesh
against itself, two seeds) and 0.02274 (simplified against original), a change of 1 %; ``chamfer_views`` on vertex
samples 1.398 and 4.121, a factor 2.9.  The self bar: two independent uniform samples of density rho = n / area lie
1 / (2 sqrt(rho)) apart on average (nearest neighbour in a planar Poisson process), 0.0235 here; twice that is asserted.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_sample_fixtures as XF  # noqa: E402
from guarded_alloc import guarded  # noqa: E402

SF = XF.SF
N = XF.N_BATCH
SEEDS = XF.BATCH_SEEDS
BOX_AREA = 8.0 * (SF.BOX_HALF[0] * SF.BOX_HALF[1] + SF.BOX_HALF[0] * SF.BOX_HALF[2] + SF.BOX_HALF[1] * SF.BOX_HALF[2])


@pytest.fixture(scope="module", autouse=True)
def _built():
    from disn_amd.csrc import build
    build.build()


def _dev(mesh):
    import torch
    return tuple(a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in mesh)


def _sample(meshes, n, seeds):
    """``sample_surface_meshes_device`` -> host arrays (points, normals, face_idx, status)"""
    from disn_amd import metrics
    return tuple(t.cpu().numpy() for t in metrics.sample_surface_meshes_device([_dev(m) for m in meshes], n, seeds))


def _batch_result():
    return XF.cached("device_batch", lambda: _sample(XF.batch(), N, SEEDS))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _raw(meshes, n, seeds, normals=True, face_idx=True):
    """the C entry itself, so that NULL outputs can be passed: -> (rc, points, normals or None, face_idx or None, status)"""
    import torch

    from disn_amd import _lib, ops
    from disn_amd.postprocess import _pack_meshes
    B = len(meshes)
    h = _lib.lib()
    v, v_off, f, f_off, ws = _pack_meshes([_dev(m) for m in meshes],
                                          lambda nv, nf: h.disn_mesh_sample_workspace_bytes(B, nv, nf, n))
    sd = np.asarray(seeds, np.uint64)
    pts = torch.empty((B, n, 3), dtype=torch.float32, device="cuda")
    nrm = torch.empty((B, n, 3), dtype=torch.float32, device="cuda") if normals else None
    idx = torch.empty((B, n), dtype=torch.int32, device="cuda") if face_idx else None
    status = torch.empty(B, dtype=torch.int32, device="cuda")
    rc = h.disn_mesh_sample_batch(v.data_ptr(), f.data_ptr(), v_off.ctypes.data, f_off.ctypes.data, B, sd.ctypes.data, n,
                                  pts.data_ptr(), None if nrm is None else nrm.data_ptr(),
                                  None if idx is None else idx.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(),
                                  ops._stream())
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()
    return rc, host(pts), host(nrm), host(idx), host(status)


def test_the_batch_equals_the_host_rule():
    pts, nrm, idx, status = _batch_result()
    assert pts.shape == nrm.shape == (5, N, 3) and idx.shape == (5, N) and idx.dtype == np.int32
    assert status.tolist() == [0, 6, 0, 6, 0]
    for b, (v, f) in enumerate(XF.batch()):
        hp, hn, hi, hs = XF.host_rule(b)
        assert status[b] == hs
        assert np.array_equal(idx[b], hi), "mesh %d: %d faces differ" % (b, (idx[b] != hi).sum())
        tol = 1e-6 * (float(np.abs(v).max()) if len(v) else 1.0)
        dp, dn = np.abs(pts[b] - hp).max(), np.abs(nrm[b] - hn).max()
        print("mesh %d (%d faces, status %d): max |point - rule| = %.3g (bar %.3g), max |normal - rule| = %.3g; values "
              "that differ in a bit: points %d, normals %d of %d" % (b, len(f), hs, dp, tol, dn, (pts[b] != hp).sum(),
                                                                     (nrm[b] != hn).sum(), hp.size))
        assert dp <= tol and dn <= 1e-6
        if hs:
            assert not pts[b].any() and not nrm[b].any() and not idx[b].any()
    drawn = XF.host_rule(4)[2]
    from disn_amd import metrics
    q = metrics.surface_face_weights(*XF.soup())
    assert (q == 0).sum() > 1000 and (q[drawn] > 0).all() and drawn.max() > 4096 * 16        # the last scan block too


def test_a_mesh_alone_has_the_bits_it_has_in_the_batch():
    batch = _batch_result()
    for b, mesh in enumerate(XF.batch()):
        alone = _sample([mesh], N, SEEDS[b:b + 1])
        for name, x, y in zip(("points", "normals", "face_idx", "status"), alone, batch):
            assert np.array_equal(_bits(x[0]), _bits(y[b])), (b, name)
    # the same call on arrays that already lie back to back
    import torch

    from disn_amd import metrics
    v_off = np.cumsum([0] + [len(m[0]) for m in XF.batch()])
    f_off = np.cumsum([0] + [len(m[1]) for m in XF.batch()])
    verts = torch.from_numpy(np.concatenate([m[0] for m in XF.batch()])).cuda()
    faces = torch.from_numpy(np.concatenate([m[1] for m in XF.batch()])).cuda()
    packed = metrics.sample_surface_arrays_device(verts, faces, v_off, f_off, N, SEEDS)
    for x, y in zip(packed, batch):
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(y))
    # and in another place, with other companions
    moved = _sample([XF.batch()[4], XF.batch()[0]], N, [SEEDS[4], SEEDS[0]])
    for x, y in zip(moved, batch):
        assert np.array_equal(_bits(x[0]), _bits(y[4])) and np.array_equal(_bits(x[1]), _bits(y[0]))


def test_a_sample_does_not_depend_on_n():
    batch = _batch_result()
    one = _sample(XF.batch(), 1, SEEDS)
    two_k = _sample(XF.batch(), 2048, SEEDS)
    for x, y, z in zip(one[:3], batch[:3], two_k[:3]):
        assert np.array_equal(_bits(x[:, :1]), _bits(y[:, :1]))
        assert np.array_equal(_bits(z[:, :N]), _bits(y))                   # the stream goes on where n = 1000 ended
    for b in (0, 2, 4):
        assert np.array_equal(two_k[2][b], XF.host_rule(b, 2048)[2])
    assert np.array_equal(one[3], batch[3]) and np.array_equal(two_k[3], batch[3])


def test_statuses_leave_the_neighbours_untouched():
    from disn_amd import metrics
    batch = _batch_result()
    v, f = SF.box_mesh(32)
    bad = f.copy()
    bad[len(f) // 2, 1] = len(v)                                            # valid in the next mesh, not in its own
    neg = f.copy()
    neg[0, 0] = -1
    nan = v.copy()
    nan[17, 2] = np.nan
    both = (nan, bad)
    meshes = [XF.batch()[0], (v, bad), XF.batch()[2], (nan, f), (v, neg), both, XF.batch()[4]]
    seeds = [SEEDS[0], 1, SEEDS[2], 2, 3, 4, SEEDS[4]]
    pts, nrm, idx, status = _sample(meshes, N, seeds)
    assert status.tolist() == [0, 2, 0, 4, 2, 4, 0]
    for b in (1, 3, 4, 5):
        assert not pts[b].any() and not nrm[b].any() and not idx[b].any()
        assert metrics.sample_surface_arrays(meshes[b][0], meshes[b][1], 4, 0)[3] == status[b]
    for here, there in ((0, 0), (2, 2), (6, 4)):
        for x, y in zip((pts, nrm, idx), batch):
            assert np.array_equal(_bits(x[here]), _bits(y[there]))


def test_null_normals_and_face_idx_are_accepted():
    batch = _batch_result()
    meshes = XF.batch()[:3]
    for normals, face_idx in ((False, False), (True, False), (False, True)):
        rc, pts, nrm, idx, status = _raw(meshes, N, SEEDS[:3], normals, face_idx)
        assert rc == 0 and status.tolist() == [0, 6, 0]
        assert np.array_equal(_bits(pts), _bits(batch[0][:3]))
        assert nrm is None or np.array_equal(_bits(nrm), _bits(batch[1][:3]))
        assert idx is None or np.array_equal(idx, batch[2][:3])


# the entries of include/disn_amd_sample.h (tests/test_guarded_alloc_host.py reads this tuple)
NEW = ("disn_mesh_sample_workspace_bytes", "disn_mesh_sample_batch")


def test_memory_contract_of_both_entries():
    """nothing is written outside points, normals, face_idx, status and ws[:workspace_bytes] (every one of them lies
    between guard bands, the workspace exactly as large as disn_mesh_sample_workspace_bytes says), and the result does
    not depend on what they held before (the two variants poison them differently).  The B = 5 call reads a
    concatenated copy of its inputs (an empty mesh breaks the adjacency ``_pack`` looks for); the packed call of the
    four meshes with faces and the B = 1 call read the guarded, frozen inputs in place."""
    import torch
    from disn_amd import metrics
    batch = _batch_result()
    results = {}
    for variant in ("A", "B"):
        with guarded(variant) as g:
            with g.recording() as called:
                meshes = [(g.put(v), g.put(f)) if len(v) and len(f) else _dev((v, f)) for v, f in XF.batch()]
                out = metrics.sample_surface_meshes_device(meshes, N, SEEDS)
                rc, pts, _, _, status = _raw(meshes[:1], 7, SEEDS[:1], normals=False, face_idx=False)   # in place
                some = [0, 2, 3, 4]                                        # one guarded allocation, sliced into views
                parts = [XF.batch()[b] for b in some]
                verts, faces = g.put(np.concatenate([m[0] for m in parts])), g.put(np.concatenate([m[1] for m in parts]))
                v_off = np.cumsum([0] + [len(m[0]) for m in parts])
                f_off = np.cumsum([0] + [len(m[1]) for m in parts])
                views = [(verts[v_off[k]:v_off[k + 1]], faces[f_off[k]:f_off[k + 1]]) for k in range(len(some))]
                from disn_amd.postprocess import _pack
                assert _pack([m[0] for m in views], torch.float32, "verts")[0].data_ptr() == verts.data_ptr()
                assert _pack([m[1] for m in views], torch.int32, "faces")[0].data_ptr() == faces.data_ptr()
                packed = metrics.sample_surface_meshes_device(views, N, [SEEDS[b] for b in some])
            g.check()
            for x, y in zip(packed, batch):
                assert np.array_equal(_bits(x.cpu().numpy()), _bits(y[some]))
            assert set(NEW) <= set(called)
            assert len(g.records) >= 5                                     # four outputs and the workspace, at least
            results[variant] = [t.cpu().numpy() for t in out] + [pts, status]
            assert rc == 0
    for a, b, ref in zip(results["A"], results["B"], list(batch) + [batch[0][:1, :7], batch[3][:1]]):
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(ref))


def test_surface_scores_see_the_surface_where_vertex_samples_see_the_tessellation():
    import torch

    from disn_amd import metrics, postprocess
    v, f = SF.box_mesh(32)
    sv, sf = XF.cached("box simplified 16", lambda: postprocess.simplify_arrays(v, f, SF.UNIT, 16)[:2])
    n = 2048
    pts, nrm, _, status = metrics.sample_surface_meshes_device([_dev((v, f)), _dev((v, f)), _dev((sv, sf))], n, [1, 2, 1])
    assert status.tolist() == [0, 0, 0]
    thresholds = metrics.f_score_thresholds(2.5)
    s = metrics.surface_scores(pts[1:], nrm[1:], pts[0], nrm[0], thresholds)
    itself, simplified = s["chamfer_l1"]
    rng = np.random.default_rng(0)
    gt = metrics.sample_vertices(v, n, rng)
    cd = metrics.chamfer_views(torch.stack([metrics.sample_vertices(v, n, rng), metrics.sample_vertices(sv, n, rng)]),
                               gt).cpu().numpy()
    print("surface samples: chamfer_l1 %.5f against itself, %.5f simplified (x %.3f), normal consistency %.4f / %.4f; "
          "vertex samples: chamfer_views %.4f against itself, %.4f simplified (x %.3f)"
          % (itself, simplified, simplified / itself, s["normal_consistency"][0], s["normal_consistency"][1], cd[0], cd[1],
             cd[1] / cd[0]))
    assert s["normal_consistency"][0] > 0.9
    assert 0 < itself < 2 * 0.5 / np.sqrt(n / BOX_AREA)
    assert s["f_score"].shape == (2, 6) and s["f_score"][0, -1] == 1.0      # every point within 0.5 of the other sample
    assert abs(simplified / itself - 1) < abs(cd[1] / cd[0] - 1)

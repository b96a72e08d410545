"""SDF gradients at query points on the device (disn_query_grad, SdfEngine.query_grad / refine_vertices,
isosurface.refine_mesh, the --refine / --normals flags) against the float64 forward-mode reference of
tests/sdf_grad_reference.py.  He weights of seed 2, oracle.synth_inputs(seed=3).

Which points a gradient comparison uses: a gradient jumps across a ReLU kink and across a bilinear cell line, so a
point counts when its kink margin is >= 3e-5, it is not clamped and not within 1e-3 px of a cell line
(sdf_grad_reference.included); at least 75 % of the points must count.  The gradient bound is not a constant: e32 is the
largest component error of the SAME reference run in numpy float32 (encoder included) on the included points of the
(2, 2085) case, and the device may err by 2 * e32 (another summation order; both are fp32-accurate)."""
import os

import numpy as np
import pytest
import torch

import reconstruct_fixtures as RF
import sdf_grad_reference as R
from conftest import report_close
from oracle import disn_oracle as O

pytestmark = pytest.mark.gpu

ATOL, RTOL = 1e-5, 1e-5          # the project's bar on pred_sdf
NMAX = 2048 + 37


@pytest.fixture(scope="module")
def world():
    """engine, the four images' device state, the float64 encoder state of the reference (once), and e32"""
    from disn_amd.engine import SdfEngine
    from disn_amd.weights import WeightStore
    store = WeightStore.random_init(2, mode="he")
    eng = SdfEngine(store)
    feed = O.synth_inputs(seed=3, batch=4, n_points=NMAX)
    imgs, pts, tm = feed["imgs"], feed["sample_pc"], feed["trans_mat"]
    W = store.arrays
    enc64 = R.encode(imgs, W, np.float64)
    enc32 = R.encode(imgs[:2], W, np.float32)
    ref2 = R.reference(W, imgs, pts[:2], tm[:2], np.float64, enc64)
    run32 = R.reference(W, imgs, pts[:2], tm[:2], np.float32, enc32)
    inc = R.included(ref2)
    e32 = float(np.abs(run32["grad"].astype(np.float64) - ref2["grad"])[inc].max())
    print("\n[sdf_grad] (2, %d): %.1f %% of the points included; e32 = %.3g (numpy float32 run vs float64), |grad| "
          "median %.3g" % (NMAX, 100 * inc.mean(), e32, np.median(np.linalg.norm(ref2["grad"], axis=-1))))
    return {"eng": eng, "store": store, "W": W, "imgs": imgs, "pts": pts, "tm": tm, "enc64": enc64, "enc": eng.encode(imgs),
            "ref2": ref2, "e32": e32}


def _case_points(world, B, N):
    if (B, N) == (1, 1):      # one point: the first one of image 0 whose gradient is comparable (by the REFERENCE's flags)
        k = int(np.argmax(R.included(world["ref2"])[0]))
        return world["pts"][:1, k:k + 1]
    return world["pts"][:B, :N]


@pytest.mark.parametrize("B,N", [(1, 1), (1, 200), (2, NMAX), (4, 256)])
def test_query_grad_vs_float64(world, B, N):
    eng, W = world["eng"], world["W"]
    pts, tm = np.ascontiguousarray(_case_points(world, B, N)), world["tm"][:B]
    ref = R.reference(W, world["imgs"], pts, tm, np.float64, world["enc64"])
    val = R.reference(W, world["imgs"], pts, tm, np.float64, world["enc64"], oracle_gather=True)["value"]
    sdf, grad = eng.query_grad(world["enc"], pts, tm)
    torch.cuda.synchronize()
    assert tuple(sdf.shape) == (B, N) and tuple(grad.shape) == (B, N, 3)
    sdf, grad = sdf.cpu().numpy(), grad.cpu().numpy().astype(np.float64)
    inc = R.included(ref)
    err = np.abs(grad - ref["grad"])
    print("\n[sdf_grad] (%d, %d): value max |d| %.3g; gradient max |d| on the %d included points %.3g (e32 %.3g)"
          % (B, N, np.abs(sdf - val).max(), inc.sum(), err[inc].max() if inc.any() else 0.0, world["e32"]))
    report_close("pred_sdf of query_grad vs oracle", sdf, val, ATOL, RTOL)
    if (B, N) == (2, NMAX):
        assert inc.mean() >= 0.75
    assert inc.any()
    # e32 = 1.85e-4 on the (2, 2085) case (|grad| ~ 3.9: the float32 projection's 1e-5 px times the slopes of the
    # folded map; 1.6e-4 with n_points=2048).  Measured on an MI355X: 3.8e-5 at (1, 1), 1.1e-4 at (1, 200), 2.45e-4 at
    # (2, 2085) with 1.1e-4 on its 181 clamped points, 2.4e-4 at (4, 256) -- against the bound of 3.7e-4
    assert err[inc].max() <= 2 * world["e32"]
    if (B, N) == (2, NMAX):
        # clamped points: the clamped coordinate adds nothing to the tangents (the reference zeroes its Jacobian)
        cl = R.clamped_comparable(ref)
        print("[sdf_grad] %d clamped points, gradient max |d| %.3g" % (cl.sum(), err[cl].max()))
        assert cl.sum() >= 50
        assert err[cl].max() <= 2 * world["e32"]
        assert np.abs(ref["grad"][cl]).max() > 0.1          # ... and the rest of the gradient is there


def test_batch_independence_bit_for_bit(world):
    """image b's value and gradients in a B = 2 (and B = 4) call are those of a call on image b alone, BIT FOR BIT:
    every image's folded bias row is formed by a launch of its own and no product's summation order depends on the row
    count (the forward ``query`` documents fp32-rounding agreement from B >= 4 on; this entry point is stricter)."""
    from disn_amd import ops
    eng, enc = world["eng"], world["enc"]
    N = 300
    pts = torch.from_numpy(np.ascontiguousarray(world["pts"][:, :N])).cuda()
    tm = torch.from_numpy(world["tm"]).cuda()
    alone = []
    for b in range(4):
        s, g = ops.query_grad(eng.weights.mlp, eng.pmap_of(enc, b), enc.embedding[b:b + 1].contiguous(), tm[b:b + 1],
                              pts[b:b + 1].contiguous())
        alone.append((s[0].clone(), g[0].clone()))
    for B in (2, 4):
        s, g = eng.query_grad(enc, pts[:B].contiguous(), tm[:B])
        torch.cuda.synchronize()
        for b in range(B):
            assert torch.equal(s[b], alone[b][0]) and torch.equal(g[b], alone[b][1]), (B, b)
    assert not torch.equal(alone[0][1], alone[1][1])
    _, g_only = ops.query_grad(eng.weights.mlp, eng.pmap_of(enc, 0), enc.embedding[:1], tm[:1], pts[:1].contiguous(),
                               want_sdf=False)                                  # sdf == NULL
    assert torch.equal(g_only[0], alone[0][1])


def test_chunk_boundary_bit_for_bit(world):
    """N above one workspace chunk (16384 points) = two calls on its halves, bit for bit"""
    eng, enc = world["eng"], world["enc"]
    N = 16384 + 70
    rng = np.random.default_rng(11)
    pts = torch.from_numpy(rng.uniform(-1, 1, (1, N, 3)).astype(np.float32)).cuda()
    tm = world["tm"][:1]
    s, g = eng.query_grad(enc, pts, tm)
    h = N // 2
    s0, g0 = (t.clone() for t in eng.query_grad(enc, pts[:, :h].contiguous(), tm))
    s1, g1 = eng.query_grad(enc, pts[:, h:].contiguous(), tm)
    torch.cuda.synchronize()
    assert torch.equal(s, torch.cat([s0, s1], 1)) and torch.equal(g, torch.cat([g0, g1], 1))
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0.1
    # ... and the value is the forward query's to fp32 rounding
    f = eng.query(enc, pts, tm, fold=True, fused=False)
    assert float((f - s).abs().max()) <= 4e-6 * max(1.0, float(f.abs().max()))


def test_argument_and_workspace_errors(world):
    import ctypes as C
    from disn_amd import _lib
    eng, enc = world["eng"], world["enc"]
    h = _lib.lib()
    assert h.disn_query_grad_workspace_bytes(0, 5) == 0 and h.disn_query_grad_workspace_bytes(1, 0) == 0
    need = h.disn_query_grad_workspace_bytes(1, 8)
    assert 0 < need < h.disn_query_grad_workspace_bytes(1, 20000) == h.disn_query_grad_workspace_bytes(1, 1 << 20)
    pm, emb = eng.pmap_of(enc, 0), enc.embedding
    pts = torch.zeros((1, 8, 3), device="cuda")
    tm = torch.from_numpy(world["tm"][:1]).cuda()
    out = torch.zeros((1, 8, 3), device="cuda")
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    call = lambda grad, nbytes: h.disn_query_grad(C.byref(eng.weights.mlp), pm.data_ptr(), emb.data_ptr(), tm.data_ptr(),
                                                  pts.data_ptr(), 1, 8, None, grad, ws.data_ptr(), nbytes, None)
    assert call(out.data_ptr(), need - 256) == -3
    assert call(None, need) == -1
    assert call(out.data_ptr(), need) == 0
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def refined(world):
    """17^3 grid over [-1,1]^3 of image 0, marching cubes at iso 0, two refinement steps"""
    from disn_amd import isosurface
    eng, enc, tm = world["eng"], world["enc"], world["tm"][:1]
    box, res = [-1, -1, -1, 1, 1, 1], 16
    grid = eng.query_grid(enc, 0, tm, box, res)
    verts, faces = isosurface.marching_cubes(grid, box, res, 0.0)
    assert len(verts) > 200 and len(faces) > 200
    new, normals, residual = eng.refine_vertices(enc, 0, tm, verts, iso=0.0, iters=2, cell=2.0 / res)
    mesh = isosurface.refine_mesh(eng, enc, 0, tm, verts, faces, box, res, 0.0, 2)
    torch.cuda.synchronize()
    return {"verts": verts, "faces": faces, "new": new, "normals": normals, "residual": residual, "mesh": mesh,
            "cell": 2.0 / res}


def test_refine_vertices(world, refined):
    """residuals by the EXISTING SdfEngine.query, not by the new code"""
    eng, enc, tm = world["eng"], world["enc"], world["tm"][:1]
    old, new = refined["verts"], refined["new"]
    r0 = eng.query(enc, old[None].contiguous(), tm).abs()[0].cpu().numpy()
    r1 = eng.query(enc, new[None].contiguous(), tm).abs()[0].cpu().numpy()
    moved = (new - old).norm(dim=1).cpu().numpy()
    print("\n[sdf_grad] refine: %d vertices, |pred| median %.3g -> %.3g, p90 %.3g -> %.3g, worse: %d, largest move %.3g "
          "cells; own residual median %.3g" % (len(r0), np.median(r0), np.median(r1), np.percentile(r0, 90),
                                               np.percentile(r1, 90), int((r1 > r0).sum()), moved.max() / refined["cell"],
                                               float(refined["residual"].median())))
    assert np.median(r1) <= np.median(r0) / 10
    assert np.percentile(r1, 90) <= np.percentile(r0, 90)
    assert not (r1 > r0).any()
    assert moved.max() <= refined["cell"] * (1 + 1e-6)
    assert tuple(refined["residual"].shape) == (len(r0),)
    # refine_mesh: the same vertices and normals, the faces untouched
    v, f, n = refined["mesh"]
    assert torch.equal(v, new) and torch.equal(n, refined["normals"]) and torch.equal(f, refined["faces"])
    # iters = 0: nothing moves
    v0, n0, _ = eng.refine_vertices(enc, 0, tm, old, iters=0, cell=refined["cell"])
    assert torch.equal(v0, old) and float(n0.norm(dim=1).max()) > 0.5


def test_normals(world, refined):
    """unit length to 1e-5 where non-zero; the direction of the float64 gradient at the refined vertices within the
    angle a component error of 2 * e32 allows: |dg| <= 2 sqrt(3) e32, so sin(angle) <= 2 sqrt(3) e32 / |g|"""
    n = refined["normals"].cpu().numpy().astype(np.float64)
    ln = np.linalg.norm(n, axis=1)
    nz = ln > 0
    assert nz.mean() > 0.99 and np.abs(ln[nz] - 1).max() <= 1e-5
    ref = R.reference(world["W"], world["imgs"], refined["new"].cpu().numpy()[None], world["tm"][:1], np.float64,
                      world["enc64"])
    inc = R.included(ref)[0] & nz
    g = ref["grad"][0]
    gl = np.linalg.norm(g, axis=1)
    sin_a = np.linalg.norm(np.cross(n, g / gl[:, None]), axis=1)
    allowed = np.minimum(1.0, 2 * np.sqrt(3.0) * world["e32"] / gl) + 1e-6     # (+ the rounding of the normalisation)
    print("\n[sdf_grad] normals: %d of %d vertices included, largest sin(angle) %.3g, smallest allowance %.3g"
          % (inc.sum(), len(n), sin_a[inc].max(), allowed[inc].min()))
    assert inc.mean() >= 0.5
    assert (sin_a[inc] <= allowed[inc]).all() and (np.sum(n * g, axis=1)[inc] > 0).all()
    # Winding against the "vn" normals, a SIGN decision: marching_cubes winds a face towards the larger GRID values
    # (test_marching_cubes.py pins that), the normals point along +grad pred (asserted above, vertex by vertex).  Were
    # the two conventions opposed, a share s of agreeing faces would become 1 - s, so the majority decides and 1/2 is
    # the threshold.  The share itself is a property of the field, not of the code: a He-initialised network is rough
    # at the scale of a 17^3 cell (the float64 reference's unit gradients at two corners of a face are more than 90
    # degrees apart on 36 % of the faces), and the float64 reference on the oracle's mesh gives 83.0 % (device: 83.2 %).
    # Face by face the device must decide as the float64 gradients at the same vertices do: on a face whose three
    # vertices are included, |n - n64| = 2 sin(angle / 2) <= sqrt(2) sin(angle) <= sqrt(2) allowed at each (angle < 90
    # degrees, asserted above), so the two sums differ by at most |fn| sqrt(2) (sum of allowed) and the signs are
    # equal wherever the float64 sum lies further from zero than that.
    v, f = refined["new"].cpu().numpy().astype(np.float64), refined["faces"].cpu().numpy()
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    n64 = g / gl[:, None]
    s = np.sum(fn * (n[f[:, 0]] + n[f[:, 1]] + n[f[:, 2]]), axis=1)
    s64 = np.sum(fn * (n64[f[:, 0]] + n64[f[:, 1]] + n64[f[:, 2]]), axis=1)
    slack = np.linalg.norm(fn, axis=1) * np.sqrt(2.0) * allowed[f].sum(axis=1)
    decided = inc[f].all(axis=1) & (np.abs(s64) > slack)
    agree = (s > 0).mean()
    print("[sdf_grad] faces whose geometric normal agrees with their vertices' normals: %.1f %% (float64 gradients at "
          "the same vertices: %.1f %%); %d of %d faces decided" % (100 * agree, 100 * (s64 > 0).mean(), decided.sum(), len(f)))
    assert agree > 0.5
    assert decided.any() and ((s > 0) == (s64 > 0))[decided].all()


def test_driver_flags(world, tmp_path, monkeypatch):
    """create_sdf.reconstruct and the command line on the fixtures of tests/reconstruct_fixtures.py: without the flags
    the bytes of today, with --refine 2 --normals nv 'vn' lines and the same faces"""
    from disn_amd import create_sdf as cs, isosurface
    eng, R_ = world["eng"], 16
    entries = RF.expected_entries(4, 3)[:3]
    sdf_dir, rendered_dir = RF.build_dataset(str(tmp_path / "data"), entries)
    batch = cs.load_group(entries, sdf_dir, rendered_dir)
    args = (batch["img"], batch["trans_mat"], batch["sdf_params"], R_)
    grids = cs.create_sdf(eng, *args)
    iso = float(grids[0].median())
    plain = cs.reconstruct(eng, *args, iso)
    both = cs.reconstruct(eng, *args, iso, refine=2, normals=True)
    only_refined = cs.reconstruct(eng, *args, iso, refine=2)
    assert len(plain) == len(both) == len(only_refined) == 3
    nonempty = 0
    for b in range(3):
        verts, faces = isosurface.marching_cubes(grids[b], np.asarray(batch["sdf_params"][b], np.float64), R_, iso)
        assert len(plain[b]) == 2 and torch.equal(plain[b][0], verts) and torch.equal(plain[b][1], faces)
        v, f, n = both[b]
        assert torch.equal(f, faces) and v.shape == verts.shape == n.shape
        assert len(only_refined[b]) == 2 and torch.equal(only_refined[b][0], v)
        p0, p1 = str(tmp_path / ("plain%d.obj" % b)), str(tmp_path / ("want%d.obj" % b))
        isosurface.write_obj(p0, verts, faces)
        isosurface.write_obj(p1, *plain[b])
        assert open(p0, "rb").read() == open(p1, "rb").read()
        nonempty += len(faces) > 0
        if len(verts):
            assert float((v - verts).norm(dim=1).max()) > 0
    assert nonempty >= 1
    # the command line, on the same weights (the engine is main's own)
    lst_dir, log_dir = str(tmp_path / "lst"), str(tmp_path / "ckpt")
    RF.write_lists(lst_dir, cats=RF.CATS[:1], objs={RF.CATS[0][1]: [entries[0][1]]})
    os.makedirs(log_dir)
    monkeypatch.setattr(cs, "restore_weights", lambda log_dir, random_init: (world["store"], "the test's store"))
    res = cs.main(["--log_dir", log_dir, "--test_lst_dir", lst_dir, "--sdf_dir", sdf_dir, "--rendered_dir", rendered_dir,
                   "--category", "chair", "--view_num", "3", "--sdf_res", str(R_), "--iso", repr(iso), "--seed", "4",
                   "--refine", "2", "--normals"])
    assert res["written"] == 3
    for b, e in enumerate(entries):
        path = cs.obj_path(res["out_dir"], *e)
        lines = open(path).read().splitlines()
        v, f, n = (t.cpu().numpy() for t in both[b])
        assert sum(l.startswith("v ") for l in lines) == len(v) and sum(l.startswith("vn ") for l in lines) == len(v)
        v1, f1 = isosurface.read_obj(path)
        assert np.array_equal(f1, f) and np.array_equal(v1, v)
        vn = np.asarray([[float(t) for t in l.split()[1:]] for l in lines if l.startswith("vn ")], np.float32)
        assert np.array_equal(vn.reshape(-1, 3), n)

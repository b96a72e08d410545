"""Dual contouring on the device (include/dc/disn_amd_dc.h, disn_amd/csrc/dual_contour.hip): points, grid normals,
vertices and faces equal the host specification ``isosurface.dual_contour_arrays`` BIT FOR BIT; the batch, the memory
contract of the five entries, and the pipeline behind ``create_sdf.reconstruct(mesher="dc")``."""
import numpy as np
import pytest
import torch

import dual_contour_fixtures as F
from guarded_alloc import guarded

pytestmark = pytest.mark.gpu

REG = 2.0 ** -10
NEW = ("disn_dc_workspace_bytes", "disn_dc_count_batch", "disn_dc_points_batch", "disn_dc_grid_normals_batch",
       "disn_dc_emit_batch")


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return F.bits(a)


def _res(vol):
    return round(vol.size ** (1.0 / 3.0)) - 1


def _normals_fn(fixtures):
    """the fixtures' own normals at the device's points (computed on the host from the points the device produced)"""
    def fn(b, points):
        return torch.from_numpy(fixtures[b][3](points.cpu().numpy())).to(points.device)
    return fn


def _run(fixtures, grid_normals=False, reg=REG):
    from disn_amd import isosurface
    R, iso = _res(fixtures[0][0]), fixtures[0][2]
    assert all(_res(fx[0]) == R and fx[2] == iso for fx in fixtures)
    sdf = torch.from_numpy(np.stack([fx[0] for fx in fixtures])).cuda()
    boxes = np.stack([fx[1] for fx in fixtures])
    return isosurface.dual_contour_batch(sdf, boxes, R, iso, None if grid_normals else _normals_fn(fixtures), reg,
                                         hermite=True)


def _check(item, fixture, grid_normals=False, reg=REG, what=""):
    """one grid's device result against the host specification"""
    from disn_amd import isosurface
    vol, box, iso, normals_at = fixture
    v, f, p, n = item
    pts = isosurface.hermite_points_arrays(vol, box, iso)
    assert p.shape == pts.shape and np.array_equal(_bits(p), _bits(pts)), "%s: points" % what
    nrm = isosurface.grid_normals_arrays(vol, box, iso) if grid_normals else normals_at(pts)
    assert n.shape == nrm.shape and np.array_equal(_bits(n), _bits(nrm)), "%s: normals" % what
    hv, hf = isosurface.dual_contour_arrays(vol, box, iso, nrm, reg)
    assert v.shape == hv.shape and f.shape == hf.shape, (what, v.shape, hv.shape, f.shape, hf.shape)
    assert v.dtype == torch.float32 and f.dtype == torch.int32
    assert np.array_equal(_bits(v), _bits(hv)), "%s: vertices" % what
    assert np.array_equal(f.cpu().numpy(), hf), "%s: faces" % what
    return hv, hf


def test_cube():
    fx = F.cube(8)
    for grid_normals in (False, True):
        v, f = _check(_run([fx], grid_normals)[0], fx, grid_normals, what="cube grid=%s" % grid_normals)
        assert len(v) == 152 and len(f) == 300
    corner = np.full(3, F.CUBE_H)
    v, _ = _check(_run([fx])[0], fx)
    assert np.abs(v.astype(np.float64) - corner).max(1).min() <= REG * F.CUBE_C / 3 + 1e-6     # the corner is there


def test_sphere_in_a_skew_box():
    fx = F.sphere(9, F.SKEW, 0.6, 0.05)
    for grid_normals in (False, True):
        v, f = _check(_run([fx], grid_normals)[0], fx, grid_normals, what="sphere grid=%s" % grid_normals)
        assert len(v) > 100 and len(f) > 200
    _check(_run([fx], reg=0.5)[0], fx, reg=0.5, what="sphere reg=1/2")
    _check(_run([fx], reg=1.0)[0], fx, reg=1.0, what="sphere reg=1")


def test_noise_with_rows_that_only_count_in_the_mean():
    fx = F.noise(5)
    vol, box, iso, normals_at = fx
    # the fixture reaches what it is for (asserted on the host): ambiguous cells, both diagonals, both windings, and
    # NaN, zero and infinite rows
    ins = vol.reshape(6, 6, 6) < 0
    a, b, c, d = ins[:, :-1, :-1], ins[:, :-1, 1:], ins[:, 1:, :-1], ins[:, 1:, 1:]
    assert ((a == d) & (b == c) & (a != b)).any(), "no ambiguous face"
    pts, nrm, hv, hf = F.mesh(fx)
    assert np.isnan(nrm).any() and np.isinf(nrm).any() and (nrm == 0).all(1).any()
    same_first = hf[0::2, 0] == hf[1::2, 0]                       # (q0 ..)(q0 ..) against (q0 ..)(q1 ..)
    assert same_first.any() and (~same_first).any(), "one diagonal only"
    v, f = _check(_run([fx])[0], fx, what="noise")
    assert len(f) > 100
    _check(_run([fx], grid_normals=True)[0], fx, True, what="noise grid normals")


@pytest.mark.parametrize("R", [1, 2])
def test_tiny_grids(R):
    fx = F.noise(R, seed=3)
    v, f = _check(_run([fx])[0], fx, what="R=%d" % R)
    assert len(v) >= 1 and (R > 1 or (len(v) == 1 and len(f) == 0))
    _check(_run([fx], grid_normals=True)[0], fx, True, what="R=%d grid normals" % R)
    empty = (np.ones((R + 1) ** 3, np.float32), F.UNIT.copy(), 0.0, fx[3])
    item = _run([empty])[0]
    assert [tuple(t.shape) for t in item] == [(0, 3)] * 4
    inside = (-np.ones((R + 1) ** 3, np.float32), F.UNIT.copy(), 0.0, fx[3])
    assert [tuple(t.shape) for t in _run([inside], grid_normals=True)[0]] == [(0, 3)] * 4


def test_a_batch_equals_its_grids_alone():
    from disn_amd import isosurface
    R = 5
    empty = (np.ones((R + 1) ** 3, np.float32), F.UNIT.copy(), 0.0, F.noise(R)[3])
    fixtures = [F.sphere(R, F.SKEW, 0.6, 0.0), empty, F.noise(R, box=F.UNIT * 0.75)]
    for grid_normals in (False, True):
        batch = _run(fixtures, grid_normals)
        assert len(batch) == 3 and [len(t) for t in batch[1]] == [0, 0, 0, 0]
        for b, fx in enumerate(fixtures):
            _check(batch[b], fx, grid_normals, what="grid %d of the batch" % b)
            alone = _run([fx], grid_normals)[0]
            for x, y in zip(batch[b], alone):
                assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y))
        assert int(batch[2][1].min()) == 0                       # the indices are local to their grid
    # several rounds (a batch beyond the edge-slot limit) give the same meshes
    sdf = torch.from_numpy(np.stack([fx[0] for fx in fixtures])).cuda()
    boxes = np.stack([fx[1] for fx in fixtures])
    rounds = isosurface.dual_contour_batch(sdf, boxes, R, 0.0, None, REG, max_edge_slots=2 * 3 * 6 ** 3 + 1)
    for x, y in zip(rounds, batch):
        assert np.array_equal(_bits(x[0]), _bits(y[0])) and torch.equal(x[1], y[1])
    one = isosurface.dual_contour(sdf[2], boxes[2], R, 0.0)
    assert np.array_equal(_bits(one[0]), _bits(batch[2][0])) and torch.equal(one[1], batch[2][1])


@pytest.mark.parametrize("fixture", [F.sphere(9, F.SKEW, 0.6, 0.05), F.noise(5)], ids=["sphere9", "noise5"])
def test_the_points_are_the_device_marching_cubes_vertices(fixture):
    from disn_amd import isosurface
    vol, box, iso, _ = fixture
    mc_v, _ = isosurface.marching_cubes(torch.from_numpy(vol).cuda(), box, _res(vol), iso)
    p = _run([fixture], grid_normals=True)[0][2]
    assert p.shape == mc_v.shape and len(p) > 50 and torch.equal(p.view(torch.int32), mc_v.view(torch.int32))


def test_memory_contract_of_the_dual_contouring_entries():
    """every buffer the wrapper hands over (counts, points, normals, vertices, faces and the workspace, each exactly as
    large as the sizes and disn_dc_workspace_bytes say) lies between guard bands and starts out poisoned: guards intact,
    const inputs unchanged, runs A and B bit-identical and equal to the rule, so every output byte was written"""
    from disn_amd import _lib, isosurface
    R = 5
    fixtures = [F.sphere(R, F.SKEW, 0.6, 0.0), F.noise(R, box=F.UNIT * 0.75)]
    boxes = np.stack([fx[1] for fx in fixtures])
    results = {}
    for variant in ("A", "B"):
        with guarded(variant) as g:
            with g.recording() as called:
                sdf = g.put(np.stack([fx[0] for fx in fixtures]))
                given = []

                def fn(b, points):
                    given.append(g.put(fixtures[b][3](points.cpu().numpy())))
                    return given[-1]
                net = isosurface.dual_contour_batch(sdf, boxes, R, 0.0, fn, REG, hermite=True)
                grid = isosurface.dual_contour_batch(sdf, boxes, R, 0.0, None, REG, hermite=True)
                sizes = sorted(r.nbytes for r in g.records)
                need = _lib.lib().disn_dc_workspace_bytes(2, R)
                ne, nv, nf = (sum(len(m[k]) for m in net) for k in (2, 0, 1))
                assert sizes.count(need) == 2 and nf > 0                        # a workspace of exactly the query's size
                for n_bytes in (2 * 3 * 8, ne * 12, nv * 12, nf * 12):          # counts, points / normals, verts, faces
                    assert n_bytes in sizes, (n_bytes, sizes)
                # one byte less of workspace: DISN_E_WS, and nothing is written
                ws = torch.empty(need, dtype=torch.uint8, device="cuda")
                counts = torch.zeros((2, 3), dtype=torch.int64, device="cuda")
                before = ws.clone()
                assert _lib.lib().disn_dc_count_batch(sdf.data_ptr(), 2, R, 0.0, counts.data_ptr(), ws.data_ptr(),
                                                      need - 1, None) == -3
                torch.cuda.synchronize()
                assert torch.equal(ws, before) and counts.tolist() == [[0, 0, 0]] * 2
            g.check()
            assert set(NEW) <= set(called)
            assert len(g.records) >= 12
            for b, fx in enumerate(fixtures):
                _check(net[b], fx, what="guarded %s grid %d" % (variant, b))
                _check(grid[b], fx, True, what="guarded %s grid %d, grid normals" % (variant, b))
            results[variant] = [_bits(t).copy() for m in net + grid for t in m]
    assert all(np.array_equal(x, y) for x, y in zip(results["A"], results["B"]))


# ------------------------------------------------------------------ the pipeline
@pytest.fixture(scope="module")
def world():
    from oracle import disn_oracle as O
    from disn_amd.engine import SdfEngine
    from disn_amd.weights import WeightStore
    eng = SdfEngine(WeightStore.random_init(0, mode="he"))
    d = O.synth_inputs(0, 2, 64)
    tms = np.stack([O.DEMO_TRANS_MAT[0], O.synth_trans_mat(30, 25, 0.8)]).astype(np.float32)
    boxes = np.stack([F.UNIT, F.SKEW])
    return {"eng": eng, "imgs": d["imgs"], "tms": tms, "boxes": boxes}


def _same(got, want):
    assert len(got) == len(want)
    for (gv, gf, *_), (wv, wf, *_) in zip(got, want):
        assert gv.shape == wv.shape and torch.equal(gv.view(torch.int32), wv.view(torch.int32))
        assert torch.equal(gf, wf)


def test_reconstruct_with_the_dual_contouring_mesher(world):
    from disn_amd import create_sdf as cs, isosurface
    eng, imgs, tms, boxes, R = world["eng"], world["imgs"], world["tms"], world["boxes"], 8
    grids = cs.create_sdf(eng, imgs, tms, boxes, R)
    iso = float(grids[0].median())
    args = (eng, imgs, tms, boxes, R, iso)
    enc = eng.encode(imgs)

    def network(b, points):
        return eng.refine_vertices(enc, b, tms, points, iso=iso, iters=0)[1]
    want = isosurface.dual_contour_batch(grids, boxes, R, iso, network, REG, hermite=True)
    assert sum(len(m[1]) for m in want) > 50
    got = cs.reconstruct(*args, mesher="dc")
    _same(got, want)
    for b in range(2):                                            # ... and the host rule on the network's normals
        fx = (grids[b].cpu().numpy(), boxes[b], iso, None)
        hv, hf = isosurface.dual_contour_arrays(fx[0], fx[1], iso, want[b][3].cpu().numpy(), REG)
        assert np.array_equal(_bits(want[b][0]), _bits(hv)) and np.array_equal(want[b][1].cpu().numpy(), hf)
    # the grid normals and another regulariser through the same door
    _same(cs.reconstruct(*args, mesher="dc", dc={"normals": "grid", "reg": 0.25}),
          isosurface.dual_contour_batch(grids, boxes, R, iso, None, 0.25))
    assert not torch.equal(cs.reconstruct(*args, mesher="dc", dc=0.25)[0][0], got[0][0])
    # later stages see a (verts, faces) pair as before
    v, f, n = cs.reconstruct(*args, normals=True, mesher="dc")[0]
    assert torch.equal(f, got[0][1]) and n.shape == v.shape
    # marching cubes stays the default and its bits stay what they are
    today = isosurface.marching_cubes_batch(grids, boxes, R, iso)
    _same(cs.reconstruct(*args), today)
    _same(cs.reconstruct(*args, mesher="mc"), today)
    with pytest.raises(ValueError):
        cs.reconstruct(*args, mesher="mc", dc=0.25)
    with pytest.raises(ValueError):
        cs.reconstruct(*args, mesher="dc", dc=2.0)


def test_reconstruct_fused_with_the_dual_contouring_mesher(world):
    from disn_amd import create_sdf as cs, isosurface
    eng, imgs, tms, boxes, R = world["eng"], world["imgs"], world["tms"], world["boxes"], 8
    enc = eng.encode(imgs)
    grid = eng.query_grid_views(enc, (0, 2), tms, boxes[0], R).reshape(1, -1)
    iso = float(grid.median())
    want = isosurface.dual_contour_batch(grid, boxes[:1], R, iso, None, REG)
    assert len(want[0][1]) > 20
    _same(cs.reconstruct_fused(eng, imgs, tms, boxes, R, iso, fuse=2, mesher="dc"), want)
    _same(cs.reconstruct_fused(eng, imgs, tms, boxes, R, iso, fuse=2, mesher="dc", dc={"normals": "network"}), want)
    today = isosurface.marching_cubes_batch(grid, boxes[:1], R, iso)
    _same(cs.reconstruct_fused(eng, imgs, tms, boxes, R, iso, fuse=2), today)
    _same(cs.reconstruct_fused(eng, imgs, tms, boxes, R, iso, fuse=2, mesher="mc"), today)

"""Multi-view reconstruction on the GPU: the pooled gather and the embedding pool against the numpy reference
(tests/multiview_reference.py) bit for bit, the whole pooled query against the float64 oracle, the grid form and
``create_sdf.reconstruct_fused``."""
import numpy as np
import pytest
import torch

import multiview_reference as MR
from oracle import disn_oracle as O

pytestmark = pytest.mark.gpu

PRED_ATOL = 1e-5      # the project's bar on what the path returns, un-divided (tests/test_gpu_model.py)
UNEVEN = np.array([0.7, 0.2, 0.1], np.float32)
TAP_SHAPES = ((224, 64), (112, 128), (56, 256), (28, 512), (14, 512))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


@pytest.fixture(scope="module")
def kernel_world():
    """standard-normal taps (signed: max is no maximum of ReLU outputs) of the true shapes for 3 views, the 70 points
    and 3 cameras of multiview_reference, and the oracle's per-view rows [3,70,1472] for the plain cameras and for
    the set whose view 1 sends the origin to NaN -- computed once, shared by every case"""
    rng = np.random.default_rng(17)
    taps = [rng.standard_normal((3, hw, hw, ch), dtype=np.float32) for hw, ch in TAP_SHAPES]
    maps = MR.view_maps(taps)
    pts, idx = MR.kernel_points()
    cams = {"plain": MR.kernel_cameras(), "nan": MR.kernel_cameras(nan_view=1)}
    rows = {k: MR.gather_views(maps, c, pts) for k, c in cams.items()}
    assert not rows["nan"][1, idx["origin"][0]].any() and rows["plain"][1, idx["origin"][0]].any()
    return {"taps": [_dev(t) for t in taps], "pts": _dev(pts), "cams": {k: _dev(c) for k, c in cams.items()},
            "rows": rows, "n": pts.shape[0]}


@pytest.mark.parametrize("cams", ["plain", "nan"])
@pytest.mark.parametrize("weights", ["default", "uneven"])
@pytest.mark.parametrize("pool", ["max", "mean"])
@pytest.mark.parametrize("V", [1, 2, 3])
def test_pooled_gather_equals_the_reference(kernel_world, V, pool, weights, cams):
    """N = 70: 18 workgroups of four waves, the last one ragged; one kernel form serves every N"""
    from disn_amd import ops
    k = kernel_world
    w = None if weights == "default" else UNEVEN[:V]
    # V = 1 and 2 of the NaN set start at view 1, so that the NaN view is pooled first / alone as well
    v0 = 1 if cams == "nan" and V < 3 else 0
    want = MR.pool_views(k["rows"][cams][v0:v0 + V], pool, w)
    n = k["n"]
    out = torch.full((n + 3, 1472), -77.0, dtype=torch.float32, device="cuda")
    got = ops.gather_taps_pool([t[v0:v0 + V] for t in k["taps"]], k["cams"][cams][v0:v0 + V], k["pts"], pool,
                               None if w is None else _dev(w), out=out)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert np.array_equal(got[:n], want), "max |diff| %g in %d elements" % (
        np.abs(got[:n] - want).max(), (got[:n] != want).sum())
    assert (got[n:] == -77.0).all()                                 # rows beyond N are untouched


@pytest.mark.parametrize("pool", ["max", "mean"])
def test_one_view_equals_gather_taps(kernel_world, pool):
    from disn_amd import ops
    k = kernel_world
    for v in range(3):
        taps = [t[v:v + 1] for t in k["taps"]]
        cam = k["cams"]["nan"][v:v + 1]
        want = ops.gather_taps(taps, cam, k["pts"][None])[0]
        assert torch.equal(ops.gather_taps_pool(taps, cam, k["pts"], pool), want)      # 1.0 * f == f


@pytest.mark.parametrize("weights", ["default", "uneven"])
@pytest.mark.parametrize("pool", ["max", "mean"])
@pytest.mark.parametrize("V", [1, 3])
def test_pool_embedding_equals_the_reference(V, pool, weights):
    from disn_amd import ops
    emb = np.random.default_rng(3).standard_normal((3, 1024)).astype(np.float32)[:V]
    w = None if weights == "default" else UNEVEN[:V]
    got = ops.pool_embedding(_dev(emb), pool, None if w is None else _dev(w))
    assert got.shape == (1, 1024)
    assert np.array_equal(got.cpu().numpy()[0], MR.pool_views(emb, pool, w))


def test_bad_shapes_are_refused():
    from disn_amd import ops
    from disn_amd._lib import DisnError
    taps = [torch.zeros((1, hw, hw, ch), device="cuda") for hw, ch in TAP_SHAPES]
    pts, cam = torch.zeros((4, 3), device="cuda"), torch.zeros((1, 4, 3), device="cuda")
    with pytest.raises(ValueError):
        ops.gather_taps_pool(taps, cam, pts, "sum")
    with pytest.raises(ValueError):
        ops.gather_taps_pool(taps, torch.zeros((2, 4, 3), device="cuda"), pts)          # two cameras, one view of taps
    arr = ops._tap_ptrs(taps)
    import ctypes as C
    for V, pool in ((0, 0), (25, 0), (1, 2)):                                           # the C ABI's own check
        rc = ops.lib().disn_gather_taps_pool(C.byref(arr), V, cam.data_ptr(), None, pool, pts.data_ptr(), 4,
                                             torch.zeros((4, 1472), device="cuda").data_ptr(), None)
        assert rc == -2
        with pytest.raises(DisnError):
            ops.check("disn_gather_taps_pool", rc)


# ---- the whole path ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_world():
    from disn_amd.engine import SdfEngine
    from disn_amd.weights import WeightStore
    store = WeightStore.random_init(0, mode="he")
    eng = SdfEngine(store)
    d = O.synth_inputs(0, 4, 64)
    tms = np.stack([O.DEMO_TRANS_MAT[0], O.synth_trans_mat(30, 25, 0.8), O.synth_trans_mat(201.5, 30, 0.65),
                    O.synth_trans_mat(110, 10, 0.9)]).astype(np.float32)
    return {"store": store, "eng": eng, "imgs": d["imgs"], "pts": d["sample_pc"][0], "tms": tms,
            "enc": eng.encode(d["imgs"])}


def test_query_views_against_the_float64_oracle(model_world):
    m = model_world
    eng, enc, W = m["eng"], m["enc"], m["store"].arrays
    _, emb64, maps, _ = O.encode(m["imgs"][:2], W, dtype=np.float64)
    per_view = [[mp[v:v + 1] for mp in maps] for v in range(2)]
    for pool, w in (("max", None), ("mean", None), ("mean", [0.25, 0.75])):
        ref = MR.pred_views(per_view, emb64, m["tms"][:2], m["pts"], W, pool, w, dtype=np.float64)
        got = eng.query_views(enc, (0, 2), m["tms"][:2], m["pts"], pool, w).cpu().numpy()
        err = float(np.abs(got - ref).max())
        print("[query_views %s %s] max |gpu - f64| %.3g, |pred| max %.3g" % (pool, w, err, float(np.abs(ref).max())))
        assert got.shape == (64,) and err <= PRED_ATOL
    # the two pools are different functions of the views, and neither is a single view's answer
    one = eng.query(enc, m["pts"][None], m["tms"][:1], fold=False)[0].cpu().numpy()
    assert np.abs(eng.query_views(enc, (0, 2), m["tms"][:2], m["pts"], "max").cpu().numpy() - one).max() > PRED_ATOL
    for pool in ("max", "mean"):          # V = 1: the single-view query (unfolded, the same arithmetic)
        alone = eng.query_views(enc, (0, 1), m["tms"][:1], m["pts"], pool).cpu().numpy()
        d = float(np.abs(alone - one).max())
        print("[query_views V=1 %s] max |views - query| %.3g" % (pool, d))
        assert d <= PRED_ATOL
    with pytest.raises(ValueError):
        eng.query_views(enc, (3, 2), m["tms"][:2], m["pts"])               # the range leaves the encoded images
    with pytest.raises(ValueError):
        eng.query_views(enc, (0, 2), m["tms"][:3], m["pts"])               # three cameras for two views


def test_query_grid_views(model_world):
    from disn_amd import ops
    m = model_world
    eng, enc = m["eng"], m["enc"]
    R, sp = 8, [-1.0, -0.9, -0.8, 0.9, 1.0, 0.7]
    total = (R + 1) ** 3
    for pool in ("max", "mean"):
        grid = eng.query_grid_views(enc, (1, 2), m["tms"][1:3], sp, R, pool)
        pts = ops.grid_points(sp, R, 0, total, "cuda")
        # (IEEE division on the host: torch divides by a Python scalar by multiplying with its reciprocal)
        want = eng.query_views(enc, (1, 2), m["tms"][1:3], pts, pool).cpu().numpy() / np.float32(10.0)
        assert grid.shape == (total,) and np.array_equal(grid.cpu().numpy(), want)
        # a range evaluates the fixed chunks it touches whole, so it is bit for bit that slice of the whole grid
        k0, k1 = 100, 401
        part = eng.query_grid_views(enc, (1, 2), m["tms"][1:3], sp, R, pool, k0=k0, k1=k1)
        assert part.shape == (k1 - k0,) and torch.equal(part, grid[k0:k1])
        out = torch.empty(total, device="cuda")
        assert eng.query_grid_views(enc, (1, 2), m["tms"][1:3], sp, R, pool, out=out) is out and torch.equal(out, grid)


def test_grid_ranges_across_chunk_boundaries_equal_the_whole_grid(model_world):
    """R = 40: 68921 points, a full chunk of 65536 (the GEMM chain) and a ragged one of 3385 (the small-set layers).
    Ranges inside either chunk, across the boundary, and ending at the last point are slices of the whole, bit for bit"""
    m = model_world
    eng, enc = m["eng"], m["enc"]
    R, sp = 40, [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
    total = (R + 1) ** 3
    grid = eng.query_grid_views(enc, (0, 2), m["tms"][:2], sp, R, "max")
    assert grid.shape == (total,) and bool(torch.isfinite(grid).all())
    for k0, k1 in ((7, 1000), (65000, 66000), (65536, 65537), (total - 500, total)):
        part = eng.query_grid_views(enc, (0, 2), m["tms"][:2], sp, R, "max", k0=k0, k1=k1)
        assert part.shape == (k1 - k0,) and torch.equal(part, grid[k0:k1]), (k0, k1)


def test_reconstruct_fused(model_world):
    from disn_amd import create_sdf as cs, isosurface
    from disn_amd.engine import SdfEngine
    m = model_world
    # strict: a view's taps do not depend on the batch it was encoded in, so a run's mesh must not either
    eng = SdfEngine(None, weights=m["eng"].weights, strict=True)
    R = 16
    boxes = np.array([[-1, -1, -1, 1, 1, 1]] * 2 + [[-0.9, -1, -0.8, 1, 0.9, 1]] * 2, np.float64)
    enc = eng.encode(m["imgs"])
    grids = [eng.query_grid_views(enc, (2 * r, 2), m["tms"][2 * r:2 * r + 2], boxes[2 * r], R) for r in range(2)]
    iso = float(grids[0].median())
    want = [isosurface.marching_cubes(grids[r], boxes[2 * r], R, iso) for r in range(2)]
    got = cs.reconstruct_fused(eng, m["imgs"], m["tms"], boxes, R, iso, fuse=2)
    assert len(got) == 2 and len(want[0][1]) > 0
    print("[reconstruct_fused] iso %.6g, triangles per run %s" % (iso, [len(w[1]) for w in want]))
    for r in range(2):
        assert torch.equal(got[r][0], want[r][0]) and torch.equal(got[r][1], want[r][1])
    alone = cs.reconstruct_fused(eng, m["imgs"][2:], m["tms"][2:], boxes[2:], R, iso, fuse=2, pool="max")
    assert len(alone) == 1
    assert torch.equal(alone[0][0], got[1][0]) and torch.equal(alone[0][1], got[1][1])
    with pytest.raises(ValueError):
        cs.reconstruct_fused(eng, m["imgs"][:3], m["tms"][:3], boxes[:3], R, iso, fuse=2)

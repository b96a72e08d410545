"""Every copy of the projection-and-resampling rule (include/disn_amd.h, disn_project) on the exact pixel lattice of
tests/resample_lattice.py: cell lines, the clamps from either side, the image corners, cell 0 and cell 135, every
tap-row relation of the legacy resize table and a NaN point -- places random points never reach
(tests/test_resample_lattice_host.py asserts that the table reaches them).

The features are synthetic: standard-normal taps of the five VGG tap shapes and their oracle map
concat(O.resize_bilinear_legacy(tap, 137, 137)), built once.  The gather-only entries are compared with the oracle bit
for bit on every point; the entries with the point MLP behind the gather against the float64 decoder on the oracle's
rows with the tolerance of their random-point tests (test_gpu_fused.py, test_gpu_fold.py, test_gpu_multiview.py); a
one-cell slip is more than a hundred such tolerances (host test).  One test or case per consumer, each printing a
``LATTICE`` line: the kernel it ran, the points compared, the worst error and its tolerance."""
import numpy as np
import pytest
import torch

import multiview_reference as MR
import resample_lattice as L
import sdf_grad_reference as R
from oracle import disn_oracle as O
from test_gpu_train_edges import _HAND_PLACED
from tests import fused_emulation as E

pytestmark = pytest.mark.gpu

ATOL, RTOL = 1e-5, 1e-5          # test_gpu_fold.py (query, query_folded); the fused forms (test_gpu_fused.py): ATOL alone
MR_ATOL = 1e-5                   # test_gpu_multiview.py PRED_ATOL


def dev(a):
    return torch.tensor(np.asarray(a, np.float32)).cuda()            # (a copy: the lattice's arrays are read-only)


def host(t):
    return t.detach().cpu().numpy()


def line(consumer, kernel, n, err, tol):
    print("\nLATTICE %s: kernel %s; %d points; worst %s" % (
        consumer, kernel, n, "0 differing elements (bit for bit)" if tol is None else "%.3g (tolerance %.3g)" % (err, tol)))


def same_bits(name, got, want):
    """bit for bit up to the sign of zero and NaN payloads, element by element, with a count in the message"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: %s vs %s" % (name, got.shape, want.shape)
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), "%s: %d elements differ, first at %s (rows %s)" % (
        name, bad.sum(), np.argwhere(bad)[0].tolist(), np.unique(np.argwhere(bad)[:, -2])[:8].tolist())


@pytest.fixture(scope="module")
def world():
    """the lattice, image 0's taps / oracle map / oracle rows (once), the suite's He store on the device (true units)"""
    from disn_amd import ops
    from disn_amd.engine import DeviceWeights
    from disn_amd.weights import WeightStore
    store = WeightStore.random_init(L.WEIGHT_SEED, mode="he")
    W = L.weight_arrays()
    for k, v in W.items():                       # the host test's teeth and share were measured on these variables
        assert np.array_equal(v, store.arrays[k]), k
    dw = DeviceWeights(store, torch.device("cuda", 0), equalise=False)
    lat, lat0 = L.lattice(True), L.lattice(False)
    fm = L.oracle_map(0)
    rows = L.oracle_rows(fm[0][None], lat["table"])
    rows.setflags(write=False)
    taps = [dev(t) for t in L.synthetic_taps(0)]
    return dict(ops=ops, mlp=dw.mlp, keep=dw, W=W, lat=lat, lat0=lat0, fm=fm, fm_d=dev(fm), rows=rows, taps=taps,
                emb=L.embedding(0), emb_d=dev(L.embedding(0)), cam_d=dev(lat["camera"]), pts_d=dev(lat["pts"][None]),
                n=len(lat["pts"]), amax=torch.stack([t.abs().max() for t in taps]).max().reshape(1).contiguous())


@pytest.fixture(scope="module")
def second_view():
    """image 1: taps, its oracle maps and an ordinary camera -- the other view of the pooled entries"""
    taps = L.synthetic_taps(1)
    return dict(taps=taps, maps=MR.view_maps([t.copy() for t in taps])[0], cam=O.synth_trans_mat(30.0, 25.0, 0.8).astype(np.float32),
                emb=L.embedding(1))


# ---- gather-only entries: bit for bit, no point left out -----------------------------------------------------------
def test_project(world):
    w = world
    xy = host(w["ops"].project(w["pts_d"], w["cam_d"]))[0]
    same_bits("project", xy, w["lat"]["table"])
    assert np.isnan(xy[w["lat"]["nan"]]).all()
    line("ops.project", "project_kernel", w["n"], 0, None)


def test_gather_raw_xy(world):
    w = world
    xy = L.raw_xy_table(_HAND_PLACED)
    got = host(w["ops"].gather(w["fm_d"], dev(xy[None])))[0]
    same_bits("gather", got, L.oracle_rows(w["fm"], xy))
    line("ops.gather (raw xy, with -1, 137, -0.0, NaN, +-inf)", "gather_kernel", len(xy), 0, None)


def test_gather_taps_thread_per_float4(world):
    w = world
    got = host(w["ops"].gather_taps(w["taps"], w["cam_d"], w["pts_d"]))[0]
    same_bits("gather_taps", got, w["rows"])
    assert not got[w["lat"]["nan"]].any()
    line("ops.gather_taps (1 image)", "project_gather_taps_kernel", w["n"], 0, None)


@pytest.fixture(scope="module")
def six_images(world):
    """6 images x 2048 points in one call (>= 10240 points: one wave per point): image 0 is the module's, the others
    are drawn on the device; every image gets the lattice, repeated to 2048 points and rolled by a different amount"""
    w = world
    B, N = 6, 2048
    g = torch.Generator(device="cuda").manual_seed(6)
    taps = [torch.cat([t] + [torch.randn(t.shape, generator=g, device="cuda") for _ in range(B - 1)]).contiguous()
            for t in w["taps"]]
    idx = np.stack([(np.arange(N) + 131 * b) % w["n"] for b in range(B)])
    pts = dev(w["lat"]["pts"][idx])
    cams = dev(np.repeat(w["lat"]["camera"], B, axis=0))
    amax = torch.stack([torch.stack([t[b].abs().max() for t in taps]).max() for b in range(B)]).contiguous()
    return dict(B=B, N=N, taps=taps, idx=idx, pts=pts, cams=cams, amax=amax)


def test_gather_taps_one_wave_per_point(world, six_images):
    w, s = world, six_images
    ops = w["ops"]
    wave = ops.gather_taps(s["taps"], s["cams"], s["pts"])
    same_bits("gather_taps, image 0 of six", host(wave[0]), w["rows"][s["idx"][0]])
    for b in range(s["B"]):
        one = ops.gather_taps([t[b:b + 1].contiguous() for t in s["taps"]], s["cams"][b:b + 1].contiguous(),
                              s["pts"][b:b + 1].contiguous())
        assert torch.equal(one[0], wave[b]), "image %d of the six-image call differs from the image alone" % b
    line("ops.gather_taps (6 images x 2048)", "project_gather_taps_wave_kernel", s["B"] * s["N"], 0, None)


def test_gather_taps_split_thread_per_float4(world):
    w = world
    got = host(w["ops"].gather_taps_split(w["taps"], w["cam_d"], w["pts_d"], w["amax"]))[0]
    want = E.split_rows(w["rows"], float(w["amax"][0]))
    assert np.array_equal(got, want), "%d bytes differ" % (got != want).sum()
    line("ops.gather_taps_split (1 image)", "project_gather_taps_kernel, split form", w["n"], 0, None)


def test_gather_taps_split_one_wave_per_point(world, six_images):
    w, s = world, six_images
    ops = w["ops"]
    got = ops.gather_taps_split(s["taps"], s["cams"], s["pts"], s["amax"])
    want0 = E.split_rows(w["rows"][s["idx"][0]], float(s["amax"][0]))
    assert np.array_equal(host(got[0]), want0), "image 0: %d bytes differ" % (host(got[0]) != want0).sum()
    rows = host(ops.gather_taps(s["taps"], s["cams"], s["pts"]))        # (the fp32 rows: the test above holds them)
    for b in range(1, s["B"]):
        assert np.array_equal(host(got[b]), E.split_rows(rows[b], float(s["amax"][b]))), "image %d" % b
    line("ops.gather_taps_split (6 images x 2048)", "project_gather_taps_wave_kernel, split form", s["B"] * s["N"], 0, None)


@pytest.mark.parametrize("pool", ["max", "mean"])
def test_gather_taps_pool(world, second_view, pool):
    """V = 2: the lattice camera for view 0, an ordinary camera for view 1"""
    w, v = world, second_view
    cams = np.stack([w["lat"]["camera"][0], v["cam"]])
    taps = [torch.cat([a, dev(b)]).contiguous() for a, b in zip(w["taps"], v["taps"])]
    want = MR.gather_pool([[w["fm"]], v["maps"]], cams, w["lat"]["pts"], pool)
    got = host(w["ops"].gather_taps_pool(taps, dev(cams), w["pts_d"][0], pool))
    same_bits("gather_taps_pool %s" % pool, got, want)
    line("ops.gather_taps_pool (V = 2, %s)" % pool, "gather_taps_pool_kernel", w["n"], 0, None)


def test_gather_fold(world):
    """relu(pre + resample(pmap) + bias), compared as test_gather_fold_one_point compares it"""
    w = world
    rng = np.random.default_rng(3)
    n = w["n"]
    pmap = rng.standard_normal((137 * 137, 512)).astype(np.float32)
    pre, bias = rng.standard_normal((n, 512)).astype(np.float32), rng.standard_normal(512).astype(np.float32)
    g = L.oracle_rows(pmap.reshape(1, 137, 137, 512), w["lat"]["table"])
    got = host(w["ops"].gather_fold(dev(pmap), w["cam_d"], w["pts_d"][0], dev(pre), dev(bias)))
    exact = pre.astype(np.float64) + g + bias
    bound = 3 * 2.0 ** -24 * (np.abs(pre) + np.abs(g) + np.abs(bias)).astype(np.float64)
    err = np.abs(got - np.maximum(exact, 0))
    k = np.unravel_index(np.argmax(err / (bound + 1e-30)), err.shape)       # the element that uses most of its bound
    line("ops.gather_fold", "gather_fold_kernel", n, err[k], bound[k])
    assert (err <= bound + 1e-30).all(), "%d elements, first rows %s" % (
        (err > bound + 1e-30).sum(), np.unique(np.argwhere(err > bound + 1e-30)[:, 0])[:8].tolist())


# ---- the point MLP behind the gather: the float64 decoder on the oracle's rows, no point left out -------------------
@pytest.mark.parametrize("entry", ["query", "query_folded", "query_fused", "query_taps_fused"])
def test_query_entries(world, entry):
    """pts -> the gather (the lattice, its NaN point included: zero features), pts_rot -> the MLP (ordinary points)"""
    w = world
    ops, mlp, n = w["ops"], w["mlp"], w["n"]
    rot = L.mlp_points(n)
    rot_d = dev(rot)
    ref = L.decoder64(w["rows"], rot[0], w["emb"], w["W"])
    if entry == "query":
        got, kernel, rtol = ops.query(mlp, w["fm_d"], w["emb_d"], w["cam_d"], w["pts_d"], rot_d), "project_gather_kernel", RTOL
    elif entry == "query_taps_fused":
        got = ops.query_taps_fused(mlp, w["taps"], w["emb_d"], w["cam_d"], w["pts_d"], rot_d)
        kernel, rtol = "project_gather_taps_kernel (split form) + mlp_fused_small", 0.0
    else:
        pmap = ops.fold_local(mlp, w["fm_d"][0]).reshape(1, 137 * 137, 512)
        if entry == "query_folded":
            got, kernel, rtol = ops.query_folded(mlp, pmap, w["emb_d"], w["cam_d"], w["pts_d"], rot_d), "gather_fold_kernel", RTOL
        else:
            got = ops.query_fused(mlp, pmap, ops.amax(pmap), w["emb_d"], w["cam_d"], w["pts_d"], rot_d)
            kernel, rtol = "mlp_fused_kernel (fm_project_taps)", 0.0
    got = host(got)[0].astype(np.float64)
    err, tol = np.abs(got - ref), ATOL + rtol * np.abs(ref)
    k = int(np.argmax(err - tol))
    line("ops.%s" % entry, kernel, n, err[k], tol[k])
    print("   max |d| %.3g, |pred| max %.3g" % (err.max(), np.abs(ref).max()))
    bad = ~(err <= tol)
    assert not bad.any(), "%d points, first %s: raw coordinates %s" % (
        bad.sum(), np.nonzero(bad)[0][:8].tolist(), w["lat"]["raw"][np.nonzero(bad)[0][:8]].tolist())


@pytest.mark.parametrize("pool", ["max", "mean"])
def test_query_views(world, second_view, pool):
    """the same point goes to the gather and the MLP: the table without its NaN point"""
    w, v = world, second_view
    ops = w["ops"]
    lat = w["lat0"]
    cams = np.stack([lat["camera"][0], v["cam"]])
    embs = np.concatenate([w["emb"], v["emb"]])
    taps = [torch.cat([a, dev(b)]).contiguous() for a, b in zip(w["taps"], v["taps"])]
    ref = MR.pred_views([[w["fm"]], v["maps"]], embs, cams, lat["pts"], w["W"], pool, dtype=np.float64)
    emb = ops.pool_embedding(dev(embs), pool)
    got = host(ops.query_views(w["mlp"], taps, emb, dev(cams), dev(lat["pts"]), pool)).astype(np.float64)
    err = np.abs(got - ref)
    line("ops.query_views (V = 2, %s)" % pool, "gather_taps_pool_kernel", len(ref), err.max(), MR_ATOL)
    assert got.shape == ref.shape and (err <= MR_ATOL).all(), "first points %s" % np.nonzero(~(err <= MR_ATOL))[0][:8].tolist()


# ---- the gradient: value and tangents on cell lines and clamps ------------------------------------------------------
def test_query_grad(world):
    """against sdf_grad_reference with the near_line (and clamped) exclusions off: the camera makes float32 and float64
    agree on the cell and on the clamp.  The convention is the reference's text: the tangent on a cell line is that of
    the cell the floor rule selects; zero along an axis whose raw coordinate is <= 0 or >= 136.  Only the points within
    MARGIN of a ReLU kink are left out.  The bound is test_gpu_sdf_grad.py's: twice e32, the largest component error of
    the same reference run in numpy float32 on the same points."""
    w = world
    ops, lat = w["ops"], w["lat0"]
    pts, n = lat["pts"], len(lat["pts"])
    ref = R.forward_mode(w["W"], w["emb"][0], w["fm"][0], pts, L.CAMERA, np.float64)
    val = R.forward_mode(w["W"], w["emb"][0], w["fm"][0], pts, L.CAMERA, np.float64, oracle_gather=True)["value"]
    run32 = R.forward_mode(w["W"], w["emb"][0], w["fm"][0], pts, L.CAMERA, np.float32)
    ok = ref["margin"] >= R.MARGIN
    e32 = float(np.abs(run32["grad"].astype(np.float64) - ref["grad"])[ok].max())
    pmap = ops.fold_local(w["mlp"], w["fm_d"][0]).reshape(1, 137 * 137, 512)
    sdf, grad = ops.query_grad(w["mlp"], pmap, w["emb_d"], w["cam_d"], dev(pts[None]))
    sdf, grad = host(sdf)[0].astype(np.float64), host(grad)[0].astype(np.float64)
    err = np.abs(grad - ref["grad"]).max(axis=1)
    on_line = ref["near_line"] & ~ref["clamped"]
    print("\nLATTICE ops.query_grad: kernel grad_local_seed_kernel (project_jac); %d points, %.1f %% comparable (%d on a "
          "cell line, %d clamped among them); value worst %.3g (tolerance %g + %g |ref|); gradient worst %.3g (bound 2 e32 "
          "= %.3g), on a line %.3g, clamped %.3g; |grad| median %.3g" % (
              n, 100 * ok.mean(), (ok & on_line).sum(), (ok & ref["clamped"]).sum(), np.abs(sdf - val).max(), ATOL, RTOL,
              err[ok].max(), 2 * e32, err[ok & on_line].max(), err[ok & ref["clamped"]].max(),
              np.median(np.linalg.norm(ref["grad"], axis=1))))
    assert ok.mean() >= L.GRAD_MIN_SHARE
    assert (np.abs(sdf - val) <= ATOL + RTOL * np.abs(val)).all()                # the value: every point
    bad = ok & ~(err <= 2 * e32)
    assert not bad.any(), "%d points, first %s: raw coordinates %s" % (
        bad.sum(), np.nonzero(bad)[0][:8].tolist(), lat["raw"][np.nonzero(bad)[0][:8]].tolist())


# ---- the backward of the gather: the adjoint identity ---------------------------------------------------------------
def test_gather_backward_adjoint(world):
    """<gather(fm, xy), dfeat> = <fm, gather_backward(dfeat, xy)> in float64 on the full raw-xy table, the left side from
    the oracle's rows.  The tolerance is test_gather_backward_edges' 1e-6, here of the sum of the magnitudes of the
    terms of the inner product (a rigorous bound: every term w * dfeat * fm is formed with a handful of float32
    roundings of 6e-8 each).  That sum grows with the number of points, so a slip at ONE point would drown in the whole
    table's tolerance: the identity is asserted for every group of 16 consecutive points (a call each), then for the
    whole table in one call (many points accumulating into the same pixels)."""
    w = world
    ops = w["ops"]
    xy = L.raw_xy_table(_HAND_PLACED)
    n = len(xy)
    dfeat = np.random.default_rng(4).standard_normal((1, n, 1472)).astype(np.float32)
    terms = L.oracle_rows(w["fm"], xy).astype(np.float64) * dfeat[0]
    fm64 = w["fm_d"].double().reshape(-1)
    xy_d, dfeat_d = dev(xy[None]), dev(dfeat)
    worst, worst_tol = 0.0, 1.0
    for a in list(range(0, n, 16)) + [None]:
        sl = slice(0, n) if a is None else slice(a, min(a + 16, n))
        dmap = ops.gather_backward(dfeat_d[:, sl].contiguous(), xy_d[:, sl].contiguous())
        rhs = float(torch.dot(dmap.reshape(-1).double(), fm64))
        lhs, tol = float(terms[sl].sum()), 1e-6 * float(np.abs(terms[sl]).sum())
        assert np.isfinite(rhs) and abs(lhs - rhs) <= tol + 1e-30, "points %s: |%r - %r| > %g, raw coordinates %s" % (
            sl, lhs, rhs, tol, xy[sl].tolist())
        if tol > 0 and abs(lhs - rhs) / tol > worst / worst_tol:
            worst, worst_tol = abs(lhs - rhs), tol
    line("ops.gather_backward (groups of 16 points and the whole table)", "gather_bwd_kernel", n, worst, worst_tol)
    # nothing of a point outside the resampler's range reaches the map
    with np.errstate(invalid="ignore"):
        outside = ~((xy > -1).all(axis=1) & (xy < 137).all(axis=1))
    assert outside.sum() >= 12 and not terms[outside].any()
    only = ops.gather_backward(dfeat_d[:, outside].contiguous(), xy_d[:, outside].contiguous())
    assert not bool(only.any())

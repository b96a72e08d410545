"""The entries whose argument checks gained a bound (sizes beyond the index arithmetic are DISN_E_SHAPE; a missing
Cin / C / workspace check; tests/test_abi_errors_host.py) still admit what they must: here at their smallest legal shape,
against the reference and under the tolerance of the entry's own test at ordinary shapes.  One workgroup, one element
per lane at the most: a bound that refused too much, or a tile path that assumed a full tile, shows here.

Entries whose smallest shape already runs elsewhere are not repeated: disn_nn_distance / disn_approx_match /
disn_match_cost / disn_emd at (1, 1, 1) (test_gpu_metrics.py); disn_conv3x3_backward (1, 1, 1, 64, 64) and (1, 1, 1, 3, 64),
disn_dense_backward (1, 64, 64), disn_maxpool2x2_backward (1, 2, 2, 4), disn_resize_bilinear_backward (1, 1, 1, 4),
disn_gather_backward (1, 1) (train_edge_shapes.py); disn_query_grad and disn_query_fused at (1, 1) (test_gpu_sdf_grad.py,
test_gpu_fused.py); disn_cam_head, disn_cam_loss_backward and disn_cam_train_step at B = 1, N = 1 (test_gpu_cam_train.py);
disn_assemble_batch at B = 1, S = 1 (test_gpu_train_driver.py); disn_voxel_surface at one triangle (test_gpu_voxel.py)."""
import numpy as np
import pytest
import torch

from conftest import report_close
from oracle import disn_oracle as O

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def ops():
    from disn_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def conv111():
    """B = H = W = 1, Cin = 32, Cout = 64: only the centre tap of the 3 x 3 kernel meets the pixel"""
    rng = np.random.default_rng(111)
    x = rng.standard_normal((1, 1, 1, 32)).astype(np.float32)
    w = (rng.standard_normal((3, 3, 32, 64)) * np.sqrt(2.0 / (9 * 32))).astype(np.float32)
    b = rng.standard_normal(64).astype(np.float32)
    return x, w, b, O.conv2d(x, w, b, "SAME", True, dtype=np.float64)


@pytest.mark.parametrize("form", ["cost model", "planned 64,64,-1", "planned 128,64,1", "x3"])
def test_conv3x3_one_pixel(ops, conv111, form):
    x, w, b, ref = conv111
    if form == "x3":
        got = ops.conv3x3_x3(dev(x), ops.pack_kn_x3(dev(w.reshape(-1, 64))), dev(b), 64, True)
    else:
        plan = tuple(int(v) for v in form.split()[1].split(",")) if form.startswith("planned") else None
        got = ops.conv3x3(dev(x), ops.pack_kn(dev(w.reshape(-1, 64))), dev(b), 64, True, plan=plan)
    report_close("conv3x3 %s (1, 1, 1, 32, 64)" % form, host(got), ref, atol=1e-5, rtol=1e-5)   # test_conv3x3_vs_oracle's


def test_maxpool_and_its_backward_one_window(ops):
    x = np.array([[[[1, -2, 3, 0], [5, -1, 3, 0]], [[2, -3, 3, 0], [4, -4, 7, 0]]]], np.float32)    # [1, 2, 2, 4]
    assert np.array_equal(host(ops.maxpool2x2(dev(x))), O.max_pool_2x2(x))
    dy = np.array([[[[10, 20, 30, 40]]]], np.float32)
    dx = host(ops.maxpool2x2_backward(dev(x), dev(dy)))
    want = np.zeros_like(x)
    want[0, 0, 1, 0], want[0, 0, 1, 1], want[0, 1, 1, 2] = 10, 20, 30      # the window's maximum
    want[0, 0, 0, 3] = 40                                                    # a tie: the first of the window
    assert np.array_equal(dx, want)


@pytest.mark.parametrize("shape,out", [((1, 1, 1, 1), 1), ((1, 1, 1, 4), 2), ((1, 2, 2, 3), 1)])
def test_resize_smallest(ops, shape, out):
    x = np.random.default_rng(sum(shape)).standard_normal(shape).astype(np.float32)
    assert np.array_equal(host(ops.resize_bilinear(dev(x), out, out)), O.resize_bilinear_legacy(x, out, out))


@pytest.mark.parametrize("K", [1, 4])
def test_fc_one_row(ops, K):
    rng = np.random.default_rng(K)
    x = np.maximum(rng.standard_normal((1, K)), 0).astype(np.float32)
    w = rng.standard_normal((K, 256)).astype(np.float32)
    b = rng.standard_normal(256).astype(np.float32)
    ref = x.astype(np.float64) @ w.astype(np.float64) + b
    report_close("fc (1, %d, 256)" % K, host(ops.fc(dev(x), dev(w), dev(b), False)), ref, atol=1e-5, rtol=1e-5)
    if K % 4 == 0:                                        # disn_fc_t: K % 4 == 0, any N
        got = host(ops.fc_t(dev(x), dev(np.ascontiguousarray(w.T[:1])), dev(b[:1]), False))
        report_close("fc_t (1, %d, 1)" % K, got, ref[:, :1], atol=1e-5, rtol=1e-5)


def test_dense_one_row(ops):
    rng = np.random.default_rng(32)
    a = rng.standard_normal((1, 32)).astype(np.float32)
    w = (rng.standard_normal((32, 64)) * 0.25).astype(np.float32)
    b = rng.standard_normal(64).astype(np.float32)
    ref = np.maximum(a.astype(np.float64) @ w.astype(np.float64) + b, 0)
    got = host(ops.dense(dev(a), ops.pack_kn(dev(w)), dev(b), 64, True))
    report_close("dense (1, 32, 0, 64)", got, ref, atol=1e-5, rtol=1e-5)           # test_dense_concat_vs_oracle's


def test_scale_channels_one_row(ops):
    x = np.array([[3.0, -5.0, 0.5, 7.0]], np.float32)
    s = np.array([2.0, 0.25, 4.0, 1.0], np.float32)
    assert np.array_equal(host(ops.scale_channels(dev(x), dev(s))), x * s)
    assert np.array_equal(host(ops.scale_channels(dev(x), dev(s), invert=True)), x / s)


def test_project_and_gather_one_point(ops):
    pts = np.array([[[0.1, -0.2, 0.05]]], np.float32)
    xy = host(ops.project(dev(pts), dev(O.DEMO_TRANS_MAT)))
    ref = O.get_img_points(pts, O.DEMO_TRANS_MAT)
    assert xy.shape == (1, 1, 2) and np.array_equal(xy, ref)
    fm = np.random.default_rng(7).standard_normal((1, 137, 137, 1472)).astype(np.float32)
    assert np.array_equal(host(ops.gather(dev(fm), dev(ref))), O.resampler(fm, ref))


def test_get_loss_one_value(ops):
    pred, gt = np.array([[0.37]], np.float32), np.array([[-0.021]], np.float32)
    got = host(ops.get_loss(dev(pred), dev(gt), 10.0, 4.0, regularization=0.25))
    want = O.get_loss(pred, gt)
    for i, nm in enumerate(("accuracy", "sdf_loss_realvalue", "sdf_loss")):                # the memory-contract scenario's bounds
        assert abs(float(got[i]) - want[nm]) <= 1e-4 * max(1.0, abs(want[nm])), nm
    assert float(got[3]) == 0.25
    assert abs(float(got[4]) - (want["sdf_loss"] + 0.25)) <= 1e-4 * max(1.0, want["sdf_loss"])


def test_conv1_1_one_pixel(ops):
    rng = np.random.default_rng(1)
    x = rng.random((1, 1, 1, 3)).astype(np.float32)
    w = (rng.standard_normal((3, 3, 3, 64)) * np.sqrt(2.0 / 27)).astype(np.float32)
    b = (rng.standard_normal(64) * 0.1).astype(np.float32)
    ref = O.conv2d(x, w, b, "SAME", True, dtype=np.float64)
    out, amax = ops.conv1_1(dev(x), dev(w), dev(b), True, want_amax=True)
    report_close("conv1_1 (1, 1, 1)", host(out), ref, atol=2e-6, rtol=2e-6)         # test_conv1_1_direct_vs_float64's
    assert float(amax) == float(np.abs(host(out)).max())


@pytest.mark.parametrize("entry", ["conv3x3_h2", "conv3x3_bf16 nsplit 3"])
def test_two_term_and_three_term_convolutions_one_pixel(ops, entry):
    """(1, 1, 1, 64, 64): the smallest shape of disn_conv3x3_h2 (Cin, Cout multiples of 64) and a legal one of
    disn_conv3x3_bf16; 2e-6 of the output scale against float64, the bar of tests/test_gpu_conv_h2.py / test_gpu_bf16.py"""
    rng = np.random.default_rng(64)
    x = np.maximum(rng.standard_normal((1, 1, 1, 64)), 0).astype(np.float32)
    w = (rng.standard_normal((3, 3, 64, 64)) / np.sqrt(4.5 * 64)).astype(np.float32)
    b = (0.1 * rng.standard_normal(64)).astype(np.float32)
    ref = O.conv2d(x, w, b, "SAME", True, dtype=np.float64)
    if entry == "conv3x3_h2":
        got = ops.conv3x3_h2(dev(x), ops.pack_conv_h2(dev(w)), dev(b), 64, True)
    else:
        got = ops.conv3x3_bf16(dev(x), dev(w), dev(b), True, nsplit=3)
    report_close("%s (1, 1, 1, 64, 64)" % entry, host(got), ref, atol=2e-6 * float(np.abs(ref).max()))


def test_dense_bf16_and_dense_h2_one_row(ops):
    rng = np.random.default_rng(65)
    a = np.maximum(rng.standard_normal((1, 64)), 0).astype(np.float32)
    w = (rng.standard_normal((64, 64)) / 8).astype(np.float32)
    b = rng.standard_normal(64).astype(np.float32)
    ref = np.maximum(a.astype(np.float64) @ w.astype(np.float64) + b, 0)
    scale = float(np.abs(ref).max())
    got3 = host(ops.dense_bf16(dev(a), dev(w), dev(b), True, None, nsplit=3))
    report_close("dense_bf16 3-term (1, 64, 64)", got3, ref, atol=2e-6 * scale)     # test_dense_three_term_split_is_fp32_accurate's
    out = ops.dense_h2(dev(a), ops.pack_dense_h2(dev(w)), dev(b), 64, True)
    report_close("dense_h2 (1, 64, 64)", host(out), ref, atol=2e-6 * scale)         # test_layer_shapes_vs_float64's


# ---------------------------------------------------------------- one image, one point through the point MLPs --------
@pytest.fixture(scope="module")
def one_point():
    """B = 1, N = 1 (V = 1): taps, map, embedding, camera, point; the oracle's feature row (float32, bit-exact rows D-F)
    and the float64 decoder on it -- computed once for the tests below"""
    from disn_amd.engine import DeviceWeights
    from disn_amd.weights import WeightStore
    from disn_amd import ops as _ops
    store = WeightStore.random_init(0, mode="he")
    dw = DeviceWeights(store, torch.device("cuda", 0), equalise=False)
    rng = np.random.default_rng(42)
    taps = [np.maximum(rng.standard_normal((1, hw, hw, ch)), 0).astype(np.float32) for hw, ch in _ops.TAP_SHAPES]
    fm = np.concatenate([O.resize_bilinear_legacy(t, 137, 137) for t in taps], axis=3)
    emb = rng.standard_normal((1, 1024)).astype(np.float32)
    tm = O.DEMO_TRANS_MAT[:1].copy()
    pts = np.array([[[0.11, -0.23, 0.07]]], np.float32)
    feat = O.resampler(fm, O.get_img_points(pts, tm))
    W = store.arrays
    g64 = O.get_sdf_basic2(pts, emb, W, dtype=np.float64)[..., 0]
    l64 = O.get_sdf_basic2_imgfeat_twostream(pts, feat[:, :, None, :], W, dtype=np.float64)[..., 0]
    return dict(mlp=dw.mlp, keep=dw, taps=[dev(t) for t in taps], fm=dev(fm), emb=dev(emb), tm=dev(tm), pts=dev(pts),
                feat=feat, sdf64=g64 + l64)


def test_gathers_from_the_taps_one_point(ops, one_point):
    from tests import fused_emulation as E
    p = one_point
    got = host(ops.gather_taps(p["taps"], p["tm"], p["pts"]))
    assert got.shape == (1, 1, 1472) and np.array_equal(got, p["feat"])            # rows D + E + F, bit for bit
    for pool in ("max", "mean"):                                                     # one view: the row itself
        assert np.array_equal(host(ops.gather_taps_pool(p["taps"], p["tm"], p["pts"][0], pool)), p["feat"][0])
    amax = torch.stack([t.abs().max() for t in p["taps"]]).max().reshape(1).contiguous()
    split = host(ops.gather_taps_split(p["taps"], p["tm"], p["pts"], amax))
    assert np.array_equal(split[0], E.split_rows(p["feat"][0], float(amax[0])))


def test_gather_fold_one_point(ops, one_point):
    p = one_point
    rng = np.random.default_rng(3)
    pmap = rng.standard_normal((137 * 137, 512)).astype(np.float32)
    pre, bias = rng.standard_normal((1, 512)).astype(np.float32), rng.standard_normal(512).astype(np.float32)
    g = O.resampler(pmap.reshape(1, 137, 137, 512), O.get_img_points(host(p["pts"]), host(p["tm"])))[0]
    got = host(ops.gather_fold(dev(pmap), p["tm"], p["pts"][0], dev(pre), dev(bias)))
    exact = pre.astype(np.float64) + g + bias
    bound = 3 * 2.0 ** -24 * (np.abs(pre) + np.abs(g) + np.abs(bias)).astype(np.float64)   # the gather scenario's bound
    assert (np.abs(got - np.maximum(exact, 0)) <= bound + 1e-30).all()


@pytest.mark.parametrize("entry", ["sdf_mlp", "query", "query_folded", "query_views", "query_taps_fused"])
def test_point_mlp_entries_one_point(ops, one_point, entry):
    """pred_sdf of one point of one image against the float64 decoder: 1e-5, the bar of every form"""
    p = one_point
    if entry == "sdf_mlp":
        got = ops.sdf_mlp(p["mlp"], p["pts"], p["emb"], dev(p["feat"]))
    elif entry == "query":
        got = ops.query(p["mlp"], p["fm"], p["emb"], p["tm"], p["pts"])
    elif entry == "query_folded":
        pmap = ops.fold_local(p["mlp"], p["fm"][0])
        got = ops.query_folded(p["mlp"], pmap.reshape(1, 137 * 137, 512), p["emb"], p["tm"], p["pts"])
    elif entry == "query_views":
        got = ops.query_views(p["mlp"], p["taps"], p["emb"], p["tm"], p["pts"][0])
    else:
        got = ops.query_taps_fused(p["mlp"], p["taps"], p["emb"], p["tm"], p["pts"])
    report_close("%s (1, 1)" % entry, host(got).reshape(1, 1), p["sdf64"], atol=1e-5, rtol=1e-5)

"""GPU parity of the camera network's training (disn_cam_train_step, disn_cam_loss_backward, train_cam.CamTrainer)
against the float64 autograd restatement in tests/cam_train_reference.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cam_train_reference as R  # noqa: E402
from conftest import report_close  # noqa: E402
from oracle import cam_oracle as CO  # noqa: E402
from oracle import disn_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ("3D", "2D", "3DM", "ALL")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def head_weights(seed, case="random"):
    """He-scaled towers; fc3 of scale / translation kept small so that s ~ 1 and z stays well away from 0.
    near_degenerate: ortho6d = fixed a, b with |x × b| = 1e-3; below_eps: |x × b| = 1e-9 (the max(|v|, 1e-8)
    branch).  Axis-aligned a makes x and x × b exact in both precisions."""
    w = CO.init_weights(seed)
    w["cameraprediction/scale/fc3/weights"] *= 0.05
    w["cameraprediction/scale/fc3/biases"][:] = 1.0
    w["cameraprediction/translation/fc3/weights"] *= 0.05
    w["cameraprediction/translation/fc3/biases"][:] = 0.0
    if case != "random":
        w["cameraprediction/ortho6d/fc3/weights"][:] = 0.0
        eps = 1e-3 if case == "near_degenerate" else 1e-9
        w["cameraprediction/ortho6d/fc3/biases"][:] = np.array([1.5, 0, 0, 2.0, eps, 0], np.float32)
    return w


def head_inputs(seed, B=4, N=2048):
    rng = np.random.default_rng(seed)
    RT, tm = R.synth_camera(rng, B)
    emb = rng.standard_normal((B, 1024)).astype(np.float32)
    pts = ((rng.random((B, N, 3)) - 0.5) * 0.9).astype(np.float32)
    return emb, pts, RT, tm


def run_head(w, emb, pts, RT, tm, mode):
    from disn_amd import ops
    from disn_amd.posenet import CameraHead
    h = CameraHead(w)
    out = ops.cam_loss_backward(h.w, dev(emb), dev(pts), dev(RT), dev(tm), mode)
    torch.cuda.synchronize()
    return h, {k: host(v) for k, v in out.items()}


def head_grad_views(flat):
    from disn_amd import ops
    from disn_amd.posenet import variable_shapes
    L = ops.cam_param_layout()
    out = {}
    for j, (name, shp) in enumerate(variable_shapes().items()):
        o = int(L.offset[32 + j] - L.offset[32])
        out[name] = flat[o:o + int(L.count[32 + j])].reshape(shp)
    return out


# ------------------------------------------------------------------ the new kernels alone ----------------------------
@pytest.mark.parametrize("case", ["random", "near_degenerate", "below_eps"])
@pytest.mark.parametrize("mode", MODES)
def test_head_losses_and_gradients(case, mode):
    check_head(case, mode)


@pytest.mark.parametrize("mode", MODES)
def test_head_at_one_image_and_one_point(mode):
    """B = 1, N = 1: the smallest call disn_cam_loss_backward and disn_cam_head admit, same reference, same bounds"""
    check_head("random", mode, B=1, N=1)


def check_head(case, mode, B=4, N=2048):
    w = head_weights(5, case)
    emb, pts, RT, tm = head_inputs(7, B=B, N=N)
    h, got = run_head(w, emb, pts, RT, tm, mode)
    assert np.array_equal(got["pred_trans_mat"], host(h.run(dev(emb))[3]))       # disn_cam_head on the same embedding
    ref, g, ptm = R.head_loss_and_grads(emb, w, pts, RT, tm, mode)
    for i, n in enumerate(("rotpc_loss", "rot2d_loss", "rotmatrix_loss", "rot2d_dist", "rot3d_dist")):
        assert abs(got["losses"][i] - ref[n]) <= 1e-5 * abs(ref[n]) + 1e-12, (n, got["losses"][i], ref[n])
    assert got["losses"][5] == 0.0
    assert abs(got["losses"][6] - ref["overall_loss"]) <= 1e-5 * abs(ref["overall_loss"]), (got["losses"][6], ref)
    report_close("rot2d_dist_all", got["dists"][0], ref["rot2d_dist_all"], atol=0, rtol=1e-5)
    report_close("rot3d_dist_all", got["dists"][1], ref["rot3d_dist_all"], atol=0, rtol=1e-5)
    report_close("pred_trans_mat", got["pred_trans_mat"], ptm, atol=1e-5 * np.abs(ptm).max())

    def near(name, a, b):
        report_close(name, a, b, atol=1e-5 * max(float(np.abs(b).max()), 1e-30))

    near("dRT", got["dRT"], g["pred_RT"])
    near("demb", got["demb"], g["embedding"])
    hg = head_grad_views(got["head_grads"])
    for name in hg:
        near(name, hg[name], g[name])


def test_head_training_forward_is_the_inference_head():
    """the head forward of training (cam_head_kernel with its save pointers) is bit-identical to disn_cam_head"""
    w = head_weights(3)
    emb, pts, RT, tm = head_inputs(4, B=8, N=512)
    h, got = run_head(w, emb, pts, RT, tm, "3D")
    _, _, _, ref = h.run(dev(emb))
    assert np.array_equal(got["pred_trans_mat"], host(ref))


def test_head_kernels_are_bitwise_repeatable():
    w = head_weights(9, "near_degenerate")
    emb, pts, RT, tm = head_inputs(10, B=32, N=2048)
    _, a = run_head(w, emb, pts, RT, tm, "ALL")
    _, b = run_head(w, emb, pts, RT, tm, "ALL")
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ------------------------------------------------------------------ the whole step ----------------------------------
def cam_weights(seed):
    vgg = O.init_weights(3, "he")
    out = {k: v for k, v in vgg.items() if k.startswith("vgg_16/")}
    out.update(head_weights(seed))
    return out


def dev_feed(feed):
    return {k: dev(feed[k]) for k in ("imgs", "sample_pc", "RT", "trans_mat")}


@pytest.fixture(scope="module")
def step_case():
    B, N = 2, 256
    weights = cam_weights(11)
    feed = R.synth_feed(21, B, N)
    refs = {m: R.loss_and_grads(feed, weights, m) for m in ("3D", "ALL")}
    return dict(weights=weights, feed=feed, refs=refs, B=B, N=N)


@pytest.fixture(scope="module")
def smallest_step_case():
    """B = 1, N = 1: the smallest step disn_cam_train_step admits"""
    weights = cam_weights(11)
    feed = R.synth_feed(23, 1, 1)
    return dict(weights=weights, feed=feed, refs={"3D": R.loss_and_grads(feed, weights, "3D")}, B=1, N=1)


def test_step_losses_at_one_image_and_one_point(smallest_step_case):
    s = smallest_step_case
    ref = s["refs"]["3D"][0]
    _, tm, losses, dists = run_step(s, "3D", "f32")
    from disn_amd.train_cam import LOSS_NAMES
    for i, n in enumerate(LOSS_NAMES):
        want = mode_total(ref, "3D") if n == "overall_loss" else ref[n]
        assert abs(losses[i] - want) <= 1e-5 * abs(want) + 1e-9, (n, losses[i], want)     # test_step_losses' bounds
    report_close("rot3d_dist_all", dists[1], ref["rot3d_dist_all"], atol=0, rtol=1e-5)
    report_close("pred_trans_mat", tm, s["refs"]["3D"][2], atol=1e-5 * np.abs(tm).max())


def run_step(s, mode, precision):
    from disn_amd.train_cam import CamTrainer
    tr = CamTrainer(s["weights"], batch_size=s["B"], loss_mode=mode, precision=precision)
    tm, losses, dists = tr.forward_backward(dev_feed(s["feed"]))
    torch.cuda.synchronize()
    return tr, host(tm), host(losses), host(dists)


def mode_total(ref_losses, mode):
    w3, w2, wm = R.mode_weights(mode)
    return (w2 * ref_losses["rot2d_loss"] + w3 * ref_losses["rotpc_loss"] + wm * ref_losses["rotmatrix_loss"]
            + ref_losses["regularization"])


def gradient_rows(got, ref_grads):
    rows = []
    for name, ref in ref_grads.items():
        g = got[name].astype(np.float64).ravel()
        r = np.asarray(ref, np.float64).ravel()
        l2 = float(np.linalg.norm(g - r) / max(np.linalg.norm(r), 1e-30))
        cos = float(g @ r / max(np.linalg.norm(g) * np.linalg.norm(r), 1e-30))
        rows.append((l2, cos, name))
    rows.sort(reverse=True)
    return rows


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("mode", MODES)
def test_step_losses(step_case, mode, precision):
    s = step_case
    ref = s["refs"]["3D"][0]
    _, tm, losses, dists = run_step(s, mode, precision)
    from disn_amd.train_cam import LOSS_NAMES
    for i, n in enumerate(LOSS_NAMES):
        want = mode_total(ref, mode) if n == "overall_loss" else ref[n]
        assert abs(losses[i] - want) <= 1e-5 * abs(want) + 1e-9, (n, losses[i], want)
    report_close("rot3d_dist_all", dists[1], ref["rot3d_dist_all"], atol=0, rtol=1e-5)
    report_close("pred_trans_mat", tm, s["refs"]["3D"][2], atol=1e-5 * np.abs(tm).max())


@pytest.mark.parametrize("mode,precision", [("3D", "f32"), ("ALL", "f32"), ("3D", "bf16")])
def test_step_gradients(step_case, mode, precision):
    """flip-tolerant, as test_gpu_train.py::test_train_step_gradients: relative L2 < 2e-2 and cosine > 0.9995 per
    variable in fp32; mixed precision (bf16 weight-gradient GEMMs) gets looser bars: relative L2 < 5e-2, cosine > 0.999"""
    s = step_case
    tr, _, _, _ = run_step(s, mode, precision)
    rows = gradient_rows(tr.flat.to_arrays(tr.grads), s["refs"][mode][1])
    print("worst (rel L2, cos):", rows[:4])
    if precision == "f32":
        assert rows[0][0] < 2e-2 and min(c for _, c, _ in rows) > 0.9995, rows[:6]
    else:
        assert rows[0][0] < 5e-2 and min(c for _, c, _ in rows) > 0.999, rows[:6]
    tr.close()


def test_step_pred_trans_mat_is_camera_estimator(step_case):
    """the step's camera equals CameraEstimator.get_model (inference encoder + disn_cam_head) with the same weights"""
    from disn_amd.posenet import CameraEstimator, variable_shapes
    from disn_amd.weights import WeightStore
    s = step_case
    _, tm, _, _ = run_step(s, "3D", "f32")
    vgg = WeightStore(O.init_weights(3, "he"))        # the same VGG (cam_weights); the SDF part is unused
    est = CameraEstimator(vgg, {k: s["weights"][k] for k in variable_shapes()})
    ref = host(est.get_model(s["feed"]["imgs"])["pred_trans_mat"])
    print("bitwise equal:", np.array_equal(tm, ref), "max |diff|:", float(np.abs(tm - ref).max()))
    report_close("pred_trans_mat", tm, ref, atol=2e-6 * np.abs(ref).max())


def test_cam_trainer_adam_matches_oracle(step_case):
    """one step: parameters follow TF Adam (beta1 = 0.9) on the float64 gradients"""
    from disn_amd.train_cam import CamTrainer
    from disn_amd.train_sdf import get_learning_rate
    from oracle import train_oracle as T
    s = step_case
    tr = CamTrainer(s["weights"], batch_size=s["B"], loss_mode="3D")
    assert tr.beta1 == 0.9
    _, losses, lr = tr.step(dev_feed(s["feed"]))
    assert lr == get_learning_rate(0, s["B"])
    got = tr.flat.to_arrays(tr.params)
    grads = s["refs"]["3D"][1]
    for k in ("vgg_16/conv1/conv1_1/weights", "vgg_16/fc8/weights", "cameraprediction/ortho6d/fc1/weights",
              "cameraprediction/translation/fc3/biases", "cameraprediction/scale/fc2/weights"):
        w0 = np.asarray(s["weights"][k], np.float64)
        w1, _, _ = T.adam_step(w0, grads[k], np.zeros_like(w0), np.zeros_like(w0), 1, lr, beta1=0.9)
        big = np.abs(grads[k]) > 1e-3 * np.abs(grads[k]).max()
        report_close(k, (got[k].astype(np.float64) - w0)[big], (w1 - w0)[big], atol=2e-6)
    st = tr.state_arrays(include_step=True)
    assert np.isclose(float(st["beta1_power"]), 0.9 ** 2) and int(st["batch"]) == 1
    tr.close()


def test_cam_trainer_reduces_the_loss(step_case):
    from disn_amd.train_cam import CamTrainer
    s = step_case
    tr = CamTrainer(s["weights"], batch_size=s["B"], loss_mode="3D")
    feed = dev_feed(s["feed"])
    vals = []
    for _ in range(30):
        _, losses, _ = tr.step(feed)
        vals.append(float(losses["overall_loss"]))
    print("overall_loss", vals[0], "->", vals[-1])
    assert np.isfinite(vals).all() and vals[-1] < 0.7 * vals[0], vals
    tr.close()

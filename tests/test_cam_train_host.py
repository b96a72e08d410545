"""CPU checks of the camera network's training: the float64 restatement against finite differences, the M_b form of
the rotpc loss, the parameter layout, the cammat loader, Saver-V2 round trips and the --create writer."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cam_train_reference as R  # noqa: E402
from oracle import cam_oracle as CO  # noqa: E402


def small_head(seed, ortho=None):
    """a narrow stand-in of the head (same code path, 8-wide embedding) for finite differences"""
    rng = np.random.default_rng(seed)
    dims = {"scale": (8, 5, 4, 1), "ortho6d": (8, 6, 5, 6), "translation": (8, 5, 4, 3)}
    w = {}
    for tower, d in dims.items():
        for i in range(3):
            w["cameraprediction/%s/fc%d/weights" % (tower, i + 1)] = rng.standard_normal((d[i], d[i + 1])) * 0.5
            w["cameraprediction/%s/fc%d/biases" % (tower, i + 1)] = rng.standard_normal(d[i + 1]) * 0.1 + 0.2
    w["cameraprediction/scale/fc3/weights"] *= 0.1
    w["cameraprediction/scale/fc3/biases"][:] = 1.0
    w["cameraprediction/translation/fc3/weights"] *= 0.1
    if ortho is not None:
        w["cameraprediction/ortho6d/fc3/weights"][:] = 0.0
        w["cameraprediction/ortho6d/fc3/biases"][:] = ortho
    return w


def fd_check(fn, x, grad, eps=1e-6, n=12, seed=0):
    rng = np.random.default_rng(seed)
    flat = x.reshape(-1)
    for i in rng.choice(flat.size, size=min(n, flat.size), replace=False):
        old = flat[i]
        flat[i] = old + eps
        fp = fn()
        flat[i] = old - eps
        fm = fn()
        flat[i] = old
        num = (fp - fm) / (2 * eps)
        assert abs(num - grad.reshape(-1)[i]) <= 1e-5 * max(1.0, abs(num)), (i, num, grad.reshape(-1)[i])


@pytest.mark.parametrize("mode", ["3D", "2D", "3DM", "ALL"])
@pytest.mark.parametrize("ortho", [None, "near", "below_eps"])
def test_reference_head_gradients_match_finite_differences(mode, ortho):
    o6 = {None: None, "near": np.array([1.5, 0, 0, 2.0, 1e-3, 0.3]),
          "below_eps": np.array([1.5, 0, 0, 2.0, 1e-9, 0.0])}[ortho]
    w = small_head(1, o6)
    rng = np.random.default_rng(2)
    B, N = 2, 16
    emb = rng.standard_normal((B, 8))
    pts = (rng.random((B, N, 3)) - 0.5) * 0.9
    RT, tm = R.synth_camera(rng, B)
    _, g, _ = R.head_loss_and_grads(emb, w, pts, RT, tm, mode)

    def f():
        return R.head_loss_and_grads(emb, w, pts, RT, tm, mode)[0]["overall_loss"]

    fd_check(f, emb, g["embedding"])
    for name in ("cameraprediction/ortho6d/fc3/biases", "cameraprediction/scale/fc2/weights",
                 "cameraprediction/translation/fc1/weights"):
        # below_eps: steps small enough to stay on the constant side of max(|x × b|, 1e-8)
        eps = 1e-11 if ortho == "below_eps" and "ortho6d" in name else 1e-6
        fd_check(f, w[name], g[name], eps=eps)


def test_below_eps_branch_passes_no_gradient_through_the_norm():
    """|x × b| < 1e-8: z = w / 1e-8 exactly, so dz/dw is the constant 1e8 I"""
    v = torch.tensor([[0.0, 0.0, 1e-9]], dtype=torch.float64, requires_grad=True)
    R.normalize(v).sum().backward()
    assert np.allclose(v.grad.numpy(), 1e8)
    u = torch.tensor([[1e-8, 0.0, 0.0]], dtype=torch.float64, requires_grad=True)   # a tie: the norm's branch
    R.normalize(u)[0, 0].backward()
    assert abs(float(u.grad[0, 0])) < 1e-6


def test_projection_gradient_matches_finite_differences():
    rng = np.random.default_rng(3)
    B, N = 2, 32
    pts = (rng.random((B, N, 3)) - 0.5) * 0.9
    RT, tm = R.synth_camera(rng, B)
    pRT = RT.astype(np.float64) + 0.05 * rng.standard_normal(RT.shape)

    def f():
        return float(R.losses(torch.tensor(pRT), pts, RT, tm, "2D")["rot2d_loss"])

    t = torch.tensor(pRT, requires_grad=True)
    R.losses(t, pts, RT, tm, "2D")["rot2d_loss"].backward()
    fd_check(f, pRT, t.grad.numpy(), eps=1e-7)


def test_rotpc_moment_form_equals_point_form():
    rng = np.random.default_rng(4)
    B, N = 3, 500
    pts = (rng.random((B, N, 3)) - 0.5)
    RT, _ = R.synth_camera(rng, B)
    pRT = RT.astype(np.float64) + 0.1 * rng.standard_normal(RT.shape)
    t = torch.tensor(pRT, requires_grad=True)
    L = R.losses(t, pts, RT, RT @ CO.K_DEFAULT.T, "3D")
    L["rotpc_loss"].backward()
    val, MD = R.rotpc_moment_form(pRT, pts, RT)
    assert abs(val - float(L["rotpc_loss"].detach())) <= 1e-12 * abs(val)
    assert np.allclose(MD, t.grad.numpy(), rtol=1e-12, atol=1e-12)


def test_loss_modes():
    assert R.mode_weights("3D") == (1.0, 0.0, 0.0) and R.mode_weights("2D") == (0.0, 1.0, 0.0)
    assert R.mode_weights("3DM") == (1.0, 0.0, 0.3) and R.mode_weights("whatever") == (1.0, 1.0, 1.0)
    from disn_amd import ops
    assert [ops.cam_loss_mode(m) for m in ("3D", "2D", "3DM", "xyz")] == [0, 1, 2, 3]


# ------------------------------------------------------------------ layout ------------------------------------------
def test_cam_param_layout_order_and_names():
    from disn_amd import ops, posenet
    from disn_amd.train_cam import VARIABLE_ORDER, variable_shapes
    from disn_amd.weights import variable_shapes as sdf_shapes
    vgg = [k for k in sdf_shapes() if k.startswith("vgg_16/")]
    assert len(vgg) == 32
    assert list(VARIABLE_ORDER) == vgg + list(posenet.variable_shapes())
    L, S = ops.cam_param_layout(), ops.param_layout()
    shapes = variable_shapes()
    end = 0
    for i, name in enumerate(VARIABLE_ORDER):
        assert L.count[i] == int(np.prod(shapes[name])), name
        assert L.offset[i] % 64 == 0 and L.offset[i] >= end
        end = L.offset[i] + L.count[i]
        if i < 32:
            assert (L.offset[i], L.count[i]) == (S.offset[i], S.count[i])
    assert L.total >= end and L.total % 64 == 0
    # the head variables in disn_cam_weights_t order (s_w1, s_b1, ..., t_b3)
    from disn_amd._lib import CAM_FIELDS
    short = {"scale": "s", "ortho6d": "r", "translation": "t"}
    assert [short[n.split("/")[1]] + "_" + ("w" if n.endswith("weights") else "b") + n.split("/")[2][-1]
            for n in VARIABLE_ORDER[32:]] == list(CAM_FIELDS)


def test_workspace_queries():
    from disn_amd._lib import lib
    h = lib()
    assert h.disn_cam_train_workspace_bytes(0, 5) == 0 and h.disn_cam_train_workspace_bytes(257, 5) == 0
    assert h.disn_cam_train_workspace_bytes(32, 2048) > h.disn_cam_train_workspace_bytes(2, 256) > 0
    assert h.disn_cam_loss_backward_workspace_bytes(4, 2048) > 0 and h.disn_cam_loss_backward_workspace_bytes(0, 1) == 0


# ------------------------------------------------------------------ loader --------------------------------------------
def flags(**kw):
    base = dict(num_points=1, num_sample_points=16, batch_size=2, img_h=137, img_w=137, max_epoch=1, cat_limit=100,
                shift=False, rotation=False)
    base.update(kw)
    return SimpleNamespace(**base)


def make_tree(root, n_obj=2, views=(0, 1), with_k=True):
    from disn_amd.data_cam import save_view_cam
    from disn_amd.data_sdf import save_sample, save_view
    rng = np.random.default_rng(0)
    sdf_dir, ren_dir = os.path.join(root, "sdf"), os.path.join(root, "ren")
    listinfo, truth = [], {}
    for o in range(n_obj):
        obj = "obj%d" % o
        smp = np.concatenate([rng.random((40, 3)) - 0.5, rng.random((40, 1)) * 0.1], 1)
        save_sample(sdf_dir, "03001627", obj, np.concatenate([rng.random((50, 3)), np.zeros((50, 1))], 1), smp,
                    np.array([0, 0, 0, 1]), np.zeros(6))
        for v in views:
            img = rng.integers(0, 256, (137, 137, 4))
            tm, om = rng.standard_normal((4, 3)), np.eye(3)
            reg = rng.standard_normal((4, 3))
            if with_k:
                save_view_cam(ren_dir, "03001627", obj, v, img, tm, om, reg, CO.K_DEFAULT)
            else:
                save_view(ren_dir, "03001627", obj, v, img, tm, om, reg)
            truth[(obj, v)] = (img, tm.astype(np.float32), reg.astype(np.float32))
            listinfo.append(("03001627", obj, v))
    return {"sdf_dir": sdf_dir, "rendered_dir": ren_dir}, listinfo, truth


def test_loader_schema_and_dtypes(tmp_path):
    from disn_amd.data_cam import Pt_sdf_img_cam
    info, listinfo, truth = make_tree(str(tmp_path))
    d = Pt_sdf_img_cam(flags(), listinfo=listinfo, info=info, shuffle=False, seed=0)
    b = d.get_batch(0)
    assert b["img"].shape == (2, 137, 137, 4) and b["img"].dtype == np.float32
    assert b["RT"].shape == (2, 4, 3) and b["RT"].dtype == np.float32
    assert b["shifts"].shape == (2, 2) and not b["shifts"].any()
    assert b["sdf_pt"].shape == (2, 16, 3) and b["sdf_val"].shape == (2, 16, 1) and b["trans_mat"].shape == (2, 4, 3)
    for i, (obj, v) in enumerate(zip(b["obj_nm"], b["view_id"])):
        img, tm, reg = truth[(obj, v)]
        assert np.array_equal(b["img"][i], img.astype(np.float32) / np.float32(255))
        assert np.array_equal(b["RT"][i], reg)           # RT is the view file's regress_mat
        assert np.array_equal(b["trans_mat"][i], tm)


def test_loader_needs_k(tmp_path):
    from disn_amd.data_cam import Pt_sdf_img_cam
    info, listinfo, _ = make_tree(str(tmp_path), with_k=False)
    d = Pt_sdf_img_cam(flags(), listinfo=listinfo, info=info, shuffle=False)
    with pytest.raises(KeyError, match="'K'"):
        d.get_batch(0)


def test_save_view_default_is_unchanged(tmp_path):
    from disn_amd.data_sdf import save_view
    save_view(str(tmp_path), "c", "o", 3, np.zeros((2, 2, 4)), np.zeros((4, 3)), np.eye(3), np.zeros((4, 3)))
    with np.load(os.path.join(str(tmp_path), "c", "o", "03.npz")) as z:
        assert sorted(z.files) == ["img_arr", "obj_rot_mat", "regress_mat", "trans_mat"]


@pytest.mark.parametrize("flag", ["shift", "rotation"])
def test_unsupported_flags_raise(tmp_path, flag):
    from disn_amd.data_cam import Pt_sdf_img_cam
    from disn_amd.train_cam import main
    info, listinfo, _ = make_tree(str(tmp_path))
    with pytest.raises(NotImplementedError, match=flag):
        Pt_sdf_img_cam(flags(**{flag: True}), listinfo=listinfo, info=info)
    with pytest.raises(NotImplementedError, match=flag):
        main(["--" + flag, "--log_dir", str(tmp_path / "log")])


def test_momentum_optimizer_raises(tmp_path):
    from disn_amd.train_cam import main
    with pytest.raises(NotImplementedError, match="momentum"):
        main(["--optimizer", "momentum", "--log_dir", str(tmp_path / "log")])


# ------------------------------------------------------------------ checkpoints + --create -------------------------
class _HostTrainer:
    """CamTrainer's checkpoint half on host buffers (no device needed): the same state_arrays / restore code"""

    def __init__(self, arrays, adam_t):
        from disn_amd.train_cam import CamTrainer, FlatCamParams
        self.__class__ = type("HostCamTrainer", (CamTrainer,), {"close": lambda self: None})
        self.flat = FlatCamParams(torch.device("cpu"))
        self.params = self.flat.from_arrays(arrays)
        rng = np.random.default_rng(1)
        self.m = torch.from_numpy(rng.standard_normal(self.flat.total).astype(np.float32))
        self.v = torch.from_numpy(rng.random(self.flat.total).astype(np.float32))
        self.beta1, self.beta2 = 0.9, 0.999
        self.adam_t, self.step_count = adam_t, adam_t
        self.ctx = None


def test_state_arrays_saver_v2_round_trip(tmp_path):
    from disn_amd import tf_checkpoint as tfc
    from disn_amd.train_cam import VARIABLE_ORDER, random_init
    arrays = random_init(0)
    tr = _HostTrainer(arrays, adam_t=6)
    st = tr.state_arrays(include_step=True)
    assert len(st) == 3 * 50 + 3
    assert np.isclose(float(st["beta1_power"]), 0.9 ** 7, rtol=1e-6)
    assert np.isclose(float(st["beta2_power"]), 0.999 ** 7, rtol=1e-6)
    assert int(st["batch"]) == 6 and st["batch"].dtype == np.int32
    for n in VARIABLE_ORDER:
        assert n + "/Adam" in st and n + "/Adam_1" in st
    prefix = str(tmp_path / "latest.ckpt")
    tfc.save_checkpoint(prefix, st)
    back = tfc.load_checkpoint(prefix)
    assert set(back) == set(st)
    for k in st:
        assert np.array_equal(np.asarray(back[k]), np.asarray(st[k])), k
    fresh = _HostTrainer(random_init(1), adam_t=0)
    fresh.m.zero_()
    fresh.v.zero_()
    assert fresh.restore(prefix) == 150
    assert fresh.adam_t == 6 and fresh.step_count == 6
    for a, b in ((fresh.params, tr.params), (fresh.m, tr.m), (fresh.v, tr.v)):
        fa, fb = fresh.flat.to_arrays(a), tr.flat.to_arrays(b)
        assert all(np.array_equal(fa[k], fb[k]) for k in fa)
    # the reference's --restore_modelcnn: the vgg_16 prefix alone
    other = _HostTrainer(random_init(2), adam_t=0)
    assert other.restore(prefix, ("vgg_16",)) == 96
    got = other.flat.to_arrays(other.params)
    assert np.array_equal(got["vgg_16/fc8/weights"], arrays["vgg_16/fc8/weights"])
    assert not np.array_equal(got["cameraprediction/scale/fc1/weights"], arrays["cameraprediction/scale/fc1/weights"])


def test_create_files_read_back_through_pt_sdf_img(tmp_path):
    from disn_amd.data_cam import Pt_sdf_img_cam, write_estimated_views
    from disn_amd.data_sdf import Pt_sdf_img
    info, listinfo, truth = make_tree(str(tmp_path))
    d = Pt_sdf_img_cam(flags(), listinfo=listinfo, info=info, shuffle=False)
    b = d.get_batch(0)
    pred = np.random.default_rng(5).standard_normal((2, 4, 3)).astype(np.float32)
    est = str(tmp_path / "est")
    paths = write_estimated_views(est, info["rendered_dir"], b, pred)
    assert len(paths) == 2 and all(os.path.exists(p) for p in paths)
    with np.load(paths[0]) as z:
        assert {"img_arr", "trans_mat", "K", "obj_rot_mat", "regress_mat"} <= set(z.files)
        assert np.array_equal(z["K"], CO.K_DEFAULT)
    sd = Pt_sdf_img(flags(), listinfo=listinfo[:2], info={"sdf_dir": info["sdf_dir"], "rendered_dir": est},
                    shuffle=False)
    back = sd.get_batch(0)
    for i, (obj, v) in enumerate(zip(b["obj_nm"], b["view_id"])):
        j = [k for k, (o2, v2) in enumerate(zip(back["obj_nm"], back["view_id"])) if (o2, v2) == (obj, v)][0]
        assert np.array_equal(back["trans_mat"][j], pred[i])
        assert np.array_equal(back["img"][j], b["img"][i][:, :, :3])

"""Float64 torch-CPU restatement of the camera network's training graph (cam_est/model_cam.py get_model / get_loss,
models/posenet.py get_cam_mat) -- TEST INFRASTRUCTURE ONLY.

  forward     imgs[..., :3] -> legacy bilinear resize to 224 -> vgg_16(num_classes=1024) -> embedding [B,1024]
              -> three ReLU towers -> Gram-Schmidt (n(v) = v / max(|v|, 1e-8); x = n(a), z = n(x × b), y = z × x,
              columns x, y, z) -> pred_RT [B,4,3] = [s Rot ; t + const], pred_trans_mat = pred_RT K^T
  losses      homo = [p, 1]; sub_3d = homo pred_RT - homo RT
              rotpc = 1/2 sum sub_3d^2; rot2d = 1/2 sum (pred_xy - gt_xy)^2 / 1e4 (xy = xyz[:2] / xyz[2], unclipped);
              rotmatrix = mean((pred_T - T)^2); regularization = wd * sum over the 16 VGG weights of |w|^2 / 2
              rot2d_dist / rot3d_dist: mean over points of |clip(gt_xy) - clip(pred_xy)| (clip [0,136]) / |sub_3d|
  loss_mode   "3D" rotpc; "2D" rot2d; "3DM" rotpc + 0.3 rotmatrix; anything else rot2d + rotpc + rotmatrix

The VGG part reuses oracle/train_oracle.py's differentiable pieces; the head comes from oracle/cam_oracle.py's
shapes and constants.
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch
import torch.nn.functional as Fnn

from disn_amd.weights import variable_shapes
from oracle import cam_oracle as CO
from oracle import disn_oracle as O
from oracle import train_oracle as T

WD = 2e-3
VGG_NAMES = tuple(k for k in variable_shapes() if k.startswith("vgg_16/"))


def mode_weights(loss_mode: str):
    """-> (w_rotpc, w_rot2d, w_rotmatrix)"""
    return {"3D": (1.0, 0.0, 0.0), "2D": (0.0, 1.0, 0.0), "3DM": (1.0, 0.0, 0.3)}.get(loss_mode, (1.0, 1.0, 1.0))


def normalize(v: torch.Tensor) -> torch.Tensor:
    mag = torch.sqrt((v * v).sum(dim=1, keepdim=True))
    # tf.maximum's gradient goes to the first argument on ties: clamp_min routes it the same way
    return v / torch.clamp_min(mag, 1e-8)


def ortho6d_to_rotation(p: torch.Tensor) -> torch.Tensor:
    x = normalize(p[:, 0:3])
    z = normalize(torch.cross(x, p[:, 3:6], dim=1))
    y = torch.cross(z, x, dim=1)
    return torch.stack([x, y, z], dim=2)


def head(emb: torch.Tensor, Wt: Dict[str, torch.Tensor]):
    """-> (pred_RT [B,4,3], o3 {tower: raw output})"""
    outs = {}
    for tower, _ in CO.TOWERS:
        h = emb
        for i in range(3):
            h = h @ Wt["cameraprediction/%s/fc%d/weights" % (tower, i + 1)] \
                + Wt["cameraprediction/%s/fc%d/biases" % (tower, i + 1)]
            if i < 2:
                h = torch.relu(h)
        outs[tower] = h
    B = emb.shape[0]
    rot = outs["scale"].reshape(B, 1, 1) * ortho6d_to_rotation(outs["ortho6d"])
    t = outs["translation"] + torch.tensor(CO.TRANS_CONST.astype(np.float64), dtype=emb.dtype)
    return torch.cat([rot, t.reshape(B, 1, 3)], dim=1), outs


def pred_trans_mat(pred_RT: torch.Tensor, K=CO.K_DEFAULT) -> torch.Tensor:
    Kt = torch.tensor(np.asarray(K, np.float64), dtype=pred_RT.dtype)
    return pred_RT @ Kt.T


def losses(pred_RT, pts, RT, trans_mat, loss_mode="3D", K=CO.K_DEFAULT, reg=None):
    """pred_RT [B,4,3] tensor; pts/RT/trans_mat numpy -> dict of scalar tensors (+ per-image distances)"""
    dt = pred_RT.dtype
    p = torch.tensor(np.asarray(pts, np.float64), dtype=dt)
    B, N, _ = p.shape
    homo = torch.cat([p, torch.ones(B, N, 1, dtype=dt)], dim=2)
    RTt = torch.tensor(np.asarray(RT, np.float64), dtype=dt)
    Tt = torch.tensor(np.asarray(trans_mat, np.float64), dtype=dt)
    pT = pred_trans_mat(pred_RT, K)
    sub = homo @ pred_RT - homo @ RTt
    pxyz, gxyz = homo @ pT, homo @ Tt
    pxy = pxyz[:, :, :2] / pxyz[:, :, 2:3]
    gxy = gxyz[:, :, :2] / gxyz[:, :, 2:3]
    rotpc = 0.5 * (sub ** 2).sum()
    rot2d = 0.5 * ((pxy - gxy) ** 2).sum() / 1e4
    rotmatrix = ((pT - Tt) ** 2).mean()
    d2_all = torch.sqrt(((gxy.clamp(0, 136) - pxy.clamp(0, 136)) ** 2).sum(-1)).mean(1)
    d3_all = torch.sqrt((sub ** 2).sum(-1)).mean(1)
    w3, w2, wm = mode_weights(loss_mode)
    r = reg if reg is not None else torch.zeros((), dtype=dt)
    overall = w2 * rot2d + w3 * rotpc + wm * rotmatrix + r
    return {"rotpc_loss": rotpc, "rot2d_loss": rot2d, "rotmatrix_loss": rotmatrix, "rot2d_dist": d2_all.mean(),
            "rot3d_dist": d3_all.mean(), "regularization": r, "overall_loss": overall,
            "rot2d_dist_all": d2_all, "rot3d_dist_all": d3_all, "pred_trans_mat": pT}


def rotpc_moment_form(pred_RT: np.ndarray, pts: np.ndarray, RT: np.ndarray):
    """rotpc = 1/2 sum_b tr(D_b^T M_b D_b) and d/d(pred_RT) = M_b D_b, M_b = sum_n homo homo^T"""
    B, N, _ = pts.shape
    homo = np.concatenate([pts, np.ones((B, N, 1))], axis=2).astype(np.float64)
    M = np.einsum("bni,bnj->bij", homo, homo)
    D = np.asarray(pred_RT, np.float64) - np.asarray(RT, np.float64)
    MD = M @ D
    return 0.5 * float(np.einsum("bij,bij->", D, MD)), MD


def head_loss_and_grads(emb: np.ndarray, head_w: Dict[str, np.ndarray], pts, RT, trans_mat, loss_mode="3D"):
    """the head part alone (no VGG, regularization 0): -> (losses floats, grads {name: array, 'embedding',
    'pred_RT'}, pred_trans_mat)"""
    Wt = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in head_w.items()}
    e = torch.tensor(np.asarray(emb, np.float64), requires_grad=True)
    pRT, _ = head(e, Wt)
    pRT.retain_grad()
    L = losses(pRT, pts, RT, trans_mat, loss_mode)
    L["overall_loss"].backward()
    g = {k: v.grad.numpy().copy() for k, v in Wt.items()}
    g["embedding"] = e.grad.numpy().copy()
    g["pred_RT"] = pRT.grad.numpy().copy()
    vals = {k: (v.detach().numpy().copy() if v.ndim else float(v.detach())) for k, v in L.items()}
    return vals, g, L["pred_trans_mat"].detach().numpy()


def vgg_embedding(imgs: np.ndarray, Wt: Dict[str, torch.Tensor]) -> torch.Tensor:
    x = torch.from_numpy(np.asarray(imgs, np.float32)[..., :3]).to(next(iter(Wt.values())).dtype)
    net = T._resize_legacy(x, 224, 224)
    for scope, n, _ in O.VGG_CFG:
        for j in range(1, n + 1):
            nm = "vgg_16/%s/%s_%d" % (scope, scope, j)
            net = T._conv(net, Wt[nm + "/weights"], Wt[nm + "/biases"], 1, True)
        net = Fnn.max_pool2d(net.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    net = T._conv(net, Wt["vgg_16/fc6/weights"], Wt["vgg_16/fc6/biases"], 0, True)
    net = T._conv(net, Wt["vgg_16/fc7/weights"], Wt["vgg_16/fc7/biases"], 0, True)
    return T._conv(net, Wt["vgg_16/fc8/weights"], Wt["vgg_16/fc8/biases"], 0, False).reshape(x.shape[0], -1)


def loss_and_grads(feed: Dict[str, np.ndarray], weights: Dict[str, np.ndarray], loss_mode="3D", wd=WD,
                   dtype=np.float64):
    """the whole camera network: feed {imgs, sample_pc, RT, trans_mat}, weights = 32 VGG + 18 head variables
    -> (losses floats, grads name -> array, pred_trans_mat)"""
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    Wt = {k: torch.tensor(np.asarray(v), dtype=tdt, requires_grad=True) for k, v in weights.items()}
    emb = vgg_embedding(feed["imgs"], Wt)
    pRT, _ = head(emb, Wt)
    reg = wd * sum(0.5 * (Wt[k] ** 2).sum() for k in VGG_NAMES if k.endswith("/weights"))
    L = losses(pRT, feed["sample_pc"], feed["RT"], feed["trans_mat"], loss_mode, reg=reg)
    L["overall_loss"].backward()
    grads = {k: v.grad.numpy().copy() for k, v in Wt.items()}
    vals = {k: (v.detach().numpy().copy() if v.ndim else float(v.detach())) for k, v in L.items()}
    return vals, grads, L["pred_trans_mat"].detach().numpy()


def synth_camera(rng, B):
    """plausible ground-truth cameras: RT = [s R ; t] with a random rotation, trans_mat = RT K^T"""
    RT = np.zeros((B, 4, 3), np.float32)
    for b in range(B):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        q *= np.sign(np.linalg.det(q))
        RT[b, :3] = (0.8 + 0.4 * rng.random()) * q
        RT[b, 3] = CO.TRANS_CONST + 0.05 * rng.standard_normal(3)
    return RT, (RT.astype(np.float64) @ CO.K_DEFAULT.T.astype(np.float64)).astype(np.float32)


def synth_feed(seed: int, B: int, N: int):
    rng = np.random.default_rng(seed)
    RT, tm = synth_camera(rng, B)
    return {"imgs": rng.random((B, 137, 137, 3)).astype(np.float32),
            "sample_pc": (rng.random((B, N, 3)) - 0.5).astype(np.float32) * 0.9,
            "RT": RT, "trans_mat": tm}

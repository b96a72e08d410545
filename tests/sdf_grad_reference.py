"""Reference for the gradient of pred_sdf at the query points: forward-mode differentiation of the
two-stream regression graph in plain numpy, written from the formulas, independent of the library.

One point carries its value and three tangents (d/dx, d/dy, d/dz; t0 = I3) through the layers:

    projection   xyz = [p,1] . T,  u = xyz0 / xyz2,  v = xyz1 / xyz2, both clamped to [0,136]
                 du/dp_k = (T[k,0] - u T[k,2]) / xyz2 (v: T[k,1]); zero for a coordinate whose clamp is active
    resampler    g = bilinear(m; u, v) with the cell x0 = floor(u), y0 = floor(v), taps outside the image zero
                 dg/du = (1-fy)(m[y0,x0+1] - m[y0,x0]) + fy (m[y0+1,x0+1] - m[y0+1,x0]),  dg/dv analogous
    layer        z = a W + b:  a' = relu(z),  t' = (t W) * [z > 0]
    global fold2/conv1   the embedding block is a per-image bias row: nothing for the tangents
    local fold2/conv1    z = a3 W_point + g(u,v) + b,  t' = (t3 W_point + dg/du (x) du/dp + dg/dv (x) dv/dp) * [z > 0],
                         m = the FOLDED map, feature map . W_feat (only the rows the points touch are formed)
    output       grad pred = sum over the streams of t5 . w6

Everything runs in ``dtype`` (float64: the reference; float32: the same run, which measures what fp32 arithmetic
costs -- ``e32`` of tests/test_gpu_sdf_grad.py), the encoder (oracle.disn_oracle.encode) included.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

from oracle import disn_oracle as O

IMG = 137
MARGIN = 3e-5        # three times the project's 1e-5 bar on pre-activation-scale quantities
LINE_PX = 1e-3       # "near a bilinear cell line": within this many pixels of an integer coordinate
G_SCOPE, L_SCOPE = "sdfprediction", "sdfprediction_imgfeat"


def encode(imgs: np.ndarray, weights: Dict[str, np.ndarray], dtype=np.float64):
    """-> (embedding [B,1024] in dtype, featmap [B,137,137,1472] float32: the five up-sampled taps concatenated)"""
    _, emb, maps, _ = O.encode(np.asarray(imgs, np.float32), weights, dtype)
    return np.asarray(emb, dtype).reshape(len(imgs), -1), np.concatenate(maps, axis=3)


def _W(weights, scope, layer, dtype):
    return np.asarray(weights["%s/%s/weights" % (scope, layer)], dtype)[0, 0]


def _B(weights, scope, layer, dtype):
    return np.asarray(weights["%s/%s/biases" % (scope, layer)], dtype)


class _Trace:
    """smallest |pre-activation| and the ReLU sign pattern of every point, over all layers seen"""

    def __init__(self, n):
        self.margin = np.full(n, np.inf)
        self.signs = []

    def see(self, z):
        self.margin = np.minimum(self.margin, np.abs(z).min(axis=1).astype(np.float64))
        self.signs.append(z > 0)


def _layer(a, t, W, b, tr: _Trace, extra_z=None, extra_t=None):
    """a [N,K] value, t [N,3,K] tangents -> relu layer (see the module docstring); extra_*: added before the ReLU"""
    z = a @ W + b
    tz = t @ W
    if extra_z is not None:
        z = z + extra_z
        tz = tz + extra_t
    tr.see(z)
    m = z > 0
    return np.where(m, z, 0), np.where(m[:, None, :], tz, 0)


def _fold1(p, weights, scope, dtype, tr):
    W1 = _W(weights, scope, "fold1/conv1", dtype)
    z = p @ W1 + _B(weights, scope, "fold1/conv1", dtype)
    tr.see(z)
    m = z > 0
    a, t = np.where(m, z, 0), np.where(m[:, None, :], W1[None, :, :], 0)       # t0 = I3: the rows of w1, masked
    for nm in ("fold1/conv2", "fold1/conv3"):
        a, t = _layer(a, t, _W(weights, scope, nm, dtype), _B(weights, scope, nm, dtype), tr)
    return a, t


def _head(a, t, weights, scope, dtype, tr):
    a, t = _layer(a, t, _W(weights, scope, "fold2/conv2", dtype), _B(weights, scope, "fold2/conv2", dtype), tr)
    w6 = _W(weights, scope, "fold2/conv5", dtype)[:, 0]
    return a @ w6 + _B(weights, scope, "fold2/conv5", dtype)[0], t @ w6


def forward_mode(weights: Dict[str, np.ndarray], emb_b: np.ndarray, featmap_b: np.ndarray, pts: np.ndarray,
                 trans_mat_b: np.ndarray, dtype=np.float64, oracle_gather: bool = False):
    """One image: emb_b [1024], featmap_b [137,137,1472], pts [N,3], trans_mat_b [4,3] ->
    {value [N] (un-divided pred_sdf), grad [N,3], margin [N] (smallest |z| over every ReLU pre-activation of both
    streams), signs [N, 2*(64+256+512+512+256)] bool (the ReLU pattern), uv_raw [N,2] (before the clamp), clamped_uv /
    near_line_uv [N,2] bool per coordinate, clamped / near_line [N] bool (either coordinate)}.
    ``oracle_gather``: the VALUE's local term is formed from oracle.get_img_points / oracle.resampler (their float32
    coordinates, weights and features), so that it equals oracle.get_model(dtype) to rounding; the tangents are the
    formulas' either way."""
    p = np.asarray(pts, dtype)
    T = np.asarray(trans_mat_b, dtype)
    N = p.shape[0]
    tr = _Trace(N)
    # ---- global stream
    a, t = _fold1(p, weights, G_SCOPE, dtype, tr)
    W4 = _W(weights, G_SCOPE, "fold2/conv1", dtype)
    row = np.asarray(emb_b, dtype).reshape(-1) @ W4[512:] + _B(weights, G_SCOPE, "fold2/conv1", dtype)
    a, t = _layer(a, t, W4[:512], row, tr)
    vg, gg = _head(a, t, weights, G_SCOPE, dtype, tr)
    # ---- projection and its Jacobian
    xyz = p @ T[:3] + T[3]
    raw = xyz[:, :2] / xyz[:, 2:3]
    uv = np.clip(raw, 0, 136)
    clamped_uv = ~((raw > 0) & (raw < 136))                                    # outside (0,136)
    J = (T[None, :3, :2] - raw[:, None, :] * T[None, :3, 2:3]) / xyz[:, 2, None, None]   # [N,k,(u,v)]
    J = np.where(clamped_uv[:, None, :], 0, J)
    near_line_uv = np.abs(uv - np.round(uv)) < LINE_PX
    # ---- the four folded-map rows of every point, bilinear value and derivatives
    f0 = np.floor(uv)
    fr = uv - f0                                                               # (fx, fy)
    i0 = f0.astype(np.int64)
    Wl4 = _W(weights, L_SCOPE, "fold2/conv1", dtype)
    fm = np.asarray(featmap_b, dtype)

    def rows(ix, iy):
        inb = (ix >= 0) & (iy >= 0) & (ix < IMG) & (iy < IMG)
        r = fm[np.clip(iy, 0, IMG - 1), np.clip(ix, 0, IMG - 1)] @ Wl4[512:]
        return np.where(inb[:, None], r, 0)

    x0, y0 = i0[:, 0], i0[:, 1]
    m00, m01 = rows(x0, y0), rows(x0 + 1, y0)                                  # m[y0,x0], m[y0,x0+1]
    m10, m11 = rows(x0, y0 + 1), rows(x0 + 1, y0 + 1)
    fx, fy = fr[:, 0:1], fr[:, 1:2]
    g = (1 - fx) * (1 - fy) * m00 + fx * (1 - fy) * m01 + (1 - fx) * fy * m10 + fx * fy * m11
    gu = (1 - fy) * (m01 - m00) + fy * (m11 - m10)
    gv = (1 - fx) * (m10 - m00) + fx * (m11 - m01)
    if oracle_gather:
        p32 = np.asarray(pts, np.float32)[None]
        xy = O.get_img_points(p32, np.asarray(trans_mat_b, np.float32)[None])
        g = np.asarray(O.resampler(np.asarray(featmap_b, np.float32)[None], xy)[0], dtype) @ Wl4[512:]
    tg = gu[:, None, :] * J[:, :, 0:1] + gv[:, None, :] * J[:, :, 1:2]         # [N,3,512]
    # ---- local stream
    a, t = _fold1(p, weights, L_SCOPE, dtype, tr)
    a, t = _layer(a, t, Wl4[:512], _B(weights, L_SCOPE, "fold2/conv1", dtype), tr, g, tg)
    vl, gl = _head(a, t, weights, L_SCOPE, dtype, tr)
    return {"value": vg + vl, "grad": gg + gl, "margin": tr.margin, "signs": np.concatenate(tr.signs, axis=1),
            "uv_raw": np.asarray(raw, np.float64), "clamped_uv": clamped_uv, "near_line_uv": near_line_uv,
            "clamped": clamped_uv.any(axis=1), "near_line": near_line_uv.any(axis=1)}


def reference(weights: Dict[str, np.ndarray], imgs: np.ndarray, pts: np.ndarray, trans_mat: np.ndarray,
              dtype=np.float64, enc=None, oracle_gather: bool = False, images: Optional[Sequence[int]] = None):
    """imgs [B,137,137,3], pts [B,N,3], trans_mat [B,4,3] -> the dictionary of ``forward_mode`` with a leading B axis.
    ``enc``: a cached ``encode(imgs, weights, dtype)``; ``images``: which rows of ``enc`` the B point sets belong to."""
    emb, featmap = encode(imgs, weights, dtype) if enc is None else enc
    B = pts.shape[0]
    images = range(B) if images is None else images
    outs = [forward_mode(weights, emb[i], featmap[i], pts[b], trans_mat[b], dtype, oracle_gather)
            for b, i in enumerate(images)]
    return {k: np.stack([o[k] for o in outs]) for k in outs[0]}


def included(ref) -> np.ndarray:
    """the points a gradient comparison may use: away from every ReLU kink, not clamped, not near a cell line
    (ON a line and on a clamp the convention is tested by test_gpu_resample_lattice.py::test_query_grad, whose camera
    makes float32 and float64 agree on the cell)"""
    return (ref["margin"] >= MARGIN) & ~ref["clamped"] & ~ref["near_line"]


def clamped_comparable(ref) -> np.ndarray:
    """clamped points whose gradient is still well defined: a coordinate is either clearly outside [0,136] (by more
    than LINE_PX, so that float32 and float64 agree that it is clamped) or inside and off the cell lines"""
    raw = ref["uv_raw"]
    out = (raw < -LINE_PX) | (raw > 136 + LINE_PX)
    inside = (raw > LINE_PX) & (raw < 136 - LINE_PX) & ~ref["near_line_uv"]
    return (ref["margin"] >= MARGIN) & out.any(axis=-1) & (out | inside).all(axis=-1)

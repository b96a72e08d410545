"""Multi-view reference (not a test module): the pooled gather and the decoder on pooled features, restated in numpy
float32 on top of the single-view oracle (``oracle/disn_oracle.py``).

Per view the oracle's own rows run unchanged -- ``O.get_img_points`` (row D), the five ``resize_bilinear(tap,
(137, 137))`` of ``O.upsampled_taps`` (row E) and ``O.gather_point_feat`` (row F) -- then the views are pooled in view
order, one float32 rounding per operation:

    max :  p = f_0;        p = maximum(p, f_v)
    mean:  p = w_0 * f_0;  p = p + w_v * f_v          (default w_v = float32(1) / float32(V))

A view whose projection is outside the resampler's range (NaN included) contributes the zeros the oracle's resampler
returns for it.  The decoder is ``O.get_sdf_basic2`` on the pooled embedding plus
``O.get_sdf_basic2_imgfeat_twostream`` on the pooled point features.
"""
import numpy as np

from oracle import disn_oracle as O

F32 = np.float32


def default_weights(V):
    return np.full((V,), F32(1.0) / F32(V), np.float32)


def pool_views(x, pool, weights=None, dtype=np.float32):
    """x [V, ...] -> [...] pooled over axis 0 in view order"""
    x = np.asarray(x, dtype)
    V = x.shape[0]
    if pool == "max":
        p = x[0].copy()
        for v in range(1, V):
            p = np.maximum(p, x[v])
        return p
    if pool != "mean":
        raise ValueError(pool)
    w = (default_weights(V) if weights is None else np.asarray(weights, np.float32)).astype(dtype)
    p = (w[0] * x[0]).astype(dtype)
    for v in range(1, V):
        p = (p + (w[v] * x[v]).astype(dtype)).astype(dtype)
    return p


def view_maps(taps):
    """taps: five arrays [V,hw,hw,ch] -> V lists of the five up-sampled maps [1,137,137,ch] (row E; the
    multi-threaded resize is bit-identical to ``O.resize_bilinear_legacy``, tests/test_oracle.py)"""
    V = taps[0].shape[0]
    return [[O.resize_bilinear_legacy_mt(np.asarray(t[v:v + 1], np.float32), O.IMG_H, O.IMG_W) for t in taps]
            for v in range(V)]


def gather_views(maps, trans_mat, pts):
    """maps: ``view_maps``; trans_mat [V,4,3]; pts [N,3] -> the oracle's 'point_img_feat' of every view [V,N,1472]"""
    pts = np.asarray(pts, np.float32)[None]
    tm = np.asarray(trans_mat, np.float32).reshape(-1, 4, 3)
    out = []
    for v, m in enumerate(maps):
        xy = O.get_img_points(pts, tm[v:v + 1])
        out.append(O.gather_point_feat(m, xy)[0, :, 0, :])
    return np.stack(out)


def gather_pool(maps, trans_mat, pts, pool, weights=None):
    """-> the pooled rows [N,1472]"""
    return pool_views(gather_views(maps, trans_mat, pts), pool, weights)


def pred_views(maps, embeddings, trans_mat, pts, W, pool, weights=None, dtype=np.float32):
    """pred_sdf [N] (un-divided) of the two decoder streams on the pooled features.  ``embeddings`` [V,1024] and the
    MLPs in ``dtype``; the gather and its pooling are float32 rows D..F either way (as ``O.get_model(dtype=...)``)."""
    feat = gather_pool(maps, trans_mat, pts, pool, weights)
    emb = pool_views(np.asarray(embeddings, dtype), pool, weights, dtype)
    pc = np.asarray(pts, np.float32)[None]
    g = O.get_sdf_basic2(pc, emb.reshape(1, -1), W, dtype=dtype)
    l = O.get_sdf_basic2_imgfeat_twostream(pc, feat[None, :, None, :], W, dtype=dtype)
    return (g + l)[0, :, 0]


# ---- the inputs of the kernel test (tests/test_gpu_multiview.py; their properties: tests/test_multiview_host.py) ------
def kernel_cameras(nan_view=None):
    """three synthetic cameras [3,4,3]; ``nan_view``: that view's translation row zeroed, so the origin projects to
    0 / 0 = NaN there (and only the origin: every other point keeps a finite or infinite quotient)"""
    cams = np.stack([O.synth_trans_mat(30.0, 25.0, 0.8), O.synth_trans_mat(201.5, 30.0, 0.65),
                     O.synth_trans_mat(110.0, 10.0, 0.9)]).astype(np.float32)
    if nan_view is not None:
        cams[nan_view, 3, :] = 0.0
    return cams


def integer_pixel_point(T, px, py, span=8):
    """a float32 point whose float32 projection by T [4,3] is EXACTLY the pixel (px, py): the float64 pre-image at
    the origin's depth, then the first neighbour within +-span ulps per coordinate that lands on it (None if none)"""
    M = np.asarray(T, np.float64).T
    p0 = np.linalg.solve(M[:, :3], M[2, 3] * np.array([px, py, 1.0]) - M[:, 3]).astype(np.float32)
    k = np.arange(-span, span + 1, dtype=np.float32)
    off = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3)
    cand = (p0[None] + off * np.spacing(np.abs(p0))[None]).astype(np.float32)
    xy = O.get_img_points(cand[None], np.asarray(T, np.float32)[None])[0]
    hit = np.nonzero((xy[:, 0] == px) & (xy[:, 1] == py))[0]
    return cand[hit[0]] if len(hit) else None


def kernel_points(n=70, seed=5):
    """-> (pts [n,3], {"origin": [i], "integer": [i ...], "clamp": [i ...]}): the origin (NaN under
    ``kernel_cameras(nan_view)``), one point per camera that lands exactly on an interior pixel of it, four points
    that sit on the 0 / 136 clamp in view 0 only, and uniform points of [-0.6, 0.6]^3"""
    cams = kernel_cameras()
    rng = np.random.default_rng(seed)
    special = [np.zeros(3, np.float32)]
    for v, (px, py) in enumerate(((40, 90), (71, 23), (100, 64))):
        special.append(integer_pixel_point(cams[v], px, py))
    wide = (rng.random((4096, 3), dtype=np.float32) * F32(2.4) - F32(1.2)).astype(np.float32)
    xy = np.stack([O.get_img_points(wide[None], cams[v:v + 1])[0] for v in range(3)])
    on = ((xy[0] == 0) | (xy[0] == 136)).any(axis=1)
    inside = ((xy[1:] > 0) & (xy[1:] < 136)).all(axis=(0, 2))
    special.extend(wide[np.nonzero(on & inside)[0][:4]])
    rest = (rng.random((n - len(special), 3), dtype=np.float32) * F32(1.2) - F32(0.6)).astype(np.float32)
    pts = np.concatenate([np.stack(special), rest]).astype(np.float32)
    return pts, {"origin": [0], "integer": [1, 2, 3], "clamp": [4, 5, 6, 7]}

"""Views of a mesh on the device, and the camera matrices stored with them: what the reference takes from a
download of Blender renders plus ``preprocessing/create_img_h5.py``.  Kernel: ``csrc/render.hip`` (a ray caster
over the BVH of ``mesh_sdf.MeshBvh``); the rule and its limits are in DESIGN §4u.

    params = render.random_view_params(np.random.default_rng(0), 24)     # rendering_metadata.txt rows
    out = render.render_views(verts, faces, params)                       # {"rgba": [24,137,137,4] uint8 on the device}
    K, RT, trans_mat, regress_mat, obj_rot_mat = render.view_matrices(params[0], norm_params)

The camera functions are restatements of ``create_img_h5.py`` with its float32 casts written out: a parameter
row is cast to float32 first, the trigonometry of ``get_az/el/inl`` and of ``getBlenderProj`` runs on float32
scalars, and so do ``az + 180`` and ``distance_ratio * 1.75`` (numpy >= 2 evaluates the reference's mixed
float32 / Python-float expressions in float32; older numpy took those two in float64, a difference of one
float32 rounding).  The matrix products are float64.

``sdf_ray_cameras`` / ``trace_field`` / ``silhouette_iou`` render the PREDICTED surface instead, straight from an
implicit field by sphere tracing (kernels ``csrc/sdf_trace.hip``; ``SdfEngine.trace`` feeds it the network).

The image is not Blender's: one headlight term on a flat albedo, no shadows, no textures, no gamma.  The camera
(and so where the object lies in the image) is the reference's.
"""
from __future__ import annotations

import os
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

f32 = np.float32

rot90y = np.array([[0, 0, -1], [0, 1, 0], [1, 0, 0]], dtype=np.float32)

CAM_MAX_DIST = 1.75
_CAM_ROT = np.asarray([[1.910685676922942e-15, 4.371138828673793e-08, 1.0],
                       [1.0, -4.371138828673793e-08, -0.0],
                       [4.371138828673793e-08, 1.0, -4.371138828673793e-08]])


# ---- create_img_h5.py restated -----------------------------------------------------------------------------------
def blender_proj(az, el, distance_ratio, img_w: int = 137, img_h: int = 137) -> Tuple[np.ndarray, np.ndarray]:
    """getBlenderProj -> (K [3,3], RT [3,4]) float64, from float32 viewpoint parameters"""
    az, el, distance_ratio = f32(az), f32(el), f32(distance_ratio)
    f_u = 35.0 * img_w * 1.0 / 32.0
    f_v = 35.0 * img_h * 1.0 * 1.0 / 32.0
    K = np.array(((f_u, 0.0, img_w * 1.0 / 2), (0.0, f_v, img_h * 1.0 / 2), (0.0, 0.0, 1.0)))
    sa, ca = np.sin(np.radians(-az)), np.cos(np.radians(-az))          # float32
    se, ce = np.sin(np.radians(-el)), np.cos(np.radians(-el))
    R_world2obj = np.array(((ca * ce, -sa, ca * se), (sa * ce, ca, sa * se), (-se, f32(0), ce)), np.float64).T
    R_obj2cam = _CAM_ROT.T
    cam_location = np.array(((float(distance_ratio * f32(CAM_MAX_DIST)),), (0.0,), (0.0,)))
    R_camfix = np.diag([1.0, -1.0, -1.0])
    R_world2cam = R_camfix @ (R_obj2cam @ R_world2obj)
    T_world2cam = R_camfix @ ((-1.0 * R_obj2cam) @ cam_location)
    return K, np.hstack((R_world2cam, T_world2cam))


def get_rotate_matrix(rotation_angle1: float) -> np.ndarray:
    """[4,4] float64: neg . Rz . Rz . scale_y_neg . Rx of the angle (the reference calls it with -pi/2)"""
    c, s = np.cos(rotation_angle1), np.sin(rotation_angle1)
    rx = np.array([[1, 0, 0, 0], [0, c, -s, 0], [0, s, c, 0], [0, 0, 0, 1]])
    rz = np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    scale_y_neg = np.diag([1.0, -1.0, 1.0, 1.0])
    neg = np.diag([-1.0, -1.0, -1.0, 1.0])
    return np.linalg.multi_dot([neg, rz, rz, scale_y_neg, rx])


def get_norm_matrix(norm_params) -> np.ndarray:
    """[4,4] float64 = T_inv . M_inv of norm_params = (centroid, m): normalised -> raw coordinates.  (The
    reference's argument is the sample file; this takes its ``norm_params``.)"""
    p = np.asarray(norm_params, np.float32).astype(np.float64)
    m_inv = np.diag([p[3], p[3], p[3], 1.0])
    t_inv = np.eye(4)
    t_inv[:3, 3] = p[:3]
    return np.matmul(t_inv, m_inv)


def degree2rad(params) -> np.ndarray:
    params = np.asarray(params, np.float32)
    out = np.zeros_like(params)
    out[0] = np.deg2rad(params[0] + f32(180.0))
    out[1] = np.deg2rad(params[1])
    out[2] = np.deg2rad(params[2])
    return out


def _f32mat(vals) -> np.ndarray:
    return np.asarray(vals, dtype=np.float32).reshape(3, 3)


def get_az(az) -> np.ndarray:
    c, s = np.cos(f32(az)), np.sin(f32(az))
    return _f32mat([c, 0.0, s, 0.0, 1.0, 0.0, f32(-1.0) * s, 0.0, c])


def get_el(el) -> np.ndarray:
    c, s = np.cos(f32(el)), np.sin(f32(el))
    return _f32mat([1.0, 0.0, 0.0, 0.0, c, f32(-1.0) * s, 0.0, s, c])


def get_inl(inl) -> np.ndarray:
    c, s = np.cos(f32(inl)), np.sin(f32(inl))
    return _f32mat([c, f32(-1.0) * s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0])


def camera_info(param) -> Tuple[np.ndarray, np.ndarray]:
    """(cam_mat float32 [3,3], cam_pos) of a parameter row in radians"""
    cam_mat = np.transpose(np.matmul(np.matmul(get_inl(param[2]), get_el(param[1])), get_az(param[0])))
    return cam_mat, -1 * np.array([0, 0, param[3]])


def get_img_cam(param) -> Tuple[np.ndarray, np.ndarray]:
    return camera_info(degree2rad(param))


def view_matrices(param_row, norm_params, img_w: int = 137, img_h: int = 137):
    """-> (K [3,3], RT [3,4], trans_mat [4,3], regress_mat [4,3], obj_rot_mat [3,3]) of one
    rendering_metadata.txt row (az, el, tilt, distance_ratio, ...) and an object's norm_params: what
    gen_obj_img_h5 stores (K, RT and the products in float64; obj_rot_mat float32 = rot90y . camR).  The
    reference's images are 137 x 137; another size only changes K."""
    param = np.asarray(param_row, np.float64).astype(np.float32)
    cam_r, _ = get_img_cam(param)
    obj_rot_mat = np.dot(rot90y, cam_r)
    K, RT = blender_proj(param[0], param[1], param[3], img_w=img_w, img_h=img_h)
    rot_mat = get_rotate_matrix(-np.pi / 2)
    norm_mat = get_norm_matrix(norm_params)
    trans_mat = np.transpose(np.linalg.multi_dot([K, RT, rot_mat, norm_mat]))
    regress_mat = np.transpose(np.linalg.multi_dot([RT, rot_mat, norm_mat]))
    return K, RT, trans_mat, regress_mat, obj_rot_mat


# ---- rendering ---------------------------------------------------------------------------------------------------
def ray_cameras(params, W: int = 137, H: int = 137) -> np.ndarray:
    """-> [V,12] float32 (org, d0, dx, dy per view, csrc/render.hip) of parameter rows [V, >=4].  Computed in
    float64 from E = RT . rot_mat = [A | t], which takes RAW model.obj coordinates to the camera (trans_mat is
    K . E . norm_mat on normalised ones): org = -A^-1 t, dir(x, y) = A^-1 K^-1 (x, y, 1), K for a W x H image."""
    params = np.atleast_2d(np.asarray(params, np.float64)).astype(np.float32)
    rot_mat = get_rotate_matrix(-np.pi / 2)
    out = np.empty((params.shape[0], 12), np.float64)
    for v, p in enumerate(params):
        K, RT = blender_proj(p[0], p[1], p[3], img_w=W, img_h=H)
        E = RT @ rot_mat
        a_inv = np.linalg.inv(E[:, :3])
        m = a_inv @ np.linalg.inv(K)
        out[v, 0:3] = -a_inv @ E[:, 3]
        out[v, 3:6] = m[:, 2]
        out[v, 6:9] = m[:, 0]
        out[v, 9:12] = m[:, 1]
    return out.astype(np.float32)


def random_view_params(rng: np.random.Generator, n: int = 24, el: Sequence[float] = (25.0, 30.0),
                       dist: Sequence[float] = (0.65, 0.95), tilt: float = 0.0) -> np.ndarray:
    """-> float64 [n,5] rows (az, el, tilt, distance_ratio, 25) as in rendering_metadata.txt: az U[0,360),
    el U[el], distance_ratio U[dist].  UNPINNED: the default ranges are recalled from the public renders'
    metadata and have not been compared with it."""
    out = np.empty((n, 5), np.float64)
    out[:, 0] = rng.uniform(0.0, 360.0, n)
    out[:, 1] = rng.uniform(el[0], el[1], n)
    out[:, 2] = tilt
    out[:, 3] = rng.uniform(dist[0], dist[1], n)
    out[:, 4] = 25.0
    return out


def render_views(mesh, faces=None, params=None, size: Tuple[int, int] = (137, 137), samples: int = 4,
                 albedo=None, ambient: float = 0.3, brute: bool = False, want: Sequence[str] = ("rgba",),
                 cams=None) -> Dict[str, "torch.Tensor"]:
    """V views of one mesh in one launch -> device tensors {"rgba": uint8 [V,H,W,4] (straight alpha), "depth":
    float32 [V,H,W] (camera-space depth, 0 = no hit), "face": int32 [V,H,W] (file-order face, -1 = no hit)},
    those named in ``want``.  ``mesh``: vertices (with ``faces``) or a ``mesh_sdf.MeshBvh``; ``params``:
    rendering_metadata.txt rows [V, >=4]; size = (W, H); samples = S of the S x S grid per pixel (1..4);
    ``albedo`` [nf,3] in file order (None: 0.8 grey); ``brute`` tests every triangle (the same bits).
    ``cams`` [V,12] replaces ``ray_cameras(params, W, H)``."""
    import torch

    from . import mesh_sdf, ops
    from ._lib import check, lib
    unknown = set(want) - {"rgba", "depth", "face"}
    if unknown or "rgba" not in want:
        raise ValueError("want must name 'rgba' and may name 'depth' and 'face', got %r" % (tuple(want),))
    W, H = int(size[0]), int(size[1])
    m = mesh_sdf._bvh(mesh, faces)
    cam = np.ascontiguousarray(ray_cameras(params, W, H) if cams is None else cams, np.float32).reshape(-1, 12)
    V = cam.shape[0]
    with torch.cuda.device(m.device):
        cam_d = torch.from_numpy(cam).to(m.device)
        alb = None
        if albedo is not None:
            alb = albedo if isinstance(albedo, torch.Tensor) else torch.from_numpy(
                np.ascontiguousarray(albedo, np.float32))
            alb = ops._chk(alb.to(m.device).reshape(-1, 3), "albedo")
            if alb.shape[0] != m.nf:
                raise ValueError("albedo must have one row per triangle (%d), got %d" % (m.nf, alb.shape[0]))
        out = {"rgba": torch.empty((V, H, W, 4), dtype=torch.uint8, device=m.device)}
        if "depth" in want:
            out["depth"] = torch.empty((V, H, W), dtype=torch.float32, device=m.device)
        if "face" in want:
            out["face"] = torch.empty((V, H, W), dtype=torch.int32, device=m.device)
        check("disn_render_views", lib().disn_render_views(
            m.image.data_ptr(), m.nf, m.order.data_ptr(), alb.data_ptr() if alb is not None else None,
            cam_d.data_ptr(), V, H, W, int(samples), float(ambient), int(brute), out["rgba"].data_ptr(),
            out["depth"].data_ptr() if "depth" in out else None, out["face"].data_ptr() if "face" in out else None,
            ops._stream()))
    return out


# ---- the predicted surface, directly (csrc/sdf_trace.hip) --------------------------------------------
def sdf_ray_cameras(trans_mat, W: int = 137, H: int = 137) -> np.ndarray:
    """-> [V,12] float32 (org, d0, dx, dy per view, the layout of ``ray_cameras``) of trans_mat [V,4,3], in the
    NORMALISED object frame the query points live in: [p, 1] . T = (u w, v w, w) with (u, v) the pixel of a 137 x
    137 image, so with M = T[:3], tt = T[3], Mi = M^-1: org = -tt Mi, d0 = Mi[2], dx = Mi[0] 137/W, dy = Mi[1]
    137/H, and the ray of image point (x, y) of a W x H image is org + t ((d0 + x dx) + y dy) with t the
    camera-space depth w.  Float64, cast at the end.  The direction is not of unit length."""
    T = np.asarray(trans_mat, np.float64).reshape(-1, 4, 3)
    out = np.empty((T.shape[0], 12), np.float64)
    for v, t in enumerate(T):
        mi = np.linalg.inv(t[:3, :])
        out[v, 0:3] = -t[3, :] @ mi
        out[v, 3:6] = mi[2, :]
        out[v, 6:9] = mi[0, :] * 137.0 / W
        out[v, 9:12] = mi[1, :] * 137.0 / H
    return out.astype(np.float32)


TRACE_OUTPUTS = ("rgba", "depth", "normal", "residual", "status")


def trace_field(field, cams, size: Tuple[int, int], sdf_params, iso: float = 0.0, grad=None,
                sdf_weight: float = 1.0, want: Sequence[str] = ("rgba",), ambient: float = 0.3, t_min: float = 0.0,
                eps: float = 1e-4, step_scale: float = 0.8, min_step: float = 1e-3, max_step: float = 0.1,
                max_steps: int = 96, refine: int = 8, device=None) -> Dict[str, object]:
    """Sphere-trace V views of the level set ``field / sdf_weight == iso`` inside the box ``sdf_params`` -> device
    tensors, those named in ``want``: "rgba" uint8 [V,H,W,4] (headlight on 0.8 grey, alpha 255 at a hit), "depth"
    float32 [V,H,W] (camera-space depth t of ``cams``, 0 = no hit), "normal" float32 [V,H,W,3] (grad / |grad|),
    "residual" float32 [V,H,W] (|field / sdf_weight - iso| at the hit), "status" uint8 [V,H,W] (0 miss, 1 hit within
    eps, 2 hit at the ray's first sample, 3 hit after ``refine`` bracket steps, 4 miss after ``max_steps`` march
    steps) -- and "stats" = {"rays", "box_rays", "evaluations", "iterations", "hits"}.

    ``field(pts [n,3]) -> [n]`` and ``grad(pts [n,3]) -> [n,3]`` (or ``(field values [n], [n,3])``) are callables on
    float32 device tensors, negative inside; without ``grad`` the normals are 0 and the image is lit by the ambient
    term alone.  cams [V,12] (``sdf_ray_cameras``), size = (W, H).  The rules and their limits: DESIGN §4x.  The host
    loop reads one 4-byte count back per iteration (it sizes the next evaluation); ``field`` is never called with
    n = 0."""
    import torch

    from . import ops
    unknown = set(want) - set(TRACE_OUTPUTS)
    if unknown:
        raise ValueError("want may name %s, got %r" % (", ".join(TRACE_OUTPUTS), tuple(want)))
    W, H = int(size[0]), int(size[1])
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if isinstance(cams, torch.Tensor):
        cam_d = cams.to(dev, torch.float32).reshape(-1, 12).contiguous()
    else:
        cam_d = torch.from_numpy(np.ascontiguousarray(cams, np.float32).reshape(-1, 12)).to(dev)
    n = cam_d.shape[0] * H * W
    march = dict(iso=iso, sdf_weight=sdf_weight, eps=eps, step_scale=step_scale, min_step=min_step, max_step=max_step,
                 max_steps=max_steps, refine=refine)
    with torch.cuda.device(dev):
        state = ops.trace_state(n, dev)
        counts = ops.trace_state_view(state, n)["counts"]
        pts = torch.empty((n, 3), dtype=torch.float32, device=dev)
        ops.trace_setup(cam_d, (W, H), sdf_params, state, pts, t_min)
        cur, active = 0, int(counts[0].item())
        stats = {"rays": n, "box_rays": active, "evaluations": 0, "iterations": 0, "hits": 0}
        while active:
            if stats["iterations"] > max_steps + refine + 1:     # a ray takes at most max_steps + refine evaluations
                raise RuntimeError("the trace did not end after %d iterations" % stats["iterations"])
            vals = field(pts[:active]).reshape(-1)
            ops.trace_advance(cam_d, (W, H), state, vals, active, cur, pts, **march)
            stats["evaluations"] += active
            stats["iterations"] += 1
            cur = 1 - cur
            active = int(counts[cur].item())
        ops.trace_collect(cam_d, (W, H), state, pts)
        hits = stats["hits"] = int(counts[2].item())
        pred = g = None
        if hits:
            hp = pts[:hits]
            r = grad(hp) if grad is not None else torch.zeros_like(hp)
            pred, g = r if isinstance(r, (tuple, list)) else (field(hp), r)
            pred, g = pred.reshape(-1), g.reshape(-1, 3)
        out = ops.trace_shade(cam_d, (W, H), state, pred, g, hits, iso, sdf_weight, ambient, tuple(want))
    out["stats"] = stats
    return out


def silhouette_iou(mask, alpha) -> float:
    """intersection / union of two [H,W] silhouettes: ``mask`` (non-zero = predicted, e.g. a traced view's alpha or
    depth) and ``alpha`` (> 0 = the image's object pixels); 1.0 when both are empty"""
    def host(a):
        return np.asarray(a.detach().cpu() if hasattr(a, "detach") else a)
    m, a = host(mask) != 0, host(alpha) > 0
    if m.ndim != 2 or m.shape != a.shape:
        raise ValueError("silhouette_iou takes two [H,W] masks of one size, got %s and %s" % (m.shape, a.shape))
    union = int(np.logical_or(m, a).sum())
    return 1.0 if union == 0 else float(np.logical_and(m, a).sum()) / union


# ---- optional colour ---------------------------------------------------------------------------------------------
def _read_mtl(path: str) -> Dict[str, np.ndarray]:
    kd: Dict[str, np.ndarray] = {}
    name = None
    with open(path, errors="replace") as f:
        for line in f:
            t = line.split()
            if len(t) >= 2 and t[0] == "newmtl":
                name = t[1]
            elif len(t) >= 4 and t[0] == "Kd" and name is not None:
                kd[name] = np.asarray([float(t[1]), float(t[2]), float(t[3])], np.float32)
    return kd


def read_obj_albedo(path: str, nf: Optional[int] = None, grey: float = 0.8) -> np.ndarray:
    """-> float32 [nf,3]: the ``Kd`` of the material (``usemtl`` / ``mtllib``) in force at each "f" record, one
    row per triangle of the fan triangulation (0, t, t+1) in file order, i.e. the rows of
    ``mesh_sdf.read_obj_mesh(path)[1]``; ``grey`` where no material or no ``.mtl`` applies.  ``nf``: the expected
    triangle count (asserted)."""
    mats: Dict[str, np.ndarray] = {}
    rows = []
    cur = np.full(3, grey, np.float32)
    with open(path, errors="replace") as f:
        for line in f:
            t = line.split()
            if not t:
                continue
            if t[0] == "mtllib" and len(t) >= 2:
                mtl = os.path.join(os.path.dirname(os.path.abspath(path)), line.split(None, 1)[1].strip())
                if os.path.exists(mtl):
                    mats.update(_read_mtl(mtl))
            elif t[0] == "usemtl":
                cur = mats.get(t[1] if len(t) >= 2 else "", np.full(3, grey, np.float32))
            elif t[0] == "f" and len(t) >= 4:
                rows += [cur] * (len(t) - 3)
    out = np.asarray(rows, np.float32).reshape(-1, 3)
    assert nf is None or out.shape[0] == int(nf), "%s: %d triangles from the materials, %s from the mesh" % (
        path, out.shape[0], nf)
    return out

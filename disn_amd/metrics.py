"""Point-cloud evaluation metrics on the device: the two custom ops of the reference's ``models/tf_ops``
(``nn_distance``, ``approx_match`` + ``match_cost``) and the arithmetic of ``test/test_cd_emd.py`` /
``test/test_f_score.py`` around them.  Kernels: ``csrc/metrics.hip``; C ABI: ``disn_nn_distance``,
``disn_approx_match``, ``disn_match_cost``, ``disn_emd``.

Inputs are float32 device tensors ``[b, n, 3]`` in the TF ops' argument order; CPU tensors raise ``TypeError``.
Every result is deterministic and a pair's result never depends on the other pairs of its call.

    from disn_amd import metrics
    d1, i1, d2, i2 = metrics.nn_distance(pred, gt)                         # tf_nndistance.nn_distance
    cost = metrics.match_cost(gt, pred, metrics.approx_match(gt, pred))   # tf_approxmatch
    cost = metrics.emd(gt, pred)                                          # the same, no [b, m, n] match buffer
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from ._lib import check, lib

# test/test_f_score.py:291 ([[0.5], [1], [2], [5], [10], [20]] * 0.01 * truethreshold)
F_SCORE_PERCENTS = (0.5, 1.0, 2.0, 5.0, 10.0, 20.0)


def f_score_thresholds(truethreshold: float = 2.5, percents: Sequence[float] = F_SCORE_PERCENTS) -> np.ndarray:
    """the F-score distance thresholds of test/test_f_score.py:167, float32 as there"""
    return (np.asarray(percents, dtype=np.float32) * 0.01 * truethreshold).astype(np.float32)


def _pair(xyz1: torch.Tensor, xyz2: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, int, int, int]:
    xyz1 = ops._chk(xyz1, "xyz1")
    xyz2 = ops._chk(xyz2, "xyz2")
    if xyz1.dim() != 3 or xyz2.dim() != 3 or xyz1.shape[2] != 3 or xyz2.shape[2] != 3:
        raise ValueError("xyz1 and xyz2 must be [b, n, 3] and [b, m, 3], got %s and %s"
                         % (tuple(xyz1.shape), tuple(xyz2.shape)))
    if xyz1.shape[0] != xyz2.shape[0]:
        raise ValueError("batch sizes differ: %d vs %d" % (xyz1.shape[0], xyz2.shape[0]))
    if xyz1.device != xyz2.device:
        raise ValueError("xyz1 and xyz2 are on different devices")
    b, n, m = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    if b < 1 or n < 1 or m < 1:
        raise ValueError("empty point cloud: b=%d n=%d m=%d" % (b, n, m))
    return xyz1, xyz2, b, n, m


def _ws(b: int, n: int, m: int, device) -> torch.Tensor:
    return ops._ws(lib().disn_metrics_workspace_bytes(b, n, m), device)


def nn_distance(xyz1: torch.Tensor, xyz2: torch.Tensor):
    """-> dist1 [b,n] f32, idx1 [b,n] i32, dist2 [b,m] f32, idx2 [b,m] i32 (tf_nndistance.nn_distance):
    squared distance to the nearest point of the other cloud and its lowest index."""
    xyz1, xyz2, b, n, m = _pair(xyz1, xyz2)
    dev = xyz1.device
    with torch.cuda.device(dev):
        d1 = torch.empty((b, n), dtype=torch.float32, device=dev)
        i1 = torch.empty((b, n), dtype=torch.int32, device=dev)
        d2 = torch.empty((b, m), dtype=torch.float32, device=dev)
        i2 = torch.empty((b, m), dtype=torch.int32, device=dev)
        ws = _ws(b, n, m, dev)
        check("disn_nn_distance", lib().disn_nn_distance(xyz1.data_ptr(), xyz2.data_ptr(), b, n, m, d1.data_ptr(),
                                                         i1.data_ptr(), d2.data_ptr(), i2.data_ptr(), ws.data_ptr(),
                                                         ws.numel(), ops._stream()))
    return d1, i1, d2, i2


def approx_match(xyz1: torch.Tensor, xyz2: torch.Tensor) -> torch.Tensor:
    """-> match [b, m, n] (tf_approxmatch.approx_match).  b*m*n floats: 403 MB at 24 x 2048 x 2048; ``emd``
    gives the cost without it."""
    xyz1, xyz2, b, n, m = _pair(xyz1, xyz2)
    dev = xyz1.device
    with torch.cuda.device(dev):
        match = torch.empty((b, m, n), dtype=torch.float32, device=dev)
        ws = _ws(b, n, m, dev)
        check("disn_approx_match", lib().disn_approx_match(xyz1.data_ptr(), xyz2.data_ptr(), b, n, m,
                                                           match.data_ptr(), ws.data_ptr(), ws.numel(),
                                                           ops._stream()))
    return match


def match_cost(xyz1: torch.Tensor, xyz2: torch.Tensor, match: torch.Tensor) -> torch.Tensor:
    """-> cost [b] = sum_{k,l} |xyz2[l] - xyz1[k]| * match[l, k] (tf_approxmatch.match_cost)"""
    xyz1, xyz2, b, n, m = _pair(xyz1, xyz2)
    match = ops._chk(match, "match")
    if tuple(match.shape) != (b, m, n):
        raise ValueError("match must be [b, m, n] = %s, got %s" % ((b, m, n), tuple(match.shape)))
    dev = xyz1.device
    with torch.cuda.device(dev):
        cost = torch.empty((b,), dtype=torch.float32, device=dev)
        ws = _ws(b, n, m, dev)
        check("disn_match_cost", lib().disn_match_cost(xyz1.data_ptr(), xyz2.data_ptr(), match.data_ptr(), b, n, m,
                                                       cost.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream()))
    return cost


def emd(xyz1: torch.Tensor, xyz2: torch.Tensor) -> torch.Tensor:
    """-> cost [b]: match_cost(xyz1, xyz2, approx_match(xyz1, xyz2)) in one fused schedule (no match buffer)"""
    xyz1, xyz2, b, n, m = _pair(xyz1, xyz2)
    dev = xyz1.device
    with torch.cuda.device(dev):
        cost = torch.empty((b,), dtype=torch.float32, device=dev)
        ws = _ws(b, n, m, dev)
        check("disn_emd", lib().disn_emd(xyz1.data_ptr(), xyz2.data_ptr(), b, n, m, cost.data_ptr(), ws.data_ptr(),
                                         ws.numel(), ops._stream()))
    return cost


# ---- the evaluation scripts' arithmetic ---------------------------------------------------------------------------
def _views(pred: torch.Tensor, gt: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """pred [v, N, 3]; gt [N, 3] (tiled to every view, test_cd_emd.py:285) or [v, N, 3]"""
    pred = ops._chk(pred, "pred")
    gt = ops._chk(gt, "gt")
    if pred.dim() == 2:
        pred = pred.unsqueeze(0)
    if gt.dim() == 2:
        gt = gt.unsqueeze(0).expand(pred.shape[0], -1, -1).contiguous()
    return pred, gt


def chamfer_views(pred: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """-> [v] float64: (mean(dist_fwd) + mean(dist_bwd)) * 1000 per view, dist_fwd = nn_distance(pred, gt)
    (test/test_cd_emd.py:292-293)"""
    pred, gt = _views(pred, gt)
    d1, _, d2, _ = nn_distance(pred, gt)
    return (d1.double().mean(1) + d2.double().mean(1)) * 1000.0


def emd_views(pred: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """-> [v] float64: match_cost(gt, pred, approx_match(gt, pred)) * 0.01 per view (test/test_cd_emd.py:300-301)"""
    pred, gt = _views(pred, gt)
    return emd(gt, pred).double() * 0.01


def precision_recall(pred: torch.Tensor, gt: torch.Tensor, thresholds) -> Tuple[np.ndarray, np.ndarray]:
    """-> (precision [T], recall [T]) float64 of one object, pooled over its views (test/test_f_score.py:232-237):
    the fraction of sqrt(dist_fwd) < t (precision) and of sqrt(dist_bwd) < t (recall), strict, float32."""
    pred, gt = _views(pred, gt)
    d1, _, d2, _ = nn_distance(pred, gt)
    t = torch.as_tensor(np.asarray(thresholds, np.float32).reshape(-1, 1), device=pred.device)
    s1, s2 = torch.sqrt(d1.reshape(1, -1)), torch.sqrt(d2.reshape(1, -1))
    pre = (s1 < t).sum(1).cpu().numpy().astype(np.float64) / s1.shape[1]
    rec = (s2 < t).sum(1).cpu().numpy().astype(np.float64) / s2.shape[1]
    return pre, rec


def sample_vertices(verts, n: int, rng: np.random.Generator, device=None) -> torch.Tensor:
    """-> [n, 3] float32 device tensor: n vertices drawn uniformly WITH replacement (test_cd_emd.py:245, :252).
    The indices come from ``rng`` on the host (the same seed gives the same points on any machine), the gather
    runs where ``verts`` lies; a mesh without vertices gives zeros, as in the reference."""
    if isinstance(verts, torch.Tensor):
        dev = verts.device if verts.is_cuda else (device or torch.device("cuda"))
        v = verts.to(dev, torch.float32).reshape(-1, 3)
    else:
        dev = device or torch.device("cuda")
        v = torch.from_numpy(np.ascontiguousarray(verts, np.float32).reshape(-1, 3)).to(dev)
    if v.shape[0] == 0:
        return torch.zeros((n, 3), dtype=torch.float32, device=dev)
    idx = torch.from_numpy(rng.integers(v.shape[0], size=n).astype(np.int64)).to(dev)
    return v.index_select(0, idx).contiguous()


def view_stats(values) -> Tuple[float, float, int]:
    """(mean, min, argmin) over the views of one object, as the scripts print them"""
    v = np.asarray(values.cpu().numpy() if isinstance(values, torch.Tensor) else values, np.float64)
    return float(v.mean()), float(v.min()), int(v.argmin())


def f_score(precision, recall) -> np.ndarray:
    """F = 2PR / (P + R) (test/test_f_score.py:180)"""
    p, r = np.asarray(precision, np.float64), np.asarray(recall, np.float64)
    return 2 * (p * r) / (p + r)


def weighted_category_average(values, counts) -> np.ndarray:
    """average of per-category values weighted by their object counts (test/test_f_score.py:178-179)"""
    return np.average(np.asarray(values, np.float64), axis=0, weights=np.asarray(counts, np.float64))


def load_points(path: str, device=None) -> Optional[torch.Tensor]:
    """a comma-separated point file written by the reference's sample_save_*_pnt (np.savetxt, delimiter ',')"""
    a = np.loadtxt(path, dtype=float, delimiter=",").astype(np.float32).reshape(-1, 3)
    return torch.from_numpy(a).to(device or torch.device("cuda"))


# ---- area-weighted surface samples (csrc/mesh_sample.hip, include/disn_amd_sample.h) -----------------------------
# Not in the reference, whose scripts sample VERTICES (sample_vertices above, which cd_emd and f_score keep using):
# vertex samples follow the tessellation, these follow the surface.  sample_surface_arrays IS the rule; the device
# form reproduces its integers (the face of every sample) and its float32 points and normals.
STATUS_INDEX, STATUS_FINITE, STATUS_NO_AREA = 2, 4, 6          # a mesh's status word (postprocess.STATUS_*; 6 is this stage's)
SAMPLE_MAX_N = 1 << 20
_GOLDEN = 0x9E3779B97F4A7C15
_M64 = (1 << 64) - 1
_M32 = np.uint64(0xFFFFFFFF)


def mix64(x: int) -> int:
    """the SplitMix64 finaliser of csrc/mesh_batch.hpp, on Python integers modulo 2^64"""
    x &= _M64
    x = ((x ^ (x >> 30)) * 0xbf58476d1ce4e5b9) & _M64
    x = ((x ^ (x >> 27)) * 0x94d049bb133111eb) & _M64
    return x ^ (x >> 31)


def mesh_seed(seed: int, name: str) -> int:
    """mix64(seed ^ crc32(name)): the seed of one mesh's samples, a function of the run's seed and the mesh's name
    alone -- so its samples do not depend on how the driver groups or orders the meshes"""
    import zlib
    return mix64((int(seed) & _M64) ^ zlib.crc32(name.encode("utf-8")))


def _mix64_np(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint64)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return x ^ (x >> np.uint64(31))


def _sample_words(seed: int, n: int) -> Tuple[np.ndarray, np.ndarray]:
    """r(i, 0), r(i, 1) for i < n: mix64(seed + GOLDEN (2 i + k + 1)) modulo 2^64"""
    with np.errstate(over="ignore"):
        r = _mix64_np(np.uint64(int(seed) & _M64) + np.uint64(_GOLDEN) * np.arange(1, 2 * n + 1, dtype=np.uint64))
    return r[0::2], r[1::2]


def _isqrt64(x: np.ndarray) -> np.ndarray:
    """the exact integer square root of uint64 x <= 2^62: a float64 estimate corrected by +-1 with integer multiplies"""
    one = np.uint64(1)
    r = np.floor(np.sqrt(x.astype(np.float64))).astype(np.uint64)
    for _ in range(2):
        r = np.where(r * r > x, r - one, r)
        r = np.where((r + one) * (r + one) <= x, r + one, r)
    return r


def _mulhi64(a: np.ndarray, b: int) -> np.ndarray:
    """(a b) >> 64 of uint64 a and 0 <= b < 2^64, from 32-bit halves: no partial sum leaves uint64"""
    s32 = np.uint64(32)
    a_lo, a_hi, b_lo, b_hi = a & _M32, a >> s32, np.uint64(b & 0xFFFFFFFF), np.uint64(b >> 32)
    p0, p1, p2, p3 = a_lo * b_lo, a_lo * b_hi, a_hi * b_lo, a_hi * b_hi
    carry = ((p0 >> s32) + (p1 & _M32) + (p2 & _M32)) >> s32
    return p3 + (p1 >> s32) + (p2 >> s32) + carry


def _face_normals64(v: np.ndarray, f: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """N = e1 x e2 [nf,3] and s = (N.x^2 + N.y^2) + N.z^2 [nf] in float64, in exactly this association"""
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    e1, e2 = b - a, c - a
    nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return np.stack([nx, ny, nz], 1), (nx * nx + ny * ny) + nz * nz


def surface_face_weights(verts, faces) -> np.ndarray:
    """-> uint64 [nf]: q = isqrt(floor((s / smax) 2^62)) in [0, 2^31], the integer a face is drawn in proportion to
    (its area relative to the largest, to 31 bits); all zeros for a mesh without area.  Indices must be valid."""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    if len(f) == 0:
        return np.zeros(0, np.uint64)
    _, s = _face_normals64(v, f)
    smax = s.max()
    if not smax > 0:
        return np.zeros(len(f), np.uint64)
    return _isqrt64(np.floor((s / smax) * 2.0 ** 62).astype(np.uint64))


def sample_surface_arrays(verts, faces, n: int, seed: int):
    """THE RULE of the surface sampler (include/disn_amd_sample.h restates it): n area-weighted samples of
    one mesh -> (points f32 [n,3], normals f32 [n,3], face_idx i32 [n], status).

    The face of a sample is chosen by integers and float64 + - x / alone: the weights of ``surface_face_weights``,
    their inclusive sum ``cum`` in uint64, ``target = (r(i,0) total) >> 64`` and the first face with ``cum > target``.
    The point is ``((1 - t) A + (t (1 - u2)) B) + (t u2) C`` in float32 with ``t = sqrt(u1)`` and u1, u2 the two
    24-bit fields of r(i,1); the normal is ``N / sqrt(s)`` in float64, rounded, the orientation of corners a, b, c.
    Sample i depends on (seed, i) and the mesh, never on n.  status: 0; 2 a face index outside [0, nv); 4 a coordinate
    that is not finite (the larger of the two when both hold); 6 no faces or no face with an area -- any non-zero
    status gives zeros in all three outputs."""
    n = int(n)
    if not 1 <= n <= SAMPLE_MAX_N:
        raise ValueError("n must be in 1..%d, got %r" % (SAMPLE_MAX_N, n))
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    zeros = (np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.int32))
    status = max(STATUS_INDEX if len(f) and (f.min() < 0 or f.max() >= len(v)) else 0,
                 0 if np.isfinite(v).all() else STATUS_FINITE)
    if status:
        return zeros + (status,)
    q = surface_face_weights(v, f)
    if len(f) == 0 or not q.any():
        return zeros + (STATUS_NO_AREA,)
    cum = np.cumsum(q, dtype=np.uint64)
    r0, r1 = _sample_words(seed, n)
    face = np.searchsorted(cum, _mulhi64(r0, int(cum[-1])), side="right").astype(np.int32)
    scale = np.float32(2.0 ** -24)
    u1 = (r1 >> np.uint64(40)).astype(np.float32) * scale
    u2 = ((r1 >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.float32) * scale
    t = np.sqrt(u1)
    wa, wb, wc = np.float32(1) - t, t * (np.float32(1) - u2), t * u2
    A, B, Cc = (v[f[face, k]] for k in range(3))
    points = (wa[:, None] * A + wb[:, None] * B) + wc[:, None] * Cc
    N, s = _face_normals64(v, f[face])
    normals = (N / np.sqrt(s)[:, None]).astype(np.float32)
    return points.astype(np.float32), normals, face, 0


_HELD = []          # (event, host arrays of a call the stream may not have passed yet)


def _hold(*arrays) -> None:
    """keeps the host arrays of an asynchronous call alive until its stream has passed it -- without waiting for it"""
    ev = torch.cuda.Event()
    ev.record()
    _HELD[:] = [h for h in _HELD if not h[0].query()]
    _HELD.append((ev, arrays))


def sample_surface_meshes_device(meshes, n: int, seeds):
    """``sample_surface_arrays`` for a group of meshes that lie on the device, in ONE call without a read-back.
    ``meshes``: B x (verts [nv,3] float32, faces [nf,3] int32, ...) device tensors, as ``marching_cubes_batch``,
    ``clean_group`` and ``simplify_group`` pass them around; ``seeds``: B integers (``mesh_seed``).
    -> (points [B,n,3] f32, normals [B,n,3] f32, face_idx [B,n] i32, status [B] i32), device tensors: the integers of
    the rule, its points and normals.  A mesh with a status (2, 4, 6) has zeros."""
    from .postprocess import _pack_meshes
    meshes = [tuple(m) for m in meshes]
    B, n = len(meshes), int(n)
    if B < 1:
        raise ValueError("no mesh to sample")
    if not 1 <= n <= SAMPLE_MAX_N:
        raise ValueError("n must be in 1..%d, got %r" % (SAMPLE_MAX_N, n))
    seeds = np.ascontiguousarray([int(s) & _M64 for s in seeds], np.uint64)
    if seeds.shape != (B,):
        raise ValueError("%d meshes, %d seeds" % (B, seeds.size))
    v, v_off, f, f_off, ws = _pack_meshes(meshes, lambda nv, nf: lib().disn_mesh_sample_workspace_bytes(B, nv, nf, n))
    dev = v.device
    with torch.cuda.device(dev):
        points = torch.empty((B, n, 3), dtype=torch.float32, device=dev)
        normals = torch.empty((B, n, 3), dtype=torch.float32, device=dev)
        face_idx = torch.empty((B, n), dtype=torch.int32, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        check("disn_mesh_sample_batch", lib().disn_mesh_sample_batch(
            v.data_ptr(), f.data_ptr(), v_off.ctypes.data, f_off.ctypes.data, B, seeds.ctypes.data, n,
            points.data_ptr(), normals.data_ptr(), face_idx.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(),
            ops._stream()))
        _hold(v_off, f_off, seeds)
    return points, normals, face_idx, status


def sample_surface_arrays_device(verts, faces, v_off, f_off, n: int, seeds):
    """the same for meshes already back to back: verts [sum nv,3] f32, faces [sum nf,3] i32 (indices local to their
    mesh), v_off / f_off [B+1] ascending from 0"""
    v_off, f_off = np.asarray(v_off, np.int64), np.asarray(f_off, np.int64)
    return sample_surface_meshes_device(
        [(verts[int(v_off[b]):int(v_off[b + 1])], faces[int(f_off[b]):int(f_off[b + 1])])
         for b in range(len(v_off) - 1)], n, seeds)


SURFACE_SCORES = ("accuracy", "completeness", "chamfer_l1", "chamfer_l2", "normal_consistency")


def surface_scores_from_nn(d_fwd, i_fwd, d_bwd, i_bwd, pred_nrm, gt_nrm, thresholds) -> Dict[str, np.ndarray]:
    """the arithmetic of ``surface_scores`` behind ``nn_distance`` (torch reductions where the tensors lie): squared
    distances [v,N] / [v,M] float32, indices of the nearest point of the other cloud, unit normals [v,N,3] / [v,M,3]"""
    s_fwd, s_bwd = torch.sqrt(d_fwd), torch.sqrt(d_bwd)                 # float32, as precision_recall
    acc, comp = s_fwd.double().mean(1), s_bwd.double().mean(1)

    def consistency(a, b, idx):
        near = torch.gather(b, 1, idx.long().unsqueeze(-1).expand(-1, -1, 3))
        return (a.double() * near.double()).sum(-1).abs().mean(1)

    t = torch.as_tensor(np.asarray(thresholds, np.float32).reshape(1, -1, 1), device=d_fwd.device)
    pre = (s_fwd.unsqueeze(1) < t).sum(2).double() / s_fwd.shape[1]
    rec = (s_bwd.unsqueeze(1) < t).sum(2).double() / s_bwd.shape[1]
    both = pre + rec
    out = {"accuracy": acc, "completeness": comp, "chamfer_l1": 0.5 * (acc + comp),
           "chamfer_l2": d_fwd.double().mean(1) + d_bwd.double().mean(1),
           "normal_consistency": 0.5 * (consistency(pred_nrm, gt_nrm, i_fwd) + consistency(gt_nrm, pred_nrm, i_bwd)),
           "precision": pre, "recall": rec,
           "f_score": torch.where(both > 0, 2 * pre * rec / torch.where(both > 0, both, torch.ones_like(both)),
                                  torch.zeros_like(both))}
    return {k: x.cpu().numpy() for k, x in out.items()}


def surface_scores(pred_pts, pred_nrm, gt_pts, gt_nrm, thresholds) -> Dict[str, np.ndarray]:
    """scores of surface samples with normals, per view, float64: pred [v,N,3]; gt [M,3] (tiled to every view) or
    [v,M,3].  With d_fwd, idx_fwd, d_bwd, idx_bwd = nn_distance(pred, gt):
      accuracy = mean sqrt(d_fwd), completeness = mean sqrt(d_bwd), chamfer_l1 their mean,
      chamfer_l2 = mean d_fwd + mean d_bwd (``chamfer_views`` without its factor 1000),
      normal_consistency = (mean |n_p . n_g[idx_fwd]| + mean |n_g . n_p[idx_bwd]|) / 2,
      precision / recall [v,T]: the fraction of sqrt(d_fwd) / sqrt(d_bwd) < t, strict as ``precision_recall``,
      f_score = 2PR / (P + R), 0 where both are 0."""
    pred_pts, gt_pts = _views(pred_pts, gt_pts)
    pred_nrm, gt_nrm = _views(pred_nrm, gt_nrm)
    if pred_nrm.shape != pred_pts.shape or gt_nrm.shape != gt_pts.shape:
        raise ValueError("points and normals differ in shape: %s / %s and %s / %s" % (
            tuple(pred_pts.shape), tuple(pred_nrm.shape), tuple(gt_pts.shape), tuple(gt_nrm.shape)))
    d1, i1, d2, i2 = nn_distance(pred_pts, gt_pts)
    return surface_scores_from_nn(d1, i1, d2, i2, pred_nrm, gt_nrm, thresholds)

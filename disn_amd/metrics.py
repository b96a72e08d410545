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

from typing import Optional, Sequence, Tuple

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

"""Scoring of reconstructed meshes: the reference's ``test/test_cd_emd.py`` (Chamfer distance and approximate
EMD, ``cd_emd_all`` / ``cd_emd_cat``) and ``test/test_f_score.py`` (``cal_f_score_all_cat`` / ``f_score_cat``),
on ``disn_amd.metrics`` instead of the TF1 + CUDA custom ops, and ``test/test_iou.py`` (voxel IoU, ``iou_all`` /
``iou_cat``) on ``disn_amd.voxel`` instead of PyMesh.

    python -m disn_amd.evaluate cd_emd  --cal_dir OBJS --gt_dir GT --test_lst_dir LSTS [--category all]
    python -m disn_amd.evaluate f_score --cal_dir OBJS --gt_dir GT --test_lst_dir LSTS [--truethreshold 2.5]
    python -m disn_amd.evaluate iou     --cal_dir OBJS --gt_dir GT --test_lst_dir LSTS [--dim 110] [--mode reference]
    python -m disn_amd.evaluate surface --pred_dir OBJS --gt_dir GT --test_lst_dir LSTS [--num_sample_points 2048]
    python -m disn_amd.evaluate sdf_acc --log_dir CKPT --test_lst_dir LSTS --sdf_dir SDF --rendered_dir VIEWS

Layout, as the reference reads it:
  predictions  <cal_dir>/<cat_id>/<cat_id>_<obj_id>_<view>.obj    (what ``isosurface.create_obj`` writes)
  ground truth <gt_dir>/<cat_id>/<obj_id>/isosurf.obj
  object lists <test_lst_dir>/<cat_id>_test.lst
  F-score point files (optional; sample_save_*_pnt of test_cd_emd.py):
               <gt_dir>/<cat_id>/<obj_id>/pnt_<N>.txt and <cal_dir>/pnt_<N>_<cat_id>/pnt_<obj_id>_<view>.txt
Only the reference's ``batch_size == view_num`` path is mirrored: its other branch (test_cd_emd.py:259-280)
stacks the ground truth with ``verts_batch[b]`` for b = 0, i.e. compares the ground truth with itself.
Point sampling draws from ``numpy.random.Generator(seed)``, the view choice from ``random.Random(seed)``.

IoU (``iou``), differences from test_iou.py: the views of an object are chosen with ``random.Random(seed)`` from
its sorted file list (the reference samples the unsorted ``os.listdir`` order with the global generator); an object
with fewer than ``view_num`` predictions is an error, not a resample with replacement; a listed object without
predictions is an error, not a skipped line; a mesh that cannot be scored (it leaves the voxel key range, or the
union is empty) raises, where the reference's bare ``try`` prints "error mesh" and then fails on the ``None``.
Kept: the ``os.stat(...)[6] > 200`` size filter on prediction files, the float32 array of per-view values with its
sum / mean / argmax, the category average over views, and the printed lines.  ``--mode solid`` (not in the
reference, whose grids are surface shells) fills the voxel sets first.

Surface scores (``surface``; NOT in the reference, whose numbers stay ``cd_emd`` and ``f_score`` on vertex samples):
accuracy, completeness, Chamfer-L1 and -L2, normal consistency and precision / recall / F-score on area-weighted
surface samples drawn on the device (``metrics.sample_surface_meshes_device``); layout and view choice as ``cd_emd``.

SDF accuracy (``sdf_acc``, the reference's ``test/test_sdf_acc.py``): the five scalars of ``get_loss`` on sampled
query points of the test views -- all 24 views of every listed object, ``sdf = sdf_val - 0.003``, one
``engine.encode_query`` + ``ops.get_loss`` per batch, the reference's per-batch lines and its ``Summary:`` (the mean
of the per-batch values).  Differences: batches are consecutive runs of ``--batch_size`` list entries in list
order, the last, shorter one included (the reference shuffles and drops the tail); the points of a batch are
drawn from ``numpy.random.default_rng(seed + batch index)``; a missing checkpoint is an error unless
``--random_init SEED`` is given; ``--view_num`` below 24 scores a seeded choice of views (the sample list of
``disn_amd.create_sdf``).
"""
from __future__ import annotations

import argparse
import glob
import os
import random
import sys
from typing import Dict, List, Optional

import numpy as np

CATS_ALL = {
    "watercraft": "04530566", "rifle": "04090263", "display": "03211117", "lamp": "03636649",
    "speaker": "03691459", "chair": "03001627", "bench": "02828884", "cabinet": "02933112",
    "car": "02958343", "airplane": "02691156", "sofa": "04256520", "table": "04379243", "phone": "04401088",
}
CATS_CLEAN = {"cabinet": "02933112", "display": "03211117", "speaker": "03691459", "rifle": "04090263",
              "watercraft": "04530566"}


def categories(category: str) -> Dict[str, str]:
    """--category: "all", "clean", one category name (test_cd_emd.py / test_f_score.py __main__), or several
    names separated by commas"""
    if "," in category:
        out: Dict[str, str] = {}
        for name in category.split(","):
            out.update(categories(name.strip()))
        return out
    if category == "all":
        return dict(CATS_ALL)
    if category == "clean":
        return dict(CATS_CLEAN)
    if category not in CATS_ALL:
        raise ValueError("unknown category %r (all, clean or one of %s)" % (category, ", ".join(sorted(CATS_ALL))))
    return {category: CATS_ALL[category]}


def build_file_dict(dir: str, min_size: Optional[int] = None) -> Dict[str, List[str]]:
    """object id -> prediction files of a category directory: field 1 of the file name split on '_'
    (test_cd_emd.py:126-136); lists sorted, so that a seed picks the same views on any file system.
    ``min_size``: only files of more than that many bytes (test_iou.py:124 keeps those above 200)"""
    d: Dict[str, List[str]] = {}
    for fn in sorted(os.listdir(dir)):
        full = os.path.join(dir, fn)
        if os.path.isfile(full) and (min_size is None or os.stat(full).st_size > min_size):
            d.setdefault(fn.split("_")[1], []).append(full)
    return d


def read_list(test_lst_f: str) -> List[str]:
    with open(test_lst_f) as f:
        objs = [l.rstrip("\r\n") for l in f]
    objs = [o for o in objs if o]
    if not objs:
        raise ValueError("%s lists no object" % test_lst_f)
    return objs


def _predictions(pred_dict, obj_id: str, cat_id: str, pred_dir: str) -> List[str]:
    if obj_id not in pred_dict:
        raise FileNotFoundError("no prediction for object %s of category %s in %s" % (obj_id, cat_id, pred_dir))
    return pred_dict[obj_id]


def _mesh_points(path: str, n: int, rng: np.random.Generator):
    from . import isosurface, metrics
    return metrics.sample_vertices(isosurface.read_obj_verts(path), n, rng)


def cd_emd_cat(cat_id: str, cat_nm: str, pred_dir: str, gt_dir: str, test_lst_f: str, view_num: int = 24,
               num_sample_points: int = 2048, rng: Optional[np.random.Generator] = None,
               pyrng: Optional[random.Random] = None, out=None) -> dict:
    """Chamfer (x1000) and EMD (x0.01) of every listed object over ``view_num`` sampled views
    (test_cd_emd.py:220-282) -> {"objects": {obj_id: {...}}, "avg_cf", "avg_emd"}"""
    import torch

    from . import metrics
    rng = rng if rng is not None else np.random.default_rng(0)
    pyrng = pyrng if pyrng is not None else random.Random(0)
    out = out or sys.stdout
    pred_dict = build_file_dict(pred_dir)
    objs = read_list(test_lst_f)
    for obj_id in objs:
        _predictions(pred_dict, obj_id, cat_id, pred_dir)
    res: Dict[str, dict] = {}
    sum_cf = sum_em = 0.0
    for count, obj_id in enumerate(objs, 1):
        src_path = os.path.join(gt_dir, obj_id, "isosurf.obj")
        preds = _predictions(pred_dict, obj_id, cat_id, pred_dir)
        if len(preds) < view_num:
            raise ValueError("object %s of category %s has %d predictions, --view_num is %d"
                             % (obj_id, cat_id, len(preds), view_num))
        gt = _mesh_points(src_path, num_sample_points, rng)
        views = pyrng.sample(preds, view_num)
        pred = torch.stack([_mesh_points(p, num_sample_points, rng) for p in views])
        cf = metrics.chamfer_views(pred, gt)
        em = metrics.emd_views(pred, gt)
        avg_cf, min_cf, arg_cf = metrics.view_stats(cf)
        avg_em, min_em, arg_em = metrics.view_stats(em)
        sum_cf += avg_cf
        sum_em += avg_em
        res[obj_id] = {"avg_cf": avg_cf, "min_cf": min_cf, "arg_cf": arg_cf, "avg_emd": avg_em,
                       "min_emd": min_em, "arg_emd": arg_em, "views": views,
                       "cf_views": cf.cpu().numpy(), "emd_views": em.cpu().numpy()}
        print("%d  %s avg cf:%s, min_cf:%s, arg_cf view:%d, avg emd:%s, min_emd:%s, arg_em view:%d"
              % (count, src_path, avg_cf, min_cf, arg_cf, avg_em, min_em, arg_em), file=out)
    summary = {"cat_nm": cat_nm, "cat_id": cat_id, "objects": res, "avg_cf": sum_cf / len(objs),
               "avg_emd": sum_em / len(objs)}
    print("cat_nm:%s, cat_id:%s, avg_cf:%s, avg_emd:%s" % (cat_nm, cat_id, summary["avg_cf"], summary["avg_emd"]),
          file=out)
    return summary


def cd_emd_all(cats: Dict[str, str], pred_dir: str, gt_dir: str, test_lst_dir: str, seed: int = 0,
               out=None, **kw) -> Dict[str, dict]:
    out = out or sys.stdout
    rng, pyrng = np.random.default_rng(seed), random.Random(seed)
    res = {}
    for cat_nm, cat_id in cats.items():
        res[cat_id] = cd_emd_cat(cat_id, cat_nm, os.path.join(pred_dir, cat_id), os.path.join(gt_dir, cat_id),
                                 os.path.join(test_lst_dir, cat_id + "_test.lst"), rng=rng, pyrng=pyrng, out=out,
                                 **kw)
    print("done!", file=out)
    return res


def f_score_cat(cat_id: str, cat_nm: str, pred_dir: str, gt_dir: str, test_lst_f: str, thresholds,
                num_sample_points: int = 2048, rng: Optional[np.random.Generator] = None, out=None) -> dict:
    """precision / recall of every listed object, pooled over all its predicted views (test_f_score.py:183-243)
    -> {"objects": {obj_id: {"precision", "recall", "points"}}, "precision", "recall", "count"}.  The reference's
    point files are scored when all of an object's exist; otherwise its points are sampled from the meshes."""
    import torch

    from . import metrics
    rng = rng if rng is not None else np.random.default_rng(0)
    out = out or sys.stdout
    pred_dict = build_file_dict(pred_dir)
    objs = read_list(test_lst_f)
    for obj_id in objs:
        _predictions(pred_dict, obj_id, cat_id, pred_dir)
    pnt_dir = os.path.join(os.path.dirname(pred_dir), "pnt_%d_%s" % (num_sample_points, cat_id))
    res: Dict[str, dict] = {}
    pre_sum = rec_sum = 0.0
    for obj_id in objs:
        preds = _predictions(pred_dict, obj_id, cat_id, pred_dir)
        gt_pnt = os.path.join(gt_dir, obj_id, "pnt_%d.txt" % num_sample_points)
        pred_pnts = [os.path.join(pnt_dir, "pnt_%s_%s.txt" % (obj_id, p[-6:-4])) for p in preds]
        if os.path.exists(gt_pnt) and all(os.path.exists(p) for p in pred_pnts):
            source = "files"
            gt = metrics.load_points(gt_pnt)
            pred = torch.stack([metrics.load_points(p) for p in pred_pnts])
        else:
            source = "meshes"
            gt = _mesh_points(os.path.join(gt_dir, obj_id, "isosurf.obj"), num_sample_points, rng)
            pred = torch.stack([_mesh_points(p, num_sample_points, rng) for p in preds])
        pre, rec = metrics.precision_recall(pred, gt, thresholds)
        pre_sum = pre_sum + pre
        rec_sum = rec_sum + rec
        res[obj_id] = {"precision": pre, "recall": rec, "points": source}
        print("cat_id %s, obj_id %s: precision %s, recall %s" % (cat_id, obj_id, pre, rec), file=out)
    summary = {"cat_nm": cat_nm, "cat_id": cat_id, "objects": res, "precision": pre_sum / len(objs),
               "recall": rec_sum / len(objs), "count": len(objs)}
    print("%s, %s, precision_avg %s, recal_avg%s, count %d"
          % (cat_nm, cat_id, summary["precision"], summary["recall"], len(objs)), file=out)
    return summary


def cal_f_score_all_cat(cats: Dict[str, str], pred_dir: str, gt_dir: str, test_lst_dir: str,
                        truethreshold: float = 2.5, num_sample_points: int = 2048, seed: int = 0,
                        out=None) -> dict:
    """category averages weighted by object count, then F = 2PR/(P+R) (test_f_score.py:159-181)"""
    from . import metrics
    out = out or sys.stdout
    thresholds = metrics.f_score_thresholds(truethreshold)
    rng = np.random.default_rng(seed)
    per = {}
    for cat_nm, cat_id in cats.items():
        per[cat_id] = f_score_cat(cat_id, cat_nm, os.path.join(pred_dir, cat_id), os.path.join(gt_dir, cat_id),
                                  os.path.join(test_lst_dir, cat_id + "_test.lst"), thresholds,
                                  num_sample_points=num_sample_points, rng=rng, out=out)
    print("done!", file=out)
    counts = [c["count"] for c in per.values()]
    pre = metrics.weighted_category_average([c["precision"] for c in per.values()], counts)
    rec = metrics.weighted_category_average([c["recall"] for c in per.values()], counts)
    f = metrics.f_score(pre, rec)
    print("pre_w_avg %s, rec_w_avg %s, f_score %s" % (pre, rec, f), file=out)
    return {"categories": per, "thresholds": thresholds, "precision": pre, "recall": rec, "f_score": f}


def _device_mesh(path: str, device=None):
    """a whole .obj (disn_read_obj_mesh) as (verts f32 [nv,3], faces i32 [nf,3]) device tensors"""
    import torch

    from . import mesh_sdf
    v, f = mesh_sdf.read_obj_mesh(path)
    dev = device or torch.device("cuda")
    return torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)


def _sampled(meshes, names, n: int, seed: int, log=None):
    """area-weighted samples of a group of device meshes in ONE call -> (points [B,n,3], normals [B,n,3], status [B]
    on the host); mesh b is seeded by ``mesh_seed(seed, names[b])``.  ValueError for a bad index or a coordinate that
    is not finite; a mesh without area (status 6) gives zeros, as ``sample_vertices`` does for a mesh without
    vertices, and ``log`` (default: a line on stderr) is told its name, so that its numbers are not taken for real ones."""
    from . import metrics
    pts, nrm, _, status = metrics.sample_surface_meshes_device(meshes, n, [metrics.mesh_seed(seed, nm) for nm in names])
    status = np.asarray(status.cpu())
    log = log or (lambda line: print(line, file=sys.stderr))
    for b, st in enumerate(status):
        if st == metrics.STATUS_NO_AREA:
            log("WARNING: %s has no area to sample (status 6): it is scored as %d points at the origin" % (names[b], n))
        elif st != 0:
            raise ValueError("%s: %s" % (names[b], "face index out of range" if st == metrics.STATUS_INDEX
                                         else "a vertex coordinate is not finite"))
    return pts, nrm, status


def surface_cat(cat_id: str, cat_nm: str, pred_dir: str, gt_dir: str, test_lst_f: str, thresholds,
                view_num: int = 24, num_sample_points: int = 2048, seed: int = 0,
                pyrng: Optional[random.Random] = None, out=None) -> dict:
    """scores on area-weighted SURFACE samples (``metrics.surface_scores``) of every listed object over ``view_num``
    sampled views; layout, view choice and logging as ``cd_emd_cat``.  The ground truth is sampled once per object,
    the predictions of its views in one batched call; a mesh's samples depend on ``seed`` and its file name alone.
    A mesh without area is scored as points at the origin, named in a WARNING line and listed under "no_area".
    -> {"objects": {obj_id: {name: mean over the views, "views", "per_view", "no_area"}}, name: category mean,
    "count", "no_area"}"""
    from . import metrics
    pyrng = pyrng if pyrng is not None else random.Random(0)
    out = out or sys.stdout
    pred_dict = build_file_dict(pred_dir)
    objs = read_list(test_lst_f)
    for obj_id in objs:
        _predictions(pred_dict, obj_id, cat_id, pred_dir)
    names = metrics.SURFACE_SCORES + ("precision", "recall", "f_score")
    warn = lambda line: print(line, file=out)
    res: Dict[str, dict] = {}
    no_area: List[str] = []
    sums = {k: 0.0 for k in names}
    for count, obj_id in enumerate(objs, 1):
        src_path = os.path.join(gt_dir, obj_id, "isosurf.obj")
        preds = _predictions(pred_dict, obj_id, cat_id, pred_dir)
        if len(preds) < view_num:
            raise ValueError("object %s of category %s has %d predictions, --view_num is %d"
                             % (obj_id, cat_id, len(preds), view_num))
        gt_pts, gt_nrm, gt_st = _sampled([_device_mesh(src_path)], ["%s/%s/isosurf.obj" % (cat_id, obj_id)],
                                         num_sample_points, seed, warn)
        views = pyrng.sample(preds, view_num)
        pts, nrm, st = _sampled([_device_mesh(p) for p in views], [os.path.basename(p) for p in views],
                                num_sample_points, seed, warn)
        flat = ([src_path] if gt_st[0] else []) + [p for p, s in zip(views, st) if s]
        no_area += flat
        per_view = metrics.surface_scores(pts, nrm, gt_pts[0], gt_nrm[0], thresholds)
        mean = {k: np.asarray(per_view[k], np.float64).mean(0) for k in names}
        for k in names:
            sums[k] = sums[k] + mean[k]
        res[obj_id] = dict(mean, views=views, per_view=per_view, no_area=flat)
        print("%d  %s %s, f_score:%s" % (count, src_path, ", ".join("%s:%s" % (k, mean[k]) for k in metrics.SURFACE_SCORES),
                                         mean["f_score"]), file=out)
    summary = {"cat_nm": cat_nm, "cat_id": cat_id, "objects": res, "count": len(objs), "no_area": no_area}
    summary.update({k: sums[k] / len(objs) for k in names})
    if no_area:
        print("WARNING: cat_id:%s, %d mesh(es) without area entered the averages as points at the origin"
              % (cat_id, len(no_area)), file=out)
    print("cat_nm:%s, cat_id:%s, %s, f_score:%s" % (cat_nm, cat_id, ", ".join(
        "%s:%s" % (k, summary[k]) for k in metrics.SURFACE_SCORES), summary["f_score"]), file=out)
    return summary


def surface_all(cats: Dict[str, str], pred_dir: str, gt_dir: str, test_lst_dir: str, truethreshold: float = 2.5,
                view_num: int = 24, num_sample_points: int = 2048, seed: int = 0, out=None) -> dict:
    """``surface_cat`` of every category, then the averages weighted by object count.  NOT in the reference: its
    numbers are ``cd_emd`` and ``f_score``, on vertex samples."""
    from . import metrics
    out = out or sys.stdout
    thresholds = metrics.f_score_thresholds(truethreshold)
    pyrng = random.Random(seed)
    per = {}
    for cat_nm, cat_id in cats.items():
        per[cat_id] = surface_cat(cat_id, cat_nm, os.path.join(pred_dir, cat_id), os.path.join(gt_dir, cat_id),
                                  os.path.join(test_lst_dir, cat_id + "_test.lst"), thresholds, view_num=view_num,
                                  num_sample_points=num_sample_points, seed=seed, pyrng=pyrng, out=out)
    print("done!", file=out)
    counts = [c["count"] for c in per.values()]
    res = {"categories": per, "thresholds": thresholds}
    for k in metrics.SURFACE_SCORES + ("precision", "recall", "f_score"):
        res[k] = metrics.weighted_category_average([c[k] for c in per.values()], counts)
    print("weighted averages: %s, precision %s, recall %s, f_score %s" % (
        ", ".join("%s %s" % (k, res[k]) for k in metrics.SURFACE_SCORES), res["precision"], res["recall"], res["f_score"]),
        file=out)
    return res


def iou_cat(cat_id: str, cat_nm: str, pred_dir: str, gt_dir: str, test_lst_f: str, view_num: int = 24,
            dim: int = 110, mode: str = "reference", pyrng: Optional[random.Random] = None, out=None) -> dict:
    """voxel IoU of every listed object over ``view_num`` sampled views (test_iou.py:174-206)
    -> {"objects": {obj_id: {...}}, "iou_avg", "count"}; iou_avg = sum of all view values / number of views"""
    from . import mesh_sdf, voxel
    pyrng = pyrng if pyrng is not None else random.Random(0)
    out = out or sys.stdout
    pred_dict = build_file_dict(pred_dir, min_size=200)
    objs = read_list(test_lst_f)
    for obj_id in objs:
        _predictions(pred_dict, obj_id, cat_id, pred_dir)
    res: Dict[str, dict] = {}
    iou_sum, count = 0.0, 0.0
    for obj_id in objs:
        src_path = os.path.join(gt_dir, obj_id, "isosurf.obj")
        preds = _predictions(pred_dict, obj_id, cat_id, pred_dir)
        if len(preds) < view_num:
            raise ValueError("object %s of category %s has %d predictions, --view_num is %d"
                             % (obj_id, cat_id, len(preds), view_num))
        views = pyrng.sample(preds, view_num)
        meshes = [mesh_sdf.read_obj_mesh(p) for p in [src_path] + views]
        iou, inter, union = voxel.iou_views(meshes[0], meshes[1:], dim=dim, mode=mode, names=[src_path] + views)
        iou_vals = np.asarray(iou, dtype=np.float32)
        iou_sum += float(np.sum(iou_vals))
        count += len(iou_vals)
        avg_iou = np.mean(iou_vals)
        ind = int(np.argmax(iou_vals))
        best = [float(iou[ind]), views[ind]]
        res[obj_id] = {"avg_iou": float(avg_iou), "best": best, "views": views, "iou_views": iou,
                       "inter": inter, "union": union}
        print("obj_id iou avg: ", avg_iou, " best pred: ", best, file=out)
    return {"cat_nm": cat_nm, "cat_id": cat_id, "objects": res, "iou_avg": float(iou_sum / count), "count": int(count)}


def iou_all(cats: Dict[str, str], pred_dir: str, gt_dir: str, test_lst_dir: str, dim: int = 110,
            mode: str = "reference", view_num: int = 24, seed: int = 0, out=None) -> Dict[str, dict]:
    """test_iou.py:165-172"""
    out = out or sys.stdout
    pyrng = random.Random(seed)
    res = {}
    for cat_nm, cat_id in cats.items():
        res[cat_id] = iou_cat(cat_id, cat_nm, os.path.join(pred_dir, cat_id), os.path.join(gt_dir, cat_id),
                              os.path.join(test_lst_dir, cat_id + "_test.lst"), view_num=view_num, dim=dim, mode=mode,
                              pyrng=pyrng, out=out)
        print("cat_nm: {}, cat_id: {}, iou_avg: {}".format(cat_nm, cat_id, res[cat_id]["iou_avg"]), file=out)
    print("done!", file=out)
    return res


SDF_ACC_NAMES = ("accuracy", "sdf_loss_realvalue", "sdf_loss", "regularization", "overall_loss")
SDF_WEIGHT = 10.0            # test/test_sdf_acc.py:61


MESH_CHECK_SHARES = ("closed", "manifold", "oriented", "no_self_intersection", "watertight")


def mesh_check_summary(rows) -> dict:
    """the lines of one category -> {"meshes", "share": {closed, manifold, oriented, no_self_intersection, watertight},
    "mean": {every count of postprocess.CHECK_FIELDS, over the meshes where it is valid (>= 0)}, "status": {status:
    meshes}}"""
    from .postprocess import CHECK_FIELDS
    n = len(rows)
    flag = lambda r, k: r["intersecting_pairs"] == 0 if k == "no_self_intersection" else bool(r[k])
    share = {k: (sum(flag(r, k) for r in rows) / n if n else 0.0) for k in MESH_CHECK_SHARES}
    mean = {}
    for k in CHECK_FIELDS:
        valid = [r[k] for r in rows if r[k] >= 0]
        mean[k] = float(np.mean(valid)) if valid else None
    status: Dict[str, int] = {}
    for r in rows:
        status[str(r["status"])] = status.get(str(r["status"]), 0) + 1
    return {"meshes": n, "share": share, "mean": mean, "status": status}


def mesh_check_all(cats: Dict[str, str], obj_dir: str, group: int = 16, pairs_per_face: Optional[int] = None,
                   out=sys.stdout, check_fn=None) -> dict:
    """``mesh_check OBJ_DIR``: every ``<obj_dir>/<cat_id>/*.obj`` of the listed categories through
    ``postprocess.check_meshes_device`` in groups of ``group`` files (``check_fn``: see ``create_sdf.check_group``);
    one JSON line per mesh in ``<obj_dir>/checks.jsonl`` (the lines of ``create_sdf --check``: "view" is the file's
    name), started afresh, and a summary per category -> {"categories": {name: mesh_check_summary}, "checked",
    "watertight", "out"}.  An empty file is a mesh without triangles.  No mesh raises: a bad file's status is in its
    line."""
    import json

    from . import mesh_sdf
    from .create_sdf import CHECK_PAIRS_PER_FACE, check_group
    if group < 1:
        raise ValueError("--group must be positive")
    pairs = CHECK_PAIRS_PER_FACE if pairs_per_face is None else pairs_per_face
    if pairs < 0:
        raise ValueError("--check_pairs must not be negative")
    path = os.path.join(obj_dir, "checks.jsonl")
    per, checked, watertight = {}, 0, 0
    with open(path, "w") as lines:
        for name, cat_id in cats.items():
            files = sorted(glob.glob(os.path.join(obj_dir, cat_id, "*.obj")))
            rows = []
            for at in range(0, len(files), group):
                part = files[at:at + group]
                host = [mesh_sdf.read_obj_mesh(f) if os.path.getsize(f) else
                        (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)) for f in part]
                if check_fn is None:
                    import torch
                    host = [(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()) for v, f in host]
                keys = [(cat_id, os.path.splitext(os.path.basename(f))[0], os.path.basename(f)) for f in part]
                rows += check_group(host, keys, pairs, check_fn)
            for r in rows:
                lines.write(json.dumps(r) + "\n")
            per[name] = mesh_check_summary(rows)
            checked += len(rows)
            watertight += sum(r["watertight"] for r in rows)
            s = per[name]
            print("%s (%s): %d meshes; %s" % (name, cat_id, s["meshes"], ", ".join(
                "%s %.1f%%" % (k, 100.0 * s["share"][k]) for k in MESH_CHECK_SHARES)), file=out)
            print("  mean " + ", ".join("%s %s" % (k, "-" if v is None else "%.4g" % v) for k, v in s["mean"].items()),
                  file=out)
    return {"categories": per, "checked": checked, "watertight": watertight, "out": path}


def regularization_of(store, wd: float = 1e-5) -> float:
    """wd * sum(w^2) / 2 over every '/weights' variable: the scalar the trainer adds to its loss, a function of the
    weights alone (float64 on the host, once per weight set)"""
    return float(sum(wd * 0.5 * float(np.sum(np.asarray(store[k], np.float64) ** 2))
                     for k in store.keys() if k.endswith("/weights")))


def sdf_acc(cats: Dict[str, str], log_dir: str, test_lst_dir: str, sdf_dir: str, rendered_dir: str,
            batch_size: int = 1, num_sample_points: int = 2048, mask_weight: float = 4.0, view_num: int = 24,
            seed: int = 0, random_init: Optional[int] = None, rot: bool = False, backcolorwhite: bool = False,
            wd: float = 1e-5, out=None) -> dict:
    """test/test_sdf_acc.py test_one_epoch -> {"accuracy", "sdf_loss_realvalue", "sdf_loss", "regularization",
    "overall_loss"} (means of the per-batch values) and "batches" (the per-batch values, [n,5])"""
    import torch

    from . import create_sdf as cs, ops
    from .engine import SdfEngine
    out = out or sys.stdout
    if batch_size < 1 or batch_size * num_sample_points > 65536:
        raise ValueError("--batch_size x --num_sample_points must be in 1..65536 (one encode_query call), got %d x %d"
                         % (batch_size, num_sample_points))
    work = cs.groups(cs.sample_list(cats, test_lst_dir, view_num, seed), batch_size)
    store, note = cs.restore_weights(log_dir, random_init)            # before any device work
    print(note, file=out)
    engine = SdfEngine(store)
    reg = regularization_of(store, wd)
    rows = []
    for gi, group in enumerate(work):
        batch = cs.load_group(group, sdf_dir, rendered_dir, backcolorwhite, num_sample_points, rot, seed + gi)
        gt = torch.from_numpy(np.ascontiguousarray(batch["sdf_val"] - 0.003, np.float32)).to(engine.device)
        pred = engine.encode_query(batch["img"], batch["sdf_pt"], batch["trans_mat"], batch["sdf_pt_rot"])[1]
        with torch.cuda.device(engine.device):
            vals = ops.get_loss(pred, gt, SDF_WEIGHT, mask_weight, reg).cpu().numpy().astype(np.float64)
        rows.append(vals)
        print(" -- %03d / %03d -- " % (gi + 1, len(work)) + "".join("%s: %f, " % (n, v)
                                                                    for n, v in zip(SDF_ACC_NAMES, vals)), file=out)
    mean = np.mean(np.asarray(rows), axis=0)
    print("Summary: " + "".join("%s: %f, " % (n, v) for n, v in zip(SDF_ACC_NAMES, mean)), file=out)
    res = {n: float(v) for n, v in zip(SDF_ACC_NAMES, mean)}
    res["batches"] = np.asarray(rows)
    return res


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m disn_amd.evaluate",
                                description="Chamfer / EMD / F-score / voxel IoU of reconstructed meshes "
                                            "(test_cd_emd.py, test_f_score.py, test_iou.py)")
    sub = p.add_subparsers(dest="command", required=True)
    for name, hlp in (("cd_emd", "Chamfer distance and approximate EMD per object and category"),
                      ("f_score", "precision, recall and F-score at six distance thresholds")):
        s = sub.add_parser(name, help=hlp)
        s.add_argument("--cal_dir", required=True, help="directory of the predicted meshes (<cat_id>/*.obj)")
        s.add_argument("--gt_dir", required=True, help="ground-truth meshes (<cat_id>/<obj_id>/isosurf.obj)")
        s.add_argument("--test_lst_dir", required=True, help="object lists (<cat_id>_test.lst)")
        s.add_argument("--category", default="all", help="all, clean or one category name [default: all]")
        s.add_argument("--view_num", type=int, default=24, help="views per object [default: 24]")
        s.add_argument("--num_sample_points", type=int, default=2048, help="points per mesh [default: 2048]")
        s.add_argument("--truethreshold", type=float, default=2.5, help="F-score side length [default: 2.5]")
        s.add_argument("--seed", type=int, default=0, help="seed of the point and view sampling [default: 0]")
    s = sub.add_parser("surface", help="Chamfer-L1, normal consistency and F-score on area-weighted surface samples "
                                       "(not in the reference)")
    s.add_argument("--pred_dir", required=True, help="directory of the predicted meshes (<cat_id>/*.obj)")
    s.add_argument("--gt_dir", required=True, help="ground-truth meshes (<cat_id>/<obj_id>/isosurf.obj)")
    s.add_argument("--test_lst_dir", required=True, help="object lists (<cat_id>_test.lst)")
    s.add_argument("--category", default="all", help="all, clean or one category name [default: all]")
    s.add_argument("--view_num", type=int, default=24, help="views per object [default: 24]")
    s.add_argument("--num_sample_points", type=int, default=2048, help="surface samples per mesh [default: 2048]")
    s.add_argument("--truethreshold", type=float, default=2.5, help="F-score side length [default: 2.5]")
    s.add_argument("--seed", type=int, default=0, help="seed of the samples and the view choice [default: 0]")
    s = sub.add_parser("iou", help="voxel IoU per object and category")
    s.add_argument("--cal_dir", required=True, help="directory of the predicted meshes (<cat_id>/*.obj)")
    s.add_argument("--gt_dir", required=True, help="ground-truth meshes (<cat_id>/<obj_id>/isosurf.obj)")
    s.add_argument("--test_lst_dir", required=True, help="object lists (<cat_id>_test.lst)")
    s.add_argument("--category", default="all", help="all, clean or one category name [default: all]")
    s.add_argument("--view_num", type=int, default=24, help="views per object [default: 24]")
    s.add_argument("--dim", type=int, default=110, help="voxels per axis of [-1, 1] [default: 110]")
    s.add_argument("--mode", default="reference", choices=("reference", "solid"),
                   help="reference: the shell IoU of test_iou.py; solid: filled voxels [default: reference]")
    s.add_argument("--seed", type=int, default=0, help="seed of the view sampling [default: 0]")
    s = sub.add_parser("mesh_check", help="topology, orientation and self-intersections of every mesh of a tree, on "
                                          "the device (not in the reference)")
    s.add_argument("obj_dir", metavar="OBJ_DIR", help="directory of the meshes (<cat_id>/*.obj)")
    s.add_argument("--category", default="all", help="all, clean or one category name [default: all]")
    s.add_argument("--group", type=int, default=16, help="meshes per device call [default: 16]")
    s.add_argument("--check_pairs", type=int, default=None, metavar="N",
                   help="the work cap, candidate pairs per face [default: 256]")
    s = sub.add_parser("sdf_acc", help="accuracy and losses of the predicted SDF on sampled points of the test views")
    s.add_argument("--log_dir", required=True, help="checkpoint directory of the SDF network")
    s.add_argument("--test_lst_dir", required=True, help="object lists (<cat_id>_test.lst)")
    s.add_argument("--sdf_dir", required=True, help="sampled SDF values (<cat_id>/<obj_id>/ori_sample.h5)")
    s.add_argument("--rendered_dir", required=True, help="rendered views (<cat_id>/<obj_id>/%%02d.h5)")
    s.add_argument("--category", default="all", help="all, clean or one category name [default: all]")
    s.add_argument("--batch_size", type=int, default=1, help="views per encode_query call [default: 1]")
    s.add_argument("--num_sample_points", type=int, default=2048, help="points per view [default: 2048]")
    s.add_argument("--mask_weight", type=float, default=4.0)
    s.add_argument("--view_num", type=int, default=24, help="views per object [default: 24, all]")
    s.add_argument("--rot", action="store_true")
    s.add_argument("--backcolorwhite", action="store_true")
    s.add_argument("--seed", type=int, default=0, help="seed of the view and point sampling [default: 0]")
    s.add_argument("--random_init", type=int, default=None, metavar="SEED",
                   help="run on freshly initialised weights when log_dir holds no complete checkpoint")
    return p


def main(argv=None) -> dict:
    a = parser().parse_args(argv)
    cats = categories(a.category)
    if a.command == "sdf_acc":
        return sdf_acc(cats, a.log_dir, a.test_lst_dir, a.sdf_dir, a.rendered_dir, batch_size=a.batch_size,
                       num_sample_points=a.num_sample_points, mask_weight=a.mask_weight, view_num=a.view_num,
                       seed=a.seed, random_init=a.random_init, rot=a.rot, backcolorwhite=a.backcolorwhite)
    if a.command == "mesh_check":
        return mesh_check_all(cats, a.obj_dir, group=a.group, pairs_per_face=a.check_pairs)
    if a.command == "surface":
        return surface_all(cats, a.pred_dir, a.gt_dir, a.test_lst_dir, truethreshold=a.truethreshold,
                           view_num=a.view_num, num_sample_points=a.num_sample_points, seed=a.seed)
    if a.command == "iou":
        return iou_all(cats, a.cal_dir, a.gt_dir, a.test_lst_dir, dim=a.dim, mode=a.mode, view_num=a.view_num,
                       seed=a.seed)
    if a.command == "cd_emd":
        return cd_emd_all(cats, a.cal_dir, a.gt_dir, a.test_lst_dir, seed=a.seed, view_num=a.view_num,
                          num_sample_points=a.num_sample_points)
    return cal_f_score_all_cat(cats, a.cal_dir, a.gt_dir, a.test_lst_dir, truethreshold=a.truethreshold,
                               num_sample_points=a.num_sample_points, seed=a.seed)


if __name__ == "__main__":
    main()

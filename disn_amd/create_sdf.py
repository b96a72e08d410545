"""Dense-grid SDF evaluation driver: the hot loop of the reference's ``test/create_sdf.py``
(and ``demo/demo.py``) on the HIP engine.

Reference (/root/reference): split arithmetic test/create_sdf.py:69-77; grid construction
:246-256; per-split ``sess.run`` loop :262-276; un-pad + ``/ SDF_WEIGHT`` :277-285; ``.dist``
writer :292-303.  Differences by design (MI355X-first):
  * the encoder runs ONCE per image, not once per split (80x at res 256);
  * grid points are generated on the device from ``sdf_params`` (float64 linspace, cast to
    float32 -- bit-identical to the numpy grid), no 204 MB host->device copy, no padding points;
  * chunks stream through ``disn_query_grid`` in the flat (iz,iy,ix) order of the reference;
  * with ``torch.distributed`` initialised the flat index range is sharded contiguously
    across ranks and collected with one all_gather (RCCL over xGMI) -- see parallel.py.

The test-set driver (``python -m disn_amd.create_sdf``, the reference's ``test/create_sdf.py --create_obj``):

    python -m disn_amd.create_sdf --log_dir CKPT --test_lst_dir LSTS --sdf_dir SDF --rendered_dir VIEWS
                                  [--category all] [--sdf_res 64] [--iso 0.0] [--view_num 24] [--cam_est]
                                  [--band STRIDE --band_margin 0.5 --band_dilate 1]

walks ``<test_lst_dir>/<cat_id>_test.lst``, encodes ``--batch_size`` views per call, fills their grids, meshes
the whole group with one read-back (``isosurface.marching_cubes_batch``) and writes
``<log_dir>/test_objs/[camest_]<res+1>_<iso>/<cat_id>/<cat_id>_<obj>_<view>.obj`` -- the directory
``disn_amd.evaluate`` and ``disn_amd.postprocess`` read.  Differences from the reference, on purpose:
  * groups are consecutive runs of ``--batch_size`` list entries and the LAST, shorter one is kept (the
    reference runs ``len // batch_size`` batches and loses the tail);
  * a missing or incomplete checkpoint is an error unless ``--random_init SEED`` is given (the reference
    prints a line and goes on with the initialiser's weights);
  * the views of an object are ``sorted(random.Random(seed).sample(range(24), view_num))``, drawn object by
    object in list order from ONE generator (the reference draws from the unseeded global one, unsorted);
  * categories come in the order of ``evaluate.CATS_ALL`` (``--category`` also takes several names separated
    by commas); ``--num_shards`` / ``--shard_id`` split the OBJECTS
    (never an object's views) after the views were drawn, so shards write what one run writes;
  * an empty mesh is written (and logged), not skipped; a writer thread's exception fails the run;
  * ``--skip_existing`` drops entries whose file exists with more than 200 bytes (the size filter of
    ``evaluate.build_file_dict(min_size=200)``) before the groups are formed;
  * ``--band STRIDE`` (2, 4 or 8; default 0 = the dense grid) evaluates the network on every STRIDE-th grid point and
    then only near the ``--iso`` surface, the rest of the grid interpolated (``SdfEngine.query_grid_band``);
  * ``--fuse_views V [--fuse_pool max|mean]`` (multi-view) fuses every run of V chosen views of an object
    into ONE mesh, the features pooled over the views (``reconstruct_fused``): view_num / V meshes per object, each
    named after the first view of its run, in ``test_objs/[camest_]fuse<V><pool>_<res+1>_<iso>`` -- score them with
    ``disn_amd.evaluate --view_num view_num/V``.  Not combinable with ``--band``, ``--refine`` or ``--normals``;
  * ``--clean CATS [--clean_dist_thresh 0.5 --clean_num_thresh 0.3 --clean_connectivity face]`` drops the small and
    the far parts (``postprocess.clean_meshes_device``) of every mesh of the listed categories (``clean`` =
    the reference's five, ``all``, or names separated by commas) while the group still lies on the device, before
    ``--refine``; the other categories are written as they are, and the tree goes to ``<...>_comb``: it is the
    ``_comb`` tree of the two-step route.  A mesh of which nothing is kept is written uncleaned,
    logged and counted as "unclean".  Composes with ``--band``, ``--refine``, ``--normals`` and ``--fuse_views``.
  * ``--simplify CELLS`` (1..1024; the reference does not simplify) clusters every mesh's vertices on a lattice of
    CELLS cells along the longest side of the view's ``sdf_params`` box and places each cluster by its faces' quadric
    (``postprocess.simplify_meshes_device``) while the group still lies on the device: behind ``--clean``
    and BEFORE ``--refine`` and ``--normals``, so the refinement pulls the moved vertices back onto the network's
    level set and the normals are the gradients at the final vertices.  The tree goes to ``<...>[_comb]_s<CELLS>``.
    ``evaluate``'s cd_emd and f_score sample VERTICES, as the reference's do: the scores of a simplified tree are
    not the reference's numbers.  Composes with every flag above.
  * ``--score GT_DIR [--score_points 2048]`` (not in the reference) scores every group's FINAL meshes -- behind clean,
    simplify and colour, while they still lie on the device -- on area-weighted surface samples against
    ``<GT_DIR>/<cat_id>/<obj>/isosurf.obj`` (``metrics.sample_surface_meshes_device`` / ``surface_scores``, DESIGN 4zc;
    the ground truth is sampled once per object and kept on the device) and appends one JSON line per mesh to
    ``<out_dir>/scores.jsonl`` (started afresh by a run that scores every listed mesh; with ``--skip_existing`` the
    lines of the meshes done now are appended to those of the earlier runs).  A ground truth without area is logged
    and marked ``"gt_status": 6`` in its lines.  A mesh's samples depend on ``--seed`` and its file name alone.  Composes with every
    flag above; without it nothing changes.
  * ``--check [--check_pairs 256]`` (not in the reference) measures every group's FINAL meshes where ``reconstruct``
    left them, before the writers take them (``postprocess.check_meshes_device``): topology, orientation
    and self-intersections, one JSON line per mesh in ``<out_dir>/checks.jsonl`` -- "cat", "obj", "view", "status",
    every field of ``postprocess.CHECK_FIELDS``, "area", "volume" and the four derived booleans -- started afresh
    by a run without ``--skip_existing``.  ``--check_pairs N``: the work cap, N candidate pairs per face (+ 4096); a
    mesh over it has status 8 and -1 in its intersection fields.  No stage: the meshes and the tree's name stay.
  * ``--repair [--repair_no_weld] [--repair_no_stitch]`` (not in the reference) welds, stitches and splits every mesh to
    a manifold while the group still lies on the device (``postprocess.repair_meshes_device``): behind
    ``--smooth``, ``--refine`` and ``--normals`` (the normals follow their vertices) and before ``--colour``, ``--score``
    and ``--check``, which see the repaired mesh.  Results go to <...>_rep[_col]; one JSON line per mesh -- "cat", "obj",
    "view" and the report of ``postprocess.repair_arrays`` -- to ``<out_dir>/repairs.jsonl``, started afresh by a run
    without ``--skip_existing``.  Without the flag nothing changes.
  * ``--close [--close_no_orient] [--close_no_fill] [--close_outward] [--close_max_hole N]`` (not in the reference)
    orients every mesh consistently and fills its holes while the group still lies on the device
    (``postprocess.close_meshes_device``): directly behind ``--repair`` (a mesh that is not manifold is
    refused: give ``--repair``) and before ``--colour``, ``--score`` and ``--check``, which see the closed mesh.  Results
    go to <...>[_rep]_cls[_col]; one JSON line per mesh -- "cat", "obj", "view" and the report of
    ``postprocess.close_arrays`` -- to ``<out_dir>/closes.jsonl``, started afresh by a run without ``--skip_existing``.
    Without the flag nothing changes.
  * ``--smooth ITERS [--smooth_cap CELLS] [--smooth_free_boundary]`` (1..64 iterations; not in the reference) fairs every
    mesh by Taubin's lambda|mu smoothing (``postprocess.smooth_meshes_device``) while the group still lies
    on the device: behind ``--clean`` and ``--simplify`` and BEFORE ``--refine`` and ``--normals``, so the smoothed
    vertices are what the Newton steps pull back onto the level set and what is coloured and scored.  No coordinate
    moves further than CELLS grid cells of its view's box (longest side / sdf_res each; default 0.5) from where it was;
    boundary vertices stay where they are unless ``--smooth_free_boundary`` is given.  Faces never change.  The tree
    goes to ``<...>[_comb]_t<ITERS>[_s<CELLS>]``.  Composes with every flag above; without it nothing changes.
"""
from __future__ import annotations

import json
import math
import os
import random
import struct
import sys
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

SDF_WEIGHT = 10.0   # test/create_sdf.py:285


def split_plan(sdf_res: int, twostream: bool = True) -> Tuple[int, int, int, int]:
    """(TOTAL_POINTS, SPLIT_SIZE, NUM_SAMPLE_POINTS, pad) exactly as test/create_sdf.py:69-77.
    Kept for callers that feed fixed-shape splits through ``Session.run``."""
    resolution = sdf_res + 1
    total = resolution ** 3
    split = int(math.ceil(total / (214669.0 if twostream else 274625.0)))
    nsp = int(math.ceil(total / split))
    return total, split, nsp, split * nsp - total


def grid_points_host(sdf_params: Sequence[float], sdf_res: int) -> np.ndarray:
    """Host grid as the reference builds it (test/create_sdf.py:246-256) -- for callers that
    still feed points through placeholders.  The device path never materialises this."""
    res = sdf_res + 1
    # float64 linspace: what numpy 1.x computes for int / float64 sdf_params (demo/demo.py:278 passes ints).  For
    # FLOAT32 sdf_params numpy 1.x forms delta = stop - start and step = delta / div as float32 scalars before the
    # float64 arange multiply; with a box whose float32 difference or division is inexact (not the +-1 demo box
    # or any dyadic box) the coordinates then drift from this grid by the accumulated step rounding, up to
    # R * ulp32(step) / 2 ~ 1e-7 of the box (tests/test_oracle.py::test_grid_float32_params_caveat).  numpy >= 2 computes in float32.
    p = np.asarray(sdf_params, dtype=np.float64)
    x_ = np.linspace(p[0], p[3], num=res)
    y_ = np.linspace(p[1], p[4], num=res)
    z_ = np.linspace(p[2], p[5], num=res)
    z, y, x = np.meshgrid(z_, y_, x_, indexing='ij')
    return np.stack((x, y, z), axis=3).astype(np.float32).reshape(-1, 3)


def to_binary(res: int, pos: Sequence[float], pred_sdf_val_all: np.ndarray, sdf_file: str) -> None:
    """The ``.dist`` wire format consumed by isosurface/computeMarchingCubes
    (test/create_sdf.py:292-303): int32 -res, res, res; 6 x float64 bbox (min xyz, max xyz);
    (res+1)^3 float32 values, x fastest."""
    vals = np.ascontiguousarray(pred_sdf_val_all, dtype=np.float32).ravel()
    with open(sdf_file, 'wb') as f:
        f.write(struct.pack('i', -res))
        f.write(struct.pack('i', res))
        f.write(struct.pack('i', res))
        f.write(struct.pack('d' * len(pos), *[float(v) for v in pos]))
        f.write(vals.astype('<f4').tobytes())


def read_dist(sdf_file: str):
    """Inverse of to_binary (format as read by preprocessing/create_point_sdf_grid.py:29-51)."""
    with open(sdf_file, 'rb') as f:
        raw = f.read()
    ress = np.frombuffer(raw[:12], dtype=np.int32)
    res = int(ress[1])
    if -ress[0] != res or ress[2] != res:
        raise ValueError("inconsistent .dist header %s" % (ress,))
    pos = np.frombuffer(raw[12:12 + 48], dtype=np.float64)
    vals = np.frombuffer(raw[60:], dtype=np.float32).reshape(res + 1, res + 1, res + 1)
    return res, pos, vals


def dense_grid_sdf(engine, enc, image_index: int, trans_mat, sdf_params, sdf_res: int,
                   sdf_weight: float = SDF_WEIGHT, out=None, k_range: Optional[Tuple[int, int]] = None):
    """SDF/10 on the (res+1)^3 grid of one encoded image, flat (iz,iy,ix) order, as a device
    tensor.  ``k_range`` restricts to a contiguous flat-index slice (used by the sharded path)."""
    total = (sdf_res + 1) ** 3
    k0, k1 = (0, total) if k_range is None else k_range
    return engine.query_grid(enc, image_index, trans_mat, sdf_params, sdf_res, k0, k1, sdf_weight, out)


def band_args(band, sdf_res: int) -> Optional[Tuple[int, float, int]]:
    """``band`` = None or (stride, margin, dilate) checked against the resolution (ValueError; no device work):
    the narrow-band evaluation of ``SdfEngine.query_grid_band``"""
    if band is None:
        return None
    stride, margin, dilate = band
    stride, margin, dilate = int(stride), float(margin), int(dilate)
    if stride not in (2, 4, 8):
        raise ValueError("--band must be 0 (dense) or one of 2, 4, 8, got %d" % stride)
    if sdf_res < stride or sdf_res % stride or sdf_res > 1289:
        raise ValueError("--band %d needs --sdf_res to be a multiple of it (at most 1289), got %d" % (stride, sdf_res))
    if not margin >= 0.0:
        raise ValueError("--band_margin must not be negative")
    if dilate < 0:
        raise ValueError("--band_dilate must not be negative")
    return stride, margin, dilate


def add_band_flags(p) -> None:
    p.add_argument("--band", type=int, default=0, metavar="STRIDE",
                   help="narrow-band grid: evaluate every STRIDE-th point (2, 4 or 8), then only near the surface "
                        "[default: 0, the dense grid]")
    p.add_argument("--band_margin", type=float, default=0.5,
                   help="a coarse cell is active when iso lies within its corner range widened by this share of it "
                        "[default: 0.5]")
    p.add_argument("--band_dilate", type=int, default=1, help="rounds of dilation of the active cells [default: 1]")


def band_from_flags(a) -> Optional[Tuple[int, float, int]]:
    """None for --band 0, else the checked (stride, margin, dilate)"""
    if a.band == 0:
        return None
    return band_args((a.band, a.band_margin, a.band_dilate), a.sdf_res)


def _encode_grids(engine, imgs, trans_mats, sdf_params, sdf_res: int, sdf_weight: float = SDF_WEIGHT):
    """one ``engine.encode`` call and the grid of every image -> (Encoded, result [B, (res+1)^3])"""
    import torch
    imgs = np.asarray(imgs, np.float32) if not isinstance(imgs, torch.Tensor) else imgs
    B = imgs.shape[0]
    enc = engine.encode(imgs)
    total = (sdf_res + 1) ** 3
    result = torch.empty((B, total), dtype=torch.float32, device=engine.device)
    sp = np.asarray(sdf_params, dtype=np.float64).reshape(B, 6)
    for b in range(B):
        dense_grid_sdf(engine, enc, b, trans_mats, sp[b], sdf_res, sdf_weight, out=result[b])
    return enc, result


def _encode_grids_band(engine, imgs, trans_mats, sdf_params, sdf_res: int, iso: float, band,
                       sdf_weight: float = SDF_WEIGHT):
    """``_encode_grids`` through the narrow band: all coarse passes, then all selections, ONE copy of the B pairs of
    data-dependent counts, then the band passes and fills -> (Encoded, result [B, (res+1)^3], stats per image).  Every
    image's grid is bit for bit ``engine.query_grid_band``'s."""
    import torch
    stride, margin, dilate = band
    imgs = np.asarray(imgs, np.float32) if not isinstance(imgs, torch.Tensor) else imgs
    B = imgs.shape[0]
    enc = engine.encode(imgs)
    total = (sdf_res + 1) ** 3
    result = torch.empty((B, total), dtype=torch.float32, device=engine.device)
    counts = torch.zeros((B, 2), dtype=torch.int64, device=engine.device)
    sp = np.asarray(sdf_params, dtype=np.float64).reshape(B, 6)
    for b in range(B):
        engine.band_coarse(enc, b, trans_mats, sp[b], sdf_res, stride, sdf_weight, out=result[b])
    picked = [engine.band_select(result[b], sdf_res, iso, stride, margin, dilate, counts=counts[b]) for b in range(B)]
    sizes = counts.cpu().numpy()                      # the one host sync of the group's grids
    stats = []
    for b in range(B):
        mask, idx, _ = picked[b]
        engine.band_finish(enc, b, trans_mats, sp[b], sdf_res, result[b], mask, idx, int(sizes[b, 0]), stride,
                           sdf_weight)
        stats.append({"coarse_points": (sdf_res // stride + 1) ** 3, "band_points": int(sizes[b, 0]),
                      "active_cells": int(sizes[b, 1]), "total_points": total})
    return enc, result, stats


def create_sdf(engine, imgs, trans_mats, sdf_params, sdf_res: int, sdf_weight: float = SDF_WEIGHT, band=None,
               iso: float = 0.0):
    """``test_one_epoch`` for one batch (test/create_sdf.py:240-285): returns ``result`` --
    a float32 device tensor [B, (res+1)^3] of pred_sdf / SDF_WEIGHT.  ``band`` = (stride, margin, dilate): the
    narrow-band evaluation around ``iso`` (``SdfEngine.query_grid_band``; points away from the surface interpolated)."""
    band = band_args(band, sdf_res)
    if band is None:
        return _encode_grids(engine, imgs, trans_mats, sdf_params, sdf_res, sdf_weight)[1]
    return _encode_grids_band(engine, imgs, trans_mats, sdf_params, sdf_res, iso, band, sdf_weight)[1]


def clean_args(clean) -> Optional[Tuple[float, float, str]]:
    """``clean`` = None or (dist_thresh, num_thresh, connectivity) checked (ValueError; no device work): what
    ``reconstruct`` / ``reconstruct_fused`` hand to ``postprocess.clean_meshes_device``"""
    if clean is None:
        return None
    from .postprocess import CONNECTIVITY
    dist_thresh, num_thresh, connectivity = clean
    dist_thresh, num_thresh = float(dist_thresh), float(num_thresh)
    if not dist_thresh >= 0.0:
        raise ValueError("--clean_dist_thresh must not be negative")
    if not num_thresh >= 0.0:
        raise ValueError("--clean_num_thresh must not be negative")
    if connectivity not in CONNECTIVITY:
        raise ValueError("--clean_connectivity must be one of %s, got %r" % (", ".join(sorted(CONNECTIVITY)),
                                                                             connectivity))
    return dist_thresh, num_thresh, connectivity


def _through(meshes, on: bool, call, select=None):
    """pick, call once, scatter back: the meshes with triangles that ``select`` marks (None: all) go through ONE
    ``call(their indices, those meshes)`` -> their new meshes in that order, None for one that stays as it is.
    -> (meshes, left [B] bool: the picked meshes that stayed).  Not ``on``, or nothing picked: no call."""
    meshes = list(meshes)
    left = [False] * len(meshes)
    picked = [b for b, m in enumerate(meshes) if (select is None or select[b]) and len(m[1])] if on else []
    if picked:
        for b, m in zip(picked, call(picked, [meshes[b] for b in picked])):
            if m is None:
                left[b] = True
            else:
                meshes[b] = m
    return meshes, left


def clean_group(meshes, clean, select=None, strict: bool = True):
    """the small-part cleanup of one group right behind its meshing: the meshes ``select`` marks (None: all) that
    have triangles go through ONE ``clean_meshes_device`` call.  -> (meshes, unclean [B] bool).  ``strict``: a mesh
    of which nothing is kept raises; otherwise it stays as it is and is marked in ``unclean``."""
    from . import postprocess
    return _through(meshes, clean is not None, lambda picked, some: postprocess.clean_meshes_device(
        some, clean[0], clean[1], clean[2], strict=strict)[0], select)


def simplify_args(simplify) -> Optional[int]:
    """``simplify`` = None or the number of lattice cells along the box's longest side, checked (ValueError; no device
    work): what ``reconstruct`` / ``reconstruct_fused`` hand to ``postprocess.simplify_meshes_device``"""
    if simplify is None:
        return None
    from .postprocess import MAX_CELLS
    try:
        cells = int(simplify)
    except (TypeError, ValueError):
        cells = None
    if cells is None or cells != simplify or not 1 <= cells <= MAX_CELLS:
        raise ValueError("--simplify must be a number of cells in 1..%d, got %r" % (MAX_CELLS, simplify))
    return cells


def simplify_group(meshes, simplify, boxes):
    """the simplification of one group behind its meshing and cleanup: the meshes that have triangles go through ONE
    ``simplify_meshes_device`` call, each on the lattice of its own box (``boxes`` [B,6]) -> the meshes"""
    from . import postprocess
    return _through(meshes, simplify is not None, lambda picked, some: postprocess.simplify_meshes_device(
        some, np.asarray(boxes, np.float64).reshape(len(meshes), 6)[picked], simplify)[0])[0]


SMOOTH_CAP_CELLS = 0.5        # --smooth_cap: the largest move of a coordinate, in grid cells of the view's box


def smooth_args(smooth) -> Optional[dict]:
    """``smooth`` = None (off), the number of iterations, or a dict with ``iters`` and some of ``lam``, ``mu``, ``cap``
    (grid cells of the view's box a coordinate may move; None: no cap) and ``pin_boundary`` -> None or the checked,
    complete dict (ValueError; no device work): what ``reconstruct`` / ``reconstruct_fused`` hand to ``smooth_group``"""
    if smooth is None:
        return None
    from .postprocess import smooth_params
    given = dict(smooth) if isinstance(smooth, dict) else {"iters": smooth}
    unknown = sorted(set(given) - {"iters", "lam", "mu", "cap", "pin_boundary"})
    if unknown:
        raise ValueError("--smooth takes iters, lam, mu, cap and pin_boundary, not %s" % ", ".join(unknown))
    if "iters" not in given:
        raise ValueError("--smooth needs the number of iterations")
    c = dict({"lam": 0.5, "mu": -0.53, "cap": SMOOTH_CAP_CELLS, "pin_boundary": True}, **given)
    try:
        c["iters"], c["lam"], c["mu"], _ = smooth_params(c["iters"], c["lam"], c["mu"])
    except ValueError as e:
        raise ValueError("--smooth: %s" % e) from e
    if c["cap"] is not None:
        try:
            cap = float(c["cap"])
        except (TypeError, ValueError):
            cap = float("nan")
        if isinstance(c["cap"], bool) or not (math.isfinite(cap) and cap >= 0.0):
            raise ValueError("--smooth_cap must be a finite number of cells >= 0, got %r" % (c["cap"],))
        c["cap"] = cap
    c["pin_boundary"] = bool(c["pin_boundary"])
    return c


def smooth_cap(smooth, boxes, sdf_res: int):
    """the cap of every mesh in the units of its vertices: ``cap`` grid cells of its box, longest side / sdf_res each
    -> float64 [B], or None without a cap"""
    if smooth["cap"] is None:
        return None
    boxes = np.asarray(boxes, np.float64).reshape(-1, 6)
    return smooth["cap"] * ((boxes[:, 3:] - boxes[:, :3]).max(1) / np.float64(sdf_res))


def smooth_group(meshes, smooth, boxes, sdf_res: int):
    """the smoothing of one group behind its meshing, cleanup and simplification: the meshes that have triangles go
    through ONE ``smooth_meshes_device`` call, each with the cap of its own box (``boxes`` [B,6]) -> the meshes"""
    from . import postprocess

    def call(picked, some):
        cap = smooth_cap(smooth, np.asarray(boxes, np.float64).reshape(len(meshes), 6), sdf_res)
        return postprocess.smooth_meshes_device(some, smooth["iters"], smooth["lam"], smooth["mu"],
                                                smooth["pin_boundary"], None if cap is None else cap[picked])[0]
    return _through(meshes, smooth is not None, call)[0]


def repair_args(repair) -> Optional[dict]:
    """``repair`` = None / False (off), True (weld and stitch) or a dict with some of ``weld``, ``stitch`` -> None or the
    checked, complete dict (ValueError; no device work): what ``reconstruct`` / ``reconstruct_fused`` hand to
    ``repair_group``"""
    if repair is None or repair is False:
        return None
    given = {} if repair is True else repair
    if not isinstance(given, dict):
        raise ValueError("--repair takes True or a dict of weld and stitch, got %r" % (repair,))
    unknown = sorted(set(given) - {"weld", "stitch"})
    if unknown:
        raise ValueError("--repair takes weld and stitch, not %s" % ", ".join(unknown))
    c = dict({"weld": True, "stitch": True}, **given)
    for k in ("weld", "stitch"):
        if not isinstance(c[k], (bool, np.bool_)):
            raise ValueError("--repair: %s must be True or False, got %r" % (k, c[k]))
        c[k] = bool(c[k])
    return c


def repair_group(meshes, repair, log: Optional[list] = None):
    """the repair of one group behind its smoothing and refinement: the meshes that have triangles go through ONE
    ``repair_meshes_device`` call; every further per-vertex array (the normals) follows its vertex -> the meshes.
    ``log``: a list that takes one report per mesh of the group, in mesh order (``postprocess.repair_arrays``; a mesh
    without triangles stays as it is and reports zeros)"""
    from . import postprocess
    reports: dict = {}

    def call(picked, some):
        repaired, reps = postprocess.repair_meshes_device(some, repair["weld"], repair["stitch"])
        reports.update(zip(picked, reps))
        return [m[:-2] for m in repaired]                     # without vmap and kept
    out = _through(meshes, repair is not None, call)[0]
    if log is not None and repair is not None:
        for b, m in enumerate(meshes):
            zeros = np.zeros(len(postprocess.REPAIR_FIELDS), np.int64)
            zeros[0] = len(m[0])
            log.append(reports.get(b) or postprocess.repair_report(zeros, len(m[0]), len(m[1])))
    return out


def close_args(close) -> Optional[dict]:
    """``close`` = None / False (off), True (orient and fill) or a dict with some of ``orient``, ``fill``, ``outward``,
    ``max_hole`` -> None or the checked, complete dict (ValueError; no device work): what ``reconstruct`` /
    ``reconstruct_fused`` hand to ``close_group``"""
    if close is None or close is False:
        return None
    given = {} if close is True else close
    if not isinstance(given, dict):
        raise ValueError("--close takes True or a dict of orient, fill, outward and max_hole, got %r" % (close,))
    unknown = sorted(set(given) - {"orient", "fill", "outward", "max_hole"})
    if unknown:
        raise ValueError("--close takes orient, fill, outward and max_hole, not %s" % ", ".join(unknown))
    from .postprocess import close_flags
    c = dict({"orient": True, "fill": True, "outward": False, "max_hole": None}, **given)
    try:
        _, cap = close_flags(c["orient"], c["fill"], c["outward"], c["max_hole"])
    except ValueError as e:
        raise ValueError("--" + str(e)) from e                 # "--close: outward needs orient"
    return {"orient": bool(c["orient"]), "fill": bool(c["fill"]), "outward": bool(c["outward"]), "max_hole": cap}


def close_group(meshes, close, log: Optional[list] = None):
    """the closing of one group directly behind its repair: the meshes that have triangles go through ONE
    ``close_meshes_device`` call; every further per-vertex array (the normals) follows ``vmap`` -> the meshes.
    ``log``: a list that takes one report per mesh of the group, in mesh order (``postprocess.close_arrays``; a mesh
    without triangles stays as it is and reports zeros)"""
    from . import postprocess
    reports: dict = {}

    def call(picked, some):
        closed, reps = postprocess.close_meshes_device(some, close["orient"], close["fill"], close["outward"],
                                                       close["max_hole"])
        reports.update(zip(picked, reps))
        return [m[:-2] for m in closed]                       # without vmap and kept
    out = _through(meshes, close is not None, call)[0]
    if log is not None and close is not None:
        for b, m in enumerate(meshes):
            zeros = np.zeros(len(postprocess.CLOSE_FIELDS), np.int64)
            zeros[0] = len(m[0])
            log.append(reports.get(b) or postprocess.close_report(zeros, len(m[0]), len(m[1])))
    return out


MIRROR_AXES = {"x": 0, "y": 1, "z": 2, "0": 0, "1": 1, "2": 2, 0: 0, 1: 1, 2: 2}
COLOUR_DEFAULTS = {"S": 2, "rel_tol": 1e-3, "mirror_axis": None, "fill_iters": 32, "bgr": True}


def colour_args(colour) -> Optional[dict]:
    """``colour`` = None / False (off), True (the defaults) or a dict with some of S, rel_tol, mirror_axis (None, 0, 1,
    2 or "x", "y", "z"), fill_iters, bgr -> None or the checked, complete dict (ValueError; no device work): the keyword
    arguments ``reconstruct`` / ``reconstruct_fused`` hand to ``postprocess.colour_meshes_device``"""
    if colour is None or colour is False:
        return None
    from .postprocess import _colour_params
    given = {} if colour is True else dict(colour)
    unknown = sorted(set(given) - set(COLOUR_DEFAULTS))
    if unknown:
        raise ValueError("--colour takes S, rel_tol, mirror_axis, fill_iters and bgr, not %s" % ", ".join(unknown))
    c = dict(COLOUR_DEFAULTS, **given)
    if c["mirror_axis"] is not None:
        if isinstance(c["mirror_axis"], bool) or c["mirror_axis"] not in MIRROR_AXES:
            raise ValueError("--colour_mirror must be x, y or z (or 0, 1, 2), got %r" % (c["mirror_axis"],))
        c["mirror_axis"] = MIRROR_AXES[c["mirror_axis"]]
    _colour_params(c["S"], c["rel_tol"], c["mirror_axis"], c["fill_iters"])
    c["bgr"] = bool(c["bgr"])
    return c


def colour_group(meshes, colour, imgs, trans_mats, views_per_mesh: int = 1, alpha=None):
    """the colouring of one group behind every other stage: ONE ``colour_meshes_device`` call for the meshes that have
    vertices, mesh b from views b V .. (b + 1) V - 1 of ``imgs`` [B V,137,137,3] and ``trans_mats`` [B V,4,3] (V =
    ``views_per_mesh``; ``alpha`` None or [B V,137,137] uint8) -> the meshes, each with ``colours`` uint8 [nv,3] as its
    last element (empty for an empty mesh); vertices, faces and normals are not touched"""
    import torch

    from .postprocess import IMG, colour_meshes_device
    meshes = [tuple(m) for m in meshes]
    if colour is None:
        return meshes
    V = int(views_per_mesh)
    picked = [b for b, m in enumerate(meshes) if len(m[0])]
    out = [m + (torch.zeros((0, 3), dtype=torch.uint8, device=m[0].device),) for m in meshes]
    if not picked:
        return out
    dev = meshes[picked[0]][0].device
    on_dev = lambda a, dt: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a))).to(dev, dt)
    im = on_dev(imgs, torch.float32).reshape(len(meshes), V, IMG, IMG, 3)
    tm = trans_mats.detach().cpu().numpy() if isinstance(trans_mats, torch.Tensor) else trans_mats
    tm = np.asarray(tm, np.float32).reshape(len(meshes), V, 4, 3)
    al = None if alpha is None else on_dev(alpha, torch.uint8).reshape(len(meshes), V, IMG, IMG)
    idx = torch.as_tensor(picked, device=dev)
    whole = len(picked) == len(meshes)
    cs, _ = colour_meshes_device([meshes[b][:2] for b in picked], im if whole else im.index_select(0, idx), tm[picked],
                                 views_per_mesh=V, alpha=al if al is None or whole else al.index_select(0, idx),
                                 **colour)
    for b, c in zip(picked, cs):
        out[b] = meshes[b] + (c,)
    return out


CHECK_PAIRS_PER_FACE = 256     # postprocess.CHECK_PAIRS_PER_FACE (imported late there: this module loads without torch)
SCORE_POINTS = 2048
SCORE_CACHE = 8               # ground-truth objects whose samples stay on the device between groups


def score_args(score) -> Optional[Tuple[str, int]]:
    """``score`` = None (off), GT_DIR or (GT_DIR, points) -> None or the checked (gt_dir, points) (ValueError; no
    device work)"""
    if score is None:
        return None
    gt_dir, n = (score, SCORE_POINTS) if isinstance(score, str) else score
    if isinstance(n, bool) or int(n) != n or not 1 <= int(n) <= 1 << 20:
        raise ValueError("--score_points must be an integer in 1..%d, got %r" % (1 << 20, n))
    if not gt_dir:
        raise ValueError("--score needs the directory of the ground-truth meshes")
    return str(gt_dir), int(n)


def score_ground_truth(gt_dir: str, cat_id: str, obj: str, n: int, seed: int, device=None, log=None):
    """-> (points [n,3], normals [n,3], status): the surface samples of <gt_dir>/<cat_id>/<obj>/isosurf.obj as device
    tensors; status 6 (zeros: the mesh has no area) is reported through ``log``, any other is a ValueError"""
    from .evaluate import _device_mesh, _sampled
    pts, nrm, status = _sampled([_device_mesh(os.path.join(gt_dir, cat_id, obj, "isosurf.obj"), device)],
                                ["%s/%s/isosurf.obj" % (cat_id, obj)], n, seed, log)
    return pts[0], nrm[0], int(status[0])


def score_group(meshes, keys, score, seed: int = 0, cache: Optional[dict] = None, truethreshold: float = 2.5,
                log=None):
    """the scoring of one group behind every other stage: ONE ``sample_surface_meshes_device`` call for the meshes that
    have triangles, ONE ``surface_scores`` call against their objects' ground truth (``cache``: (cat_id, obj) -> its
    samples, filled here; it keeps every object of the group, however many, and beyond SCORE_CACHE objects drops
    those the group does not need) -> one dict per mesh, ``keys`` [(cat_id, obj, view)] in mesh order: the scores as
    floats and lists, "status" (None for a mesh without triangles, which is not scored) and "gt_status" (6: the ground
    truth has no area, the scores are against n points at the origin; ``log`` gets a line naming it).  The meshes are
    not touched."""
    import torch

    from . import metrics
    gt_dir, n = score
    cache = {} if cache is None else cache
    rows = [{"cat_id": c, "obj": o, "view": int(v), "points": n, "status": None} for c, o, v in keys]
    picked = [b for b, m in enumerate(meshes) if len(m[0]) and len(m[1])]
    if not picked:
        return rows
    dev = getattr(meshes[picked[0]][0], "device", None)
    need = dict.fromkeys(tuple(keys[b][:2]) for b in picked)
    if len(set(cache) | set(need)) > SCORE_CACHE:           # make room, but never at the cost of this group's objects
        for key in [k for k in cache if k not in need]:
            del cache[key]
    for c, o in need:
        if (c, o) not in cache:
            cache[(c, o)] = score_ground_truth(gt_dir, c, o, n, seed, dev, log)
    pts, nrm, _, status = metrics.sample_surface_meshes_device(
        [tuple(meshes[b][:2]) for b in picked], n,
        [metrics.mesh_seed(seed, os.path.basename(obj_path("", *keys[b]))) for b in picked])
    gt_pts = torch.stack([cache[tuple(keys[b][:2])][0] for b in picked])
    gt_nrm = torch.stack([cache[tuple(keys[b][:2])][1] for b in picked])
    thresholds = metrics.f_score_thresholds(truethreshold)
    scores = metrics.surface_scores(pts, nrm, gt_pts, gt_nrm, thresholds)
    status = np.asarray(status.cpu())
    for k, b in enumerate(picked):
        rows[b]["status"] = int(status[k])
        rows[b]["gt_status"] = int(cache[tuple(keys[b][:2])][2])
        if status[k] == 0:
            rows[b].update({name: float(scores[name][k]) for name in metrics.SURFACE_SCORES})
            rows[b].update({name: [float(x) for x in scores[name][k]] for name in ("precision", "recall", "f_score")})
            rows[b]["thresholds"] = [float(t) for t in thresholds]
    return rows


def dc_args(mesher: str = "mc", dc=None) -> Optional[dict]:
    """``mesher`` = "mc" (marching cubes, the default), "dc" (dual contouring, ``isosurface.dual_contour_batch``) or
    "dcs" (the same with one vertex per SHEET of a cell, ``sheets=True``: the checked dict then carries "sheets": True);
    ``dc`` = None, a regulariser REG, or a dict with any of ``normals`` ("network": the network's unit gradients at the
    Hermite points, the default; "grid": the grid's finite differences) and ``reg`` (0 < reg <= 1, default 2^-10 --
    the constant of the simplification, NOT measured on a trained network's normals).  -> None for "mc", else the
    checked dict (ValueError; no device work): what ``reconstruct*`` and ``--mesher`` take"""
    if mesher not in ("mc", "dc", "dcs"):
        raise ValueError("--mesher must be mc, dc or dcs, got %r" % (mesher,))
    if mesher == "mc":
        if dc is not None:
            raise ValueError("--dc_normals / --dc_reg need --mesher dc or dcs")
        return None
    from .isosurface import DC_REG
    d = {"normals": "network", "reg": DC_REG}
    if isinstance(dc, dict):
        if set(dc) - set(d) - {"sheets"}:
            raise ValueError("dc: unknown keys %s" % sorted(set(dc) - set(d) - {"sheets"}))
        if "sheets" in dc and bool(dc["sheets"]) != (mesher == "dcs"):       # a checked dict handed on: it must agree
            raise ValueError("dc: sheets = %r does not go with --mesher %s" % (dc["sheets"], mesher))
        d.update({k: v for k, v in dc.items() if v is not None and k != "sheets"})
    elif dc is not None:
        d["reg"] = dc
    if d["normals"] not in ("network", "grid"):
        raise ValueError("--dc_normals must be network or grid, got %r" % (d["normals"],))
    d["reg"] = float(d["reg"])
    if not (0.0 < d["reg"] <= 1.0):
        raise ValueError("--dc_reg must be in (0, 1], got %r" % (d["reg"],))
    if mesher == "dcs":
        d["sheets"] = True
    return d


def mesh_group(grids, sp, sdf_res: int, iso: float, dc=None, engine=None, enc=None, trans_mats=None):
    """the group's grids [B,(res+1)^3] -> B x (verts, faces): ``isosurface.marching_cubes_batch`` (``dc`` None), or
    ``isosurface.dual_contour_batch`` with the checked ``dc`` of ``dc_args``: the normals of view b are the network's
    unit gradients at its Hermite points from the view's cached folded map (``SdfEngine.refine_vertices(iters=0)``),
    or -- ``normals`` = "grid", or no ``enc`` (the fused route has no gradient entry) -- the grid normals; with
    "sheets" in ``dc`` (``mesher`` = "dcs") one vertex per sheet of a cell"""
    from . import isosurface
    if dc is None:
        return isosurface.marching_cubes_batch(grids, sp, sdf_res, iso)
    fn = None
    if dc["normals"] == "network" and enc is not None:
        def fn(b, points):
            return engine.refine_vertices(enc, b, trans_mats, points, iso=iso, iters=0)[1]
    return isosurface.dual_contour_batch(grids, sp, sdf_res, iso, fn, dc["reg"], sheets=bool(dc.get("sheets")))


def reconstruct(engine, imgs, trans_mats, sdf_params, sdf_res: int, iso: float = 0.0, refine: int = 0,
                normals: bool = False, band=None, clean=None, simplify=None, colour=None, alpha=None, smooth=None,
                mesher: str = "mc", dc=None, repair=None, repair_log=None, close=None, close_log=None):
    """``reconstruct_select`` for callers that clean every mesh or none (see there); -> the meshes"""
    return reconstruct_select(engine, imgs, trans_mats, sdf_params, sdf_res, iso, refine, normals, band, clean,
                              simplify=simplify, colour=colour, alpha=alpha, smooth=smooth, mesher=mesher, dc=dc,
                              repair=repair, repair_log=repair_log, close=close, close_log=close_log)[0]


def _mesh_stages(engine, enc, imgs, trans_mats, grids, sp, sdf_res: int, iso: float, views_per_mesh: int, clean,
                 simplify, smooth, colour, dc, refine: int = 0, normals: bool = False, select=None,
                 strict: bool = True, alpha=None, repair=None, repair_log=None, close=None, close_log=None):
    """THE stage chain of ``reconstruct_select`` and ``reconstruct_fused_select``: the group's grids [M,(res+1)^3] with
    their boxes ``sp`` [M,6] -> (M meshes, unclean [M] bool).  The stage values are the CHECKED ones of the ``*_args``
    functions (None: the stage is off and makes no device call); mesh m belongs to views m V .. (m + 1) V - 1 of
    ``imgs`` / ``trans_mats`` / ``alpha`` (V = ``views_per_mesh``).  The order, and what every stage sees:
      1. ``mesh_group``: the grids -> (verts, faces) per mesh, marching cubes or (``dc``) dual contouring -- with the
         network's normals from ``enc``, with the grid's when ``enc`` is None (the fused route);
      2. ``clean_group``: the meshes as they were meshed, so the rule sees the vertices the reference's rule sees and
         a dropped part is never simplified, smoothed or refined; only the meshes ``select`` marks;
      3. ``simplify_group``: the cleaned meshes, each on the lattice of its own box;
      4. ``smooth_group``: the cleaned, simplified meshes, each with the cap of its own box;
      5. ``isosurface.refine_mesh`` mesh by mesh, when ``refine`` > 0 or ``normals`` (needs ``enc``: V = 1): the Newton
         steps pull the moved vertices back onto the network's level set, the normals are the gradients at the final
         vertices;
      5b. ``repair_group``: the smoothed, refined meshes are welded, stitched and split to a manifold.  It stands HERE
         because smoothing or refining the copies of one position could pull them apart: behind those stages the copies
         stay coincident, the normals follow their vertices, and the colours and a driver's ``--check`` see the repaired
         mesh (``repair_log``: see ``repair_group``);
      5c. ``close_group``: the repaired meshes are oriented consistently and their holes filled, directly behind the
         repair (whose output is what the closing's rule asks for) and before the colours, so that a centre is coloured
         like any vertex and a driver's ``--check`` sees the closed mesh; a centre's normal is that of its loop's
         smallest vertex (``close_log``: see ``close_group``);
      6. ``colour_group``: the final meshes; vertices, faces and normals are not touched.
    Faces change in stages 2, 3 and 5b, and 5c flips faces and adds new ones behind them."""
    from . import isosurface
    meshes = mesh_group(grids, sp, sdf_res, iso, dc, engine, enc, trans_mats)
    meshes, unclean = clean_group(meshes, clean, select, strict)
    meshes = smooth_group(simplify_group(meshes, simplify, sp), smooth, sp, sdf_res)
    if refine > 0 or normals:
        meshes = [tuple(isosurface.refine_mesh(engine, enc, b, trans_mats, verts, faces, sp[b], sdf_res, iso,
                                               max(int(refine), 0))[:3 if normals else 2])
                  for b, (verts, faces) in enumerate(meshes)]
    meshes = close_group(repair_group(meshes, repair, repair_log), close, close_log)
    if colour is not None:
        meshes = colour_group(meshes, colour, imgs, trans_mats, views_per_mesh, alpha)
    return meshes, unclean


def reconstruct_select(engine, imgs, trans_mats, sdf_params, sdf_res: int, iso: float = 0.0, refine: int = 0,
                       normals: bool = False, band=None, clean=None, select=None, strict: bool = True,
                       simplify=None, colour=None, alpha=None, smooth=None, mesher: str = "mc", dc=None, repair=None,
                       repair_log=None, close=None, close_log=None):
    """images -> meshes for one group of views: one ``engine.encode`` call, the per-image grids of
    ``create_sdf`` in one [B,(res+1)^3] tensor, ONE batched meshing (one host sync for the group).
    -> B x (verts [nv,3] float32, faces [nf,3] int32) device views; the bits are those of ``create_sdf``
    followed by ``isosurface.marching_cubes`` image by image.
    The stages behind the meshing, all off by default, run in the order of ``_mesh_stages`` (see there for what each
    one sees), whatever the order of the arguments:
    ``refine`` > 0: every view's vertices take that many Newton steps onto the network's iso level set
    (``isosurface.refine_mesh``, from the view's cached folded map); ``normals``: every mesh is a triple
    (verts, faces, normals [nv,3]) with the unit gradient at its (refined) vertices.  Faces never change.
    ``band`` = (stride, margin, dilate): the grids come from the narrow-band evaluation (one more host sync for the
    group: the band sizes); the bits are those of ``engine.query_grid_band`` and ``marching_cubes`` image by image.
    ``clean`` = (dist_thresh, num_thresh, connectivity): the small and the far parts are dropped on the device
    (``clean_group``: one more host sync for the group, the cleaned sizes); the bits are those of
    ``postprocess.clean_arrays`` on the uncleaned mesh.  ``select`` [B] bool: only those meshes are cleaned.
    A mesh of which nothing is kept raises ValueError (``strict``; False: it stays uncleaned).
    ``simplify`` = CELLS: every mesh with triangles is simplified on the lattice of CELLS cells along the longest side
    of its view's ``sdf_params`` box (``simplify_group``: one more host sync for the group, the simplified sizes); the
    bits are those of ``postprocess.simplify_arrays`` on the (cleaned) mesh.
    ``smooth`` = ITERS or a dict (``smooth_args``): every mesh with triangles is faired by Taubin smoothing
    (``smooth_group``: one more host sync for the group, the status words), no coordinate further than ``cap`` grid
    cells of its view's box from where it was; the bits are those of ``postprocess.smooth_arrays`` on the (cleaned,
    simplified) mesh.  Faces never change.
    ``colour`` = True or a dict (``colour_args``): each mesh is coloured from its own view (``colour_group``; ``alpha``
    None or [B,137,137] uint8 masks the background) and gains ``colours`` uint8 [nv,3] as its last element: (verts,
    faces[, normals], colours).  Vertices, faces and normals are bit for bit those of the call without it; the bytes
    are those of ``postprocess.colour_arrays`` on the final mesh.
    ``mesher`` = "dc" (``dc``: see ``dc_args``): the grids, dense or banded, go through dual contouring instead of
    marching cubes (``mesh_group``: one vertex per crossed cell placed by a quadric from the network's gradients at
    the cut edges, so creases survive; the mesh can be non-manifold where a cell holds several sheets); every later
    stage sees a (verts, faces) pair as before.  The bits are those of ``isosurface.dual_contour_batch`` on the grids.
    ``repair`` = True or a dict (``repair_args``): every mesh with triangles is welded, stitched and split to a manifold
    behind the smoothing and the refinement (``repair_group``: one more host sync for the group, the repaired sizes); the
    integers and the position bits are those of ``postprocess.repair_arrays`` on the mesh of the call without it, the
    normals follow their vertices, the colours are those of the repaired mesh.  ``repair_log``: a list that takes one
    report per mesh.
    ``close`` = True or a dict (``close_args``): every mesh with triangles is oriented consistently and its holes are
    filled directly behind the repair (``close_group``: one more host sync for the group, the closed sizes); the integers
    and the position bits are those of ``postprocess.close_arrays`` on the mesh of the call without it; a mesh that is
    not manifold raises ValueError (``repair`` comes first).  ``close_log``: a list that takes one report per mesh.
    -> (meshes, unclean [B] bool)"""
    band = band_args(band, sdf_res)
    clean, simplify, colour, smooth = clean_args(clean), simplify_args(simplify), colour_args(colour), smooth_args(smooth)
    dc, repair, close = dc_args(mesher, dc), repair_args(repair), close_args(close)
    if band is None:
        enc, grids = _encode_grids(engine, imgs, trans_mats, sdf_params, sdf_res)
    else:
        enc, grids, _ = _encode_grids_band(engine, imgs, trans_mats, sdf_params, sdf_res, iso, band)
    sp = np.asarray(sdf_params, dtype=np.float64).reshape(grids.shape[0], 6)
    return _mesh_stages(engine, enc, imgs, trans_mats, grids, sp, sdf_res, iso, 1, clean, simplify, smooth, colour, dc,
                        refine, normals, select, strict, alpha, repair, repair_log, close, close_log)


def fuse_args(fuse, pool: str = "max") -> Optional[Tuple[int, str]]:
    """``fuse`` = None / 0 (off) or the number of views fused into one mesh -> None or the checked (V, pool)
    (ValueError; no device work): what ``reconstruct_fused`` and ``--fuse_views`` take"""
    if not fuse:
        return None
    V = int(fuse)
    if V == 1:
        raise ValueError("--fuse_views 1 fuses nothing: use the normal path")
    if not 2 <= V <= 24:
        raise ValueError("--fuse_views must be in 2..24, got %d" % V)
    if pool not in ("max", "mean"):
        raise ValueError("--fuse_pool must be max or mean, got %r" % (pool,))
    return V, pool


def reconstruct_fused(engine, imgs, trans_mats, sdf_params, sdf_res: int, iso: float = 0.0, fuse: int = 2,
                      pool: str = "max", clean=None, simplify=None, colour=None, alpha=None, smooth=None,
                      mesher: str = "mc", dc=None, repair=None, repair_log=None, close=None, close_log=None):
    """``reconstruct_fused_select`` for callers that clean every mesh or none (see there); -> the meshes"""
    return reconstruct_fused_select(engine, imgs, trans_mats, sdf_params, sdf_res, iso, fuse, pool, clean,
                                    simplify=simplify, colour=colour, alpha=alpha, smooth=smooth, mesher=mesher,
                                    dc=dc, repair=repair, repair_log=repair_log, close=close,
                                    close_log=close_log)[0]


def reconstruct_fused_select(engine, imgs, trans_mats, sdf_params, sdf_res: int, iso: float = 0.0, fuse: int = 2,
                             pool: str = "max", clean=None, select=None, strict: bool = True, simplify=None,
                             colour=None, alpha=None, smooth=None, mesher: str = "mc", dc=None, repair=None,
                             repair_log=None, close=None, close_log=None):
    """multi-view ``reconstruct``: the B images are B / ``fuse`` runs of ``fuse`` consecutive views of one object each
    (cameras trans_mats [B,4,3] in the object's frame, the run's grid box = its first view's sdf_params).  One
    ``engine.encode`` call, one ``engine.query_grid_views`` grid per run (features pooled over the run's views,
    ``pool`` = "max" or "mean"), ONE batched meshing -> B / fuse x (verts, faces); a run's bits are those of
    ``query_grid_views`` followed by ``isosurface.marching_cubes`` on that run alone.  The stages behind the meshing
    run in the order of ``_mesh_stages``: ``clean``, ``select`` (one entry per RUN), ``strict``, ``simplify`` (on the
    lattice of the run's box) and ``smooth`` (the cap in cells of the run's box) as in ``reconstruct_select``;
    ``colour``: every run's mesh is coloured from ALL ``fuse`` views of the run (``alpha`` None or [B,137,137]).
    ``mesher`` = "dc": dual contouring with the GRID normals whatever ``dc`` asks for (this route has no gradient entry,
    and so no ``refine`` and no ``normals``).  ``repair``, ``repair_log``, ``close``, ``close_log``: as in
    ``reconstruct_select``.
    -> (meshes, unclean [B / fuse] bool)"""
    import torch
    checked = fuse_args(fuse, pool)
    if checked is None:
        raise ValueError("reconstruct_fused needs the number of views to fuse")
    V, pool = checked
    clean, simplify, colour, smooth = clean_args(clean), simplify_args(simplify), colour_args(colour), smooth_args(smooth)
    dc, repair, close = dc_args(mesher, dc), repair_args(repair), close_args(close)
    imgs = np.asarray(imgs, np.float32) if not isinstance(imgs, torch.Tensor) else imgs
    B = imgs.shape[0]
    if B % V:
        raise ValueError("%d images are no whole number of runs of %d views" % (B, V))
    tm = np.asarray(trans_mats, np.float32).reshape(B, 4, 3) if not isinstance(trans_mats, torch.Tensor) \
        else trans_mats.reshape(B, 4, 3)
    sp = np.asarray(sdf_params, dtype=np.float64).reshape(B, 6)[::V]
    enc = engine.encode(imgs)
    grids = torch.empty((B // V, (sdf_res + 1) ** 3), dtype=torch.float32, device=engine.device)
    for r in range(B // V):
        engine.query_grid_views(enc, (r * V, V), tm[r * V:(r + 1) * V], sp[r], sdf_res, pool, out=grids[r])
    return _mesh_stages(engine, None, imgs, tm, grids, sp, sdf_res, iso, V, clean, simplify, smooth, colour, dc,
                        select=select, strict=strict, alpha=alpha, repair=repair, repair_log=repair_log, close=close,
                        close_log=close_log)


def fuse_runs(entries: Sequence, fuse: int) -> List[List]:
    """the listed views in runs of ``fuse`` consecutive entries, each run the views of ONE object (ValueError
    otherwise: ``view_num`` must be a multiple of ``fuse``)"""
    if len(entries) % fuse:
        raise ValueError("%d views are no whole number of runs of %d" % (len(entries), fuse))
    runs = [list(entries[i:i + fuse]) for i in range(0, len(entries), fuse)]
    for run in runs:
        if any(e[:2] != run[0][:2] for e in run):
            raise ValueError("a run of %d views spans two objects: %s" % (fuse, run))
    return runs


# ---- the test-set driver ---------------------------------------------------------------------------
MIN_OBJ_BYTES = 200          # evaluate.build_file_dict(min_size=200) / test_iou.py:124
MAX_WRITERS = 16


def sample_list(cats: Dict[str, str], test_lst_dir: str, view_num: int = 24, seed: int = 0,
                num_shards: int = 1, shard_id: int = 0, all_views: int = 24) -> List[Tuple[str, str, int]]:
    """(cat_id, obj, view) of the run: categories in the order of ``evaluate.CATS_ALL``, objects in list-file
    order, ``sorted(sample(range(24), view_num))`` per object from one ``random.Random(seed)``; then the shard's
    objects ``objects[shard_id::num_shards]`` with all their views"""
    from .evaluate import CATS_ALL, read_list
    if not 1 <= view_num <= all_views:
        raise ValueError("--view_num must be in 1..%d, got %d" % (all_views, view_num))
    if num_shards < 1 or not 0 <= shard_id < num_shards:
        raise ValueError("--shard_id must be in 0..num_shards-1, got %d of %d" % (shard_id, num_shards))
    rng = random.Random(seed)
    objects = []
    for cat_nm in CATS_ALL:
        if cat_nm not in cats:
            continue
        cat_id = cats[cat_nm]
        for obj in read_list(os.path.join(test_lst_dir, cat_id + "_test.lst")):
            objects.append((cat_id, obj.strip(), sorted(rng.sample(range(all_views), view_num))))
    return [(cat_id, obj, v) for cat_id, obj, views in objects[shard_id::num_shards] for v in views]


def groups(entries: Sequence, batch_size: int) -> List[List]:
    """consecutive runs of ``batch_size`` entries; the last one is shorter, nothing is dropped"""
    if batch_size < 1:
        raise ValueError("--batch_size must be positive")
    return [list(entries[i:i + batch_size]) for i in range(0, len(entries), batch_size)]


def result_obj_path(log_dir: str, sdf_res: int, iso: float, cam_est: bool = False, fuse=None,
                    clean: bool = False, simplify=None, colour: bool = False, smooth=None, mesher: str = "mc",
                    repair: bool = False, close: bool = False) -> str:
    """test/create_sdf.py:88-93: <log_dir>/test_objs/[camest_]<res+1>_<str(iso)>; ``fuse`` = (V, pool): the fused
    meshes' own directory [camest_]fuse<V><pool>_<res+1>_<str(iso)>; ``clean``: the tree with the cleaned categories,
    <...>_comb (the name INTEGRATION 3e gives the combined tree); ``simplify`` = CELLS: the simplified meshes' tree,
    <...>[_comb]_s<CELLS>; ``colour``: the coloured meshes' tree, <...>[_comb][_s<CELLS>]_col; ``smooth`` = ITERS: the
    smoothed meshes' tree, _t<ITERS> between _comb and _s<CELLS>: <...>[_comb]_t<ITERS>[_s<CELLS>][_col];
    ``mesher`` = "dc" / "dcs": the dual-contoured meshes' tree, _dc / _dcs directly behind <res+1>_<str(iso)>;
    ``repair``: the repaired meshes' tree, _rep in front of _col: <...>[_s<CELLS>]_rep[_col]; ``close``: the closed
    meshes' tree, _cls behind _rep: <...>[_rep]_cls[_col]"""
    prefix = ("camest_" if cam_est else "") + ("fuse%d%s_" % tuple(fuse) if fuse else "")
    return os.path.join(log_dir, "test_objs", prefix + str(sdf_res + 1) + "_" + str(iso)
                        + ("_" + mesher if mesher in ("dc", "dcs") else "") + ("_comb" if clean else "")
                        + ("_t%d" % smooth if smooth is not None else "")
                        + ("_s%d" % simplify if simplify is not None else "") + ("_rep" if repair else "")
                        + ("_cls" if close else "") + ("_col" if colour else ""))


def obj_path(out_dir: str, cat_id: str, obj: str, view: int) -> str:
    return os.path.join(out_dir, cat_id, "%s_%s_%02d.obj" % (cat_id, obj, view))


def pending(entries: Sequence, out_dir: str) -> List:
    """--skip_existing: the entries whose file is missing or holds at most MIN_OBJ_BYTES bytes"""
    def done(e):
        p = obj_path(out_dir, *e)
        return os.path.isfile(p) and os.stat(p).st_size > MIN_OBJ_BYTES
    return [e for e in entries if not done(e)]


def parser():
    import argparse
    p = argparse.ArgumentParser(prog="python -m disn_amd.create_sdf",
                                description="meshes of the test set (test/create_sdf.py --create_obj)")
    p.add_argument("--log_dir", default="checkpoint/exp_200", help="checkpoint directory; results go below it")
    p.add_argument("--test_lst_dir", required=True, help="object lists (<cat_id>_test.lst)")
    p.add_argument("--category", default="all", help="all, or category names separated by commas [default: all]")
    p.add_argument("--sdf_res", type=int, default=64, help="cells per axis of the grid [default: 64]")
    p.add_argument("--iso", type=float, default=0.0, help="iso value [default: 0.0]")
    p.add_argument("--view_num", type=int, default=24, help="views per object [default: 24]")
    p.add_argument("--batch_size", type=int, default=None, help="images per encode call [default: view_num]")
    p.add_argument("--cam_est", action="store_true", help="--rendered_dir holds the estimated cameras "
                                                          "(what train_cam --create wrote)")
    p.add_argument("--backcolorwhite", action="store_true")
    for flag in ("binary", "threedcnn", "img_feat_onestream", "multi_view", "alpha"):
        p.add_argument("--" + flag, action="store_true", help="not supported")
    p.add_argument("--img_feat_twostream", action="store_true", help="the one supported mode (implied)")
    # storage of this implementation (the reference takes them from its info.json)
    p.add_argument("--sdf_dir", default="")
    p.add_argument("--rendered_dir", default="")
    p.add_argument("--seed", type=int, default=0, help="seed of the view choice [default: 0]")
    p.add_argument("--random_init", type=int, default=None, metavar="SEED",
                   help="run on freshly initialised weights when log_dir holds no complete checkpoint")
    p.add_argument("--strict", action="store_true", help="single-image kernel forms for every call size: a view's "
                                                         "mesh does not depend on the group it was encoded in")
    p.add_argument("--skip_existing", action="store_true", help="leave out views whose .obj exists (> 200 bytes)")
    p.add_argument("--writers", type=int, default=4, help="writer threads, at most %d [default: 4]" % MAX_WRITERS)
    p.add_argument("--num_shards", type=int, default=1)
    p.add_argument("--shard_id", type=int, default=0)
    p.add_argument("--refine", type=int, default=0, metavar="ITERS",
                   help="Newton steps that move every vertex onto the network's iso level set [default: 0, none]")
    p.add_argument("--normals", action="store_true", help="write the unit SDF gradient at every vertex as 'vn' lines")
    p.add_argument("--fuse_views", type=int, default=0, metavar="V",
                   help="multi-view: fuse every run of V chosen views of an object into ONE mesh (features pooled "
                        "over the views); view_num and batch_size must be multiples of V [default: 0, one mesh per view]")
    p.add_argument("--fuse_pool", default="max", choices=("max", "mean"), help="how --fuse_views pools [default: max]")
    p.add_argument("--clean", default=None, metavar="CATS",
                   help="drop the small and the far parts of the meshes of these categories on the device: clean (the "
                        "reference's five), all, or names separated by commas; results go to <...>_comb")
    add_stage_flags(p)
    add_score_flags(p)
    add_check_flags(p)
    add_repair_flags(p)
    add_close_flags(p)
    return p


def add_stage_flags(p) -> None:
    """the flags of the stages that both command lines share; ``--clean`` itself stays with each parser (categories
    here, a switch in the demo)"""
    for add in (add_band_flags, add_clean_flags, add_simplify_flag, add_smooth_flags, add_colour_flags, add_dc_flags):
        add(p)


def stages_from_flags(a, clean_on: bool) -> dict:
    """the checked stage values of a command line, as ``reconstruct_select`` takes them: every key always there, None
    for a stage that is off (ValueError for a bad value or an option whose stage is off; no device work)"""
    return {"band": band_from_flags(a), "clean": clean_from_flags(a, clean_on), "simplify": simplify_from_flags(a),
            "smooth": smooth_from_flags(a), "colour": colour_from_flags(a), "mesher": a.mesher, "dc": dc_from_flags(a)}


def write_mesh(path: str, mesh, coloured: bool) -> str:
    """(verts, faces[, normals][, colours]) -> the .obj at ``path``; ``coloured``: the last element is the colours"""
    from . import isosurface
    verts, faces, *extras = mesh
    if coloured:
        isosurface.write_obj(path, verts, faces, *extras[:-1], colours=extras[-1])
    else:
        isosurface.write_obj(path, verts, faces, *extras)
    return path


def add_dc_flags(p) -> None:
    p.add_argument("--mesher", default="mc", choices=("mc", "dc", "dcs"),
                   help="mc: marching cubes; dc: dual contouring from Hermite data (one vertex per crossed cell, placed "
                        "by a quadric: keeps creases; can be non-manifold where a cell holds several sheets); dcs: the "
                        "same with one vertex per sheet of a cell (thin parts stay apart); results go to <...>_dc / "
                        "<...>_dcs [default: mc]")
    p.add_argument("--dc_normals", default=None, choices=("network", "grid"),
                   help="with --mesher dc or dcs: the network's gradients at the cut edges, or the grid's finite differences "
                        "(always grid with --fuse_views) [default: network]")
    p.add_argument("--dc_reg", type=float, default=None, metavar="REG",
                   help="with --mesher dc or dcs: the pull towards the mean of a cell's crossings, 0 < REG <= 1 [default: "
                        "2^-10, the simplification's constant; not measured on a trained network]")


def dc_from_flags(a) -> Optional[dict]:
    """None without --mesher dc or dcs (ValueError for --dc_normals / --dc_reg without it), else the checked dict of
    ``dc_args``"""
    dc = {"normals": a.dc_normals, "reg": a.dc_reg}
    return dc_args(a.mesher, None if a.dc_normals is None and a.dc_reg is None else dc)


def add_smooth_flags(p) -> None:
    p.add_argument("--smooth", type=int, default=None, metavar="ITERS",
                   help="fair every mesh on the device by ITERS (1..64) iterations of Taubin's lambda|mu smoothing, "
                        "behind --simplify and before --refine; results go to <...>_t<ITERS>")
    p.add_argument("--smooth_cap", type=float, default=None, metavar="CELLS",
                   help="with --smooth: no coordinate moves further than CELLS grid cells of the view's box "
                        "[default: %g]" % SMOOTH_CAP_CELLS)
    p.add_argument("--smooth_free_boundary", action="store_true",
                   help="with --smooth: boundary vertices move too [default: they stay where they are]")


def smooth_from_flags(a) -> Optional[dict]:
    """None without --smooth, else the checked dict of ``smooth_args`` (ValueError for --smooth_cap or
    --smooth_free_boundary without --smooth, iterations outside 1..64, a cap that is negative or not finite)"""
    if a.smooth is None:
        for flag in ("smooth_cap", "smooth_free_boundary"):
            if getattr(a, flag) not in (None, False):
                raise ValueError("--%s needs --smooth" % flag)
        return None
    return smooth_args({"iters": a.smooth, "cap": SMOOTH_CAP_CELLS if a.smooth_cap is None else a.smooth_cap,
                        "pin_boundary": not a.smooth_free_boundary})


def add_score_flags(p) -> None:
    p.add_argument("--score", default=None, metavar="GT_DIR",
                   help="score every final mesh on the device, on area-weighted surface samples, against "
                        "GT_DIR/<cat_id>/<obj>/isosurf.obj; one JSON line per mesh in <out_dir>/scores.jsonl")
    p.add_argument("--score_points", type=int, default=None, metavar="N",
                   help="with --score: surface samples per mesh, 1..1048576 [default: %d]" % SCORE_POINTS)


def score_from_flags(a) -> Optional[Tuple[str, int]]:
    """None without --score, else the checked (gt_dir, points) (ValueError for --score_points without --score or
    outside its range)"""
    if a.score is None:
        if a.score_points is not None:
            raise ValueError("--score_points needs --score")
        return None
    return score_args((a.score, SCORE_POINTS if a.score_points is None else a.score_points))


def add_repair_flags(p) -> None:
    p.add_argument("--repair", action="store_true",
                   help="weld, stitch and split every mesh to a manifold on the device, behind the smoothing and the "
                        "refinement; results go to <...>_rep, one JSON line per mesh to <out_dir>/repairs.jsonl")
    p.add_argument("--repair_no_weld", action="store_true", help="with --repair: do not merge coincident vertices")
    p.add_argument("--repair_no_stitch", action="store_true",
                   help="with --repair: cut every singular edge instead of pairing its faces by angle")


def repair_from_flags(a) -> Optional[dict]:
    """None without --repair, else the checked dict of ``repair_args`` (ValueError for --repair_no_weld or
    --repair_no_stitch without --repair)"""
    if not a.repair:
        for flag in ("repair_no_weld", "repair_no_stitch"):
            if getattr(a, flag):
                raise ValueError("--%s needs --repair" % flag)
        return None
    return repair_args({"weld": not a.repair_no_weld, "stitch": not a.repair_no_stitch})


def add_close_flags(p) -> None:
    p.add_argument("--close", action="store_true",
                   help="orient every mesh consistently and fill its holes on the device, directly behind --repair; "
                        "results go to <...>_cls, one JSON line per mesh to <out_dir>/closes.jsonl")
    p.add_argument("--close_no_orient", action="store_true", help="with --close: leave every face's orientation")
    p.add_argument("--close_no_fill", action="store_true", help="with --close: fill no hole")
    p.add_argument("--close_outward", action="store_true",
                   help="with --close: turn every closed component so that its volume is positive (wrong for cavities)")
    p.add_argument("--close_max_hole", type=int, default=None, metavar="N",
                   help="with --close: fill only the holes of at most N boundary edges (default and limit 2^22)")


def close_from_flags(a) -> Optional[dict]:
    """None without --close, else the checked dict of ``close_args`` (ValueError for a --close_* flag without --close)"""
    if not a.close:
        for flag in ("close_no_orient", "close_no_fill", "close_outward"):
            if getattr(a, flag):
                raise ValueError("--%s needs --close" % flag)
        if a.close_max_hole is not None:
            raise ValueError("--close_max_hole needs --close")
        return None
    return close_args({"orient": not a.close_no_orient, "fill": not a.close_no_fill, "outward": a.close_outward,
                       "max_hole": a.close_max_hole})


def add_check_flags(p) -> None:
    p.add_argument("--check", action="store_true",
                   help="check every final mesh on the device: topology, orientation, self-intersections; one JSON "
                        "line per mesh in <out_dir>/checks.jsonl")
    p.add_argument("--check_pairs", type=int, default=None, metavar="N",
                   help="with --check: the work cap, candidate pairs per face [default: %d]" % CHECK_PAIRS_PER_FACE)


def check_from_flags(a) -> Optional[int]:
    """None without --check, else the checked pairs per face (ValueError for --check_pairs without --check or a
    negative one)"""
    if not a.check:
        if a.check_pairs is not None:
            raise ValueError("--check_pairs needs --check")
        return None
    n = CHECK_PAIRS_PER_FACE if a.check_pairs is None else a.check_pairs
    if n < 0:
        raise ValueError("--check_pairs must not be negative, got %r" % (n,))
    return int(n)


def check_group(meshes, keys, pairs_per_face: int, check_fn: Optional[Callable] = None) -> List[dict]:
    """the FINAL meshes of one group, where ``reconstruct`` left them: ONE ``postprocess.check_meshes_device`` call (or
    ``check_fn(meshes, max_pairs)`` in its place, for host-side tests of the drivers) -> one dict per mesh, ``keys``
    [(cat_id, obj, view)] in mesh order: "cat", "obj", "view", then the dict of ``postprocess.check_arrays``.  The cap
    of a mesh is ``pairs_per_face`` nf + 4096.  No mesh raises: its status is in its line."""
    from . import postprocess
    pairs = [(m[0], m[1]) for m in meshes]
    caps = [pairs_per_face * int(m[1].shape[0]) + postprocess.CHECK_PAIRS_BASE for m in pairs]
    if check_fn is None:
        results = postprocess.check_meshes_device(pairs, max_pairs=caps, strict=False) if pairs else []
    else:
        results = check_fn(pairs, caps)
    rows = []
    for (c, o, v), r in zip(keys, results):
        row = {"cat": c, "obj": o, "view": v}
        row.update(r)
        rows.append(row)
    return rows


def add_colour_flags(p) -> None:
    p.add_argument("--colour", "--color", dest="colour", action="store_true",
                   help="colour every mesh's vertices on the device from the view(s) it was reconstructed from "
                        "('v x y z r g b' lines); results go to <...>_col")
    p.add_argument("--colour_mirror", "--color_mirror", dest="colour_mirror", default=None, metavar="AXIS",
                   help="with --colour: a vertex no view sees takes the colour of its reflection in the plane AXIS = 0 "
                        "(x, y or z) of the object frame when that is seen [default: off]")


def colour_from_flags(a) -> Optional[dict]:
    """None without --colour, else the checked keyword arguments (ValueError for --colour_mirror without --colour or
    with an axis that is none)"""
    if not a.colour:
        if a.colour_mirror is not None:
            raise ValueError("--colour_mirror needs --colour")
        return None
    return colour_args(True if a.colour_mirror is None else {"mirror_axis": a.colour_mirror})


def add_simplify_flag(p) -> None:
    p.add_argument("--simplify", type=int, default=None, metavar="CELLS",
                   help="simplify every mesh on the device: cluster its vertices on a lattice of CELLS cells (1..1024) "
                        "along the box's longest side, one quadric-placed vertex per cell; results go to <...>_s<CELLS>")


def simplify_from_flags(a) -> Optional[int]:
    """None without --simplify, else the checked number of cells (ValueError outside 1..1024)"""
    return simplify_args(a.simplify)


def add_clean_flags(p) -> None:
    p.add_argument("--clean_dist_thresh", type=float, default=None,
                   help="largest centroid distance of a kept part [default: 0.5]")
    p.add_argument("--clean_num_thresh", type=float, default=None,
                   help="smallest share of the largest part's vertices [default: 0.3]")
    p.add_argument("--clean_connectivity", default=None, help="face or vertex [default: face]")


def clean_from_flags(a, on: bool) -> Optional[Tuple[float, float, str]]:
    """the checked (dist_thresh, num_thresh, connectivity) when cleaning is ``on``; ValueError for a --clean_* option
    without it, a negative threshold or an unknown connectivity"""
    given = [f for f in ("clean_dist_thresh", "clean_num_thresh", "clean_connectivity") if getattr(a, f) is not None]
    if not on:
        if given:
            raise ValueError("--%s needs --clean" % given[0])
        return None
    return clean_args((0.5 if a.clean_dist_thresh is None else a.clean_dist_thresh,
                       0.3 if a.clean_num_thresh is None else a.clean_num_thresh,
                       a.clean_connectivity or "face"))


def clean_cats_from_flags(a):
    """None without --clean, else ((dist_thresh, num_thresh, connectivity), the set of category ids to clean)"""
    from .evaluate import categories
    clean = clean_from_flags(a, a.clean is not None)
    if clean is None:
        return None
    return clean, set(categories(a.clean).values())      # ValueError for an unknown category


def fuse_from_flags(a) -> Optional[Tuple[int, str]]:
    """None without --fuse_views, else the checked (V, pool): ValueError for V = 1, a view_num or batch_size that is
    no multiple of V, or a combination with --band / --refine / --normals (those read ONE image's folded map)"""
    fuse = fuse_args(a.fuse_views, a.fuse_pool)
    if fuse is None:
        return None
    V = fuse[0]
    if a.view_num % V:
        raise ValueError("--view_num %d is no multiple of --fuse_views %d" % (a.view_num, V))
    batch_size = a.view_num if a.batch_size is None else a.batch_size
    if batch_size < V or batch_size % V:
        raise ValueError("--batch_size %d is no multiple of --fuse_views %d" % (batch_size, V))
    for flag, on in (("--band", a.band != 0), ("--refine", a.refine > 0), ("--normals", a.normals)):
        if on:
            raise ValueError("--fuse_views cannot be combined with %s: that path reads one image's folded feature "
                             "map, and max pooling has none" % flag)
    return fuse


def check_flags(a) -> Optional[Tuple[int, str]]:
    """every flag rule, before any list, checkpoint or device is touched -> the checked --fuse_views (V, pool) or None"""
    from . import model_normalization as model
    F = model._flags(a)
    F.img_feat_twostream = True
    model._check_supported(F)
    if not 1 <= a.writers <= MAX_WRITERS:
        raise ValueError("--writers must be in 1..%d, got %d" % (MAX_WRITERS, a.writers))
    if a.sdf_res < 1:
        raise ValueError("--sdf_res must be positive")
    if a.refine < 0:
        raise ValueError("--refine must not be negative")
    stages_from_flags(a, a.clean is not None)
    clean_cats_from_flags(a)                     # (an unknown category)
    score_from_flags(a)
    check_from_flags(a)
    repair_from_flags(a)
    close_from_flags(a)
    return fuse_from_flags(a)


def restore_weights(log_dir: str, random_init: Optional[int]):
    """``WeightStore.restore_latest``; absent or incomplete -> error, or ``--random_init SEED``'s weights"""
    from .weights import WeightStore
    store = WeightStore.restore_latest(log_dir) if os.path.isdir(log_dir) else None
    if store is not None and store.complete():
        return store, "restored from %s" % log_dir
    what = "no checkpoint" if store is None else "an incomplete checkpoint (%d of %d variables)" % (
        len(store.arrays), len(store.shapes))
    if random_init is None:
        raise FileNotFoundError("%s holds %s; give --random_init SEED to run on initialised weights" % (log_dir, what))
    return WeightStore.random_init(random_init), "%s holds %s: random init, seed %d" % (log_dir, what, random_init)


def load_group(group: Sequence, sdf_dir: str, rendered_dir: str, backcolorwhite: bool = False,
               num_sample_points: int = 1, rot: bool = False, seed: Optional[int] = None) -> dict:
    """the loader's batch dictionary (data_sdf.Pt_sdf_img, shuffle=False) for one group of list entries"""
    from types import SimpleNamespace

    from .data_sdf import Pt_sdf_img
    F = SimpleNamespace(num_points=1, num_sample_points=num_sample_points, batch_size=len(group), img_h=137,
                        img_w=137, backcolorwhite=backcolorwhite, rot=rot, max_epoch=1)
    data = Pt_sdf_img(F, listinfo=list(group), info={"sdf_dir": sdf_dir, "rendered_dir": rendered_dir},
                      shuffle=False, seed=seed)
    return data.get_batch(0)


def main(argv=None, reconstruct_fn: Optional[Callable] = None, check_fn: Optional[Callable] = None,
         repair_log: Optional[list] = None, close_log: Optional[list] = None) -> dict:
    """-> {"written", "skipped", "empty", "out_dir"}, with ``--score`` also "scored" (the meshes with a score line of
    status 0), with ``--check`` also "checked" and "watertight" (the meshes with a line in checks.jsonl, and those of
    them that are watertight; ``check_fn``: see ``check_group``), with ``--clean`` also "unclean", with ``--simplify`` also "simplified" (the
    meshes with triangles: those that went through the stage), with ``--smooth`` also "smoothed" (likewise), with
    ``--colour`` also "coloured" (likewise; every mesh
    then ends in ``colours`` uint8 [nv,3], behind the normals when there are any).  ``reconstruct_fn(imgs, trans_mats, sdf_params)``
    replaces the device work (engine + ``reconstruct``) -- for host-side tests of the driver.  With ``--clean`` it is
    called as ``reconstruct_fn(imgs, trans_mats, sdf_params, select)`` -- ``select``: one bool per mesh, True for the
    listed categories -- and returns (meshes, unclean): ``unclean`` marks the meshes of which nothing was kept.
    With ``--repair`` also "repaired" (the meshes with a line in repairs.jsonl: "cat", "obj", "view", then the report of
    ``postprocess.repair_arrays``); ``repair_log``: the list an injected ``reconstruct_fn`` appends one report per mesh
    to (the device route fills its own).  With ``--close`` also "closed" (the meshes with a line in closes.jsonl: "cat",
    "obj", "view", then the report of ``postprocess.close_arrays``); ``close_log``: as ``repair_log``."""
    from concurrent.futures import ThreadPoolExecutor
    from datetime import datetime

    from .evaluate import categories
    a = parser().parse_args(argv)
    fuse = check_flags(a)
    batch_size = a.view_num if a.batch_size is None else a.batch_size
    per_mesh = fuse[0] if fuse else 1            # views that make one mesh; a mesh is named after the first of them
    stages = stages_from_flags(a, a.clean is not None)
    cleaning = stages["clean"] is not None
    clean_cats = clean_cats_from_flags(a)[1] if cleaning else set()
    score = score_from_flags(a)
    check = check_from_flags(a)
    repair = repair_from_flags(a)
    repair_log = [] if repair_log is None else repair_log
    close = close_from_flags(a)
    close_log = [] if close_log is None else close_log
    smooth, coloured = stages["smooth"], stages["colour"] is not None
    out_dir = result_obj_path(a.log_dir, a.sdf_res, a.iso, a.cam_est, fuse, clean=cleaning, simplify=stages["simplify"],
                              colour=coloured, smooth=None if smooth is None else smooth["iters"],
                              mesher=stages["mesher"], repair=repair is not None, close=close is not None)
    entries = sample_list(categories(a.category), a.test_lst_dir, a.view_num, a.seed, a.num_shards, a.shard_id)
    if fuse:
        runs = fuse_runs(entries, per_mesh)
        heads = set(pending([r[0] for r in runs], out_dir)) if a.skip_existing else None
        todo = [e for r in runs if heads is None or r[0] in heads for e in r]
    else:
        todo = pending(entries, out_dir) if a.skip_existing else entries
    work = groups(todo, batch_size)              # (batch_size is a multiple of per_mesh: a group holds whole runs)
    note = "device work replaced by the caller"
    if reconstruct_fn is None and work:
        store, note = restore_weights(a.log_dir, a.random_init)       # before any device work
        import torch

        from .engine import SdfEngine
        engine = SdfEngine(store, torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available()
                           else None, strict=a.strict)

        def reconstruct_fn(imgs, trans_mats, sdf_params, select=None):
            if fuse:                             # (no band: ``fuse_from_flags`` refuses it, the route does not take it)
                out = reconstruct_fused_select(engine, imgs, trans_mats, sdf_params, a.sdf_res, a.iso, fuse=fuse[0],
                                               pool=fuse[1], select=select, strict=False, repair=repair,
                                               repair_log=repair_log, close=close, close_log=close_log,
                                               **{k: v for k, v in stages.items() if k != "band"})
            else:
                out = reconstruct_select(engine, imgs, trans_mats, sdf_params, a.sdf_res, a.iso, refine=a.refine,
                                         normals=a.normals, select=select, strict=False, repair=repair,
                                         repair_log=repair_log, close=close, close_log=close_log, **stages)
            return out if cleaning else out[0]   # the contract of an injected function: the pair only with --clean

    os.makedirs(out_dir, exist_ok=True)
    logf = open(os.path.join(a.log_dir, "log_test.txt"), "a")

    def log_string(s):
        logf.write(s + "\n")
        logf.flush()
        print(s)

    written = empty = unclean = scored = checked = watertight = repaired = closed = 0
    score_cache: dict = {}
    scores_path = os.path.join(out_dir, "scores.jsonl")
    if score is not None and not a.skip_existing:           # every mesh is scored again: the file starts afresh
        open(scores_path, "w").close()
    checks_path = os.path.join(out_dir, "checks.jsonl")
    if check is not None and not a.skip_existing:           # every mesh is checked again: the file starts afresh
        open(checks_path, "w").close()
    repairs_path = os.path.join(out_dir, "repairs.jsonl")
    if repair is not None and not a.skip_existing:          # every mesh is repaired again: the file starts afresh
        open(repairs_path, "w").close()
    closes_path = os.path.join(out_dir, "closes.jsonl")
    if close is not None and not a.skip_existing:           # every mesh is closed again: the file starts afresh
        open(closes_path, "w").close()
    try:
        log_string(str(a))
        log_string("%s; %d views listed, %d to do in %d groups -> %s  (%s)"
                   % (note, len(entries), len(todo), len(work), out_dir, datetime.now()))
        with ThreadPoolExecutor(max_workers=a.writers) as writers, ThreadPoolExecutor(max_workers=1) as loader:
            def fetch(g):
                return loader.submit(load_group, g, a.sdf_dir, a.rendered_dir, a.backcolorwhite)

            nxt = fetch(work[0]) if work else None
            in_flight: List = []
            for gi, group in enumerate(work):
                batch = nxt.result()
                nxt = fetch(work[gi + 1]) if gi + 1 < len(work) else None
                if cleaning:
                    meshes, left = reconstruct_fn(batch["img"], batch["trans_mat"], batch["sdf_params"],
                                                  [e[0] in clean_cats for e in group[::per_mesh]])
                else:
                    meshes = reconstruct_fn(batch["img"], batch["trans_mat"], batch["sdf_params"])
                    left = [False] * len(meshes)
                if len(meshes) * per_mesh != len(group):
                    raise RuntimeError("group %d: %d meshes for %d views" % (gi, len(meshes), len(group)))
                for f in in_flight:                         # the group before this one: a writer's exception surfaces
                    f.result()
                in_flight = []
                if repair is not None:                      # the reports the group's reconstruction left
                    with open(repairs_path, "a") as rf:
                        for (cat_id, obj, view), report in zip(group[::per_mesh], repair_log):
                            rf.write(json.dumps(dict({"cat": cat_id, "obj": obj, "view": view}, **report)) + "\n")
                            repaired += 1
                    del repair_log[:]
                if close is not None:                       # likewise
                    with open(closes_path, "a") as cf:
                        for (cat_id, obj, view), report in zip(group[::per_mesh], close_log):
                            cf.write(json.dumps(dict({"cat": cat_id, "obj": obj, "view": view}, **report)) + "\n")
                            closed += 1
                    del close_log[:]
                if score is not None:                       # the final meshes, still where reconstruct left them
                    rows = score_group(meshes, group[::per_mesh], score, a.seed, score_cache, log=log_string)
                    with open(scores_path, "a") as sf:
                        for row in rows:
                            sf.write(json.dumps(row) + "\n")
                    scored += sum(r["status"] == 0 for r in rows)
                if check is not None:                       # likewise, before the writers take them
                    rows = check_group(meshes, group[::per_mesh], check, check_fn)
                    with open(checks_path, "a") as cf:
                        for row in rows:
                            cf.write(json.dumps(row) + "\n")
                    checked += len(rows)
                    watertight += sum(r["watertight"] for r in rows)
                for (cat_id, obj, view), mesh, as_it_is in zip(group[::per_mesh], meshes, left):
                    verts, faces = mesh[:2]
                    path = obj_path(out_dir, cat_id, obj, view)
                    if as_it_is:
                        unclean += 1
                        log_string("%d/%d, UNCLEAN mesh (no part is kept, written as it is): %s" % (gi, len(work), path))
                    if len(verts) == 0 or len(faces) == 0:
                        empty += 1
                        log_string("%d/%d, EMPTY mesh (no surface at iso %s): %s" % (gi, len(work), a.iso, path))
                    else:
                        log_string("%d/%d, submit create_obj %s, %s, %s" % (gi, len(work), cat_id, obj, view))
                    in_flight.append(writers.submit(write_mesh, path, mesh, coloured))     # device-to-host copy + file
                    written += 1
            for f in in_flight:
                f.result()
        log_string("done: %d written (%d empty), %d skipped  (%s)"
                   % (written, empty, len(entries) - len(todo), datetime.now()))
    finally:
        logf.close()
    res = {"written": written, "skipped": len(entries) - len(todo), "empty": empty, "out_dir": out_dir}
    for key, stage, count in (("unclean", stages["clean"], unclean), ("simplified", stages["simplify"], written - empty),
                              ("smoothed", smooth, written - empty), ("coloured", stages["colour"], written - empty),
                              ("scored", score, scored), ("checked", check, checked),
                              ("watertight", check, watertight), ("repaired", repair, repaired),
                              ("closed", close, closed)):
        if stage is not None:
            res[key] = count
    return res


if __name__ == "__main__":
    main()

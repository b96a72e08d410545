"""One image to one mesh: the reference's ``demo/demo.py [--cam_est]`` on the HIP engine.

    python -m disn_amd.demo --img VIEW.png --log_dir CKPT [--cam_est --cam_log_dir CAM_CKPT]
                            [--sdf_res 64] [--iso 0.0] [--out demo/result.obj] [--refine ITERS] [--normals]
                            [--band STRIDE --band_margin 0.5 --band_dilate 1]
                            [--clean --clean_dist_thresh 0.5 --clean_num_thresh 0.3 --clean_connectivity face]
                            [--simplify CELLS]
                            [--smooth ITERS --smooth_cap 0.5 --smooth_free_boundary]
                            [--preview OUT.png [--preview_size 137]]
                            [--check [--check_pairs 256]]

The image is read as demo/demo.py:261-279 reads it (``cv2.imread(IMREAD_UNCHANGED)[:, :, :3] / 255``: the
channels in B, G, R order, alpha dropped) -- through PIL, which is what this project has.  Without ``--cam_est``
the camera is the ground-truth matrix the reference hard-codes for its demo image (:272-276); with it the
matrix is ``pred_trans_mat`` of ``posenet.CameraEstimator``, restored from ``--cam_log_dir``.  The box is
[-1,-1,-1,1,1,1] (:278), and the mesh comes from ONE ``create_sdf.reconstruct`` call.  As everywhere in this
project a missing checkpoint is an error unless ``--random_init SEED`` asks for initialised weights (the
reference goes on silently).

``--preview OUT.png`` also writes the predicted surface as seen by the camera in use, sphere-traced from the network
without a grid or a mesh (``SdfEngine.trace``), prints the trace's statistics and, when the input PNG has
an alpha channel, the 2-D IoU of the predicted silhouette with it: low with a good mesh means a camera failure.

``--simplify CELLS`` simplifies the mesh on the device before it is written (``postprocess.simplify_meshes_device``,
DESIGN §4za): one quadric-placed vertex per cell of a lattice of CELLS cells per side of the box, behind ``--clean`` and
before ``--refine`` / ``--normals``.

``--smooth ITERS`` fairs the mesh on the device by Taubin's lambda|mu smoothing (``postprocess.smooth_meshes_device``,
DESIGN §4zd) behind ``--simplify`` and before ``--refine`` / ``--normals``: the faces stay, no coordinate moves further
than ``--smooth_cap`` grid cells (default 0.5), boundary vertices stay unless ``--smooth_free_boundary`` is given.

``--check`` measures the final mesh on the device before it is written (``postprocess.check_meshes_device``, DESIGN
§4zh): topology, orientation and self-intersections, printed and written as one JSON line to ``checks.jsonl`` beside
``--out`` (started afresh).  It changes nothing of the mesh.
"""
from __future__ import annotations

import argparse
import os
from typing import Optional

import numpy as np

DEMO_TRANS_MAT = np.asarray(           # demo/demo.py:272-276
    [[[-68.453156, 5.5086656, -0.37556022],
      [-17.138561, -84.685486, -0.250198],
      [-47.284092, -3.6569588, 0.2493176],
      [101.133705, 101.34268, 1.4305686]]], dtype=np.float32)
DEMO_SDF_PARAMS = np.array([[-1, -1, -1, 1, 1, 1]], np.float64)     # demo/demo.py:278


def read_image(path: str) -> np.ndarray:
    """-> [1,H,W,3] float32 in [0,1], channels B,G,R (what cv2 gives the reference), alpha dropped"""
    from PIL import Image
    rgba = np.asarray(Image.open(path).convert("RGBA"), dtype=np.uint8)
    return (rgba[:, :, [2, 1, 0]].astype(np.float32) / np.float32(255.0))[None]


def restore_camera(cam_log_dir: str, random_init: Optional[int]):
    """(encoder store, head arrays) of the camera network from the latest checkpoint of ``cam_log_dir`` (what
    ``train_cam`` saves: 32 vgg_16/* and 18 cameraprediction/* variables).  The engine uploads a whole SDF-network
    store; the point-MLP variables, which the camera network does not have and its encoder call never reads, are
    ``WeightStore.random_init(0)``'s."""
    from . import posenet, tf_checkpoint as tfc, train_cam
    from .weights import WeightStore
    prefix = tfc.get_checkpoint_state(cam_log_dir) if cam_log_dir and os.path.isdir(cam_log_dir) else None
    arrays = None
    if prefix is not None:
        shapes = train_cam.variable_shapes()
        have = tfc.list_variables(prefix)
        if all(n in have for n in shapes):
            arrays = tfc.load_checkpoint(prefix, list(shapes))
            if any(tuple(arrays[n].shape) != tuple(shp) for n, shp in shapes.items()):
                arrays = None
    if arrays is None:
        if random_init is None:
            raise FileNotFoundError("%r holds no complete camera checkpoint; give --random_init SEED to run on "
                                    "initialised weights" % cam_log_dir)
        arrays = train_cam.random_init(random_init)
    store = WeightStore.random_init(0)
    store.assign({k: v for k, v in arrays.items() if k.startswith("vgg_16/")}, strict=True)
    return store, {k: np.asarray(arrays[k], np.float32) for k in posenet.variable_shapes()}


def estimate_camera(img: np.ndarray, cam_log_dir: str, random_init: Optional[int] = None):
    """pred_trans_mat [1,4,3] (device tensor) of the camera network for the image"""
    from .posenet import CameraEstimator
    store, head = restore_camera(cam_log_dir, random_init)
    return CameraEstimator(store, head).get_model(img)["pred_trans_mat"]


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m disn_amd.demo", description="one image -> one mesh (demo/demo.py)")
    p.add_argument("--img", required=True, help="137x137 RGBA rendering (.png)")
    p.add_argument("--log_dir", default="checkpoint/SDF_DISN", help="checkpoint directory of the SDF network")
    p.add_argument("--cam_est", action="store_true", help="estimate the camera instead of the demo image's own")
    p.add_argument("--cam_log_dir", default="cam_est/checkpoint/cam_DISN", help="checkpoint of the camera network")
    p.add_argument("--sdf_res", type=int, default=64, help="cells per axis of the grid [default: 64]")
    p.add_argument("--iso", type=float, default=0.0, help="iso value [default: 0.0]")
    p.add_argument("--out", default=os.path.join("demo", "result.obj"), help="the mesh to write")
    p.add_argument("--random_init", type=int, default=None, metavar="SEED",
                   help="run on freshly initialised weights where a checkpoint is missing")
    p.add_argument("--refine", type=int, default=0, metavar="ITERS",
                   help="Newton steps that move every vertex onto the network's iso level set [default: 0, none]")
    p.add_argument("--normals", action="store_true", help="write the unit SDF gradient at every vertex as 'vn' lines")
    p.add_argument("--preview", default=None, metavar="OUT.png",
                   help="also write the sphere-traced view of the predicted surface from the camera in use")
    p.add_argument("--preview_size", type=int, default=137, metavar="N", help="the preview is N x N [default: 137]")
    from .create_sdf import add_check_flags, add_close_flags, add_repair_flags, add_stage_flags
    p.add_argument("--clean", action="store_true",
                   help="drop the mesh's small and far parts on the device (postprocess.clean_meshes_device)")
    add_stage_flags(p)
    add_check_flags(p)
    add_repair_flags(p)
    add_close_flags(p)
    return p


def read_alpha(path: str) -> Optional[np.ndarray]:
    """-> [H,W] uint8 alpha channel of a PNG, None when it has none"""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("RGBA", "LA"):
            return None
        return np.asarray(im.getchannel("A"), dtype=np.uint8)


def write_preview(engine, img: np.ndarray, trans_mat, path: str, size: int, iso: float,
                  alpha: Optional[np.ndarray] = None) -> dict:
    """the traced view of image 0 from its own camera -> ``path``; returns {"stats", "iou" (None without alpha)}"""
    from . import render
    from .create_img_h5 import _write_png
    if size < 1:
        raise ValueError("--preview_size must be positive")
    out = engine.trace(engine.encode(img), 0, trans_mat, size=(size, size), sdf_params=DEMO_SDF_PARAMS[0], iso=iso)
    rgba = out["rgba"][0].cpu().numpy()
    _write_png(path, rgba)
    print("preview %s: %s" % (path, out["stats"]))
    iou = None
    if alpha is not None:
        rows = ((np.arange(size) + 0.5) * alpha.shape[0] / size).astype(np.int64)     # the alpha at the rays' pixels
        cols = ((np.arange(size) + 0.5) * alpha.shape[1] / size).astype(np.int64)
        iou = render.silhouette_iou(rgba[:, :, 3], alpha[rows][:, cols])
        print("silhouette IoU with the input's alpha channel: %.4f" % iou)
    return {"stats": out["stats"], "iou": iou}


def main(argv=None) -> dict:
    """-> {"out", "verts", "faces", "trans_mat"}, with ``--colour`` also "coloured" (True) and "colours" (uint8 [nv,3]),
    with ``--check`` also "checked" (1), "watertight" (0 or 1) and "check" (the mesh's line of checks.jsonl), with
    ``--repair`` also "repair" (the mesh's line of repairs.jsonl, written beside ``--out``), with ``--close`` also
    "close" (likewise, closes.jsonl)"""
    a = parser().parse_args(argv)
    from .create_sdf import (check_from_flags, check_group, close_from_flags, reconstruct, repair_from_flags,
                             restore_weights, stages_from_flags, write_mesh)
    stages = stages_from_flags(a, a.clean)                             # a bad flag: before anything else
    check = check_from_flags(a)
    repair, repair_log = repair_from_flags(a), []
    close, close_log = close_from_flags(a), []
    coloured = stages["colour"] is not None
    img = read_image(a.img)
    if img.shape[1:3] != (137, 137):
        raise ValueError("%s is %dx%d; the network reads 137x137 renderings" % (a.img, img.shape[2], img.shape[1]))
    store, note = restore_weights(a.log_dir, a.random_init)            # before any device work
    print(note)
    from .engine import SdfEngine
    if a.cam_est:
        print("here we use our cam est network to estimate cam parameters:")
        trans_mat = estimate_camera(img, a.cam_log_dir, a.random_init)
        print("pred_trans_mat_val", trans_mat.cpu().numpy())
    else:
        print("here we use gt cam parameters")
        trans_mat = DEMO_TRANS_MAT
    engine = SdfEngine(store)
    if a.refine < 0:
        raise ValueError("--refine must not be negative")
    alpha = read_alpha(a.img) if coloured else None                    # the background of the rendering colours nothing
    mesh = reconstruct(engine, img, trans_mat, DEMO_SDF_PARAMS, a.sdf_res, a.iso, a.refine, a.normals,
                       alpha=None if alpha is None else alpha[None], repair=repair, repair_log=repair_log,
                       close=close, close_log=close_log, **stages)[0]
    verts, faces = mesh[:2]
    if repair_log:                                                     # the report of --repair, beside the mesh
        import json
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(os.path.join(os.path.dirname(os.path.abspath(a.out)), "repairs.jsonl"), "w") as rf:
            rf.write(json.dumps(dict({"cat": "", "obj": os.path.basename(a.out), "view": 0}, **repair_log[0])) + "\n")
        print("repair: %s" % repair_log[0])
    if close_log:                                                      # likewise, the report of --close
        import json
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(os.path.join(os.path.dirname(os.path.abspath(a.out)), "closes.jsonl"), "w") as cf:
            cf.write(json.dumps(dict({"cat": "", "obj": os.path.basename(a.out), "view": 0}, **close_log[0])) + "\n")
        print("close: %s" % close_log[0])
    row = None
    if check is not None:                                              # the final mesh, before it is written
        import json
        row = check_group([mesh], [("", os.path.basename(a.out), 0)], check)[0]
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(os.path.join(os.path.dirname(os.path.abspath(a.out)), "checks.jsonl"), "w") as cf:
            cf.write(json.dumps(row) + "\n")
        print("check: %s" % row)
    write_mesh(a.out, mesh, coloured)
    print("wrote %s: %d vertices, %d triangles" % (a.out, len(verts), len(faces)))
    tm = trans_mat.cpu().numpy() if hasattr(trans_mat, "cpu") else trans_mat
    res = {"out": a.out, "verts": len(verts), "faces": len(faces), "trans_mat": tm}
    if coloured:
        res["coloured"], res["colours"] = True, mesh[-1].cpu().numpy()
    if row is not None:
        res["checked"], res["watertight"], res["check"] = 1, int(row["watertight"]), row
    if repair_log:
        res["repair"] = repair_log[0]
    if close_log:
        res["close"] = close_log[0]
    if a.preview:
        res["preview"] = write_preview(engine, img, trans_mat, a.preview, a.preview_size, a.iso, read_alpha(a.img))
    return res


if __name__ == "__main__":
    main()

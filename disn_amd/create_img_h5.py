"""Per-view files for the loaders: the reference's ``preprocessing/create_img_h5.py``, and with ``--render`` the
renders it starts from.

    python -m disn_amd.create_img_h5 --info info.json [--category chair]
    python -m disn_amd.create_img_h5 --info info.json --render [--views 24] [--samples 4] [--seed 0] [--materials]

Layout (info.json as for ``disn_amd.preprocess``, with rendered_dir / renderedh5_dir / sdf_dir / mesh_dir in
"raw_dirs_v1"):
  input   <rendered_dir>/<cat_id>/<obj>/rendering/{renderings.txt, rendering_metadata.txt, NN.png}
          <sdf_dir>/<cat_id>/<obj>/ori_sample.{npz,h5}     (norm_params; written by ``disn_amd.preprocess``)
  output  <renderedh5_dir>/<cat_id>/<obj>/NN.npz           img_arr (BGRA, as cv2.imread(IMREAD_UNCHANGED) gives it),
                                                           trans_mat, regress_mat, obj_rot_mat, K, RT
The view files are what ``data_sdf.Pt_sdf_img`` and ``data_cam.Pt_sdf_img_cam`` read when their
``info["rendered_dir"]`` names <renderedh5_dir>.  The default mode is the reference's ``convert_img2h5`` and needs no
device.

``--render`` first creates the ``rendering/`` directory of every listed object from
<mesh_dir>/<cat_id>/<obj>/model.obj (``--version 2``: models/model_normalized.obj) on the device
(``render.render_views``: one BVH upload, one launch and one read-back per object; PNG encoding on writer threads):
RGBA PNGs, ``renderings.txt`` and ``rendering_metadata.txt`` with rows "az el tilt distance_ratio 25".  The
viewpoints come from ``render.random_view_params`` with a generator seeded by (seed, object index); their default
ranges are UNPINNED (recalled from the public renders' metadata, not compared with it) and are flags.  The images
are a headlight shading of a flat albedo, not Blender's lighting and materials.

Views that exist and load are skipped in both modes, so a second run writes nothing.
"""
from __future__ import annotations

import argparse
import os
import sys
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Tuple

import numpy as np

from . import data_cam, render
from .data_sdf import _load

MAX_WRITERS = 16


def list_objects(cats: Dict[str, str], lst_dir: str) -> List[Tuple[int, str, str]]:
    """(object index, cat_id, obj) in the order of ``preprocess.create_sdf``: per category the test list, then
    the train list"""
    out = []
    for _, cat_id in cats.items():
        for split in ("test", "train"):
            with open(os.path.join(lst_dir, str(cat_id) + "_%s.lst" % split)) as f:
                for line in f.readlines():
                    if line.strip():
                        out.append((len(out), cat_id, line.strip()))
    return out


def read_png_as_cv2(path: str) -> np.ndarray:
    """cv2.imread(path, IMREAD_UNCHANGED) for 8-bit PNGs: [H,W,4] BGRA, [H,W,3] BGR or [H,W] grey, uint8"""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("RGBA", "RGB", "L"):
            im = im.convert("RGBA")
        a = np.asarray(im, dtype=np.uint8)
    if a.ndim == 3 and a.shape[2] == 4:
        return np.ascontiguousarray(a[:, :, [2, 1, 0, 3]])
    if a.ndim == 3:
        return np.ascontiguousarray(a[:, :, ::-1])
    return a


def _view_file_loads(path: str) -> bool:
    try:
        with np.load(path) as z:
            return z["trans_mat"].shape == (4, 3) and "img_arr" in z.files
    except Exception:
        return False


def _png_loads(path: str) -> bool:
    from PIL import Image
    try:
        with Image.open(path) as im:
            im.load()
        return True
    except Exception:
        return False


def _rendering_lists(img_dir: str):
    with open(os.path.join(img_dir, "renderings.txt")) as f:
        file_lst = [line.strip() for line in f.read().splitlines() if line.strip()]
    params = np.atleast_2d(np.loadtxt(os.path.join(img_dir, "rendering_metadata.txt")))
    return file_lst, params


def gen_obj_img_h5(source_dir: str, target_dir: str, sdf_dir: str, cat_id: str, obj: str) -> int:
    """the view files of one object (the reference's function of this name) -> the number written"""
    img_dir = os.path.join(source_dir, cat_id, obj, "rendering")
    file_lst, params = _rendering_lists(img_dir)
    norm_params = None
    written = 0
    for i, name in enumerate(file_lst):
        num = int(name[:2])
        if _view_file_loads(os.path.join(target_dir, cat_id, obj, "%02d.npz" % num)):
            continue
        if norm_params is None:
            norm_params = _load(os.path.join(sdf_dir, cat_id, obj, "ori_sample.h5"), ("norm_params",))["norm_params"]
        K, RT, trans_mat, regress_mat, obj_rot_mat = render.view_matrices(params[i], norm_params)
        img_arr = read_png_as_cv2(os.path.join(img_dir, name))
        data_cam.save_view_cam(target_dir, cat_id, obj, num, img_arr, trans_mat, obj_rot_mat, regress_mat, K, RT)
        written += 1
    return written


def _write_png(path: str, rgba: np.ndarray) -> None:
    from PIL import Image
    tmp = path + ".tmp"
    Image.fromarray(np.ascontiguousarray(rgba, np.uint8)).save(tmp, format="PNG")
    os.replace(tmp, path)


def render_obj(model_file: str, img_dir: str, rng: np.random.Generator, a, writers: ThreadPoolExecutor) -> list:
    """the rendering/ directory of one object -> the futures of its PNG writes (empty when nothing was missing).
    An existing rendering_metadata.txt keeps its viewpoints; only missing or unreadable PNGs are written."""
    from . import mesh_sdf
    os.makedirs(img_dir, exist_ok=True)
    meta = os.path.join(img_dir, "rendering_metadata.txt")
    names = ["%02d.png" % k for k in range(a.views)]
    params = None
    if os.path.exists(meta):
        try:
            params = np.atleast_2d(np.loadtxt(meta))
        except Exception:
            params = None
    if params is None or params.shape[0] != a.views or params.shape[1] < 4:
        params = render.random_view_params(rng, a.views, el=(a.el_min, a.el_max), dist=(a.dist_min, a.dist_max))
        np.savetxt(meta, params, fmt="%.17g")
        params = np.atleast_2d(np.loadtxt(meta))
    lst = os.path.join(img_dir, "renderings.txt")
    missing = [k for k, n in enumerate(names) if not _png_loads(os.path.join(img_dir, n))]
    if not os.path.exists(lst):
        with open(lst, "w") as f:
            f.write("\n".join(names) + "\n")
    if not missing:
        return []
    verts, faces = mesh_sdf.read_obj_mesh(model_file)
    albedo = render.read_obj_albedo(model_file, len(faces)) if a.materials else None
    out = render.render_views(mesh_sdf.MeshBvh(verts, faces), None, params, size=(137, 137), samples=a.samples,
                              albedo=albedo, ambient=a.ambient)
    rgba = out["rgba"].cpu().numpy()
    return [writers.submit(_write_png, os.path.join(img_dir, names[k]), rgba[k]) for k in missing]


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m disn_amd.create_img_h5",
                                description="per-view files (image + camera matrices) from renders "
                                            "(preprocessing/create_img_h5.py); --render makes the renders")
    p.add_argument("--info", required=True, help="info.json: lst_dir, cats, all_cats, raw_dirs_v1")
    p.add_argument("--category", default="all", help="which single class to generate [default: all]")
    p.add_argument("--render", action="store_true", help="render the views from the meshes first (needs the device)")
    p.add_argument("--views", type=int, default=24)
    p.add_argument("--samples", type=int, default=4, help="S of the S x S sample grid per pixel, 1..4")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--materials", action="store_true", help="colour the faces by the Kd of their usemtl material")
    p.add_argument("--version", type=int, default=1, help="1: <obj>/model.obj, 2: <obj>/models/model_normalized.obj")
    p.add_argument("--ambient", type=float, default=0.3)
    p.add_argument("--el_min", type=float, default=25.0, help="elevation range in degrees (unpinned)")
    p.add_argument("--el_max", type=float, default=30.0)
    p.add_argument("--dist_min", type=float, default=0.65, help="distance-ratio range (unpinned)")
    p.add_argument("--dist_max", type=float, default=0.95)
    p.add_argument("--writers", type=int, default=4, help="PNG writer threads, at most %d [default: 4]" % MAX_WRITERS)
    return p


def main(argv=None) -> Dict[str, int]:
    from .preprocess import get_all_info
    a = parser().parse_args(argv)
    if not 1 <= a.writers <= MAX_WRITERS:
        raise ValueError("--writers must be in 1..%d, got %d" % (MAX_WRITERS, a.writers))
    if not 1 <= a.views <= 100:
        raise ValueError("--views must be in 1..100 (two-digit file names), got %d" % a.views)
    lst_dir, cats, _, raw_dirs = get_all_info(a.info)
    if a.category != "all":
        cats = {a.category: cats[a.category]}
    objects = list_objects(cats, lst_dir)
    rendered = 0
    if a.render:
        with ThreadPoolExecutor(max_workers=a.writers) as writers:
            in_flight: list = []
            for indx, cat_id, obj in objects:
                sub = ("model.obj",) if a.version == 1 else ("models", "model_normalized.obj")
                model_file = os.path.join(raw_dirs["mesh_dir"], cat_id, obj, *sub)
                img_dir = os.path.join(raw_dirs["rendered_dir"], cat_id, obj, "rendering")
                futures = render_obj(model_file, img_dir, np.random.default_rng([int(a.seed), int(indx)]), a, writers)
                for f in in_flight:                      # the object before this one: a writer's exception surfaces
                    f.result()
                in_flight = futures
                rendered += len(futures)
            for f in in_flight:
                f.result()
    written = 0
    for _, cat_id, obj in objects:
        written += gen_obj_img_h5(raw_dirs["rendered_dir"], raw_dirs["renderedh5_dir"], raw_dirs["sdf_dir"], cat_id,
                                  obj)
    print("create_img_h5: %d objects, %d images rendered, %d view files written" % (len(objects), rendered, written))
    return {"objects": len(objects), "rendered": rendered, "written": written}


if __name__ == "__main__":
    sys.exit(0 if main() is not None else 1)

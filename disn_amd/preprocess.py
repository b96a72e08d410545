"""Training samples and ground-truth meshes from raw meshes: the reference's
``preprocessing/create_point_sdf_grid.py``, same function names and arguments, with the two closed binaries
replaced by the device: ``computeDistanceField`` by ``mesh_sdf.sdf_grid`` and ``computeMarchingCubes`` by
``isosurface.marching_cubes``.

    python -m disn_amd.preprocess --info info.json [--category chair] [--res 256] [--g 0.0]

Layout (info.json of the reference: "lst_dir", "cats", "raw_dirs_v1" with mesh_dir / norm_mesh_dir / sdf_dir):
  input   <mesh_dir>/<cat_id>/<obj>/model.obj              (--version 2: <obj>/models/model_normalized.obj)
          <lst_dir>/<cat_id>_test.lst, <cat_id>_train.lst
  output  <sdf_dir>/<cat_id>/<obj>/ori_sample.npz          (what data_sdf.Pt_sdf_img reads; isinsideout.txt)
          <norm_mesh_dir>/<cat_id>/<obj>/isosurf.obj       (what ``python -m disn_amd.evaluate --gt_dir`` reads)
          <norm_mesh_dir>/<cat_id>/<obj>/pc_norm.obj       (the normalised input mesh; the reference deletes it)
Samples are written as .npz (data_sdf.save_sample), not HDF5.  Randomness comes from a seeded
``numpy.random.Generator``, one per object (seed, object index), so a run is reproducible.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from typing import Dict, Optional

import numpy as np
import torch

from . import create_sdf as _cs
from . import data_sdf, isosurface, mesh_sdf

INSIDEOUT_CATS = ("02958343", "02691156", "04530566")    # car, airplane, watercraft


def sample_surface(verts, faces, count: int, rng: np.random.Generator) -> np.ndarray:
    """``trimesh.sample.sample_surface``: a face picked by cumulative area, (u, v) uniform, reflected when
    u + v > 1 -> float64 [count, 3]"""
    v = np.asarray(verts, np.float64)
    tri = v[np.asarray(faces, np.int64)]
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    cum = np.cumsum(area)
    face_index = np.searchsorted(cum, rng.random(count) * cum[-1])
    origins = tri[face_index, 0]
    vectors = tri[face_index, 1:] - tri[face_index, :1]
    lengths = rng.random((count, 2, 1))
    flip = lengths.sum(axis=1).reshape(-1) > 1.0
    lengths[flip] -= 1.0
    lengths = np.abs(lengths)
    return (vectors * lengths).sum(axis=1) + origins


def normalize_params(verts, faces, rng: np.random.Generator, total: int = 16384):
    """(centroid float64 [3], m float64): the mean of ``total`` area-weighted surface samples and their largest
    distance from it (get_normalize_mesh)"""
    pts = sample_surface(verts, faces, total, rng)
    centroid = np.mean(pts, axis=0)
    m = float(np.max(np.sqrt(np.sum((pts - centroid) ** 2, axis=1))))
    return centroid, m


def get_normalize_mesh(model_file: str, norm_mesh_sub_dir: str, rng: Optional[np.random.Generator] = None):
    """-> (obj_file, centroid, m); writes <norm_mesh_sub_dir>/pc_norm.obj = (verts - centroid) / m"""
    rng = rng if rng is not None else np.random.default_rng(0)
    verts, faces = mesh_sdf.read_obj_mesh(model_file)
    centroid, m = normalize_params(verts, faces, rng)
    obj_file = os.path.join(norm_mesh_sub_dir, "pc_norm.obj")
    isosurface.write_obj(obj_file, ((verts.astype(np.float64) - centroid) / m).astype(np.float32), faces)
    return obj_file, centroid, m


def create_one_sdf(res: int, expand_rate: float, sdf_file: Optional[str], obj_file: str, indx: int = 0,
                   g: float = 0.0, seal: float = 1.0):
    """computeDistanceField <obj_file> res res res -s -e expand_rate -m 1 [-g g] -> {"param": float32 [6],
    "value": device tensor [(res+1)^3]} (get_sdf's dictionary); the .dist file is written when ``sdf_file`` is
    given.  ``indx`` is accepted for the reference's signature (it named a temporary file)."""
    verts, faces = mesh_sdf.read_obj_mesh(obj_file)
    sdf, params = mesh_sdf.sdf_grid(verts, faces, res, expand=expand_rate, seal=seal, offset=g)
    if sdf_file:
        _cs.to_binary(res, params.astype(np.float64), sdf.cpu().numpy(), sdf_file)
    return {"param": params, "value": sdf}


def _bins(bandwidth: float, num_sample: int):
    """the reference's four distance bins [lo, hi) with their float32 bounds and requested counts"""
    return [[np.float32(-1. * bandwidth), np.float32(-1. * bandwidth * 0.30), int(num_sample * 0.25)],
            [np.float32(-1. * bandwidth * 0.30), np.float32(0), int(num_sample * 0.25)],
            [np.float32(0), np.float32(bandwidth * 0.30), int(num_sample * 0.25)],
            [np.float32(bandwidth * 0.30), np.float32(bandwidth), int(num_sample * 0.25)]]


def sample_sdf(cat_id, num_sample, bandwidth, iso_val, sdf_dict, sdf_res, rng: Optional[np.random.Generator] = None):
    """-> (rows float32 [k, 4] of (x, y, z, value), is_insideout).  Four bins of value - iso, a bin's shortfall
    carried into the next bin only; draws with replacement among a bin's nodes in increasing flat index.  The
    counting and the gather run where ``sdf_dict["value"]`` lies (device or CPU tensor, or numpy); only the bin
    counts come to the host."""
    rng = rng if rng is not None else np.random.default_rng(0)
    params = np.asarray(sdf_dict["param"], np.float32)
    vals = sdf_dict["value"]
    vals = vals if isinstance(vals, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(vals, np.float32))
    vals = vals.reshape(-1)
    dev = vals.device
    n1 = sdf_res + 1
    x, y, z = mesh_sdf.grid_axes(params, sdf_res)
    axes = [torch.from_numpy(a).to(dev) for a in (x, y, z)]
    dis = vals - float(iso_val)            # float32 - float32(iso), as numpy computes it
    percentages = _bins(bandwidth, num_sample)
    masks = [(dis >= float(lo)) & (dis < float(hi)) for lo, hi, _ in percentages]
    counts = torch.stack([mk.sum() for mk in masks]).cpu().tolist()
    rows = []
    for i in range(len(percentages)):
        cnt = int(counts[i])
        if cnt < percentages[i][2]:
            if i < len(percentages) - 1:
                percentages[i + 1][2] += percentages[i][2] - cnt
            percentages[i][2] = cnt
        if cnt == 0:
            continue
        ind = torch.nonzero(masks[i]).reshape(-1)
        choice = torch.from_numpy(rng.integers(cnt, size=percentages[i][2]).astype(np.int64)).to(dev)
        k = ind.index_select(0, choice)
        rows.append(torch.stack([axes[0][k % n1], axes[1][(k // n1) % n1], axes[2][k // (n1 * n1)],
                                 vals.index_select(0, k)], dim=1))
    out = torch.cat(rows).cpu().numpy() if rows else np.zeros((0, 4), np.float32)
    return out.astype(np.float32), check_insideout(cat_id, vals, sdf_res, x, y, z)


def check_insideout(cat_id, sdf_val, sdf_res, x, y, z) -> bool:
    """car / airplane / watercraft: the node nearest the origin has a positive value"""
    if cat_id in INSIDEOUT_CATS:
        x_ind = int(np.argmin(np.absolute(x)))
        y_ind = int(np.argmin(np.absolute(y)))
        z_ind = int(np.argmin(np.absolute(z)))
        flat = x_ind + y_ind * (sdf_res + 1) + z_ind * (sdf_res + 1) ** 2
        v = sdf_val.reshape(-1)[flat]
        return bool(float(v) > 0.0)
    return False


def create_h5_sdf_pt(cat_id, h5_file, sdf_dict, flag_file, cube_obj_file, norm_obj_file, centroid, m, sdf_res,
                     num_sample, bandwidth, iso_val, max_verts, normalize, rng: Optional[np.random.Generator] = None):
    """samples + flags of one object -> ``ori_sample.npz`` next to ``h5_file`` (data_sdf.save_sample).  The
    reference reads the .dist file here; this takes get_sdf's dictionary.  ``cube_obj_file``, ``norm_obj_file``,
    ``max_verts`` and ``normalize`` are accepted for the reference's signature."""
    ori_verts = np.asarray([0.0, 0.0, 0.0], dtype=np.float32).reshape((1, 3))
    samplesdf, is_insideout = sample_sdf(cat_id, num_sample, bandwidth, iso_val, sdf_dict, sdf_res, rng)
    if is_insideout:
        with open(flag_file, "w") as f:
            f.write("mid point sdf val > 0")
    elif os.path.exists(flag_file):
        os.remove(flag_file)
    norm_params = np.concatenate((np.asarray(centroid, np.float32), np.asarray([m]).astype(np.float32)))
    obj_dir = os.path.dirname(os.path.abspath(h5_file))
    cat_dir = os.path.dirname(obj_dir)
    data_sdf.save_sample(os.path.dirname(cat_dir), os.path.basename(cat_dir), os.path.basename(obj_dir), ori_verts,
                         samplesdf, norm_params, sdf_dict["param"])
    return samplesdf, is_insideout


def create_one_cube_obj(sdf_dict, sdf_res, i, cube_obj_file) -> str:
    """computeMarchingCubes -i i on the grid where it lies (isosurface.marching_cubes)"""
    verts, faces = isosurface.marching_cubes(sdf_dict["value"], np.asarray(sdf_dict["param"], np.float64), sdf_res,
                                             float(i))
    isosurface.write_obj(cube_obj_file, verts, faces)
    return cube_obj_file


def create_sdf_obj(cat_mesh_dir, cat_norm_mesh_dir, cat_sdf_dir, obj, res, iso_val, expand_rate, indx, ish5,
                   normalize, num_sample, bandwidth, max_verts, cat_id, g, version, skip_all_exist,
                   keep_dist: bool = False, seed: int = 0):
    """one object: normalise, signed distance grid, isosurf.obj, samples.  Returns the sample path (or None when
    skipped)."""
    obj = obj.rstrip('\r\n')
    sdf_sub_dir = os.path.join(cat_sdf_dir, obj)
    norm_mesh_sub_dir = os.path.join(cat_norm_mesh_dir, obj)
    os.makedirs(sdf_sub_dir, exist_ok=True)
    os.makedirs(norm_mesh_sub_dir, exist_ok=True)
    sdf_file = os.path.join(sdf_sub_dir, "isosurf.sdf")
    flag_file = os.path.join(sdf_sub_dir, "isinsideout.txt")
    cube_obj_file = os.path.join(norm_mesh_sub_dir, "isosurf.obj")
    h5_file = os.path.join(sdf_sub_dir, "ori_sample.h5")
    npz_file = os.path.join(sdf_sub_dir, "ori_sample.npz")
    if ish5 and os.path.exists(npz_file) and (skip_all_exist or not os.path.exists(flag_file)):
        print("skip existed: ", npz_file)
        return None
    if not ish5 and os.path.exists(sdf_file):
        print("skip existed: ", sdf_file)
        return None
    if version == 1:
        model_file = os.path.join(cat_mesh_dir, obj, "model.obj")
    else:
        model_file = os.path.join(cat_mesh_dir, obj, "models", "model_normalized.obj")
    rng = np.random.default_rng([int(seed), int(indx)])
    if normalize:
        norm_obj_file, centroid, m = get_normalize_mesh(model_file, norm_mesh_sub_dir, rng)
    else:
        norm_obj_file, centroid, m = model_file, np.zeros(3), 1.0
    sdf_dict = create_one_sdf(res, expand_rate, sdf_file if (keep_dist or not ish5) else None, norm_obj_file, indx,
                              g=g)
    create_one_cube_obj(sdf_dict, res, iso_val, cube_obj_file)
    if ish5:
        create_h5_sdf_pt(cat_id, h5_file, sdf_dict, flag_file, cube_obj_file, norm_obj_file, centroid, m, res,
                         num_sample, bandwidth, iso_val, max_verts, normalize, rng)
        return npz_file
    return sdf_file


def create_sdf(num_sample, bandwidth, res, expand_rate, cats: Dict[str, str], raw_dirs, lst_dir, iso_val, max_verts,
               ish5=True, normalize=True, g=0.00, version=2, skip_all_exist=False, keep_dist=False, seed=0):
    """every object of <lst_dir>/<cat_id>_test.lst and _train.lst of every category, one after the other on the
    current device"""
    sdf_dir = raw_dirs["sdf_dir"]
    os.makedirs(sdf_dir, exist_ok=True)
    start = 0
    for catnm, cat_id in cats.items():
        cat_sdf_dir = os.path.join(sdf_dir, cat_id)
        os.makedirs(cat_sdf_dir, exist_ok=True)
        cat_mesh_dir = os.path.join(raw_dirs["mesh_dir"], cat_id)
        cat_norm_mesh_dir = os.path.join(raw_dirs["norm_mesh_dir"], cat_id)
        list_obj = []
        for split in ("test", "train"):
            with open(os.path.join(lst_dir, str(cat_id) + "_%s.lst" % split)) as f:
                list_obj += [l for l in f.readlines() if l.strip()]
        for indx, obj in enumerate(list_obj, start):
            create_sdf_obj(cat_mesh_dir, cat_norm_mesh_dir, cat_sdf_dir, obj, res, iso_val, expand_rate, indx, ish5,
                           normalize, num_sample, bandwidth, max_verts, cat_id, g, version, skip_all_exist,
                           keep_dist=keep_dist, seed=seed)
        start += len(list_obj)
    print("finish all")


def get_all_info(info_file: str):
    """create_file_lst.get_all_info: (lst_dir, cats, all_cats, raw_dirs) of an info.json"""
    with open(info_file) as f:
        data = json.load(f)
    return data["lst_dir"], data["cats"], data["all_cats"], data["raw_dirs_v1"]


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m disn_amd.preprocess",
                                description="signed distance samples and ground-truth meshes from raw meshes "
                                            "(preprocessing/create_point_sdf_grid.py)")
    p.add_argument("--info", required=True, help="info.json: lst_dir, cats, all_cats, raw_dirs_v1")
    p.add_argument("--category", default="all", help="which single class to generate [default: all]")
    p.add_argument("--res", type=int, default=256)
    p.add_argument("--expand_rate", type=float, default=1.2)
    p.add_argument("--num_sample", type=int, default=32768)
    p.add_argument("--bandwidth", type=float, default=0.1)
    p.add_argument("--iso_val", type=float, default=0.003)
    p.add_argument("--g", type=float, default=0.0, help="offset subtracted from the field (computeDistanceField -g)")
    p.add_argument("--version", type=int, default=1, help="1: <obj>/model.obj, 2: <obj>/models/model_normalized.obj")
    p.add_argument("--skip_all_exist", action="store_true")
    p.add_argument("--keep_dist", action="store_true", help="also write <obj>/isosurf.sdf (.dist format)")
    p.add_argument("--seed", type=int, default=0)
    return p


def main(argv=None) -> None:
    a = parser().parse_args(argv)
    lst_dir, cats, _, raw_dirs = get_all_info(a.info)
    if a.category != "all":
        cats = {a.category: cats[a.category]}
    create_sdf(a.num_sample, a.bandwidth, a.res, a.expand_rate, cats, raw_dirs, lst_dir, a.iso_val, 16384,
               ish5=True, normalize=True, g=a.g, version=a.version, skip_all_exist=a.skip_all_exist,
               keep_dist=a.keep_dist, seed=a.seed)


if __name__ == "__main__":
    sys.exit(main())

"""Removal of small disconnected parts from reconstructed meshes: the reference's ``postprocessing/clean_smallparts.py``
(``pymesh.separate_mesh`` + ``pymesh.merge_meshes``), which it runs on five categories (``evaluate.CATS_CLEAN``)
before scoring them.

    python -m disn_amd.postprocess --src_dir OBJS --tar_dir OBJS_CLEAN [--category clean]

Layout: <src_dir>/<cat_id>/*.obj -> <tar_dir>/<cat_id>/<same name>.  Rule, as the reference: a part is kept when
it has more than ``num_thresh`` times the largest part's vertex count and the mean of its vertices lies within
``dist_thresh`` of the origin; the kept parts are merged in component order, vertices re-indexed (each part's
vertices in their original order), unreferenced vertices dropped.
Differences from the reference: if no part is kept, this raises instead of writing an empty file; the component
labelling is ``disn_mesh_components`` (host C++, union-find), with "face" connectivity (triangles that share an
edge) standing for PyMesh's ``auto`` on a surface mesh -- restated from reading, PyMesh itself is unpinned -- and
"vertex" connectivity (triangles that share a vertex) on request.  The step is bound by reading and writing the
.obj files; it has no device part.
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys
from typing import Dict, List, Tuple

import numpy as np

from ._lib import lib

CONNECTIVITY = {"face": 0, "vertex": 1}


def _host(verts, faces) -> Tuple[np.ndarray, np.ndarray]:
    v = verts.detach().cpu().numpy() if hasattr(verts, "detach") else verts
    f = faces.detach().cpu().numpy() if hasattr(faces, "detach") else faces
    return (np.ascontiguousarray(v, np.float32).reshape(-1, 3), np.ascontiguousarray(f, np.int32).reshape(-1, 3))


def separate_mesh(verts, faces, connectivity: str = "face") -> Tuple[np.ndarray, np.ndarray]:
    """-> (labels int32 [nf], vert_counts int64 [ncomp]): the connected component of every triangle (a component's
    id is the rank of its smallest face index) and the number of distinct vertices each component references"""
    if connectivity not in CONNECTIVITY:
        raise ValueError("connectivity must be 'face' or 'vertex' (got %r)" % (connectivity,))
    v, f = _host(verts, faces)
    nf = f.shape[0]
    labels = np.empty(nf, np.int32)
    ncomp = C.c_int64(0)
    rc = lib().disn_mesh_components(f.ctypes.data if nf else None, nf, v.shape[0], CONNECTIVITY[connectivity],
                                    labels.ctypes.data if nf else None, C.byref(ncomp))
    if rc == -1:
        raise ValueError("face index out of range (mesh of %d vertices)" % v.shape[0])
    if rc != 0:
        raise ValueError("disn_mesh_components failed (status %d)" % rc)
    counts = np.zeros(ncomp.value, np.int64)
    if nf:
        pairs = np.unique(np.stack([np.repeat(labels, 3).astype(np.int64), f.reshape(-1).astype(np.int64)], 1), axis=0)
        counts = np.bincount(pairs[:, 0], minlength=ncomp.value).astype(np.int64)
    return labels, counts


def clean_arrays(verts, faces, dist_thresh: float = 0.5, num_thresh: float = 0.3, connectivity: str = "face"
                 ) -> Tuple[np.ndarray, np.ndarray, List[int]]:
    """-> (verts, faces, kept component ids) of the mesh without its small or far parts (host arrays)"""
    v, f = _host(verts, faces)
    if f.shape[0] == 0:
        raise ValueError("the mesh has no triangles")
    labels, counts = separate_mesh(v, f, connectivity)
    biggest = counts.max()
    out_v, out_f, kept, base = [], [], [], 0
    for c in range(counts.size):
        if not counts[c] > biggest * num_thresh:
            continue
        fc = f[labels == c]
        used = np.unique(fc)                                   # ascending: the part's vertices in their original order
        centroid = v[used].astype(np.float64).mean(0)
        if not np.sqrt(np.sum(np.square(centroid))) < dist_thresh:
            continue
        out_v.append(v[used])
        out_f.append((np.searchsorted(used, fc) + base).astype(np.int32))
        base += used.size
        kept.append(c)
    if not kept:
        raise ValueError("no part is kept (dist_thresh %g, num_thresh %g): %d parts, the largest of %d vertices"
                         % (dist_thresh, num_thresh, counts.size, biggest))
    return np.concatenate(out_v), np.concatenate(out_f), kept


def clean_single_mesh(src: str, tar: str, dist_thresh: float = 0.5, num_thresh: float = 0.3,
                      connectivity: str = "face", out=None) -> List[int]:
    """clean_smallparts.py:44-59: read ``src``, drop the small and the far parts, write ``tar``"""
    from . import isosurface, mesh_sdf
    v, f = mesh_sdf.read_obj_mesh(src)
    try:
        cv, cf, kept = clean_arrays(v, f, dist_thresh, num_thresh, connectivity)
    except ValueError as e:
        raise ValueError("%s: %s" % (src, e)) from e
    isosurface.write_obj(tar, cv, cf)
    print("threshes: %s %s  clean:  %s  create:  %s" % (dist_thresh, num_thresh, src, tar), file=out or sys.stdout)
    return kept


def clean_meshes(cats: Dict[str, str], src_dir: str, tar_dir: str, dist_thresh: float = 0.5, num_thresh: float = 0.3,
                 connectivity: str = "face", out=None) -> int:
    """every file of <src_dir>/<cat_id> -> <tar_dir>/<cat_id> (clean_smallparts.py:61-76) -> the number written"""
    out = out or sys.stdout
    n = 0
    for cat_nm, cat_id in cats.items():
        src_cat, tar_cat = os.path.join(src_dir, cat_id), os.path.join(tar_dir, cat_id)
        os.makedirs(tar_cat, exist_ok=True)
        for fn in sorted(os.listdir(src_cat)):
            if os.path.isfile(os.path.join(src_cat, fn)):
                clean_single_mesh(os.path.join(src_cat, fn), os.path.join(tar_cat, fn), dist_thresh, num_thresh,
                                  connectivity, out=out)
                n += 1
        print("done with  %s %s" % (cat_nm, cat_id), file=out)
    print("done!", file=out)
    return n


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m disn_amd.postprocess",
                                description="remove small disconnected parts (postprocessing/clean_smallparts.py)")
    p.add_argument("--src_dir", required=True, help="src directory, before clean (<cat_id>/*.obj)")
    p.add_argument("--tar_dir", required=True, help="where to store")
    p.add_argument("--category", default="clean", help="all, clean or one category name [default: clean]")
    p.add_argument("--dist_thresh", type=float, default=0.5, help="largest centroid distance of a kept part [0.5]")
    p.add_argument("--num_thresh", type=float, default=0.3, help="smallest share of the largest part's vertices [0.3]")
    p.add_argument("--connectivity", default="face", choices=sorted(CONNECTIVITY), help="[default: face]")
    return p


def main(argv=None) -> int:
    from . import evaluate
    a = parser().parse_args(argv)
    return clean_meshes(evaluate.categories(a.category), a.src_dir, a.tar_dir, a.dist_thresh, a.num_thresh,
                        a.connectivity)


if __name__ == "__main__":
    main()

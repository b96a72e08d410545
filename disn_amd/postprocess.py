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
"vertex" connectivity (triangles that share a vertex) on request.  This file-to-file step is bound by reading and
writing the .obj files.  Its device part, for meshes that still lie on the device (``create_sdf --clean``,
``demo --clean``): ``separate_mesh_device``, ``clean_meshes_device`` and ``clean_arrays_device`` (mesh_clean.hip) give
the values of ``separate_mesh`` / ``clean_arrays`` without a file or a host copy of the meshes -- one read-back of
the [B,5] sizes per group.
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


# ---- the device path (mesh_clean.hip) --------------------------------------------------------------------------
STATUS_NOTHING_KEPT, STATUS_INDEX, STATUS_TABLE = 1, 2, 3


def _pack(parts, dtype, what: str):
    """[n_i,3] device tensors -> (one contiguous [sum n_i,3] tensor, offsets int64 [B+1]); views that already lie
    back to back in one allocation (``isosurface.marching_cubes_batch``) are taken as they are, anything else is
    concatenated"""
    import torch
    for t in parts:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.dim() == 2 and t.shape[1] == 3):
            raise TypeError("%s must be [n,3] %s CUDA tensors (the HIP path has no CPU fallback)"
                            % (what, str(dtype).replace("torch.", "")))
    off = np.zeros(len(parts) + 1, np.int64)
    off[1:] = np.cumsum([t.shape[0] for t in parts])
    total, first, size = int(off[-1]), parts[0], parts[0].element_size() * 3
    adjacent = all(t.is_contiguous() for t in parts) and all(
        a.untyped_storage().data_ptr() == first.untyped_storage().data_ptr()
        and b.data_ptr() == a.data_ptr() + a.shape[0] * size for a, b in zip(parts, parts[1:]))
    if adjacent and len(parts) > 1:
        whole = first.new_empty(0).set_(first.untyped_storage(), first.storage_offset(), (total, 3), (3, 1))
    elif len(parts) == 1:
        whole = first.contiguous()
    else:
        whole = torch.cat(list(parts), 0)
    return whole, off


def _clean_ws(B: int, nv: int, nf: int, device):
    from . import ops
    need = lib().disn_mesh_clean_workspace_bytes(B, nv, nf)
    if need == 0:
        raise ValueError("unsupported batch: %d meshes, %d vertices, %d triangles" % (B, nv, nf))
    return ops._ws(need, device)


def _connectivity(connectivity: str) -> int:
    if connectivity not in CONNECTIVITY:
        raise ValueError("connectivity must be 'face' or 'vertex' (got %r)" % (connectivity,))
    return CONNECTIVITY[connectivity]


def separate_mesh_device(verts, faces, connectivity: str = "face"):
    """``separate_mesh`` on the device -> (labels int32 [nf], vert_counts int64 [ncomp]), device tensors with the
    values of ``separate_mesh`` (disn_mesh_components_device; one read-back: the number of components)"""
    import torch

    from . import ops
    from ._lib import check
    conn = _connectivity(connectivity)
    (v, v_off), (f, f_off) = _pack([verts], torch.float32, "verts"), _pack([faces], torch.int32, "faces")
    nv, nf, dev = int(v_off[1]), int(f_off[1]), f.device
    labels = torch.empty(nf, dtype=torch.int32, device=dev)
    if nf == 0:
        return labels, torch.zeros(0, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        ws = _clean_ws(1, nv, nf, dev)
        ncomp = torch.zeros(1, dtype=torch.int64, device=dev)
        comp_verts = torch.zeros(nf, dtype=torch.int64, device=dev)
        check("disn_mesh_components_device", lib().disn_mesh_components_device(
            v.data_ptr(), f.data_ptr(), v_off.ctypes.data, f_off.ctypes.data, 1, conn, labels.data_ptr(),
            ncomp.data_ptr(), comp_verts.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream()))
        n = int(ncomp.item())
    if n == -STATUS_INDEX:
        raise ValueError("face index out of range (mesh of %d vertices)" % nv)
    if n < 0:
        raise RuntimeError("disn_mesh_components_device failed (status %d)" % -n)
    return labels, comp_verts[:n]


def clean_meshes_device(meshes, dist_thresh: float = 0.5, num_thresh: float = 0.3, connectivity: str = "face",
                        strict: bool = True):
    """``clean_arrays`` for a group of meshes that lie on the device.  ``meshes``: B x (verts [nv,3] float32, faces
    [nf,3] int32[, normals [nv,3]]) device tensors (the views ``isosurface.marching_cubes_batch`` returns are used in
    place).  ONE count call, ONE read-back of the [B,5] sizes, ONE emit call.
    -> (cleaned, kept): B x (verts', faces'[, normals']) views of the outputs, the bits of ``clean_arrays`` (further
    arrays ride along through the vertex map), and B int32 device tensors of kept component ids (left on the device:
    reading them is a second host sync).  An empty mesh stays empty.  A mesh of which nothing is kept raises
    ValueError -- or, with ``strict=False``, gives None in ``cleaned`` and no ids in ``kept``.  ValueError for a face
    index out of range."""
    import torch

    from . import ops
    from ._lib import check
    conn = _connectivity(connectivity)
    meshes = [tuple(m) for m in meshes]
    if not meshes:
        return [], []
    (v, v_off), (f, f_off) = (_pack([m[0] for m in meshes], torch.float32, "verts"),
                              _pack([m[1] for m in meshes], torch.int32, "faces"))
    B, nv, nf, dev = len(meshes), int(v_off[-1]), int(f_off[-1]), v.device
    h = lib()
    with torch.cuda.device(dev):
        ws = _clean_ws(B, nv, nf, dev)
        counts = torch.zeros((B, 5), dtype=torch.int64, device=dev)
        st = ops._stream()
        check("disn_mesh_clean_count_batch", h.disn_mesh_clean_count_batch(
            v.data_ptr(), f.data_ptr(), v_off.ctypes.data, f_off.ctypes.data, B, conn, float(dist_thresh),
            float(num_thresh), counts.data_ptr(), ws.data_ptr(), ws.numel(), st))
        sizes = np.ascontiguousarray(counts.cpu().numpy())      # the one host sync of the group
        for b in range(B):
            if sizes[b, 4] == STATUS_INDEX:
                raise ValueError("mesh %d: face index out of range (mesh of %d vertices)"
                                 % (b, v_off[b + 1] - v_off[b]))
            if sizes[b, 4] == STATUS_TABLE:
                raise RuntimeError("mesh %d: internal table full (disn_mesh_clean_count_batch)" % b)
            if sizes[b, 4] == STATUS_NOTHING_KEPT and strict:
                raise ValueError("mesh %d: no part is kept (dist_thresh %g, num_thresh %g): %d parts"
                                 % (b, dist_thresh, num_thresh, sizes[b, 0]))
        nk, nvo, nfo = (int(sizes[:, c].sum()) for c in (1, 2, 3))
        out_v = torch.empty((nvo, 3), dtype=torch.float32, device=dev)
        out_f = torch.empty((nfo, 3), dtype=torch.int32, device=dev)
        vmap = torch.empty(nvo, dtype=torch.int32, device=dev)
        kept_ids = torch.empty(nk, dtype=torch.int32, device=dev)
        if nk:
            check("disn_mesh_clean_emit_batch", h.disn_mesh_clean_emit_batch(
                v.data_ptr(), f.data_ptr(), v_off.ctypes.data, f_off.ctypes.data, sizes.ctypes.data, B,
                out_v.data_ptr(), out_f.data_ptr(), vmap.data_ptr(), kept_ids.data_ptr(), ws.data_ptr(), ws.numel(),
                st))
    cleaned, kept, k0, v0, f0 = [], [], 0, 0, 0
    for b, m in enumerate(meshes):
        nkb, nvb, nfb = (int(x) for x in sizes[b, 1:4])
        if sizes[b, 4] == STATUS_NOTHING_KEPT:
            cleaned.append(None)
            kept.append(kept_ids[k0:k0])
            continue
        rest = tuple(x.index_select(0, vmap[v0:v0 + nvb].long()) for x in m[2:])
        cleaned.append((out_v[v0:v0 + nvb], out_f[f0:f0 + nfb]) + rest)
        kept.append(kept_ids[k0:k0 + nkb])
        k0, v0, f0 = k0 + nkb, v0 + nvb, f0 + nfb
    return cleaned, kept


def clean_arrays_device(verts, faces, dist_thresh: float = 0.5, num_thresh: float = 0.3, connectivity: str = "face"):
    """``clean_arrays`` for one mesh on the device -> (verts, faces, kept component ids), device tensors with the
    bits of ``clean_arrays``; the same ValueErrors (no triangles, no part kept, index out of range)"""
    if faces.shape[0] == 0:
        raise ValueError("the mesh has no triangles")
    try:
        cleaned, kept = clean_meshes_device([(verts, faces)], dist_thresh, num_thresh, connectivity)
    except ValueError as e:
        msg = str(e)
        raise ValueError(msg[len("mesh 0: "):] if msg.startswith("mesh 0: ") else msg) from e
    return cleaned[0][0], cleaned[0][1], kept[0].tolist()


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

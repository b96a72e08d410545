"""Mesh extraction from the predicted SDF grid: the stage behind the hot path in
``test/create_sdf.py`` (create_obj :305-317, create_one_cube_obj :319-323), without the
``.dist`` file and the ``./isosurface/computeMarchingCubes`` subprocess.

``marching_cubes`` meshes the grid where it already lies (device tensor from
``create_sdf.dense_grid_sdf``); ``create_obj`` mirrors the reference helper's name and arguments
and writes ``<dir>/<cat_id>/<cat_id>_<obj_nm>_<view_id>.obj``.  The case table is derived in
``tools/gen_mc_tables.py``; the reference's closed binary cannot be compared against
(SURVEY §2 row 11): where a cell is topologically ambiguous its triangulation may differ, the
vertices (on grid edges, linear interpolation at ``iso``) do not.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import ops
from ._lib import check, lib


def marching_cubes(sdf: torch.Tensor, sdf_params, res: int, iso: float = 0.0,
                   ws: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """sdf: float32 device tensor with (res+1)^3 values in the flat (iz,iy,ix) order of the
    ``.dist`` format.  -> (verts [nv,3] float32, faces [nf,3] int32 0-based), on the device."""
    sdf = ops._chk(sdf.reshape(-1), "sdf")
    n = res + 1
    if sdf.numel() != n * n * n:
        raise ValueError("sdf must hold (res+1)^3 = %d values, got %d" % (n * n * n, sdf.numel()))
    dev = sdf.device
    with torch.cuda.device(dev):
        need = lib().disn_mc_workspace_bytes(res)
        if need == 0:
            raise ValueError("unsupported resolution %d" % res)
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        st = ops._stream()
        check("disn_mc_count", lib().disn_mc_count(sdf.data_ptr(), res, float(iso), counts.data_ptr(),
                                                   ws.data_ptr(), ws.numel(), st))
        nv, nf = (int(v) for v in counts.tolist())          # the one host sync: sizes are data dependent
        verts = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((nf, 3), dtype=torch.int32, device=dev)
        if nv and nf:
            p6 = ops._params6(sdf_params)
            check("disn_mc_emit", lib().disn_mc_emit(sdf.data_ptr(), C.byref(p6), res, float(iso),
                                                     verts.data_ptr(), faces.data_ptr(), ws.data_ptr(),
                                                     ws.numel(), st))
    return verts, faces


MC_EDGE_SLOTS = 1 << 32      # a batch's 3*B*(res+1)^3 edge slots must stay below this (the 32-bit scan)


def marching_cubes_batch(sdf: torch.Tensor, sdf_params, res: int, iso: float = 0.0,
                         ws: Optional[torch.Tensor] = None, max_edge_slots: int = MC_EDGE_SLOTS
                         ) -> List[Tuple[torch.Tensor, torch.Tensor]]:
    """sdf: float32 device tensor [B,(res+1)^3], sdf_params [B,6] -> B x (verts [nv,3], faces [nf,3]), views of
    two device tensors; every pair is bit for bit what ``marching_cubes`` gives for that grid alone.  One count
    call, ONE device-to-host copy of the [B,2] sizes and one emit call for the whole batch; a batch whose
    3*B*(res+1)^3 edge slots reach ``max_edge_slots`` is meshed in several such rounds."""
    n = res + 1
    if sdf.dim() != 2 or sdf.shape[1] != n * n * n:
        raise ValueError("sdf must be [B, (res+1)^3 = %d], got %s" % (n * n * n, tuple(sdf.shape)))
    sdf = ops._chk(sdf, "sdf")
    B = sdf.shape[0]
    sp = np.ascontiguousarray(np.asarray(sdf_params, np.float64).reshape(-1, 6))
    if sp.shape[0] != B:
        raise ValueError("sdf_params must be [B,6] with B = %d, got %s" % (B, sp.shape))
    per = (min(int(max_edge_slots), MC_EDGE_SLOTS) - 1) // (3 * n * n * n)      # grids per round
    if B and (per < 1 or lib().disn_mc_batch_workspace_bytes(1, res) == 0):
        raise ValueError("unsupported resolution %d" % res)
    dev = sdf.device
    out: List[Tuple[torch.Tensor, torch.Tensor]] = []
    with torch.cuda.device(dev):
        st = ops._stream()
        for b0 in range(0, B, max(per, 1)):
            nb = min(per, B - b0)
            need = lib().disn_mc_batch_workspace_bytes(nb, res)
            if ws is None or ws.numel() < need:
                ws = torch.empty(need, dtype=torch.uint8, device=dev)
            part = sdf[b0:b0 + nb]
            counts = torch.zeros((nb, 2), dtype=torch.int64, device=dev)
            check("disn_mc_count_batch", lib().disn_mc_count_batch(part.data_ptr(), nb, res, float(iso),
                                                                   counts.data_ptr(), ws.data_ptr(), ws.numel(), st))
            sizes = counts.cpu().numpy()                   # the one host sync of the round: sizes are data dependent
            nv, nf = int(sizes[:, 0].sum()), int(sizes[:, 1].sum())
            verts = torch.empty((nv, 3), dtype=torch.float32, device=dev)
            faces = torch.empty((nf, 3), dtype=torch.int32, device=dev)
            if nv and nf:
                check("disn_mc_emit_batch", lib().disn_mc_emit_batch(part.data_ptr(), sp[b0:b0 + nb].ctypes.data, nb,
                                                                     res, float(iso), verts.data_ptr(),
                                                                     faces.data_ptr(), ws.data_ptr(), ws.numel(), st))
            v0 = f0 = 0
            for k in range(nb):
                out.append((verts[v0:v0 + int(sizes[k, 0])], faces[f0:f0 + int(sizes[k, 1])]))
                v0 += int(sizes[k, 0])
                f0 += int(sizes[k, 1])
    return out


def write_obj(path: str, verts, faces, normals=None, colours=None) -> None:
    """Wavefront .obj ("v x y z" / "f a b c", 1-based).  With ``normals`` [nv,3]: one "vn x y z" line per vertex
    behind the vertices and faces "f a//a b//b c//c"; without, the plain file.  With ``colours`` uint8 [nv,3] (R G B):
    "v x y z r g b", r, g, b = c / 255 in four decimals (``read_obj_colours``; the readers of plain files stop after
    the third number of a "v" line and read these as they read the others)."""
    host = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    v = np.ascontiguousarray(host(verts), np.float32)
    f = np.ascontiguousarray(host(faces), np.int32)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    if normals is None and colours is None:
        check("disn_write_obj", lib().disn_write_obj(path.encode(), v.ctypes.data, v.shape[0], f.ctypes.data, f.shape[0]))
        return
    n = None
    if normals is not None:
        n = np.ascontiguousarray(host(normals), np.float32)
        if n.shape != v.shape:
            raise ValueError("normals must be [nv,3] like verts, got %s for %s" % (n.shape, v.shape))
    if colours is None:
        check("disn_write_obj_normals", lib().disn_write_obj_normals(path.encode(), v.ctypes.data, v.shape[0],
                                                                     n.ctypes.data, f.ctypes.data, f.shape[0]))
        return
    c = host(colours)
    if c.dtype != np.uint8 or c.shape != v.shape:
        raise ValueError("colours must be uint8 [nv,3] like verts, got %s %s for %s" % (c.dtype, c.shape, v.shape))
    c = np.ascontiguousarray(c)
    check("disn_write_obj_colours", lib().disn_write_obj_colours(path.encode(), v.ctypes.data, v.shape[0], c.ctypes.data,
                                                                 None if n is None else n.ctypes.data, f.ctypes.data,
                                                                 f.shape[0]))


def read_obj_colours(path: str) -> np.ndarray:
    """the colours of a coloured .obj as uint8 [nv,3]: rint(255 c) of the three numbers behind x y z on every "v" line
    (ValueError for a "v" line without them)"""
    cs = []
    for line in open(path):
        if line.startswith("v "):
            t = line.split()
            if len(t) < 7:
                raise ValueError("%s: a vertex without colour: %r" % (path, line.rstrip()))
            cs.append([float(x) for x in t[4:7]])
    return np.rint(np.asarray(cs, np.float64).reshape(-1, 3) * 255.0).astype(np.uint8)


def refine_mesh(engine, enc, image_index: int, trans_mat, verts, faces, sdf_params, res: int, iso: float = 0.0,
                iters: int = 2, sdf_weight: float = 10.0):
    """The vertices of a ``marching_cubes`` mesh of image ``image_index`` moved onto the network's own ``iso`` level
    set (``SdfEngine.refine_vertices``; the grid cell of ``sdf_params`` / ``res`` -- its shortest edge -- bounds a
    step by half and a vertex's way by one cell), with the unit gradient at the new positions as normals.
    -> (verts' [nv,3], faces (unchanged), normals [nv,3]).  ``iters`` = 0: the vertices as they are, their normals.
    WINDING: ``marching_cubes`` orders a triangle so that its geometric normal (b - a) x (c - a) points towards
    larger values (disn_mc_emit), i.e. ALONG +grad pred; the "vn" normals written here point the same way."""
    p = np.asarray(sdf_params, np.float64).reshape(6)
    cell = float(np.min((p[3:] - p[:3]) / float(res)))
    v, n, _ = engine.refine_vertices(enc, image_index, trans_mat, verts, iso=iso, iters=iters, sdf_weight=sdf_weight,
                                     cell=cell)
    return v, faces, n


def read_obj(path: str):
    vs, fs = [], []
    for line in open(path):
        if line.startswith("v "):
            vs.append([float(t) for t in line.split()[1:4]])
        elif line.startswith("f "):
            fs.append([int(t.split("/")[0]) - 1 for t in line.split()[1:4]])
    return np.asarray(vs, np.float32).reshape(-1, 3), np.asarray(fs, np.int32).reshape(-1, 3)


def read_obj_verts(path: str) -> np.ndarray:
    """the vertices of a Wavefront .obj as float32 [nv, 3], in file order (native reader, disn_read_obj_verts:
    what the evaluation driver loads; ``read_obj`` is the full Python reader)"""
    h = lib()
    nv = h.disn_read_obj_verts(path.encode(), None, 0)
    if nv < 0:
        raise OSError("cannot read vertices of %s" % path)
    v = np.empty((nv, 3), np.float32)
    if nv:
        got = h.disn_read_obj_verts(path.encode(), v.ctypes.data, nv)
        if got != nv:
            raise OSError("%s changed while it was read" % path)
    return v


def create_obj(pred_sdf_val, sdf_params, dir, cat_id, obj_nm, view_id, i, res: Optional[int] = None) -> str:
    """test/create_sdf.py:305-317 -- same arguments (``i`` is the iso value), same output path;
    ``pred_sdf_val`` may be a device tensor (preferred) or a numpy array of (res+1)^3 values."""
    if not isinstance(view_id, str):
        view_id = "%02d" % view_id
    out_dir = os.path.join(dir, cat_id)
    os.makedirs(out_dir, exist_ok=True)
    cube_obj_file = os.path.join(out_dir, cat_id + "_" + obj_nm + "_" + view_id + ".obj")
    if not isinstance(pred_sdf_val, torch.Tensor):
        pred_sdf_val = torch.from_numpy(np.ascontiguousarray(pred_sdf_val, np.float32)).cuda()
    n = round(pred_sdf_val.numel() ** (1.0 / 3.0))
    res = (n - 1) if res is None else res
    verts, faces = marching_cubes(pred_sdf_val, np.asarray(sdf_params, np.float64), res, float(i))
    write_obj(cube_obj_file, verts, faces)
    return cube_obj_file

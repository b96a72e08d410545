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

Not in the reference: simplification by quadric vertex clustering (``--simplify CELLS`` of ``create_sdf`` and ``demo``,
DESIGN 4za).  ``simplify_arrays`` is the rule, on the host; ``simplify_meshes_device`` / ``simplify_arrays_device``
(mesh_simplify.hip) give its integers and its position bits for meshes that lie on the device.
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


# ---- simplification by quadric vertex clustering: the rule (the device restates it, mesh_simplify.hip) ----
MAX_CELLS = 1024
_FIX = 4294967296.0            # 2^32: every accumulated real has magnitude <= 1 and is added as rint(x * 2^32), an int64
_QUADRIC = ((0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3))   # of w [n;d][n;d]^T


def simplify_lattice(box, cells: int) -> Tuple[np.ndarray, float]:
    """-> (origin float64 [3], h): the cubic lattice of ``cells`` cells of side h = max extent / cells along the box's
    longest axis, anchored at the box's minimum corner.  ValueError for ``cells`` outside 1..1024 or a box without
    extent."""
    if int(cells) != cells or not 1 <= int(cells) <= MAX_CELLS:
        raise ValueError("--simplify must be a number of cells in 1..%d, got %r" % (MAX_CELLS, cells))
    p = np.asarray(box, np.float64).reshape(-1)
    if p.size != 6 or not np.isfinite(p).all():
        raise ValueError("the box must be six finite numbers (x0, y0, z0, x1, y1, z1)")
    h = float(np.max(p[3:] - p[:3]) / np.float64(int(cells)))
    with np.errstate(all="ignore"):
        inv32 = np.float32(1.0 / h) if h > 0.0 else np.float32(0.0)
    if not (h > 0.0 and np.isfinite(h * h) and inv32 > 0.0 and np.isfinite(inv32)):
        raise ValueError("the box has no extent the lattice can be laid on (h = %r)" % h)
    return p[:3].copy(), h


def _simplify_cells(v: np.ndarray, origin: np.ndarray, h: float, cells: int) -> np.ndarray:
    """float32: floor((v - float32(origin)) * float32(1/h)), clamped to [0, cells-1] -> int64 [nv,3]"""
    o32, inv32 = origin.astype(np.float32), np.float32(1.0 / h)
    c = np.floor((v - o32[None, :]) * inv32)
    return np.minimum(np.maximum(c, np.float32(0.0)), np.float32(cells - 1)).astype(np.int64)


def _simplify_solve(acc: np.ndarray):
    """acc int64 [nc,14] (ten quadric entries, three sums of rel, the member count) -> (x, m) float64 [nc,3]: the
    regularised minimiser in the operation order the kernel restates, and the members' mean"""
    s = acc[:, :13].astype(np.float64) * (1.0 / _FIX)
    axx, axy, axz, bx, ayy, ayz, by, azz, bz = (s[:, k] for k in range(9))
    n = acc[:, 13].astype(np.float64)
    mx, my, mz = s[:, 10] / n, s[:, 11] / n, s[:, 12] / n
    lam = (((axx + ayy) + azz) * 0.0009765625) / 3.0 + 9.094947017729282e-13          # 2^-10 tr / 3 + 2^-40
    m00, m11, m22 = axx + lam, ayy + lam, azz + lam
    m01, m02, m12 = axy, axz, ayz
    r0, r1, r2 = lam * mx - bx, lam * my - by, lam * mz - bz
    c00 = m11 * m22 - m12 * m12
    c01 = m02 * m12 - m01 * m22
    c02 = m01 * m12 - m02 * m11
    c11 = m00 * m22 - m02 * m02
    c12 = m01 * m02 - m00 * m12
    c22 = m00 * m11 - m01 * m01
    det = (m00 * c00 + m01 * c01) + m02 * c02
    with np.errstate(all="ignore"):
        x0 = ((c00 * r0 + c01 * r1) + c02 * r2) / det
        x1 = ((c01 * r0 + c11 * r1) + c12 * r2) / det
        x2 = ((c02 * r0 + c12 * r1) + c22 * r2) / det
    ok = (det > 0.0) & np.isfinite(x0) & np.isfinite(x1) & np.isfinite(x2)
    m = np.stack([mx, my, mz], 1)
    return np.where(ok[:, None], np.stack([x0, x1, x2], 1), m), m


def simplify_arrays(verts, faces, box, cells: int, dedup: bool = True, placement: str = "qef"
                    ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """Simplification by vertex clustering with quadric placement, on the host: THE SPECIFICATION of
    ``simplify_meshes_device`` (same integers, same position bits).
    -> (verts' float32 [nc,3], faces' int32 [nf',3], vmap int32 [nv], first int32 [nc]).

    Lattice: ``simplify_lattice(box, cells)``; a vertex's cell per axis is floor((v - float32(origin)) * float32(1/h))
    in float32, clamped to [0, cells-1]; the vertices of one cell are a cluster.  Clusters are numbered by their
    smallest member ``first[new]``; ``vmap[old]`` is a vertex's cluster.  A face whose three clusters are not distinct
    is dropped; with ``dedup`` only the smallest face index survives among the faces of one unordered cluster triple;
    survivors keep their order and their orientation.
    Position, in cell units about the cell centre: rel = clip((v - centre) / h, -1/2, 1/2) in float64.  A face with
    normal n = (b - a) x (c - a) (float64; |n| = 0 or not finite: no contribution), unit normal n^ and weight
    w = min(|n| / h^2, 1) adds, once to each of its distinct clusters, the ten entries of w [n^;d][n^;d]^T with
    d = -n^ . rel(its first corner in that cluster); every member vertex adds its rel and 1.  Every real is added as
    rint(x 2^32) in int64: the sums do not depend on the order.  x solves (A + lam I) x = -b + lam m, m = the mean
    rel, lam = 2^-10 tr(A) / 3 + 2^-40, by the adjugate (``_simplify_solve``); det <= 0 or x not finite: x = m.  x is
    clipped to the cell and v' = float32(centre + h x).  ``placement`` = "mean" puts every cluster on m instead (the
    comparison of DESIGN 4za; the device has no such mode).
    ValueError for a face index out of range or a coordinate that is not finite."""
    if placement not in ("qef", "mean"):
        raise ValueError("placement must be 'qef' or 'mean'")
    v, f = _host(verts, faces)
    origin, h = simplify_lattice(box, cells)
    cells = int(cells)
    nv, nf = v.shape[0], f.shape[0]
    if nf and (f.min() < 0 or f.max() >= nv):
        raise ValueError("face index out of range (mesh of %d vertices)" % nv)
    if not np.isfinite(v).all():
        raise ValueError("a vertex coordinate is not finite")
    if nv == 0:
        return v, f, np.zeros(0, np.int32), np.zeros(0, np.int32)
    cell = _simplify_cells(v, origin, h, cells)
    key = (cell[:, 0] * cells + cell[:, 1]) * cells + cell[:, 2]
    _, first_of, inverse = np.unique(key, return_index=True, return_inverse=True)
    order = np.argsort(first_of, kind="stable")
    rank = np.empty(order.size, np.int64)
    rank[order] = np.arange(order.size)
    vmap = rank[inverse.reshape(-1)]
    first = first_of[order]
    nc = first.size
    centre = origin[None, :] + (cell.astype(np.float64) + 0.5) * h
    rel = np.minimum(np.maximum((v.astype(np.float64) - centre) / h, -0.5), 0.5)
    acc = np.zeros((nc, 14), np.int64)
    member = np.concatenate([np.rint(rel * _FIX).astype(np.int64), np.ones((nv, 1), np.int64)], 1)
    np.add.at(acc[:, 10:], vmap, member)
    g = vmap[f]                                                     # [nf,3] clusters of the corners
    if nf:
        p = v.astype(np.float64)
        a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
        with np.errstate(all="ignore"):
            ux, uy, uz = (b[:, k] - a[:, k] for k in range(3))
            wx, wy, wz = (c[:, k] - a[:, k] for k in range(3))
            nx, ny, nz = uy * wz - uz * wy, uz * wx - ux * wz, ux * wy - uy * wx
            ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
            good = np.isfinite(ln) & (ln > 0.0)
            safe = np.where(good, ln, 1.0)
            hx, hy, hz = nx / safe, ny / safe, nz / safe
            w = np.minimum(ln / (h * h), 1.0)
        for k in range(3):
            fresh = good.copy()
            for j in range(k):
                fresh &= g[:, k] != g[:, j]
            r = rel[f[fresh, k]]
            q = [hx[fresh], hy[fresh], hz[fresh], None]
            q[3] = -((q[0] * r[:, 0] + q[1] * r[:, 1]) + q[2] * r[:, 2])
            wq = w[fresh]
            contrib = np.stack([np.rint(((wq * q[i]) * q[j]) * _FIX) for i, j in _QUADRIC], 1).astype(np.int64)
            np.add.at(acc[:, :10], g[fresh, k], contrib)
    x, m = _simplify_solve(acc)
    if placement == "mean":
        x = m
    x = np.minimum(np.maximum(x, -0.5), 0.5)
    out_v = (centre[first] + h * x).astype(np.float32)
    keep = (g[:, 0] != g[:, 1]) & (g[:, 1] != g[:, 2]) & (g[:, 0] != g[:, 2])
    if dedup and keep.any():
        ids = np.nonzero(keep)[0]
        _, lowest = np.unique(np.sort(g[ids], 1), axis=0, return_index=True)     # ids ascend: the first is the smallest
        keep = np.zeros(nf, bool)
        keep[ids[lowest]] = True
    return out_v, g[keep].astype(np.int32).reshape(-1, 3), vmap.astype(np.int32), first.astype(np.int32)


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


# ---- simplification on the device (mesh_simplify.hip) ----------------------------------------------------------
STATUS_FINITE, STATUS_CAPACITY = 4, 5


def simplify_meshes_device(meshes, boxes, cells, dedup: bool = True):
    """``simplify_arrays`` for a group of meshes that lie on the device.  ``meshes``: B x (verts [nv,3] float32, faces
    [nf,3] int32[, further per-vertex arrays]) device tensors (the views ``isosurface.marching_cubes_batch`` and
    ``clean_meshes_device`` return are used in place); ``boxes`` [B,6], each mesh's own; ``cells`` one number or B.
    ONE count call, ONE read-back of the [B,4] sizes, ONE emit call.
    -> (simplified, maps): B x (verts', faces'[, arrays']) views of the outputs -- the integers and the position bits
    of ``simplify_arrays``; a further array takes, for every output vertex, the row of the cluster's smallest member
    (``first``) -- and B x (vmap int32 [nv], first int32 [nv']) device tensors.  An empty mesh stays empty.
    ValueError for a face index out of range or a coordinate that is not finite."""
    import torch

    from . import ops
    from ._lib import check
    meshes = [tuple(m) for m in meshes]
    if not meshes:
        return [], []
    B = len(meshes)
    boxes = np.asarray(boxes, np.float64).reshape(-1, 6)
    if boxes.shape[0] != B:
        raise ValueError("%d boxes for %d meshes" % (boxes.shape[0], B))
    cells_in = np.broadcast_to(np.asarray(cells), (B,))
    lattice = np.empty((B, 4), np.float64)
    for b in range(B):
        lattice[b, :3], lattice[b, 3] = simplify_lattice(boxes[b], cells_in[b])       # (checks the cells too)
    cells_h = np.ascontiguousarray(cells_in, np.int32)
    (v, v_off), (f, f_off) = (_pack([m[0] for m in meshes], torch.float32, "verts"),
                              _pack([m[1] for m in meshes], torch.int32, "faces"))
    nv, nf, dev = int(v_off[-1]), int(f_off[-1]), v.device
    h = lib()
    with torch.cuda.device(dev):
        need = h.disn_mesh_simplify_workspace_bytes(B, nv, nf)
        if need == 0:
            raise ValueError("unsupported batch: %d meshes, %d vertices, %d triangles" % (B, nv, nf))
        ws = ops._ws(need, dev)
        counts = torch.zeros((B, 4), dtype=torch.int64, device=dev)
        st = ops._stream()
        check("disn_mesh_simplify_count_batch", h.disn_mesh_simplify_count_batch(
            v.data_ptr(), f.data_ptr(), v_off.ctypes.data, f_off.ctypes.data, lattice.ctypes.data, cells_h.ctypes.data,
            B, 1 if dedup else 0, counts.data_ptr(), ws.data_ptr(), ws.numel(), st))
        sizes = np.ascontiguousarray(counts.cpu().numpy())      # the one host sync of the group
        for b in range(B):
            if sizes[b, 3] == STATUS_INDEX:
                raise ValueError("mesh %d: face index out of range (mesh of %d vertices)"
                                 % (b, v_off[b + 1] - v_off[b]))
            if sizes[b, 3] == STATUS_FINITE:
                raise ValueError("mesh %d: a vertex coordinate is not finite" % b)
            if sizes[b, 3] == STATUS_TABLE:
                raise RuntimeError("mesh %d: internal table full (disn_mesh_simplify_count_batch)" % b)
            if sizes[b, 3] == STATUS_CAPACITY:
                raise RuntimeError("mesh %d: more than 2^21 clusters in one batch with dedup: simplify fewer meshes "
                                   "per call" % b)
            if sizes[b, 3] != 0:
                raise RuntimeError("mesh %d: disn_mesh_simplify_count_batch gave status %d" % (b, sizes[b, 3]))
        nvo, nfo = int(sizes[:, 0].sum()), int(sizes[:, 1].sum())
        out_v = torch.empty((nvo, 3), dtype=torch.float32, device=dev)
        out_f = torch.empty((nfo, 3), dtype=torch.int32, device=dev)
        vmap = torch.empty(nv, dtype=torch.int32, device=dev)
        first = torch.empty(nvo, dtype=torch.int32, device=dev)
        if nv:
            check("disn_mesh_simplify_emit_batch", h.disn_mesh_simplify_emit_batch(
                v.data_ptr(), f.data_ptr(), v_off.ctypes.data, f_off.ctypes.data, B, sizes.ctypes.data,
                out_v.data_ptr(), out_f.data_ptr(), vmap.data_ptr(), first.data_ptr(), ws.data_ptr(), ws.numel(), st))
    simplified, maps, v0, f0 = [], [], 0, 0
    for b, m in enumerate(meshes):
        nvb, nfb = int(sizes[b, 0]), int(sizes[b, 1])
        fi = first[v0:v0 + nvb]
        rest = tuple(x.index_select(0, fi.long()) for x in m[2:])
        simplified.append((out_v[v0:v0 + nvb], out_f[f0:f0 + nfb]) + rest)
        maps.append((vmap[int(v_off[b]):int(v_off[b + 1])], fi))
        v0, f0 = v0 + nvb, f0 + nfb
    return simplified, maps


def simplify_arrays_device(verts, faces, box, cells: int, dedup: bool = True):
    """``simplify_arrays`` for one mesh on the device -> (verts', faces', vmap, first), device tensors with the
    integers and the position bits of ``simplify_arrays``; the same ValueErrors"""
    try:
        simplified, maps = simplify_meshes_device([(verts, faces)], [box], cells, dedup)
    except ValueError as e:
        msg = str(e)
        raise ValueError(msg[len("mesh 0: "):] if msg.startswith("mesh 0: ") else msg) from e
    return simplified[0][0], simplified[0][1], maps[0][0], maps[0][1]


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

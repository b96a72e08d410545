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

Not in the reference either: vertex colours from the input views (``--colour`` of ``create_sdf`` and ``demo``, DESIGN
4zb).  ``zbuffer_arrays`` / ``colour_arrays`` are the rule, on the host; ``zbuffer_meshes_device``,
``colour_meshes_device`` and ``colour_arrays_device`` (mesh_colour.hip) give its depth bits and its colour bytes for
meshes that lie on the device.

Not in the reference either: fairing by Taubin's lambda|mu smoothing (``--smooth ITERS`` of ``create_sdf`` and ``demo``,
DESIGN 4zd).  ``smooth_arrays`` is the rule, on the host; ``smooth_meshes_device`` / ``smooth_arrays_device``
(mesh_smooth.hip) give its position bits for meshes that lie on the device.

Not in the reference either: checks of a mesh's topology, orientation and self-intersections (``--check`` of
``create_sdf`` and ``demo``, ``evaluate mesh_check``).  ``check_arrays`` is the rule, on the host;
``check_meshes_device`` / ``check_arrays_device`` (mesh_check.hip) give its integers for meshes that lie on the device.
They measure and repair nothing.

Not in the reference either: repair of a mesh to a manifold -- weld, drop, stitch and split (``--repair`` of
``create_sdf`` and ``demo``).  ``repair_arrays`` is the rule, on the host; ``repair_meshes_device`` /
``repair_arrays_device`` (mesh_repair.hip) give its integers and its position bits for meshes that lie on the device.
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


# ---- Taubin smoothing: the rule (the device restates it, mesh_smooth.hip) -------------------------------
SMOOTH_MAX_ITERS = 64
SMOOTH_RANGE = 1024.0          # a coordinate beyond it, at input or after a step: status 7
SMOOTH_MAX_DEGREE = 1 << 20    # with the range: every sum of neighbours stays below 2^20 2^10 2^32 = 2^62
STATUS_SMOOTH_RANGE = 7


def smooth_params(iters=10, lam=0.5, mu=-0.53, max_move=None):
    """-> (iters, lam, mu, max_move) checked: ``iters`` an integer in 1..64, 0 < ``lam`` <= 1, -1.5 <= ``mu`` < 0,
    ``max_move`` None or finite and >= 0 (a scalar or an array); ValueError otherwise"""
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or not 1 <= int(iters) <= SMOOTH_MAX_ITERS:
        raise ValueError("smooth: iters must be an integer in 1..%d, got %r" % (SMOOTH_MAX_ITERS, iters))
    try:
        lam, mu = float(lam), float(mu)
    except (TypeError, ValueError):
        raise ValueError("smooth: lam and mu must be numbers, got %r and %r" % (lam, mu)) from None
    if not 0.0 < lam <= 1.0:
        raise ValueError("smooth: lam must lie in (0, 1], got %r" % lam)
    if not -1.5 <= mu < 0.0:
        raise ValueError("smooth: mu must lie in [-1.5, 0), got %r" % mu)
    if max_move is not None:
        try:
            r = np.asarray(max_move, np.float64)
        except (TypeError, ValueError):
            raise ValueError("smooth: max_move must be None or finite and >= 0, got %r" % (max_move,)) from None
        if not (np.isfinite(r).all() and (r >= 0.0).all()):
            raise ValueError("smooth: max_move must be None or finite and >= 0, got %r" % (max_move,))
        max_move = float(r) if r.ndim == 0 else r
    return int(iters), lam, mu, max_move


def smooth_graph(faces, nv: int):
    """the edges of the rule -> (indptr int64 [nv+1], nbr int64 [2 E], boundary bool [nv]): row i of the CSR holds the
    distinct neighbours of i, ascending; an undirected edge counts once however many faces hold it, a corner pair
    (i, i) not at all; a vertex is on the boundary when one of its edges is held by exactly one corner pair"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b = f[:, (0, 1, 2)].reshape(-1), f[:, (1, 2, 0)].reshape(-1)
    proper = a != b
    lo, hi = np.minimum(a, b)[proper], np.maximum(a, b)[proper]
    key, held = np.unique(lo * np.int64(max(nv, 1)) + hi, return_counts=True)
    lo, hi = key // max(nv, 1), key % max(nv, 1)
    boundary = np.zeros(nv, bool)
    boundary[lo[held == 1]] = True
    boundary[hi[held == 1]] = True
    src, dst = np.concatenate([lo, hi]), np.concatenate([hi, lo])
    order = np.lexsort((dst, src))
    indptr = np.zeros(nv + 1, np.int64)
    indptr[1:] = np.cumsum(np.bincount(src, minlength=nv))
    return indptr, dst[order], boundary


def smooth_status(verts, faces) -> int:
    """the status of a mesh BEFORE its first step: the largest of 2 (a face index outside the mesh), 4 (a coordinate that
    is not finite), 7 (a finite coordinate beyond +-1024; more than 2^20 distinct neighbours at a vertex of a mesh that
    is otherwise in order); 0 when none applies"""
    v, f = _host(verts, faces)
    status = 0
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        status = STATUS_INDEX
    finite = np.isfinite(v)
    if not finite.all():
        status = max(status, STATUS_FINITE)
    if (np.abs(v[finite]) > np.float32(SMOOTH_RANGE)).any():
        status = STATUS_SMOOTH_RANGE
    if status == 0 and f.size and np.diff(smooth_graph(f, v.shape[0])[0]).max() > SMOOTH_MAX_DEGREE:
        status = STATUS_SMOOTH_RANGE
    return status


def smooth_arrays_status(verts, faces, iters=10, lam=0.5, mu=-0.53, pin_boundary=True, max_move=None
                         ) -> Tuple[np.ndarray, int]:
    """``smooth_arrays`` with the status word instead of the exceptions -> (verts', status): a mesh with a status keeps
    its input vertices, as on the device"""
    iters, lam, mu, max_move = smooth_params(iters, lam, mu, max_move)
    if max_move is not None and np.ndim(max_move):
        raise ValueError("smooth: one mesh takes one max_move")
    v0, f = _host(verts, faces)
    nv = v0.shape[0]
    status = smooth_status(v0, f)
    if status or nv == 0:
        return v0.copy(), status
    indptr, nbr, boundary = smooth_graph(f, nv)
    deg = np.diff(indptr)
    movable = deg > 0
    if pin_boundary:
        movable &= ~boundary
    rows = np.nonzero(movable)[0]
    n = deg[rows].astype(np.float64)[:, None]
    x0 = v0.astype(np.float64)
    cur = v0.copy()
    for t in range(2 * iters):
        s = lam if t % 2 == 0 else mu
        q = np.rint(cur.astype(np.float64) * _FIX).astype(np.int64)
        run = np.zeros((nbr.size + 1, 3), np.int64)
        np.cumsum(q[nbr], axis=0, out=run[1:])                  # int64: exact, whatever the order
        S = run[indptr[rows + 1]] - run[indptr[rows]]
        m = (S.astype(np.float64) * (1.0 / _FIX)) / n
        x = cur[rows].astype(np.float64)
        y = x + s * (m - x)
        if max_move is not None:
            y = np.minimum(np.maximum(y, x0[rows] - max_move), x0[rows] + max_move)
        new = y.astype(np.float32)
        if (np.abs(new) > np.float32(SMOOTH_RANGE)).any():
            return v0.copy(), STATUS_SMOOTH_RANGE
        cur = cur.copy()
        cur[rows] = new
    return cur, 0


def smooth_arrays(verts, faces, iters=10, lam=0.5, mu=-0.53, pin_boundary=True, max_move=None) -> np.ndarray:
    """Taubin lambda|mu smoothing on the host: THE SPECIFICATION of ``smooth_meshes_device`` (same position bits).
    -> verts' float32 [nv,3]; the faces never change.

    Edges: every face gives its three corner pairs, a pair of equal indices is ignored (degenerate faces are legal), an
    undirected edge {i, j} counts once however many faces hold it; N(i) the distinct neighbours of i, deg(i) = |N(i)|.
    An edge held by exactly ONE corner pair of the whole mesh is a boundary edge, its two ends boundary vertices.  A
    vertex moves when deg(i) > 0 and it is no pinned boundary vertex (``pin_boundary``); any other vertex keeps its
    input bits.  2 ``iters`` Jacobi steps, step t with the factor s = ``lam`` (t even) or ``mu`` (t odd), every vertex
    from the positions of the step before:  q(x) = int64(rint(float64(x) 2^32));  S_i = sum of q(v_j) over N(i), an
    int64 sum, so its order does not matter;  m_i = (float64(S_i) 2^-32) / float64(deg(i));  v'_i = float32(float64(v_i)
    + s (m_i - float64(v_i))) in float64 exactly as written.  ``max_move`` = r: after every step each coordinate is
    clamped in float64 to [float64(v0_i) - r, float64(v0_i) + r], v0 the input position, before the cast -- a box, not
    a ball.  ValueError (the device: the status word) for a face index outside the mesh (2), a coordinate that is not
    finite (4), and for a coordinate beyond +-1024 at input or after any step or a vertex of more than 2^20 neighbours
    (7: ``smooth_arrays_status``); ValueError for parameters outside ``smooth_params``' ranges."""
    out, status = smooth_arrays_status(verts, faces, iters, lam, mu, pin_boundary, max_move)
    if status == STATUS_SMOOTH_RANGE:
        raise ValueError("a coordinate leaves +-%g (at input or after a step), or a vertex has more than 2^20 neighbours"
                         % SMOOTH_RANGE)
    _one_mesh(_raise_status, 0, status, [0, out.shape[0]], "smooth_arrays")
    return out


# ---- mesh checks: the rule (the device restates it, mesh_check.hip) ------------------------------------
CHECK_FIELDS = ("nv", "nf", "unreferenced_vertices", "index_degenerate_faces", "edges", "boundary_edges",
                "nonmanifold_edges", "misoriented_edges", "nonmanifold_vertices", "euler", "zero_area_faces",
                "candidate_pairs", "intersecting_pairs", "intersecting_faces")      # DISN_CHECK_NV .. in this order
CHECK_PAIRS_PER_FACE = 256     # the default work cap of a mesh: CHECK_PAIRS_PER_FACE nf + CHECK_PAIRS_BASE candidate pairs
CHECK_PAIRS_BASE = 4096
STATUS_CHECK_PAIRS = 8
FLAG_INTERSECTS, FLAG_DEGENERATE, FLAG_BOUNDARY, FLAG_NONMANIFOLD, FLAG_MISORIENTED = 1, 2, 4, 8, 16
_CHECK_TOPOLOGY, _CHECK_GEOMETRY = CHECK_FIELDS[2:10], CHECK_FIELDS[10:]


def check_max_pairs(max_pairs, nf: int) -> int:
    """the work cap of one mesh: ``max_pairs`` candidate pairs, by default CHECK_PAIRS_PER_FACE nf + CHECK_PAIRS_BASE"""
    cap = CHECK_PAIRS_PER_FACE * int(nf) + CHECK_PAIRS_BASE if max_pairs is None else int(max_pairs)
    if cap < 0:
        raise ValueError("check: max_pairs must be >= 0 (got %r)" % (max_pairs,))
    return cap


def check_orient(a, b, c, d):
    """the float64 determinant of [b - a, c - a, d - a], expanded along its first row:
    (u0 (v1 w2 - v2 w1) - u1 (v0 w2 - v2 w0)) + u2 (v0 w1 - v1 w0), every product and difference rounded once"""
    u, v, w = b - a, c - a, d - a
    return ((u[..., 0] * (v[..., 1] * w[..., 2] - v[..., 2] * w[..., 1])
             - u[..., 1] * (v[..., 0] * w[..., 2] - v[..., 2] * w[..., 0]))
            + u[..., 2] * (v[..., 0] * w[..., 1] - v[..., 1] * w[..., 0]))


def _check_pierces(P, T):
    """[n] bool: an edge (p, q) of triangle P[n] goes through the inside of triangle T[n] (float64 [n,3,3])"""
    a, b, c = T[:, 0], T[:, 1], T[:, 2]
    hit = np.zeros(P.shape[0], bool)
    for k in range(3):
        p, q = P[:, k], P[:, (k + 1) % 3]
        across = check_orient(a, b, c, p) * check_orient(a, b, c, q) < 0
        s1, s2, s3 = check_orient(p, q, a, b), check_orient(p, q, b, c), check_orient(p, q, c, a)
        hit |= across & (((s1 > 0) & (s2 > 0) & (s3 > 0)) | ((s1 < 0) & (s2 < 0) & (s3 < 0)))
    return hit


def _check_candidates(lo, hi):
    """the pairs i < j of boxes [lo, hi] (float32 [n,3]) that overlap, closed -> (i, j), int64 each; a sweep along x"""
    order = np.argsort(lo[:, 0], kind="stable")
    I, J = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for n, i in enumerate(order):
        j = order[n + 1:]
        j = j[:np.searchsorted(lo[j, 0], hi[i, 0], side="right")]
        j = j[np.all((lo[j] <= hi[i]) & (lo[i] <= hi[j]), axis=1)]
        I.append(np.minimum(i, j))
        J.append(np.maximum(i, j))
    return np.concatenate(I), np.concatenate(J)


def _check_fans(f: np.ndarray, key: np.ndarray, lo_first: np.ndarray, nv: int) -> int:
    """the vertices with two or more fans.  f [n,3] the faces that take part, key [3n] the undirected edge of corner pair
    (face, k) -> (k+1)%3 in face-major order, lo_first [3n]: that pair runs from its smaller index"""
    n3 = key.size
    parent = np.arange(n3)

    def root(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    corner = np.arange(n3)
    nxt = corner - corner % 3 + (corner % 3 + 1) % 3             # the corner of the pair's second index, same face
    at_lo, at_hi = np.where(lo_first, corner, nxt), np.where(lo_first, nxt, corner)
    order = np.argsort(key, kind="stable")
    same = np.nonzero(key[order][1:] == key[order][:-1])[0]
    for k in same:                                               # two corner pairs of one edge: their faces share it
        for at in (at_lo, at_hi):
            a, b = root(at[order[k]]), root(at[order[k + 1]])
            if a != b:
                parent[max(a, b)] = min(a, b)
    roots = np.array([root(x) for x in range(n3)], np.int64)
    fans = np.bincount(f.reshape(-1)[np.unique(roots)], minlength=nv)
    return int((fans >= 2).sum())


def _check_derive(out: dict) -> dict:
    """the four derived booleans; an invalid field (-1) makes its boolean False"""
    out["closed"] = out["boundary_edges"] == 0
    out["manifold"] = out["nonmanifold_edges"] == 0 and out["nonmanifold_vertices"] == 0
    out["oriented"] = out["misoriented_edges"] == 0
    out["watertight"] = (out["closed"] and out["manifold"] and out["oriented"] and out["intersecting_pairs"] == 0
                         and out["status"] == 0)
    return out


def _check(verts, faces, max_pairs=None) -> Tuple[dict, np.ndarray]:
    v32 = np.ascontiguousarray(verts.detach().cpu().numpy() if hasattr(verts, "detach") else verts,
                               np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces.detach().cpu().numpy() if hasattr(faces, "detach") else faces).reshape(-1, 3)
    f = f.astype(np.int64)
    nv, nf = v32.shape[0], f.shape[0]
    cap = check_max_pairs(max_pairs, nf)
    out = {"status": 0}
    out.update((k, 0) for k in CHECK_FIELDS)
    out.update(nv=nv, nf=nf, area=0.0, volume=0.0)
    flags = np.zeros(nf, np.uint8)

    def done():
        return _check_derive(out), flags

    if nf and (f.min() < 0 or f.max() >= nv):
        out["status"] = STATUS_INDEX
        out.update((k, -1) for k in _CHECK_TOPOLOGY + _CHECK_GEOMETRY)
        return done()
    finite = bool(np.isfinite(v32).all())
    # -- topology: the indices alone
    part = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])
    ids = np.nonzero(part)[0]
    g = f[part]
    flags[~part] |= FLAG_DEGENERATE
    referenced = np.zeros(nv, bool)
    referenced[g.reshape(-1)] = True
    a, b = g.reshape(-1), g[:, (1, 2, 0)].reshape(-1)             # corner pair 3 n + k: index k -> index (k+1)%3
    key = np.minimum(a, b) * np.int64(max(nv, 1)) + np.maximum(a, b)
    uniq, inv, held = np.unique(key, return_inverse=True, return_counts=True)
    forward = np.bincount(inv.reshape(-1), weights=(a < b), minlength=uniq.size).astype(np.int64)
    boundary, nonmanifold = held == 1, held >= 3
    misoriented = (held == 2) & (forward != 1)
    for mark, bit in ((boundary, FLAG_BOUNDARY), (nonmanifold, FLAG_NONMANIFOLD), (misoriented, FLAG_MISORIENTED)):
        on = mark[inv.reshape(-1)].reshape(-1, 3).any(axis=1)
        flags[ids[on]] |= bit
    out.update(unreferenced_vertices=int(nv - referenced.sum()), index_degenerate_faces=int(nf - g.shape[0]),
               edges=int(uniq.size), boundary_edges=int(boundary.sum()), nonmanifold_edges=int(nonmanifold.sum()),
               misoriented_edges=int(misoriented.sum()), nonmanifold_vertices=_check_fans(g, key, a < b, nv),
               euler=int(referenced.sum()) - int(uniq.size) + int(g.shape[0]))
    if not finite:
        out["status"] = STATUS_FINITE
        out.update((k, -1) for k in _CHECK_GEOMETRY)
        return done()
    # -- geometry: float64 arithmetic on the float32 coordinates
    p = v32.astype(np.float64)[g]                                 # [n,3,3]
    u, w = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    cross = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                      u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)
    flat = (cross == 0).all(axis=1)
    flags[ids[flat]] |= FLAG_DEGENERATE
    out["zero_area_faces"] = int(flat.sum())
    out["area"] = float(np.sum(0.5 * np.sqrt((cross[:, 0] * cross[:, 0] + cross[:, 1] * cross[:, 1])
                                             + cross[:, 2] * cross[:, 2])))
    out["volume"] = float(np.sum(_check_volume_terms(p)))
    # -- self-intersections
    t32 = v32[g]
    I, J = _check_candidates(t32.min(axis=1), t32.max(axis=1))
    out["candidate_pairs"] = int(I.size)
    if I.size > cap:
        out["status"] = STATUS_CHECK_PAIRS
        out["intersecting_pairs"] = out["intersecting_faces"] = -1
        return done()
    hit = _check_pierces(p[I], p[J]) | _check_pierces(p[J], p[I])
    out["intersecting_pairs"] = int(hit.sum())
    faces_hit = np.unique(np.concatenate([I[hit], J[hit]]))
    out["intersecting_faces"] = int(faces_hit.size)
    flags[ids[faces_hit]] |= FLAG_INTERSECTS
    return done()


def _check_volume_terms(p: np.ndarray) -> np.ndarray:
    """p0 . (p1 x p2) / 6 of every triangle p [n,3,3] float64: ((x0 c0 + y0 c1) + z0 c2) / 6, c = p1 x p2"""
    a, b, c = p[:, 0], p[:, 1], p[:, 2]
    c0 = b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]
    c1 = b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2]
    c2 = b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0]
    return ((a[:, 0] * c0 + a[:, 1] * c1) + a[:, 2] * c2) / 6.0


def check_arrays(verts, faces, max_pairs=None) -> dict:
    """Topology, orientation and self-intersections of one mesh on the host: THE SPECIFICATION of
    ``check_meshes_device`` (same integers; ``area`` and ``volume`` up to the order of their sums).  -> a dict of
    ``status``, the CHECK_FIELDS, ``area``, ``volume`` and four derived booleans.  It repairs nothing.

    Status: 0; 2 a face index outside [0, nv): only nv and nf are valid; 4 a coordinate that is not finite: the
    topological fields are valid, the geometric ones not; 8 (STATUS_CHECK_PAIRS) more than ``max_pairs`` candidate
    pairs: ``intersecting_pairs`` and ``intersecting_faces`` are invalid.  Of several the largest; an invalid count is
    -1, an invalid sum 0.0.  An empty mesh has status 0 and zeros.

    Topology (the indices alone).  A face with a repeated index counts in ``index_degenerate_faces`` and takes no
    further part.  Every other face gives three corner pairs (a, b), (b, c), (c, a).  ``unreferenced_vertices``: named
    by no face that takes part.  ``edges``: distinct undirected {i, j}; ``boundary_edges``: held by exactly one corner
    pair; ``nonmanifold_edges``: by three or more; ``misoriented_edges``: by exactly two that run the same way.
    ``nonmanifold_vertices``: two corners (f, i), (g, i) of vertex i are related when f and g share an undirected edge
    {i, j}, however many faces it has; a fan is a class of the transitive closure; the field counts the vertices with
    two or more fans.  ``euler`` = referenced vertices - edges + faces that take part.

    Geometry, in float64 on the float32 coordinates, + - * and sqrt only, each rounded once, in the order written.
    cross = (p1 - p0) x (p2 - p0) = (u1 w2 - u2 w1, u2 w0 - u0 w2, u0 w1 - u1 w0); ``zero_area_faces``: faces that take
    part whose cross is (0, 0, 0), either sign; ``area`` = sum of 0.5 sqrt((c0 c0 + c1 c1) + c2 c2); ``volume`` = sum
    of ((x0 c0 + y0 c1) + z0 c2) / 6 with c = p1 x p2 written the same way.  The order of the two sums is the
    implementation's (here numpy's pairwise sum).

    Self-intersections among the faces that take part.  ``candidate_pairs``: the pairs f < g whose float32 bounding
    boxes overlap, closed.  orient(a, b, c, d) is ``check_orient``.  An edge (p, q) pierces a triangle (a, b, c) when
    orient(a,b,c,p) orient(a,b,c,q) < 0 (the float64 product) and orient(p,q,a,b), orient(p,q,b,c), orient(p,q,c,a) are
    all > 0 or all < 0.  A pair intersects when one of the three edges (p0,p1), (p1,p2), (p2,p0) of either face
    pierces the other.  Every zero is a no: touching and coplanar overlaps do not count.  ``intersecting_pairs``,
    ``intersecting_faces`` (faces in at least one such pair).

    Derived: ``closed`` (no boundary edge), ``manifold`` (no non-manifold edge or vertex), ``oriented`` (no
    misoriented edge), ``watertight`` (all three, no intersecting pair, status 0); False where a field is invalid.
    Not covered: connected components (``separate_mesh`` reports them), duplicate faces (they show as non-manifold
    edges), coplanar overlaps."""
    return _check(verts, faces, max_pairs)[0]


def check_face_flags(verts, faces, max_pairs=None) -> np.ndarray:
    """uint8 [nf] beside ``check_arrays``: 1 in an intersecting pair, 2 zero area or a repeated index, 4 on a boundary
    edge, 8 on a non-manifold edge, 16 on a misoriented edge; a bit whose field is invalid stays 0"""
    return _check(verts, faces, max_pairs)[1]


# ---- mesh repair: the rule (the device restates it, mesh_repair.hip) -----------------------------------
REPAIR_FIELDS = ("nv_out", "nf_out", "status", "welded_vertices", "repeated_faces", "duplicate_faces", "pillow_faces",
                 "singular_edges", "stitched_edges", "pinched_edges", "added_vertices",
                 "dropped_vertices")                              # DISN_REPAIR_NV_OUT .. in this order
REPAIR_WELD, REPAIR_STITCH = 1, 2                                 # the flag bits of disn_mesh_repair_count_batch
REPAIR_MAX_FAN = 16                                               # the most faces of an edge the stitch orders


def _repair_cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _repair_dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _repair_det(a, b, c):
    """the determinant of the rows a, b, c, written as ``check_orient`` writes it"""
    return (a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0])) + a[2] * (b[0] * c[1] - b[1] * c[0])


def repair_stitch_edge(e, d, forward):
    """the angular rule of ``repair_arrays`` on ONE singular edge: e = p_hi - p_lo, d [k,3] = p_opp - p_lo of the edge's
    faces in ascending face order (float64), forward [k]: the face's corner pair runs lo -> hi.  -> the partners
    [(m, n)] as positions in that order, or None when the rule fails (a tie, a rounding inconsistency, or directions that
    do not alternate)"""
    k = len(d)
    r = d[0]
    er = _repair_cross(e, r)
    half = [0] * k
    for m in range(1, k):
        s, c = _repair_det(e, r, d[m]), _repair_dot(er, _repair_cross(e, d[m]))
        if s > 0 or (s == 0 and c > 0):
            half[m] = 0
        elif s < 0 or (s == 0 and c < 0):
            half[m] = 1
        else:
            return None
    rank = [0] * k
    for m in range(1, k):
        n_before = 1                                              # the reference is before everyone
        for n in range(1, k):
            if n != m and (half[n] < half[m] or (half[n] == half[m] and _repair_det(e, d[n], d[m]) > 0)):
                n_before += 1
        rank[m] = n_before
    at = [-1] * k
    for m in range(k):
        if at[rank[m]] >= 0:
            return None                                           # two faces of one rank: no permutation
        at[rank[m]] = m
    if any(forward[at[q]] == forward[at[(q + 1) % k]] for q in range(k)):
        return None
    return [(at[q], at[(q + 1) % k]) for q in range(k) if not forward[at[q]]]


def _repair_identity(v32, f, status: int):
    nv, nf = v32.shape[0], f.shape[0]
    report = {"status": status, "nv": nv, "nf": nf}
    report.update((k, 0) for k in REPAIR_FIELDS if k != "status")
    report.update(nv_out=nv, nf_out=nf)
    return v32.copy(), f.astype(np.int32), np.arange(nv, dtype=np.int32), np.arange(nf, dtype=np.int32), report


def repair_arrays(verts, faces, weld: bool = True, stitch: bool = True):
    """Repair of one mesh to a manifold on the host: THE SPECIFICATION of ``repair_meshes_device`` (every integer; the
    positions are a gather, so their bits follow).  -> (verts' float32 [nv',3], faces' int32 [nf',3], vmap int32 [nv']:
    the ORIGINAL vertex a new one copies, kept int32 [nf']: the original face of a new one, report: ``status``, ``nv``,
    ``nf`` and the REPAIR_FIELDS).  All geometry is float64 on the float32 coordinates, + - x only, each operation
    rounded once, no contraction (as ``check_orient``).

    Status: 2 a face index outside [0, nv); 4 a coordinate that is not finite; of both the larger.  The mesh then comes
    back unchanged, ``vmap`` and ``kept`` the identity, every other count zero.  An empty mesh has status 0 and zeros.

    Weld (``weld``): vertices whose three float32 coordinates are equal (after adding float32(0): -0 equals +0) merge
    into the smallest index of the group (``welded_vertices``: the vertices merged away); otherwise every vertex stands
    for itself.  Drop, on the welded indices: a face with a repeated index (``repeated_faces``); of several faces with
    the same unordered triple, all of one cyclic orientation, all but the smallest face index (``duplicate_faces``); a
    triple held in BOTH orientations is a pillow and loses all its faces (``pillow_faces``).  Zero-area faces on three
    distinct positions stay (dropping one opens a hole).  The survivors keep their order and orientation.

    Edges of the survivors: an undirected edge held by exactly two corner pairs is regular and its two faces are
    PARTNERS there; one held by three or more is singular (``singular_edges``).  Stitch (``stitch``), on a singular edge
    of k faces, k even and k <= REPAIR_MAX_FAN: lo < hi its ends, e = p_hi - p_lo, d_m = p_opp(m) - p_lo, r the d of the
    edge's smallest face; cross(a, b) = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0), dot(a, b) = (a0 b0 + a1 b1) +
    a2 b2, det(a, b, c) = (a0 (b1 c2 - b2 c1) - a1 (b0 c2 - b2 c0)) + a2 (b0 c1 - b1 c0).  For every other face s_m =
    det(e, r, d_m), c_m = dot(cross(e, r), cross(e, d_m)); half 0 when s_m > 0 or (s_m = 0 and c_m > 0), half 1 when
    s_m < 0 or (s_m = 0 and c_m < 0), both zero: the edge fails.  Face m is before n when half_m < half_n, or the halves
    are equal and det(e, d_m, d_n) > 0; the reference is before everyone; rank_m = the number of faces before m.  The
    ranks must be a permutation of 0 .. k-1 (any tie or inconsistency of rounding fails the edge: no sort is involved),
    and the direction of the corner pair (lo -> hi or not) must alternate around the cycle of ranks.  Then each face that
    runs hi -> lo, at rank q, is the partner of the face at rank (q + 1) mod k: the wedge between them is the inside of
    both (``stitched_edges``).  An edge the rule does not apply to, or fails on, is CUT: no face has a partner there.

    Split: the corners (f, i), (g, i) of partners f, g at an edge {i, j} are related, and so are their corners at j; the
    classes are the transitive closure.  A stitched edge two of whose pairs have the same (class at lo, class at hi) is
    pinched (``pinched_edges``, counted among the stitched ones too); the classes are computed AGAIN with every pinched
    edge cut, and that result is final.  Numbering: first the referenced welded vertices in ascending order, each for
    the class of its smallest corner (corner 3 f + k of original face f), then one new vertex per further class in the
    order of the classes' smallest corners (``added_vertices``); unreferenced and welded-away vertices disappear
    (``dropped_vertices``).  Normals and colours ride along through ``vmap``.

    Why the result is manifold: every face has at most one partner per edge, so the corners of a vertex form paths and
    cycles under the partner relation, and a class touches a cut edge with at most its two path ends.  The second pass
    only refines the classes of the first, so distinct pairs of an unpinched stitched edge keep distinct (class at lo,
    class at hi).  Hence every output edge has at most two faces and every output vertex one fan: for status 0,
    ``check_arrays`` of the result gives nonmanifold_edges = nonmanifold_vertices = index_degenerate_faces =
    unreferenced_vertices = 0, and with ``weld=False`` the repair of the result is the identity.

    Not in scope: self-intersections and the other pairing choice at a pinched edge.  Faces keep their orientation
    and a cut edge becomes boundary: ``close_arrays`` orients and closes what this leaves."""
    v32 = np.ascontiguousarray(verts.detach().cpu().numpy() if hasattr(verts, "detach") else verts,
                               np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces.detach().cpu().numpy() if hasattr(faces, "detach") else faces).reshape(-1, 3)
    f = f.astype(np.int64)
    nv, nf = v32.shape[0], f.shape[0]
    status = 0
    if nf and (f.min() < 0 or f.max() >= nv):
        status = STATUS_INDEX
    if not np.isfinite(v32).all():
        status = STATUS_FINITE
    if status:
        return _repair_identity(v32, f, status)
    # -- weld
    rep = np.arange(nv, dtype=np.int64)
    if weld and nv:
        bits = (v32 + np.float32(0)).view(np.uint32)
        _, inv = np.unique(bits, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        smallest = np.full(int(inv.max()) + 1, nv, np.int64)
        np.minimum.at(smallest, inv, np.arange(nv))
        rep = smallest[inv]
    g = rep[f] if nf else f
    # -- drop
    repeated = (g[:, 0] == g[:, 1]) | (g[:, 1] == g[:, 2]) | (g[:, 2] == g[:, 0])
    keep = ~repeated
    even = ((g[:, 0] < g[:, 1]).astype(np.int64) + (g[:, 1] < g[:, 2]) + (g[:, 2] < g[:, 0])) == 2
    duplicate = pillow = 0
    ids = np.nonzero(keep)[0]
    if ids.size:
        _, tinv = np.unique(np.sort(g[ids], axis=1), axis=0, return_inverse=True)
        tinv = tinv.reshape(-1)
        n_even = np.bincount(tinv, weights=even[ids]).astype(np.int64)
        n_all = np.bincount(tinv)
        both = (n_even > 0) & (n_even < n_all)
        first = np.full(n_all.size, nf, np.int64)
        np.minimum.at(first, tinv, ids)
        in_pillow = both[tinv]
        is_dup = ~in_pillow & (first[tinv] != ids)
        pillow, duplicate = int(in_pillow.sum()), int(is_dup.sum())
        keep[ids[in_pillow | is_dup]] = False
    kept = np.nonzero(keep)[0]
    g = g[kept]
    n = g.shape[0]
    # -- edges and partners; corner pair 3 j + k of survivor j runs from its index k to its index (k+1)%3
    a, b = g.reshape(-1), g[:, (1, 2, 0)].reshape(-1)
    forward = a < b
    pair = np.arange(3 * n)
    nxt = pair - pair % 3 + (pair % 3 + 1) % 3
    at_lo, at_hi = np.where(forward, pair, nxt), np.where(forward, nxt, pair)
    ekey = np.minimum(a, b) * np.int64(max(nv, 1)) + np.maximum(a, b)
    order = np.argsort(ekey, kind="stable")                      # the pairs of an edge in ascending face order
    starts = np.nonzero(np.r_[True, ekey[order][1:] != ekey[order][:-1]])[0] if n else np.zeros(0, np.int64)
    ends = np.r_[starts[1:], 3 * n] if n else starts
    partner = np.full(3 * n, -1, np.int64)
    p64 = v32.astype(np.float64)
    singular, stitched = 0, []
    for s0, s1 in zip(starts, ends):
        k = s1 - s0
        row = order[s0:s1]
        if k == 2:
            partner[row[0]], partner[row[1]] = row[1], row[0]
        elif k >= 3:
            singular += 1
            if not (stitch and k % 2 == 0 and k <= REPAIR_MAX_FAN):
                continue
            lo, hi = min(a[row[0]], b[row[0]]), max(a[row[0]], b[row[0]])
            d = [p64[g[c // 3, (c % 3 + 2) % 3]] - p64[lo] for c in row]
            pairs = repair_stitch_edge(p64[hi] - p64[lo], d, [bool(forward[c]) for c in row])
            if pairs is None:
                continue
            for m, q in pairs:
                partner[row[m]], partner[row[q]] = row[q], row[m]
            stitched.append(row)

    def classes():
        parent = np.arange(3 * n)

        def root(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        for c in np.nonzero(partner > pair)[0]:
            for at in (at_lo, at_hi):
                x, y = root(at[c]), root(at[partner[c]])
                if x != y:
                    parent[max(x, y)] = min(x, y)
        return np.array([root(x) for x in range(3 * n)], np.int64)

    roots = classes()
    pinched = 0
    for row in stitched:
        sig = [(roots[at_lo[c]], roots[at_hi[c]]) for c in row if not forward[c]]
        if len(set(sig)) < len(sig):
            pinched += 1
            partner[row] = -1
    if pinched:
        roots = classes()
    # -- numbering
    first_corner = np.full(nv, 3 * n, np.int64)
    np.minimum.at(first_corner, a, pair)
    ref = first_corner < 3 * n
    main_root = np.full(nv, -1, np.int64)
    main_root[ref] = roots[first_corner[ref]]
    extra = (roots == pair) & (main_root[a] != pair)
    n_main = int(ref.sum())
    new_of_root = np.where(extra, n_main + np.cumsum(extra) - 1, (np.cumsum(ref) - 1)[a])
    faces_out = new_of_root[roots].reshape(-1, 3).astype(np.int32)
    vmap = np.r_[np.nonzero(ref)[0], a[extra]].astype(np.int32)
    report = {"status": 0, "nv": nv, "nf": nf, "nv_out": int(vmap.size), "nf_out": int(n),
              "welded_vertices": int((rep != np.arange(nv)).sum()), "repeated_faces": int(repeated.sum()),
              "duplicate_faces": duplicate, "pillow_faces": pillow, "singular_edges": singular,
              "stitched_edges": len(stitched), "pinched_edges": pinched, "added_vertices": int(extra.sum()),
              "dropped_vertices": nv - n_main}
    return v32[vmap], faces_out, vmap, kept.astype(np.int32), report


# ---- mesh closing: the rule (the device restates it, mesh_close.hip) -----------------------------------
CLOSE_FIELDS = ("nv_out", "nf_out", "status", "components", "unorientable_components", "flipped_faces", "loops",
                "filled_loops", "fill_faces")                     # DISN_CLOSE_NV_OUT .. in this order
CLOSE_ORIENT, CLOSE_FILL, CLOSE_OUTWARD = 1, 2, 4                 # the flag bits of disn_mesh_close_count_batch
CLOSE_MAX_HOLE = 1 << 22                                          # the longest loop that is filled: 2^22 2^40 = 2^62
STATUS_NOT_MANIFOLD = 16


def close_flags(orient=True, fill=True, outward=False, max_hole=None) -> Tuple[int, int]:
    """the checked (flag bits, max_hole) of ``close_arrays`` and ``close_meshes_device``; ValueError otherwise"""
    for name, x in (("orient", orient), ("fill", fill), ("outward", outward)):
        if not isinstance(x, (bool, np.bool_)):
            raise ValueError("close: %s must be True or False, got %r" % (name, x))
    if outward and not orient:
        raise ValueError("close: outward needs orient")
    cap = CLOSE_MAX_HOLE if max_hole is None else max_hole
    if isinstance(cap, (bool, np.bool_)) or not isinstance(cap, (int, np.integer)) or not 0 <= cap <= CLOSE_MAX_HOLE:
        raise ValueError("close: max_hole must be an integer in 0..%d, got %r" % (CLOSE_MAX_HOLE, max_hole))
    return ((CLOSE_ORIENT if orient else 0) | (CLOSE_FILL if fill else 0) | (CLOSE_OUTWARD if outward else 0)), int(cap)


def close_exponent(v32: np.ndarray) -> int:
    """E: the ``frexp`` exponent of the largest |coordinate| (largest = 2^E m, 0.5 <= m < 1), 0 when that is 0"""
    largest = float(np.abs(v32).max()) if v32.size else 0.0
    return int(np.frexp(largest)[1]) if largest != 0.0 else 0


def _close_identity(v32, f, status: int):
    nv, nf = v32.shape[0], f.shape[0]
    report = {"status": status, "nv": nv, "nf": nf}
    report.update((k, 0) for k in CLOSE_FIELDS if k != "status")
    report.update(nv_out=nv, nf_out=nf)
    return v32.copy(), f.astype(np.int32), np.arange(nv, dtype=np.int32), np.arange(nf, dtype=np.int32), report


def close_arrays(verts, faces, orient: bool = True, fill: bool = True, outward: bool = False, max_hole=None):
    """Closing of one manifold mesh on the host: consistent orientation and hole filling.  THE SPECIFICATION of
    ``close_meshes_device`` (every integer and every position bit).  -> (verts' float32 [nv',3], faces' int32 [nf',3],
    vmap int32 [nv'], kept int32 [nf'], report: ``status``, ``nv``, ``nf`` and the CLOSE_FIELDS).  It stands behind
    ``repair_arrays``, whose output never has status 16.

    Status, of several the largest: 0; 2 a face index outside [0, nv); 4 a coordinate that is not finite; 16
    (STATUS_NOT_MANIFOLD) a face with a repeated index, an undirected edge held by three or more corner pairs, or a
    vertex on more than two boundary edges -- tests on integers alone, made where every index is valid (a mesh with a
    bad index is not looked at through its indices: it has status 2, or 4).  A mesh with a status comes back unchanged,
    ``vmap`` and ``kept`` the identity, every counter 0.  An empty mesh has status 0 and zeros.

    Edges as in ``repair_arrays``: face (a, b, c) gives the corner pairs (a, b), (b, c), (c, a), corner 3 f + k is pair
    k of face f; an undirected edge held by two pairs makes its faces PARTNERS, one held by one pair is boundary.

    Orient (``orient``; without it ``components``, ``unorientable_components`` and ``flipped_faces`` are 0).  The
    components are the classes of faces under "partners" (``components``); a component's root is its smallest face.
    Two partners are related by 1 when their corner pairs at the shared edge run the same way (``check_arrays`` calls
    that edge misoriented), else by 0.  A component is orientable when every face can be given a parity, the root 0,
    such that every relation holds; the parity is then unique.  A non-orientable component
    (``unorientable_components``) keeps the orientation of its faces; it is still filled.  Of an orientable one, n0 and
    n1 are the faces of parity 0 and 1 and K = 1 if n1 > n0 else 0: the majority stays, a tie keeps the root's
    orientation.  Every face of parity != K is written as (a, c, b) (``flipped_faces``).  A consistent component
    (n1 = 0) is never touched without ``outward``: an inward-facing cavity is legitimate.

    Fill (``fill``; without it ``loops``, ``filled_loops`` and ``fill_faces`` are 0).  Boundary vertices joined by a
    boundary corner pair belong to one loop, whose id is its smallest vertex and whose length L its number of boundary
    pairs (``loops``); under status 0 the loops are simple and vertex-disjoint.  A loop with L <= ``max_hole`` (default
    and limit CLOSE_MAX_HOLE = 2^22) is filled (``filled_loops``): one new vertex c, and for every boundary pair
    (a -> b) of the loop one face (c, b, a) -- (c, a, b) when the pair's face is flipped -- (``fill_faces``).  A fan
    from a centre never names an edge the mesh already has; a fan from a rim vertex can.  The centre, in integers and
    single roundings: E = ``close_exponent`` of all nv vertices; q(x) = rint(float64(x) 2^(40-E)) as int64 of every
    coordinate of the tail a of every boundary pair of the loop (in the input's orientation); S = their exact sum;
    centre = float32(float64(S) / float64(L) * 2^(E-40)) per axis.

    Outward (``outward``, needs ``orient``; wrong for cavities, hence off by default), on the orientable components
    with no unfilled boundary pair: t_f = ``_check_volume_terms`` of face f, an input face as it came, a fill face as
    (c, b, a); tq_f = rint(t_f 2^(30-3E)) as int64 (|tq| <= 2^30); V = the sum of tq_f over the component's faces,
    fill faces included, + for a face of parity K and - otherwise, a fill face having the parity of the face of its
    pair.  V < 0: K becomes 1 - K.  V is an integer, so its sign does not depend on the order of the sum.

    Numbering: verts' = the nv input vertices untouched and in place (closing drops nothing, unreferenced vertices
    stay), then one centre per filled loop in ascending loop id; faces' = the nf input faces in order, then the fill
    faces in ascending corner 3 f + k of their pairs.  vmap[i] = i for i < nv and the loop id for a centre: the vertex
    whose rows of any further per-vertex array (the normals) the centre inherits.  kept[f] = f for an input face, the
    face of its pair for a fill face.

    Guarantee: for status 0 with ``orient`` and ``fill`` and no loop over ``max_hole``, ``check_arrays`` of the result
    has boundary_edges = 0, nonmanifold_edges = 0, nonmanifold_vertices as the input's, and misoriented_edges = 0 when
    ``unorientable_components`` = 0; closing the result again changes nothing.  Limits: a fan over a non-planar loop
    may intersect itself or the mesh, caps are flat, non-orientable components stay as they are, the centre inherits a
    rim vertex's normal."""
    v32 = np.ascontiguousarray(verts.detach().cpu().numpy() if hasattr(verts, "detach") else verts,
                               np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces.detach().cpu().numpy() if hasattr(faces, "detach") else faces).reshape(-1, 3)
    f = f.astype(np.int64)
    nv, nf = v32.shape[0], f.shape[0]
    flags, cap = close_flags(orient, fill, outward, max_hole)
    valid = not (nf and (f.min() < 0 or f.max() >= nv))
    status = 0 if valid else STATUS_INDEX
    if not np.isfinite(v32).all():
        status = STATUS_FINITE
    a, b = f.reshape(-1), f[:, (1, 2, 0)].reshape(-1)            # corner pair 3 f + k: index k -> index (k+1)%3
    if valid and nf:
        key = np.minimum(a, b) * np.int64(nv) + np.maximum(a, b)
        _, inv, held = np.unique(key, return_inverse=True, return_counts=True)
        inv = inv.reshape(-1)
        boundary = held[inv] == 1
        degree = np.bincount(a[boundary], minlength=nv) + np.bincount(b[boundary], minlength=nv)
        if (a == b).any() or (held >= 3).any() or (degree > 2).any():
            status = STATUS_NOT_MANIFOLD
    if status or not nf:
        return _close_identity(v32, f, status)
    forward = a < b
    order = np.argsort(inv, kind="stable")
    first = (np.cumsum(held) - held)[held == 2]
    c0, c1 = order[first], order[first + 1]                      # the two pairs of every regular edge
    rel = (forward[c0] == forward[c1]).astype(np.int64)
    p64 = v32.astype(np.float64)
    E = close_exponent(v32)
    # -- orient: a union-find of faces that carries each face's parity against its parent; roots only decrease
    root, parity = np.arange(nf), np.zeros(nf, np.int64)
    orientable = np.ones(nf, bool)                               # read at the roots
    if orient:
        parent, par = list(range(nf)), [0] * nf

        def find(x):
            path = []
            while parent[x] != x:
                path.append(x)
                x = parent[x]
            p = 0
            for y in reversed(path):
                p ^= par[y]
                parent[y], par[y] = x, p
            return x, p

        clash = []
        for x, y, r in zip((c0 // 3).tolist(), (c1 // 3).tolist(), rel.tolist()):
            (rx, px), (ry, py) = find(x), find(y)
            if rx == ry:
                if px ^ py != r:
                    clash.append(x)
            else:
                hi, lo = max(rx, ry), min(rx, ry)
                parent[hi], par[hi] = lo, px ^ py ^ r
        found = [find(x) for x in range(nf)]
        root, parity = np.array([r for r, _ in found], np.int64), np.array([p for _, p in found], np.int64)
        orientable[root[np.array(clash, np.int64)]] = False
    n1 = np.bincount(root, weights=parity, minlength=nf).astype(np.int64)
    K = (n1 > np.bincount(root, minlength=nf) - n1).astype(np.int64)
    # -- fill: a union-find of vertices over the boundary pairs
    bc = np.nonzero(boundary)[0]
    filled_pair = np.zeros(3 * nf, bool)
    ids = np.zeros(0, np.int64)
    loops = 0
    centres = np.zeros((0, 3), np.float32)
    if fill and bc.size:
        vparent = list(range(nv))

        def vroot(x):
            while vparent[x] != x:
                vparent[x] = vparent[vparent[x]]
                x = vparent[x]
            return x

        for x, y in zip(a[bc].tolist(), b[bc].tolist()):
            rx, ry = vroot(x), vroot(y)
            if rx != ry:
                vparent[max(rx, ry)] = min(rx, ry)
        loop = np.array([vroot(x) for x in a[bc].tolist()], np.int64)
        L = np.bincount(loop, minlength=nv)
        loops = int((L > 0).sum())
        ids = np.nonzero((L > 0) & (L <= cap))[0]                # the filled loops, ascending
        filled_pair[bc] = L[loop] <= cap
        S = np.zeros((nv, 3), np.int64)
        np.add.at(S, loop, np.rint(p64[a[bc]] * np.ldexp(1.0, 40 - E)).astype(np.int64))
        centres = (S[ids].astype(np.float64) / L[ids].astype(np.float64)[:, None]
                   * np.ldexp(1.0, E - 40)).astype(np.float32)
    fc = np.nonzero(filled_pair)[0]                              # the pairs that get a face, ascending
    rank = np.zeros(nv, np.int64)
    rank[ids] = np.arange(ids.size)
    centre_of = nv + rank[np.array([vroot(x) for x in a[fc].tolist()], np.int64)] if fc.size else fc
    verts_out = np.concatenate([v32, centres])
    caps = np.stack([centre_of, b[fc], a[fc]], axis=1)
    # -- outward
    if outward:
        still_open = np.zeros(nf, bool)
        still_open[root[bc[~filled_pair[bc]] // 3]] = True
        scale = np.ldexp(1.0, 30 - 3 * E)
        tq = np.rint(_check_volume_terms(p64[f]) * scale).astype(np.int64)
        tq_caps = np.rint(_check_volume_terms(verts_out.astype(np.float64)[caps]) * scale).astype(np.int64)
        V = np.zeros(nf, np.int64)
        np.add.at(V, root, np.where(parity == K[root], tq, -tq))
        np.add.at(V, root[fc // 3], np.where(parity[fc // 3] == K[root[fc // 3]], tq_caps, -tq_caps))
        K = np.where(orientable & ~still_open & (V < 0), 1 - K, K)
    flip = orientable[root] & (parity != K[root]) if orient else np.zeros(nf, bool)
    faces_out = f.copy()
    faces_out[flip] = faces_out[flip][:, (0, 2, 1)]
    caps[flip[fc // 3]] = caps[flip[fc // 3]][:, (0, 2, 1)]
    is_root = root == np.arange(nf)
    report = {"status": 0, "nv": nv, "nf": nf, "nv_out": nv + int(ids.size), "nf_out": nf + int(fc.size),
              "components": int(is_root.sum()) if orient else 0,
              "unorientable_components": int((is_root & ~orientable).sum()) if orient else 0,
              "flipped_faces": int(flip.sum()), "loops": loops, "filled_loops": int(ids.size),
              "fill_faces": int(fc.size)}
    return (verts_out, np.concatenate([faces_out, caps]).astype(np.int32),
            np.r_[np.arange(nv), ids].astype(np.int32), np.r_[np.arange(nf), fc // 3].astype(np.int32), report)


# ---- vertex colours from the input views: the rule (the device restates it, mesh_colour.hip) ----------
IMG = 137                                   # the views are IMG x IMG, pixel centres at integer (u, v)
COLOUR_SAMPLES = (1, 2, 4)                  # z-buffer samples per image pixel and axis
COLOUR_MAX_VIEWS, COLOUR_MAX_FILL = 256, 4096
CLASS_FALLBACK, CLASS_SEEN, CLASS_MIRROR, CLASS_FILL = 0, 1, 2, 3
MIRROR_FRONT = 32                           # a reflection may lie this many rel_tol in FRONT of the stored surface
_UNCOLOURED = 255                           # the working state of ``seen`` before the fallback
_GREY16 = 32768                             # mid grey: 128 of 255
_TINY = np.float32(1.17549435e-38)          # the smallest positive normal float32
_F32_0, _F32_1, _F32_HALF = np.float32(0.0), np.float32(1.0), np.float32(0.5)


def _colour_params(S, rel_tol, mirror_axis, fill_iters):
    if S not in COLOUR_SAMPLES:
        raise ValueError("S must be one of %s, got %r" % (COLOUR_SAMPLES, S))
    if mirror_axis not in (None, 0, 1, 2):
        raise ValueError("mirror_axis must be None, 0, 1 or 2, got %r" % (mirror_axis,))
    if int(fill_iters) != fill_iters or not 0 <= int(fill_iters) <= COLOUR_MAX_FILL:
        raise ValueError("fill_iters must be in 0..%d, got %r" % (COLOUR_MAX_FILL, fill_iters))
    tol = np.float32(rel_tol)
    if not (tol >= 0.0 and tol < 1.0):
        raise ValueError("rel_tol must be in [0, 1), got %r" % (rel_tol,))
    return int(S), tol, -1 if mirror_axis is None else int(mirror_axis), int(fill_iters)


def _colour_mesh(verts, faces):
    v, f = _host(verts, faces)
    if f.shape[0] and (f.min() < 0 or f.max() >= v.shape[0]):
        raise ValueError("face index out of range (mesh of %d vertices)" % v.shape[0])
    if not np.isfinite(v).all():
        raise ValueError("a vertex coordinate is not finite")
    return v, f


def _colour_views(trans_mats) -> np.ndarray:
    T = np.ascontiguousarray(trans_mats, np.float32)
    if T.ndim == 2:
        T = T[None]
    if T.ndim != 3 or T.shape[1:] != (4, 3) or not 1 <= T.shape[0] <= COLOUR_MAX_VIEWS:
        raise ValueError("trans_mats must be [V,4,3] with 1 <= V <= %d, got %s" % (COLOUR_MAX_VIEWS, T.shape))
    return T


def _screen(v: np.ndarray, T: np.ndarray, S: int):
    """float32, the gather's projection [p, 1] . T = (u w, v w, w) in its order of operations -> sub-pixel position
    (x, y) = ((u + 1/2) S, (v + 1/2) S), q = 1/w, (u, v), and ok = w > 0 with x, y, q finite"""
    with np.errstate(all="ignore"):
        p = []
        for j in range(3):
            a = v[:, 0] * T[0, j] + v[:, 1] * T[1, j]
            a = a + v[:, 2] * T[2, j]
            p.append(a + T[3, j])
        w = p[2]
        u, vv, q = p[0] / w, p[1] / w, _F32_1 / w
        x, y = (u + _F32_HALF) * np.float32(S), (vv + _F32_HALF) * np.float32(S)
        ok = (w > 0.0) & np.isfinite(x) & np.isfinite(y) & np.isfinite(q)
    return x, y, q, u, vv, ok


def _cover(t, cx, cy):
    """the sub-pixels with centres (cx, cy) against the triangles ``t`` (a dict of float32 arrays that broadcast with
    cx, cy) -> (inside, value): conservative coverage and the biased, clamped plane of q"""
    inside = None
    for k in range(3):
        a, b, xi, yi = t["a"][k], t["b"][k], t["ex"][k], t["ey"][k]
        e = ((a * (cx - xi) + b * (cy - yi)) + _F32_HALF * (np.abs(a) + np.abs(b))) >= 0.0
        inside = e if inside is None else inside & e
    val = t["q0"] + (t["gx"] * (cx - t["x0"]) + t["gy"] * (cy - t["y0"]))
    val = np.where(val > t["qmax"], t["qmax"], val)
    val = np.where(val < t["qmin"], t["qmin"], val)
    val = val - (np.abs(t["gx"]) + np.abs(t["gy"]))
    return inside, np.where(val >= _TINY, val, _TINY).astype(np.float32)


def _raster_view(v: np.ndarray, f: np.ndarray, T: np.ndarray, S: int) -> np.ndarray:
    N = IMG * S
    zb = np.zeros(N * N, np.uint32)               # positive floats order as their bits do
    x, y, q, _, _, ok = _screen(v, T, S)
    keep = np.nonzero(ok[f[:, 0]] & ok[f[:, 1]] & ok[f[:, 2]])[0] if f.shape[0] else np.zeros(0, np.int64)
    if keep.size == 0:
        return zb.view(np.float32).reshape(N, N)
    c = f[keep]
    with np.errstate(all="ignore"):
        X, Y, Q = [x[c[:, k]] for k in range(3)], [y[c[:, k]] for k in range(3)], [q[c[:, k]] for k in range(3)]
        area = (X[1] - X[0]) * (Y[2] - Y[0]) - (X[2] - X[0]) * (Y[1] - Y[0])
        dq1, dq2 = Q[1] - Q[0], Q[2] - Q[0]
        gx = (dq1 * (Y[2] - Y[0]) - dq2 * (Y[1] - Y[0])) / area
        gy = (dq2 * (X[1] - X[0]) - dq1 * (X[2] - X[0])) / area
        fi0, fi1 = np.floor(np.minimum(np.minimum(X[0], X[1]), X[2])), np.floor(np.maximum(np.maximum(X[0], X[1]), X[2]))
        fj0, fj1 = np.floor(np.minimum(np.minimum(Y[0], Y[1]), Y[2])), np.floor(np.maximum(np.maximum(Y[0], Y[1]), Y[2]))
        good = (np.isfinite(area) & (area != 0.0) & np.isfinite(gx) & np.isfinite(gy)
                & (fi1 >= 0.0) & (fi0 <= N - 1.0) & (fj1 >= 0.0) & (fj0 <= N - 1.0))
    g = np.nonzero(good)[0]
    if g.size == 0:
        return zb.view(np.float32).reshape(N, N)
    X, Y, Q = [a[g] for a in X], [a[g] for a in Y], [a[g] for a in Q]
    s = np.where(area[g] > 0.0, _F32_1, -_F32_1).astype(np.float32)
    t = {"a": [s * (Y[i] - Y[j]) for i, j in ((1, 2), (2, 0), (0, 1))],
         "b": [s * (X[j] - X[i]) for i, j in ((1, 2), (2, 0), (0, 1))],
         "ex": [X[1], X[2], X[0]], "ey": [Y[1], Y[2], Y[0]], "x0": X[0], "y0": Y[0], "q0": Q[0], "gx": gx[g], "gy": gy[g],
         "qmin": np.minimum(np.minimum(Q[0], Q[1]), Q[2]), "qmax": np.maximum(np.maximum(Q[0], Q[1]), Q[2])}
    i0 = np.maximum(fi0[g], _F32_0).astype(np.int64)
    i1 = np.minimum(fi1[g], np.float32(N - 1)).astype(np.int64)
    j0 = np.maximum(fj0[g], _F32_0).astype(np.int64)
    j1 = np.minimum(fj1[g], np.float32(N - 1)).astype(np.int64)
    bw, bh = i1 - i0 + 1, j1 - j0 + 1
    pick = lambda m: {k: ([a[m] for a in val] if isinstance(val, list) else val[m]) for k, val in t.items()}
    # (how the triangles are grouped is the host's business: the buffer keeps a maximum, whatever the order)
    small = np.nonzero((bw <= 8) & (bh <= 8))[0]
    if small.size:
        ts = pick(small)
        for dj in range(int(bh[small].max())):
            for di in range(int(bw[small].max())):
                m = (di < bw[small]) & (dj < bh[small])
                if not m.any():
                    continue
                ii, jj = i0[small] + di, j0[small] + dj
                inside, val = _cover(ts, ii.astype(np.float32) + _F32_HALF, jj.astype(np.float32) + _F32_HALF)
                m &= inside
                np.maximum.at(zb, (jj * N + ii)[m], val.view(np.uint32)[m])
    for n in np.nonzero((bw > 8) | (bh > 8))[0]:
        tn = pick(n)
        ii, jj = np.arange(i0[n], i1[n] + 1), np.arange(j0[n], j1[n] + 1)
        inside, val = _cover(tn, (ii.astype(np.float32) + _F32_HALF)[None, :], (jj.astype(np.float32) + _F32_HALF)[:, None])
        idx = (jj[:, None] * N + ii[None, :])[inside]
        np.maximum.at(zb, idx, val.view(np.uint32)[inside])
    return zb.view(np.float32).reshape(N, N)


def zbuffer_arrays(verts, faces, trans_mats, S: int = 2) -> np.ndarray:
    """Depth maps of a mesh from its views, on the host: THE SPECIFICATION of ``zbuffer_meshes_device`` (same bits).
    -> [V, 137 S, 137 S] float32 of q = 1/w, larger is nearer, 0 is empty.  Everything is float32, operation by operation.

    A vertex goes to x = (u + 1/2) S, y = (v + 1/2) S with [p, 1] . trans_mat = (u w, v w, w); sub-pixel (i, j) covers
    [i, i+1) x [j, j+1) and is stored at [j, i].  A triangle with a vertex at w <= 0 (or x, y, 1/w not finite), of zero
    screen area, or whose plane of q has no finite gradient, is skipped.  Coverage is conservative: a sub-pixel of the
    bounding box, clipped to the image, belongs to the triangle when its three edge functions at the centre, oriented by
    the sign of the area and each raised by (|a| + |b|) / 2, are >= 0.  The value is the plane of q at the centre,
    clamped to the vertices' [min q, max q], THEN lowered by |dq/dx| + |dq/dy| and floored at the smallest positive
    normal float; the buffer keeps the maximum (of the bits: positive floats order as their bits do).
    ValueError for a face index out of range or a coordinate that is not finite."""
    if S not in COLOUR_SAMPLES:
        raise ValueError("S must be one of %s, got %r" % (COLOUR_SAMPLES, S))
    v, f = _colour_mesh(verts, faces)
    T = _colour_views(trans_mats)
    return np.stack([_raster_view(v, f, T[k], int(S)) for k in range(T.shape[0])])


def _seen_view(v, T, zb, alpha, S: int, tol, reflected: bool):
    """-> (seen bool [n], u, v): w > 0, the sub-pixel inside the image, 1/w >= (1 - tol) zbuf there (and, for a
    reflection, 1/w <= (1 + 32 tol) zbuf: on the visible surface), alpha > 0 at the nearest image pixel"""
    N = IMG * S
    x, y, q, u, vv, ok = _screen(v, T, S)
    with np.errstate(all="ignore"):
        fi, fj = np.floor(x), np.floor(y)
        ok = ok & (fi >= 0.0) & (fi <= N - 1.0) & (fj >= 0.0) & (fj <= N - 1.0)
        i, j = np.where(ok, fi, _F32_0).astype(np.int64), np.where(ok, fj, _F32_0).astype(np.int64)
        z = zb[j, i]
        ok &= q >= (_F32_1 - tol) * z
        if reflected:
            ok &= q <= (_F32_1 + np.float32(MIRROR_FRONT) * tol) * z
        u, vv = np.where(ok, u, _F32_0), np.where(ok, vv, _F32_0)
        if alpha is not None:
            top = np.float32(IMG - 1)
            pu = np.rint(np.minimum(np.maximum(u, _F32_0), top)).astype(np.int64)
            pv = np.rint(np.minimum(np.maximum(vv, _F32_0), top)).astype(np.int64)
            ok &= alpha[pv, pu] > 0
    return ok, u, vv


def _sample16(image, u, vv, bgr: bool) -> np.ndarray:
    """bilinear at (u, v) clamped to [0, 136], float32 lerps in the gather's form -> rint(c 65535) int64 [n,3]"""
    top = np.float32(IMG - 1)
    uc, vc = np.minimum(np.maximum(u, _F32_0), top), np.minimum(np.maximum(vv, _F32_0), top)
    fx0, fy0 = np.floor(uc), np.floor(vc)
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, IMG - 1), np.minimum(y0 + 1, IMG - 1)
    xl, yl = (uc - fx0)[:, None], (vc - fy0)[:, None]
    tl, tr, bl, br = image[y0, x0], image[y0, x1], image[y1, x0], image[y1, x1]
    with np.errstate(all="ignore"):
        t = tl + (tr - tl) * xl
        b = bl + (br - bl) * xl
        val = t + (b - t) * yl
        val = np.where(val > 0.0, val, _F32_0)
        val = np.where(val < 1.0, val, _F32_1)
        c = np.rint(val * np.float32(65535.0)).astype(np.int64)
    return c[:, ::-1] if bgr else c


def _mean_half_up(total: np.ndarray, n: np.ndarray) -> np.ndarray:
    return (2 * total + n) // (2 * n)


def colour_arrays(verts, faces, images, trans_mats, alpha=None, S: int = 2, rel_tol: float = 1e-3, mirror_axis=None,
                  fill_iters: int = 32, bgr: bool = True) -> Tuple[np.ndarray, np.ndarray]:
    """Vertex colours of a mesh from its V input views, on the host: THE SPECIFICATION of ``colour_meshes_device`` (same
    bytes).  images [V,137,137,3] float32 in [0,1], trans_mats [V,4,3], alpha [V,137,137] uint8 or None.
    -> (colours uint8 [nv,3], R G B; seen uint8 [nv], the class).

    seen      vertex p is seen by view k when w > 0, its sub-pixel lies inside the image, 1/w >= (1 - rel_tol) zbuf
              there (``zbuffer_arrays``; an empty cell hides nothing) and, with ``alpha``, alpha > 0 at the nearest
              image pixel rint(clamp(u)), rint(clamp(v))
    sample    bilinear at (u, v) clamped to [0, 136] in float32, clamped to [0, 1]; a channel is rint(c 65535), an integer;
              ``bgr``: the images are in cv2 order, channel 2 is written first
    class 1   seen by >= 1 view: the integer mean over those views, (2 sum + n) // (2 n)
    class 2   ``mirror_axis``: an unseen vertex whose reflection in that coordinate plane passes the same test and also
              1/w <= (1 + 32 rel_tol) zbuf (it lies ON the visible surface, not in front of it; the stored value is
              lowered by a sub-pixel's extent of its plane, 0.3 to 2 % of q on a 32 x 16 sphere, so the bound on this
              side is ``MIRROR_FRONT`` = 32 times wider) takes the mean of the reflection's samples
    class 3   up to ``fill_iters`` rounds: a still uncoloured vertex that shares a face with coloured ones takes the
              integer mean of those corners (once per shared face) as they were before the round
    class 0   what is left: the integer mean of the mesh's coloured vertices, or mid grey (128) when there are none
    colours = (c16 255 + 32767) // 65535.  Every sum is an integer sum: no result depends on an order of additions.
    ValueError for a face index out of range or a coordinate that is not finite."""
    S, tol, axis, fill_iters = _colour_params(S, rel_tol, mirror_axis, fill_iters)
    v, f = _colour_mesh(verts, faces)
    T = _colour_views(trans_mats)
    V, nv = T.shape[0], v.shape[0]
    img = np.ascontiguousarray(images, np.float32).reshape(V, IMG, IMG, 3)
    al = None if alpha is None else np.ascontiguousarray(alpha, np.uint8).reshape(V, IMG, IMG)
    zb = [_raster_view(v, f, T[k], S) for k in range(V)]
    c16, cls = np.zeros((nv, 3), np.int64), np.full(nv, _UNCOLOURED, np.uint8)
    if nv == 0:
        return np.zeros((0, 3), np.uint8), np.zeros(0, np.uint8)

    def gather(p, reflected):
        total, n = np.zeros((nv, 3), np.int64), np.zeros(nv, np.int64)
        for k in range(V):
            ok, u, vv = _seen_view(p, T[k], zb[k], None if al is None else al[k], S, tol, reflected)
            total[ok] += _sample16(img[k], u[ok], vv[ok], bgr)
            n += ok
        return total, n

    total, n = gather(v, False)
    hit = n > 0
    c16[hit], cls[hit] = _mean_half_up(total[hit], n[hit, None]), CLASS_SEEN
    if axis >= 0:
        r = v.copy()
        r[:, axis] = -r[:, axis]
        total, n = gather(r, True)
        hit = (n > 0) & (cls == _UNCOLOURED)
        c16[hit], cls[hit] = _mean_half_up(total[hit], n[hit, None]), CLASS_MIRROR
    for _ in range(fill_iters):
        done = cls != _UNCOLOURED
        total, n = np.zeros((nv, 3), np.int64), np.zeros(nv, np.int64)
        for k in range(3):
            for m in range(3):
                if m != k:
                    sel = ~done[f[:, k]] & done[f[:, m]]
                    np.add.at(total, f[sel, k], c16[f[sel, m]])
                    np.add.at(n, f[sel, k], 1)
        new = ~done & (n > 0)
        if not new.any():
            break
        c16[new], cls[new] = _mean_half_up(total[new], n[new, None]), CLASS_FILL
    done = cls != _UNCOLOURED
    if not done.all():
        k = int(done.sum())
        c16[~done] = _mean_half_up(c16[done].sum(0), np.int64(k)) if k else _GREY16
        cls[~done] = CLASS_FALLBACK
    return ((c16 * 255 + 32767) // 65535).astype(np.uint8), cls


# ---- the device path: B meshes back to back (mesh_clean.hip, mesh_simplify.hip, mesh_colour.hip) ---------------
# a mesh's status word (csrc/mesh_batch.hpp and the stages' own; include/): 1 is the cleanup's, 5 the simplification's,
# 7 the smoothing's (STATUS_SMOOTH_RANGE above; 6 is the sampler's, metrics.STATUS_NO_AREA)
STATUS_NOTHING_KEPT, STATUS_INDEX, STATUS_TABLE, STATUS_FINITE, STATUS_CAPACITY = 1, 2, 3, 4, 5


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


def _pack_meshes(meshes, workspace_bytes, what: str = ""):
    """B x (verts, faces, ...) -> (verts, v_off, faces, f_off, workspace): the meshes packed and the workspace of a
    stage whose query is ``workspace_bytes(nv, nf)``; ValueError when the query refuses the batch (0)"""
    import torch

    from . import ops
    (v, v_off), (f, f_off) = (_pack([m[0] for m in meshes], torch.float32, "verts"),
                              _pack([m[1] for m in meshes], torch.int32, "faces"))
    nv, nf = int(v_off[-1]), int(f_off[-1])
    need = workspace_bytes(nv, nf)
    if need == 0:
        raise ValueError("unsupported batch: %d meshes, %s%d vertices, %d triangles" % (len(meshes), what, nv, nf))
    return v, v_off, f, f_off, ops._ws(need, v.device)


def _raise_status(b: int, status: int, v_off, entry: str):
    """the statuses the stages share -> their exceptions (a stage adds its own cases behind this)"""
    if status == STATUS_INDEX:
        raise ValueError("mesh %d: face index out of range (mesh of %d vertices)" % (b, v_off[b + 1] - v_off[b]))
    if status == STATUS_FINITE:
        raise ValueError("mesh %d: a vertex coordinate is not finite" % b)
    if status == STATUS_TABLE:
        raise RuntimeError("mesh %d: internal table full (%s)" % (b, entry))


def _one_mesh(fn, *args, **kw):
    """``fn(*args, **kw)``, a group call on one mesh, with the "mesh 0: " taken off its ValueErrors"""
    try:
        return fn(*args, **kw)
    except ValueError as e:
        msg = str(e)
        raise ValueError(msg[len("mesh 0: "):] if msg.startswith("mesh 0: ") else msg) from e


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
    v, v_off, f, f_off, ws = _pack_meshes([(verts, faces)],
                                          lambda nv, nf: lib().disn_mesh_clean_workspace_bytes(1, nv, nf))
    nv, nf, dev = int(v_off[1]), int(f_off[1]), f.device
    labels = torch.empty(nf, dtype=torch.int32, device=dev)
    if nf == 0:
        return labels, torch.zeros(0, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
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
    B, h = len(meshes), lib()
    v, v_off, f, f_off, ws = _pack_meshes(meshes, lambda nv, nf: h.disn_mesh_clean_workspace_bytes(B, nv, nf))
    dev = v.device
    with torch.cuda.device(dev):
        counts = torch.zeros((B, 5), dtype=torch.int64, device=dev)
        st = ops._stream()
        check("disn_mesh_clean_count_batch", h.disn_mesh_clean_count_batch(
            v.data_ptr(), f.data_ptr(), v_off.ctypes.data, f_off.ctypes.data, B, conn, float(dist_thresh),
            float(num_thresh), counts.data_ptr(), ws.data_ptr(), ws.numel(), st))
        sizes = np.ascontiguousarray(counts.cpu().numpy())      # the one host sync of the group
        for b in range(B):
            _raise_status(b, sizes[b, 4], v_off, "disn_mesh_clean_count_batch")
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
    cleaned, kept = _one_mesh(clean_meshes_device, [(verts, faces)], dist_thresh, num_thresh, connectivity)
    return cleaned[0][0], cleaned[0][1], kept[0].tolist()


# ---- simplification on the device (mesh_simplify.hip) ----------------------------------------------------------
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
    h = lib()
    v, v_off, f, f_off, ws = _pack_meshes(meshes, lambda nv, nf: h.disn_mesh_simplify_workspace_bytes(B, nv, nf))
    nv, dev = int(v_off[-1]), v.device
    with torch.cuda.device(dev):
        counts = torch.zeros((B, 4), dtype=torch.int64, device=dev)
        st = ops._stream()
        check("disn_mesh_simplify_count_batch", h.disn_mesh_simplify_count_batch(
            v.data_ptr(), f.data_ptr(), v_off.ctypes.data, f_off.ctypes.data, lattice.ctypes.data, cells_h.ctypes.data,
            B, 1 if dedup else 0, counts.data_ptr(), ws.data_ptr(), ws.numel(), st))
        sizes = np.ascontiguousarray(counts.cpu().numpy())      # the one host sync of the group
        for b in range(B):
            _raise_status(b, sizes[b, 3], v_off, "disn_mesh_simplify_count_batch")
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
    simplified, maps = _one_mesh(simplify_meshes_device, [(verts, faces)], [box], cells, dedup)
    return simplified[0][0], simplified[0][1], maps[0][0], maps[0][1]


# ---- Taubin smoothing on the device (mesh_smooth.hip) ------------------------------------------------------------
def smooth_meshes_device(meshes, iters=10, lam=0.5, mu=-0.53, pin_boundary=True, max_move=None, strict: bool = True):
    """``smooth_arrays`` for a group of meshes that lie on the device.  ``meshes``: B x (verts [nv,3] float32, faces
    [nf,3] int32[, further arrays]) device tensors (the views the earlier stages return are used in place);
    ``max_move`` None, one number or B numbers (each mesh's own cap).  ONE call, no read-back but the B status words.
    -> (smoothed, status): B x (verts', faces[, arrays]) -- verts' views of one output with the bits of
    ``smooth_arrays``, the faces and every further array as they were given -- and the status words, int32 [B] on the
    host.  An empty mesh stays empty.  A mesh with a status (2 a face index out of range, 4 a coordinate that is not
    finite, 7 a coordinate beyond +-1024 at input or after a step) raises ValueError naming the mesh -- with
    ``strict=False`` it keeps its input vertices and the call returns."""
    import torch

    from . import ops
    from ._lib import check
    iters, lam, mu, max_move = smooth_params(iters, lam, mu, max_move)
    meshes = [tuple(m) for m in meshes]
    if not meshes:
        return [], np.zeros(0, np.int32)
    B, h = len(meshes), lib()
    cap = None
    if max_move is not None:
        if np.ndim(max_move) and np.shape(max_move) != (B,):
            raise ValueError("smooth: %d values of max_move for %d meshes" % (np.size(max_move), B))
        cap = np.ascontiguousarray(np.broadcast_to(np.asarray(max_move, np.float64), (B,)))
    v, v_off, f, f_off, ws = _pack_meshes(meshes, lambda nv, nf: h.disn_mesh_smooth_workspace_bytes(B, nv, nf))
    nv, dev = int(v_off[-1]), v.device
    with torch.cuda.device(dev):
        out = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        check("disn_mesh_smooth_batch", h.disn_mesh_smooth_batch(
            v.data_ptr(), f.data_ptr(), v_off.ctypes.data, f_off.ctypes.data, B, iters, lam, mu, 1 if pin_boundary else 0,
            None if cap is None else cap.ctypes.data, out.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(),
            ops._stream()))
        st = status.cpu().numpy()                               # the one host sync of the group
    for b in np.nonzero(st)[0] if strict else ():
        _raise_status(b, st[b], v_off, "disn_mesh_smooth_batch")
        if st[b] == STATUS_SMOOTH_RANGE:
            raise ValueError("mesh %d: a coordinate leaves +-%g (at input or after a step), or a vertex has more than "
                             "2^20 neighbours" % (b, SMOOTH_RANGE))
        raise RuntimeError("mesh %d: disn_mesh_smooth_batch gave status %d" % (b, st[b]))
    return [(out[int(v_off[b]):int(v_off[b + 1])],) + m[1:] for b, m in enumerate(meshes)], st


def smooth_arrays_device(verts, faces, **kw):
    """``smooth_arrays`` for one mesh on the device -> verts' (a device tensor with the bits of ``smooth_arrays``); the
    same ValueErrors"""
    return _one_mesh(smooth_meshes_device, [(verts, faces)], **kw)[0][0][0]


# ---- mesh checks on the device (mesh_check.hip) -------------------------------------------------------------------
def check_result(status: int, counts, area: float, volume: float) -> dict:
    """one mesh's status word, its DISN_CHECK_FIELDS counts and its two sums -> the dict of ``check_arrays``"""
    out = {"status": int(status)}
    out.update((k, int(c)) for k, c in zip(CHECK_FIELDS, counts))
    out.update(area=float(area), volume=float(volume))
    return _check_derive(out)


def check_meshes_device(meshes, max_pairs=None, face_flags: bool = False, strict: bool = True):
    """``check_arrays`` for a group of meshes that lie on the device.  ``meshes``: B x (verts [nv,3] float32, faces
    [nf,3] int32[, further arrays]) device tensors, used in place; ``max_pairs`` None (the default cap of every mesh),
    one number or B numbers.  ONE call and ONE device-to-host copy for the group: the status words, the counts and the
    sums travel in one buffer.
    -> B dicts with the integers of ``check_arrays`` (``area`` and ``volume`` up to the order of their sums, which is
    fixed: the same bits from run to run and in any batch); with ``face_flags`` -> (dicts, B uint8 [nf] device tensors
    with the bits of ``check_face_flags``).  A mesh with status 2 (a face index out of range) or 4 (a coordinate that is
    not finite) raises ValueError naming the mesh -- with ``strict=False`` its dict carries the status and -1 in the
    fields that status makes invalid.  Status 8 (more candidate pairs than the cap) never raises: the dict carries it."""
    import torch

    from . import ops
    from ._lib import check
    meshes = [tuple(m) for m in meshes]
    if not meshes:
        return ([], []) if face_flags else []
    B, h = len(meshes), lib()
    if max_pairs is not None and np.ndim(max_pairs) and np.shape(max_pairs) != (B,):
        raise ValueError("check: %d values of max_pairs for %d meshes" % (np.size(max_pairs), B))
    caps = np.ascontiguousarray([check_max_pairs(None if max_pairs is None else np.broadcast_to(max_pairs, (B,))[b],
                                                 m[1].shape[0]) for b, m in enumerate(meshes)], np.int64)
    v, v_off, f, f_off, ws = _pack_meshes(
        meshes, lambda nv, nf: h.disn_mesh_check_workspace_bytes(B, nv, nf, int(min(caps.sum(), 2 ** 62))))
    nf, dev = int(f_off[-1]), v.device
    words = 1 + len(CHECK_FIELDS) + 2                              # per mesh: status, the counts, the two sums
    with torch.cuda.device(dev):
        out = torch.empty(B * words, dtype=torch.int64, device=dev)
        status, counts, sums = out[:B].view(torch.int32), out[B:B * (1 + len(CHECK_FIELDS))], out[B * (words - 2):]
        flags = torch.empty(nf, dtype=torch.uint8, device=dev) if face_flags else None
        check("disn_mesh_check_batch", h.disn_mesh_check_batch(
            v.data_ptr(), f.data_ptr(), v_off.ctypes.data, f_off.ctypes.data, B, caps.ctypes.data, counts.data_ptr(),
            sums.view(torch.float64).data_ptr(), None if flags is None else flags.data_ptr(), status.data_ptr(),
            ws.data_ptr(), ws.numel(), ops._stream()))
        host = out.cpu().numpy()                                # the one copy (and host sync) of the group
    st = host[:B].view(np.int32)[:B]
    cnt = host[B:B * (1 + len(CHECK_FIELDS))].reshape(B, len(CHECK_FIELDS))
    sm = host[B * (words - 2):].view(np.float64).reshape(B, 2)
    for b in np.nonzero(st)[0] if strict else ():
        _raise_status(b, st[b], v_off, "disn_mesh_check_batch")
        if st[b] != STATUS_CHECK_PAIRS:
            raise RuntimeError("mesh %d: disn_mesh_check_batch gave status %d" % (b, st[b]))
    results = [check_result(st[b], cnt[b], sm[b, 0], sm[b, 1]) for b in range(B)]
    if not face_flags:
        return results
    return results, [flags[int(f_off[b]):int(f_off[b + 1])] for b in range(B)]


def check_arrays_device(verts, faces, max_pairs=None, face_flags: bool = False, strict: bool = True):
    """``check_arrays`` for one mesh on the device -> its dict (with ``face_flags``: (dict, uint8 [nf] device tensor));
    the ValueErrors of ``check_meshes_device``"""
    r = _one_mesh(check_meshes_device, [(verts, faces)], max_pairs=max_pairs, face_flags=face_flags, strict=strict)
    return (r[0][0], r[1][0]) if face_flags else r[0]


# ---- vertex colours on the device (mesh_colour.hip) -------------------------------------------------------------
# ---- mesh repair on the device (mesh_repair.hip) ------------------------------------------------------------------
def repair_report(counts, nv: int, nf: int) -> dict:
    """one mesh's DISN_REPAIR_FIELDS counts and its input sizes -> the report of ``repair_arrays``"""
    out = {"status": int(counts[REPAIR_FIELDS.index("status")]), "nv": int(nv), "nf": int(nf)}
    out.update((k, int(c)) for k, c in zip(REPAIR_FIELDS, counts) if k != "status")
    return out


def repair_meshes_device(meshes, weld: bool = True, stitch: bool = True, strict: bool = True):
    """``repair_arrays`` for a group of meshes that lie on the device.  ``meshes``: B x (verts [nv,3] float32, faces
    [nf,3] int32[, further per-vertex arrays]) device tensors (the views the earlier stages return are used in place).
    ONE count call, ONE read-back of the [B,12] sizes, ONE emit call.
    -> (repaired, reports): B x (verts', faces'[, arrays'], vmap int32 [nv'], kept int32 [nf']) views of the outputs --
    the integers and the position bits of ``repair_arrays``; a further array takes, for every output vertex, the row of
    the vertex it copies (``vmap``) -- and B reports, the dicts of ``repair_arrays``.  An empty mesh stays empty.  A mesh
    with status 2 (a face index out of range) or 4 (a coordinate that is not finite) raises ValueError naming the mesh --
    with ``strict=False`` it comes back unchanged and its report carries the status."""
    import torch

    from . import ops
    from ._lib import check
    meshes = [tuple(m) for m in meshes]
    if not meshes:
        return [], []
    B, h = len(meshes), lib()
    flags = (REPAIR_WELD if weld else 0) | (REPAIR_STITCH if stitch else 0)
    v, v_off, f, f_off, ws = _pack_meshes(meshes, lambda nv, nf: h.disn_mesh_repair_workspace_bytes(B, nv, nf))
    dev, K = v.device, len(REPAIR_FIELDS)
    with torch.cuda.device(dev):
        counts = torch.zeros((B, K), dtype=torch.int64, device=dev)
        st = ops._stream()
        check("disn_mesh_repair_count_batch", h.disn_mesh_repair_count_batch(
            v.data_ptr(), f.data_ptr(), v_off.ctypes.data, f_off.ctypes.data, B, flags, counts.data_ptr(), ws.data_ptr(),
            ws.numel(), st))
        sizes = np.ascontiguousarray(counts.cpu().numpy())      # the one host sync of the group
        status = sizes[:, REPAIR_FIELDS.index("status")]
        for b in np.nonzero(status)[0]:
            if strict or status[b] not in (STATUS_INDEX, STATUS_FINITE):
                _raise_status(b, status[b], v_off, "disn_mesh_repair_count_batch")
                raise RuntimeError("mesh %d: disn_mesh_repair_count_batch gave status %d" % (b, status[b]))
        nvo, nfo = int(sizes[:, 0].sum()), int(sizes[:, 1].sum())
        out_v = torch.empty((nvo, 3), dtype=torch.float32, device=dev)
        out_f = torch.empty((nfo, 3), dtype=torch.int32, device=dev)
        vmap = torch.empty(nvo, dtype=torch.int32, device=dev)
        kept = torch.empty(nfo, dtype=torch.int32, device=dev)
        if nvo or nfo:
            check("disn_mesh_repair_emit_batch", h.disn_mesh_repair_emit_batch(
                v.data_ptr(), f.data_ptr(), v_off.ctypes.data, f_off.ctypes.data, B, flags, sizes.ctypes.data,
                out_v.data_ptr(), out_f.data_ptr(), vmap.data_ptr(), kept.data_ptr(), ws.data_ptr(), ws.numel(), st))
    repaired, reports, v0, f0 = [], [], 0, 0
    for b, m in enumerate(meshes):
        nvb, nfb = int(sizes[b, 0]), int(sizes[b, 1])
        vm = vmap[v0:v0 + nvb]
        rest = tuple(x.index_select(0, vm.long()) for x in m[2:])
        repaired.append((out_v[v0:v0 + nvb], out_f[f0:f0 + nfb]) + rest + (vm, kept[f0:f0 + nfb]))
        reports.append(repair_report(sizes[b], v_off[b + 1] - v_off[b], f_off[b + 1] - f_off[b]))
        v0, f0 = v0 + nvb, f0 + nfb
    return repaired, reports


def repair_arrays_device(verts, faces, weld: bool = True, stitch: bool = True, strict: bool = True):
    """``repair_arrays`` for one mesh on the device -> (verts', faces', vmap, kept, report): device tensors with the
    integers and the position bits of ``repair_arrays``, and its report; the ValueErrors of ``repair_meshes_device``"""
    repaired, reports = _one_mesh(repair_meshes_device, [(verts, faces)], weld=weld, stitch=stitch, strict=strict)
    return repaired[0] + (reports[0],)


# ---- mesh closing on the device (mesh_close.hip) ------------------------------------------------------------------
def close_report(counts, nv: int, nf: int) -> dict:
    """one mesh's DISN_CLOSE_FIELDS counts and its input sizes -> the report of ``close_arrays``"""
    out = {"status": int(counts[CLOSE_FIELDS.index("status")]), "nv": int(nv), "nf": int(nf)}
    out.update((k, int(c)) for k, c in zip(CLOSE_FIELDS, counts) if k != "status")
    return out


def close_meshes_device(meshes, orient: bool = True, fill: bool = True, outward: bool = False, max_hole=None,
                        strict: bool = True):
    """``close_arrays`` for a group of meshes that lie on the device.  ``meshes``: B x (verts [nv,3] float32, faces
    [nf,3] int32[, further per-vertex arrays]) device tensors (the views the earlier stages return are used in place).
    ONE count call, ONE read-back of the [B,9] sizes, ONE emit call.
    -> (closed, reports): B x (verts', faces'[, arrays'], vmap int32 [nv'], kept int32 [nf']) views of the outputs --
    the integers and the position bits of ``close_arrays``; a further array takes, for every output vertex, the row of
    ``vmap``: its own for an input vertex, that of its loop's smallest vertex for a centre -- and B reports, the dicts
    of ``close_arrays``.  An empty mesh stays empty.  A mesh with status 2 (a face index out of range), 4 (a coordinate
    that is not finite) or 16 (not manifold: ``repair_meshes_device`` comes first) raises ValueError naming the mesh --
    with ``strict=False`` it comes back unchanged and its report carries the status."""
    import torch

    from . import ops
    from ._lib import check
    flags, cap = close_flags(orient, fill, outward, max_hole)
    meshes = [tuple(m) for m in meshes]
    if not meshes:
        return [], []
    B, h = len(meshes), lib()
    v, v_off, f, f_off, ws = _pack_meshes(meshes, lambda nv, nf: h.disn_mesh_close_workspace_bytes(B, nv, nf))
    dev, K = v.device, len(CLOSE_FIELDS)
    with torch.cuda.device(dev):
        counts = torch.zeros((B, K), dtype=torch.int64, device=dev)
        st = ops._stream()
        check("disn_mesh_close_count_batch", h.disn_mesh_close_count_batch(
            v.data_ptr(), f.data_ptr(), v_off.ctypes.data, f_off.ctypes.data, B, flags, cap, counts.data_ptr(),
            ws.data_ptr(), ws.numel(), st))
        sizes = np.ascontiguousarray(counts.cpu().numpy())      # the one host sync of the group
        status = sizes[:, CLOSE_FIELDS.index("status")]
        for b in np.nonzero(status)[0]:
            if strict or status[b] not in (STATUS_INDEX, STATUS_FINITE, STATUS_NOT_MANIFOLD):
                _raise_status(b, status[b], v_off, "disn_mesh_close_count_batch")
                if status[b] == STATUS_NOT_MANIFOLD:
                    raise ValueError("mesh %d: not manifold (a repeated index, an edge of three faces or a vertex on "
                                     "more than two boundary edges): repair it first" % b)
                raise RuntimeError("mesh %d: disn_mesh_close_count_batch gave status %d" % (b, status[b]))
        nvo, nfo = int(sizes[:, 0].sum()), int(sizes[:, 1].sum())
        out_v = torch.empty((nvo, 3), dtype=torch.float32, device=dev)
        out_f = torch.empty((nfo, 3), dtype=torch.int32, device=dev)
        vmap = torch.empty(nvo, dtype=torch.int32, device=dev)
        kept = torch.empty(nfo, dtype=torch.int32, device=dev)
        if nvo or nfo:
            check("disn_mesh_close_emit_batch", h.disn_mesh_close_emit_batch(
                v.data_ptr(), f.data_ptr(), v_off.ctypes.data, f_off.ctypes.data, B, flags, cap, sizes.ctypes.data,
                out_v.data_ptr(), out_f.data_ptr(), vmap.data_ptr(), kept.data_ptr(), ws.data_ptr(), ws.numel(), st))
    closed, reports, v0, f0 = [], [], 0, 0
    for b, m in enumerate(meshes):
        nvb, nfb = int(sizes[b, 0]), int(sizes[b, 1])
        vm = vmap[v0:v0 + nvb]
        rest = tuple(x.index_select(0, vm.long()) for x in m[2:])
        closed.append((out_v[v0:v0 + nvb], out_f[f0:f0 + nfb]) + rest + (vm, kept[f0:f0 + nfb]))
        reports.append(close_report(sizes[b], v_off[b + 1] - v_off[b], f_off[b + 1] - f_off[b]))
        v0, f0 = v0 + nvb, f0 + nfb
    return closed, reports


def close_arrays_device(verts, faces, orient: bool = True, fill: bool = True, outward: bool = False, max_hole=None,
                        strict: bool = True):
    """``close_arrays`` for one mesh on the device -> (verts', faces', vmap, kept, report): device tensors with the
    integers and the position bits of ``close_arrays``, and its report; the ValueErrors of ``close_meshes_device``"""
    closed, reports = _one_mesh(close_meshes_device, [(verts, faces)], orient=orient, fill=fill, outward=outward,
                                max_hole=max_hole, strict=strict)
    return closed[0] + (reports[0],)


def _colour_inputs(meshes, trans_mats, views_per_mesh: int, S: int):
    """-> (B, V, verts, v_off, faces, f_off, trans_mat [B,V,4,3] device, workspace)"""
    import torch
    if S not in COLOUR_SAMPLES:
        raise ValueError("S must be one of %s, got %r" % (COLOUR_SAMPLES, S))
    V, B = int(views_per_mesh), len(meshes)
    if not 1 <= V <= COLOUR_MAX_VIEWS:
        raise ValueError("views_per_mesh must be in 1..%d, got %r" % (COLOUR_MAX_VIEWS, views_per_mesh))
    v, v_off, f, f_off, ws = _pack_meshes(
        meshes, lambda nv, nf: lib().disn_mesh_colour_workspace_bytes(B, V, nv, nf, int(S)), "%d views, " % V)
    dev = v.device
    tm = torch.as_tensor(np.ascontiguousarray(trans_mats.detach().cpu().numpy() if hasattr(trans_mats, "detach")
                                              else trans_mats, np.float32))
    if tm.numel() != B * V * 12:
        raise ValueError("trans_mats must hold %d meshes x %d views x [4,3], got %s" % (B, V, tuple(tm.shape)))
    tm_d = torch.empty((B, V, 4, 3), dtype=torch.float32, device=dev)
    tm_d.copy_(tm.reshape(B, V, 4, 3))
    return B, V, v, v_off, f, f_off, tm_d, ws


def _colour_status(status, v_off, strict: bool, entry: str) -> np.ndarray:
    st = status.cpu().numpy()
    for b in np.nonzero(st)[0] if strict else ():
        _raise_status(b, st[b], v_off, entry)
        raise RuntimeError("mesh %d: status %d" % (b, st[b]))
    return st


def zbuffer_meshes_device(meshes, trans_mats, views_per_mesh: int = 1, S: int = 2, strict: bool = True):
    """``zbuffer_arrays`` for a group of meshes that lie on the device: depth maps without a BVH.  ``meshes``: B x
    (verts [nv,3] float32, faces [nf,3] int32, ...) device tensors; ``trans_mats`` [B, V, 4, 3] (host or device), V =
    ``views_per_mesh``.  -> [B, V, 137 S, 137 S] float32 device tensor with the bits of ``zbuffer_arrays`` (q = 1/w, 0
    empty).  ValueError for a face index out of range or a coordinate that is not finite -- with ``strict=False`` such
    a mesh gets empty maps and the call returns (zbuf, status int32 [B] on the host)."""
    import torch

    from . import ops
    from ._lib import check
    meshes = [tuple(m) for m in meshes]
    if not meshes:
        return torch.zeros((0, int(views_per_mesh), IMG * S, IMG * S)) if strict else (None, np.zeros(0, np.int32))
    B, V, v, v_off, f, f_off, tm, ws = _colour_inputs(meshes, trans_mats, views_per_mesh, S)
    dev = v.device
    with torch.cuda.device(dev):
        zbuf = torch.empty((B, V, IMG * S, IMG * S), dtype=torch.float32, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        check("disn_mesh_zbuffer_batch", lib().disn_mesh_zbuffer_batch(
            v.data_ptr(), f.data_ptr(), v_off.ctypes.data, f_off.ctypes.data, B, tm.data_ptr(), V, int(S),
            zbuf.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream()))
        st = _colour_status(status, v_off, strict, "disn_mesh_zbuffer_batch")
    return zbuf if strict else (zbuf, st)


def colour_meshes_device(meshes, imgs, trans_mats, views_per_mesh: int = 1, alpha=None, S: int = 2,
                         rel_tol: float = 1e-3, mirror_axis=None, fill_iters: int = 32, bgr: bool = True,
                         strict: bool = True):
    """``colour_arrays`` for a group of meshes that lie on the device.  ``meshes``: B x (verts [nv,3] float32, faces
    [nf,3] int32, ...) device tensors (the views the earlier stages return are used in place); ``imgs`` [B, V, 137, 137,
    3] float32 device tensor in [0,1] (or anything with that many elements), ``trans_mats`` [B, V, 4, 3], ``alpha`` None
    or [B, V, 137, 137] uint8; V = ``views_per_mesh``.  ONE call, no read-back but the B status words.
    -> (colours, seen): B x uint8 [nv,3] (R G B) and B x uint8 [nv] (the class) device views, the bytes of
    ``colour_arrays``.  An empty mesh gives empty arrays.  ValueError for a face index out of range or a coordinate that
    is not finite -- with ``strict=False`` such a mesh is mid grey, class 0, and the call returns (colours, seen,
    status int32 [B] on the host)."""
    import torch

    from . import ops
    from ._lib import check
    S, tol, axis, fill_iters = _colour_params(S, rel_tol, mirror_axis, fill_iters)
    meshes = [tuple(m) for m in meshes]
    if not meshes:
        return ([], []) if strict else ([], [], np.zeros(0, np.int32))
    B, V, v, v_off, f, f_off, tm, ws = _colour_inputs(meshes, trans_mats, views_per_mesh, S)
    dev, nv = v.device, int(v_off[-1])
    if not (isinstance(imgs, torch.Tensor) and imgs.is_cuda and imgs.dtype == torch.float32
            and imgs.numel() == B * V * IMG * IMG * 3):
        raise TypeError("imgs must be a float32 CUDA tensor of %d x %d x 137 x 137 x 3 values (the HIP path has no CPU "
                        "fallback)" % (B, V))
    imgs = imgs.contiguous()
    if alpha is not None:
        if not (isinstance(alpha, torch.Tensor) and alpha.is_cuda and alpha.dtype == torch.uint8
                and alpha.numel() == B * V * IMG * IMG):
            raise TypeError("alpha must be a uint8 CUDA tensor of %d x %d x 137 x 137 values" % (B, V))
        alpha = alpha.contiguous()
    with torch.cuda.device(dev):
        colours = torch.empty((nv, 3), dtype=torch.uint8, device=dev)
        seen = torch.empty(nv, dtype=torch.uint8, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        check("disn_mesh_colour_batch", lib().disn_mesh_colour_batch(
            v.data_ptr(), f.data_ptr(), v_off.ctypes.data, f_off.ctypes.data, B, imgs.data_ptr(),
            None if alpha is None else alpha.data_ptr(), tm.data_ptr(), V, S, float(tol), axis, fill_iters,
            1 if bgr else 0, colours.data_ptr(), seen.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(),
            ops._stream()))
        st = _colour_status(status, v_off, strict, "disn_mesh_colour_batch")
    cs = [colours[int(v_off[b]):int(v_off[b + 1])] for b in range(B)]
    ss = [seen[int(v_off[b]):int(v_off[b + 1])] for b in range(B)]
    return (cs, ss) if strict else (cs, ss, st)


def colour_arrays_device(verts, faces, images, trans_mats, alpha=None, **kw):
    """``colour_arrays`` for one mesh on the device: images [V,137,137,3] device float32, trans_mats [V,4,3], alpha None
    or [V,137,137] device uint8 -> (colours uint8 [nv,3], seen uint8 [nv]) device tensors; the same ValueErrors"""
    V = int(np.asarray(trans_mats.shape if hasattr(trans_mats, "shape") else np.shape(trans_mats))[:-2].prod())
    cs, ss = _one_mesh(colour_meshes_device, [(verts, faces)], images, trans_mats, views_per_mesh=max(V, 1), alpha=alpha,
                       **kw)
    return cs[0], ss[0]


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

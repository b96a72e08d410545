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


def _batch_args(sdf: torch.Tensor, sdf_params, res: int, max_edge_slots: int):
    """the arguments of a batched mesher -> (sdf checked, sdf_params as float64 [B,6], grids per round)"""
    n = res + 1
    if sdf.dim() != 2 or sdf.shape[1] != n * n * n:
        raise ValueError("sdf must be [B, (res+1)^3 = %d], got %s" % (n * n * n, tuple(sdf.shape)))
    sdf = ops._chk(sdf, "sdf")
    B = sdf.shape[0]
    sp = np.ascontiguousarray(np.asarray(sdf_params, np.float64).reshape(-1, 6))
    if sp.shape[0] != B:
        raise ValueError("sdf_params must be [B,6] with B = %d, got %s" % (B, sp.shape))
    return sdf, sp, (min(int(max_edge_slots), MC_EDGE_SLOTS) - 1) // (3 * n * n * n)


def _batch_rounds(sdf: torch.Tensor, sp: np.ndarray, res: int, per: int, ws: Optional[torch.Tensor], ws_bytes,
                  width: int, count, emit) -> List[Tuple[torch.Tensor, ...]]:
    """The rounds of a batched mesher, ``per`` grids each: the workspace grown to ``ws_bytes(nb, res)``,
    ``count(part, nb, counts, ws, st)`` fills the [nb, width] sizes, ONE device-to-host copy brings them over,
    ``emit(b0, part, boxes, nb, sizes, ws, st)`` -> the round's arrays as (tensor, its column of ``sizes``), all grids
    back to back.  -> per grid the tuple of its views of those arrays."""
    B = sdf.shape[0]
    if B and (per < 1 or ws_bytes(1, res) == 0):
        raise ValueError("unsupported resolution %d" % res)
    dev = sdf.device
    out: List[Tuple[torch.Tensor, ...]] = []
    with torch.cuda.device(dev):
        st = ops._stream()
        for b0 in range(0, B, max(per, 1)):
            nb = min(per, B - b0)
            need = ws_bytes(nb, res)
            if ws is None or ws.numel() < need:
                ws = torch.empty(need, dtype=torch.uint8, device=dev)
            part, boxes = sdf[b0:b0 + nb], sp[b0:b0 + nb]
            counts = torch.zeros((nb, width), dtype=torch.int64, device=dev)
            count(part, nb, counts, ws, st)
            sizes = counts.cpu().numpy()                   # the one host sync of the round: sizes are data dependent
            arrays = emit(b0, part, boxes, nb, sizes, ws, st)
            offs = [np.concatenate([[0], np.cumsum(sizes[:, col])]).tolist() for _, col in arrays]
            for k in range(nb):
                out.append(tuple(a[o[k]:o[k + 1]] for (a, _), o in zip(arrays, offs)))
    return out


def marching_cubes_batch(sdf: torch.Tensor, sdf_params, res: int, iso: float = 0.0,
                         ws: Optional[torch.Tensor] = None, max_edge_slots: int = MC_EDGE_SLOTS
                         ) -> List[Tuple[torch.Tensor, torch.Tensor]]:
    """sdf: float32 device tensor [B,(res+1)^3], sdf_params [B,6] -> B x (verts [nv,3], faces [nf,3]), views of
    two device tensors; every pair is bit for bit what ``marching_cubes`` gives for that grid alone.  One count
    call, ONE device-to-host copy of the [B,2] sizes and one emit call for the whole batch; a batch whose
    3*B*(res+1)^3 edge slots reach ``max_edge_slots`` is meshed in several such rounds."""
    sdf, sp, per = _batch_args(sdf, sdf_params, res, max_edge_slots)
    dev = sdf.device

    def count(part, nb, counts, ws, st):
        check("disn_mc_count_batch", lib().disn_mc_count_batch(part.data_ptr(), nb, res, float(iso),
                                                               counts.data_ptr(), ws.data_ptr(), ws.numel(), st))

    def emit(b0, part, boxes, nb, sizes, ws, st):
        nv, nf = int(sizes[:, 0].sum()), int(sizes[:, 1].sum())
        verts = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((nf, 3), dtype=torch.int32, device=dev)
        if nv and nf:
            check("disn_mc_emit_batch", lib().disn_mc_emit_batch(part.data_ptr(), boxes.ctypes.data, nb, res,
                                                                 float(iso), verts.data_ptr(), faces.data_ptr(),
                                                                 ws.data_ptr(), ws.numel(), st))
        return (verts, 0), (faces, 1)

    return _batch_rounds(sdf, sp, res, per, ws, lib().disn_mc_batch_workspace_bytes, 2, count, emit)


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


# ---- dual contouring from Hermite data (include/dc/disn_amd_dc.h) ----------------------------------------------
# cube edge -> (dx, dy, dz) of its lower grid point and its axis: tools/gen_mc_tables.edge_geometry(), the order in
# which a cell visits its cut edges (csrc/mc_tables.h kMcEdge is the same table)
DC_CUBE_EDGES = ((0, 0, 0, 0), (1, 0, 0, 1), (0, 1, 0, 0), (0, 0, 0, 1), (0, 0, 1, 0), (1, 0, 1, 1), (0, 1, 1, 0),
                 (0, 0, 1, 1), (0, 0, 0, 2), (1, 0, 0, 2), (1, 1, 0, 2), (0, 1, 0, 2))
DC_REG = 2.0 ** -10          # the regulariser ``postprocess.simplify_arrays`` uses; NOT measured on a trained network's normals
_DC_QUAD = ((-1, -1), (0, -1), (0, 0), (-1, 0))      # (u, v) offsets of the cells q0 .. q3 around an edge


def _dc_axes(sdf_params, R: int):
    """the float32 axis values ``disn_mc_emit`` uses for the box (numpy.linspace in float64, cast)"""
    p = np.asarray(sdf_params, np.float64).reshape(6)
    return [np.linspace(p[a], p[a + 3], num=R + 1).astype(np.float32) for a in range(3)]


class _DcEdges:
    """the cut grid edges of one grid in rank order (flat order 3*p + axis), with what every rule below needs"""

    def __init__(self, vol, sdf_params, iso):
        vol = np.ascontiguousarray(vol, np.float32).reshape(-1)
        n = int(round(vol.size ** (1.0 / 3.0)))
        if n < 2 or n * n * n != vol.size:
            raise ValueError("vol must hold (R+1)^3 values with R >= 1, got %d" % vol.size)
        self.vol, self.n, self.R = vol, n, n - 1
        self.iso = np.float32(iso)
        self.ax = _dc_axes(sdf_params, n - 1)
        cube = vol.reshape(n, n, n)
        self.inside = cube < self.iso
        flags = np.zeros((n, n, n, 3), bool)
        flags[:, :, :-1, 0] = self.inside[:, :, :-1] != self.inside[:, :, 1:]
        flags[:, :-1, :, 1] = self.inside[:, :-1, :] != self.inside[:, 1:, :]
        flags[:-1, :, :, 2] = self.inside[:-1, :, :] != self.inside[1:, :, :]
        self.flat = flags.reshape(-1)
        self.eidx = np.cumsum(self.flat, dtype=np.int64) - self.flat          # exclusive scan: an edge's rank
        act = np.nonzero(self.flat)[0]
        self.p, self.axis = act // 3, act % 3
        self.idx = np.stack([self.p % n, (self.p // n) % n, self.p // (n * n)], 1)       # ix, iy, iz
        self.step = np.array([1, n, n * n])[self.axis]
        self.v0, self.v1 = vol[self.p], vol[self.p + self.step]
        with np.errstate(all="ignore"):
            self.t = ((self.iso - self.v0) / (self.v1 - self.v0)).astype(np.float32)
        ia = self.idx[np.arange(len(act)), self.axis] if len(act) else np.zeros(0, np.int64)
        self.c0 = np.zeros(len(act), np.float32)
        self.c1 = np.zeros(len(act), np.float32)
        for a in range(3):
            m = self.axis == a
            self.c0[m], self.c1[m] = self.ax[a][ia[m]], self.ax[a][ia[m] + 1]

    def points(self) -> np.ndarray:
        pts = np.stack([self.ax[k][self.idx[:, k]] for k in range(3)], 1).astype(np.float32)
        with np.errstate(all="ignore"):
            cut = (self.c0 + (self.t * (self.c1 - self.c0).astype(np.float32)).astype(np.float32)).astype(np.float32)
        for a in range(3):
            m = self.axis == a
            pts[m, a] = cut[m]
        return pts.reshape(-1, 3)


def hermite_points_arrays(vol, sdf_params, iso: float = 0.0) -> np.ndarray:
    """The Hermite points of a grid on the host: one per cut grid edge, ranked in the flat order 3*p + axis
    (p = (iz*n + iy)*n + ix, inside = vol < float32(iso)), c0 + t*(c1 - c0) on the cut axis with
    t = (iso - v0)/(v1 - v0) in float32 -- bit for bit and in order the vertices ``marching_cubes`` gives for the same
    grid.  ``vol``: (R+1)^3 float32 values in ``.dist`` order -> float32 [ne,3]."""
    return _DcEdges(vol, sdf_params, iso).points()


def grid_normals_arrays(vol, sdf_params, iso: float = 0.0) -> np.ndarray:
    """The field's finite-difference gradient at the Hermite points, for callers without a network: THE SPECIFICATION
    of ``disn_dc_grid_normals_batch``.  At the point of an edge of axis a between grid points p0, p1, in float64 from
    the float32 values: g_a = (v1 - v0)/(c1 - c0); for another axis k, g_k = (1 - t) D_k(p0) + t D_k(p1) with the
    float32 t of the point and D_k(p) = (vol[p + e_k] - vol[p - e_k]) / (ax_k[i+1] - ax_k[i-1]), the indices clamped
    to the grid.  Cast to float32, NOT normalised -> float32 [ne,3] in the points' order."""
    E = _DcEdges(vol, sdf_params, iso)
    n, R = E.n, E.R
    vol = E.vol.astype(np.float64)
    t = E.t.astype(np.float64)
    g = np.zeros((len(E.p), 3), np.float64)
    with np.errstate(all="ignore"):
        for k in range(3):
            stepk = (1, n, n * n)[k]
            axk = E.ax[k].astype(np.float64)
            on = E.axis == k
            g[on, k] = (E.v1[on].astype(np.float64) - E.v0[on].astype(np.float64)) \
                / (E.c1[on].astype(np.float64) - E.c0[on].astype(np.float64))
            off = ~on
            i = E.idx[off, k]
            ip, im = np.minimum(i + 1, R), np.maximum(i - 1, 0)
            den = axk[ip] - axk[im]
            d = []
            for pt in (E.p[off], E.p[off] + E.step[off]):
                d.append((vol[pt + (ip - i) * stepk] - vol[pt - (i - im) * stepk]) / den)
            g[off, k] = (1.0 - t[off]) * d[0] + t[off] * d[1]
        return g.astype(np.float32)


def dual_contour_arrays(vol, sdf_params, iso, normals, reg: float = DC_REG) -> Tuple[np.ndarray, np.ndarray]:
    """Dual contouring of one grid from Hermite data, on the host: THE SPECIFICATION of ``dual_contour`` /
    ``dual_contour_batch`` (same position bits, same integers).  ``vol``: (R+1)^3 float32 in ``.dist`` order,
    ``normals`` float32 [ne,3]: the field's gradient at ``hermite_points_arrays(vol, sdf_params, iso)``, any length
    -> (verts float32 [nv,3], faces int32 [nf,3]).

    Cells: a cell of the R^3 cells is active when any of its 12 edges is cut; its vertex id is its rank among the
    active cells in flat (iz,iy,ix) order.
    Quadric of a cell, float64, relative to its low corner: d_i = double(point_i) - double(corner); the cut edges in
    the order of ``DC_CUBE_EDGES``; a row with normal g: s = (gx gx + gy gy) + gz gz; s finite and positive:
    A += g g^T / s, b -= g (g.d) / s (no square root); otherwise nothing is added to A and b.  Every cut edge counts
    in the mean m of the d_i.
    Position: lam = reg tr(A)/3 + 2^-40; x solves (A + lam I) x = lam m - b by the adjugate in the operation order of
    ``postprocess._simplify_solve``; det <= 0 or x not finite: x = m; x is clipped to the cell
    [0, double(ax[i+1]) - double(ax[i])] per axis; v = float32(double(corner) + x).  ``reg`` in (0, 1]; the default
    2^-10 is the constant ``simplify_arrays`` uses -- whether it is the best value on a trained network's normals has
    NOT been measured.
    Faces: the cut edges in rank order; an edge of axis a has a quad when its two other indices are in 1..R-1; (u, v)
    the two axes after a in cyclic order; the cells at (u, v) offsets (-1,-1), (0,-1), (0,0), (-1,0) are q0..q3; split
    along q0-q2 unless |q1-q3|^2 < |q0-q2|^2 (float64 of the float32 positions, (dx^2+dy^2)+dz^2; equality keeps
    q0-q2).  Low end of the edge inside: (q0,q1,q2),(q0,q2,q3) or (q0,q1,q3),(q1,q2,q3); otherwise each triangle has
    its last two indices swapped: the geometric normal points along +grad (``refine_mesh``).  Edges on the grid's
    boundary leave the surface open there, as marching cubes does.
    KNOWN LIMITS: in a cell that the surface crosses in more than one sheet one vertex serves both sheets, so the mesh
    can be non-manifold there (``dual_contour_sheets_arrays`` gives every sheet its own vertex); triangles may be
    degenerate in position, never in index."""
    reg = float(reg)
    if not (0.0 < reg <= 1.0):
        raise ValueError("reg must be in (0, 1], got %r" % (reg,))
    E, pts, nrm = _dc_hermite(vol, sdf_params, iso, normals)
    active = _dc_cases(E)[1].reshape(-1)
    cid = np.cumsum(active, dtype=np.int64) - active
    cells = np.nonzero(active)[0]
    verts = _dc_vertices(E, pts, nrm, cells, None, reg)
    return verts.reshape(-1, 3), _dc_faces(E, verts, lambda k, cell, axis: cid[cell])


def _dc_hermite(vol, sdf_params, iso, normals):
    """the edges of a grid, their points and the given normals in float64 (ValueError for normals of another shape)"""
    E = _DcEdges(vol, sdf_params, iso)
    pts = E.points().astype(np.float64)
    nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3).astype(np.float64)
    if nrm.shape != pts.shape:
        raise ValueError("normals must be [ne,3] with ne = %d, got %s" % (pts.shape[0], nrm.shape))
    return E, pts, nrm


def _dc_cases(E):
    """per cell [R,R,R]: its marching-cubes case (bit i = corner i of ``gen_mc_tables`` inside) and whether it is
    active (its eight corners not all on one side)"""
    R, ins = E.R, E.inside
    case = np.zeros((R, R, R), np.int32)
    cnt8 = np.zeros((R, R, R), np.int32)
    for i, (dx, dy, dz) in enumerate(_DC_CORNERS):
        c = ins[dz:dz + R, dy:dy + R, dx:dx + R]
        case |= c.astype(np.int32) << i
        cnt8 += c
    return case, (cnt8 != 0) & (cnt8 != 8)


def _dc_vertices(E, pts, nrm, cells, member, reg):
    """one vertex per entry of ``cells`` (flat cell ids, a cell may repeat): the quadric of the cell's cut edges, or --
    ``member`` bool [len(cells),12] -- of those of its cube edges that ``member`` names (all of them cut)"""
    n, R = E.n, E.R
    cx, cy, cz = cells % R, (cells // R) % R, cells // (R * R)
    ci = np.stack([cx, cy, cz], 1)
    corner = np.stack([E.ax[k][ci[:, k]].astype(np.float64) for k in range(3)], 1).reshape(-1, 3)
    hi = np.stack([E.ax[k][ci[:, k] + 1].astype(np.float64) for k in range(3)], 1).reshape(-1, 3) - corner
    nc = len(cells)
    A = {k: np.zeros(nc) for k in ("xx", "xy", "xz", "yy", "yz", "zz")}
    b = [np.zeros(nc) for _ in range(3)]
    sm = [np.zeros(nc) for _ in range(3)]
    cnt = np.zeros(nc)
    with np.errstate(all="ignore"):
        for e, (dx, dy, dz, a) in enumerate(DC_CUBE_EDGES):
            slot = 3 * (((cz + dz) * n + (cy + dy)) * n + (cx + dx)) + a
            cut = E.flat[slot] if member is None else member[:, e]
            r = np.where(cut, E.eidx[slot], 0)
            if not len(pts):
                break
            d = [pts[r, k] - corner[:, k] for k in range(3)]
            for k in range(3):
                sm[k] = np.where(cut, sm[k] + d[k], sm[k])
            cnt = np.where(cut, cnt + 1.0, cnt)
            gx, gy, gz = nrm[r, 0], nrm[r, 1], nrm[r, 2]
            s = (gx * gx + gy * gy) + gz * gz
            ok = cut & np.isfinite(s) & (s > 0.0)
            gd = (gx * d[0] + gy * d[1]) + gz * d[2]
            for key, u, v in (("xx", gx, gx), ("xy", gx, gy), ("xz", gx, gz), ("yy", gy, gy), ("yz", gy, gz), ("zz", gz, gz)):
                A[key] = np.where(ok, A[key] + (u * v) / s, A[key])
            for k, u in enumerate((gx, gy, gz)):
                b[k] = np.where(ok, b[k] - (u * gd) / s, b[k])
        mx, my, mz = sm[0] / cnt, sm[1] / cnt, sm[2] / cnt
        axx, axy, axz, ayy, ayz, azz = (A[k] for k in ("xx", "xy", "xz", "yy", "yz", "zz"))
        lam = (((axx + ayy) + azz) * reg) / 3.0 + 9.094947017729282e-13                  # reg tr / 3 + 2^-40
        m00, m11, m22 = axx + lam, ayy + lam, azz + lam
        m01, m02, m12 = axy, axz, ayz
        r0, r1, r2 = lam * mx - b[0], lam * my - b[1], lam * mz - b[2]
        c00 = m11 * m22 - m12 * m12
        c01 = m02 * m12 - m01 * m22
        c02 = m01 * m12 - m02 * m11
        c11 = m00 * m22 - m02 * m02
        c12 = m01 * m02 - m00 * m12
        c22 = m00 * m11 - m01 * m01
        det = (m00 * c00 + m01 * c01) + m02 * c02
        x0 = ((c00 * r0 + c01 * r1) + c02 * r2) / det
        x1 = ((c01 * r0 + c11 * r1) + c12 * r2) / det
        x2 = ((c02 * r0 + c12 * r1) + c22 * r2) / det
        ok = (det > 0.0) & np.isfinite(x0) & np.isfinite(x1) & np.isfinite(x2)
        x = np.where(ok[:, None], np.stack([x0, x1, x2], 1), np.stack([mx, my, mz], 1)).reshape(-1, 3)
        x = np.where(x < 0.0, 0.0, np.where(x > hi, hi, x))
        return (corner + x).astype(np.float32)


def _dc_faces(E, verts, vertex_of):
    """the triangles of the cut edges with a quad, in rank order; ``vertex_of(k, cell, axis)`` -> the vertex ids that
    the flat cells ``cell`` (q_k of edges of axes ``axis``) contribute"""
    R, ins = E.R, E.inside
    u, v = (E.axis + 1) % 3, (E.axis + 2) % 3
    rows = np.arange(len(E.p))
    iu, iv = E.idx[rows, u] if len(rows) else rows, E.idx[rows, v] if len(rows) else rows
    has = (iu >= 1) & (iu <= R - 1) & (iv >= 1) & (iv <= R - 1)
    sel = np.nonzero(has)[0]
    if not len(sel):
        return np.zeros((0, 3), np.int32)
    q = []
    for k, (du, dv) in enumerate(_DC_QUAD):
        c = E.idx[sel].copy()
        c[np.arange(len(sel)), u[sel]] += du
        c[np.arange(len(sel)), v[sel]] += dv
        q.append(vertex_of(k, (c[:, 2] * R + c[:, 1]) * R + c[:, 0], E.axis[sel]))
    P = [verts[k].astype(np.float64) for k in q]
    d02, d13 = P[0] - P[2], P[1] - P[3]
    d02 = (d02[:, 0] * d02[:, 0] + d02[:, 1] * d02[:, 1]) + d02[:, 2] * d02[:, 2]
    d13 = (d13[:, 0] * d13[:, 0] + d13[:, 1] * d13[:, 1]) + d13[:, 2] * d13[:, 2]
    other = d13 < d02
    t1 = np.where(other[:, None], np.stack([q[0], q[1], q[3]], 1), np.stack([q[0], q[1], q[2]], 1))
    t2 = np.where(other[:, None], np.stack([q[1], q[2], q[3]], 1), np.stack([q[0], q[2], q[3]], 1))
    tri = np.stack([t1, t2], 1).reshape(-1, 3)
    flip = np.repeat(~ins.reshape(-1)[E.p[sel]], 2)
    tri[flip] = tri[flip][:, [0, 2, 1]]
    return tri.astype(np.int32)


# the cell's corners in the order of the case bits (tools/gen_mc_tables.CORNERS)
_DC_CORNERS = ((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1))


def _dcs_quad_edges():
    """[axis][k]: the cube-edge id under which cell q_k sees a grid edge of that axis -- the cube edge of the same axis
    whose low corner lies at (-du, -dv) on the (u, v) axes, (du, dv) = q_k's offset"""
    out = []
    for a in range(3):
        u, v = (a + 1) % 3, (a + 2) % 3
        out.append(tuple([e for e, g in enumerate(DC_CUBE_EDGES) if g[3] == a and (g[u], g[v]) == (-du, -dv)][0]
                         for du, dv in _DC_QUAD))
    return tuple(out)


DCS_QUAD_EDGES = _dcs_quad_edges()


def dual_contour_sheets_arrays(vol, sdf_params, iso, normals, reg: float = DC_REG) -> Tuple[np.ndarray, np.ndarray]:
    """Dual contouring with one vertex per SHEET of a cell, on the host: THE SPECIFICATION of
    ``dual_contour_batch(sheets=True)`` (same position bits, same integers).  Arguments, Hermite points, their order
    and ``normals`` are those of ``dual_contour_arrays`` -> (verts float32 [nv,3], faces int32 [nf,3]).

    Case of a cell: bit i set when corner i is inside (vol < float32(iso)), in the corner order of
    ``tools/gen_mc_tables``.  The cut edges of a case lie on closed loops, one per sheet of the surface in the cell
    (``mc_loops.MC_NLOOP`` / ``MC_LOOP``, derived by ``tools/gen_mc_loops.py``: 0..4 loops of 3..7 edges, numbered by
    their smallest cube-edge id).
    Vertex ids: the cells in flat (iz,iy,ix) order, the loops of a cell in loop-id order:
    id = (exclusive scan of MC_NLOOP[case] over the cells)[cell] + loop; nv = the sum of the loop counts.
    Quadric of a (cell, loop): ``dual_contour_arrays``' quadric restricted to the loop's edges -- visited in cube-edge-id
    order, the same float64 arithmetic, the same s = g.g rule for NaN, infinite and zero rows, the mean m over the
    loop's edges only, the same lam, adjugate solve, fallback to m and clip to the cell.  A loop in a one-loop cell has
    ``dual_contour_arrays``' vertex bit for bit; a grid whose active cells all have one loop gives its mesh bit for bit.
    Faces: the quads, their order, the shorter-diagonal split, the tie rule and the winding flip are
    ``dual_contour_arrays``' (ne and nf too); the index of cell q_k is base[cell] + MC_LOOP[case(cell)][e], e the cube
    edge under which that cell sees the grid edge (``DCS_QUAD_EDGES[axis][k]``).
    KNOWN LIMIT that remains: when two cells share an ambiguous face (four cut edges) and in BOTH cells both of that
    face's segments lie on one loop, the two dual edges across the face join the same two vertices; that edge then
    carries four faces (three where a quad is missing at the grid's boundary).  Curing it means re-pairing such faces
    per grid; not built.  Triangles may be degenerate in position, never in index."""
    from .mc_loops import MC_LOOP, MC_NLOOP
    reg = float(reg)
    if not (0.0 < reg <= 1.0):
        raise ValueError("reg must be in (0, 1], got %r" % (reg,))
    E, pts, nrm = _dc_hermite(vol, sdf_params, iso, normals)
    case = _dc_cases(E)[0].reshape(-1)
    nloop = np.asarray(MC_NLOOP, np.int64)[case]
    loops = np.asarray(MC_LOOP, np.int64)
    base = np.cumsum(nloop) - nloop
    cells = np.repeat(np.arange(len(case)), nloop)
    which = np.arange(len(cells)) - base[cells]
    member = loops[case[cells]] == which[:, None]
    verts = _dc_vertices(E, pts, nrm, cells, member, reg)
    quad = np.asarray(DCS_QUAD_EDGES, np.int64)
    return verts.reshape(-1, 3), _dc_faces(E, verts, lambda k, cell, axis: base[cell] + loops[case[cell], quad[axis, k]])


def dual_contour_batch(sdf: torch.Tensor, sdf_params, res: int, iso: float = 0.0, normals_fn=None,
                       reg: float = DC_REG, ws: Optional[torch.Tensor] = None, max_edge_slots: int = MC_EDGE_SLOTS,
                       hermite: bool = False, sheets: bool = False) -> List[Tuple[torch.Tensor, ...]]:
    """sdf: float32 device tensor [B,(res+1)^3], sdf_params [B,6] -> B x (verts [nv,3] float32, faces [nf,3] int32),
    views of two device tensors; every pair is bit for bit ``dual_contour_arrays`` of that grid with its normals.
    One count call, ONE device-to-host copy of the [B,3] sizes {ne, nv, nf}, one points call and one emit call for the
    whole batch (a batch whose 3*B*(res+1)^3 edge slots reach ``max_edge_slots`` is meshed in several such rounds).
    ``normals_fn(b, points_b)`` -> float32 [ne_b,3] on the device: the field's gradient at grid b's Hermite points
    (any length; a NaN, infinite or zero row only counts in its cells' means); None: the grid's own finite
    differences (``grid_normals_arrays``, one more call).  ``reg``: see ``dual_contour_arrays`` (the default is
    unmeasured on a trained network).  ``hermite``: every item is (verts, faces, points, normals).
    The mesh can be non-manifold where a cell holds more than one sheet of the surface (``sheets`` splits such cells);
    triangles may be degenerate in position, never in index; the winding is ``marching_cubes``' (geometric normal along
    +grad).
    ``sheets``: one vertex per sheet of a cell instead (include/dc/disn_amd_dc_sheets.h): every pair is bit for bit
    ``dual_contour_sheets_arrays`` of that grid, nv the grid's loops; the same points, normals, ne and nf.  A round then
    also keeps 4*B*res^3 below 2^32.  Its remaining limit is stated there."""
    reg = float(reg)
    if not (0.0 < reg <= 1.0):
        raise ValueError("reg must be in (0, 1], got %r" % (reg,))
    sdf, sp, per = _batch_args(sdf, sdf_params, res, max_edge_slots)
    h = lib()
    fam = "disn_dcs_" if sheets else "disn_dc_"
    ws_bytes, count_batch, points_batch, grid_normals_batch, emit_batch = (
        getattr(h, fam + k) for k in ("workspace_bytes", "count_batch", "points_batch", "grid_normals_batch", "emit_batch"))
    if sheets:
        per = min(per, (MC_EDGE_SLOTS - 1) // max(4 * res ** 3, 1))             # the loop ranks: 4*B*res^3 < 2^32
    dev = sdf.device

    def count(part, nb, counts, ws, st):
        check(fam + "count_batch", count_batch(part.data_ptr(), nb, res, float(iso), counts.data_ptr(), ws.data_ptr(),
                                               ws.numel(), st))

    def emit(b0, part, boxes, nb, sizes, ws, st):
        ne, nv, nf = (int(sizes[:, k].sum()) for k in range(3))
        points = torch.empty((ne, 3), dtype=torch.float32, device=dev)
        verts = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((nf, 3), dtype=torch.int32, device=dev)
        e_off = np.concatenate([[0], np.cumsum(sizes[:, 0])]).astype(np.int64)
        normals = points
        if ne:
            check(fam + "points_batch", points_batch(part.data_ptr(), boxes.ctypes.data, nb, res, float(iso),
                                                     points.data_ptr(), ws.data_ptr(), ws.numel(), st))
            if normals_fn is None:
                normals = torch.empty((ne, 3), dtype=torch.float32, device=dev)
                check(fam + "grid_normals_batch", grid_normals_batch(
                    part.data_ptr(), boxes.ctypes.data, nb, res, float(iso), normals.data_ptr(), ws.data_ptr(),
                    ws.numel(), st))
            else:
                rows = []
                for k in range(nb):
                    pk = points[e_off[k]:e_off[k + 1]]
                    nk = normals_fn(b0 + k, pk) if len(pk) else pk
                    if nk.shape != pk.shape or nk.dtype != torch.float32 or nk.device != pk.device:
                        raise ValueError("normals_fn must return float32 %s on %s for grid %d, got %s %s" % (
                            tuple(pk.shape), dev, b0 + k, nk.dtype, tuple(nk.shape)))
                    rows.append(nk)
                normals = rows[0].contiguous() if nb == 1 else torch.cat(rows)
            # a batch without a quad still has its vertices: the entry takes no NULL, so faces gets one spare row
            fbuf = faces if nf else torch.empty((1, 3), dtype=torch.int32, device=dev)
            check(fam + "emit_batch", emit_batch(part.data_ptr(), boxes.ctypes.data, nb, res, float(iso),
                                                 points.data_ptr(), normals.data_ptr(), reg, verts.data_ptr(),
                                                 fbuf.data_ptr(), ws.data_ptr(), ws.numel(), st))
        return ((verts, 1), (faces, 2)) + (((points, 0), (normals, 0)) if hermite else ())

    return _batch_rounds(sdf, sp, res, per, ws, ws_bytes, 3, count, emit)


def dual_contour(sdf: torch.Tensor, sdf_params, res: int, iso: float = 0.0, normals_fn=None, reg: float = DC_REG,
                 ws: Optional[torch.Tensor] = None, sheets: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """``dual_contour_batch`` for one grid of (res+1)^3 values; ``normals_fn(points)`` -> [ne,3] on the device, or
    None for the grid normals; ``sheets``: one vertex per sheet of a cell.  -> (verts [nv,3] float32, faces [nf,3]
    int32), on the device."""
    fn = None if normals_fn is None else (lambda b, pts: normals_fn(pts))
    return dual_contour_batch(sdf.reshape(1, -1), np.asarray(sdf_params, np.float64).reshape(1, 6), res, iso, fn, reg,
                              ws, sheets=sheets)[0][:2]

"""Signed distance grids of triangle meshes on the device: the ``isosurface/computeDistanceField <obj> 256 256 256
-s -e 1.2 -m 1 [-g g]`` step of the reference's ``preprocessing/create_point_sdf_grid.py`` (a closed Vega-FEM
binary), restated for the MI355X.  Kernels: ``csrc/mesh_sdf.hip``; host parts (OBJ reader, BVH build):
``csrc/mesh_host.cpp``; the rule is in DESIGN §4p.

    verts, faces = mesh_sdf.read_obj_mesh("model.obj")
    sdf, sdf_params = mesh_sdf.sdf_grid(verts, faces, 256)       # (257^3,) device tensor in the .dist order

The sign needs no face orientation: the outside is what a flood from the box boundary reaches without crossing a
triangle, so open containers are outside inside and polygon soups need no repair.  Not Vega's exact offset
surface: near holes narrower than ~2 tau (tau = seal * largest grid spacing) the two may differ.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from ._lib import check, lib


def read_obj_mesh(path: str) -> Tuple[np.ndarray, np.ndarray]:
    """-> (verts float32 [nv, 3], faces int32 [nf, 3], 0-based): every "v" record and every "f" record (v, v/vt,
    v//vn, v/vt/vn tokens, negative indices relative to the vertices read so far), polygons fan-triangulated in
    file order; all other records are skipped.  Raises OSError on an I/O or parse error or a bad index."""
    h = lib()
    counts = (C.c_int64 * 2)()
    rc = h.disn_read_obj_mesh(path.encode(), None, 0, None, 0, counts)
    if rc != 0:
        raise OSError("cannot read mesh %s (status %d)" % (path, rc))
    nv, nf = int(counts[0]), int(counts[1])
    v = np.empty((nv, 3), np.float32)
    f = np.empty((nf, 3), np.int32)
    rc = h.disn_read_obj_mesh(path.encode(), v.ctypes.data if nv else None, nv, f.ctypes.data if nf else None, nf,
                              counts)
    if rc != 0 or (int(counts[0]), int(counts[1])) != (nv, nf):
        raise OSError("%s changed while it was read" % path)
    return v, f


def _mesh_arrays(verts, faces) -> Tuple[np.ndarray, np.ndarray]:
    v = verts.detach().cpu().numpy() if isinstance(verts, torch.Tensor) else verts
    f = faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else faces
    v = np.ascontiguousarray(v, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(f, np.int32).reshape(-1, 3)
    if f.shape[0] == 0 or v.shape[0] == 0:
        raise ValueError("the mesh has no triangles")
    return v, f


def build_bvh_host_order(verts, faces) -> Tuple[np.ndarray, np.ndarray]:
    """-> (image, order): the BVH image (uint8, private layout: csrc/mesh_bvh.hpp) of a triangle soup, built on
    the host, and order int32 [nf], the face stored in each triangle slot of the image (the image keeps the
    triangles in leaf order); deterministic: the same mesh gives the same bytes"""
    v, f = _mesh_arrays(verts, faces)
    h = lib()
    nbytes = h.disn_mesh_bvh_bytes(f.shape[0])
    if nbytes == 0:
        raise ValueError("unsupported triangle count %d" % f.shape[0])
    out = np.empty(nbytes, np.uint8)
    order = np.empty(f.shape[0], np.int32)
    rc = h.disn_mesh_bvh_build_order(v.ctypes.data, v.shape[0], f.ctypes.data, f.shape[0], out.ctypes.data, nbytes,
                                     order.ctypes.data)
    if rc == -1:
        raise ValueError("face index out of range (mesh of %d vertices)" % v.shape[0])
    check("disn_mesh_bvh_build_order", rc)
    return out, order


def build_bvh_host(verts, faces) -> np.ndarray:
    """the BVH image alone (``build_bvh_host_order``)"""
    return build_bvh_host_order(verts, faces)[0]


class MeshBvh:
    """a triangle soup's BVH on the device (built once, reused by every distance and sign call)"""

    def __init__(self, verts, faces, device=None):
        v, f = _mesh_arrays(verts, faces)
        self.nf = int(f.shape[0])
        self.host, self.order_host = build_bvh_host_order(v, f)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.image = torch.from_numpy(self.host).to(self.device)
        self._order = None

    @property
    def order(self) -> torch.Tensor:
        """the slot -> face map on the device (uploaded on first use: only the renderer reads it)"""
        if self._order is None:
            self._order = torch.from_numpy(self.order_host).to(self.device)
        return self._order


def _bvh(mesh, faces=None) -> MeshBvh:
    if isinstance(mesh, MeshBvh):
        return mesh
    if faces is None:
        raise ValueError("faces are required with a vertex array")
    return MeshBvh(mesh, faces)


def unsigned_distance(verts, faces, points, brute: bool = False) -> torch.Tensor:
    """-> [n] float32 device tensor: min over triangles of |p - T| for the points [n, 3] (a device tensor).
    ``verts`` may be a ``MeshBvh`` (then ``faces`` is ignored).  ``brute``: test every triangle (the reference
    form the BVH result equals bit for bit)."""
    m = _bvh(verts, faces)
    pts = ops._chk(points.reshape(-1, 3), "points")
    n = pts.shape[0]
    with torch.cuda.device(pts.device):
        out = torch.empty(n, dtype=torch.float32, device=pts.device)
        if n:
            check("disn_mesh_udf_points", lib().disn_mesh_udf_points(m.image.data_ptr(), m.nf, pts.data_ptr(), n,
                                                                     int(brute), out.data_ptr(), ops._stream()))
    return out


def grid_axes(sdf_params: Sequence[float], res: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """the node coordinates per axis: np.linspace(float64(lo), float64(hi), res+1).astype(float32), i.e. what
    ``sample_sdf`` reports and ``create_sdf.grid_points_host`` builds for the same params"""
    p = np.asarray(sdf_params, np.float32).astype(np.float64)
    return tuple(np.linspace(p[a], p[a + 3], num=res + 1).astype(np.float32) for a in range(3))


def default_bbox(verts, expand: float = 1.2) -> np.ndarray:
    """the mesh AABB scaled by ``expand`` about its centre, per axis (computeDistanceField -e), float64 [6]"""
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    c, half = (lo + hi) * 0.5, (hi - lo) * 0.5 * float(expand)
    return np.concatenate([c - half, c + half])


def seal_params(axes, seal: float = 1.0) -> Tuple[float, int]:
    """(tau, steps): tau = float32(seal * h_max), steps = 2 * ceil(tau / h_min) + 1, h = (hi - lo) / (n - 1) per axis
    in float64"""
    if not seal > 0.5:
        raise ValueError("seal must be > 0.5 (got %r): far nodes must not straddle a triangle" % seal)
    h = [(float(a[-1]) - float(a[0])) / (len(a) - 1) for a in axes]
    if min(h) <= 0:
        raise ValueError("degenerate grid box")
    tau = float(np.float32(seal * max(h)))
    return tau, 2 * int(math.ceil(tau / min(h))) + 1


def _axes_dev(axes, device):
    return [torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device) for a in axes]


def unsigned_distance_grid(mesh, faces, axes, brute: bool = False) -> torch.Tensor:
    """-> [nz*ny*nx] float32 device tensor at the nodes (axes[0][ix], axes[1][iy], axes[2][iz]), x fastest"""
    m = _bvh(mesh, faces)
    xs, ys, zs = _axes_dev(axes, m.device)
    nx, ny, nz = xs.numel(), ys.numel(), zs.numel()
    with torch.cuda.device(m.device):
        u = torch.empty(nx * ny * nz, dtype=torch.float32, device=m.device)
        check("disn_mesh_udf_grid", lib().disn_mesh_udf_grid(m.image.data_ptr(), m.nf, xs.data_ptr(), ys.data_ptr(),
                                                             zs.data_ptr(), nx, ny, nz, int(brute), u.data_ptr(),
                                                             ops._stream()))
    return u


def sign_grid(mesh, faces, axes, u: torch.Tensor, tau: float, steps: int, offset: float = 0.0
              ) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (sdf [N] float32, outside [N] uint8) on the device from the unsigned grid ``u``"""
    m = _bvh(mesh, faces)
    xs, ys, zs = _axes_dev(axes, m.device)
    nx, ny, nz = xs.numel(), ys.numel(), zs.numel()
    u = ops._chk(u.reshape(-1), "u")
    if u.numel() != nx * ny * nz:
        raise ValueError("u must hold %d values, got %d" % (nx * ny * nz, u.numel()))
    h = lib()
    with torch.cuda.device(m.device):
        sdf = torch.empty_like(u)
        outside = torch.empty(u.numel(), dtype=torch.uint8, device=m.device)
        ws = ops._ws(h.disn_mesh_sign_workspace_bytes(nx, ny, nz), m.device)
        check("disn_mesh_sign", h.disn_mesh_sign(m.image.data_ptr(), m.nf, xs.data_ptr(), ys.data_ptr(),
                                                 zs.data_ptr(), nx, ny, nz, u.data_ptr(), float(tau), int(steps),
                                                 float(offset), sdf.data_ptr(), outside.data_ptr(), ws.data_ptr(),
                                                 ws.numel(), ops._stream()))
    return sdf, outside


def sdf_grid(verts, faces, res: int, bbox: Optional[Sequence[float]] = None, expand: float = 1.2,
             seal: float = 1.0, offset: float = 0.0) -> Tuple[torch.Tensor, np.ndarray]:
    """-> (sdf, sdf_params): the signed distance at the (res+1)^3 nodes of ``bbox`` (default: the mesh AABB scaled
    by ``expand``) as a float32 device tensor in the .dist order, and sdf_params = float32(bbox) [6].
    ``offset`` is subtracted from every value (the reference's -g: thickens open sheets)."""
    v, f = _mesh_arrays(verts, faces)
    if res < 1:
        raise ValueError("res must be >= 1")
    params = np.asarray(default_bbox(v, expand) if bbox is None else bbox, np.float64).astype(np.float32)
    axes = grid_axes(params, res)
    tau, steps = seal_params(axes, seal)
    m = MeshBvh(v, f)
    u = unsigned_distance_grid(m, None, axes)
    sdf, _ = sign_grid(m, None, axes, u, tau, steps, offset)
    return sdf, params

"""Voxel IoU of triangle meshes on the device: what the reference's ``test/test_iou.py`` asks PyMesh for
(``pymesh.VoxelGrid(2./dim)``, ``insert_mesh``, ``create_grid``, then its corner -> index arithmetic), restated for
the MI355X.  Kernels: ``csrc/voxel.hip``; the definitions are in DESIGN §4r.  Parity with PyMesh itself is
unpinned (PyMesh runs on none of the machines this was built on): cell alignment and the closed-box overlap are
restated from reading, and ``tests/voxel_reference.py`` is the contract the tests enforce.

    gt = mesh_sdf.read_obj_mesh("isosurf.obj")
    iou, inter, union = voxel.iou_views(gt, [(verts, faces), "pred_00.obj", ...])      # the reference's number
    iou, inter, union = voxel.iou_views(gt, preds, mode="solid")                        # occupancy IoU

Voxel key k (per axis) is the closed box of centre k*h and half side h/2, h = float32(2/dim).  ``surface_voxels``
marks every key a triangle overlaps; ``fill`` adds what the outside cannot reach; ``index_grid`` is the
reference's dim^3 array: every occupied voxel's eight corners c set cell int((c + 1.1) / 2.4 * dim).
A mesh that leaves the key range (``key_range``) raises ValueError: nothing is clamped or wrapped.
"""
from __future__ import annotations

import functools
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import ops
from ._lib import check, lib

Mesh = Union[str, Tuple[object, object]]
MODES = ("reference", "solid")


@functools.lru_cache(maxsize=None)
def corner_lut(dim: int) -> Tuple[int, np.ndarray]:
    """-> (kmin, lut): lut[j] is the reference's index of corner number kmin + j, whose coordinate is
    (kmin + j - 0.5) * (2.0 / dim): the low face of key kmin + j and the high face of key kmin + j - 1.  Formed in
    float64 with the reference's expression, ``((c + 1.1) / 2.4 * dim).astype(int)``; the corners kept are the
    contiguous run on which 0 <= (c + 1.1) / 2.4 * dim < dim, so keys kmin .. kmin + len(lut) - 2 have both."""
    if not 1 <= int(dim) <= 512:
        raise ValueError("dim must be in 1..512 (got %r)" % (dim,))
    dim = int(dim)
    n = np.arange(-2 * dim - 2, 2 * dim + 3, dtype=np.int64)
    c = (n.astype(np.float64) - 0.5) * (2.0 / dim)
    val = (c + 1.1) / 2.4 * dim
    ok = (val >= 0) & (val < dim)
    good = np.nonzero(ok)[0]
    assert good.size >= 2 and good[-1] - good[0] + 1 == good.size
    lut = val[good].astype(int).astype(np.int32)
    return int(n[good[0]]), lut


def key_range(dim: int) -> Tuple[int, int]:
    """-> (kmin, nkeys): the keys whose eight corners all map into the reference's dim^3 array"""
    kmin, lut = corner_lut(dim)
    return kmin, int(lut.size) - 1


class VoxelBits:
    """an n^3 bit grid on the device: ``words`` int32 [n*n*ceil(n/32)], cell (x, y, z) = bit (x & 31) of word
    (z*n + y)*ceil(n/32) + (x >> 5).  kind "key": x = kx - kmin (``surface_voxels``, ``fill``); kind "index": the
    reference's array (``index_grid``)."""

    def __init__(self, words: torch.Tensor, n: int, kind: str, dim: int, kmin: int = 0):
        self.words, self.n, self.kind, self.dim, self.kmin = words, int(n), kind, int(dim), int(kmin)

    @property
    def wpr(self) -> int:
        return (self.n + 31) // 32

    def count(self) -> int:
        return int(to_dense(self).sum())


def _device(*xs) -> torch.device:
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    return torch.device("cuda", torch.cuda.current_device())


def _mesh_dev(mesh: Mesh, device) -> Tuple[torch.Tensor, torch.Tensor]:
    if isinstance(mesh, str):
        from . import mesh_sdf
        mesh = mesh_sdf.read_obj_mesh(mesh)
    verts, faces = mesh
    v = verts if isinstance(verts, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(verts, np.float32))
    f = faces if isinstance(faces, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(faces, np.int32))
    v = v.to(device=device, dtype=torch.float32).reshape(-1, 3).contiguous()
    f = f.to(device=device, dtype=torch.int32).reshape(-1, 3).contiguous()
    return v, f


def _surface_async(mesh: Mesh, dim: int, device, flags: torch.Tensor) -> VoxelBits:
    """launch only: ``flags`` (int32 [1], the caller's) is OR-ed on the device and read by the caller later"""
    kmin, nkeys = key_range(dim)
    v, f = _mesh_dev(mesh, device)
    h = lib()
    nv, nf = v.shape[0], f.shape[0]
    with torch.cuda.device(device):
        words = torch.empty(h.disn_voxel_grid_words(nkeys), dtype=torch.int32, device=device)
        ws = ops._ws(h.disn_voxel_surface_workspace_bytes(nf), device)
        check("disn_voxel_surface", h.disn_voxel_surface(v.data_ptr() if nv else None, nv, f.data_ptr() if nf else None,
                                                         nf, dim, kmin, nkeys, words.data_ptr(), flags.data_ptr(),
                                                         ws.data_ptr(), ws.numel(), ops._stream()))
    return VoxelBits(words, nkeys, "key", dim, kmin)


def _raise_flags(flag: int, name: str, dim: int) -> None:
    if flag & 2:
        raise ValueError("%s: a face index is outside the vertex array" % name)
    if flag & 1:
        kmin, nkeys = key_range(dim)
        raise ValueError("%s reaches outside the voxel key range %d..%d of dim %d (coordinates beyond about [%.3f, %.3f]"
                         " or not finite): the reference's index arithmetic has no cell for it"
                         % (name, kmin, kmin + nkeys - 1, dim, (kmin - 0.5) * 2.0 / dim, (kmin + nkeys - 0.5) * 2.0 / dim))


def surface_voxels(verts, faces, dim: int = 110, name: str = "the mesh") -> VoxelBits:
    """the key grid of the voxels that the triangles (verts [nv,3], faces [nf,3]; numpy or device tensors) overlap.
    An empty face list gives an empty grid.  ValueError (naming ``name``) if the mesh leaves the key range."""
    device = _device(verts, faces)
    flags = torch.zeros(1, dtype=torch.int32, device=device)
    vox = _surface_async((verts, faces), dim, device, flags)
    _raise_flags(int(flags.item()), name, dim)
    return vox


def fill(vox: VoxelBits) -> VoxelBits:
    """surface voxels plus every voxel that the outside of the key range cannot reach through unoccupied voxels by
    6-connectivity (scipy.ndimage.binary_fill_holes of the key grid)"""
    if vox.kind != "key":
        raise ValueError("fill works on a key grid (surface_voxels), not on an index grid")
    h = lib()
    device = vox.words.device
    with torch.cuda.device(device):
        out = torch.empty_like(vox.words)
        ws = ops._ws(h.disn_voxel_fill_workspace_bytes(vox.n), device)
        check("disn_voxel_fill", h.disn_voxel_fill(vox.words.data_ptr(), vox.n, out.data_ptr(), ws.data_ptr(),
                                                   ws.numel(), ops._stream()))
    return VoxelBits(out, vox.n, "key", vox.dim, vox.kmin)


@functools.lru_cache(maxsize=8)
def _lut_dev(dim: int, device_index: int) -> torch.Tensor:
    return torch.from_numpy(corner_lut(dim)[1]).to(torch.device("cuda", device_index))


def index_grid(vox: VoxelBits) -> VoxelBits:
    """the reference's dim^3 array of a key grid: the eight corners of every occupied voxel through ``corner_lut``"""
    if vox.kind != "key":
        raise ValueError("index_grid works on a key grid")
    h = lib()
    device = vox.words.device
    lut = _lut_dev(vox.dim, device.index if device.index is not None else torch.cuda.current_device())
    if lut.numel() != vox.n + 1:
        raise ValueError("the key grid does not belong to dim %d" % vox.dim)
    with torch.cuda.device(device):
        out = torch.empty(h.disn_voxel_grid_words(vox.dim), dtype=torch.int32, device=device)
        check("disn_voxel_index_grid", h.disn_voxel_index_grid(vox.words.data_ptr(), vox.n, lut.data_ptr(), vox.dim,
                                                               out.data_ptr(), ops._stream()))
    return VoxelBits(out, vox.dim, "index", vox.dim)


def to_dense(bits: VoxelBits) -> np.ndarray:
    """-> bool [n, n, n] indexed [x, y, z] (n = dim for an index grid, the key count for a key grid), on the host"""
    n, wpr = bits.n, bits.wpr
    w = bits.words.detach().cpu().numpy().view(np.uint32).reshape(n, n, wpr)          # [z, y, xw]
    b = np.unpackbits(w.view(np.uint8), axis=-1, bitorder="little").reshape(n, n, wpr * 32)[:, :, :n]
    return np.ascontiguousarray(b.transpose(2, 1, 0)).astype(bool)


def _grid_for(vox: VoxelBits, mode: str) -> VoxelBits:
    return index_grid(vox) if mode == "reference" else fill(vox)


def iou_views(gt: Mesh, preds: Sequence[Mesh], dim: int = 110, mode: str = "reference",
              names: Optional[Sequence[str]] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """-> (iou float64 [V], inter int64 [V], union int64 [V]) of V predicted meshes against one ground truth.
    A mesh is (verts, faces) as numpy arrays or device tensors, or the path of a Wavefront .obj.
    mode "reference": the reference's shell IoU on its index grid; "solid": filled voxels, counted on the key grid.
    ``names`` (ground truth first, then the predictions) are what error messages call the meshes.
    All 1 + V meshes are voxelised without a host synchronisation between them; iou = float(inter) / union on the
    host in float64.  ValueError if a mesh leaves the key range or a union is empty."""
    if mode not in MODES:
        raise ValueError("mode must be one of %s (got %r)" % (", ".join(MODES), mode))
    preds = list(preds)
    if not preds:
        raise ValueError("no prediction to score")
    meshes: List[Mesh] = [gt] + preds
    if names is None:
        names = [m if isinstance(m, str) else ("the ground truth" if i == 0 else "prediction %d" % (i - 1))
                 for i, m in enumerate(meshes)]
    if len(names) != len(meshes):
        raise ValueError("names must list the ground truth and every prediction")
    device = _device(*[x for m in meshes if not isinstance(m, str) for x in m])
    V = len(preds)
    h = lib()
    with torch.cuda.device(device):
        flags = torch.zeros(len(meshes), dtype=torch.int32, device=device)
        vox = [_surface_async(m, dim, device, flags[i:i + 1]) for i, m in enumerate(meshes)]
        if mode == "solid":            # the fill reads a convergence flag: check the meshes first
            for i, fl in enumerate(flags.cpu().tolist()):
                _raise_flags(fl, names[i], dim)
        grids = [_grid_for(v, mode) for v in vox]
        words = grids[0].words.numel()
        stack = torch.stack([g.words for g in grids[1:]])
        counts = torch.empty(2, V, dtype=torch.int64, device=device)
        check("disn_voxel_iou", h.disn_voxel_iou(grids[0].words.data_ptr(), stack.data_ptr(), V, words,
                                                 counts[0].data_ptr(), counts[1].data_ptr(), ops._stream()))
        if mode != "solid":
            for i, fl in enumerate(flags.cpu().tolist()):
                _raise_flags(fl, names[i], dim)
        inter, union = counts.cpu().numpy()
    iou = np.empty(V, np.float64)
    for v in range(V):
        if union[v] == 0:
            raise ValueError("%s and %s occupy no voxel: the IoU is undefined" % (names[1 + v], names[0]))
        iou[v] = float(inter[v]) / union[v]
    return iou, inter.copy(), union.copy()

"""Times of voxel IoU (csrc/voxel.hip, disn_amd/voxel.py) on the GPU.

    python tools/voxel_time.py [--out FILE] [--quick]

Rows: the triangle pass for a ~50 k-triangle marching-cubes mesh and for a 12-triangle box spanning the grid, the
fill, the corner map, the 24-view count (device events around back-to-back calls after a warm-up, median of the
rounds), and one object (1 + 24 meshes) end to end from .obj files (wall clock, ended by the device-to-host copy of
the counts).  There is no runnable reference to time against (PyMesh): the expectation is that everything but the
triangle pass and the file reads is launch-bound, and that the box is not slower than the 50 k-triangle mesh.
--quick: one call of each (a workload for a rocprofv3 pass).
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from disn_amd import isosurface, mesh_sdf, voxel  # noqa: E402

BOX = [-1, -1, -1, 1, 1, 1]


def sphere_mesh(res, r, c=(0.0, 0.0, 0.0)):
    ax = np.linspace(-1, 1, res + 1)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    sdf = (np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r).astype(np.float32)
    return isosurface.marching_cubes(torch.from_numpy(sdf).cuda(), BOX, res)


def box_mesh(a):
    v = np.array([[x, y, z] for z in (-a, a) for y in (-a, a) for x in (-a, a)], np.float32)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 7, 5], [4, 6, 7], [0, 5, 1], [0, 4, 5], [2, 3, 7], [2, 7, 6],
                  [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)
    return torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()


def timed(fn, warmup, iters, rounds):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e) / iters * 1e3)          # us per call
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--dim", type=int, default=110)
    a = ap.parse_args()
    w, it, rounds = (0, 1, 1) if a.quick else (3, 20, 7)
    dim = a.dim
    kmin, nkeys = voxel.key_range(dim)
    lines = ["voxel IoU timings, MI355X, dim %d (key grid %d^3 = %d KB of bits, index grid %d KB); us per call, "
             "median (min .. max) of %d rounds of %d calls"
             % (dim, nkeys, 4 * voxel.lib().disn_voxel_grid_words(nkeys) // 1024,
                4 * voxel.lib().disn_voxel_grid_words(dim) // 1024, rounds, it)]
    mc = sphere_mesh(112, 0.62)
    box = box_mesh(0.98)
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    rows = {}
    for name, m in (("marching-cubes sphere", mc), ("box spanning the grid", box)):
        vox = voxel.surface_voxels(*m, dim)
        t = timed(lambda: voxel._surface_async(m, dim, m[0].device, flags), w, it, rounds)
        rows[name] = t[0]
        lines.append("triangle pass, %s (%d triangles, %d surface voxels): %.1f (%.1f .. %.1f)"
                     % (name, m[1].shape[0], vox.count(), *t))
    assert int(flags.item()) == 0
    vox = voxel.surface_voxels(*mc, dim)
    t = timed(lambda: voxel.fill(vox), w, max(1, it // 4), rounds)
    lines.append("fill of the sphere's shell (%d solid voxels; host reads a flag every 8 sweeps): %.1f (%.1f .. %.1f)"
                 % (voxel.fill(vox).count(), *t))
    t = timed(lambda: voxel.index_grid(vox), w, it, rounds)
    lines.append("corner map (key grid -> index grid): %.1f (%.1f .. %.1f)" % t)
    grids = [voxel.index_grid(voxel.surface_voxels(*sphere_mesh(64, 0.6 + 0.002 * i), dim)) for i in range(25)]
    stack = torch.stack([g.words for g in grids[1:]])
    counts = torch.empty(2, 24, dtype=torch.int64, device="cuda")
    h = voxel.lib()

    def count():
        voxel.check("disn_voxel_iou", h.disn_voxel_iou(grids[0].words.data_ptr(), stack.data_ptr(), 24, stack.shape[1],
                                                       counts[0].data_ptr(), counts[1].data_ptr(),
                                                       torch.cuda.current_stream().cuda_stream))
    t = timed(count, w, it, rounds)
    lines.append("24-view intersection / union count (one launch): %.1f (%.1f .. %.1f)" % t)
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for i in range(25):
            v, f = sphere_mesh(64, 0.6 + 0.002 * i, (0.002 * i, 0.0, 0.0))
            paths.append(os.path.join(d, "m%02d.obj" % i))
            isosurface.write_obj(paths[-1], v, f)
        nf = mesh_sdf.read_obj_mesh(paths[0])[1].shape[0]
        for mode in voxel.MODES:
            voxel.iou_views(paths[0], paths[1:], dim, mode)                      # warm-up
            ts = []
            for _ in range(1 if a.quick else 5):
                t0 = time.perf_counter()
                voxel.iou_views(paths[0], paths[1:], dim, mode)
                ts.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            for p in paths:
                mesh_sdf.read_obj_mesh(p)
            t_read = (time.perf_counter() - t0) * 1e3
            lines.append("one object end to end, mode %s (25 .obj files of ~%d triangles -> 24 IoU values): %.1f ms "
                         "median (%.1f .. %.1f), of which reading the files %.1f ms"
                         % (mode, nf, statistics.median(ts), min(ts), max(ts), t_read))
    lines.append("load balance: the box's triangle pass takes %.2f x the marching-cubes mesh's"
                 % (rows["box spanning the grid"] / rows["marching-cubes sphere"]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(text + "\n")


if __name__ == "__main__":
    main()

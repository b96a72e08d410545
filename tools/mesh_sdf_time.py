"""Times of mesh-to-SDF preprocessing (csrc/mesh_sdf.hip, disn_amd/preprocess.py) on the GPU, next to the goals.

    python tools/mesh_sdf_time.py [--out FILE] [--quick]

Mesh: a torus of 50 k triangles (and one of 200 k), normalised into the unit ball; grid 257^3 over the AABB x 1.2.
Rows: host BVH build, the unsigned field (device events around back-to-back calls after a warm-up), the sign pass,
and one object end to end (OBJ file -> ori_sample.npz + isosurf.obj, wall clock).  --quick: one call of each
(a workload for a rocprofv3 pass).
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from disn_amd import isosurface, mesh_sdf, preprocess  # noqa: E402

LANE_OPS = 256 * 4 * 16 * 2.4e9           # fp32 lane-ops/s: 256 CU x 4 SIMD x 16 lanes/clk x 2.4 GHz


def torus(nu, nv, R=0.6, r=0.25):
    us, vs = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing="ij")
    v = np.stack([(R + r * np.cos(vs)) * np.cos(us), (R + r * np.cos(vs)) * np.sin(us), r * np.sin(vs)], -1)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    a, b = i * nv + j, ((i + 1) % nu) * nv + j
    c, d = ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
    f = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return v.reshape(-1, 3).astype(np.float32), f.astype(np.int32)


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters                # ms per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    w, it = (0, 1) if a.quick else (1, 5)
    res = 256
    lines = ["mesh_sdf timings, MI355X, grid %d^3 (res %d)" % (res + 1, res)]
    for nu, nv in ((256, 98), (512, 196)):
        v, f = torus(nu, nv)
        t0 = time.perf_counter()
        m = mesh_sdf.MeshBvh(v, f)
        torch.cuda.synchronize()
        t_bvh = (time.perf_counter() - t0) * 1e3
        params = mesh_sdf.default_bbox(v, 1.2).astype(np.float32)
        axes = mesh_sdf.grid_axes(params, res)
        tau, steps = mesh_sdf.seal_params(axes, 1.0)
        u = mesh_sdf.unsigned_distance_grid(m, None, axes)
        t_u = timed(lambda: mesh_sdf.unsigned_distance_grid(m, None, axes), w, it)
        t_s = timed(lambda: mesh_sdf.sign_grid(m, None, axes, u, tau, steps), w, it)
        floor = (res + 1) ** 3 * 64 * 45 / LANE_OPS * 1e3
        lines.append("%d triangles: BVH build (host) %.1f ms; unsigned field %.2f ms (goal <= 50 ms at 50 k, VALU "
                     "floor ~%.1f ms); sign pass (%d band steps) %.2f ms (goal <= 20 ms)"
                     % (len(f), t_bvh, t_u, floor, steps, t_s))
    v, f = torus(256, 98)
    with tempfile.TemporaryDirectory() as d:
        isosurface.write_obj(os.path.join(d, "mesh", "c", "o", "model.obj"), v, f)
        args = (os.path.join(d, "mesh", "c"), os.path.join(d, "norm", "c"), os.path.join(d, "sdf", "c"))
        kw = dict(res=res, iso_val=0.003, expand_rate=1.2, ish5=True, normalize=True, num_sample=32768,
                  bandwidth=0.1, max_verts=16384, cat_id="c", g=0.0, version=1, skip_all_exist=False)
        preprocess.create_sdf_obj(*args, "o", indx=0, **kw)            # warm-up (and the library load)
        os.remove(os.path.join(d, "sdf", "c", "o", "ori_sample.npz"))
        t0 = time.perf_counter()
        preprocess.create_sdf_obj(*args, "o", indx=1, **kw)
        torch.cuda.synchronize()
        t_e2e = time.perf_counter() - t0
    lines.append("one object end to end (%d triangles, OBJ -> ori_sample.npz + isosurf.obj): %.3f s (goal <= 1 s)"
                 % (len(f), t_e2e))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(text + "\n")


if __name__ == "__main__":
    main()

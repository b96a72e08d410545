"""Times of view rendering (csrc/render.hip, disn_amd/create_img_h5.py --render) on the GPU.

    python tools/render_time.py [--out FILE]

Mesh: icosphere(6), 81 920 triangles, radius 0.7; 24 views of 137 x 137 from render.random_view_params(seed 0).
Rows: host BVH build + upload, one launch of disn_render_views at S = 4 and S = 1 (device events around single
launches after a warm-up), the brute-force launch (once; S = 4 only when S = 1 predicts under 20 s) with the equality
of its image, and the objects/s of the --render driver on 8 objects of that mesh (OBJ read, BVH, launch, read-back,
PNG encoding on 8 writer threads, view files; wall clock).  Prints one JSON object, and writes it to --out.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_sdf_reference as R  # noqa: E402
from disn_amd import create_img_h5, data_sdf, isosurface, mesh_sdf, render  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
args = ap.parse_args()

out = {}
v, f = R.icosphere(6, 0.7)
out["triangles"] = int(len(f))
t0 = time.perf_counter(); m = mesh_sdf.MeshBvh(v, f); out["bvh_build_upload_s"] = time.perf_counter() - t0
params = render.random_view_params(np.random.default_rng(0), 24)

def timed(S, brute, reps):
    for _ in range(2 if not brute else 0):
        render.render_views(m, None, params, samples=S, brute=brute)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); r = render.render_views(m, None, params, samples=S, brute=brute); b.record()
        torch.cuda.synchronize(); ts.append(a.elapsed_time(b))
    return ts, r

ts, r4 = timed(4, False, 30)
out["bvh_S4_ms"] = {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts)), "reps": len(ts)}
ts, r1 = timed(1, False, 30)
out["bvh_S1_ms"] = {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts)), "reps": len(ts)}
print(json.dumps(out), flush=True)
ts, b1 = timed(1, True, 1)
out["brute_S1_ms"] = ts[0]
out["S1_equal"] = bool(torch.equal(r1["rgba"], b1["rgba"]))
print(json.dumps(out), flush=True)
if ts[0] * 16 < 20000:
    ts, b4 = timed(4, True, 1)
    out["brute_S4_ms"] = ts[0]
    out["S4_equal"] = bool(torch.equal(r4["rgba"], b4["rgba"]))
hitfrac = float((r4["rgba"][..., 3] > 0).float().mean())
out["hit_fraction"] = hitfrac
print(json.dumps(out), flush=True)

# objects/s of --render: 8 objects of that mesh, samples preset (preprocess is not part of this step)
N = 8
with tempfile.TemporaryDirectory() as tmp:
    cat = "03001627"
    dirs = {k: os.path.join(tmp, k) for k in ("mesh_dir", "norm_mesh_dir", "sdf_dir", "rendered_dir", "renderedh5_dir")}
    os.makedirs(os.path.join(tmp, "lst"))
    names = ["obj%d" % i for i in range(N)]
    for n in names:
        os.makedirs(os.path.join(dirs["mesh_dir"], cat, n))
        isosurface.write_obj(os.path.join(dirs["mesh_dir"], cat, n, "model.obj"), v, f)
        data_sdf.save_sample(dirs["sdf_dir"], cat, n, np.zeros((1, 3), np.float32), np.zeros((4, 4), np.float32),
                             np.float32([0, 0, 0, 0.7]), np.float32([-1, -1, -1, 1, 1, 1]))
    open(os.path.join(tmp, "lst", cat + "_test.lst"), "w").write("\n".join(names) + "\n")
    open(os.path.join(tmp, "lst", cat + "_train.lst"), "w").write("")
    json.dump({"lst_dir": os.path.join(tmp, "lst"), "cats": {"chair": cat}, "all_cats": ["chair"],
               "raw_dirs_v1": dirs}, open(os.path.join(tmp, "info.json"), "w"))
    t0 = time.perf_counter()
    stats = create_img_h5.main(["--info", os.path.join(tmp, "info.json"), "--render", "--writers", "8"])
    dt = time.perf_counter() - t0
    out["driver"] = {"objects": N, "seconds": dt, "objects_per_s": N / dt, "stats": stats, "writers": 8}
print(json.dumps(out), flush=True)
if args.out:
    with open(args.out, "w") as fo:
        json.dump(out, fo, indent=1)

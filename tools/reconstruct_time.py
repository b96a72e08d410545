"""One object of the test set at the reference's production shape -- 24 views, --sdf_res 64 -- the parent's way and
through ``create_sdf.reconstruct``; random weights, seeded inputs, one process.

    python tools/reconstruct_time.py [--reps 20] [--out profiles/reconstruct_time.json]

  (a) ``create_sdf`` (one encode call, 24 grids) followed by 24 x ``isosurface.marching_cubes`` (24 host syncs)
  (b) ``reconstruct``: the same encode and grids, ``marching_cubes_batch`` (one host sync)
Both variants are warmed, then alternate; every figure is the median over ``--reps`` repetitions with the spread
(min .. max).  The stages are timed with a device synchronise on both sides, so their sum exceeds the end-to-end
time of a variant, which is timed without the inner synchronisations.  The iso level is the median of view 0's grid
(random weights have no surface at 0).
"""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from disn_amd import create_sdf as cs, isosurface  # noqa: E402
from disn_amd.engine import SdfEngine  # noqa: E402
from disn_amd.weights import WeightStore  # noqa: E402

DEMO_TM = np.asarray([[-68.453156, 5.5086656, -0.37556022], [-17.138561, -84.685486, -0.250198],
                      [-47.284092, -3.6569588, 0.2493176], [101.133705, 101.34268, 1.4305686]], np.float32)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(xs):
    xs = np.asarray(xs, np.float64)
    return {"median_ms": float(np.median(xs)), "min_ms": float(xs.min()), "max_ms": float(xs.max()), "n": len(xs)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--sdf_res", type=int, default=64)
    ap.add_argument("--writers", type=int, default=4)
    ap.add_argument("--out", default=os.path.join("profiles", "reconstruct_time.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("reconstruct_time.py measures on a HIP device; none is visible")
    B, R = a.views, a.sdf_res
    rng = np.random.default_rng(0)
    eng = SdfEngine(WeightStore.random_init(0, mode="he"))
    imgs = torch.from_numpy(rng.random((B, 137, 137, 3), dtype=np.float32)).cuda()
    tms = torch.from_numpy(np.repeat(DEMO_TM[None], B, axis=0) * (1.0 + 0.01 * np.arange(B, dtype=np.float32)
                                                                   ).reshape(B, 1, 1)).cuda()
    boxes = np.tile(np.array([[-1, -1, -1, 1, 1, 1]], np.float64), (B, 1))
    iso = float(cs.create_sdf(eng, imgs, tms, boxes, R)[0].median())
    tmp = tempfile.mkdtemp(prefix="reconstruct_time_")

    def grids_of(enc):
        out = torch.empty((B, (R + 1) ** 3), dtype=torch.float32, device=eng.device)
        for b in range(B):
            cs.dense_grid_sdf(eng, enc, b, tms, boxes[b], R, out=out[b])
        return out

    def mesh_single(grids):
        return [isosurface.marching_cubes(grids[b], boxes[b], R, iso) for b in range(B)]

    def mesh_batch(grids):
        return isosurface.marching_cubes_batch(grids, boxes, R, iso)

    def write(meshes, pool):
        fs = [pool.submit(isosurface.write_obj, os.path.join(tmp, "v%02d.obj" % b), v, f)
              for b, (v, f) in enumerate(meshes)]
        for f in fs:
            f.result()

    def end_to_end_a(pool):
        g = cs.create_sdf(eng, imgs, tms, boxes, R)
        write(mesh_single(g), pool)

    def end_to_end_b(pool):
        write(cs.reconstruct(eng, imgs, tms, boxes, R, iso), pool)

    T = {k: [] for k in ("encode", "grids", "mesh_single", "mesh_batch", "write_single", "write_batch",
                         "end_to_end_single", "end_to_end_batch")}
    with ThreadPoolExecutor(max_workers=a.writers) as pool:
        for rep in range(-3, a.reps):                       # three warm-up rounds of everything, not recorded
            t_enc, enc = timed(lambda: eng.encode(imgs))
            t_grid, grids = timed(lambda: grids_of(enc))
            order = ("single", "batch") if rep % 2 == 0 else ("batch", "single")     # alternate who goes first
            t, m = {}, {}
            for which in order:
                t["mesh_" + which], m[which] = timed(lambda: (mesh_single if which == "single" else mesh_batch)(grids))
            for which in order:
                t["write_" + which], _ = timed(lambda: write(m[which], pool))
            for which in order:
                t["end_to_end_" + which], _ = timed(lambda: (end_to_end_a if which == "single" else end_to_end_b)(pool))
            if rep == 0:                                    # faster and different is not faster
                for b in range(B):
                    assert torch.equal(m["single"][b][0], m["batch"][b][0]) and torch.equal(m["single"][b][1],
                                                                                           m["batch"][b][1]), b
                tris = [int(f.shape[0]) for _, f in m["batch"]]
            if rep >= 0:
                T["encode"].append(t_enc)
                T["grids"].append(t_grid)
                for k, v in t.items():
                    T[k].append(v)
    res = {"views": B, "sdf_res": R, "iso": iso, "reps": a.reps, "writers": a.writers,
           "triangles_per_view": {"min": min(tris), "median": int(np.median(tris)), "max": max(tris)},
           "device": torch.cuda.get_device_name(0), "stages": {k: stats(v) for k, v in T.items()}}
    s = res["stages"]
    spread = max(s["mesh_single"]["max_ms"] - s["mesh_single"]["min_ms"],
                 s["mesh_batch"]["max_ms"] - s["mesh_batch"]["min_ms"])
    res["meshing"] = {"single_over_batch": s["mesh_single"]["median_ms"] / s["mesh_batch"]["median_ms"],
                      "spread_ms": spread,
                      "batch_not_slower": s["mesh_batch"]["median_ms"] <= s["mesh_single"]["median_ms"] + spread}
    print("%d views, sdf_res %d, iso %.6g, %d repetitions (median, min .. max; ms)" % (B, R, iso, a.reps))
    for k in T:
        print("  %-18s %9.3f  (%.3f .. %.3f)" % (k, s[k]["median_ms"], s[k]["min_ms"], s[k]["max_ms"]))
    print("  meshing: 24 single calls / one batched call = %.2f x; batched not slower: %s"
          % (res["meshing"]["single_over_batch"], res["meshing"]["batch_not_slower"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for fn in os.listdir(tmp):
        os.remove(os.path.join(tmp, fn))
    os.rmdir(tmp)
    return res


if __name__ == "__main__":
    main()

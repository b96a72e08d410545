"""What dual contouring costs beside marching cubes (DESIGN, "Dual contouring" and "Per-sheet dual contouring"): one
sphere field per resolution, the three meshers in one process, the network-normal pass timed on its own.

    python tools/dual_contour_time.py [--reps 20] [--out profiles/dual_contour_sheets_time.json]

(profiles/dual_contour_time.json is the record of this tool before it timed the per-sheet mesher.)

Per resolution (--sdf_res 64 and 256, one grid, a sphere of radius 0.6 in [-1,1]^3, iso 0), alternating who goes first:
  marching_cubes    ``isosurface.marching_cubes_batch``: count, read-back of the sizes, emit
  dual_contour      ``isosurface.dual_contour_batch`` with normals that are already on the device (the analytic ones,
                    computed before the clock starts): count, read-back of the sizes, points, emit
  dual_contour_grid the same with the grid normals (one more kernel)
  dual_contour_sheets, dual_contour_sheets_grid
                    the two above with ``sheets=True``: one vertex per sheet of a cell (on a sphere every cell has one
                    sheet, so the meshes are the same and the difference is the cost of the rule alone)
  network_normals   the network's unit gradients at the Hermite points (``SdfEngine.refine_vertices(iters=0)``, random
                    weights, in chunks of 32768 points): what ``--dc_normals network`` adds per view
with a device synchronise on both sides of every stage; every figure is the median over ``--reps`` repetitions with the
spread (min .. max) after three warm-up rounds.  Nothing is asserted: the numbers are a record.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from disn_amd import isosurface  # noqa: E402
from disn_amd.engine import SdfEngine  # noqa: E402
from disn_amd.weights import WeightStore  # noqa: E402

DEMO_TM = np.asarray([[-68.453156, 5.5086656, -0.37556022], [-17.138561, -84.685486, -0.250198],
                      [-47.284092, -3.6569588, 0.2493176], [101.133705, 101.34268, 1.4305686]], np.float32)
CHUNK = 32768


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(xs):
    xs = np.asarray(xs, np.float64)
    return {"median_ms": float(np.median(xs)), "min_ms": float(xs.min()), "max_ms": float(xs.max()), "n": len(xs)}


def shape(eng, enc, R, reps):
    box = np.array([[-1, -1, -1, 1, 1, 1]], np.float64)
    ax = torch.linspace(-1.0, 1.0, R + 1, dtype=torch.float64, device="cuda")
    z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")
    grid = (torch.sqrt(x * x + y * y + z * z) - 0.6).to(torch.float32).reshape(1, -1).contiguous()
    points = isosurface.dual_contour_batch(grid, box, R, 0.0, None, hermite=True)[0][2]
    analytic = (points / points.norm(dim=1, keepdim=True)).contiguous()

    def network(pts):
        return torch.cat([eng.refine_vertices(enc, 0, DEMO_TM, pts[k:k + CHUNK], iters=0)[1]
                          for k in range(0, len(pts), CHUNK)])

    stages = {
        "marching_cubes": lambda: isosurface.marching_cubes_batch(grid, box, R, 0.0),
        "dual_contour": lambda: isosurface.dual_contour_batch(grid, box, R, 0.0, lambda b, p: analytic),
        "dual_contour_grid": lambda: isosurface.dual_contour_batch(grid, box, R, 0.0, None),
        "dual_contour_sheets": lambda: isosurface.dual_contour_batch(grid, box, R, 0.0, lambda b, p: analytic,
                                                                     sheets=True),
        "dual_contour_sheets_grid": lambda: isosurface.dual_contour_batch(grid, box, R, 0.0, None, sheets=True),
        "network_normals": lambda: network(points),
    }
    T = {k: [] for k in stages}
    sizes = {}
    for rep in range(-3, reps):                                 # three warm-up rounds of everything, not recorded
        names = list(stages) if rep % 2 == 0 else list(stages)[::-1]
        for k in names:
            t, out = timed(stages[k])
            if rep >= 0:
                T[k].append(t)
            if rep == 0 and k != "network_normals":
                sizes[k] = {"vertices": int(len(out[0][0])), "triangles": int(len(out[0][1]))}
    s = {k: stats(v) for k, v in T.items()}
    res = {"sdf_res": R, "grids": 1, "reps": reps, "hermite_points": int(len(points)), "sizes": sizes, "stages": s,
           "dual_contour_over_marching_cubes": s["dual_contour"]["median_ms"] / s["marching_cubes"]["median_ms"],
           "dual_contour_sheets_over_dual_contour": s["dual_contour_sheets"]["median_ms"] / s["dual_contour"]["median_ms"]}
    print("sdf_res %d, %d Hermite points, %d repetitions (median, min .. max; ms)" % (R, len(points), reps))
    for k in stages:
        print("  %-26s %10.3f  (%.3f .. %.3f)   %s" % (k, s[k]["median_ms"], s[k]["min_ms"], s[k]["max_ms"],
                                                        sizes.get(k, "")))
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "dual_contour_sheets_time.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("dual_contour_time.py measures on a HIP device; none is visible")
    eng = SdfEngine(WeightStore.random_init(0, mode="he"))
    rng = np.random.default_rng(0)
    enc = eng.encode(torch.from_numpy(rng.random((1, 137, 137, 3), dtype=np.float32)).cuda())
    res = {"device": torch.cuda.get_device_name(0), "shapes": [shape(eng, enc, R, a.reps) for R in (64, 256)]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return res


if __name__ == "__main__":
    main()

"""Measure the sphere tracer (SdfEngine.trace) for the demo image and camera at 137 x 137 next to the grid +
marching-cubes path at R = 64 and R = 128 -> profiles/sdf_trace_time.json.

    python tools/sdf_trace_time.py [--size 137] [--runs 7] [--out profiles/sdf_trace_time.json]

He weights of seed 0 on the demo image (a RANDOM network's field: rough and far from metric; no trained checkpoint
exists here), iso 0 and the median of the 65^3 grid.  Every variant is warmed up once, then timed ``runs`` times in one
process, alternating, wall clock around a call that ends synchronised (the trace reads a count back every iteration, so
host time is part of what it costs); the median counts and the spread is recorded.  Also recorded, as a statistic:
the share of hit pixels whose depth lies behind the first sign change of a 256-sample uniform march along the same ray
through ``eng.query`` -- crossings the step rule walked over.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from disn_amd import isosurface, render       # noqa: E402
from disn_amd.engine import SdfEngine         # noqa: E402
from disn_amd.weights import WeightStore      # noqa: E402
from oracle import disn_oracle as O           # noqa: E402

BOX = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
ALL = ("rgba", "depth", "normal", "residual", "status")


def box_interval(cams, W, H):
    """float64 slab interval [t0, t1] of every ray with BOX (t0 >= 0; t1 < t0: no interval) and the rays"""
    c = cams.astype(np.float64)[0]
    x = np.arange(W) + 0.5
    y = np.arange(H) + 0.5
    d = c[3:6] + x[None, :, None] * c[6:9] + y[:, None, None] * c[9:12]
    d = d.reshape(-1, 3)
    with np.errstate(divide="ignore"):
        a = (np.asarray(BOX[:3]) - c[:3]) / d
        b = (np.asarray(BOX[3:]) - c[:3]) / d
    t0 = np.maximum(np.minimum(a, b).max(axis=1), 0.0)
    t1 = np.maximum(a, b).min(axis=1)
    return c[:3], d, t0, t1


def late_share(eng, enc, tm, cams, W, H, iso, depth, samples=256):
    """share of the hit pixels whose depth is later than the first sample of a uniform march at which f < 0"""
    org, d, t0, t1 = box_interval(cams, W, H)
    hit = np.nonzero(depth.reshape(-1) > 0)[0]
    if hit.size == 0:
        return None, 0
    t = t0[hit, None] + (t1[hit] - t0[hit])[:, None] * (np.arange(samples) + 0.5)[None, :] / samples
    p = (org[None, None, :] + t[:, :, None] * d[hit, None, :]).astype(np.float32).reshape(1, -1, 3)
    f = eng.query(enc, p, tm, fold=True, fused=True).cpu().numpy().reshape(hit.size, samples) / np.float32(10.0) - iso
    neg = f < 0
    first = np.where(neg.any(axis=1), t[np.arange(hit.size), neg.argmax(axis=1)], np.inf)
    late = depth.reshape(-1)[hit].astype(np.float64) > first
    return float(late.mean()), int(hit.size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=137)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sdf_trace_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sdf_trace_time needs a GPU")
    eng = SdfEngine(WeightStore.random_init(0, mode="he"))
    kat = np.load(os.path.join(ROOT, "tests", "golden", "oracle_kat.npz"))
    enc = eng.encode(kat["demo_img"].astype(np.float32) / np.float32(255.0))
    tm = torch.from_numpy(O.DEMO_TRANS_MAT).to(eng.device)
    W = H = a.size
    cams = render.sdf_ray_cameras(O.DEMO_TRANS_MAT, W, H)
    median = float(eng.query_grid(enc, 0, tm, BOX, 64, fused=True).median())
    result = {"size": a.size, "weights": "he seed 0", "image": "demo", "box": BOX, "median_iso": median, "runs": a.runs,
              "note": "random-network field; a trained field is unmeasured", "iso": {}}
    for iso_name, iso in (("iso0", 0.0), ("median", median)):
        last = {}

        def trace(iso=iso, last=last):
            last["out"] = eng.trace(enc, 0, tm, size=(W, H), sdf_params=BOX, iso=iso, want=ALL)

        def mesh(R, iso=iso, last=last):
            grid = eng.query_grid(enc, 0, tm, BOX, R, fused=True)
            v, f = isosurface.marching_cubes(grid, BOX, R, iso)
            last["mesh%d" % R] = (int(v.shape[0]), int(f.shape[0]))

        variants = {"trace": trace, "grid_mc_64": lambda: mesh(64), "grid_mc_128": lambda: mesh(128)}
        times = {k: [] for k in variants}
        for rnd in range(a.runs + 1):                   # round 0 warms up
            for k, f in variants.items():
                torch.cuda.synchronize()
                t = time.perf_counter()
                f()
                torch.cuda.synchronize()
                if rnd:
                    times[k].append((time.perf_counter() - t) * 1e3)
        out = last["out"]
        status = np.bincount(out["status"].cpu().numpy().reshape(-1), minlength=5).tolist()
        share, nhit = late_share(eng, enc, tm, cams, W, H, iso, out["depth"].cpu().numpy())
        res = out["residual"].cpu().numpy().reshape(-1)
        entry = {"iso": iso, "stats": out["stats"], "status_counts": status, "late_hit_share_256": share,
                 "max_residual_status1": float(res[out["status"].cpu().numpy().reshape(-1) == 1].max()) if status[1] else None,
                 "evaluations_over_65cubed": out["stats"]["evaluations"] / 65.0 ** 3,
                 "mesh_64": last["mesh64"], "mesh_128": last["mesh128"],
                 "ms": {k: float(np.median(v)) for k, v in times.items()}, "runs_ms": times}
        result["iso"][iso_name] = entry
        print("%-7s iso %.5f: %s status %s late share %s | trace %.2f ms, grid+mc 64 %.2f ms, 128 %.2f ms"
              % (iso_name, iso, out["stats"], status, share, entry["ms"]["trace"], entry["ms"]["grid_mc_64"],
                 entry["ms"]["grid_mc_128"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"out": a.out, "ms": {k: v["ms"] for k, v in result["iso"].items()}}))


if __name__ == "__main__":
    main()

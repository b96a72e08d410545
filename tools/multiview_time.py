"""Measure the multi-view grid (SdfEngine.query_grid_views) at R = 64 for V = 1, 2, 3, 8 views and both pools
next to the single-view grid of the same unfused arithmetic, query_grid(fold=False, fused=False)
-> profiles/multiview_time.json.

    python tools/multiview_time.py [--res 64] [--runs 9] [--reps 3] [--out profiles/multiview_time.json]

He weights of seed 0 on eight seeded random images with eight synthetic cameras (timing does not depend on what the
network has learnt).  Every variant is warmed up once, then timed ``runs`` times in one process, alternating; a sample
is a host clock around ``reps`` calls that end synchronised, divided by ``reps``; the median counts and every sample
is recorded.  The gather alone (65536 grid points, one chunk of the grid call) is timed the same way for every V next
to the single-view gather from the feature map (ops.project + ops.gather) and from the taps (ops.gather_taps), so
that the grid ratios can be told apart into gather and MLP.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from disn_amd import ops                      # noqa: E402
from disn_amd.engine import SdfEngine         # noqa: E402
from disn_amd.weights import WeightStore      # noqa: E402
from oracle import disn_oracle as O           # noqa: E402

BOX = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
VIEWS = (1, 2, 3, 8)
POOLS = ("max", "mean")
CHUNK = 65536


def alternate(variants, runs, reps):
    """{name: [ms per call] x runs}: round 0 warms up, then every round times every variant once"""
    times = {k: [] for k in variants}
    for rnd in range(runs + 1):
        for k, f in variants.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(reps):
                f()
            torch.cuda.synchronize()
            if rnd:
                times[k].append((time.perf_counter() - t) * 1e3 / reps)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=64)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multiview_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multiview_time needs a GPU")
    eng = SdfEngine(WeightStore.random_init(0, mode="he"))
    nv = max(VIEWS)
    imgs = O.synth_inputs(0, nv, 8)["imgs"]
    tms = np.stack([O.synth_trans_mat(30.0 + 41.0 * v, 15.0 + 3.0 * v, 0.8) for v in range(nv)]).astype(np.float32)
    enc = eng.encode(imgs)
    tm = torch.from_numpy(tms).to(eng.device)
    R = a.res
    total = (R + 1) ** 3

    grid = {"single_unfused": lambda: eng.query_grid(enc, 0, tm[:1], BOX, R, fold=False, fused=False)}
    for V in VIEWS:
        for pool in POOLS:
            grid["views%d_%s" % (V, pool)] = (lambda V=V, pool=pool: eng.query_grid_views(enc, (0, V), tm[:V], BOX, R, pool))
    grid_ms = alternate(grid, a.runs, a.reps)

    n = min(CHUNK, total)
    pts = ops.grid_points(BOX, R, 0, n, eng.device)
    feat = torch.empty((n, ops.FEAT_DIM), dtype=torch.float32, device=eng.device)
    fm = eng.featmap_of(enc)
    gather = {"single_from_map": lambda: ops.gather(fm[:1], ops.project(pts[None], tm[:1]), out=feat[None]),
              "single_from_taps": lambda: ops.gather_taps([t[:1] for t in enc.taps], tm[:1], pts[None], out=feat[None])}
    for V in VIEWS:
        for pool in POOLS:
            gather["views%d_%s" % (V, pool)] = (lambda V=V, pool=pool: ops.gather_taps_pool(
                [t[:V] for t in enc.taps], tm[:V], pts, pool, out=feat))
    gather_ms = alternate(gather, a.runs, max(a.reps, 10))

    med = lambda d: {k: float(np.median(v)) for k, v in d.items()}
    g, h = med(grid_ms), med(gather_ms)
    result = {"res": R, "points": total, "weights": "he seed 0", "images": "8 seeded random images", "runs": a.runs,
              "reps": a.reps, "grid_ms": g, "grid_runs_ms": grid_ms,
              "grid_ratio_to_single_unfused": {k: g[k] / g["single_unfused"] for k in g},
              "gather_points": n, "gather_ms": h, "gather_runs_ms": gather_ms,
              "gather_out_GBps": {k: n * ops.FEAT_DIM * 4 / (h[k] * 1e-3) / 1e9 for k in h},
              "device": torch.cuda.get_device_name(eng.device)}
    for k in g:
        print("grid   %-16s %8.3f ms  x%.3f" % (k, g[k], result["grid_ratio_to_single_unfused"][k]))
    for k in h:
        print("gather %-16s %8.3f ms  (%d points)" % (k, h[k], n))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"out": a.out, "grid_ms": g, "gather_ms": h}))


if __name__ == "__main__":
    main()

"""Time the narrow-band grid (SdfEngine.query_grid_band) against the dense fused grid (SdfEngine.query_grid) for one
image at R = 256 -> profiles/grid_band_time.json.

    python tools/grid_band_time.py [--res 256] [--reps 3] [--rounds 5] [--out profiles/grid_band_time.json] [--once]

He weights of the config-1 fixture (seed 0) on the demo image and camera; strides 4 and 8 at the defaults (margin 0.5,
dilate 1); iso 0 and the dense grid's median.  Every variant is warmed up, then the variants are timed with device
events around ``reps`` calls, ``rounds`` times ALTERNATING in one process (the spread between rounds is recorded: other
work shares the machine); the median counts.  The band call includes its one device-to-host copy of the two counts.
Next to every time ratio stands the share of the grid's points the network evaluated (stats): the expectation is
ratio ~ share + the selection and fill passes (a few streaming passes over (R+1)^3 floats).  The field is a RANDOM
network's: rough, its share an upper bound of what a smooth trained field needs -- the share on a trained field is
unmeasured.  ``--once``: warm up, then a single call of each variant -- the window for
``rocprofv3 --kernel-trace --stats -- python tools/grid_band_time.py --once``.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from disn_amd.engine import SdfEngine         # noqa: E402
from disn_amd.weights import WeightStore      # noqa: E402
from oracle import disn_oracle as O           # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_band_time.json"))
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grid_band_time needs a GPU")
    eng = SdfEngine(WeightStore.random_init(0, mode="he"))
    kat = np.load(os.path.join(ROOT, "tests", "golden", "oracle_kat.npz"))
    enc = eng.encode(kat["demo_img"].astype(np.float32) / np.float32(255.0))
    tm = torch.from_numpy(O.DEMO_TRANS_MAT).to(eng.device)
    box, R = [-1, -1, -1, 1, 1, 1], a.res
    total = (R + 1) ** 3
    out = torch.empty(total, dtype=torch.float32, device=eng.device)
    dense = lambda: eng.query_grid(enc, 0, tm, box, R, fused=True, out=out)
    median = float(dense().median())
    variants = {"dense": dense}
    stats = {}
    for iso_name, iso in (("iso0", 0.0), ("median", median)):
        for s in (4, 8):
            name = "band_s%d_%s" % (s, iso_name)

            def run(s=s, iso=iso, name=name):
                stats[name] = eng.query_grid_band(enc, 0, tm, box, R, iso=iso, stride=s, out=out)[1]
            variants[name] = run
    for _ in range(2):
        for f in variants.values():
            f()
    torch.cuda.synchronize()
    if a.once:
        for f in variants.values():
            f()
        torch.cuda.synchronize()
        return

    def window(f):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.reps):
            f()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / a.reps

    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, f in variants.items():
            times[k].append(window(f))
    d = float(np.median(times["dense"]))
    result = {"res": R, "total_points": total, "weights": "he seed 0", "image": "demo", "margin": 0.5, "dilate": 1,
              "median_iso": median, "reps": a.reps, "rounds": a.rounds,
              "dense_ms": d, "dense_rounds_ms": times["dense"], "variants": {},
              "note": "random-network field; the share on a trained field is unmeasured"}
    for k in variants:
        if k == "dense":
            continue
        t = float(np.median(times[k]))
        st = stats[k]
        share = (st["coarse_points"] + st["band_points"]) / float(st["total_points"])
        result["variants"][k] = {"ms": t, "rounds_ms": times[k], "time_ratio": t / d, "evaluated_share": share,
                                 "ratio_minus_share": t / d - share, "stats": st}
        print("%-16s %8.3f ms  ratio %.3f  evaluated share %.3f  (dense %.3f ms)" % (k, t, t / d, share, d))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"out": a.out, "dense_ms": d,
                      "ratios": {k: v["time_ratio"] for k, v in result["variants"].items()}}))


if __name__ == "__main__":
    main()

"""Times of the evaluation metrics (csrc/metrics.hip) on the GPU, with the VALU floor of the issue's cost model.

    python tools/metrics_time.py [--out FILE] [--quick]

Shapes: nn_distance (both directions) and emd at (1, 2048, 2048) and (24, 2048, 2048), approx_match at
(24, 2048, 2048), nn_distance at (1, 100000, 100000).  Device events around `iters` back-to-back calls after a
warm-up; random surface-like clouds.  --quick: a few calls of each (a workload for a rocprofv3 pass).
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from disn_amd import metrics  # noqa: E402

LANE_OPS = 256 * 4 * 16 * 2.4e9           # fp32 lane-ops/s: 256 CU x 4 SIMD x 16 lanes/clk x 2.4 GHz
SLOTS_NN, SLOTS_EMD = 6, 14               # issue slots per pair evaluation (cost model)


def clouds(b, n, m, seed=0):
    rng = np.random.default_rng(seed)

    def one(k):
        v = rng.standard_normal((b, k, 3))
        v /= np.linalg.norm(v, axis=2, keepdims=True)
        return torch.from_numpy((0.4 * v + 0.02 * rng.standard_normal((b, k, 3))).astype(np.float32)).cuda()
    return one(n), one(m)


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
    return s.elapsed_time(e) / iters * 1e3           # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    w, it = (1, 3) if a.quick else (5, 50)
    rows = []
    for name, (b, n, m), fn_name, slots, passes in (
            ("nn_distance", (1, 2048, 2048), "nn_distance", SLOTS_NN, 2),
            ("nn_distance", (24, 2048, 2048), "nn_distance", SLOTS_NN, 2),
            ("emd", (1, 2048, 2048), "emd", SLOTS_EMD, 30),
            ("emd", (24, 2048, 2048), "emd", SLOTS_EMD, 30),
            ("approx_match", (24, 2048, 2048), "approx_match", SLOTS_EMD, 30),
            ("nn_distance", (1, 100000, 100000), "nn_distance", SLOTS_NN, 2)):
        x1, x2 = clouds(b, n, m)
        f = getattr(metrics, fn_name)
        k = max(3, it // 10) if n >= 100000 or fn_name == "approx_match" else it
        us = timed(lambda: f(x1, x2), w, k)
        floor = passes * b * n * m * slots / LANE_OPS * 1e6
        rows.append("%-13s b=%-3d n=%-6d m=%-6d %10.1f us   VALU floor %8.1f us (%.0f %% of it)"
                    % (name, b, n, m, us, floor, 100.0 * floor / us))
        print(rows[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()

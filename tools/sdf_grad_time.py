"""Time SdfEngine.query_grad against the fused SdfEngine.query on one image x 65536 points.

    python tools/sdf_grad_time.py [--points 65536] [--reps 30] [--rounds 5] [--once]

The yardstick: central differences through ``query`` cost a user SIX evaluations per point (at far worse accuracy),
so ``query_grad`` should stay below 6 x the ``query`` time.  Both are timed with device events around ``reps`` calls,
warmed up, ``rounds`` times ALTERNATING (the spread between rounds is printed: other work shares the host); the last
line is one JSON object.  ``--once``: warm up, then a single call of each -- the window for
``rocprofv3 --kernel-trace --stats -- python tools/sdf_grad_time.py --once``.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from disn_amd import ops                      # noqa: E402
from disn_amd.engine import SdfEngine         # noqa: E402
from disn_amd.weights import WeightStore      # noqa: E402
from oracle import disn_oracle as O           # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sdf_grad_time needs a GPU")
    eng = SdfEngine(WeightStore.random_init(2, mode="he"))
    feed = O.synth_inputs(seed=3, n_points=8)
    enc = eng.encode(feed["imgs"])
    tm = torch.from_numpy(feed["trans_mat"]).to(eng.device)
    # a slab of the 257^3 grid: neighbouring points, what refinement and the dense grid feed
    pts = ops.grid_points([-1, -1, -1, 1, 1, 1], 256, 8000000, 8000000 + a.points, eng.device)[None].contiguous()
    grad = lambda: eng.query_grad(enc, pts, tm)
    fwd = lambda: eng.query(enc, pts, tm, fold=True, fused=True)
    for f in (grad, fwd, grad, fwd):
        f()
    torch.cuda.synchronize()
    if a.once:
        grad()
        fwd()
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

    tg, tf = [], []
    for _ in range(a.rounds):
        tg.append(window(grad))
        tf.append(window(fwd))
    g, q = float(np.median(tg)), float(np.median(tf))
    # both streams, four stacked rows per point: 64x256 + 256x512 + 512x512 + 512x256 multiply-adds per row and stream
    flop = 2.0 * 2 * 4 * a.points * (64 * 256 + 256 * 512 + 512 * 512 + 512 * 256)
    print("query_grad %.3f ms (rounds %s), fused query %.3f ms (rounds %s)"
          % (g, ["%.3f" % t for t in tg], q, ["%.3f" % t for t in tf]))
    print(json.dumps({"points": a.points, "query_grad_ms": g, "query_fused_ms": q, "ratio": g / q,
                      "yardstick_6x_query_ms": 6 * q, "query_grad_gemm_tflops": flop / (g * 1e-3) / 1e12}))


if __name__ == "__main__":
    main()

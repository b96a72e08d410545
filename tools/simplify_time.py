"""What the on-device mesh simplification costs and what it saves the writer: one object of the test set
the parent's way and with ``--simplify``, in one process; random weights, seeded inputs.

    python tools/simplify_time.py [--reps 20] [--out profiles/simplify_time.json]

Two shapes: 24 views at --sdf_res 64 with 32 cells, and ``--views_256`` (default 4) views at --sdf_res 256 with 64 cells.
Per shape the encoder and the grids run once (they are the same for both variants); then, alternating who goes first,
  baseline  ``marching_cubes_batch`` -> device-to-host copy + ``write_obj`` of every mesh (the parent commit's path)
  simplify  the same meshing -> ``simplify_meshes_device`` -> copy + ``write_obj`` of the simplified meshes
with a device synchronise on both sides of every stage; every figure is the median over ``--reps`` repetitions with the
spread (min .. max) after three warm-up rounds.  At --sdf_res 64 both variants are also timed end to end through
``create_sdf.reconstruct`` (encoder and grids included, no inner synchronisation).  The iso level is the median of view
0's grid (random weights have no surface at 0).  Triangles and bytes written are recorded in and out.
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

from disn_amd import create_sdf as cs, isosurface, postprocess  # noqa: E402
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


def shape(eng, B, R, cells, reps, writers, end_to_end):
    rng = np.random.default_rng(0)
    imgs = torch.from_numpy(rng.random((B, 137, 137, 3), dtype=np.float32)).cuda()
    tms = torch.from_numpy(np.repeat(DEMO_TM[None], B, axis=0) * (1.0 + 0.01 * np.arange(B, dtype=np.float32)
                                                                   ).reshape(B, 1, 1)).cuda()
    boxes = np.tile(np.array([[-1, -1, -1, 1, 1, 1]], np.float64), (B, 1))
    iso = float(cs.create_sdf(eng, imgs[:1], tms[:1], boxes[:1], min(R, 64))[0].median())
    t_enc, enc = timed(lambda: eng.encode(imgs))

    def grids_of():
        out = torch.empty((B, (R + 1) ** 3), dtype=torch.float32, device=eng.device)
        for b in range(B):
            cs.dense_grid_sdf(eng, enc, b, tms, boxes[b], R, out=out[b])
        return out

    t_grid, grids = timed(grids_of)
    tmp = tempfile.mkdtemp(prefix="simplify_time_")

    def write(meshes, pool, tag):
        fs = [pool.submit(isosurface.write_obj, os.path.join(tmp, "%s%02d.obj" % (tag, b)), m[0], m[1])
              for b, m in enumerate(meshes)]
        for f in fs:
            f.result()

    def size(tag):
        return sum(os.path.getsize(os.path.join(tmp, fn)) for fn in os.listdir(tmp) if fn.startswith(tag))

    keys = ["mesh", "simplify", "write_baseline", "write_simplified"]
    if end_to_end:
        keys += ["end_to_end_baseline", "end_to_end_simplify"]
    T = {k: [] for k in keys}
    with ThreadPoolExecutor(max_workers=writers) as pool:
        for rep in range(-3, reps):                         # three warm-up rounds of everything, not recorded
            t = {}
            t["mesh"], meshes = timed(lambda: isosurface.marching_cubes_batch(grids, boxes, R, iso))
            t["simplify"], (small, _) = timed(lambda: postprocess.simplify_meshes_device(meshes, boxes, cells))
            order = ("baseline", "simplified") if rep % 2 == 0 else ("simplified", "baseline")     # alternate
            for which in order:
                t["write_" + which], _ = timed(lambda: write(meshes if which == "baseline" else small, pool, which[0]))
            if end_to_end:
                for which in (("baseline", "simplify") if rep % 2 == 0 else ("simplify", "baseline")):
                    more = {} if which == "baseline" else {"simplify": cells}
                    t["end_to_end_" + which], _ = timed(
                        lambda: write(cs.reconstruct(eng, imgs, tms, boxes, R, iso, **more), pool, "e"))
            if rep == 0:
                tris_in, tris_out = [int(len(m[1])) for m in meshes], [int(len(m[1])) for m in small]
                verts_in, verts_out = [int(len(m[0])) for m in meshes], [int(len(m[0])) for m in small]
                bytes_in, bytes_out = size("b"), size("s")
            if rep >= 0:
                for k, v in t.items():
                    T[k].append(v)
    for fn in os.listdir(tmp):
        os.remove(os.path.join(tmp, fn))
    os.rmdir(tmp)
    s = {k: stats(v) for k, v in T.items()}
    res = {"views": B, "sdf_res": R, "cells": cells, "iso": iso, "reps": reps, "writers": writers,
           "encode_once_ms": t_enc, "grids_once_ms": t_grid,
           "triangles": {"in": sum(tris_in), "out": sum(tris_out), "per_view_in": [min(tris_in), max(tris_in)],
                         "per_view_out": [min(tris_out), max(tris_out)]},
           "vertices": {"in": sum(verts_in), "out": sum(verts_out)},
           "bytes_written": {"in": bytes_in, "out": bytes_out}, "stages": s}
    saved = s["write_baseline"]["median_ms"] - s["write_simplified"]["median_ms"]
    res["write_time_saved_ms"] = saved
    res["simplify_costs_less_than_it_saves"] = bool(s["simplify"]["median_ms"] < saved)
    print("%d views, sdf_res %d, cells %d, iso %.6g, %d repetitions (median, min .. max; ms)" % (B, R, cells, iso, reps))
    print("  encode (once) %.3f   grids (once) %.3f" % (t_enc, t_grid))
    for k in keys:
        print("  %-20s %10.3f  (%.3f .. %.3f)" % (k, s[k]["median_ms"], s[k]["min_ms"], s[k]["max_ms"]))
    print("  triangles %d -> %d, vertices %d -> %d, bytes written %d -> %d" % (
        sum(tris_in), sum(tris_out), sum(verts_in), sum(verts_out), bytes_in, bytes_out))
    print("  the stage costs %.3f ms and takes %.3f ms off the write: %s" % (
        s["simplify"]["median_ms"], saved, "it pays" if res["simplify_costs_less_than_it_saves"] else "IT DOES NOT PAY"))
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--views", type=int, default=24, help="views at --sdf_res 64 [24]")
    ap.add_argument("--views_256", type=int, default=4, help="views at --sdf_res 256 [4]")
    ap.add_argument("--writers", type=int, default=4)
    ap.add_argument("--out", default=os.path.join("profiles", "simplify_time.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("simplify_time.py measures on a HIP device; none is visible")
    eng = SdfEngine(WeightStore.random_init(0, mode="he"))
    res = {"device": torch.cuda.get_device_name(0),
           "shapes": [shape(eng, a.views, 64, 32, a.reps, a.writers, True),
                      shape(eng, a.views_256, 256, 64, a.reps, a.writers, False)]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return res


if __name__ == "__main__":
    main()

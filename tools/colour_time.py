"""What colouring the meshes on the device costs, and what the six-number vertex lines cost the writer: one
object of the test set the parent's way and with ``--colour``, in one process; random weights, seeded inputs.

    python tools/colour_time.py [--reps 20] [--reps_256 5] [--out profiles/colour_time.json]

Two shapes: 24 views at --sdf_res 64, and ``--views_256`` (default 4) views at --sdf_res 256; every mesh is coloured
from its own view (S = 2, 32 fill rounds: the defaults of ``--colour``).  Per shape the encoder and the grids run once;
then, alternating who goes first,
  baseline  ``marching_cubes_batch`` -> device-to-host copy + ``write_obj`` of every mesh (the parent commit's path)
  colour    the same meshing -> ``colour_meshes_device`` -> copy + ``write_obj(colours=)``
with a device synchronise on both sides of every stage, and both variants end to end through ``create_sdf.reconstruct``
(encoder and grids included, no inner synchronisation) + write.  Every figure is the median over the repetitions with
the spread (min .. max) after the warm-up rounds.  The iso level is the median of view 0's grid (random weights have no
surface at 0).  Vertices, classes and bytes written are recorded.
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


def shape(eng, B, R, reps, warm, writers):
    rng = np.random.default_rng(0)
    imgs = torch.from_numpy(rng.random((B, 137, 137, 3), dtype=np.float32)).cuda()
    tms_h = np.repeat(DEMO_TM[None], B, axis=0) * (1.0 + 0.01 * np.arange(B, dtype=np.float32)).reshape(B, 1, 1)
    tms = torch.from_numpy(tms_h).cuda()
    boxes = np.tile(np.array([[-1, -1, -1, 1, 1, 1]], np.float64), (B, 1))
    iso = float(cs.create_sdf(eng, imgs[:1], tms[:1], boxes[:1], min(R, 64))[0].median())
    t_enc, enc = timed(lambda: eng.encode(imgs))

    def grids_of():
        out = torch.empty((B, (R + 1) ** 3), dtype=torch.float32, device=eng.device)
        for b in range(B):
            cs.dense_grid_sdf(eng, enc, b, tms, boxes[b], R, out=out[b])
        return out

    t_grid, grids = timed(grids_of)
    tmp = tempfile.mkdtemp(prefix="colour_time_")

    def write(meshes, pool, tag, coloured):
        fs = [pool.submit(isosurface.write_obj, os.path.join(tmp, "%s%02d.obj" % (tag, b)), m[0], m[1],
                          **({"colours": m[-1]} if coloured else {})) for b, m in enumerate(meshes)]
        for f in fs:
            f.result()

    def size(tag):
        return sum(os.path.getsize(os.path.join(tmp, fn)) for fn in os.listdir(tmp) if fn.startswith(tag))

    keys = ["mesh", "colour", "write_baseline", "write_coloured", "end_to_end_baseline", "end_to_end_colour"]
    T = {k: [] for k in keys}
    with ThreadPoolExecutor(max_workers=writers) as pool:
        for rep in range(-warm, reps):                      # warm-up rounds of everything, not recorded
            t = {}
            t["mesh"], meshes = timed(lambda: isosurface.marching_cubes_batch(grids, boxes, R, iso))
            t["colour"], (cols, classes) = timed(lambda: postprocess.colour_meshes_device(meshes, imgs, tms_h))
            both = [m + (c,) for m, c in zip(meshes, cols)]
            for which in (("baseline", "coloured") if rep % 2 == 0 else ("coloured", "baseline")):     # alternate
                t["write_" + which], _ = timed(lambda: write(both, pool, which[0], which == "coloured"))
            for which in (("baseline", "colour") if rep % 2 == 0 else ("colour", "baseline")):
                more = {} if which == "baseline" else {"colour": True}
                t["end_to_end_" + which], _ = timed(
                    lambda: write(cs.reconstruct(eng, imgs, tms, boxes, R, iso, **more), pool, "e", bool(more)))
            if rep == 0:
                verts, tris = sum(int(len(m[0])) for m in meshes), sum(int(len(m[1])) for m in meshes)
                counts = np.bincount(torch.cat(classes).cpu().numpy(), minlength=4).tolist()
                bytes_plain, bytes_col = size("b"), size("c")
            if rep >= 0:
                for k, v in t.items():
                    T[k].append(v)
    for fn in os.listdir(tmp):
        os.remove(os.path.join(tmp, fn))
    os.rmdir(tmp)
    s = {k: stats(v) for k, v in T.items()}
    res = {"views": B, "sdf_res": R, "iso": iso, "reps": reps, "warm_up": warm, "writers": writers, "S": 2,
           "fill_iters": 32, "encode_once_ms": t_enc, "grids_once_ms": t_grid, "vertices": verts, "triangles": tris,
           "classes": {"fallback": counts[0], "seen": counts[1], "mirror": counts[2], "fill": counts[3]},
           "bytes_written": {"plain": bytes_plain, "coloured": bytes_col}, "stages": s}
    print("%d views, sdf_res %d, iso %.6g, %d repetitions (median, min .. max; ms)" % (B, R, iso, reps))
    print("  encode (once) %.3f   grids (once) %.3f" % (t_enc, t_grid))
    for k in keys:
        print("  %-20s %10.3f  (%.3f .. %.3f)" % (k, s[k]["median_ms"], s[k]["min_ms"], s[k]["max_ms"]))
    print("  %d vertices, %d triangles, classes %s, bytes written %d -> %d" % (verts, tris, res["classes"], bytes_plain,
                                                                             bytes_col))
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="repetitions at --sdf_res 64 [20]")
    ap.add_argument("--reps_256", type=int, default=5, help="repetitions at --sdf_res 256 [5]")
    ap.add_argument("--views", type=int, default=24, help="views at --sdf_res 64 [24]")
    ap.add_argument("--views_256", type=int, default=4, help="views at --sdf_res 256 [4]")
    ap.add_argument("--writers", type=int, default=4)
    ap.add_argument("--out", default=os.path.join("profiles", "colour_time.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("colour_time.py measures on a HIP device; none is visible")
    eng = SdfEngine(WeightStore.random_init(0, mode="he"))
    res = {"device": torch.cuda.get_device_name(0),
           "shapes": [shape(eng, a.views, 64, a.reps, 3, a.writers), shape(eng, a.views_256, 256, a.reps_256, 2, a.writers)]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return res


if __name__ == "__main__":
    main()

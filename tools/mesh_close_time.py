"""What the mesh closing costs beside the mesh repair of the same group.

    python tools/mesh_close_time.py [--reps 20] [--group 4] [--commit ID] [--out profiles/mesh_close_time.json]
    rocprofv3 --kernel-trace --stats -- python tools/mesh_close_time.py --only 256 --reps 3      (the kernel table)

Per resolution (--sdf_res 64 and 256: 65^3 and 257^3 grid points) two groups of ``--group`` sphere grids in [-1,1]^3, iso
0, meshed by dual contouring with the grid's normals:
  closed  radii 0.45 .. 0.75: nothing to flip and nothing to fill, the stage's fixed cost
  open    radii 1.05 .. 1.25: the sphere leaves the box, six holes per mesh, and every second face is turned over
          first, so that the stage flips and fills
and per group, on the SAME meshes:
  repair  ``postprocess.repair_meshes_device`` of the meshes: ONE count call, one read-back, ONE emit call
  close   ``postprocess.close_meshes_device`` of what the repair left, orient and fill on: likewise
Each call is timed by a pair of device events on the stream the entries use (the read-back in the middle of a call lies
between them); the two calls alternate in order from repetition to repetition; every figure is the median over
``--reps`` repetitions with the spread (min .. max) after three warm-up rounds; ``close_over_repair`` is the ratio of the
two medians.  There is no bar: nothing is asserted beyond the stage's own guarantee, the numbers are a record.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from disn_amd import isosurface, postprocess  # noqa: E402

GROUPS = (("closed", 0.45, 0.75), ("open", 1.05, 1.25))


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    out = fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end), out


def stats(xs):
    xs = np.asarray(xs, np.float64)
    return {"median_ms": float(np.median(xs)), "min_ms": float(xs.min()), "max_ms": float(xs.max()), "n": len(xs)}


def shape(R, group, reps):
    boxes = np.tile(np.array([[-1, -1, -1, 1, 1, 1]], np.float64), (group, 1))
    ax = torch.linspace(-1.0, 1.0, R + 1, dtype=torch.float64, device="cuda")
    z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")
    d = torch.sqrt(x * x + y * y + z * z)
    res = {"sdf_res": R, "grids": group, "reps": reps, "groups": {}}
    print("sdf_res %d, %d grids, %d repetitions (median, min .. max; ms)" % (R, group, reps))
    for name, r0, r1 in GROUPS:
        grids = torch.stack([(d - r).to(torch.float32).reshape(-1) for r in np.linspace(r0, r1, group)]).contiguous()
        meshes = [m[:2] for m in isosurface.dual_contour_batch(grids, boxes, R, 0.0, None)]
        if name == "open":
            meshes = [(v, torch.where((torch.arange(len(f), device=f.device) % 2 == 0)[:, None], f[:, [0, 2, 1]], f)
                       .contiguous()) for v, f in meshes]
        repair = lambda: postprocess.repair_meshes_device(meshes, strict=False)
        repaired = [m[:2] for m in repair()[0]]
        close = lambda: postprocess.close_meshes_device(repaired, strict=False)
        T = {"repair": [], "close": []}
        for rep in range(-3, reps):
            for k, fn in (("repair", repair), ("close", close)) if rep % 2 == 0 else (("close", close), ("repair", repair)):
                t, out = timed(fn)
                if rep >= 0:
                    T[k].append(t)
        s = {k: stats(v) for k, v in T.items()}
        closed, reports = close()
        after = postprocess.check_meshes_device([m[:2] for m in closed], max_pairs=0, strict=False)
        ok = all(c["closed"] and c["oriented"] for c, r in zip(after, reports) if r["status"] == 0)
        nv, nf = sum(len(m[0]) for m in repaired), sum(len(m[1]) for m in repaired)
        res["groups"][name] = {
            "triangles": int(nf), "vertices": int(nv), "repair": s["repair"], "close": s["close"],
            "close_over_repair": s["close"]["median_ms"] / s["repair"]["median_ms"],
            "workspace_bytes": int(postprocess.lib().disn_mesh_close_workspace_bytes(group, nv, nf)),
            "status": [r["status"] for r in reports], "closed_and_oriented_after": bool(ok),
            "sums": {k: int(sum(r[k] for r in reports)) for k in postprocess.CLOSE_FIELDS if k != "status"}}
        g = res["groups"][name]
        print("  %-6s %9d triangles  repair %8.3f (%.3f .. %.3f)  close %8.3f (%.3f .. %.3f)  ratio %.2f  %s"
              % (name, nf, s["repair"]["median_ms"], s["repair"]["min_ms"], s["repair"]["max_ms"], s["close"]["median_ms"],
                 s["close"]["min_ms"], s["close"]["max_ms"], g["close_over_repair"], g["sums"]))
        if not ok:
            raise SystemExit("the closed meshes of group %r are not closed and oriented" % name)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--group", type=int, default=4)
    ap.add_argument("--only", type=int, default=None, metavar="RES", help="one resolution (for a profiler)")
    ap.add_argument("--commit", default="unknown", help="the commit this is measured at, for the record")
    ap.add_argument("--kernels", default=None, metavar="NOTE", help="what the profiler's kernel table showed, for the record")
    ap.add_argument("--out", default=os.path.join("profiles", "mesh_close_time.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("mesh_close_time.py measures on a HIP device; none is visible")
    if a.only is not None:
        return shape(a.only, a.group, a.reps)
    res = {"device": torch.cuda.get_device_name(0), "commit": a.commit,
           "shapes": [shape(R, a.group, a.reps) for R in (64, 256)], "kernels": a.kernels}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return res


if __name__ == "__main__":
    main()

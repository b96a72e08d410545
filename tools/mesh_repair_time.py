"""What the mesh repair costs beside the meshing of the same group and beside the mesh checks, and what
it does to the three meshers' meshes on the 65^3 grid of BASELINE config 1.

    python tools/mesh_repair_time.py [--reps 10] [--group 4] [--commit ID] [--out profiles/mesh_repair_time.json]
    rocprofv3 --kernel-trace --stats -- python tools/mesh_repair_time.py --only 256 --reps 3      (the kernel table)

Per resolution (--sdf_res 64 and 256: 65^3 and 257^3 grid points) a group of ``--group`` grids -- spheres of radius
0.45 .. 0.75 in [-1,1]^3, iso 0 -- and per mesher (``mc`` marching cubes, ``dc`` dual contouring and ``dcs`` per-sheet dual
contouring, both with the grid's normals):
  mesh    ``isosurface.marching_cubes_batch`` / ``dual_contour_batch`` of the group
  repair  ``postprocess.repair_meshes_device`` of the meshes it left, weld and stitch on: ONE count call, one read-back,
          ONE emit call
with a device synchronise on both sides of every stage; every figure is the median over ``--reps`` repetitions with the
spread (min .. max) after three warm-up rounds; ``repair_over_mesh`` is the ratio of the two medians, and ``check`` is the
check stage's median for the same group as profiles/mesh_check_time.json records it (None where it has no such group).
Then, once, the 65^3 grid of config 1 on random-init weights (tests/golden/mc_skimage.npz, ``cfg1grid65_vol``) through the
three meshers: the repair's report and what the check says before and after it -- a finding about an UNTRAINED network
(no trained one was available: the meshes of a trained network are unmeasured), not a pass or a fail.  There is no bar:
nothing is asserted, the numbers are a record.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from disn_amd import isosurface, postprocess  # noqa: E402

MESHERS = ("mc", "dc", "dcs")
CHECK_KEYS = ("boundary_edges", "nonmanifold_edges", "nonmanifold_vertices", "misoriented_edges", "zero_area_faces")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(xs):
    xs = np.asarray(xs, np.float64)
    return {"median_ms": float(np.median(xs)), "min_ms": float(xs.min()), "max_ms": float(xs.max()), "n": len(xs)}


def mesher(name, grids, boxes, R, iso):
    if name == "mc":
        return lambda: isosurface.marching_cubes_batch(grids, boxes, R, iso)
    return lambda: isosurface.dual_contour_batch(grids, boxes, R, iso, None, sheets=name == "dcs")


def check_record(R, group):
    """mesher -> the check stage's median of the group of this size, from profiles/mesh_check_time.json"""
    try:
        rec = json.load(open(os.path.join(ROOT, "profiles", "mesh_check_time.json")))
    except OSError:
        return {}
    for s in rec.get("shapes", []):
        if s["sdf_res"] == R and s["grids"] == group:
            return {k: m["check"]["median_ms"] for k, m in s["meshers"].items()}
    return {}


def shape(R, group, reps):
    boxes = np.tile(np.array([[-1, -1, -1, 1, 1, 1]], np.float64), (group, 1))
    ax = torch.linspace(-1.0, 1.0, R + 1, dtype=torch.float64, device="cuda")
    z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")
    d = torch.sqrt(x * x + y * y + z * z)
    radii = np.linspace(0.45, 0.75, group)
    grids = torch.stack([(d - r).to(torch.float32).reshape(-1) for r in radii]).contiguous()
    checks = check_record(R, group)
    res = {"sdf_res": R, "grids": group, "reps": reps, "meshers": {}}
    print("sdf_res %d, %d grids, %d repetitions (median, min .. max; ms)" % (R, group, reps))
    for name in MESHERS:
        make = mesher(name, grids, boxes, R, 0.0)
        meshes = [m[:2] for m in make()]
        repair = lambda: postprocess.repair_meshes_device(meshes, strict=False)
        T = {"mesh": [], "repair": []}
        for rep in range(-3, reps):
            for k, fn in (("mesh", make), ("repair", repair)) if rep % 2 == 0 else (("repair", repair), ("mesh", make)):
                t, out = timed(fn)
                if rep >= 0:
                    T[k].append(t)
        s = {k: stats(v) for k, v in T.items()}
        reports = repair()[1]
        res["meshers"][name] = {
            "triangles": int(sum(len(m[1]) for m in meshes)), "vertices": int(sum(len(m[0]) for m in meshes)),
            "mesh": s["mesh"], "repair": s["repair"],
            "repair_over_mesh": s["repair"]["median_ms"] / s["mesh"]["median_ms"], "check_median_ms": checks.get(name),
            "workspace_bytes": int(postprocess.lib().disn_mesh_repair_workspace_bytes(
                group, sum(len(m[0]) for m in meshes), sum(len(m[1]) for m in meshes))),
            "status": [r["status"] for r in reports],
            "sums": {k: int(sum(r[k] for r in reports)) for k in postprocess.REPAIR_FIELDS if k != "status"}}
        m = res["meshers"][name]
        print("  %-4s %9d triangles  mesh %9.3f (%.3f .. %.3f)  repair %9.3f (%.3f .. %.3f)  ratio %.2f  check %s"
              % (name, m["triangles"], s["mesh"]["median_ms"], s["mesh"]["min_ms"], s["mesh"]["max_ms"],
                 s["repair"]["median_ms"], s["repair"]["min_ms"], s["repair"]["max_ms"], m["repair_over_mesh"],
                 "%.3f" % checks[name] if name in checks else "not recorded"))
    return res


def config1():
    gold = np.load(os.path.join(ROOT, "tests", "golden", "mc_skimage.npz"))
    vol, iso, box = gold["cfg1grid65_vol"], float(gold["cfg1grid65_iso"]), gold["box"].reshape(1, 6)
    grids = torch.from_numpy(np.ascontiguousarray(vol.reshape(1, -1))).cuda()
    out = {"grid": "tests/golden/mc_skimage.npz cfg1grid65_vol", "iso": iso, "trained_network": "not available: unmeasured",
           "meshers": {}}
    for name in MESHERS:
        mesh = mesher(name, grids, box, 64, iso)()[0][:2]
        row = {}
        for label, kw in (("stitch", {}), ("cut", {"stitch": False})):
            (fixed,), (report,) = postprocess.repair_meshes_device([mesh], strict=False, **kw)
            after = postprocess.check_meshes_device([fixed[:2]], max_pairs=0, strict=False)[0]
            row[label] = {"report": report, "after": {k: after[k] for k in CHECK_KEYS}}
        before = postprocess.check_meshes_device([mesh], max_pairs=0, strict=False)[0]
        row["before"] = {k: before[k] for k in CHECK_KEYS}
        out["meshers"][name] = row
        print("config 1, %s: %s" % (name, row))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--group", type=int, default=4)
    ap.add_argument("--only", type=int, default=None, metavar="RES", help="one resolution, no config 1 (for a profiler)")
    ap.add_argument("--commit", default="unknown", help="the commit this is measured at, for the record")
    ap.add_argument("--kernels", default=None, metavar="NOTE", help="what the profiler's kernel table showed, for the record")
    ap.add_argument("--out", default=os.path.join("profiles", "mesh_repair_time.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("mesh_repair_time.py measures on a HIP device; none is visible")
    if a.only is not None:
        return shape(a.only, a.group, a.reps)
    res = {"device": torch.cuda.get_device_name(0), "commit": a.commit,
           "shapes": [shape(R, a.group, a.reps) for R in (64, 256)], "config1_random_init": config1(),
           "kernels": a.kernels}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return res


if __name__ == "__main__":
    main()

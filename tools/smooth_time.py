"""What the on-device Taubin smoothing costs: one ``smooth_meshes_device`` call on the 24 meshes the batched
mesher leaves at --sdf_res 64, 10 iterations, next to the ``simplify_meshes_device`` (32 cells) and
``clean_meshes_device`` calls on the same batch in the same run, and the host rule on one of the meshes
-> profiles/smooth_time.json.

    python tools/smooth_time.py [--reps 20] [--views 24] [--out profiles/smooth_time.json]

He weights of seed 0 on seeded random images; the iso level is the median of view 0's grid (random weights have no
surface at 0).  Three warm-up rounds of everything, then ``--reps`` rounds in which the three stages alternate who goes
first; a sample is a host clock around one call that ends in a device synchronise; median, min and max are recorded.
One step of the iteration is (call at 11 iterations - call at 1 iteration) / 20, the build the call at 1 iteration less
two steps.  How a step splits between the gather over the neighbours and the update of the vertex: the same number of
vertices wired as rings of degree 2, 6 and 12 (faces (i, i + k, i + k): the pair of equal corners counts for nothing),
whose step times are fitted by a line in the degree -- the intercept is the update with the step's own loads and
stores, the slope times the mesh's mean degree the gather; the real meshes' step against that line is what their
irregular rows cost.  Needs a GPU: there is no fallback.
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


def alternate(variants, reps, warm=3):
    """{name: [ms] x reps}: ``warm`` rounds not recorded, then every round times every variant once, rotating the order"""
    names = list(variants)
    times = {k: [] for k in names}
    for rnd in range(-warm, reps):
        for k in names[rnd % len(names):] + names[:rnd % len(names)]:
            ms, _ = timed(variants[k])
            if rnd >= 0:
                times[k].append(ms)
    return times


def ring(n, degree):
    """n vertices on a circle, vertex i joined to i +- 1 .. i +- degree / 2 -> (verts, faces) on the device"""
    t = np.linspace(0.0, 2.0 * np.pi, n, endpoint=False)
    v = np.stack([0.5 * np.cos(t), 0.5 * np.sin(t), 0.01 * np.sin(40.0 * t)], 1).astype(np.float32)
    i = np.arange(n, dtype=np.int64)
    f = np.concatenate([np.stack([i, (i + k) % n, (i + k) % n], 1) for k in range(1, degree // 2 + 1)]).astype(np.int32)
    return torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--sdf_res", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_time.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("smooth_time.py measures on a HIP device; none is visible")
    eng = SdfEngine(WeightStore.random_init(0, mode="he"))
    B, R = a.views, a.sdf_res
    rng = np.random.default_rng(0)
    imgs = torch.from_numpy(rng.random((B, 137, 137, 3), dtype=np.float32)).cuda()
    tms = torch.from_numpy(np.repeat(DEMO_TM[None], B, axis=0) * (1.0 + 0.01 * np.arange(B, dtype=np.float32)
                                                                   ).reshape(B, 1, 1)).cuda()
    boxes = np.tile(np.array([[-1, -1, -1, 1, 1, 1]], np.float64), (B, 1))
    iso = float(cs.create_sdf(eng, imgs[:1], tms[:1], boxes[:1], R)[0].median())
    enc = eng.encode(imgs)
    grids = torch.empty((B, (R + 1) ** 3), dtype=torch.float32, device=eng.device)
    for b in range(B):
        cs.dense_grid_sdf(eng, enc, b, tms, boxes[b], R, out=grids[b])
    meshes = [m for m in isosurface.marching_cubes_batch(grids, boxes, R, iso) if len(m[1])]
    boxes = boxes[:len(meshes)]
    smooth = cs.smooth_args(a.iters)
    cap = cs.smooth_cap(smooth, boxes, R)
    nv, nf = sum(len(m[0]) for m in meshes), sum(len(m[1]) for m in meshes)

    def smooth_call(ms, iters, c):
        return postprocess.smooth_meshes_device(ms, iters, smooth["lam"], smooth["mu"], True, c)

    out, status = smooth_call(meshes, a.iters, cap)
    assert not status.any(), status
    calls = alternate({
        "smooth": lambda: smooth_call(meshes, a.iters, cap),
        "smooth_1_iteration": lambda: smooth_call(meshes, 1, cap),
        "smooth_11_iterations": lambda: smooth_call(meshes, 11, cap),
        "simplify_32_cells": lambda: postprocess.simplify_meshes_device(meshes, boxes, 32),
        "clean": lambda: postprocess.clean_meshes_device(meshes, 0.5, 0.3, "face", strict=False),
    }, a.reps)
    s = {k: stats(v) for k, v in calls.items()}
    step = (s["smooth_11_iterations"]["median_ms"] - s["smooth_1_iteration"]["median_ms"]) / 20.0
    build = s["smooth_1_iteration"]["median_ms"] - 2.0 * step

    # the host rule on the largest mesh, and that the device gave its bits
    big = max(range(len(meshes)), key=lambda b: len(meshes[b][0]))
    hv, hf = meshes[big][0].cpu().numpy(), meshes[big][1].cpu().numpy()
    t0 = time.perf_counter()
    want = postprocess.smooth_arrays(hv, hf, iters=a.iters, max_move=float(cap[big]))
    host_ms = (time.perf_counter() - t0) * 1e3
    same_bits = bool(np.array_equal(out[big][0].cpu().numpy().view(np.uint32), want.view(np.uint32)))
    indptr, _, boundary = postprocess.smooth_graph(hf, len(hv))
    moved = np.abs(want.astype(np.float64) - hv.astype(np.float64))

    # gather against update: rings of the same number of vertices, degree 2, 6, 12
    degrees = {}
    for b, m in enumerate(meshes):
        degrees[b] = 2.0 * 3.0 * len(m[1]) / 2.0 / max(len(m[0]), 1)        # 3 nf / 2 edges, two ends each
    mean_degree = float(sum(degrees[b] * len(meshes[b][0]) for b in degrees) / nv)
    rings = {d: ring(nv, d) for d in (2, 6, 12)}
    variants = {}
    for d, m in rings.items():
        variants["ring%d_1" % d] = (lambda m=m: smooth_call([m], 1, None))
        variants["ring%d_11" % d] = (lambda m=m: smooth_call([m], 11, None))
    ring_ms = {k: stats(v) for k, v in alternate(variants, a.reps).items()}
    ring_step = {d: (ring_ms["ring%d_11" % d]["median_ms"] - ring_ms["ring%d_1" % d]["median_ms"]) / 20.0 for d in rings}
    slope, intercept = np.polyfit(np.array(list(ring_step), np.float64), np.array(list(ring_step.values())), 1)
    gather = float(slope) * mean_degree

    res = {"device": torch.cuda.get_device_name(0), "views": len(meshes), "sdf_res": R, "iso": iso, "iters": a.iters,
           "lam": smooth["lam"], "mu": smooth["mu"], "cap_cells": smooth["cap"], "reps": a.reps,
           "vertices": nv, "triangles": nf, "mean_degree": mean_degree, "calls": s,
           "step_ms": step, "build_ms": build, "steps_share_of_the_call": 2 * a.iters * step / s["smooth"]["median_ms"],
           "step_bytes_floor": {"bytes": int(nv * (12 + 12 + 12 + 4 + 4 + 1) + mean_degree * nv * (4 + 12)),
                                "note": "own position in and out, the input position, degree, row start, boundary "
                                        "byte; per neighbour its id and its position (no reuse counted)"},
           "host_rule": {"mesh": big, "vertices": len(hv), "triangles": len(hf), "ms": host_ms,
                         "device_has_its_bits": same_bits, "boundary_vertices": int(boundary.sum()),
                         "max_degree": int(np.diff(indptr).max()), "moved_max": float(moved.max()),
                         "moved_mean": float(moved.mean()), "cap": float(cap[big])},
           "rings": {"vertices": nv, "calls": ring_ms, "step_ms_by_degree": {str(d): t for d, t in ring_step.items()},
                     "fit_ms": {"per_neighbour": float(slope), "intercept": float(intercept)},
                     "split_at_the_meshes_mean_degree": {"update_ms": float(intercept), "gather_ms": gather,
                                                         "gather_share": gather / (gather + float(intercept)),
                                                         "real_step_over_fit": step / (gather + float(intercept))}}}
    res["step_bytes_floor"]["GBps_at_the_measured_step"] = res["step_bytes_floor"]["bytes"] / (step * 1e-3) / 1e9
    print("%d meshes, %d vertices, %d triangles, mean degree %.2f" % (len(meshes), nv, nf, mean_degree))
    for k, v in s.items():
        print("  %-22s %9.3f ms  (%.3f .. %.3f)" % (k, v["median_ms"], v["min_ms"], v["max_ms"]))
    print("  one step %.4f ms, build %.3f ms; rings: %s; fit %.5f ms / neighbour + %.4f ms" % (
        step, build, {d: round(t, 4) for d, t in ring_step.items()}, slope, intercept))
    print("  host rule on mesh %d (%d vertices): %.1f ms; the device has its bits: %s" % (big, len(hv), host_ms, same_bits))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    return res


if __name__ == "__main__":
    main()

"""Time of the device small-part cleanup against the host path it replaces.

    python tools/mesh_clean_time.py [--out profiles/mesh_clean_time.txt] [--reps 20]

Field: the union of three spheres (radius 0.3 at the origin, 0.08 at distance 0.25, 0.2 at distance 0.7) on [-1,1]^3.
  (a) the 24 meshes of a 65^3 group   (b) one 257^3 mesh
device = ``postprocess.clean_meshes_device`` on the views ``marching_cubes_batch`` returns (count, read-back, emit);
host   = the device-to-host copy of every mesh and ``postprocess.clean_arrays`` (what the two-step route pays, without
         its file reads and writes).
Both also give the cleanup's share of meshing + cleanup; (b) also its share of one ``create_sdf.reconstruct`` call at
257^3 (one random image through a He-initialised network: the encoder, 257^3 queries, the meshing).
Medians over ``--reps`` runs after 3 warm-up runs; device times are wall-clock around a synchronize."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from disn_amd import isosurface, postprocess  # noqa: E402


def field(R, k=0):
    ax = np.linspace(-1.0, 1.0, R + 1, dtype=np.float32)
    z, y, x = torch.meshgrid(*(torch.from_numpy(ax).cuda(),) * 3, indexing="ij")
    p = torch.stack([x, y, z], -1)
    e = torch.roll(torch.tensor([1.0, 0.0, 0.0], device="cuda"), k % 3) * (1.0 + 0.01 * (k // 3))
    d = torch.minimum(torch.minimum(p.norm(dim=-1) - 0.3, (p - 0.25 * e).norm(dim=-1) - 0.08),
                      (p + 0.7 * e).norm(dim=-1) - 0.2)
    return d.reshape(-1).contiguous()


def median_ms(fn, reps):
    for _ in range(3):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def case(name, R, B, reps, lines):
    sdf = torch.stack([field(R, k) for k in range(B)])
    boxes = np.tile(np.array([-1, -1, -1, 1, 1, 1], np.float64), (B, 1))
    meshes = isosurface.marching_cubes_batch(sdf, boxes, R, 0.0)
    nv, nf = sum(len(m[0]) for m in meshes), sum(len(m[1]) for m in meshes)

    def host():
        return [postprocess.clean_arrays(v.cpu().numpy(), f.cpu().numpy()) for v, f in meshes]

    def device():
        return postprocess.clean_meshes_device(meshes)

    want, (got, _) = host(), device()
    same = all(np.array_equal(g[0].cpu().numpy(), w[0]) and np.array_equal(g[1].cpu().numpy(), w[1])
               for g, w in zip(got, want))
    t_mc = median_ms(lambda: isosurface.marching_cubes_batch(sdf, boxes, R, 0.0), reps)
    t_dev, t_host = median_ms(device, reps), median_ms(host, max(3, reps // 4))
    lines.append("%s: %d meshes of %d^3, %d vertices, %d triangles in all, %d kept vertices; equal to the host: %s"
                 % (name, B, R + 1, nv, nf, sum(len(g[0]) for g in got), same))
    lines.append("    clean_meshes_device %.3f ms   host copy + clean_arrays %.3f ms   (ratio %.1f)"
                 % (t_dev, t_host, t_host / t_dev))
    lines.append("    marching_cubes_batch %.3f ms: the cleanup is %.1f %% of meshing + cleanup"
                 % (t_mc, 100.0 * t_dev / (t_mc + t_dev)))
    return same, t_dev


def reconstruct_share(t_dev, lines):
    from disn_amd import create_sdf as cs
    from disn_amd.demo import DEMO_SDF_PARAMS, DEMO_TRANS_MAT
    from disn_amd.engine import SdfEngine
    from disn_amd.weights import WeightStore
    eng = SdfEngine(WeightStore.random_init(0, mode="he"))
    img = np.random.default_rng(0).random((1, 137, 137, 3), dtype=np.float32)
    iso = float(cs.create_sdf(eng, img, DEMO_TRANS_MAT, DEMO_SDF_PARAMS, 32)[0].median())
    t = median_ms(lambda: cs.reconstruct(eng, img, DEMO_TRANS_MAT, DEMO_SDF_PARAMS, 256, iso), 3)
    lines.append("    reconstruct at 257^3 %.1f ms: the cleanup of (b), %.3f ms, is %.2f %% of it" % (t, t_dev, 100.0 * t_dev / t))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=None)
    p.add_argument("--reps", type=int, default=20)
    a = p.parse_args(argv)
    lines = ["device %s, %d repetitions (median)" % (torch.cuda.get_device_name(0), a.reps)]
    ok, _ = case("(a)", 64, 24, a.reps, lines)
    ok_b, t_b = case("(b)", 256, 1, a.reps, lines)
    reconstruct_share(t_b, lines)
    ok = ok and ok_b
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

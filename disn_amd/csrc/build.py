"""Build libdisn_amd.so for gfx950 with hipcc (cross-compiles without a GPU).

    python -m disn_amd.csrc.build [--force] [--verbose] [--tuning]

The library is built IN-TREE (disn_amd/csrc/libdisn_amd.so) so that it travels to the GPU
box with the repo snapshot.  elementwise.hip is compiled with -ffp-contract=off (bit-exact
rows A/D/E/F/J); everything else with the default contraction.
"""
from __future__ import annotations

import hashlib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(HERE, "libdisn_amd.so")
LIB_TUNING = os.path.join(HERE, "libdisn_amd_tuning.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = "gfx950"

SOURCES = {
    "gemm_mfma.hip": [],
    "gemv.hip": [],
    "gemm_tn_mfma.hip": [],
    "gemm_bf16_mfma.hip": [],
    "backward.hip": [],
    "backward_img.hip": ["-munsafe-fp-atomics", "-ffp-contract=off"],  # same lerp weights as the forward
    "train.hip": [],
    "cam_head.hip": [],
    "cam_train.hip": ["-ffp-contract=off"],    # fixed-order camera losses and head gradients
    "mlp_small.hip": [],
    "mlp_fused.hip": [],
    "sdf_grad.hip": ["-ffp-contract=off"],      # the projection rounds as elementwise.hip's: the forward gather's cell
    "conv_h2.hip": ["-mllvm", "-pragma-unroll-threshold=1000000"],
    "conv_h2w.hip": ["-mllvm", "-pragma-unroll-threshold=1000000"],   # the unrolled chunk bodies exceed the default 16 k
    "dense_h2.hip": [],
    "dense_h2w.hip": [],
    "elementwise.hip": ["-ffp-contract=off"],
    "marching_cubes.hip": ["-ffp-contract=off"],
    "grid_band.hip": ["-ffp-contract=off"],     # the rule and the fill bit-identical to their float32 restatement
    "metrics.hip": ["-ffp-contract=off"],       # nn_distance bit-identical to a float32 restatement
    "mesh_sdf.hip": ["-ffp-contract=off"],      # distances and crossings bit-identical to their restatements
    "render.hip": ["-ffp-contract=off"],        # hits, depth and shading bit-identical to their float32 restatement
    "sdf_trace.hip": ["-ffp-contract=off"],     # the ray state machine bit-identical to its float32 restatement
    "voxel.hip": ["-ffp-contract=off"],         # the overlap test bit-identical to its float32 restatement
    "mesh_clean.hip": ["-ffp-contract=off"],    # the keep rule's float64 arithmetic as clean_arrays states it
    "mesh_simplify.hip": ["-ffp-contract=off"],   # the cell and the solve round as simplify_arrays states them
    "mesh_colour.hip": ["-ffp-contract=off"],     # the raster and the samples round as colour_arrays states them
    "mesh_sample.hip": ["-ffp-contract=off"],     # the weights and the points round as sample_surface_arrays states them
    "mesh_smooth.hip": ["-ffp-contract=off"],     # the steps' float64 arithmetic rounds as smooth_arrays states it
    "mesh_check.hip": ["-ffp-contract=off"],      # the determinants, the areas and the volumes round as check_arrays states them
    "mesh_repair.hip": ["-ffp-contract=off"],     # the determinants of the angular rule round as repair_arrays states them
    "mesh_close.hip": ["-ffp-contract=off"],      # the centres and the volume terms round as close_arrays states them
    "dual_contour.hip": ["-ffp-contract=off"],    # the points, the quadric and the solve round as dual_contour_arrays states them
    "batch_assemble.hip": ["-ffp-contract=off"],  # sample_pc_rot in the order its bound is derived for
    "api.hip": [],
    "host_util.cpp": ["-msse4.2"],
    "mesh_host.cpp": [],
}
COMMON = ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]
HEADERS = ["kernels.hpp", "tuning.hpp", "h2_common.hpp", "mc_tables.h", "mesh_bvh.hpp", "mesh_batch.hpp",
           "grid_mesh.hpp", "mc_loops.h",
           os.path.join(ROOT, "include", "disn_amd.h"),
           os.path.join(ROOT, "include", "disn_amd_simplify.h"), os.path.join(ROOT, "include", "disn_amd_colour.h"),
           os.path.join(ROOT, "include", "disn_amd_sample.h"), os.path.join(ROOT, "include", "disn_amd_smooth.h"),
           os.path.join(ROOT, "include", "dc", "disn_amd_dc.h"),
           os.path.join(ROOT, "include", "dc", "disn_amd_dc_sheets.h"),
           os.path.join(ROOT, "include", "check", "disn_amd_check.h"),
           os.path.join(ROOT, "include", "repair", "disn_amd_repair.h"),
           os.path.join(ROOT, "include", "close", "disn_amd_close.h")]


def _digest(paths, extra=""):
    h = hashlib.sha256(extra.encode())
    for p in paths:
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def build(force: bool = False, verbose: bool = False, tuning: bool = False) -> str:
    """tuning=True: the same sources with -DDISN_TUNING (run-time knobs + disn_tuning_set, csrc/tuning.hpp)
    as libdisn_amd_tuning.so -- for tools/ only; the product library has no knobs."""
    lib = LIB_TUNING if tuning else LIB
    extra = ["-DDISN_TUNING"] if tuning else []
    srcs = {s: f + extra for s, f in SOURCES.items() if os.path.exists(os.path.join(HERE, s))}
    hdrs = [h if os.path.isabs(h) else os.path.join(HERE, h) for h in HEADERS]
    objs, jobs = [], []
    for src, flags in srcs.items():
        sp = os.path.join(HERE, src)
        tag = _digest([sp] + hdrs, " ".join(COMMON + flags))
        obj = os.path.join(HERE, "build", "%s.%s.o" % (src, tag))
        objs.append(obj)
        if force or not os.path.exists(obj):
            jobs.append((sp, obj, flags))
    os.makedirs(os.path.join(HERE, "build"), exist_ok=True)

    def compile_one(job):
        sp, obj, flags = job
        cmd = [HIPCC] + COMMON + flags + ["-c", sp, "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed for %s:\n%s\n%s" % (sp, r.stdout, r.stderr))
        if verbose and r.stderr.strip():
            print(r.stderr)
        return obj

    with ThreadPoolExecutor(max_workers=min(8, max(1, len(jobs)))) as ex:
        list(ex.map(compile_one, jobs))
    stamp = os.path.join(HERE, "build", "link_tuning.stamp" if tuning else "link.stamp")
    want = _digest(objs) if all(os.path.exists(o) for o in objs) else ""
    have = open(stamp).read().strip() if os.path.exists(stamp) else ""
    if force or jobs or not os.path.exists(lib) or want != have:
        cmd = [HIPCC, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", lib] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("link failed:\n%s\n%s" % (r.stdout, r.stderr))
        with open(stamp, "w") as f:
            f.write(want)
    # objects of earlier source states (other digests) would otherwise pile up and travel with every snapshot;
    # the twin build's objects (product <-> tuning) are recognised by ITS stamp's digest list and kept
    keep = set(objs)
    other = os.path.join(HERE, "build", "objs_tuning.txt" if not tuning else "objs.txt")
    if os.path.exists(other):
        keep.update(l.strip() for l in open(other))
    with open(os.path.join(HERE, "build", "objs.txt" if not tuning else "objs_tuning.txt"), "w") as f:
        f.write("\n".join(objs))
    for fn in os.listdir(os.path.join(HERE, "build")):
        fp = os.path.join(HERE, "build", fn)
        if fn.endswith(".o") and fp not in keep:
            os.remove(fp)
    return lib


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose="--verbose" in sys.argv or "-v" in sys.argv,
                tuning="--tuning" in sys.argv))

#!/usr/bin/env python
"""Benchmark of the DISN SDF-query hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Metric (BASELINE.json): SDF point queries / s on a 137x137 image with a 2048-point batch.
One STEP = one pass of the whole hot path over one batch of synthetic input, nothing cached:
resize 137->224, VGG-16, five tap up-samples, projection, gather, both point MLPs and their sum
for 2048 random query points (BASELINE config 2: "1xMI355X: VGG-16 encode + 2048 random query
points, img_feat_twostream, fp32, random-init weights").  Inputs are resident in HBM before the
timed region.  With N>1 every rank runs the same per-GPU workload on its own image / points
(replicas: the 2048-point step has no exchange step), value = N*2048*K / max-over-ranks time.
`python bench.py --gpus N` without a launcher re-executes itself under torch.distributed.run with N
ranks (one per GPU; on a box with fewer GPUs the ranks share devices -- plumbing only, it says so).

--workload grid: BASELINE configs 3 / 4 end to end.  One STEP = encode the image batch (every rank,
redundantly), evaluate the (R+1)^3 dense grid of every image with the flat index range sharded
contiguously over the ranks (disn_amd/parallel.py: no data-path collective), ONE all_gather of the
slices (RCCL over xGMI), marching cubes of image b on rank b % N.  N = 1: one image (config 3);
N > 1: eight images (config 4).  value = grid points evaluated per second, whole job.

A plain run does only what the headline figure needs: set-up, warm-up, the K timed steps, --dump-outputs if given,
the JSON line.  --dump-outputs DIR writes what the timed path returned in its last step as DIR/<name>.npy (float32 /
float64, 64 MB at most: a fixed, seeded sample of anything larger); the inputs depend on the arguments only, so two
builds run with the same arguments can be compared output for output.

With --full (off by default) the run also checks and measures what follows; the JSON then carries, besides the
contract line's fields,
  max_abs_diff_of_a_repeated_job (config) -- jobs submitted again after the timed region agree with their first run;
  phases_rank0 / roofline / all_gather (--workload grid) -- one extra instrumented step, phase by phase;
  roofline      -- the dominant kernel family (the 13 convolutions of one submitted call: conv_h2w.hip / conv_h2.hip,
                   two-term f16 split on the f16 MFMA pipes), duration of the launch chain measured with events on the
                   launch stream.  ONE convention for every MFMA roofline of the line: `achieved` / `frac` = EXECUTED
                   f16 MFMA flop (3 per fp32-accurate product block) against the 2.5 PFLOP/s dense f16 peak,
                   `frac_algorithmic` = 2 M N K flop against the same peak, `ceiling_tflops` = 2500 / 3 = 833;
  single_stream -- one step at a time (the main line submits --batch independent steps per call and keeps
                   --in-flight calls on the GPU);
  roofline_gather -- the gathers that are actually on the timed paths: project_gather_taps_kernel (the
                   step), gather_fold_kernel (layer-by-layer dense grid), and gather_kernel from
                   materialised maps incl. a 3-image case that exceeds the 256 MB Infinity Cache;
  roofline_mlp  -- the fused point-MLP kernels (same convention as `roofline`) and the layer-by-layer chain;
  query_only    -- encoder amortised (the >=1e7 pts/s target of north_star applies here);
  grid256       -- wall-clock of a full 257^3 dense-grid evaluation on this GPU (config 3, no MC);
  cpu_baseline  -- the oracle (numpy/torch-CPU restatement of the reference's algorithm as
                   written) timed on this box's host cores on the same workload (rank 0, N=1).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_FP32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
PEAK_F16_MFMA_TFLOPS = 2500.0      # MI355X_MICROARCH.md: v_mfma_f32_32x32x16_f16 / bf16, dense
PEAK_HBM_GBS = 8000.0              # MI355X_MICROARCH.md: HBM3E spec peak (6.3 TB/s achievable)
GATHER_BYTES_PER_PT = 29440        # 4 taps x 1472 ch x 4 B read + 1472 x 4 B write
MLP_FLOP_PER_PT = 2 * 1835904      # 3.67 MFLOP/pt, global 1024x512 block folded per image
VGG_LAYERS = [(3, 64, 224), (64, 64, 224), (64, 128, 112), (128, 128, 112), (128, 256, 56), (256, 256, 56),
              (256, 256, 56), (256, 512, 28), (512, 512, 28), (512, 512, 28), (512, 512, 14), (512, 512, 14),
              (512, 512, 14)]
N_POINTS = 2048


def ev_time_ms(fn, reps, torch):
    """average duration of fn() in ms, events recorded on the stream the kernels run on"""
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


DUMP_CAP_BYTES = 64 << 20


def dump_outputs(path, arrays):
    """--dump-outputs: arrays (name -> host array) as path/<name>.npy; float64 stays float64, everything else becomes
    float32 (integers float64: exact).  Each array gets an equal share of DUMP_CAP_BYTES; a larger one is cut to a fixed,
    seeded sample along its longest axis (the same indices from run to run for the same shape)."""
    os.makedirs(path, exist_ok=True)
    share = DUMP_CAP_BYTES // max(1, len(arrays)) - 1024          # (room for the .npy header)
    for name, a in arrays.items():
        a = np.asarray(a)
        a = a.astype(np.float64 if a.dtype == np.float64 or a.dtype.kind in "iub" else np.float32)
        if a.nbytes > share:
            ax = int(np.argmax(a.shape))
            keep = max(1, share // (a.nbytes // a.shape[ax]))
            idx = np.sort(np.random.default_rng(0).choice(a.shape[ax], size=keep, replace=False))
            a = np.take(a, idx, axis=ax)
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a))


def train_feed(torch, dev, B, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    feed = {"imgs": torch.rand((B, 137, 137, 3), device=dev, generator=g),
            "sample_pc": torch.rand((B, N_POINTS, 3), device=dev, generator=g) - 0.5,
            "trans_mat": torch.tensor([[[-68.453156, 5.5086656, -0.37556022], [-17.138561, -84.685486, -0.250198],
                                        [-47.284092, -3.6569588, 0.2493176], [101.133705, 101.34268, 1.4305686]]] * B,
                                      dtype=torch.float32, device=dev),
            "sdf": 0.05 * torch.randn((B, N_POINTS, 1), device=dev, generator=g)}
    feed["sample_pc_rot"] = feed["sample_pc"].clone()
    return feed


def train_bench(args, torch, dist, dev, world, rank, launched):
    """timed region = K full optimizer steps (forward, get_loss, backward of every variable, gradient
    exchange, Adam) with the batch resident in HBM"""
    from disn_amd.train_sdf import Trainer
    from disn_amd.weights import WeightStore
    B = args.train_batch
    bf = args.train_dtype == "bf16"
    tr = Trainer(WeightStore.random_init(0, mode="he"), dev, batch_size=B * world, precision=args.train_dtype)
    feed = train_feed(torch, dev, B, 1000 + rank)
    for _ in range(args.warmup):
        tr.step(feed)
    torch.cuda.synchronize()
    if launched:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        pred, losses, _ = tr.step(feed)
    torch.cuda.synchronize()
    if launched:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if launched:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"pred_sdf": pred.float().cpu().numpy(),
                                         **{"loss_" + k: np.float64(float(v)) for k, v in losses.items()}})
    loss = float(losses["overall_loss"])
    assert np.isfinite(loss)
    tr.close()
    return {"metric": "training samples/sec (train_sdf.py step: VGG-16 + two-stream SDF net, 2048 points/sample, "
                      "all variables trained, Adam)",
            "value": world * B * args.steps / dt, "unit": "samples/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": 1000.0 * dt / args.steps, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "bf16" if bf else "f32", "data": "synthetic",
            "config": {"workload": "BASELINE config 5 shape, %s: data-parallel training step, %d samples x %d "
                                   "points per GPU, random-init (he) weights" % (
                                       "bf16 multiply / fp32 accumulate, master weights and optimizer" if bf
                                       else "fp32 accuracy (the reference's precision; precision=%s)" % args.train_dtype,
                                       B, N_POINTS),
                       "global_batch": B * world, "points_per_sample": N_POINTS,
                       "parallelism": "dp%d (one sum all-reduce of the flat gradient buffer in two buckets, the "
                                      "fc+MLP bucket under the conv backward)" % world},
            "final_loss": loss}


def self_launch(args, argv):
    """python bench.py --gpus N (N > 1) without a launcher: run N ranks of this script on this node"""
    import socket
    import subprocess
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"),
               MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + argv
    return subprocess.call(cmd, env=env)


DEMO_TM = [[-68.453156, 5.5086656, -0.37556022], [-17.138561, -84.685486, -0.250198],
           [-47.284092, -3.6569588, 0.2493176], [101.133705, 101.34268, 1.4305686]]      # demo/demo.py:272-276
PEAK_F16X2_TFLOPS = 2500.0 / 3.0   # two-term fp16 split: 3 MFMAs (2.5 PFLOP/s dense) per product block


def grid_bench(args, torch, dist, dev, world, rank, launched, shared_gpu, backend):
    """BASELINE config 3 (N = 1) / config 4 (N > 1), end to end, nothing cached between steps"""
    from disn_amd import isosurface as iso
    from disn_amd import parallel
    from disn_amd.engine import SdfEngine
    from disn_amd.weights import WeightStore
    B = args.grid_images or (1 if world == 1 else 8)
    R = args.grid_res
    total = (R + 1) ** 3
    eng = SdfEngine(WeightStore.random_init(0, mode="xavier"), dev, fused=not args.unfused)
    rng = np.random.default_rng(7)                      # the same images on every rank (config 4 shards points)
    imgs = torch.from_numpy(rng.random((B, 137, 137, 3), dtype=np.float32)).to(dev)
    tms = torch.tensor([DEMO_TM] * B, dtype=torch.float32, device=dev)
    params = [[-1, -1, -1, 1, 1, 1]] * B
    mine = list(range(rank, B, world))

    a2a = args.exchange == "all_to_all"

    def step():
        if a2a:    # rank r receives the full grids of ITS images only (1/world of the all_gather's bytes)
            full, own = parallel.sharded_create_sdf(eng, imgs, tms, params, R, exchange="all_to_all")
            meshes = [iso.marching_cubes(full[i], params[b], R, 0.0) for i, b in enumerate(own)]
        else:
            full = parallel.sharded_create_sdf(eng, imgs, tms, params, R)          # [B, total] on every rank
            meshes = [iso.marching_cubes(full[b], params[b], R, 0.0) for b in mine]
        return full, meshes

    for _ in range(args.warmup):
        full, meshes = step()
    torch.cuda.synchronize()
    if launched:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        full, meshes = step()
    torch.cuda.synchronize()
    if launched:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if launched:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    assert bool(torch.isfinite(full).all())
    if args.dump_outputs and rank == 0:
        # this rank's grids (all_to_all: the images it meshes) and the first mesh it made
        out = {"sdf": full.cpu().numpy()}
        if meshes:
            out.update({"mesh_vertices": meshes[0][0].cpu().numpy(), "mesh_faces": meshes[0][1].cpu().numpy()})
        dump_outputs(args.dump_outputs, out)
    line = {
        "metric": "dense-grid SDF points/sec, end to end (encode + %d^3 grid + RCCL gather + marching cubes)" % (R + 1),
        "value": B * total * args.steps / dt, "unit": "points/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": 1000.0 * dt / args.steps, "higher_is_better": True,
        "scaling": "strong" if args.grid_images else ("weak" if world == 1 else "strong"),
        "vs_baseline": None,
        "dtype": "f32 results (products: two-term f16 split on v_mfma_f32_32x32x16_f16, ~22-bit operands, fp32 accumulate; "
                 "gather / projection / grid points / marching cubes: fp32 / fp64 as the reference)",
        "data": "synthetic",
        "config": {"workload": "BASELINE config %s: %d image(s) x %d^3 dense grid, query chunks sharded over %d "
                               "rank(s), one %s, marching cubes; img_feat_twostream, fp32, random-init "
                               "(xavier) weights, nothing cached between steps" % (
                                   "3" if world == 1 else "4", B, R + 1, world, args.exchange),
                   "images": B, "grid_points_per_image": total, "seconds_per_step": dt / args.steps,
                   "seconds_per_image": dt / args.steps / B,
                   "point_mlp": "layer-by-layer GEMMs (three-term bf16)" if args.unfused else
                                "fused kernels (two-term fp16, activations in registers)",
                   "parallelism": "contiguous flat-index slices x%d, redundant encode, one %s (%s)%s" % (
                       world, args.exchange, backend if launched else "none: single process",
                       "; ranks SHARE GPUs (plumbing run, not a scaling measurement)" if shared_gpu else "")},
        "mesh": {"vertices": int(sum(m[0].shape[0] for m in meshes)), "triangles": int(sum(m[1].shape[0] for m in meshes)),
                 "images_meshed_on_rank0": len(mine)},
    }
    if args.full:
        line.update(grid_phases(args, torch, dist, dev, world, rank, launched, backend, eng, imgs, tms, params, mine, full))
    return line


def grid_phases(args, torch, dist, dev, world, rank, launched, backend, eng, imgs, tms, params, mine, full):
    """--full: one instrumented step of the grid workload, where the time goes (synchronised phases; not part of the
    timed region)"""
    from disn_amd import isosurface as iso
    from disn_amd import parallel
    B, R = imgs.shape[0], args.grid_res
    total = (R + 1) ** 3
    a2a = args.exchange == "all_to_all"

    def timed(fn):
        torch.cuda.synchronize()
        a = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, time.perf_counter() - a
    from disn_amd.create_sdf import dense_grid_sdf
    enc, t_enc = timed(lambda: eng.encode(imgs))
    k0, k1 = parallel.shard_range(total, world, rank)
    pad = (total + world - 1) // world
    mine_buf = torch.zeros((B, pad), dtype=torch.float32, device=dev)

    def fill():
        for b in range(B):
            dense_grid_sdf(eng, enc, b, tms, params[b], R, out=mine_buf[b, :k1 - k0], k_range=(k0, k1))
    _, t_fold = timed(lambda: [eng.pmap_amax_of(enc, b) for b in range(B)])
    _, t_grid = timed(fill)
    gath, t_gather = None, None
    if launched:
        gath = torch.empty((world, B, pad), dtype=torch.float32, device=dev)

        def ag():
            if a2a:
                order = [b for d in range(world) for b in parallel.owned_images(B, world, d)]
                send = mine_buf[order].contiguous()
                recv = torch.empty((world, len(mine), pad), dtype=torch.float32, device=dev)
                dist.all_to_all_single(recv.view(-1), send.view(-1), output_split_sizes=[len(mine) * pad] * world,
                                       input_split_sizes=[len(parallel.owned_images(B, world, d)) * pad for d in range(world)])
            elif backend == "nccl":
                dist.all_gather_into_tensor(gath.view(-1), mine_buf.view(-1))
            else:
                dist.all_gather(list(gath.unbind(0)), mine_buf)
        _, t_gather = timed(ag)
    _, t_mc = timed(lambda: [iso.marching_cubes(full[i if a2a else b], params[b], R, 0.0) for i, b in enumerate(mine)])
    pts_rank = B * (k1 - k0)
    flop_pt = MLP_FLOP_PER_PT - 2 * 1472 * 512           # executed: local fold2/conv1 folded into the map
    peak = PEAK_FP32_MFMA_TFLOPS if args.unfused else PEAK_F16X2_TFLOPS
    mlp_tf = pts_rank * flop_pt / t_grid / 1e12
    return {
        "phases_rank0": {"encode_s": t_enc, "fold_local_s": t_fold, "grid_slice_s": t_grid,
                         "all_gather_s": t_gather, "marching_cubes_s": t_mc,
                         "note": "one extra step with a host sync between phases (their sum exceeds the "
                                 "overlapped step)"},
        "roofline": {"kernel": "mlp_fused_kernel<global> + <local>" if not args.unfused else "gemm_bf16_mfma<128,128,DENSE,3> chain",
                     "bound": "mfma", "achieved": mlp_tf, "peak": peak, "unit": "TFLOP/s", "frac": mlp_tf / peak,
                     "traffic": None, "flop_per_point": flop_pt, "points_this_rank": pts_rank,
                     "seconds_this_rank": t_grid,
                     "frac_of_f32_mfma_peak": mlp_tf / PEAK_FP32_MFMA_TFLOPS,
                     "note": "executed flops of this rank's grid slices / their wall time (gather from the "
                             "folded map and the final dot included in the time)"},
        "all_gather": None if t_gather is None else {
            "exchange": args.exchange,
            "bytes_received_per_rank": int(world * (len(mine) if a2a else B) * pad * 4), "seconds": t_gather,
            "GB_per_s": world * (len(mine) if a2a else B) * pad * 4 / t_gather / 1e9, "backend": backend},
    }


def dry_run(args, torch, dist, world, rank, launched):
    """the protocol of a run without its GPU work: what the driver's `python -m torch.distributed.run
    --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N [--workload grid|train]`
    goes through before and after the timed region -- env ranks, process group, barrier, K 'steps', barrier, MAX of the
    ranks' times, ONE JSON line from rank 0 -- with the compute replaced by nothing.  Backend gloo unless nccl is asked
    for (no device here); the shard arithmetic of the grid workload is the real one (disn_amd/parallel.py)."""
    backend = "gloo" if args.dist_backend in ("auto", "gloo") else args.dist_backend
    if launched:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend)
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        pass
    if launched:
        dist.barrier()
    dt = time.perf_counter() - t0
    if launched:
        t = torch.tensor([dt], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    extra = {}
    if args.workload == "grid":
        from disn_amd import parallel
        total = (args.grid_res + 1) ** 3
        lo, hi = parallel.shard_range(total, world, rank)
        sizes = torch.tensor([hi - lo], dtype=torch.int64)
        if launched:
            dist.all_reduce(sizes)
        assert int(sizes.item()) == total, "the ranks' flat-index slices do not tile the grid"
        extra = {"grid_points": total, "slice_rank0": [lo, hi], "exchange": args.exchange}
    metric = {"query": "SDF point queries/sec (VGG-16 encode + 2048-point two-stream query per step, 137x137 image)",
              "grid": "dense-grid SDF points/sec end to end (encode + (R+1)^3 grid + exchange + marching cubes)",
              "train": "training samples/sec (train_sdf.py step)"}[args.workload]
    line = {"metric": metric, "value": None, "unit": {"query": "points/s", "grid": "points/s", "train": "samples/s"}[args.workload],
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1000.0 * dt / max(1, args.steps),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "DRY RUN of --workload %s: launch / rendezvous / timing protocol only, no GPU work" % args.workload,
                       "parallelism": "%d ranks over %s" % (world, backend if launched else "none: single process")},
            "dry_run": True, **extra}
    if rank == 0:
        print(json.dumps(line))
    if launched:
        dist.barrier()
        dist.destroy_process_group()



def _accuracy_of_the_timed_mode(strict: bool, sb: int):
    """north_star's tolerance for the kernel FORMS the main line times, from the committed full sweep of this round
    (tests/test_gpu_sweep.py with DISN_SWEEP=full on a GPU box -> profiles/r06w_sweep_full.json: 48 trained-like weight
    sets x 8 images, max |pred_sdf - float64 oracle| per request); the line's own three-set spot check of the same
    forms on this box is cpu_baseline.parity_trained_like.sweep"""
    out = {"bar": 1e-5, "on": "pred_sdf (the un-divided network output; the SDF value is pred_sdf / 10)",
           "timed_forms": ("strict: the single-image forms for every call size" if strict else
                           ("batched forms (calls of >= 4 requests): segmented convolutions, matrix-pipe fc head, fused small-set MLP"
                            if sb >= 4 else "single-image forms (calls of < 4 requests)"))}
    try:
        sw = json.load(open(os.path.join(ROOT, "profiles", "r06w_sweep_full.json")))["summary"]
        bf = sw["by_form"]
        forms = ("strict4", "strict16") if strict else (("batch4", "batch16") if sb >= 4 else ("single",))
        out.update({"sweep_worst_of_the_timed_forms": max(bf[f]["max"] for f in forms),
                    "sweep_requests": sum(bf[f]["n"] for f in forms), "sweep_sets": sw["sets"],
                    "sweep_worst_of_every_form": sw["worst"], "within_bar": max(bf[f]["max"] for f in forms) <= 1e-5,
                    "source": "profiles/r06w_sweep_full.json (tests/test_gpu_sweep.py, DISN_SWEEP=full; asserts <= bar for every form)"})
    except Exception as e:   # the committed file is the evidence; its absence must not cost the line
        out["sweep"] = "profiles/r06w_sweep_full.json not readable: %r" % (e,)
    return out

def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default: 300 query, 5 grid, 50 train)")
    ap.add_argument("--warmup", type=int, default=None, help="untimed warm-up steps (default: 20 query, 1 grid, 5 train)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline figure: the repeated-job check, the roofline / grid / train / cpu legs "
                         "(--workload query) and the instrumented phase step (--workload grid)")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip roofline / grid / cpu legs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path returned in its last step as DIR/<name>.npy")
    ap.add_argument("--in-flight", type=int, default=2,
                    help="--workload query: independent submissions in flight on this GPU (disn_amd.engine.StepPipeline: "
                         "one HIP stream + host thread per context); 1 = one at a time")
    ap.add_argument("--batch", type=int, default=16,
                    help="--workload query: consecutive independent steps (image + 2048 points each) submitted as ONE "
                         "disn_encode_query call (StepPipeline(batch=)); every image keeps its own activation scales, "
                         "so its result is bit for bit the single-step one; 1 = one step per call")
    ap.add_argument("--reramp-s", type=float, default=0.05,
                    help="untimed: seconds of rehearsal steps between parking the garbage collector and the warm-up (the "
                         "collection idles the GPU long enough for its clocks to drop)")
    ap.add_argument("--spinup-s", type=float, default=0.25,
                    help="--workload query: seconds of untimed set-up steps before the --warmup steps (clock ramp, "
                         "allocator pools); 0 = none")
    ap.add_argument("--balance", type=int, default=0,
                    help="--workload query: 1 = the K steps of a run are cut into calls of equal size (a multiple of "
                         "--in-flight calls, none longer than --batch) instead of full calls + a short last one")
    ap.add_argument("--chained", type=int, default=0,
                    help="--workload query: 1 = one host thread submits the calls in order and call g + 1's convolution stack "
                         "starts behind call g's (two-stage pipeline: convolutions beside the previous call's tail)")
    ap.add_argument("--cpu-runs", type=int, default=5)
    ap.add_argument("--workload", choices=("query", "grid", "train"), default="query",
                    help="query: BASELINE.json metric (default); grid: configs 3/4 (dense grid + gather + marching "
                         "cubes); train: config-5 training step")
    ap.add_argument("--grid-res", type=int, default=256)
    ap.add_argument("--grid-images", type=int, default=0, help="0: 1 image at N=1 (config 3), 8 at N>1 (config 4)")
    ap.add_argument("--exchange", choices=("all_to_all", "all_gather"), default="all_to_all",
                    help="--workload grid, N > 1: all_to_all = rank r receives the full grids of the images it meshes "
                         "(1/N of the bytes); all_gather = every rank receives every grid")
    ap.add_argument("--unfused", action="store_true",
                    help="dense-grid / large queries through the layer-by-layer GEMM chain instead of the fused kernels")
    ap.add_argument("--dist-backend", choices=("auto", "nccl", "gloo"), default="auto",
                    help="auto: nccl (= RCCL); gloo when ranks must share a GPU (RCCL rejects duplicate devices)")
    ap.add_argument("--strict", action="store_true",
                    help="--workload query: disn_vgg_weights_t.strict_forms = 1 -- the single-image convolution kernels for calls "
                         "of any size (a request's taps are bit for bit those of the request alone; every request "
                         "of the trained-like sweep within 1e-5 of the float64 oracle) at about a third less throughput")
    ap.add_argument("--dry-run", action="store_true",
                    help="no GPU work: exercise the launch path only (self-launch -> torch.distributed.run -> rendezvous on "
                         "127.0.0.1 -> barrier / max-over-ranks timing -> ONE contract line from rank 0 with value null and "
                         "dry_run true); runs on a box without a GPU with --dist-backend gloo (tests/test_parallel.py)")
    ap.add_argument("--train-batch", type=int, default=8, help="images per GPU per training step")
    ap.add_argument("--train-dtype", choices=("f32", "f32_mfma", "bf16"), default="f32",
                    help="--workload train: f32 = the reference's precision (forward / data-gradient GEMMs as "
                         "a three-term bf16 split on the bf16 MFMA pipes, same error as f32_mfma = everything "
                         "on the f32-input MFMA); bf16 = mixed precision (bf16 multiply, fp32 accumulate / "
                         "master weights / optimizer)")
    args = ap.parse_args()
    if args.steps is None:
        args.steps = {"query": 300, "grid": 5, "train": 50}[args.workload]
    if args.warmup is None:
        args.warmup = {"query": 20, "grid": 1, "train": 5}[args.workload]
    launched = "RANK" in os.environ and "MASTER_PORT" in os.environ   # torch.distributed.run / torchrun
    if args.gpus > 1 and not launched:
        sys.exit(self_launch(args, sys.argv[1:]))

    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    shared_gpu, backend = False, "nccl"
    if args.dry_run:
        return dry_run(args, torch, dist, world, rank, launched)
    if launched:       # also with one rank: same RCCL init / barrier / all-reduce sequence as N ranks
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        ndev = torch.cuda.device_count()
        shared_gpu = world > ndev            # fewer GPUs than ranks: ranks share devices (plumbing runs only)
        torch.cuda.set_device(local % ndev)
        backend = args.dist_backend if args.dist_backend != "auto" else ("gloo" if shared_gpu else "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local % ndev))
        else:
            dist.init_process_group("gloo")
    else:
        torch.cuda.set_device(0)
    if args.gpus != world and rank == 0:
        print("warning: --gpus %d but WORLD_SIZE %d; reporting n_gpus=%d" % (args.gpus, world, world), file=sys.stderr)
    dev = torch.device("cuda", torch.cuda.current_device())

    from disn_amd import ops
    from disn_amd.engine import SdfEngine
    from disn_amd.weights import WeightStore

    if args.workload == "grid":
        line = grid_bench(args, torch, dist, dev, world, rank, launched, shared_gpu, backend)
        if rank == 0:
            print(json.dumps(line))
        if launched:
            dist.barrier()
            dist.destroy_process_group()
        return
    if args.workload == "train":
        # BASELINE config 5 (not the north-star metric): data-parallel training step, B images x 2048
        # points per GPU, fp32, TF Adam; gradients exchanged by RCCL under the convolution backward
        line = train_bench(args, torch, dist, dev, world, rank, launched)
        if rank == 0:
            print(json.dumps(line))
        if launched:
            dist.barrier()
            dist.destroy_process_group()
        return

    from disn_amd.engine import StepPipeline
    store = WeightStore.random_init(0, mode="xavier")          # "random-init weights" (create_sdf.py:184-192)
    S = max(1, args.in_flight)
    SB = max(1, args.batch)
    pipe = StepPipeline(store, dev, in_flight=S, batch=SB, strict=args.strict)
    eng = pipe.engines[0]
    rng = np.random.default_rng(1000 + rank)
    # every step of a call -- and of the calls in flight beside it -- has its own image, point set and camera:
    # a pool of 2 S SB distinct jobs, step k takes job k % pool
    POOL = 2 * S * SB
    # the requests of the pool lie back to back in three device buffers (images, point sets, cameras): consecutive jobs
    # of a call are then submitted without a concatenation (StepPipeline: zero-copy for contiguous requests)
    pool_img = torch.empty((POOL, 137, 137, 3), dtype=torch.float32, device=dev)
    pool_pts = torch.empty((POOL, N_POINTS, 3), dtype=torch.float32, device=dev)
    pool_tm = torch.empty((POOL, 4, 3), dtype=torch.float32, device=dev)
    pool = []
    for k in range(POOL):
        pool_img[k] = torch.from_numpy(rng.random((137, 137, 3), dtype=np.float32) * np.float32(0.5 + 0.5 * rng.random())).to(dev)
        pool_pts[k] = torch.from_numpy((rng.random((N_POINTS, 3), dtype=np.float32) * 2 - 1).astype(np.float32)).to(dev)
        ptm = torch.tensor(DEMO_TM, dtype=torch.float32, device=dev)
        ptm[3, :2] += float(k % 7) - 3.0                         # (shifts the projected points by a few pixels)
        pool_tm[k] = ptm
        pool.append((pool_img[k:k + 1], pool_pts[k:k + 1], pool_tm[k:k + 1]))
    img, pts, tm = pool[0]

    def run_steps(k):
        # rows A..H, every step, through the single overlapped entry (disn_encode_query): SB consecutive steps per
        # call, call j on engine context j % S (own HIP stream, own host thread); nothing cached between steps
        if args.balance or args.chained:
            return pipe.run([pool[i % POOL] for i in range(k)], balance=args.balance, chained=bool(args.chained))
        # step i takes job i % POOL; the jobs lie back to back in the pool's buffers and POOL is a multiple of SB: every
        # call is handed its SB consecutive requests as one view (StepPipeline.run_calls: no per-request host work)
        calls = [(pool_img[o % POOL:o % POOL + n], pool_pts[o % POOL:o % POOL + n], pool_tm[o % POOL:o % POOL + n])
                 for o, n in zip(range(0, k, SB), StepPipeline.call_sizes(k, SB, S, False))]
        res = pipe.run_calls(calls)
        return [r[j:j + 1] for r in res for j in range(r.shape[0])]

    # Set-up, untimed and independent of W: ~--spinup-s seconds of the same steps (GPU clocks, the caching allocator's
    # pools, every code path once), then the collector is parked -- a generation-2 collection of a process with torch
    # loaded stops every host thread for ~50 ms (measured: both feeder threads idle from 0.8 to 50.1 ms of a 60 ms
    # timed region), which is what timeit's gc.disable() is for.
    import gc
    t1 = time.perf_counter()
    # (with the call sizes of the timed run: K steps cut the same way -- a call size seen for the first time inside
    # the timed region costs allocator work, measured up to 5 ms once: r03n)
    rehearsal = args.steps if args.steps <= 8 * S * SB else 4 * S * SB
    while time.perf_counter() - t1 < args.spinup_s:
        run_steps(rehearsal)
        torch.cuda.synchronize()
    gc.collect()
    gc.freeze()
    gc.disable()
    # the collection above is ~50-100 ms of host work with an idle GPU: the part drops its clocks, and the warm-up calls
    # alone (4-6 ms of work) do not bring them back -- a 20-step run measured 12.7 M points/s behind 32 warm-up steps and
    # 13.7 M behind 200 (tools/driver_cmd_ab.sh, r04).  So the last --reramp-s of the set-up run AFTER the collector is
    # parked: the same rehearsal steps again, then the warm-up, then the timed region with nothing in between.
    t2 = time.perf_counter()
    while time.perf_counter() - t2 < args.reramp_s:
        run_steps(rehearsal)
        torch.cuda.synchronize()
    run_steps(max(args.warmup, S * SB))
    torch.cuda.synchronize()
    if os.environ.get("BENCH_DEBUG"):
        pipe.trace = []
    if launched:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    outs = run_steps(args.steps)
    torch.cuda.synchronize()
    if launched:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    gc.enable()
    if pipe.trace:
        print("[bench] enqueue times (ms after t0) per call: " +
              " ".join("%d[%s]:%.2f" % (i, g, (t - t0) * 1e3) for i, g, t in sorted(pipe.trace, key=lambda x: x[2])) +
              " | done %.2f" % (dt * 1e3), file=sys.stderr)
    out = outs[0]
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"pred_sdf": outs[-1].cpu().numpy()})      # [1, 2048]: the last timed step
    # Repeated-job check (--full; ADVICE r3: with --steps <= the pool size no job repeats INSIDE the timed region): after
    # the timed region the first jobs are submitted again, untimed, shifted by one position -- another slot of another
    # call, possibly the other form of the convolutions when the call is shorter than four images -- and must give the
    # same prediction up to fp32 summation order.  null = nothing was repeated (or no --full).
    n_rep = min(len(outs) - 1, POOL - 1, 2 * SB) if args.full else 0
    rep_diff = None
    if n_rep >= 1:
        again = pipe.run([pool[i + 1] for i in range(n_rep)])
        torch.cuda.synchronize()
        rep_diff = max(float((again[i] - outs[i + 1]).abs().max()) for i in range(n_rep))
    in_region = [float((outs[k] - outs[k - POOL]).abs().max()) for k in range(POOL, len(outs))] if args.full else []
    if in_region:
        rep_diff = max([rep_diff or 0.0] + in_region)
    assert rep_diff is None or rep_diff <= 1e-5, "a repeated step disagrees with its first run: %g" % rep_diff
    if launched:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    assert bool(torch.isfinite(out).all())
    value = world * N_POINTS * args.steps / dt
    line = {
        "metric": "SDF point queries/sec (137x137 img, 2048-pt batch, VGG-16 encode + two-stream query per batch)",
        "value": value, "unit": "points/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": 1000.0 * dt / args.steps, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32 results (products: two-term f16 split on v_mfma_f32_32x32x16_f16, ~22-bit operands, fp32 accumulate; "
                 "gather / projection / resize / fc: fp32 FMA)",
        "data": "synthetic", "steps_per_call": SB, "calls_in_flight": S,
        "accuracy": _accuracy_of_the_timed_mode(args.strict, SB),
        "config": {"workload": "BASELINE config 2: VGG-16 encode + 2048 random query points, img_feat_twostream, "
                               "fp32, random-init (xavier) weights, nothing cached between steps" + (
                                   " [--strict: single-image convolution kernels for every call size]" if args.strict else ""),
                   "strict": bool(args.strict),
                   "images_per_step_per_gpu": 1, "points_per_step_per_gpu": N_POINTS,
                   "steps_per_call": SB, "calls_in_flight": S, "spinup_s": args.spinup_s,
                   "distinct_jobs": POOL, "max_abs_diff_of_a_repeated_job": rep_diff,
                   "repeated_jobs_checked": max(0, n_rep) + len(in_region),
                   "untimed_warmup_note": "before the timed region: %.2f s of rehearsal steps (clock ramp, allocator pools; "
                                          "--spinup-s), the garbage collector parked, %.2f s of rehearsal steps again (the "
                                          "collection idles the GPU and its clocks drop; --reramp-s), then max(--warmup, %d) "
                                          "= %d warm-up steps -- more than --warmup %d asks for whenever that is less than "
                                          "one full round of calls" % (
                                              args.spinup_s, args.reramp_s, S * SB, max(args.warmup, S * SB), args.warmup),
                   "submission_note": "a STEP is one image + its 2048 query points, all of rows A..H; %d consecutive "
                                      "independent steps go into one disn_encode_query call (the fc weights, 495 MB, "
                                      "are read once per call; every launch carries %d images against the same fixed "
                                      "cost; per-image activation scales make an image's result independent of its "
                                      "companions: tests/test_gpu_model.py) and %d such calls are in flight "
                                      "(own workspaces, HIP stream and host thread each), filling the gaps between "
                                      "each other's dependent launches; --batch 1 --in-flight 1 = one step at a "
                                      "time (see single_stream)" % (SB, SB, S),
                   "parallelism": "replicas x%d (no data-path collective)%s" % (
                       world, "; ranks SHARE GPUs (plumbing run)" if shared_gpu else "")},
    }

    if rank == 0:
        print("[bench] main line: %.4g points/s, %.4f ms/step" % (value, line["ms_per_step"]), file=sys.stderr)
    if rank == 0 and world == 1 and args.full and not args.no_extras:   # roofline / cpu legs: N=1 only (bench contract)
        pmc = {}   # profiles/pmc_traffic.json (read in the roofline leg; the gather legs quote it too)
        # ---- one step at a time (the latency of a step; the main line overlaps S independent steps) ----------
        try:
            if S > 1 or SB > 1:
                ms1 = ev_time_ms(lambda: eng.encode_query(img, pts, tm), 50, torch)
                line["single_stream"] = {"ms_per_step": ms1, "points_per_s": N_POINTS / ms1 * 1e3,
                                         "note": "--batch 1 --in-flight 1: one step at a time, its ~35 dependent launches back to back "
                                                 "(the latency of a step)"}
        except Exception as e:   # a failing extra must not cost the contract line
            line.setdefault("extras_failed", {})['one step at a time'] = repr(e)
            print("[bench] extra failed: %s: %r" % ('one step at a time', e), file=sys.stderr)
        # ---- strict mode (strict_forms = 1): the same submission through the single-image convolution kernels -------
        try:
            if not args.strict and SB >= 4:
                pipe_s = StepPipeline(store, dev, in_flight=S, batch=SB, strict=True)
                ncall = 4 * S
                calls_s = [(pool_img[(g * SB) % POOL:(g * SB) % POOL + SB], pool_pts[(g * SB) % POOL:(g * SB) % POOL + SB],
                            pool_tm[(g * SB) % POOL:(g * SB) % POOL + SB]) for g in range(ncall)]
                pipe_s.run_calls(calls_s)
                torch.cuda.synchronize()
                ts = time.perf_counter()
                res_s = pipe_s.run_calls(calls_s)
                torch.cuda.synchronize()
                dts = time.perf_counter() - ts
                d_fast = float((res_s[0] - torch.cat(outs[:SB])).abs().max()) if len(outs) >= SB else None
                line["strict_mode"] = {"points_per_s": ncall * SB * N_POINTS / dts, "ms_per_step": 1e3 * dts / (ncall * SB),
                                       "steps": ncall * SB, "max_abs_diff_to_the_default_form": d_fast,
                                       "note": "disn_vgg_weights_t.strict_forms = 1 (StepPipeline(strict=True), --strict): the "
                                               "single-image forms of every kernel for every call size; a request's taps, embedding "
                                               "and pred_sdf are bit for bit those of the request alone.  Accuracy of both "
                                               "modes: cpu_baseline.parity_trained_like.sweep"}
                pipe_s.close()
                del pipe_s, res_s
                torch.cuda.empty_cache()
        except Exception as e:   # a failing extra must not cost the contract line
            line.setdefault("extras_failed", {})['strict mode'] = repr(e)
            print("[bench] extra failed: %s: %r" % ('strict mode', e), file=sys.stderr)
        # ---- roofline of the dominant kernel family: the 13 convolution launches of one step ----------------
        try:
            # Timed as the step runs them: ONE disn_vgg16_conv_stack call = resize + conv1_1_direct_kernel + 12
            # conv_h2_kernel launches (two-term f16 split: fp32-accurate, f16 MFMA pipes, fused pools), back to back
            # on the launch stream, HIP events around the call.  The resize launch (~5 us, 0.08 GFLOP-equivalent of
            # nothing) is inside the bracket and charged to the family.
            # The main line submits SB images per call, so the launches of the timed region are the SB-image ones:
            # they are the roofline's primary figures; the single-image chain (what rounds 1 and 2a reported, and what a
            # step run alone executes) is kept beside them as `single_image`.
            flop1 = sum(2.0 * hw * hw * cout * 9 * cin for cin, cout, hw in VGG_LAYERS)
            flop1_mfma = sum(2.0 * hw * hw * cout * 9 * cin for cin, cout, hw in VGG_LAYERS[1:])   # conv1_1 (K = 27) is fp32 FMA
            stack1 = ops.ConvStackRun(eng.weights.vgg, img, want_pool5=False)
            ms_1 = ev_time_ms(stack1.run, 50, torch)
            if SB > 1:
                imgs_sb = torch.cat([pool[k][0] for k in range(SB)], dim=0)      # SB distinct images
                stack = ops.ConvStackRun(eng.weights.vgg, imgs_sb, want_pool5=False)
                tot_ms = ev_time_ms(stack.run, 50, torch)
            else:
                tot_ms = ms_1
            tot_flop = flop1 * SB
            # EXECUTED matrix work: every product block of the 12 MFMA layers is three v_mfma_f32_32x32x16_f16
            # (l_a h_b + h_a l_b + h_a h_b) -> 3x the algorithmic FLOP on the f16 pipe, priced against ITS dense peak
            exec_tflops = 3.0 * flop1_mfma * SB / tot_ms / 1e9
            alg_tflops = tot_flop / tot_ms / 1e9
            # HBM-side bytes of the same 13 launches from the PMC passes of THIS round's build
            # (profiles/pmc_traffic.json: separate --pmc FETCH_SIZE / WRITE_SIZE runs, gfx950 x2 fetch correction,
            # write counter calibrated on the gather's known output bytes); the file names the build it was
            # measured on -- None if absent or measured at another batch size
            traffic, pmc = None, {}
            try:
                pmc = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
                if SB == 1:
                    traffic = pmc["conv_family_per_step"]["hbm_bytes"]
                elif (pmc.get("conv_family_batched") or {}).get("images") == SB:
                    traffic = pmc["conv_family_batched"]["hbm_bytes"]
            except Exception:
                pass
            line["roofline"] = {"kernel": "the 13 convolutions of one VGG-16 forward on the %d image(s) of one submitted call, "
                                          "as one disn_vgg16_conv_stack call: " % SB +
                                          "conv1_1_direct_kernel (fp32 FMA) + 12 conv_h2w_kernel / conv_h2_kernel launches "
                                          "(two-term f16 split, fp32-accurate, f16 MFMA pipes, pools fused) + the resize launch",
                                "bound": "mfma", "achieved": exec_tflops, "peak": PEAK_F16_MFMA_TFLOPS, "unit": "TFLOP/s",
                                "frac": exec_tflops / PEAK_F16_MFMA_TFLOPS,
                                "frac_algorithmic": alg_tflops / PEAK_F16_MFMA_TFLOPS,
                                "ceiling_tflops": PEAK_F16X2_TFLOPS,
                                "frac_of_ceiling": alg_tflops / PEAK_F16X2_TFLOPS,
                                "convention": "frac = EXECUTED f16 MFMA flop (3 per fp32-accurate product block) / time / 2500; "
                                              "frac_algorithmic = 2*M*N*K flop of all 13 layers / time / 2500; ceiling_tflops = 2500 / 3 = "
                                              "the most an fp32-accurate product can reach on the f16 pipe (frac_of_ceiling ~ frac)",
                                "achieved_note": "EXECUTED f16-MFMA TFLOP/s = 3 x the algorithmic FLOP of the 12 MFMA layers "
                                                 "(three v_mfma_f32_32x32x16_f16 per product block) / the duration of the whole "
                                                 "14-launch chain (conv1_1 and the resize are in the time, not in the FLOP), "
                                                 "against the dense f16 MFMA peak (MI355X_MICROARCH.md: 2.5 PFLOP/s)",
                                "algorithmic_tflops": alg_tflops,
                                "frac_of_f32_mfma_peak": alg_tflops / PEAK_FP32_MFMA_TFLOPS,
                                "sustained_mfma_ceiling": {
                                    "pure_mfma_tflops": 1690.0, "with_operand_reads_tflops": 1500.0,
                                    "frac_of_sustained": exec_tflops / 1500.0,
                                    "note": "measured on this part (tools/ubench/mfma_f16_rate.hip, profiles/r06i_mfma_f16_rate.txt): a kernel that "
                                            "issues NOTHING but back-to-back v_mfma_f32_32x32x16_f16 on random operands, every CU, 1 or 2 waves "
                                            "per SIMD, sustains 1.69 PFLOP/s = 0.68 of the 2.5 PFLOP/s data-sheet peak (DVFS: the clock drops "
                                            "under matrix load), and 1.50 PFLOP/s = 0.60 with the convolutions' operand traffic beside it (two "
                                            "ds_read_b128 per MFMA triple).  `frac` above stays priced against the data-sheet peak; "
                                            "frac_of_sustained is the same executed rate against what the silicon delivers to a pure MFMA+LDS stream"},
                                "traffic": traffic,
                                "traffic_measured_on": pmc.get("build"),
                                "traffic_note": "memory-side bytes per call of the 13 conv launches (FETCH_SIZE x2 + calibrated "
                                                "WRITE_SIZE; L2 misses served by MALL count), from profiles/pmc_traffic.json "
                                                "(separate --pmc passes on the build named in traffic_measured_on); "
                                                "algorithmic per call ~59 MB two-plane f16 weights "
                                                "+ ~104 MB per image (inputs 36 + outputs and pooled copies 68)",
                                "images_per_call": SB, "flop_per_call": tot_flop, "executed_mfma_flop_per_call": 3.0 * flop1_mfma * SB,
                                "ms_per_call": tot_ms, "launches": 14,
                                "single_image": {"ms": ms_1, "achieved": 3.0 * flop1_mfma / ms_1 / 1e9,
                                                 "frac": 3.0 * flop1_mfma / ms_1 / 1e9 / PEAK_F16_MFMA_TFLOPS,
                                                 "algorithmic_tflops": flop1 / ms_1 / 1e9,
                                                 "traffic": (pmc.get("conv_family_per_step") or {}).get("hbm_bytes"),
                                                 "note": "the same chain on ONE image (a step run alone: conv_h2_kernel, K "
                                                         "parallel inside the workgroup)"},
                                "per_launch": "profiles/r0*_conv_stack_b16_trace.txt (rocprofv3 kernel trace of the same call; the latest round's file)"}
        except Exception as e:   # a failing extra must not cost the contract line
            line.setdefault("extras_failed", {})['roofline of the dominant kernel family'] = repr(e)
            print("[bench] extra failed: %s: %r" % ('roofline of the dominant kernel family', e), file=sys.stderr)
        # ---- gathers (HBM / cache bound): the kernels that ARE on the timed paths ---------------------
        try:
            ACHIEVABLE = 6300.0      # MI355X_MICROARCH.md: measured float4-copy HBM rate; above it = cache bandwidth
            enc = eng.encode(img)
            eng.featmap_of(enc)
            g = {}

            def gline(ms, alg_bytes, note, traffic_key=None):
                gbs = alg_bytes / ms / 1e6
                d = {"ms": ms, "algorithmic_bytes": alg_bytes, "achieved": gbs, "frac": gbs / PEAK_HBM_GBS,
                     "traffic": (pmc.get(traffic_key) or {}).get("hbm_bytes") if traffic_key else None, "note": note}
                if gbs > ACHIEVABLE:
                    d["exceeds_achievable_hbm"] = ("%.0f GB/s is above the ~6300 GB/s HBM can stream: the source is "
                                                   "served by L2 / the 256 MB Infinity Cache" % gbs)
                return d
            # (1) the step's gather: project_gather_taps_kernel, 2048 points, taps resident in L2 / MALL.  Its
            #     algorithmic bytes in SURVEY 8(d)'s terms (a materialised map): 29 440 B/point; what it actually
            #     reads are 16 tap pixels per output float4 = 94 208 B/point of (cached) tap data + 5 888 written
            p2k = torch.rand((1, N_POINTS, 3), device=dev) * 2 - 1
            feat2k = torch.empty((1, N_POINTS, 1472), device=dev)
            ms = ev_time_ms(lambda: ops.gather_taps(enc.taps, tm, p2k, feat2k), 20, torch)
            g["step_project_gather_taps_n2048"] = gline(
                ms, N_POINTS * GATHER_BYTES_PER_PT,
                "the gather of ONE request (thread-per-float4 kernel: below 10 240 points per launch; hidden under fc6 on the auxiliary stream); 29 440 B/point convention; "
                "it reads %d B/point of L2/MALL-resident tap pixels" % (94208 + 5888), "gather_taps_n2048")
            # (2) the dense grid's gather in the layer-by-layer path: gather_fold_kernel, 65 536 points of one
            #     chunk: 4 x 2 KB pmap rows + 2 KB pre-activation read + 2 KB written per point = 12 288 B/point
            p64k = torch.rand((65536, 3), device=dev) * 2 - 1
            pm = eng.pmap_of(enc, 0)
            pre = torch.rand((65536, 512), device=dev)
            bias = torch.zeros(512, device=dev)
            h = torch.empty((65536, 512), device=dev)
            ms = ev_time_ms(lambda: ops.gather_fold(pm, tm[0].contiguous(), p64k, pre, bias, h), 20, torch)
            g["grid_gather_fold_n65536"] = gline(
                ms, 65536 * 12288, "layer-by-layer dense-grid path (--unfused); the 38 MB pmap is cache resident, "
                "only the 2 x 134 MB activation rows stream; in the fused kernels this gather is 16 LDS-DMA loads per "
                "tile inside mlp_fused_kernel<local> and has no launch of its own", "gather_fold_n65536")
            # (3) gather_kernel from a materialised map (disn_query): 1 image (110 MB map: Infinity-Cache resident)
            #     and 3 images (331 MB of maps: exceeds the 256 MB cache, so the reads are HBM reads)
            for nimg, n in ((1, N_POINTS), (1, 262144), (3, 262144)):
                fm = enc.featmap if nimg == 1 else enc.featmap.expand(3, -1, -1, -1).contiguous()
                p = torch.rand((nimg, n, 3), device=dev) * 2 - 1
                xy = ops.project(p, tm.expand(nimg, -1, -1).contiguous())
                feat = torch.empty((nimg, n, 1472), device=dev)
                ms = ev_time_ms(lambda: ops.gather(fm, xy, feat), 10, torch)
                g["gather_kernel_%dimg_n%d" % (nimg, n)] = gline(
                    ms, nimg * n * GATHER_BYTES_PER_PT,
                    "disn_gather from %d materialised map(s) of 110.5 MB%s" % (
                        nimg, " (> Infinity Cache: an HBM measurement)" if nimg == 3 else " (cache resident)"),
                    "gather_n%d" % n if nimg == 1 else None)
                del fm, p, xy, feat
            line["roofline_gather"] = {"bound": "hbm", "peak": PEAK_HBM_GBS, "achievable": ACHIEVABLE, "unit": "GB/s",
                                       "bytes_per_point_convention": GATHER_BYTES_PER_PT, **g}
            del pre, h, p64k, feat2k
        except Exception as e:   # a failing extra must not cost the contract line
            line.setdefault("extras_failed", {})['gathers'] = repr(e)
            print("[bench] extra failed: %s: %r" % ('gathers', e), file=sys.stderr)
        # ---- point MLP + query-only (encoder amortised): fused kernels and the layer-by-layer chain ----------
        try:
            from disn_amd.engine import FOLD_MIN_POINTS
            q = {}
            for n in (N_POINTS, 65536, 262144, 1048576):
                p = torch.rand((1, n, 3), device=dev) * 2 - 1
                folded = n >= FOLD_MIN_POINTS       # engine default: local fold2/conv1 folded into the feature map
                flop = MLP_FLOP_PER_PT - (2 * 1472 * 512 if folded else 0)
                e = {"folded_local_stream": folded, "executed_flop_per_point": flop}
                for name, kw in (("fused", {"fused": True}), ("layer_by_layer", {"fused": False})):
                    if name == "fused" and not folded:
                        continue                     # the engine uses the fused kernels for the folded form only
                    if name == "layer_by_layer" and n > 262144:
                        continue
                    eng.query(enc, p, tm, **kw)      # (builds the folded map once; it is per-image state)
                    ms = ev_time_ms(lambda: eng.query(enc, p, tm, **kw), 10 if n <= 262144 else 5, torch)
                    e[name] = {"ms": ms, "points_per_s": n / ms * 1e3, "mlp_tflops_lower_bound": n * flop / ms / 1e9}
                e["points_per_s"] = max(v["points_per_s"] for k, v in e.items() if isinstance(v, dict))
                q["n%d" % n] = e
            line["query_only"] = q
            bf = max(v["fused"]["mlp_tflops_lower_bound"] for v in q.values() if "fused" in v)
            bl = max(v["layer_by_layer"]["mlp_tflops_lower_bound"] for v in q.values() if "layer_by_layer" in v)
            line["roofline_mlp"] = {
                "kernel": "mlp_fused_kernel<global> + mlp_fused_kernel<local> (two launches per point set)",
                "bound": "mfma", "achieved": 3.0 * bf, "peak": PEAK_F16_MFMA_TFLOPS, "unit": "TFLOP/s",
                "frac": 3.0 * bf / PEAK_F16_MFMA_TFLOPS,
                "frac_algorithmic": bf / PEAK_F16_MFMA_TFLOPS, "algorithmic_tflops": bf,
                "ceiling_tflops": PEAK_F16X2_TFLOPS, "frac_of_ceiling": bf / PEAK_F16X2_TFLOPS,
                "convention": "same as `roofline`: achieved = EXECUTED f16 MFMA flop (3 per product block) / time against the "
                              "2.5 PFLOP/s dense f16 peak; frac_algorithmic = fp32-equivalent flop / time / 2500",
                "frac_of_f32_mfma_peak": bf / PEAK_FP32_MFMA_TFLOPS,
                "flop_per_point": MLP_FLOP_PER_PT - 2 * 1472 * 512,
                "layer_by_layer": {"kernel": "gemm_bf16_mfma<128,128,DENSE,3> x8 (+gather, embed, final) per chunk",
                                   "achieved": bl, "peak": PEAK_FP32_MFMA_TFLOPS, "frac": bl / PEAK_FP32_MFMA_TFLOPS},
                "note": "fp32-equivalent flops = 2.16 MFLOP/point (the 1472 feature rows of the local "
                        "fold2/conv1 are pre-multiplied into the feature map once per image, disn_fold_local) / wall "
                        "time of the whole query (projection, gather, final dot included): a lower bound on the MFMA rate"}
        except Exception as e:   # a failing extra must not cost the contract line
            line.setdefault("extras_failed", {})['point MLP + query-only'] = repr(e)
            print("[bench] extra failed: %s: %r" % ('point MLP + query-only', e), file=sys.stderr)
        # ---- the point MLP of the TIMED line: fused small-set kernels on the SB x 2048 points of one call ------------
        try:
            nb = max(SB, 4)
            imgs_nb = torch.cat([pool[k % POOL][0] for k in range(nb)], dim=0)
            pts_nb = torch.cat([pool[k % POOL][1] for k in range(nb)], dim=0)
            tms_nb = torch.cat([pool[k % POOL][2] for k in range(nb)], dim=0)
            enc_nb = eng.encode(imgs_nb)
            amax_nb = torch.stack([torch.stack([t[b].abs().max() for t in enc_nb.taps]).max() for b in range(nb)]).contiguous()
            ms_gather = ev_time_ms(lambda: ops.gather_taps_split(enc_nb.taps, tms_nb, pts_nb, amax_nb), 20, torch)
            ms_all = ev_time_ms(lambda: ops.query_taps_fused(eng.weights.mlp, enc_nb.taps, enc_nb.embedding, tms_nb, pts_nb), 20, torch)
            flop = nb * N_POINTS * MLP_FLOP_PER_PT
            # the gather of a batched call (round 6: one wave per point, project_gather_taps_wave_kernel<split>), alone on the GPU
            if isinstance(line.get("roofline_gather"), dict):
                gb = nb * N_POINTS * GATHER_BYTES_PER_PT
                line["roofline_gather"]["call_project_gather_taps_wave_%dx%d" % (nb, N_POINTS)] = {
                    "ms": ms_gather, "algorithmic_bytes": gb, "achieved": gb / ms_gather / 1e6, "frac": gb / ms_gather / 1e6 / PEAK_HBM_GBS,
                    "traffic": (((pmc.get("small_set_b16") or {}).get("gather_split") or {}).get("hbm_bytes")
                                if nb == 16 and ((pmc.get("small_set_b16") or {}).get("gather_split") or {}).get("kernel") == "project_gather_taps_wave_kernel" else None),
                    "note": "the gather of the timed call in split form [h8 | l8] (project_gather_taps_wave_kernel: one wave per point, "
                            "duplicate tap rows / columns skipped by scalar branches; ~36 KB/point requested through L1 against the "
                            "thread-per-float4 kernel's 100 KB; the same bits); 29 440 B/point convention; A/B: profiles/r06j_gather_ab.txt"}
            line["roofline_mlp_small"] = {
                "kernel": "disn_query_taps_fused on the %d x %d points of one call: 5 x amax64 + tap_amax + project_gather_taps_wave_kernel "
                          "(split form) + mlp_fused_kernel<local, FEAT> + the global bias fold (split-K GEMV) + mlp_fused_kernel<global>" % (nb, N_POINTS),
                "bound": "mfma", "ms": ms_all, "ms_gather_alone": ms_gather, "ms_mlp_without_gather": ms_all - ms_gather,
                "achieved": 3.0 * flop / ms_all / 1e9, "peak": PEAK_F16_MFMA_TFLOPS, "unit": "TFLOP/s",
                "frac": 3.0 * flop / ms_all / 1e9 / PEAK_F16_MFMA_TFLOPS,
                "frac_algorithmic": flop / ms_all / 1e9 / PEAK_F16_MFMA_TFLOPS, "ceiling_tflops": PEAK_F16X2_TFLOPS,
                "flop_per_point": MLP_FLOP_PER_PT, "points_per_s": nb * N_POINTS / ms_all * 1e3,
                "note": "gather + point MLP of one submitted call, alone on the GPU (VERDICT r3 #1's figure; round 3's seven "
                        "dense_h2w launches + two gathers took ~0.72 ms for 16 x 2048 points)"}
            del enc_nb, imgs_nb, pts_nb
        except Exception as e:   # a failing extra must not cost the contract line
            line.setdefault("extras_failed", {})['small-set point MLP'] = repr(e)
            print("[bench] extra failed: %s: %r" % ('small-set point MLP', e), file=sys.stderr)
        # ---- config 3: full 257^3 grid on one GPU (no marching cubes yet) -----------------------
        try:
            from disn_amd import create_sdf as cs
            g256 = {}
            for name, fz in (("fused", True), ("layer_by_layer", False)):
                eng.fused = fz
                cs.dense_grid_sdf(eng, eng.encode(img), 0, tm, [-1, -1, -1, 1, 1, 1], 256)   # warm-up (workspaces)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                enc3 = eng.encode(img)
                full = cs.dense_grid_sdf(eng, enc3, 0, tm, [-1, -1, -1, 1, 1, 1], 256)
                torch.cuda.synchronize()
                t1 = time.perf_counter() - t0
                g256[name] = {"seconds": t1, "points_per_s": 257 ** 3 / t1}
            eng.fused = True
            line["grid256"] = {"points": 257 ** 3, "seconds": g256["fused"]["seconds"],
                               "points_per_s": g256["fused"]["points_per_s"], **g256,
                               "includes": "encode + feature-map fold + every grid point + /10, single GPU, no marching "
                                           "cubes; `fused`: mlp_fused_kernel (engine default), `layer_by_layer`: the "
                                           "65536-point chunks of GEMM launches (round-1 path)"}
            # config 3 end to end: + marching cubes on the device (+ the .obj the reference writes)
            from disn_amd import isosurface as iso
            iso.marching_cubes(full, [-1, -1, -1, 1, 1, 1], 256, 0.0)         # warm-up (workspace, code)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            enc3 = eng.encode(img)
            full = cs.dense_grid_sdf(eng, enc3, 0, tm, [-1, -1, -1, 1, 1, 1], 256)
            verts, faces = iso.marching_cubes(full, [-1, -1, -1, 1, 1, 1], 256, 0.0)
            torch.cuda.synchronize()
            t2 = time.perf_counter() - t0
            with tempfile.TemporaryDirectory() as td_:
                t0 = time.perf_counter()
                iso.write_obj(os.path.join(td_, "mesh.obj"), verts, faces)
                t3 = time.perf_counter() - t0
            line["grid256_mesh"] = {"seconds": t2, "vertices": int(verts.shape[0]), "triangles": int(faces.shape[0]),
                                    "obj_write_seconds": t3,
                                    "includes": "encode + 257^3 SDF + marching cubes on one GPU (random-init weights: "
                                                "the iso-surface of an untrained net); .obj write timed separately"}
            del full
        except Exception as e:   # a failing extra must not cost the contract line
            line.setdefault("extras_failed", {})['config 3'] = repr(e)
            print("[bench] extra failed: %s: %r" % ('config 3', e), file=sys.stderr)
        # ---- training step (BASELINE config 5 shape, one GPU's share: 8 samples x 2048 points) -----
        try:
            try:
                from disn_amd.train_sdf import Trainer
                tr = Trainer(WeightStore.random_init(0, mode="he"), dev, batch_size=8)
                tfeed = train_feed(torch, dev, 8, 1)
                for _ in range(2):
                    tr.step(tfeed)
                ms_fb = ev_time_ms(lambda: tr.forward_backward(tfeed), 5, torch)
                ms_step = ev_time_ms(lambda: tr.step(tfeed), 5, torch)
                # 3x the forward MACs of the convolutions and the two point MLPs (data + weight gradients)
                conv_flop = 8 * sum(2.0 * hw * hw * cout * 9 * cin for cin, cout, hw in VGG_LAYERS)
                mlp_flop = 8 * N_POINTS * MLP_FLOP_PER_PT
                line["train_step"] = {"samples": 8, "points_per_sample": N_POINTS, "ms_forward_backward": ms_fb,
                                      "ms_step": ms_step, "samples_per_s": 8 / ms_step * 1e3, "dtype": "f32",
                                      "mfma_tflops": 3 * (conv_flop + mlp_flop) / ms_fb / 1e9,
                                      "note": "forward + get_loss + gradient of all 56 variables + TF Adam; "
                                              "python bench.py --workload train [--gpus N] times it as the main line"}
                tr.close()
                del tr
                torch.cuda.empty_cache()
                tb = Trainer(WeightStore.random_init(0, mode="he"), dev, batch_size=8, precision="bf16")
                for _ in range(2):
                    tb.step(tfeed)
                ms_b = ev_time_ms(lambda: tb.step(tfeed), 5, torch)
                line["train_step"]["mixed_precision"] = {
                    "ms_step": ms_b, "samples_per_s": 8 / ms_b * 1e3, "dtype": "bf16",
                    "note": "bf16 multiply (v_mfma_f32_32x32x16_bf16) with fp32 accumulate in the conv / MLP "
                            "forward, data-gradient and 128-tile weight-gradient GEMMs; fp32 activations, "
                            "master weights, gradients and Adam; --workload train --train-dtype bf16"}
                tb.close()
                del tb, tfeed
                torch.cuda.empty_cache()
            except Exception as e:  # the north-star line must survive a failure of this leg
                line["train_step"] = {"error": repr(e)}
        except Exception as e:   # a failing extra must not cost the contract line
            line.setdefault("extras_failed", {})['training step'] = repr(e)
            print("[bench] extra failed: %s: %r" % ('training step', e), file=sys.stderr)
        # ---- CPU baseline: the oracle on the same workload, host cores -----------------------------
        try:
            # The reference's algorithm as written (VGG + five materialised 137x137 up-samples + resampler +
            # unfused MLPs), stage by stage.  The two numpy-bound stages (legacy resize, resampler) are timed
            # through their torch-CPU forms (bit-identical, tests/test_oracle.py) so that they use the host's
            # threads like the conv / MLP stages (MKL / oneDNN) do.
            from oracle import disn_oracle as O
            Wn = store.arrays
            f_img, f_pts, f_tm = img.cpu().numpy(), pts.cpu().numpy(), tm.cpu().numpy()

            # threads of the two numpy-bound resize stages (row blocks on a thread pool; bit-identical to the one-pass
            # form, tests/test_oracle.py); the conv / MLP stages use torch's / BLAS's own pools
            cpu_workers = [min(32, torch.get_num_threads())]

            def cpu_step(stages=None):
                t = [time.perf_counter()]
                resized = O.resize_bilinear_legacy_blocks(f_img, 224, 224, cpu_workers[0]); t.append(time.perf_counter())
                emb, eps = O.vgg16(resized, Wn); t.append(time.perf_counter())
                maps = [O.resize_bilinear_legacy_blocks(np.asarray(eps["vgg_16/%s/%s" % (nm[:5], nm)], np.float32), 137, 137,
                                                        cpu_workers[0])
                        for nm in O.TAP_NAMES]; t.append(time.perf_counter())
                xy = O.get_img_points(f_pts, f_tm)
                feat = np.concatenate([O.resampler_mt(m, xy) for m in maps], axis=2)[:, :, None, :]; t.append(time.perf_counter())
                pred = (O.get_sdf_basic2(f_pts, emb, Wn) + O.get_sdf_basic2_imgfeat_twostream(f_pts, feat, Wn))
                t.append(time.perf_counter())
                if stages is not None:
                    for k, (a_, b_) in zip(("resize_224", "vgg16", "upsample_5_taps", "project_resample", "point_mlps"),
                                           zip(t[:-1], t[1:])):
                        stages.setdefault(k, []).append(b_ - a_)
                return t[-1] - t[0], pred
            _, pred_cpu = cpu_step()
            ts, stages = [], {}
            for _ in range(max(1, args.cpu_runs)):
                ts.append(cpu_step(stages)[0])
            med = float(np.median(ts))
            cpu_name = ""
            try:
                cpu_name = [l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")][0]
            except Exception:
                pass
            nthreads = torch.get_num_threads()
            one = None
            try:   # one-thread figure
                torch.set_num_threads(1)
                cpu_workers[0] = 1
                try:
                    from threadpoolctl import threadpool_limits
                    limiter = threadpool_limits(limits=1)
                except Exception:
                    limiter = None
                one = cpu_step()[0]
                if limiter is not None:
                    limiter.unregister() if hasattr(limiter, "unregister") else limiter.restore_original_limits()
            except Exception:
                pass
            finally:
                torch.set_num_threads(nthreads)
                cpu_workers[0] = min(32, nthreads)
            # parity on He-scaled weights (|pred| ~ 1.7; the xavier set of the timed line gives |pred| ~ 0.02 and says
            # little): the step run alone (conv_h2.hip form) and as image 0 of an SB-image call (conv_h2w.hip form)
            # against the oracle in float64 and in float32
            parity = None
            try:
                st_he = WeightStore.random_init(0, mode="he")
                eng_he = SdfEngine(st_he, dev)
                feed = {"imgs": f_img, "sample_pc": f_pts, "sample_pc_rot": f_pts, "trans_mat": f_tm}
                r64 = O.get_model(feed, st_he.arrays, dtype=np.float64)["pred_sdf"][..., 0]
                r32 = O.get_model(feed, st_he.arrays, dtype=np.float32)["pred_sdf"][..., 0]
                g1 = eng_he.encode_query(img, pts, tm)[1].cpu().numpy()
                nb = max(SB, 4)
                gb = eng_he.encode_query(torch.cat([pool[k % POOL][0] for k in range(nb)]), torch.cat([pool[k % POOL][1] for k in range(nb)]),
                                         torch.cat([pool[k % POOL][2] for k in range(nb)]))[1][:1].cpu().numpy()
                parity = {"weights": "he", "max_abs_pred": float(np.abs(r64).max()),
                          "single_step_form": {"max_abs_gpu_minus_f64": float(np.abs(g1 - r64).max()),
                                               "max_abs_gpu_minus_oracle32": float(np.abs(g1 - r32).max())},
                          "batched_call_form": {"images_per_call": nb, "max_abs_gpu_minus_f64": float(np.abs(gb - r64).max()),
                                                "max_abs_gpu_minus_oracle32": float(np.abs(gb - r32).max())},
                          "max_abs_oracle32_minus_f64": float(np.abs(r32.astype(np.float64) - r64).max()),
                          "bar": "1e-5 absolute against the reference's arithmetic; the float64 oracle is the truth both "
                                 "fp32 implementations (TF CPU / this GPU path) approximate -- two fp32 paths that sum "
                                 "K <= 25088-term dot products in different orders differ by ~1e-5 themselves"}
                del eng_he
                torch.cuda.empty_cache()
            except Exception as e:
                parity = {"error": repr(e)}
            # ... and on the trained-like stress set (heavy-tailed weights, log-normal channel gains, 1 % outlier channels
            # x 1000, demo / white-background images: tests/golden/make_golden_stress.py) against the committed float64
            # oracle run of tests/golden/stress_trained_like.npz -- the statistics the per-image / per-channel power-of-two
            # operand scales exist for (VERDICT r3 #2c)
            parity_tl = None
            try:
                gdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests", "golden")
                sys.path.insert(0, gdir)
                import make_golden_stress as MGS
                gold = np.load(os.path.join(gdir, "stress_trained_like.npz"))
                sin = MGS.stress_inputs()
                eng_tl = SdfEngine(WeightStore(O.trained_like_weights(MGS.STRESS_SEED)), dev)
                td = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                one_f = [float(np.abs(eng_tl.encode_query(td(sin["imgs"][b:b + 1]), td(sin["pts_a"][b:b + 1]),
                                                          td(sin["trans_mat"][b:b + 1]))[1].cpu().numpy().reshape(-1)
                                      - gold["pred64_a"][b]).max()) for b in range(4)]
                pb = eng_tl.encode_query(td(sin["imgs"]), td(sin["pts_a"]), td(sin["trans_mat"]))[1].cpu().numpy()
                bat_f = [float(np.abs(pb[b].reshape(-1) - gold["pred64_a"][b]).max()) for b in range(4)]
                parity_tl = {"weights": "oracle.trained_like_weights(%d)" % MGS.STRESS_SEED,
                             "max_abs_pred": float(np.abs(gold["pred64_a"]).max()),
                             "single_step_form": {"max_abs_gpu_minus_f64_per_image": one_f},
                             "batched_call_form": {"images_per_call": 4, "max_abs_gpu_minus_f64_per_image": bat_f},
                             "worst": max(one_f + bat_f), "bar": 1e-5,
                             "reference": "tests/golden/stress_trained_like.npz (float64 oracle, nothing from the GPU)"}
                del eng_tl
                torch.cuda.empty_cache()
                # ... and a slice of the SWEEP (tests/golden/make_golden_sweep.py: 8 seeds x sigma {1, 1.5, 2} x outliers
                # {1e3, 1e4} x 8 images; tests/test_gpu_sweep.py runs 12 / all 48 sets): three weight sets here, one per
                # sigma, requests one at a time (images 0 and 4) and as one 16-request call -- the DISTRIBUTION of
                # max |gpu - f64| per request, not one worst case (VERDICT r4 #1a)
                import make_golden_sweep as MSW
                gs = np.load(os.path.join(gdir, "stress_sweep.npz"))
                sw = MSW.sweep_inputs()
                errs, per_set = {"single": [], "batch16": [], "strict16": []}, []
                for (seed_, sg_, og_) in ((MSW.SEEDS[2], 1.0, 1e4), (MSW.SEEDS[1], 1.5, 1e3), (MSW.SEEDS[0], 2.0, 1e4)):
                    i_ = MSW.SETS.index((seed_, sg_, og_))
                    eng_s = SdfEngine(WeightStore(O.trained_like_weights(seed_, sigma=sg_, outlier_gain=og_)), dev)
                    e1 = [float(np.abs(eng_s.encode_query(td(sw["imgs"][b:b + 1]), td(sw["pts"][b, 0][None]),
                                                          td(sw["trans_mat"][b:b + 1]))[1][0].cpu().numpy()
                                       - gs["pred64_%02d" % i_][b, 0]).max()) for b in (0, 4)]
                    p16 = eng_s.encode_query(td(np.concatenate([sw["imgs"], sw["imgs"]])),
                                             td(np.concatenate([sw["pts"][:, 0], sw["pts"][:, 1]])),
                                             td(np.concatenate([sw["trans_mat"], sw["trans_mat"]])))[1].cpu().numpy()
                    e16 = [float(np.abs(p16[k] - gs["pred64_%02d" % i_][k % 8, k // 8]).max()) for k in range(16)]
                    eng_st = SdfEngine(None, dev, weights=eng_s.weights, strict=True)
                    ps16 = eng_st.encode_query(td(np.concatenate([sw["imgs"], sw["imgs"]])),
                                               td(np.concatenate([sw["pts"][:, 0], sw["pts"][:, 1]])),
                                               td(np.concatenate([sw["trans_mat"], sw["trans_mat"]])))[1].cpu().numpy()
                    es16 = [float(np.abs(ps16[k] - gs["pred64_%02d" % i_][k % 8, k // 8]).max()) for k in range(16)]
                    del eng_st
                    errs["single"] += e1
                    errs["batch16"] += e16
                    errs["strict16"] += es16
                    per_set.append({"seed": seed_, "sigma": sg_, "outlier_gain": og_,
                                    "channel_gain_span_log2": eng_s.weights.status["max_span_log2"],
                                    "single_worst": max(e1), "batch16_worst": max(e16), "strict16_worst": max(es16),
                                    "oracle32_minus_f64": float(gs["o32_%02d" % i_])})
                    del eng_s
                    torch.cuda.empty_cache()
                dist_ = lambda v: {"n": len(v), "min": float(np.min(v)), "median": float(np.median(v)),
                                   "p90": float(np.sort(v)[int(0.9 * (len(v) - 1))]), "max": float(np.max(v))}
                parity_tl["sweep"] = {"sets": per_set, "single_step_form": dist_(errs["single"]),
                                      "batched_call_form_16": dist_(errs["batch16"]),
                                      "strict_call_form_16": dist_(errs["strict16"]),
                                      "worst": max(errs["single"] + errs["batch16"]), "bar": 1e-5,
                                      "equalised_weights": True,
                                      "reference": "tests/golden/stress_sweep.npz (float64 oracle); the full sweep: "
                                                   "tests/test_gpu_sweep.py, profiles/r06w_sweep_full.json"}
                parity_tl["worst"] = max(parity_tl["worst"], parity_tl["sweep"]["worst"])
            except Exception as e:
                parity_tl = {"error": repr(e)} if parity_tl is None else dict(parity_tl, sweep_error=repr(e))
            best, cores = (N_POINTS / med, nthreads)
            if one and N_POINTS / one > best:
                best, cores = N_POINTS / one, 1
            line["cpu_baseline"] = {"value": best, "unit": "points/s", "cores": cores,
                                    "kind": "port", "seconds_per_step": N_POINTS / best,
                                    "value_all_threads": N_POINTS / med, "threads_all": nthreads,
                                    "stage_seconds_median": {k: float(np.median(v)) for k, v in stages.items()},
                                    "value_1thread": (N_POINTS / one) if one else None,
                                    "max_abs_gpu_minus_cpu_oracle": float(np.abs(out.cpu().numpy() - pred_cpu[..., 0]).max()),
                                    "max_abs_gpu_minus_cpu_oracle_note": "xavier weights of the timed line (|pred| ~ 0.02): see parity_he",
                                    "parity_he": parity,
                                    "parity_trained_like": parity_tl,
                                    "sample": "%d full steps (encode + 2048 points) of the numpy/torch-CPU oracle after "
                                              "1 warm-up, median, with all threads (resize stages: row blocks on a thread pool) and with one: the faster is `value`; "
                                              "nproc=%d; %s" % (len(ts), os.cpu_count(), cpu_name)}
        except Exception as e:   # a failing extra must not cost the contract line
            line.setdefault("extras_failed", {})['CPU baseline'] = repr(e)
            print("[bench] extra failed: %s: %r" % ('CPU baseline', e), file=sys.stderr)
    if rank == 0:
        print(json.dumps(line))
    if launched:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

"""The training driver's data path at the reference's shape (batch 20 x 2048 points), on a synthetic tree of
``--objects`` objects x 32 768 samples x 24 views:

    python tools/train_driver_time.py [--objects 40] [--reps 20] [--out profiles/train_driver_time.json]

  (a) wall time to ONE ready batch on the device, synchronised: the resident set (host index draw + index upload +
      disn_assemble_batch) and the loader (Pt_sdf_img.get_batch + feed_from_batch), warmed, alternating, median and
      spread over ``--reps``; the host draw alone, which both perform
  (b) read + upload time and bytes of the set
  (c) two epochs of ``train_sdf.main`` with each loader: samples/s of the second epoch and the log's `fetch` column
Compare (c) with ``bench.py --workload train --train-batch 20`` (the bare step on synthetic inputs, same shape).
"""
import argparse
import json
import os
import re
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import train_driver_fixtures as TF  # noqa: E402
from disn_amd import data_resident as R, data_sdf as D, train_sdf as T  # noqa: E402


def write_tree(root, n_obj):
    """the tests' synthetic tree (tests/train_driver_fixtures.py) at the reference's sizes: one category, 32 768
    sample rows per object, 24 views"""
    objects = [(TF.CHAIR, "o%03d" % i, 32768, 32768) for i in range(n_obj)]
    info, _ = TF.write_tree(root, objects, views=range(24), seed=0, sphere=True)
    return info, TF.write_lists(root, objects)


def stats(xs):
    xs = np.asarray(xs, np.float64) * 1e3
    return {"median_ms": float(np.median(xs)), "min_ms": float(xs.min()), "max_ms": float(xs.max()), "n": len(xs)}


def epoch_figures(log_path):
    lines = open(log_path).read().splitlines()
    rate = [float(m.group(1)) for l in lines for m in [re.search(r"\| ([0-9.]+) samples/s", l)] if m]
    cols = [(float(m.group(1)), float(m.group(2))) for l in lines
            for m in [re.search(r"\| ([0-9.]+) s/batch, fetch ([0-9.]+) s", l)] if m]
    half = len(cols) // 2                        # the second epoch's lines: the first holds the warm-up
    return {"samples_per_s_epoch": rate, "s_per_batch": float(np.mean([c[0] for c in cols[half:]])),
            "fetch_s_per_batch": float(np.mean([c[1] for c in cols[half:]])), "log_lines": len(cols)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=40)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "train_driver_time.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("train_driver_time.py measures on a HIP device; none is visible")
    B, S = 20, 2048
    root = tempfile.mkdtemp(prefix="train_driver_time_")
    try:
        info, lst = write_tree(root, a.objects)
        listinfo, cats_limit = T.train_listinfo(lst, "chair")
        fl = argparse.Namespace(num_points=1, num_sample_points=S, batch_size=B, img_h=137, img_w=137, rot=False,
                                max_epoch=1, cat_limit=168000, backcolorwhite=False)
        t0 = time.perf_counter()
        rset = R.ResidentSet.from_tree(listinfo, info, workers=8)
        t1 = time.perf_counter()
        rset.to("cuda:0")
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        stream = R.PlanStream(rset, B, 1, S, cats_limit=cats_limit, seed=0)
        loader = D.Pt_sdf_img(fl, listinfo=listinfo, info=info, cats_limit=cats_limit, shuffle=True, seed=0)

        def resident(index):
            rset.assemble(stream.work(index))
            torch.cuda.synchronize()

        def thread(index):
            T.feed_from_batch(loader.work(0, index), "cuda:0")
            torch.cuda.synchronize()

        times = {"resident": [], "loader": [], "host_draw": []}
        for rep in range(-2, a.reps):
            index = (rep + 2) * B % (stream.num_batches * B)
            order = (("resident", resident), ("loader", thread))
            for name, fn in (order if rep % 2 == 0 else order[::-1]):
                t = time.perf_counter()
                fn(index)
                if rep >= 0:
                    times[name].append(time.perf_counter() - t)
            t = time.perf_counter()
            stream.work(index)
            if rep >= 0:
                times["host_draw"].append(time.perf_counter() - t)
        res = {"shape": {"batch": B, "points": S, "objects": a.objects, "samples_per_object": 32768,
                         "views": len(listinfo)},
               "device": torch.cuda.get_device_name(0),
               "ready_batch": {k: stats(v) for k, v in times.items()},
               "set": {"read_s": t1 - t0, "upload_s": t2 - t1, "device_bytes": rset.device_bytes()}}
        rb = res["ready_batch"]
        rb["loader_over_resident"] = rb["loader"]["median_ms"] / rb["resident"]["median_ms"]
        del rset, stream, loader
        torch.cuda.empty_cache()
        res["driver"] = {}
        for which in ("resident", "thread"):
            log_dir = os.path.join(root, "log_" + which)
            T.main(["--category", "chair", "--train_lst_dir", lst, "--sdf_dir", info["sdf_dir"], "--rendered_dir",
                    info["rendered_dir"], "--log_dir", log_dir, "--batch_size", str(B), "--num_sample_points", str(S),
                    "--max_epoch", "2", "--log_every", "8", "--loader", which])
            res["driver"][which] = epoch_figures(os.path.join(log_dir, "log_train.txt"))
    finally:
        shutil.rmtree(root, ignore_errors=True)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return res


if __name__ == "__main__":
    main()

"""The ordered launches of one warmed training step per stream, out of a rocprofv3 kernel trace.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/train_step_launches.py run sdf|cam
    python tools/train_step_launches.py list DIR/.../*_kernel_trace.csv

run: two forward_backward calls of the trainer at B = 2, N = 256, precision f32 (seeded weights and feed).
list: the library's launches (torch's own kernels dropped) per stream in dispatch order as "name grid workgroup"; the
two calls must give the same list, and the second -- the warmed step -- is printed, the busiest stream first.
"""
import csv
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(which):
    import torch
    B, N = 2, 256
    rng = np.random.default_rng(0)
    q = np.linalg.qr(rng.standard_normal((B, 3, 3)))[0]
    RT = np.concatenate([q, np.tile([[-0.0019, 0.0017, 1.39]], (B, 1, 1))], 1).astype(np.float32)
    K = np.array([[149.84375, 0, 68.5], [0, 149.84375, 68.5], [0, 0, 1]], np.float32)
    feed = {"imgs": rng.random((B, 137, 137, 3)), "sample_pc": (rng.random((B, N, 3)) - 0.5) * 0.9, "RT": RT,
            "trans_mat": RT @ K.T, "sdf": 0.05 * rng.standard_normal((B, N, 1))}
    feed = {k: torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda() for k, v in feed.items()}
    feed["sample_pc_rot"] = feed["sample_pc"]
    if which == "sdf":
        from disn_amd.train_sdf import Trainer
        from disn_amd.weights import WeightStore
        tr = Trainer(WeightStore.random_init(0, mode="he"), batch_size=B, precision="f32")
    else:
        from disn_amd.train_cam import CamTrainer, random_init
        tr = CamTrainer(random_init(0), batch_size=B, precision="f32")
    for _ in range(2):
        tr.forward_backward(feed)
        torch.cuda.synchronize()
    tr.close()


def listing(path):
    streams = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = re.sub(r"^void ", "", r["Kernel_Name"]).replace("(anonymous namespace)::", "")
            name = re.sub(r"\(.*$", "", name)
            if "at::" in name:
                continue
            sid = r.get("Stream_Id") or r["Queue_Id"]
            streams.setdefault(sid, []).append((int(r["Dispatch_Id"]), "%s grid %s wg %s" % (
                name.replace("disn::", ""), r.get("Grid_Size_X", r.get("Grid_Size", "")), r.get("Workgroup_Size_X", ""))))
    for i, rows in enumerate(sorted(streams.values(), key=len, reverse=True)):
        rows = [x[1] for x in sorted(rows)]
        half = len(rows) // 2
        if rows[:half] != rows[half:]:
            print("WARNING: the two steps launched differently on this stream (%d launches in all)" % len(rows))
        print("stream %d (%s): %d launches" % (i, "main" if i == 0 else "auxiliary", half))
        for x in rows[half:]:
            print("  " + x)


if __name__ == "__main__":
    run(sys.argv[2]) if sys.argv[1] == "run" else listing(sys.argv[2])

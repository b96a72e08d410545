"""Times of the camera network's training step (disn_cam_train_step) and of its new kernels alone on the GPU.

    python tools/cam_train_time.py [--out FILE] [--quick]

B = 32 images, N = 2048 points (the reference's batch).  Rows: the head part alone (disn_cam_loss_backward: head
forward with saved activations, camera losses, head backward, head weight gradients; device events around
back-to-back calls), the whole step in the fp32-accurate and the mixed-precision mode, and -- the yardstick --
disn_train_step at 8 x 2048 in the same modes, per sample.  --quick: one call of each camera row, no yardstick (a
rocprofv3 workload).
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from disn_amd import ops  # noqa: E402
from disn_amd.posenet import CameraHead, random_init as head_init  # noqa: E402
from disn_amd.train_cam import CamTrainer, random_init  # noqa: E402
from disn_amd.train_sdf import Trainer  # noqa: E402
from disn_amd.weights import WeightStore  # noqa: E402


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters                # ms per call


def cam_feed(B, N, rng):
    q = np.linalg.qr(rng.standard_normal((B, 3, 3)))[0]
    RT = np.concatenate([q, np.tile([[-0.0019, 0.0017, 1.39]], (B, 1, 1))], 1).astype(np.float32)
    K = np.array([[149.84375, 0, 68.5], [0, 149.84375, 68.5], [0, 0, 1]], np.float32)
    f = {"imgs": rng.random((B, 137, 137, 3)), "sample_pc": (rng.random((B, N, 3)) - 0.5) * 0.9, "RT": RT,
         "trans_mat": RT @ K.T}
    return {k: torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda() for k, v in f.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    w, it = (0, 1) if a.quick else (3, 10)
    B, N = 32, 2048
    rng = np.random.default_rng(0)
    feed = cam_feed(B, N, rng)
    lines = ["camera network training timings, MI355X, B = %d, N = %d" % (B, N)]
    head = CameraHead(head_init(0))
    emb = torch.from_numpy(rng.standard_normal((B, 1024)).astype(np.float32)).cuda()
    t_head = timed(lambda: ops.cam_loss_backward(head.w, emb, feed["sample_pc"], feed["RT"], feed["trans_mat"],
                                                 "ALL"), w, it)
    lines.append("head part alone (disn_cam_loss_backward: head forward + losses + head backward + head weight "
                 "gradients, loss_mode ALL): %.3f ms (goal <= 0.15 ms for the new kernels)" % t_head)
    arrays = random_init(0)
    sdf = WeightStore.random_init(0, mode="he")
    for prec in ("f32", "bf16"):
        tr = CamTrainer(arrays, batch_size=B, precision=prec)
        t_step = timed(lambda: tr.forward_backward(feed), w, it)
        t_full = timed(lambda: tr.step(feed), w, it)
        tr.close()
        del tr
        torch.cuda.empty_cache()
        if a.quick:
            lines.append("precision %-4s: camera step %.2f ms" % (prec, t_step))
            continue
        Bs = 8
        st = Trainer(sdf, batch_size=Bs, precision=prec)
        f2 = {"imgs": feed["imgs"][:Bs], "sample_pc": feed["sample_pc"][:Bs], "sample_pc_rot": feed["sample_pc"][:Bs],
              "trans_mat": feed["trans_mat"][:Bs],
              "sdf": torch.rand((Bs, N), device="cuda") * 0.1 - 0.05}
        t_sdf = timed(lambda: st.forward_backward(f2), w, it)
        st.close()
        del st
        torch.cuda.empty_cache()
        lines.append("precision %-4s: camera step %.2f ms = %.3f ms/sample (+ Adam: %.2f ms); disn_train_step at "
                     "%d x %d %.2f ms = %.3f ms/sample (goal: camera <= SDF per sample)"
                     % (prec, t_step, t_step / B, t_full, Bs, N, t_sdf, t_sdf / Bs))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

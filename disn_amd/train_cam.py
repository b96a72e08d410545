"""Training of the camera network -- mirrors cam_est/train_sdf_cam.py of the reference.

  CamTrainer.step     one sess.run([train_op, ...losses]) of train_one_epoch: disn_cam_train_step (VGG-16 +
                      camera head forward, get_loss, gradients of all 50 variables) and tf.train.AdamOptimizer(lr)
                      with TF's defaults (beta1 = 0.9, unlike the SDF trainer's 0.5) over every variable
  learning rate       train_sdf.get_learning_rate (the same staircase decay, floor 1e-6)
  checkpoints         Saver-V2 bundles with the reference's names: vgg_16/*, cameraprediction/*, their Adam /
                      Adam_1 slots, beta1_power, beta2_power (and `batch` with include_step)

    python -m disn_amd.train_cam --category chair --log_dir ckpt/cam          # train
    python -m disn_amd.train_cam --test --restore_model ckpt/cam               # eval: 2-D / 3-D distances
    python -m disn_amd.train_cam --create --restore_model ckpt/cam --img_h5_dir est/   # estimated-camera views

Not supported, with a clear error: --shift, --rotation, --optimizer momentum, multi-GPU gradient exchange.
"""
from __future__ import annotations

import argparse
import os
import sys
import time
from typing import Dict

import numpy as np
import torch

from . import ops, posenet
from .train_common import PRECISIONS, FlatBuffer, TrainerBase
from .train_sdf import adam_step_from_checkpoint, schedule_step_from_checkpoint
from .weights import WeightStore, variable_shapes as sdf_variable_shapes

LOSS_NAMES = ops.CAM_LOSS_NAMES


def variable_shapes() -> Dict[str, tuple]:
    """the 50 variables in disn_cam_param_layout order: 32 vgg_16/* then 18 cameraprediction/*"""
    vgg = [(k, v) for k, v in sdf_variable_shapes().items() if k.startswith("vgg_16/")]
    return dict(vgg + list(posenet.variable_shapes().items()))


VARIABLE_ORDER = tuple(variable_shapes())


def random_init(seed: int = 0) -> Dict[str, np.ndarray]:
    """VGG as WeightStore.random_init, head as posenet.random_init"""
    vgg = WeightStore.random_init(seed).arrays
    out = {k: vgg[k] for k in VARIABLE_ORDER if k.startswith("vgg_16/")}
    out.update(posenet.random_init(seed))
    return out


class FlatCamParams(FlatBuffer):
    """the 50 variables of the camera network in ONE device buffer (disn_cam_param_layout)"""

    def __init__(self, device):
        super().__init__(ops.cam_param_layout(), variable_shapes(), device)

    def from_arrays(self, arrays: Dict[str, np.ndarray]) -> torch.Tensor:
        return self.fill(arrays.get, check=True)


class CamTrainer(TrainerBase):
    def __init__(self, arrays: Dict[str, np.ndarray], device="cuda:0", batch_size: int = 32, base_lr: float = 1e-4,
                 decay_step: int = 200000, decay_rate: float = 0.9, wd: float = 2e-3, loss_mode="3D",
                 beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, precision: str = "f32",
                 optimizer: str = "adam"):
        if optimizer != "adam":
            raise NotImplementedError("only the Adam optimizer is supported (the reference's default)")
        self.loss_mode = ops.cam_loss_mode(loss_mode)
        self._init_state(FlatCamParams(torch.device(device)), arrays.get, True, precision, batch_size, base_lr,
                         decay_step, decay_rate, wd, beta1, beta2, eps)

    def forward_backward(self, feed: Dict[str, torch.Tensor]):
        """gradients into self.grads; -> (pred_trans_mat [B,4,3], losses [7], dists [2,B]) device tensors"""
        B, N = feed["sample_pc"].shape[:2]
        ws = self._fit_ws(ops.lib().disn_cam_train_workspace_bytes(B, N))
        with torch.cuda.device(self.params.device):
            return ops.cam_train_step(self.params, self.grads, feed["imgs"], feed["sample_pc"], feed["RT"],
                                      feed["trans_mat"], self.wd, self.loss_mode, compute_bf16=self.compute_bf16,
                                      ws=ws, ctx=self.ctx)

    def step(self, feed: Dict[str, torch.Tensor]):
        """-> (pred_trans_mat [B,4,3] device, losses dict name -> device scalar, lr)"""
        tm, losses, dists = self.forward_backward(feed)
        lr = self.apply_gradients()
        out = {n: losses[i] for i, n in enumerate(LOSS_NAMES)}
        out["rot2d_dist_all"], out["rot3d_dist_all"] = dists[0], dists[1]
        return tm, out, lr

    def evaluate(self, feed: Dict[str, torch.Tensor]):
        """forward + losses only (the gradients are computed into self.grads and dropped; no update)"""
        return self.forward_backward(feed)

    # ---- checkpoints ----------------------------------------------------------------------
    def save(self, prefix: str, include_step: bool = True) -> None:
        self._save(prefix, include_step, 5)

    def restore(self, prefix: str, prefixes=("",)) -> int:
        """exact-name, exact-shape restore of the variables and their Adam slots whose names start with one of
        `prefixes` ('vgg_16' alone: the reference's --restore_modelcnn; '': everything), then Adam's timestep and the
        schedule step when the bundle carries them; -> #restored"""
        from . import tf_checkpoint as tfc
        arrays = tfc.load_checkpoint(prefix)
        n = self._restore_matching(arrays, slots=True, prefixes=prefixes)
        if "" in prefixes:
            self.adam_t = adam_step_from_checkpoint(arrays, self.beta2, self.adam_t)
            self.step_count = schedule_step_from_checkpoint(arrays)
        return n

    def arrays(self) -> Dict[str, np.ndarray]:
        return self.flat.to_arrays(self.params)


def feed_from_batch(batch_data: Dict[str, np.ndarray], device) -> Dict[str, torch.Tensor]:
    """the feed_dict of train_sdf_cam.py train_one_epoch: imgs = img[..., :3], sample_pc = sdf_pt, RT, trans_mat"""
    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device, non_blocking=True)

    return {"imgs": dev(batch_data["img"][:, :, :, :3]), "sample_pc": dev(batch_data["sdf_pt"]),
            "RT": dev(batch_data["RT"]), "trans_mat": dev(batch_data["trans_mat"])}


# ---- the driver ---------------------------------------------------------------------------------
def parse_args(argv=None):
    p = argparse.ArgumentParser(description="train / test the camera network (cam_est/train_sdf_cam.py)")
    p.add_argument("--gpu", type=str, default="0")
    p.add_argument("--category", default="all")
    p.add_argument("--log_dir", default="checkpoint/sdf_2d_twostream_cam_pcrot_all")
    p.add_argument("--num_points", type=int, default=1)
    p.add_argument("--num_sample_points", type=int, default=2048)
    p.add_argument("--max_epoch", type=int, default=200)
    p.add_argument("--batch_size", type=int, default=32)
    p.add_argument("--img_h", type=int, default=137)
    p.add_argument("--img_w", type=int, default=137)
    p.add_argument("--verbose_freq", type=int, default=100)
    p.add_argument("--learning_rate", type=float, default=1e-4)
    p.add_argument("--momentum", type=float, default=0.9)
    p.add_argument("--optimizer", default="adam")
    p.add_argument("--restore_model", default="")
    p.add_argument("--restore_modelcnn", default="")
    p.add_argument("--rotation", action="store_true")
    p.add_argument("--decay_step", type=int, default=200000)
    p.add_argument("--decay_rate", type=float, default=0.9)
    p.add_argument("--loss_mode", type=str, default="3D")
    p.add_argument("--test", action="store_true")
    p.add_argument("--create", action="store_true")
    p.add_argument("--cat_limit", type=int, default=168000)
    p.add_argument("--img_h5_dir", type=str, default="")
    p.add_argument("--shift", action="store_true")
    p.add_argument("--shift_weight", type=float, default=0.5)
    # storage of this implementation (the reference takes them from its info.json)
    p.add_argument("--sdf_dir", default="")
    p.add_argument("--rendered_dir", default="")
    p.add_argument("--train_lst", default="")
    p.add_argument("--test_lst", default="")
    p.add_argument("--precision", default="f32", choices=tuple(PRECISIONS))
    p.add_argument("--wd", type=float, default=2e-3)
    p.add_argument("--seed", type=int, default=0)
    return p.parse_args(argv)


def check_flags(FLAGS) -> None:
    from .data_cam import check_flags as data_check
    data_check(FLAGS)
    if FLAGS.optimizer != "adam":
        raise NotImplementedError("--optimizer %s is not supported: only adam (the reference's default)" % FLAGS.optimizer)
    if FLAGS.create and not FLAGS.img_h5_dir:
        raise ValueError("--create needs --img_h5_dir")


def _listinfo(path, category):
    out = []
    for line in open(path):
        parts = line.split()
        if len(parts) < 2:
            continue
        cat, obj = parts[0], parts[1]
        views = [int(v) for v in parts[2:]] or list(range(24))
        if category == "all" or cat == category:
            out.extend((cat, obj, v) for v in views)
    return out


def main(argv=None) -> int:
    FLAGS = parse_args(argv)
    check_flags(FLAGS)
    FLAGS.img_feat, FLAGS.rot = True, False
    from .data_cam import Pt_sdf_img_cam, write_estimated_views
    os.makedirs(FLAGS.log_dir, exist_ok=True)
    logf = open(os.path.join(FLAGS.log_dir, "log_train.txt"), "a")

    def log_string(s):
        logf.write(s + "\n")
        logf.flush()
        print(s)

    log_string(str(FLAGS))
    info = {"sdf_dir": FLAGS.sdf_dir, "rendered_dir": FLAGS.rendered_dir}
    trainer = CamTrainer(random_init(FLAGS.seed), batch_size=FLAGS.batch_size, base_lr=FLAGS.learning_rate,
                         decay_step=FLAGS.decay_step, decay_rate=FLAGS.decay_rate, wd=FLAGS.wd,
                         loss_mode=FLAGS.loss_mode, precision=FLAGS.precision, optimizer=FLAGS.optimizer)
    if FLAGS.restore_modelcnn:
        log_string("vgg_16 variables restored: %d" % trainer.restore(FLAGS.restore_modelcnn, ("vgg_16",)))
    if FLAGS.restore_model:
        from . import tf_checkpoint as tfc
        prefix = FLAGS.restore_model
        if os.path.isdir(prefix):
            prefix = tfc.get_checkpoint_state(prefix) or os.path.join(prefix, "latest.ckpt")
        log_string("Model loaded in file: %s (%d tensors)" % (prefix, trainer.restore(prefix)))
    dev = trainer.params.device
    if FLAGS.test or FLAGS.create:
        data = Pt_sdf_img_cam(FLAGS, listinfo=_listinfo(FLAGS.test_lst, FLAGS.category), info=info, shuffle=False)
        n_batches = len(data) // FLAGS.batch_size
        d2, d3 = [], []
        tic = time.time()
        for batch_idx in range(n_batches):
            batch = data.get_batch(batch_idx * FLAGS.batch_size)
            tm, losses, dists = trainer.evaluate(feed_from_batch(batch, dev))
            dist = dists.cpu().numpy()
            d2.extend(dist[0].tolist())
            d3.extend(dist[1].tolist())
            if (batch_idx + 1) % FLAGS.verbose_freq == 0 or batch_idx + 1 == n_batches:
                lv = losses.cpu().numpy()
                log_string(" -- %03d / %03d -- " % (batch_idx + 1, n_batches)
                           + "".join("%s: %f, " % (n, v) for n, v in zip(LOSS_NAMES, lv))
                           + "time: %.02f, " % (time.time() - tic))
                tic = time.time()
            if FLAGS.create:
                for path in write_estimated_views(FLAGS.img_h5_dir, FLAGS.rendered_dir, batch, tm.cpu().numpy()):
                    print("write:", path)
        if d2:
            d2a, d3a = np.asarray(d2), np.asarray(d3)
            print("avg 2d dist {}, max 2d dist {}, min 2d dist {}".format(d2a.mean(), d2a.max(), d2a.min()))
            print("avg 3d dist {}, max 3d dist {}, min 3d dist {}".format(d3a.mean(), d3a.max(), d3a.min()))
        trainer.close()
        return 0

    data = Pt_sdf_img_cam(FLAGS, listinfo=_listinfo(FLAGS.train_lst, FLAGS.category), info=info)
    data.start()
    num_batches = len(data) // FLAGS.batch_size
    try:
        for epoch in range(FLAGS.max_epoch):
            log_string("**** EPOCH %03d ****" % epoch)
            sums = torch.zeros(len(LOSS_NAMES), dtype=torch.float64, device=dev)
            tic = time.time()
            for batch_idx in range(num_batches):
                batch = data.fetch()
                _, losses, lr = trainer.step(feed_from_batch(batch, dev))
                sums += torch.stack([losses[n] for n in LOSS_NAMES]).to(torch.float64)
                if (batch_idx + 1) % 1000 == 0:
                    trainer.save(os.path.join(FLAGS.log_dir, "latest.ckpt"))
                    log_string("Model saved in file: %s" % os.path.join(FLAGS.log_dir, "latest.ckpt"))
                if batch_idx % FLAGS.verbose_freq == 0:
                    w = (sums / FLAGS.verbose_freq).tolist()
                    log_string(" -- %03d / %03d -- " % (batch_idx + 1, num_batches)
                               + "".join("%s: %f, " % (n, v) for n, v in zip(LOSS_NAMES, w))
                               + "time: %.02f, " % (time.time() - tic))
                    sums.zero_()
                    tic = time.time()
            trainer.save(os.path.join(FLAGS.log_dir, "latest.ckpt"))
    finally:
        data.shutdown()
        trainer.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Host side of the training step and the training driver -- mirrors train/train_sdf.py of the reference.

    python -m disn_amd.train_sdf --category chair --train_lst_dir lst/ --sdf_dir sdf/ --rendered_dir img/ \\
        --restore_modelcnn vgg_16.ckpt --log_dir ckpt/sdf --pack_dir pack/         # INTEGRATION.md §4

  get_learning_rate   train/train_sdf.py:153-161 (staircase exponential decay, floor 1e-6)
  Trainer.step        one sess.run([train_op, step, lr, loss, pred_sdf, ...]) of :371-387
  Trainer.save/restore  tf.train.Saver over every global variable whose name lacks 'lr'/'batch'
                      (:285-286): the model variables AND the Adam slots '<var>/Adam', '<var>/Adam_1',
                      'beta1_power', 'beta2_power', as a TF V2 bundle (disn_amd/tf_checkpoint.py)

All device work is the HIP library (disn_train_step / disn_adam_update); data-parallel training is one
process per GPU, each on its own shard of the batch, with ONE sum all-reduce over the flat gradient
buffer (RCCL over xGMI; gloo on CPU tensors is not supported: the path has no CPU fallback) and the
1/world scale folded into the Adam kernel.
"""
from __future__ import annotations

import math
import os
from typing import Dict, Optional

import numpy as np
import torch

from . import ops
from .parallel import GradientReducer
from .train_common import PRECISIONS, FlatBuffer, TrainerBase, get_learning_rate  # noqa: F401  (re-exported)
from .weights import WeightStore, variable_shapes

LOSS_NAMES = ("accuracy", "sdf_loss_realvalue", "sdf_loss", "regularization", "overall_loss")
VARIABLE_ORDER = tuple(variable_shapes())  # == the order of disn_param_layout
HEAD_FIRST_VAR = 26  # vgg_16/fc6/weights: everything from here on is final before the conv backward


class FlatParams(FlatBuffer):
    """the 56 variables of the graph in ONE device buffer (include/disn_amd.h, disn_param_layout)"""

    def __init__(self, device):
        super().__init__(ops.param_layout(), variable_shapes(), device)

    def from_store(self, store: WeightStore) -> torch.Tensor:
        return self.fill(lambda n: store[n])


def adam_step_from_checkpoint(arrays: Dict[str, np.ndarray], beta2: float, current: int = 0,
                              underflow_step: Optional[int] = None) -> int:
    """Adam's timestep t of a restored bundle, from its slot variable beta2_power = beta2^(t+1) -- what a TF restore
    gives the optimizer back (train/train_sdf.py:285-286 saves every global variable except those named 'lr' / 'batch',
    so beta1_power / beta2_power ARE in a reference bundle; TF keeps multiplying them and uses
    lr_t = lr sqrt(1 - beta2_power) / (1 - beta1_power)).  While the power is a usable float32 (t < ~8e4; it goes
    denormal near 8.7e4 steps and reaches 0 near 1.03e5) t is recovered exactly; a power of exactly 0 means the bias
    correction is saturated (lr_t == lr in TF as well): ``underflow_step`` is then returned -- an explicit caller choice;
    None = max(current, 200000), any t at which beta2^t is 0 in the arithmetic of apply_gradients.  No beta2_power in
    the bundle: ``current``."""
    b2 = arrays.get("beta2_power")
    if b2 is not None and 0.0 < float(b2) < 1.0:
        return max(int(round(math.log(float(b2)) / math.log(beta2))) - 1, 0)
    if b2 is not None and float(b2) == 0.0:
        return int(underflow_step) if underflow_step is not None else max(int(current), 200000)
    return int(current)


def schedule_step_from_checkpoint(arrays: Dict[str, np.ndarray]) -> int:
    """the step the learning-rate schedule resumes at.  The reference's Saver leaves `batch` (its global step,
    train/train_sdf.py:232) OUT of every bundle (:285-286: names containing 'lr' or 'batch' are filtered), so a
    restored reference run restarts the schedule at step 0 with lr = base_lr -- and so does this function for a
    reference-written bundle.  A bundle written by Trainer.save(include_step=True) carries `batch` (an extension of
    this implementation, off by default) and resumes there."""
    gs = arrays.get("batch")
    if gs is not None and np.asarray(gs).size == 1:
        return max(int(np.asarray(gs).reshape(())), 0)
    return 0


class Trainer(TrainerBase):
    def __init__(self, store: WeightStore, device="cuda:0", batch_size: int = 20, base_lr: float = 1e-4,
                 decay_step: int = 200000, decay_rate: float = 0.9, wd: float = 1e-5,
                 sdf_weight: float = 10.0, mask_weight: float = 4.0, beta1: float = 0.5,
                 beta2: float = 0.999, eps: float = 1e-8, process_group=None, compute_bf16: bool = False,
                 precision: Optional[str] = None):
        # precision: "f32" (default), "f32_mfma" or "bf16" (TrainerBase._init_state); compute_bf16=True: "bf16"
        if precision is None:
            precision = "bf16" if compute_bf16 else "f32"
        self._init_state(FlatParams(torch.device(device)), lambda n: store[n], False, precision, batch_size,
                         base_lr, decay_step, decay_rate, wd, beta1, beta2, eps)
        self.sdf_weight, self.mask_weight = sdf_weight, mask_weight
        self.pg = process_group
        if process_group is not None or (torch.distributed.is_available() and torch.distributed.is_initialized()):
            self.world = torch.distributed.get_world_size(process_group)
        with torch.cuda.device(self.params.device):
            # gradient exchange: fc + MLP bucket under the convolution backward, conv bucket at the end
            self.reducer = GradientReducer(int(self.flat.layout.offset[HEAD_FIRST_VAR]), process_group)
            self.head_ready = torch.cuda.Event()
            self.head_ready.record()  # creates the hipEvent_t handed to the library

    # ---- one step ---------------------------------------------------------------------
    def reserve_workspace(self, B: int, N: int) -> int:
        """the step's workspace for B samples x N points on this rank, allocated now (the first step would do it);
        -> its size in bytes.  Lets a caller measure the free device memory with the workspace in place."""
        need = ops.lib().disn_train_workspace_bytes(B, N)
        if need == 0:
            raise ValueError("unsupported training shape B=%d N=%d (B*N <= 65536)" % (B, N))
        self._fit_ws(need)
        return need

    def forward_backward(self, feed: Dict[str, torch.Tensor]):
        """gradients of THIS rank's shard into self.grads; -> (pred, losses tensor[5])"""
        B, N = feed["sample_pc"].shape[:2]
        ws = self._fit_ws(ops.lib().disn_train_workspace_bytes(B, N))
        with torch.cuda.device(self.params.device):
            out = ops.train_step(self.params, self.grads, feed["imgs"], feed["trans_mat"], feed["sample_pc"],
                                 feed["sample_pc_rot"], feed["sdf"], self.wd, self.sdf_weight,
                                 self.mask_weight, ws=ws, ctx=self.ctx, head_ready=self.head_ready,
                                 compute_bf16=self.compute_bf16)
            self.reducer.start_head(self.grads, self.head_ready)
        return out

    def step(self, feed: Dict[str, torch.Tensor]):
        """-> (pred [B,N] device, losses dict name -> device scalar, lr)"""
        pred, losses = self.forward_backward(feed)
        lr = self.apply_gradients()
        return pred, {n: losses[i] for i, n in enumerate(LOSS_NAMES)}, lr

    # ---- checkpoints --------------------------------------------------------------------
    def weight_store(self) -> WeightStore:
        return WeightStore(self.flat.to_arrays(self.params))

    def save(self, prefix: str, include_step: bool = False, max_to_keep: int = 5) -> None:
        """variables + Adam slots + beta powers as a TF Saver-V2 bundle with its `checkpoint` state file
        (TrainerBase._save)"""
        self._save(prefix, include_step, max_to_keep)

    def restore(self, prefix: str, underflow_step: Optional[int] = None, prefixes=None) -> int:
        """prefix + exact-shape match, as load_model (train/train_sdf.py:190-219); -> #restored.  Adam's timestep comes
        back from beta2_power (adam_step_from_checkpoint; ``underflow_step`` for a power that underflowed to 0), the
        learning-rate schedule restarts at 0 unless the bundle carries `batch` (schedule_step_from_checkpoint) -- the
        reference's behaviour for its own bundles.
        ``prefixes`` (e.g. ("vgg_16",) for --restore_modelcnn, ("sdfprediction",) for --restore_modelpn): only the
        model variables whose names start with one of them, as load_model's Saver over the matching trainable
        variables -- the Adam slots, Adam's timestep and the schedule are left alone."""
        from . import tf_checkpoint as tfc
        arrays = tfc.load_checkpoint(prefix)
        if prefixes is not None:
            return self._restore_matching(arrays, slots=False, prefixes=prefixes)
        n = self._restore_matching(arrays, slots=True)
        self.adam_t = adam_step_from_checkpoint(arrays, self.beta2, self.adam_t, underflow_step)
        self.step_count = schedule_step_from_checkpoint(arrays)
        if "batch" not in arrays and self.adam_t > 0:
            # the reference's Saver leaves `batch` out (train/train_sdf.py:285-286), so its own resume restarts the
            # learning-rate decay too -- say so instead of doing it silently; save(include_step=True) keeps it
            import warnings
            warnings.warn("restored a bundle without `batch` after %d Adam steps: the learning-rate schedule restarts at "
                          "step 0 (the reference's behaviour); save with include_step=True to carry the step" % self.adam_t)
        return n


def feed_from_batch(batch_data: Dict[str, np.ndarray], device, rank: int = 0, world: int = 1
                    ) -> Dict[str, torch.Tensor]:
    """the feed_dict of train/train_sdf.py:371-378 ('sdf' = sdf_val - 0.003, :375) as device tensors;
    with world > 1 this rank's shard of the batch (parallel.shard_batch)"""
    from .parallel import shard_batch
    B = batch_data["img"].shape[0]
    b0, b1 = shard_batch(B, world, rank) if world > 1 else (0, B)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a[b0:b1], np.float32)).to(device, non_blocking=True)

    return {"imgs": dev(batch_data["img"]), "sample_pc": dev(batch_data["sdf_pt"]),
            "sample_pc_rot": dev(batch_data["sdf_pt_rot"]), "trans_mat": dev(batch_data["trans_mat"]),
            "sdf": dev(batch_data["sdf_val"] - np.float32(0.003))}


def train_one_epoch(trainer: Trainer, dataset, num_batches: int, log=print, log_every: int = 20,
                    rank: int = 0, feed_fn=None) -> Dict[str, float]:
    """train/train_sdf.py:349-440: fetch -> feed -> one optimizer step -> running means of the five
    losses, a log line every `log_every` batches.  Loss scalars stay on the device until a log line
    needs them (one host sync per log line instead of one per batch).
    ``feed_fn(fetched)`` replaces feed_from_batch (the device-resident set: what is fetched is a batch plan)."""
    import time
    sums = torch.zeros(len(LOSS_NAMES), dtype=torch.float64, device=trainer.params.device)
    window = torch.zeros_like(sums)
    fetch_time, tic = 0.0, time.time()
    for batch_idx in range(num_batches):
        t0 = time.time()
        batch_data = dataset.fetch()
        fetch_time += time.time() - t0
        feed = feed_fn(batch_data) if feed_fn is not None else \
            feed_from_batch(batch_data, trainer.params.device, rank, trainer.world)
        _, losses, lr = trainer.step(feed)
        vals = torch.stack([losses[n] for n in LOSS_NAMES]).to(torch.float64)
        sums += vals
        window += vals
        if (batch_idx + 1) % log_every == 0:
            w = (window / log_every).tolist()
            log("batch %d/%d lr %.3g  %s  | %.3f s/batch, fetch %.3f s" % (
                batch_idx + 1, num_batches, lr, "  ".join("%s %.5g" % (n, v) for n, v in zip(LOSS_NAMES, w)),
                (time.time() - tic) / log_every, fetch_time / log_every))
            window.zero_()
            fetch_time, tic = 0.0, time.time()
    means = (sums / max(num_batches, 1)).tolist()
    return dict(zip(LOSS_NAMES, means))


# ---- the driver: python -m disn_amd.train_sdf (train/train_sdf.py of the reference) ------------------------------
LOADERS = ("auto", "resident", "thread")
UNSUPPORTED = ("binary", "threedcnn", "img_feat_onestream", "multi_view", "alpha", "volimp")


def parse_args(argv=None):
    import argparse
    p = argparse.ArgumentParser(prog="python -m disn_amd.train_sdf",
                                description="train the SDF network (train/train_sdf.py)")
    p.add_argument("--gpu", type=str, default="0", help="device index [default: 0]; under torchrun LOCAL_RANK")
    p.add_argument("--category", default="all", help="all, or category names separated by commas [default: all]")
    p.add_argument("--log_dir", default="checkpoint")
    p.add_argument("--num_points", type=int, default=1)
    p.add_argument("--beta1", type=float, default=0.5)
    p.add_argument("--num_sample_points", type=int, default=256)
    p.add_argument("--max_epoch", type=int, default=200)
    p.add_argument("--batch_size", type=int, default=32, help="the GLOBAL batch (all ranks under torchrun)")
    p.add_argument("--learning_rate", type=float, default=1e-4)
    p.add_argument("--optimizer", default="adam")
    p.add_argument("--restore_model", default="", help="checkpoint DIRECTORY to resume from")
    p.add_argument("--restore_modelpn", default="", help="bundle prefix: the sdfprediction variables")
    p.add_argument("--restore_modelcnn", default="", help="bundle prefix: the vgg_16 variables (slim's vgg_16.ckpt)")
    p.add_argument("--train_lst_dir", default="", help="object lists (<cat_id>_train.lst), 24 views per object")
    p.add_argument("--decay_step", type=int, default=200000)
    p.add_argument("--decay_rate", type=float, default=0.9)
    p.add_argument("--mask_weight", type=float, default=4.0)
    p.add_argument("--cat_limit", type=int, default=168000)
    for flag in UNSUPPORTED:
        p.add_argument("--" + flag, action="store_true", help="not supported")
    p.add_argument("--tanh", action="store_true", help="not supported by the training step")
    p.add_argument("--img_feat_twostream", action="store_true", help="the one supported mode (implied)")
    p.add_argument("--augcolorfore", action="store_true", help="accepted; a no-op, as in the reference")
    p.add_argument("--augcolorback", action="store_true", help="accepted; a no-op, as in the reference")
    p.add_argument("--backcolorwhite", action="store_true")
    p.add_argument("--rot", action="store_true")
    p.add_argument("--cam_est", action="store_true", help="--rendered_dir holds the estimated cameras")
    # storage and choices of this implementation (the reference takes the directories from its info.json)
    p.add_argument("--sdf_dir", default="")
    p.add_argument("--rendered_dir", default="")
    p.add_argument("--pack_dir", default="", help="packed copy of the training set: read when it exists, else written")
    p.add_argument("--loader", default="auto", choices=LOADERS,
                   help="resident: the set lives on the device; thread: the reference's loader; auto: resident if it fits")
    p.add_argument("--workers", type=int, default=8, help="file-reading threads of the first pack, at most 16")
    p.add_argument("--precision", default="f32", choices=tuple(PRECISIONS))
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--wd", type=float, default=1e-5)
    p.add_argument("--log_every", type=int, default=20, help="batches per log line")
    return p.parse_args(argv)


def check_flags(FLAGS) -> None:
    """everything that can be refused without a device, a list or a checkpoint"""
    from . import model_normalization as model
    F = model._flags(FLAGS)
    F.img_feat_twostream = True
    F.threedcnn = F.threedcnn or bool(getattr(FLAGS, "volimp", False))   # volimp: a branch of the 3-D CNN model
    model._check_supported(F)
    if FLAGS.tanh:
        raise NotImplementedError("--tanh is not supported: the training step has no tanh output")
    if FLAGS.optimizer != "adam":
        raise NotImplementedError("--optimizer %s is not supported: only adam (the reference's default)" % FLAGS.optimizer)
    if FLAGS.batch_size < 1 or FLAGS.num_sample_points < 1 or FLAGS.max_epoch < 0 or FLAGS.log_every < 1:
        raise ValueError("--batch_size, --num_sample_points and --log_every must be positive")
    if not FLAGS.gpu.isdigit():
        raise ValueError("--gpu takes one device index, got %r" % FLAGS.gpu)
    if not 1 <= FLAGS.workers <= 16:
        raise ValueError("--workers must be in 1..16, got %d" % FLAGS.workers)


def save_decision(epoch: int, avg_accuracy: float, best_acc: float):
    """train/train_sdf.py:322-328 -> (bundle name or None, the new best accuracy): a strictly better mean accuracy
    saves model.ckpt; otherwise every 10th epoch (0 included) saves model_epoch_%03d.ckpt"""
    if avg_accuracy > best_acc:
        return "model.ckpt", avg_accuracy
    if epoch % 10 == 0:
        return "model_epoch_%03d.ckpt" % epoch, best_acc
    return None, best_acc


def train_listinfo(train_lst_dir: str, category: str):
    """:111-130: categories in the order of evaluate.CATS_ALL, 24 views per listed object; -> (listinfo, cats_limit)"""
    from .evaluate import CATS_ALL, categories, read_list
    cats = categories(category)
    listinfo, cats_limit = [], {}
    for cat_nm in CATS_ALL:
        if cat_nm not in cats:
            continue
        cat_id = cats[cat_nm]
        path = os.path.join(train_lst_dir, cat_id + "_train.lst")
        if not os.path.isfile(path):
            raise FileNotFoundError("no training list %s" % path)
        objs = read_list(path)
        cats_limit[cat_id] = 24 * len(objs)
        listinfo += [(cat_id, o.strip(), v) for o in objs for v in range(24)]
    return listinfo, cats_limit


def _bundle(path: str, flag: str) -> str:
    if not os.path.isfile(path + ".index"):
        raise FileNotFoundError("%s: no checkpoint bundle %s(.index)" % (flag, path))
    return path


def choose_loader(want: str, set_bytes: int, free_bytes: int, log=print) -> str:
    """--loader: auto is resident when the set fits into the free device memory, measured by the caller after the
    Trainer and its workspace exist; resident raises where auto would fall back"""
    if want == "thread":
        return "thread"
    if set_bytes <= free_bytes:
        return "resident"
    if want == "resident":
        raise MemoryError("--loader resident: the training set takes %d bytes, %d are free on the device"
                          % (set_bytes, free_bytes))
    log("loader: the training set takes %d bytes, %d are free on the device -> thread loader" % (set_bytes, free_bytes))
    return "thread"


def main(argv=None) -> dict:
    """-> {"loader", "adam_t_start", "history" (the mean losses of every epoch), "saved" (bundle names, rank 0)}"""
    import time
    FLAGS = parse_args(argv)
    check_flags(FLAGS)
    FLAGS.img_h = FLAGS.img_w = 137
    FLAGS.img_feat_twostream = True
    listinfo, cats_limit = train_listinfo(FLAGS.train_lst_dir, FLAGS.category)
    ddp = "RANK" in os.environ and "WORLD_SIZE" in os.environ            # started by torchrun
    world = int(os.environ["WORLD_SIZE"]) if ddp else 1
    rank = int(os.environ["RANK"]) if ddp else 0
    local_rank = int(os.environ.get("LOCAL_RANK", "0")) if ddp else 0
    if FLAGS.batch_size % world:
        raise ValueError("--batch_size %d (the global batch) is not divisible by the world size %d"
                         % (FLAGS.batch_size, world))
    if len(listinfo) < FLAGS.batch_size:
        raise ValueError("%d training views are fewer than one batch of %d" % (len(listinfo), FLAGS.batch_size))
    from . import tf_checkpoint as tfc
    restore_prefix = None
    if FLAGS.restore_modelcnn:
        _bundle(FLAGS.restore_modelcnn, "--restore_modelcnn")
    if FLAGS.restore_modelpn:
        _bundle(FLAGS.restore_modelpn, "--restore_modelpn")
    if FLAGS.restore_model:
        restore_prefix = tfc.get_checkpoint_state(FLAGS.restore_model) if os.path.isdir(FLAGS.restore_model) else None
        if restore_prefix is None:
            raise FileNotFoundError("--restore_model %s holds no checkpoint" % FLAGS.restore_model)
        _bundle(restore_prefix, "--restore_model")
    from . import data_resident as R
    if FLAGS.loader == "thread" or not R.ResidentSet.is_pack(FLAGS.pack_dir):      # a pack replaces the tree
        for d in (FLAGS.sdf_dir, FLAGS.rendered_dir):
            if not os.path.isdir(d):
                raise FileNotFoundError("no data directory %r (--sdf_dir / --rendered_dir)" % d)

    logf = None
    if rank == 0:
        os.makedirs(FLAGS.log_dir, exist_ok=True)
        logf = open(os.path.join(FLAGS.log_dir, "log_train.txt"), "a")

    def log_string(s):
        if logf is not None:
            logf.write(s + "\n")
            logf.flush()
            print(s)

    log_string(str(FLAGS))
    from .data_sdf import Pt_sdf_img
    device = torch.device("cuda", local_rank if ddp else int(FLAGS.gpu))
    torch.cuda.set_device(device)
    own_group = False
    if ddp and not torch.distributed.is_initialized():
        torch.distributed.init_process_group("nccl", device_id=device)
        own_group = True
    trainer = Trainer(WeightStore.random_init(FLAGS.seed), device=device, batch_size=FLAGS.batch_size,
                      base_lr=FLAGS.learning_rate, decay_step=FLAGS.decay_step, decay_rate=FLAGS.decay_rate,
                      wd=FLAGS.wd, mask_weight=FLAGS.mask_weight, beta1=FLAGS.beta1, precision=FLAGS.precision)
    data = None
    result = {"loader": None, "adam_t_start": 0, "history": [], "saved": []}
    try:
        for flag, path, prefix in (("--restore_modelcnn", FLAGS.restore_modelcnn, "vgg_16"),
                                   ("--restore_modelpn", FLAGS.restore_modelpn, "sdfprediction")):
            if path:
                n = trainer.restore(path, prefixes=(prefix,))
                if n == 0:      # the reference would train on from random weights without a word
                    raise ValueError("%s %s holds no %s variable of a matching shape" % (flag, path, prefix))
                log_string("%s variables restored: %d" % (prefix, n))
        if restore_prefix:
            n = trainer.restore(restore_prefix)
            log_string("Model loaded in file: %s (%d tensors, Adam step %d)" % (restore_prefix, n, trainer.adam_t))
        result["adam_t_start"] = trainer.adam_t
        B_local, S = FLAGS.batch_size // world, FLAGS.num_sample_points
        trainer.reserve_workspace(B_local, S)

        info = {"sdf_dir": FLAGS.sdf_dir, "rendered_dir": FLAGS.rendered_dir}
        rset, loader = None, FLAGS.loader
        if loader != "thread":
            tic = time.time()
            if R.ResidentSet.is_pack(FLAGS.pack_dir):
                rset = R.ResidentSet.load(FLAGS.pack_dir)
                if rset.listinfo != listinfo:
                    raise ValueError("--pack_dir %s was packed from another list (%d views, this run has %d)"
                                     % (FLAGS.pack_dir, len(rset.listinfo), len(listinfo)))
                log_string("training set: pack %s mapped in %.2f s" % (FLAGS.pack_dir, time.time() - tic))
            else:
                rset = R.ResidentSet.from_tree(listinfo, info, workers=FLAGS.workers)
                log_string("training set: %d objects, %d views read in %.2f s"
                           % (len(rset.objects), len(rset.listinfo), time.time() - tic))
                if FLAGS.pack_dir and rank == 0:
                    rset.save(FLAGS.pack_dir)
                    log_string("training set: packed into %s" % FLAGS.pack_dir)
            loader = choose_loader(loader, rset.device_bytes(), torch.cuda.mem_get_info(device)[0], log_string)
        if loader == "resident":
            tic = time.time()
            rset.to(device)
            torch.cuda.synchronize(device)
            log_string("loader: resident, %d bytes uploaded in %.3f s" % (rset.device_bytes(), time.time() - tic))
            stream = R.PlanStream(rset, FLAGS.batch_size, FLAGS.num_points, S, cats_limit=cats_limit,
                                  cat_limit=FLAGS.cat_limit, shuffle=True, seed=FLAGS.seed)
            data = R.ResidentLoader(stream, FLAGS.max_epoch)

            def feed_fn(plan):
                return rset.assemble(plan, FLAGS.rot, FLAGS.backcolorwhite, rank, world)
        else:
            rset = None
            log_string("loader: thread")
            data = Pt_sdf_img(FLAGS, listinfo=listinfo, info=info, cats_limit=cats_limit, shuffle=True, seed=FLAGS.seed)
            feed_fn = None
        result["loader"] = loader
        num_batches = data.num_batches
        data.start()
        best_acc = 0.0
        for epoch in range(FLAGS.max_epoch):
            log_string("**** EPOCH %03d ****" % epoch)
            tic = time.time()
            means = train_one_epoch(trainer, data, num_batches, log=log_string, log_every=FLAGS.log_every, rank=rank,
                                    feed_fn=feed_fn)
            if rset is not None:
                rset.raise_on_flags()
            log_string("epoch %03d mean  %s  | %.1f samples/s" % (
                epoch, "  ".join("%s %.5g" % (n, means[n]) for n in LOSS_NAMES),
                num_batches * FLAGS.batch_size / max(time.time() - tic, 1e-9)))
            result["history"].append(means)
            name, best_acc = save_decision(epoch, means["accuracy"], best_acc)
            if name is not None and rank == 0:
                path = os.path.join(FLAGS.log_dir, name)
                trainer.save(path)
                result["saved"].append(name)
                log_string(("best Model saved in file: %s" if name == "model.ckpt" else "Model saved in file: %s") % path)
        if own_group:
            torch.distributed.barrier()
    finally:
        if data is not None:
            data.shutdown()
        trainer.close()
        if own_group:
            torch.distributed.destroy_process_group()
        if logf is not None:
            logf.close()
    return result


if __name__ == "__main__":
    main()

"""What the SDF trainer (train_sdf.Trainer) and the camera trainer (train_cam.CamTrainer) share: the flat parameter
buffer in a library layout, and a trainer base -- precision, the four flat buffers, the concurrency context, the
workspace, the learning-rate schedule, the Adam update and the Saver-V2 checkpoint writing.  Each trainer keeps its
step, its restore contract and its defaults.
"""
from __future__ import annotations

import math
import os
from typing import Dict, Optional

import numpy as np
import torch

from . import ops

PRECISIONS = {"f32_mfma": 0, "bf16": 1, "f32": 2}   # -> compute_bf16 of disn_train_step / disn_cam_train_step
SLOTS = ("", "/Adam", "/Adam_1")                    # suffixes of a variable and its two Adam slots in a bundle


def get_learning_rate(step: int, batch_size: int, base_lr: float = 1e-4, decay_step: int = 200000,
                      decay_rate: float = 0.9) -> float:
    """tf.train.exponential_decay(base, step*batch, decay_step, decay_rate, staircase=True) floored
    at 1e-6 (train/train_sdf.py:153-161; flags :36-40)"""
    return max(base_lr * decay_rate ** ((step * batch_size) // decay_step), 1e-6)


class FlatBuffer:
    """the variables of a network in ONE device buffer: ``layout`` from the library (offset / count per variable, total),
    ``shapes`` name -> shape in the layout's variable order"""

    def __init__(self, layout, shapes: Dict[str, tuple], device):
        self.layout = layout
        self.total = int(layout.total)
        self.device = device
        self.shapes = shapes
        self.index = {n: i for i, n in enumerate(shapes)}

    def _span(self, name: str):
        i = self.index[name]
        return int(self.layout.offset[i]), int(self.layout.count[i])

    def zeros(self) -> torch.Tensor:
        return torch.zeros(self.total, dtype=torch.float32, device=self.device)

    def view(self, buf: torch.Tensor, name: str) -> torch.Tensor:
        o, c = self._span(name)
        return buf[o:o + c].view(self.shapes[name])

    def fill(self, get, check: bool = False) -> torch.Tensor:
        """a new buffer with variable n = get(n); check: ValueError for a missing or mis-shaped one"""
        host = np.zeros(self.total, np.float32)
        for n in self.index:
            a = get(n)
            if check and (a is None or tuple(np.shape(a)) != tuple(self.shapes[n])):
                raise ValueError("variable %s missing or of the wrong shape" % n)
            o, c = self._span(n)
            host[o:o + c] = np.asarray(a, np.float32).reshape(-1)
        return torch.from_numpy(host).to(self.device)

    def to_arrays(self, buf: torch.Tensor, suffix: str = "") -> Dict[str, np.ndarray]:
        host = buf.detach().cpu().numpy()
        out = {}
        for n in self.index:
            o, c = self._span(n)
            out[n + suffix] = host[o:o + c].reshape(self.shapes[n]).copy()
        return out

    def copy_matching(self, buf: torch.Tensor, arrays: Dict[str, np.ndarray], suffix: str = "", prefixes=None) -> int:
        """arrays[name + suffix] into buf for every variable of the same name and exact shape whose name starts with
        one of ``prefixes`` (None: every variable); -> how many were copied"""
        n = 0
        for name in self.index:
            if prefixes is not None and not any(name.startswith(p) for p in prefixes):
                continue
            a = arrays.get(name + suffix)
            if a is not None and tuple(a.shape) == tuple(self.shapes[name]):
                self.view(buf, name).copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))
                n += 1
        return n


class TrainerBase:
    """``reducer`` (parallel.GradientReducer or None) and ``world`` are the data-parallel hook of apply_gradients: the
    gradient exchange is finished before the update and the gradient scaled by 1/world inside the Adam kernel"""
    reducer = None
    world = 1

    def _init_state(self, flat: FlatBuffer, get, check: bool, precision: str, batch_size: int, base_lr: float,
                    decay_step: int, decay_rate: float, wd: float, beta1: float, beta2: float, eps: float) -> None:
        # get, check: the initial values, as FlatBuffer.fill takes them
        # precision of the conv / MLP GEMMs (everything else is fp32 in every mode):
        #   "f32"       fp32-accurate, the reference's precision: forward and data-gradient GEMMs as a
        #               three-term bf16 split on the bf16 MFMA pipes (same error as the f32-input MFMA,
        #               faster), weight gradients on the f32-input MFMA            [default]
        #   "f32_mfma"  every product on the f32-input MFMA
        #   "bf16"      mixed precision: bf16 multiply, fp32 accumulate / master weights / optimizer
        if precision not in PRECISIONS:
            raise ValueError("precision must be one of %s" % (tuple(PRECISIONS),))
        self.precision = precision
        self.compute_bf16 = PRECISIONS[precision]
        self.flat = flat
        self.params = flat.fill(get, check)
        self.grads = flat.zeros()
        self.m = flat.zeros()
        self.v = flat.zeros()
        self.step_count = 0  # the reference's `batch` variable (global step): drives the learning-rate schedule
        self.adam_t = 0      # Adam's timestep (TF keeps it as beta1_power / beta2_power): drives the bias correction
        self.batch_size = batch_size  # GLOBAL batch (all ranks), as the LR schedule counts samples
        self.base_lr, self.decay_step, self.decay_rate = base_lr, decay_step, decay_rate
        self.wd = wd
        self.beta1, self.beta2, self.eps = beta1, beta2, eps
        self._ws: Optional[torch.Tensor] = None
        # every stream / event this object owns lives on params.device, and every launch runs under
        # torch.cuda.device(params.device): ops._stream() is the CURRENT device's current stream
        with torch.cuda.device(self.params.device):
            self.ctx = ops.ctx_create()  # auxiliary stream for the HBM-bound side work of the step

    def close(self) -> None:
        if self.ctx:
            torch.cuda.synchronize(self.params.device)
            with torch.cuda.device(self.params.device):
                ops.ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    def _fit_ws(self, need: int) -> torch.Tensor:
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.params.device)
        return self._ws

    def learning_rate(self) -> float:
        return get_learning_rate(self.step_count, self.batch_size, self.base_lr, self.decay_step, self.decay_rate)

    def apply_gradients(self) -> float:
        lr = self.learning_rate()
        t = self.adam_t + 1
        lr_t = lr * math.sqrt(1.0 - self.beta2 ** t) / (1.0 - self.beta1 ** t)
        with torch.cuda.device(self.params.device):
            if self.reducer is not None:
                self.reducer.finish(self.grads)
            ops.adam_update(self.params, self.grads, self.m, self.v, lr_t, self.beta1, self.beta2, self.eps,
                            1.0 / self.world)
        self.adam_t = t
        self.step_count += 1
        return lr

    # ---- checkpoints --------------------------------------------------------------------
    def state_arrays(self, include_step: bool = False) -> Dict[str, np.ndarray]:
        """what the reference's Saver writes (train/train_sdf.py:285-286): every variable, the Adam slots and the two
        beta powers -- NOT `batch` / the learning rate.  include_step: also `batch` (int32, as TF creates it), an
        extension that lets restore() resume the learning-rate schedule (train_sdf.schedule_step_from_checkpoint)."""
        out = {}
        for buf, suffix in zip((self.params, self.m, self.v), SLOTS):
            out.update(self.flat.to_arrays(buf, suffix))
        out["beta1_power"] = np.asarray(self.beta1 ** (self.adam_t + 1), np.float32)
        out["beta2_power"] = np.asarray(self.beta2 ** (self.adam_t + 1), np.float32)
        if include_step:
            out["batch"] = np.asarray(self.step_count, np.int32)
        return out

    def _save(self, prefix: str, include_step: bool, max_to_keep: int) -> None:
        """state_arrays as a TF Saver-V2 bundle, and the `checkpoint` state file next to it (what saver.save writes,
        train/train_sdf.py:285-286,322-328), so that restore_latest / get_checkpoint_state find it.  The state file
        keeps the last ``max_to_keep`` prefixes in all_model_checkpoint_paths, as tf.train.Saver does (older bundles
        stay on disk here; TF would delete them)."""
        from . import tf_checkpoint as tfc
        tfc.save_checkpoint(prefix, self.state_arrays(include_step))
        d = os.path.dirname(os.path.abspath(prefix))
        base = os.path.basename(prefix)
        paths = [p for p in tfc.all_checkpoint_paths(d) if p != base] + [base]
        tfc.write_checkpoint_state(d, base, paths[-max(1, int(max_to_keep)):])

    def _restore_matching(self, arrays: Dict[str, np.ndarray], slots: bool, prefixes=None) -> int:
        """the variables (slots: and their Adam slots) of a loaded bundle into the buffers; -> how many"""
        bufs = (self.params, self.m, self.v)
        return sum(self.flat.copy_matching(buf, arrays, suffix, prefixes)
                   for buf, suffix in zip(bufs, SLOTS if slots else SLOTS[:1]))

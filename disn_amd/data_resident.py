"""The training set held on the device: one upload, then every batch is built there by one launch.

`data_sdf.Pt_sdf_img` (the reference's loader, data/data_sdf_h5_queue.py) reads two files per sample of every batch.
The whole ShapeNet training set is 16 GB of SDF samples and 55 GB of RGBA views -- a quarter of one MI355X's HBM -- so
`ResidentSet` keeps it there and `disn_assemble_batch` (csrc/batch_assemble.hip) gathers a batch from three small
index arrays.  DESIGN §4t.

  ResidentSet      the arrays (see the class), `from_tree` / `save` / `load` / `to(device)`, `host_batch(plan)` -- the
                   numpy statement of what the kernel computes -- and `assemble(plan)` -- the kernel
  PlanStream       the loader's random stream restated: for a seed, the batches are bit for bit those of
                   `Pt_sdf_img(FLAGS, listinfo, info, cats_limit, shuffle=True, seed=seed)`: the same
                   numpy.random.default_rng(seed) consumed in the same order (epoch shuffle and category quota of
                   `refill_data_order`; per sample `integers(ori_n, size=num_points)` -- the `pc` draw, whose rows
                   nobody reads -- then the `choice` rule; the wrap-around of `get_batch`)
  ResidentLoader   `start` / `fetch` / `shutdown` like the loader thread, but `fetch` gives a BatchPlan drawn one batch
                   ahead on a worker thread

Data parallel: every rank draws the plan of the whole global batch from the same seed and assembles only its
`parallel.shard_batch` slice, so the global batch does not depend on the world size.
"""
from __future__ import annotations

import json
import os
import queue
import threading
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, NamedTuple, Optional, Sequence

import numpy as np

from .data_sdf import _load

IMG = 137
MAX_WORKERS = 16
UPLOAD_CHUNK_BYTES = 256 << 20
_ARRAYS = ("samples", "sample_off", "ori_n", "norm_params", "sdf_params", "img", "trans_mat", "obj_rot_mat",
           "view_obj")


class BatchPlan(NamedTuple):
    entries: np.ndarray     # [B] int32: index into listinfo (= the view index of the set)
    obj_idx: np.ndarray     # [B] int32
    choice: np.ndarray      # [B,S] int32: rows of the object's range

    def shard(self, world: int, rank: int) -> "BatchPlan":
        from .parallel import shard_batch
        b0, b1 = shard_batch(len(self.entries), world, rank)
        return BatchPlan(self.entries[b0:b1], self.obj_idx[b0:b1], self.choice[b0:b1])


class ResidentSet:
    """the training data of a list of (cat_id, obj, view) entries

        samples      float32 [total,4]   the pc_sdf_sample rows of all objects, concatenated
        sample_off   int64   [n_obj+1]   object o owns rows sample_off[o] .. sample_off[o+1]-1 (ragged)
        ori_n        int64   [n_obj]     row count of pc_sdf_original (host; the rows are not kept: Trainer never reads pc)
        norm_params  float32 [n_obj,4]   host            sdf_params  float32 [n_obj,6]   host
        img          uint8   [n_view,137,137,4]          trans_mat   float32 [n_view,4,3]
        obj_rot_mat  float32 [n_view,3,3]                view_obj    int32   [n_view]
    """

    def __init__(self, listinfo: Sequence, objects: Sequence, arrays: Dict[str, np.ndarray]):
        self.listinfo = [(str(c), str(o), int(v)) for c, o, v in listinfo]
        self.objects = [(str(c), str(o)) for c, o in objects]
        missing = [k for k in _ARRAYS if k not in arrays]
        if missing:
            raise KeyError("resident set lacks %s" % missing)
        for k in _ARRAYS:
            setattr(self, k, arrays[k])
        n_obj, n_view = len(self.objects), len(self.listinfo)
        if self.sample_off.shape != (n_obj + 1,) or self.samples.shape != (int(self.sample_off[-1]), 4) \
                or self.img.shape != (n_view, IMG, IMG, 4) or self.view_obj.shape != (n_view,) \
                or self.img.dtype != np.uint8 or self.samples.dtype != np.float32:
            raise ValueError("resident set: the arrays do not fit %d objects and %d views" % (n_obj, n_view))
        self.device = None
        self._dev: Dict[str, "torch.Tensor"] = {}
        self._flags = None

    # ---- construction ---------------------------------------------------------------------------------------------
    @classmethod
    def from_tree(cls, listinfo: Sequence, info: Dict[str, str], workers: int = 8) -> "ResidentSet":
        """reads the files `Pt_sdf_img` reads (`data_sdf._load`: .npz or .h5), each once, on a pool of <= 16 threads.
        The whole set is assembled in host memory (71 GB for the full ShapeNet lists, and the concatenation of the
        sample rows briefly holds them twice: + 16 GB); under torchrun every rank that finds no pack does so.  Pack
        once with a single process (`--pack_dir`), then the ranks memory-map the pack and share the page cache."""
        if not 1 <= workers <= MAX_WORKERS:
            raise ValueError("workers must be in 1..%d, got %d" % (MAX_WORKERS, workers))
        listinfo = [(c, o, int(v)) for c, o, v in listinfo]
        if len(set(listinfo)) != len(listinfo):
            raise ValueError("the list names a view twice")
        objects: List = list(dict.fromkeys((c, o) for c, o, _ in listinfo))
        obj_of = {k: i for i, k in enumerate(objects)}
        n_view = len(listinfo)

        def load_obj(key):
            cat_id, obj = key
            d = _load(os.path.join(info["sdf_dir"], cat_id, obj, "ori_sample.h5"),
                      ("pc_sdf_original", "pc_sdf_sample", "norm_params", "sdf_params"))
            if not all(k in d for k in ("pc_sdf_original", "pc_sdf_sample", "norm_params", "sdf_params")):
                raise Exception(cat_id, obj, "no sdf and sample")
            smp = np.ascontiguousarray(d["pc_sdf_sample"], np.float32)
            if smp.ndim != 2 or smp.shape[1] != 4 or smp.shape[0] < 1:
                raise ValueError("%s/%s: pc_sdf_sample must be [m,4], got %s" % (cat_id, obj, smp.shape))
            return smp, int(d["pc_sdf_original"].shape[0]), np.asarray(d["norm_params"], np.float32).reshape(4), \
                np.asarray(d["sdf_params"], np.float32).reshape(6)

        img = np.empty((n_view, IMG, IMG, 4), np.uint8)
        trans_mat = np.empty((n_view, 4, 3), np.float32)
        rot = np.empty((n_view, 3, 3), np.float32)

        def load_view(i):
            cat_id, obj, num = listinfo[i]
            d = _load(os.path.join(info["rendered_dir"], cat_id, obj, "%02d.h5" % num),
                      ("img_arr", "trans_mat", "obj_rot_mat"))
            raw = d["img_arr"]
            if raw.dtype != np.uint8 or raw.shape[:2] != (IMG, IMG) or raw.shape[2] not in (3, 4):
                raise ValueError("%s/%s/%02d: img_arr must be uint8 [%d,%d,4], got %s %s"
                                 % (cat_id, obj, num, IMG, IMG, raw.dtype, raw.shape))
            img[i, :, :, :raw.shape[2]] = raw
            if raw.shape[2] == 3:
                img[i, :, :, 3] = 255          # no alpha: nothing is background, as in Pt_sdf_img.get_img
            trans_mat[i] = d["trans_mat"]
            rot[i] = d["obj_rot_mat"]

        with ThreadPoolExecutor(max_workers=workers) as ex:
            objs = list(ex.map(load_obj, objects))
            list(ex.map(load_view, range(n_view)))
        counts = np.array([o[0].shape[0] for o in objs], np.int64)
        arrays = {"samples": np.concatenate([o[0] for o in objs], 0),
                  "sample_off": np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
                  "ori_n": np.array([o[1] for o in objs], np.int64),
                  "norm_params": np.stack([o[2] for o in objs]), "sdf_params": np.stack([o[3] for o in objs]),
                  "img": img, "trans_mat": trans_mat, "obj_rot_mat": rot,
                  "view_obj": np.array([obj_of[(c, o)] for c, o, _ in listinfo], np.int32)}
        return cls(listinfo, objects, arrays)

    def save(self, directory: str) -> None:
        """flat .npy files + index.json: a later run memory-maps them instead of parsing every small file again.
        The index is what makes a directory a pack (`is_pack`): it is written last, under a temporary name, and
        renamed into place, so another process never sees a pack whose files are still being written."""
        os.makedirs(directory, exist_ok=True)
        for k in _ARRAYS:
            np.save(os.path.join(directory, k + ".npy"), np.asarray(getattr(self, k)))
        tmp = os.path.join(directory, "index.json.%d.tmp" % os.getpid())
        with open(tmp, "w") as f:
            json.dump({"format": 1, "listinfo": self.listinfo, "objects": self.objects,
                       "arrays": {k: [str(getattr(self, k).dtype), list(getattr(self, k).shape)] for k in _ARRAYS}}, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, os.path.join(directory, "index.json"))

    @classmethod
    def load(cls, directory: str) -> "ResidentSet":
        with open(os.path.join(directory, "index.json")) as f:
            index = json.load(f)
        if index.get("format") != 1:
            raise ValueError("%s: unknown pack format %r" % (directory, index.get("format")))
        arrays = {}
        for k, (dtype, shape) in index["arrays"].items():
            a = np.load(os.path.join(directory, k + ".npy"), mmap_mode="r")
            if str(a.dtype) != dtype or list(a.shape) != shape:
                raise ValueError("%s/%s.npy is %s %s, the index says %s %s" % (directory, k, a.dtype, a.shape, dtype, shape))
            arrays[k] = a
        return cls([tuple(e) for e in index["listinfo"]], [tuple(o) for o in index["objects"]], arrays)

    @staticmethod
    def is_pack(directory: str) -> bool:
        return bool(directory) and os.path.isfile(os.path.join(directory, "index.json"))

    # ---- the device copy ------------------------------------------------------------------------------------------
    _DEVICE_ARRAYS = ("samples", "sample_off", "img", "trans_mat", "obj_rot_mat")

    def device_bytes(self) -> int:
        return int(sum(getattr(self, k).nbytes for k in self._DEVICE_ARRAYS))

    def to(self, device, chunk_bytes: int = UPLOAD_CHUNK_BYTES) -> "ResidentSet":
        """upload, at most `chunk_bytes` of host staging at a time (the host arrays may be memory maps)"""
        import torch
        self.device = torch.device(device)
        for k in self._DEVICE_ARRAYS:
            a = getattr(self, k)
            t = torch.empty(a.shape, dtype=getattr(torch, str(a.dtype)), device=self.device)
            rows = max(1, chunk_bytes // max(1, a.nbytes // max(1, a.shape[0])))
            for r0 in range(0, a.shape[0], rows):
                t[r0:r0 + rows].copy_(torch.from_numpy(np.array(a[r0:r0 + rows])))
            self._dev[k] = t
        self._flags = torch.zeros(1, dtype=torch.int32, device=self.device)
        return self

    def check_plan(self, plan: BatchPlan) -> None:
        cnt = (self.sample_off[1:] - self.sample_off[:-1])[plan.obj_idx]
        if plan.entries.min() < 0 or plan.entries.max() >= len(self.listinfo) or plan.choice.min() < 0 \
                or (plan.choice >= cnt[:, None]).any():
            raise IndexError("batch plan points outside the resident set")

    def assemble(self, plan: BatchPlan, rot: bool = False, backcolorwhite: bool = False, rank: int = 0, world: int = 1):
        """the feed of Trainer.step for this rank's slice of the plan: one upload of the indices, one launch"""
        import torch

        from . import ops
        if not self._dev:
            raise RuntimeError("the set is not on a device: call .to(device) first")
        if world > 1:
            plan = plan.shard(world, rank)
        self.check_plan(plan)
        B, S = plan.choice.shape
        idx = torch.from_numpy(np.concatenate([plan.obj_idx, plan.entries, plan.choice.reshape(-1)]).astype(np.int32))
        idx = idx.to(self.device, non_blocking=True)
        d = self._dev
        with torch.cuda.device(self.device):
            return ops.assemble_batch(d["samples"], d["sample_off"], d["img"], d["trans_mat"], d["obj_rot_mat"],
                                      idx[:B], idx[B:2 * B], idx[2 * B:].view(B, S), self._flags, rot, backcolorwhite)

    def raise_on_flags(self) -> None:
        """one host sync: the kernel's own range check (check_plan makes it unreachable from assemble)"""
        if self._flags is not None and int(self._flags.item()):
            raise IndexError("disn_assemble_batch met an index outside the resident set")

    # ---- the same batch in numpy ----------------------------------------------------------------------------------
    def host_batch(self, plan: BatchPlan, rot: bool = False, backcolorwhite: bool = False) -> Dict:
        """the dictionary `Pt_sdf_img.get_batch` gives for this plan (without `pc`), from the held arrays"""
        B, S = plan.choice.shape
        out = {"sdf_pt": np.zeros((B, S, 3), np.float32), "sdf_pt_rot": np.zeros((B, S, 3), np.float32),
               "sdf_val": np.zeros((B, S, 1), np.float32), "norm_params": np.zeros((B, 4), np.float32),
               "sdf_params": np.zeros((B, 6), np.float32), "img": np.zeros((B, IMG, IMG, 3), np.float32),
               "trans_mat": np.zeros((B, 4, 3), np.float32), "cat_id": [], "obj_nm": [], "view_id": []}
        self.check_plan(plan)
        for b in range(B):
            e, o = int(plan.entries[b]), int(plan.obj_idx[b])
            rows = np.asarray(self.samples[int(self.sample_off[o]) + plan.choice[b].astype(np.int64)])
            pts = np.ascontiguousarray(rows[:, :3])
            out["sdf_pt"][b] = pts
            out["sdf_val"][b, :, 0] = rows[:, 3]
            out["sdf_pt_rot"][b] = pts @ np.asarray(self.obj_rot_mat[e]) if rot else pts
            raw = np.asarray(self.img[e])
            img = raw[:, :, :3].astype(np.float32)
            if backcolorwhite:
                img[raw[:, :, 3] == 0] = 255.0
            out["img"][b] = np.clip(img, 0, 255) / np.float32(255.0)
            out["trans_mat"][b] = self.trans_mat[e]
            out["norm_params"][b] = self.norm_params[o]
            out["sdf_params"][b] = self.sdf_params[o]
            cat_id, obj, num = self.listinfo[e]
            out["cat_id"].append(cat_id)
            out["obj_nm"].append(obj)
            out["view_id"].append(num)
        return out


class PlanStream:
    """`Pt_sdf_img`'s order and draws (data_sdf.py: set_cat_limit, refill_data_order, work, get_batch) without its
    file reads: `work(index)` is the BatchPlan of the batch `Pt_sdf_img.work(epoch, index)` returns"""

    def __init__(self, rset: ResidentSet, batch_size: int, num_points: int, num_sample_points: int, cats_limit=None,
                 cat_limit: Optional[int] = None, shuffle: bool = True, seed=None):
        self.rset = rset
        self.batch_size, self.num_points, self.gen_num_pt = batch_size, num_points, num_sample_points
        self.listinfo = rset.listinfo
        self.data_num = len(self.listinfo)
        self.num_batches = self.data_num // batch_size
        self.shuffle = shuffle
        if cats_limit is None:
            cats_limit = {}
            for cat_id, _, _ in self.listinfo:
                cats_limit[cat_id] = cats_limit.get(cat_id, 0) + 1
        self.cats_limit = dict(cats_limit)
        self.epoch_amount = 0
        for cat in self.cats_limit:
            if cat_limit is not None:
                self.cats_limit[cat] = min(cat_limit, self.cats_limit[cat])
            self.epoch_amount += self.cats_limit[cat]
        self.data_order = list(range(self.data_num))
        self.order = self.data_order
        self.rng = np.random.default_rng(seed)
        self._count = np.asarray(rset.sample_off[1:] - rset.sample_off[:-1])
        self._ori_n = np.asarray(rset.ori_n)
        self._view_obj = np.asarray(rset.view_obj)

    def __len__(self):
        return self.epoch_amount

    def refill_data_order(self):
        order = list(self.data_order)
        self.rng.shuffle(order)
        quota = dict(self.cats_limit)
        epoch_order = []
        for idx in order:
            if len(epoch_order) >= self.epoch_amount:
                break
            cat_id = self.listinfo[idx][0]
            if quota.get(cat_id, 0) > 0:
                epoch_order.append(idx)
                quota[cat_id] -= 1
        return epoch_order

    def work(self, index: int) -> BatchPlan:
        if index == 0 and self.shuffle:
            self.order = self.refill_data_order()
        B, S = self.batch_size, self.gen_num_pt
        if index + B > self.epoch_amount:
            index = index + B - self.epoch_amount
        entries = np.array([self.order[i] for i in range(index, index + B)], np.int32)
        obj_idx = self._view_obj[entries].astype(np.int32)
        choice = np.empty((B, S), np.int32)
        for b in range(B):
            o = int(obj_idx[b])
            self.rng.integers(int(self._ori_n[o]), size=self.num_points)       # the loader's `pc` draw
            n = int(self._count[o])
            choice[b] = self.rng.integers(n, size=S) if S > n else self.rng.choice(n, size=S, replace=False)
        return BatchPlan(entries, obj_idx, choice)


class ResidentLoader(threading.Thread):
    """`Pt_sdf_img`'s thread contract over a PlanStream: the host draws of batch k+1 run while batch k trains.
    `run` / `shutdown` repeat `Pt_sdf_img`'s on purpose (that class mirrors the reference and stays as it is); `fetch`
    differs on purpose: an exception of the producer is re-raised here, and the end of the stream raises instead of
    blocking for ever -- keep the two in step except for that."""

    def __init__(self, stream: PlanStream, max_epoch: int, ahead: int = 1):
        super().__init__(daemon=True)
        self.stream = stream
        self.max_epoch = max_epoch
        self.queue: "queue.Queue" = queue.Queue(max(1, ahead))
        self.stopped = False
        self.bno = 0
        self.num_batches = stream.num_batches
        self.error: Optional[BaseException] = None

    def __len__(self):
        return len(self.stream)

    def run(self):
        per_epoch = self.num_batches * self.stream.batch_size
        try:
            while per_epoch > 0 and (self.bno // per_epoch) < self.max_epoch and not self.stopped:
                plan = self.stream.work(self.bno % per_epoch)
                while not self.stopped:
                    try:
                        self.queue.put(plan, timeout=0.2)
                        break
                    except queue.Full:
                        continue
                self.bno += self.stream.batch_size
        except BaseException as e:          # surfaces in fetch(): a dead producer must not look like a slow one
            self.error = e

    def fetch(self, timeout: Optional[float] = None):
        if self.stopped:
            return None
        while True:
            try:
                return self.queue.get(timeout=0.2 if timeout is None else min(timeout, 0.2))
            except queue.Empty:
                if self.error is not None:
                    raise self.error
                if not self.is_alive() and self.queue.empty():
                    raise RuntimeError("the plan stream has ended")
                if timeout is not None:
                    timeout -= 0.2
                    if timeout <= 0:
                        raise

    def shutdown(self):
        self.stopped = True
        while not self.queue.empty():
            try:
                self.queue.get_nowait()
            except queue.Empty:
                break

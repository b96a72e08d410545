"""Training-data loader of the camera network -- host mirror of data/data_sdf_h5_queue_mask_imgh5_cammat.py.

The batch of data_sdf.Pt_sdf_img (same sources, epoch order and point sampling), with the camera schema of the
reference's cammat loader (get_img :161-180, get_batch :232-335):

    img [B,H,W,4]  (RGBA / 255: all four channels; the network takes img[..., :3])
    RT [B,4,3]     the view file's `regress_mat`
    shifts [B,2]   zeros (--shift is not supported, see below)

and every view file must carry `K` [3,3] (the reference reads it and fails without it).  Files are `.npz` with the
same keys next to (or instead of) the reference's `.h5`, as in data_sdf.py; `save_view_cam` writes one, `K` included
(data_sdf.save_view keeps writing what it always wrote).

Not supported, with a clear error: FLAGS.shift (the reference's camera model calls a posenet function that does not
exist) and FLAGS.rotation (it needs the renderer's rendering_metadata.txt, and the camera losses never read
sample_pc_rot).
"""
from __future__ import annotations

import os

import numpy as np

from .data_sdf import Pt_sdf_img, _load


def check_flags(FLAGS) -> None:
    if getattr(FLAGS, "shift", False):
        raise NotImplementedError("--shift is not supported: the reference's camera model calls "
                                  "posenet.get_cam_mat_shft, which does not exist")
    if getattr(FLAGS, "rotation", False):
        raise NotImplementedError("--rotation is not supported: it needs the renderer's rendering_metadata.txt, and "
                                  "the camera losses never read sample_pc_rot")


def save_view_cam(rendered_dir: str, cat_id: str, obj: str, num: int, img_arr, trans_mat, obj_rot_mat, regress_mat,
                  K, RT=None):
    """a view file for the camera loader: data_sdf.save_view's keys plus K (and RT when given)"""
    d = os.path.join(rendered_dir, cat_id, obj)
    os.makedirs(d, exist_ok=True)
    arrays = dict(img_arr=np.asarray(img_arr, np.uint8), trans_mat=np.asarray(trans_mat, np.float32),
                  obj_rot_mat=np.asarray(obj_rot_mat, np.float32), regress_mat=np.asarray(regress_mat, np.float32),
                  K=np.asarray(K, np.float32))
    if RT is not None:
        arrays["RT"] = np.asarray(RT, np.float32)
    path = os.path.join(d, "%02d.npz" % num)
    np.savez(path, **arrays)
    return path


class Pt_sdf_img_cam(Pt_sdf_img):
    """data_sdf.Pt_sdf_img with the cammat loader's batch schema"""

    def __init__(self, FLAGS, *args, **kwargs):
        check_flags(FLAGS)
        super().__init__(FLAGS, *args, **kwargs)

    def get_img_cam(self, img_dir, num):
        d = _load(os.path.join(img_dir, "%02d.h5" % num),
                  ("img_arr", "trans_mat", "obj_rot_mat", "regress_mat", "K"))
        for k in ("img_arr", "trans_mat", "regress_mat", "K"):
            if k not in d:
                raise KeyError("%s/%02d: view file has no '%s'" % (img_dir, num, k))
        img = d["img_arr"][:, :, :4].astype(np.float32) / np.float32(255.0)
        return img, d["trans_mat"].astype(np.float32), d["regress_mat"].astype(np.float32)

    def get_batch(self, index):
        out = super().get_batch(index)
        B = self.batch_size
        out["img"] = np.zeros((B, self.FLAGS.img_h, self.FLAGS.img_w, 4), np.float32)
        out["RT"] = np.zeros((B, 4, 3), np.float32)
        out["shifts"] = np.zeros((B, 2), np.float32)
        for cnt, (cat_id, obj, num) in enumerate(zip(out["cat_id"], out["obj_nm"], out["view_id"])):
            img, trans_mat, RT = self.get_img_cam(os.path.join(self.img_dir, cat_id, obj), num)
            out["img"][cnt, :, :, :img.shape[2]] = img
            out["trans_mat"][cnt] = trans_mat
            out["RT"][cnt] = RT
        return out


def write_estimated_views(img_h5_dir: str, rendered_dir: str, batch, pred_trans_mat) -> list:
    """cam_est/train_sdf_cam.py create_img_h5: for every sample of the batch copy its view file's img_arr, K, RT,
    obj_rot_mat and regress_mat to <img_h5_dir>/<cat>/<obj>/%02d with trans_mat = the PREDICTED camera.  The files
    are what data_sdf.Pt_sdf_img reads, so create_sdf / evaluate run on estimated cameras unchanged."""
    pred = np.asarray(pred_trans_mat, np.float32)
    written = []
    for i, (cat_id, obj, num) in enumerate(zip(batch["cat_id"], batch["obj_nm"], batch["view_id"])):
        src = _load(os.path.join(rendered_dir, cat_id, obj, "%02d.h5" % num),
                    ("img_arr", "K", "RT", "obj_rot_mat", "regress_mat"))
        written.append(save_view_cam(img_h5_dir, cat_id, obj, num, src["img_arr"], pred[i], src["obj_rot_mat"],
                                     src["regress_mat"], src["K"], src.get("RT")))
    return written

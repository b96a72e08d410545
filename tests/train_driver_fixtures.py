"""A synthetic training tree in the reference's directory layout, written with data_sdf.save_sample / save_view:
two categories, objects with more and with fewer samples than a batch asks for, several views per object, RGBA
images with alpha-0 pixels, a rotation per view.  Shared by test_train_driver_host.py and test_gpu_train_driver.py."""
import os
import types

import numpy as np

from disn_amd import data_sdf as D

CHAIR, CAR = "03001627", "02958343"
# a camera of the reference's renderings (oracle.disn_oracle.DEMO_TRANS_MAT[0]): the points project into the image
TRANS_MAT = np.array([[-68.453156, 5.5086656, -0.37556022], [-17.138561, -84.685486, -0.250198],
                      [-47.284092, -3.6569588, 0.2493176], [101.133705, 101.34268, 1.4305686]], np.float32)


def _rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q.astype(np.float32)


def write_tree(root, objects, views, seed=0, sphere=False):
    """objects: [(cat_id, name, n_samples, n_original)]; views: the view numbers every object gets.
    -> (info, listinfo) with listinfo in object-major order, as train/train_sdf.py:123-130 builds it"""
    rng = np.random.default_rng(seed)
    info = {"sdf_dir": os.path.join(str(root), "sdf"), "rendered_dir": os.path.join(str(root), "img")}
    listinfo = []
    for cat_id, name, n_smp, n_ori in objects:
        def cloud(n):
            pts = rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
            val = np.linalg.norm(pts, axis=1, keepdims=True) - 0.3 if sphere else rng.normal(0, 0.1, (n, 1))
            return np.concatenate([pts, val], 1).astype(np.float32)
        D.save_sample(info["sdf_dir"], cat_id, name, cloud(n_ori), cloud(n_smp), rng.normal(size=4),
                      [-1, -1, -1, 1, 1, 1] + rng.normal(0, 0.01, 6))
        for v in views:
            img = rng.integers(0, 256, (137, 137, 4), dtype=np.uint8)
            img[rng.random((137, 137)) < 0.3, 3] = 0            # background pixels: alpha 0, colour arbitrary
            tm = TRANS_MAT + rng.normal(0, 0.01, (4, 3)).astype(np.float32)
            D.save_view(info["rendered_dir"], cat_id, name, v, img, tm, _rotation(rng), tm)
            listinfo.append((cat_id, name, v))
    return info, listinfo


def write_lists(root, objects):
    d = os.path.join(str(root), "lst")
    os.makedirs(d, exist_ok=True)
    per_cat = {}
    for cat_id, name, _, _ in objects:
        per_cat.setdefault(cat_id, []).append(name)
    for cat_id, names in per_cat.items():
        with open(os.path.join(d, cat_id + "_train.lst"), "w") as f:
            f.write("\n".join(names) + "\n")
    return d


def flags(batch_size, num_sample_points, num_points=1, rot=False, backcolorwhite=False, cat_limit=168000, max_epoch=2):
    return types.SimpleNamespace(num_points=num_points, num_sample_points=num_sample_points, batch_size=batch_size,
                                 img_h=137, img_w=137, rot=rot, max_epoch=max_epoch, cat_limit=cat_limit,
                                 backcolorwhite=backcolorwhite, alpha=False)


SMALL_OBJECTS = [(CHAIR, "a0", 300, 50), (CHAIR, "a1", 40, 70), (CAR, "c0", 64, 20), (CAR, "c1", 500, 90),
                 (CHAIR, "a2", 65, 33)]

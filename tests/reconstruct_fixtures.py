"""Shared inputs of tests/test_reconstruct_host.py and tests/test_gpu_reconstruct.py (not a test module)."""
import os
import random

import numpy as np

CATS = (("chair", "03001627"), ("car", "02958343"))        # in the order of evaluate.CATS_ALL
OBJS = {"03001627": ["obj_a", "obj_b"], "02958343": ["obj_c", "obj_d"]}


def sphere(R, r=0.6, c=(0.05, -0.1, 0.02)):
    ax = np.linspace(-1, 1, R + 1)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    return (np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r).astype(np.float32)


def noise(R, seed):
    v = np.random.default_rng(seed).standard_normal((R + 1,) * 3).astype(np.float32)
    v[0] = v[-1] = 1; v[:, 0] = v[:, -1] = 1; v[:, :, 0] = v[:, :, -1] = 1     # outside shell -> closed surface
    return v


def mc_batch_grids(R=20):
    """[(name, volume [n,n,n], box [6], empty?)] x 6: three noise grids, an off-centre sphere, an all-positive
    (empty) grid BETWEEN non-empty ones, and a sphere pushed through the last x and z planes (cut edges ON the
    planes ix = R and iz = R, where the +1 / +n^2 neighbours of a point do not exist)"""
    vols = [("noise0", noise(R, 0), False), ("sphere_off", sphere(R, 0.55, (0.3, -0.25, 0.1)), False),
            ("all_positive", np.ones((R + 1,) * 3, np.float32), True), ("noise1", noise(R, 1), False),
            ("sphere_last_plane", sphere(R, 0.6, (0.55, 0.0, 0.5)), False), ("noise2", noise(R, 2), False)]
    out = []
    for b, (name, vol, empty) in enumerate(vols):
        box = [-1.0 - 0.1 * b, -1.0, -0.5 - 0.05 * b, 1.0 + 0.2 * b, 1.25, 0.5 + 0.1 * b]     # anisotropic, per grid
        out.append((name, vol, box, empty))
    return out


def expected_entries(seed, view_num, cats=CATS, objs=OBJS, num_shards=1, shard_id=0):
    """the documented sample list, restated: categories in CATS_ALL order, objects in list order, per object
    sorted(Random(seed).sample(range(24), view_num)) from one generator; shards take objects[shard_id::num_shards]"""
    rng = random.Random(seed)
    objects = []
    for _, cat_id in cats:
        for obj in objs[cat_id]:
            objects.append((cat_id, obj, sorted(rng.sample(range(24), view_num))))
    return [(c, o, v) for c, o, views in objects[shard_id::num_shards] for v in views]


def write_lists(lst_dir, cats=CATS, objs=OBJS):
    os.makedirs(lst_dir, exist_ok=True)
    for _, cat_id in cats:
        with open(os.path.join(lst_dir, cat_id + "_test.lst"), "w") as f:
            f.write("\n".join(objs[cat_id]) + "\n")


def build_dataset(root, entries, n_samples=512, seed=11):
    """sdf_dir / rendered_dir with one ori_sample per object and one view file per entry (data_sdf.save_*)"""
    from disn_amd import data_sdf
    from oracle import disn_oracle as O
    rng = np.random.default_rng(seed)
    sdf_dir, rendered_dir = os.path.join(root, "sdf"), os.path.join(root, "views")
    seen = {}
    for k, (cat_id, obj, view) in enumerate(entries):
        if (cat_id, obj) not in seen:
            j = len(seen)
            pts = (rng.random((n_samples, 3), dtype=np.float32) * 1.6 - 0.8).astype(np.float32)
            val = (np.linalg.norm(pts - np.float32(0.05 * j), axis=1) - np.float32(0.5)).astype(np.float32)
            smp = np.concatenate([pts, val[:, None]], axis=1)
            box = [-1.0 - 0.05 * j, -1.0, -0.9, 1.0, 1.0 + 0.1 * j, 0.95]
            data_sdf.save_sample(sdf_dir, cat_id, obj, smp[:64], smp, [0, 0, 0, 1], box)
            seen[(cat_id, obj)] = j
        img = rng.integers(0, 256, size=(137, 137, 4), dtype=np.uint8)
        img[:, :, 3] = np.where(rng.random((137, 137)) < 0.3, 0, 255)
        tm = O.DEMO_TRANS_MAT[0] if k % 3 == 0 else O.synth_trans_mat(25.0 + 40.0 * k, 20.0 + k, 0.8)
        data_sdf.save_view(rendered_dir, cat_id, obj, view, img, tm, np.eye(3), np.zeros((4, 3)))
    return sdf_dir, rendered_dir

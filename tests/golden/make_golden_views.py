"""Generate tests/golden/view_pins.npz: what the REFERENCE'S OWN camera code (preprocessing/create_img_h5.py) stores
for a set of rendering_metadata.txt rows and two norm_params.

Run in the BUILD container (needs /root/reference):   python tests/golden/make_golden_views.py

The functions are extracted by ``ast`` (make_golden.extract), so the module's imports of h5py, cv2 and trimesh never
run; ``get_norm_matrix`` reads its file through a stand-in for ``h5py.File`` that serves the norm_params, and the
per-view statements of ``gen_obj_img_h5`` (:178-179, :182-186) are evaluated verbatim.  Only the recorded arrays
are committed; no test reads the reference.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, extract, statements  # noqa: E402

# az, el, tilt, distance_ratio, 25 (the columns of rendering_metadata.txt)
ROWS = np.array([[30.0, 27.0, 0.0, 0.8, 25.0],
                 [0.0, 0.0, 0.0, 0.9, 25.0],
                 [200.0, 25.0, 0.0, 0.7, 25.0],
                 [123.0, 30.0, 0.0, 0.95, 25.0],
                 [359.2176, 25.3312, 0.0, 0.6512, 25.0],
                 [77.7777, 29.9999, 7.5, 0.7333, 25.0],
                 [270.0, 12.5, -3.25, 1.0, 25.0],
                 [181.0625, 28.125, 0.5, 0.8125, 25.0]])
NORMS = np.array([[0.0, 0.0, 0.0, 1.0],
                  [0.0123, -0.0456, 0.0789, 0.4321]], np.float32)


class _File:   # h5py.File(path, 'r') as a context manager over one dictionary
    store = {}

    def __init__(self, path, mode="r"):
        pass

    def __enter__(self):
        return self.store

    def __exit__(self, *a):
        return False


def view_pins():
    src = os.path.join(REF, "preprocessing/create_img_h5.py")
    names = {"rot90y", "getBlenderProj", "get_rotate_matrix", "get_norm_matrix", "get_img_cam", "degree2rad",
             "camera_info", "get_cam_pos", "get_az", "get_el", "get_inl"}
    h5py = type("h5py", (), {"File": _File})
    g = extract(src, names, {"h5py": h5py})
    code = statements(src, 178, 179) + "\n" + statements(src, 182, 186)
    out = {k: [] for k in ("K", "RT", "trans_mat", "regress_mat", "obj_rot_mat")}
    for norm in NORMS:
        _File.store = {"norm_params": norm}
        env = dict(g)
        env["norm_mat"] = g["get_norm_matrix"]("ori_sample.h5")
        env["rot_mat"] = g["get_rotate_matrix"](-np.pi / 2)
        env["param_lst"] = [ROWS[num, ...].astype(np.float32) for num in range(len(ROWS))]    # :167
        for i in range(len(ROWS)):
            env["i"] = i
            exec(code, env)
            out["K"].append(np.asarray(env["K"], np.float64))
            out["RT"].append(np.asarray(env["RT"], np.float64))
            out["trans_mat"].append(np.asarray(env["trans_mat_right"], np.float64))
            out["regress_mat"].append(np.asarray(env["regress_mat"], np.float64))
            out["obj_rot_mat"].append(np.asarray(env["obj_rot_mat"]))
    pins = {k: np.stack(v).reshape((len(NORMS), len(ROWS)) + v[0].shape) for k, v in out.items()}
    pins["rows"] = ROWS
    pins["norm_params"] = NORMS
    pins["rot_mat"] = np.asarray(g["get_rotate_matrix"](-np.pi / 2), np.float64)
    return pins


if __name__ == "__main__":
    pins = view_pins()
    np.savez(os.path.join(HERE, "view_pins.npz"), **pins)
    for k, v in pins.items():
        print(k, v.shape, v.dtype)

"""Digests of the two training steps, to compare two builds of the library bit for bit.

    python tools/train_step_digest.py run OUT.txt [--dump DIR] [--unstable-from OTHER.txt]
    python tools/train_step_digest.py compare PARENT.txt NEW.txt [--parent-dump DIR --new-dump DIR]

run: both trainers from seeded weights (WeightStore.random_init(0, mode="he"), train_cam.random_init(0)) and a seeded
feed at (B, N) = (2, 256) and (3, 200); SDF precisions f32, f32_mfma, bf16; camera precisions f32, bf16 with loss_mode
3D and ALL.  forward_backward runs twice per case; per run one line per slice -- every output and every variable's
gradient -- with its CRC-32C (disn_crc32c).  --dump: the gradient slices whose two runs differ (and those OTHER.txt
marks as differing) as DIR/<case>.<run>.<variable>.npy, for the comparison by value.

compare: PARENT.txt and NEW.txt side by side.  A slice whose two parent runs agree must have that digest in both new
runs; one that differs between the parent's own runs (the float atomics of gather_bwd reach the SDF step's conv
gradients) is compared by value: max |new - parent run 0| <= 2 x max |parent run 1 - parent run 0|.  Exit status 1 when
a slice fails.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ((2, 256), (3, 200))


def _read(path):
    """-> {(case, slice): [digest run 0, digest run 1]} in file order"""
    out = {}
    for line in open(path):
        case, run, name, crc = line.split()
        out.setdefault((case, name), [None, None])[int(run)] = crc
    return out


def _fname(case, run, name):
    return "%s.%d.%s.npy" % (case, run, name.replace("/", "_"))


def run(a):
    import torch
    from disn_amd import tf_checkpoint as tfc
    from disn_amd import train_cam
    from disn_amd.train_sdf import Trainer
    from disn_amd.weights import WeightStore
    from oracle import disn_oracle as O
    other = _read(a.unstable_from) if a.unstable_from else {}
    lines = []

    def case_runs(case, tr, feed, out_names):
        """two forward_backward calls; digests of the outputs and of every gradient slice"""
        runs = []
        for _ in range(2):
            outs = tr.forward_backward(feed)
            torch.cuda.synchronize()
            sl = {n: o.cpu().numpy() for n, o in zip(out_names, outs)}
            sl.update(tr.flat.to_arrays(tr.grads, "/grad"))
            runs.append(sl)
        for r, sl in enumerate(runs):
            for n, v in sl.items():
                lines.append("%s %d %s %08x" % (case, r, n, tfc.crc32c(np.ascontiguousarray(v))))
        if a.dump:
            for n in runs[0]:
                o = other.get((case, n))
                if not np.array_equal(runs[0][n], runs[1][n]) or (o and o[0] != o[1]):
                    for r in range(2):
                        np.save(os.path.join(a.dump, _fname(case, r, n)), runs[r][n])

    def dev(d):
        return {k: torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda() for k, v in d.items()}

    store = WeightStore.random_init(0, mode="he")
    for prec in ("f32", "f32_mfma", "bf16"):
        tr = Trainer(store, batch_size=2, precision=prec)
        for B, N in SHAPES:
            feed = O.synth_inputs(seed=3, batch=B, n_points=N)
            feed["sample_pc_rot"] = feed["sample_pc"][..., [2, 1, 0]] * np.array([-1, 1, 1], np.float32)
            feed["sdf"] = (0.05 * np.random.default_rng(4).standard_normal((B, N, 1))).astype(np.float32)
            case_runs("sdf:%s:%dx%d" % (prec, B, N), tr,
                      dev({k: feed[k] for k in ("imgs", "trans_mat", "sample_pc", "sample_pc_rot", "sdf")}),
                      ("pred", "losses"))
        tr.close()
        del tr
        torch.cuda.empty_cache()
    arrays = train_cam.random_init(0)
    K = np.array([[149.84375, 0, 68.5], [0, 149.84375, 68.5], [0, 0, 1]], np.float32)
    for prec in ("f32", "bf16"):
        for mode in ("3D", "ALL"):
            tr = train_cam.CamTrainer(arrays, batch_size=2, precision=prec, loss_mode=mode)
            for B, N in SHAPES:
                rng = np.random.default_rng(5)
                q = np.linalg.qr(rng.standard_normal((B, 3, 3)))[0]
                RT = np.concatenate([q, np.tile([[-0.0019, 0.0017, 1.39]], (B, 1, 1))], 1).astype(np.float32)
                feed = {"imgs": rng.random((B, 137, 137, 3)), "sample_pc": (rng.random((B, N, 3)) - 0.5) * 0.9,
                        "RT": RT, "trans_mat": RT @ K.T}
                case_runs("cam:%s:%s:%dx%d" % (prec, mode, B, N), tr, dev(feed), ("pred_trans_mat", "losses", "dists"))
            tr.close()
            del tr
            torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("%d digests -> %s" % (len(lines), a.out))
    return 0


def compare(a):
    P, Nw = _read(a.parent), _read(a.new)
    bad, by_value = 0, 0
    print("# case slice | parent run 0, run 1 | new run 0, run 1 | verdict")
    for key, p in P.items():
        n = Nw.get(key, [None, None])
        if p[0] == p[1]:
            ok = n[0] == p[0] and n[1] == p[0]
            verdict = "same" if ok else "DIFFERS"
        elif a.parent_dump and a.new_dump:
            by_value += 1
            p0, p1 = (np.load(os.path.join(a.parent_dump, _fname(key[0], r, key[1]))) for r in range(2))
            noise = float(np.abs(p1 - p0).max())
            d = [float(np.abs(np.load(os.path.join(a.new_dump, _fname(key[0], r, key[1]))) - p0).max()) for r in range(2)]
            ok = max(d) <= 2 * noise
            verdict = "by value: parent run-to-run %.3g, new to parent %.3g %.3g, scale %.3g: %s" % (
                noise, d[0], d[1], float(np.abs(p0).max()), "within 2x" if ok else "OUTSIDE 2x")
        else:
            ok, verdict = False, "parent runs differ and no dumps were given"
        bad += not ok
        print("%s %s | %s %s | %s %s | %s" % (key[0], key[1], p[0], p[1], n[0], n[1], verdict))
    missing = [k for k in Nw if k not in P]
    print("# %d slices, %d compared by value, %d failed, %d only in the new file" % (len(P), by_value, bad, len(missing)))
    return 1 if bad or missing else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("out")
    r.add_argument("--dump")
    r.add_argument("--unstable-from")
    c = sub.add_parser("compare")
    c.add_argument("parent")
    c.add_argument("new")
    c.add_argument("--parent-dump")
    c.add_argument("--new-dump")
    a = ap.parse_args()
    if getattr(a, "dump", None):
        os.makedirs(a.dump, exist_ok=True)
    sys.exit(run(a) if a.cmd == "run" else compare(a))

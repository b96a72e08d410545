"""GPU tests of the device-resident training set (disn_assemble_batch, disn_amd/csrc/batch_assemble.hip) and of the
training driver ``python -m disn_amd.train_sdf``: the kernel against ``ResidentSet.host_batch``, the feed against the
loader thread's, the driver end to end (best / resume), data parallel, and the time to a ready batch."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import train_driver_fixtures as TF
from disn_amd import data_resident as R
from disn_amd import data_sdf as D
from disn_amd import train_sdf as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
GAMMA3 = 3 * U / (1 - 3 * U)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("train_tree_gpu")
    info, listinfo = TF.write_tree(root, TF.SMALL_OBJECTS, views=(0, 3, 7), seed=5)
    rset = R.ResidentSet.from_tree(listinfo, info, workers=4).to("cuda:0")
    return info, listinfo, rset


def _host(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("rot", [False, True])
@pytest.mark.parametrize("white", [False, True])
def test_kernel_equals_the_host_restatement(tree, rot, white):
    """B = 7 of the 15 views, S = 77: objects of 40, 64 and 65 rows are sampled with replacement (S larger than the
    object), 300 and 500 without; 77 is no multiple of the 256-point block, 7 of nothing"""
    _, _, rset = tree
    stream = R.PlanStream(rset, 7, 1, 77, seed=3 + rot + 2 * white)
    for index in (0, 7):
        plan = stream.work(index)
        want = rset.host_batch(plan, rot=rot, backcolorwhite=white)
        feed = {k: _host(v) for k, v in rset.assemble(plan, rot=rot, backcolorwhite=white).items()}
        rset.raise_on_flags()
        assert np.array_equal(feed["imgs"], want["img"])
        assert np.array_equal(feed["sample_pc"], want["sdf_pt"])
        assert np.array_equal(feed["sdf"], want["sdf_val"] - np.float32(0.003)) and feed["sdf"].shape == (7, 77, 1)
        assert np.array_equal(feed["trans_mat"], want["trans_mat"])
        if not rot:
            assert np.array_equal(feed["sample_pc_rot"], want["sdf_pt"])
            continue
        # both sides are a three-term fp32 dot product, numpy's in an unknown association: each is within
        # gamma_3 * sum |p_k||r_k| of the exact value (Higham, Accuracy and Stability, §3.1), so they are within twice that
        p = want["sdf_pt"].astype(np.float64)
        Rm = np.stack([np.asarray(rset.obj_rot_mat[e]) for e in plan.entries]).astype(np.float64)
        bound = 2 * GAMMA3 * np.einsum("bsk,bkj->bsj", np.abs(p), np.abs(Rm))
        err = np.abs(feed["sample_pc_rot"].astype(np.float64) - want["sdf_pt_rot"].astype(np.float64))
        print("sample_pc_rot: max |gpu - host| %.3g, max of the bound %.3g, worst ratio %.3g"
              % (err.max(), bound.max(), (err / bound).max()))
        assert (err <= bound).all()
        assert not np.array_equal(feed["sample_pc_rot"], feed["sample_pc"])
        exact = np.einsum("bsk,bkj->bsj", p, Rm)             # ... and each side alone within gamma_3
        assert (np.abs(feed["sample_pc_rot"] - exact) <= 0.5 * bound).all()


def test_kernel_at_one_sample_of_one_point(tree):
    """B = 1, S = 1: the smallest batch disn_assemble_batch admits, against the same host restatement"""
    _, _, rset = tree
    plan = R.PlanStream(rset, 1, 1, 1, seed=9).work(0)
    want = rset.host_batch(plan, rot=False, backcolorwhite=False)
    feed = {k: _host(v) for k, v in rset.assemble(plan, rot=False, backcolorwhite=False).items()}
    rset.raise_on_flags()
    assert feed["sample_pc"].shape == (1, 1, 3) and feed["sdf"].shape == (1, 1, 1)
    assert np.array_equal(feed["imgs"], want["img"]) and np.array_equal(feed["sample_pc"], want["sdf_pt"])
    assert np.array_equal(feed["sdf"], want["sdf_val"] - np.float32(0.003))
    assert np.array_equal(feed["trans_mat"], want["trans_mat"]) and np.array_equal(feed["sample_pc_rot"], want["sdf_pt"])


def test_kernel_reads_nothing_outside_the_set(tree):
    """the library's own range check (ResidentSet.assemble refuses such a plan on the host before any launch): an
    index outside its range gives zeros and raises the flag, the other samples are untouched"""
    from disn_amd import ops
    _, _, rset = tree
    plan = R.PlanStream(rset, 3, 1, 20, seed=1).work(0)
    d = rset._dev
    good = rset.assemble(plan)
    choice = plan.choice.copy()
    count = int(rset.sample_off[plan.obj_idx[1] + 1] - rset.sample_off[plan.obj_idx[1]])
    choice[1, 4], choice[1, 5] = count, -1
    view = plan.entries.copy()
    view[2] = len(rset.listinfo)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    feed = ops.assemble_batch(d["samples"], d["sample_off"], d["img"], d["trans_mat"], d["obj_rot_mat"],
                              dev(plan.obj_idx), dev(view), dev(choice), flags)
    assert int(flags.item()) == 1
    assert torch.equal(feed["sample_pc"][1, 4:6], torch.zeros(2, 3, device="cuda"))
    assert torch.equal(feed["sample_pc_rot"][1, 4:6], torch.zeros(2, 3, device="cuda"))
    assert torch.equal(feed["sdf"][1, 4:6], torch.zeros(2, 1, device="cuda"))        # 0, not -0.003
    assert float(feed["imgs"][2].abs().max()) == 0.0 and float(feed["trans_mat"][2].abs().max()) == 0.0
    keep = torch.ones(3, 20, dtype=torch.bool, device="cuda")
    keep[1, 4:6] = False
    assert torch.equal(feed["sample_pc"][keep], good["sample_pc"][keep]) and torch.equal(feed["sdf"][keep], good["sdf"][keep])
    assert torch.equal(feed["imgs"][:2], good["imgs"][:2])
    with pytest.raises(IndexError):
        rset.assemble(R.BatchPlan(plan.entries, plan.obj_idx, choice))
    with pytest.raises(TypeError):
        ops.assemble_batch(d["samples"], d["sample_off"], d["img"], d["trans_mat"], d["obj_rot_mat"],
                           dev(plan.obj_idx).long(), dev(view), dev(choice), flags)


@pytest.mark.parametrize("world", [1, 2])
def test_first_feed_equals_the_loaders(tree, world):
    """what Trainer.step receives from the resident path == feed_from_batch(loader.fetch()) for the same seed"""
    info, listinfo, rset = tree
    fl = TF.flags(6, 96, backcolorwhite=True, cat_limit=7, max_epoch=1)
    loader = D.Pt_sdf_img(fl, listinfo=listinfo, info=info, qsize=2, shuffle=True, seed=21)
    rl = R.ResidentLoader(R.PlanStream(rset, 6, 1, 96, cat_limit=7, seed=21), max_epoch=1)
    loader.start()
    rl.start()
    try:
        for _ in range(2):
            batch, plan = loader.fetch(timeout=60), rl.fetch(timeout=60)
            for rank in range(world):
                want = T.feed_from_batch(batch, "cuda:0", rank, world)
                got = rset.assemble(plan, backcolorwhite=True, rank=rank, world=world)
                assert set(got) == set(want)
                for k in want:
                    assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), (k, rank)
    finally:
        loader.shutdown()
        rl.shutdown()


def _driver_tree(root, objects):
    info, _ = TF.write_tree(root, objects, views=range(24), seed=8, sphere=True)
    return ["--train_lst_dir", TF.write_lists(root, objects), "--sdf_dir", info["sdf_dir"],
            "--rendered_dir", info["rendered_dir"]]


def test_driver_end_to_end(tmp_path):
    """three epochs over a two-category tree (96 views, batch 8: 12 steps an epoch), then a resumed run"""
    from disn_amd import tf_checkpoint as tfc
    from disn_amd.weights import WeightStore, variable_shapes
    objects = [(TF.CHAIR, "a0", 600, 40), (TF.CAR, "c0", 200, 40), (TF.CHAIR, "a1", 700, 40), (TF.CAR, "c1", 650, 40)]
    log_dir, pack = str(tmp_path / "log"), str(tmp_path / "pack")
    base = _driver_tree(tmp_path, objects) + ["--category", "chair,car", "--log_dir", log_dir, "--batch_size", "8",
                                              "--num_sample_points", "512", "--log_every", "4", "--backcolorwhite"]
    res = T.main(base + ["--max_epoch", "3", "--loader", "resident", "--pack_dir", pack])
    hist = res["history"]
    print("sdf_loss per epoch:", [h["sdf_loss"] for h in hist], "accuracy:", [h["accuracy"] for h in hist])
    assert res["loader"] == "resident" and res["adam_t_start"] == 0 and len(hist) == 3
    assert all(np.isfinite(v) for h in hist for v in h.values()) and hist[-1]["sdf_loss"] < hist[0]["sdf_loss"]
    assert "model.ckpt" in res["saved"] and os.path.isfile(os.path.join(log_dir, "model.ckpt.index"))
    assert WeightStore.restore_latest(log_dir).complete()
    bundle = tfc.load_checkpoint(tfc.get_checkpoint_state(log_dir))
    for name in variable_shapes():
        assert name + "/Adam" in bundle and name + "/Adam_1" in bundle
    assert "beta1_power" in bundle and "beta2_power" in bundle
    assert R.ResidentSet.is_pack(pack)
    log = open(os.path.join(log_dir, "log_train.txt")).read().splitlines()
    assert log[0].startswith("Namespace(") and "num_sample_points=512" in log[0] and "backcolorwhite=True" in log[0]
    assert sum(l.startswith("**** EPOCH") for l in log) == 3
    assert sum(l.startswith("batch ") and "fetch" in l for l in log) == 3 * (12 // 4)
    assert any(l.startswith("best Model saved in file") for l in log)

    # resume from the directory: Adam's timestep comes back from the bundle; this run uses the loader thread
    saved_t = T.adam_step_from_checkpoint(bundle, 0.999)
    assert saved_t in (12, 24, 36)                            # the end of the epoch that saved last
    with pytest.warns(UserWarning, match="learning-rate schedule restarts"):
        res2 = T.main(base + ["--max_epoch", "1", "--restore_model", log_dir, "--loader", "thread"])
    assert res2["adam_t_start"] == saved_t and res2["loader"] == "thread"
    assert len(res2["history"]) == 1 and np.isfinite(res2["history"][0]["sdf_loss"])
    assert any(l.startswith("Model loaded in file") for l in open(os.path.join(log_dir, "log_train.txt")))
    res3 = T.main(base + ["--max_epoch", "1", "--loader", "auto", "--pack_dir", pack, "--log_dir", str(tmp_path / "l3")])
    assert res3["loader"] == "resident"                       # 7 MB fit; the pack is mapped, not rebuilt
    assert any("pack" in l and "mapped" in l for l in open(str(tmp_path / "l3" / "log_train.txt")))


def test_prefix_filtered_restore(tmp_path):
    """steps 2 and 3 of train() (train/train_sdf.py:276-283): --restore_modelcnn takes the vgg_16 variables of a bundle,
    --restore_modelpn the sdfprediction ones; every other variable, the Adam slots, Adam's timestep and the schedule
    step stay as they were; a variable of another shape (slim's 1000-class fc8) is skipped, as load_model skips it"""
    from disn_amd import tf_checkpoint as tfc
    from disn_amd.train_sdf import VARIABLE_ORDER, Trainer
    from disn_amd.weights import WeightStore
    src = Trainer(WeightStore.random_init(3, mode="he"), batch_size=2)
    prefix = str(tmp_path / "src.ckpt")
    bundle = src.flat.to_arrays(src.params)
    tfc.save_checkpoint(prefix, bundle)                  # the variables alone, as slim's vgg_16.ckpt holds them
    vgg = [n for n in VARIABLE_ORDER if n.startswith("vgg_16")]
    net = [n for n in VARIABLE_ORDER if n.startswith("sdfprediction")]
    assert len(vgg) == 32 and len(net) == 24 and len(vgg) + len(net) == len(VARIABLE_ORDER)

    dst = Trainer(WeightStore.random_init(4, mode="he"), batch_size=2)
    dst.m.fill_(1.0), dst.v.fill_(2.0)
    dst.adam_t, dst.step_count = 3, 5
    before = dst.params.clone()

    def check(taken):
        for name in VARIABLE_ORDER:
            got = dst.flat.view(dst.params, name)
            want = torch.from_numpy(bundle[name]).cuda() if name in taken else dst.flat.view(before, name)
            assert torch.equal(got, want), name
        assert bool((dst.m == 1.0).all()) and bool((dst.v == 2.0).all()) and (dst.adam_t, dst.step_count) == (3, 5)

    assert not torch.equal(dst.params, src.params)
    assert dst.restore(prefix, prefixes=("nothing_of_that_name",)) == 0
    check(())
    assert dst.restore(prefix, prefixes=("vgg_16",)) == 32
    check(vgg)
    assert dst.restore(prefix, prefixes=("sdfprediction",)) == 24
    check(vgg + net)
    assert torch.equal(dst.params, src.params)
    # slim's vgg_16.ckpt: fc8 has 1000 classes and is skipped; the bundle carries no sdfprediction variable at all
    slim = {n: bundle[n] for n in vgg}
    slim["vgg_16/fc8/weights"] = np.zeros((1, 1, 4096, 1000), np.float32)
    slim["vgg_16/fc8/biases"] = np.zeros((1000,), np.float32)
    slim_prefix = str(tmp_path / "vgg_16.ckpt")
    tfc.save_checkpoint(slim_prefix, slim)
    dst.params.copy_(before)
    assert dst.restore(slim_prefix, prefixes=("vgg_16",)) == 30
    check([n for n in vgg if "fc8" not in n])
    src.close(), dst.close()

    # through the driver: the logged counts; a bundle without a matching variable is an error, not a silent random VGG
    base = _driver_tree(tmp_path, [(TF.CHAIR, "a0", 100, 40)]) + [
        "--category", "chair", "--batch_size", "4", "--num_sample_points", "64", "--max_epoch", "0", "--loader", "thread"]
    log_dir = str(tmp_path / "log")
    res = T.main(base + ["--log_dir", log_dir, "--restore_modelcnn", slim_prefix, "--restore_modelpn", prefix])
    log = open(os.path.join(log_dir, "log_train.txt")).read().splitlines()
    assert "vgg_16 variables restored: 30" in log and "sdfprediction variables restored: 24" in log
    assert res["history"] == [] and res["adam_t_start"] == 0 and res["saved"] == []
    with pytest.raises(ValueError, match="--restore_modelpn"):
        T.main(base + ["--log_dir", str(tmp_path / "log2"), "--restore_modelpn", slim_prefix])


def _launch(world, argv, port, out_dir, limit=600, module=False):
    """one fresh process per rank, each under its own time limit; their output goes to files (no pipe to fill).
    module: the documented command itself, `python -m disn_amd.train_sdf`; else tools/ddp_train_driver.py around the
    same `main` (it adds a digest of the final parameters).  -> per rank the helper's JSON, or the standard output"""
    procs, files = [], []
    prog = ["-m", "disn_amd.train_sdf"] if module else [os.path.join(ROOT, "tools", "ddp_train_driver.py")]
    for rank in range(world):
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", RANK=str(rank), WORLD_SIZE=str(world),
                   LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        files.append((open(os.path.join(str(out_dir), "rank%d.out" % rank), "w+"),
                      open(os.path.join(str(out_dir), "rank%d.err" % rank), "w+")))
        procs.append(subprocess.Popen(["timeout", "-k", "10", str(limit), sys.executable] + prog + argv, cwd=ROOT,
                                      stdout=files[-1][0], stderr=files[-1][1], env=env))
    try:
        for p in procs:
            p.wait(timeout=limit + 30)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    outs = []
    for rank, (p, (fo, fe)) in enumerate(zip(procs, files)):
        fo.seek(0), fe.seek(0)
        out, err = fo.read(), fe.read()
        fo.close(), fe.close()
        assert p.returncode == 0 and (module or "DDP_TRAIN_OK %d " % rank in out), "rank %d (exit %s):\n%s" % (
            rank, p.returncode, "\n".join(err.splitlines()[-25:]))
        outs.append(out if module else json.loads(out.split("DDP_TRAIN_OK %d " % rank, 1)[1].splitlines()[0]))
    return outs


def _ddp_args(tmp_path):
    log_dir = str(tmp_path / "log")
    return log_dir, _driver_tree(tmp_path, [(TF.CHAIR, "a0", 300, 40)]) + [
        "--category", "chair", "--log_dir", log_dir, "--batch_size", "12", "--num_sample_points", "64",
        "--max_epoch", "1", "--log_every", "1", "--loader", "resident", "--rot"]


def test_the_command_under_a_one_rank_torchrun_environment(tmp_path):
    """`python -m disn_amd.train_sdf` itself as a fresh child with RANK / WORLD_SIZE / LOCAL_RANK / MASTER_* set: main
    creates the 'nccl' group on device LOCAL_RANK, trains, meets its final barrier, destroys the group and exits 0;
    rank 0 wrote the log and the checkpoint"""
    from disn_amd import tf_checkpoint as tfc
    log_dir, argv = _ddp_args(tmp_path)
    (out,) = _launch(1, argv, 29547, tmp_path, module=True)
    log = open(os.path.join(log_dir, "log_train.txt")).read().splitlines()
    assert log[0].startswith("Namespace(") and log[0] in out                            # rank 0 prints what it logs
    assert sum(l.startswith("batch ") for l in log) == 2 and "loader: resident" in "\n".join(log)
    assert sum("Model saved in file" in l for l in log) == 1
    prefix = tfc.get_checkpoint_state(log_dir)
    assert prefix is not None and os.path.isfile(prefix + ".index")
    assert T.adam_step_from_checkpoint(tfc.load_checkpoint(prefix, ["beta2_power"]), 0.999) == 2


def test_driver_on_two_ranks(tmp_path):
    """--batch_size 12 is the global batch: 6 per rank, two steps; main owns the process group on every rank
    (tools/ddp_train_driver.py only adds a digest of the final parameters); the ranks end with the same parameters bit
    for bit, rank 0 alone logs and saves"""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    log_dir, argv = _ddp_args(tmp_path)
    r0, r1 = _launch(2, argv, 29548, tmp_path)
    assert r0["steps"] == r1["steps"] == 2 and r0["world"] == r1["world"] == 2
    assert r0["params_sha256"] == r1["params_sha256"]
    assert r0["saved"] and r1["saved"] == []
    assert sorted(f for f in os.listdir(log_dir) if f.endswith(".index")) == sorted(s + ".index" for s in r0["saved"])
    assert sum(l.startswith("batch ") for l in open(os.path.join(log_dir, "log_train.txt"))) == 2


def test_ready_batch_is_faster_than_the_loader(tmp_path):
    """40 objects x 32 768 samples, B = 20, S = 2048: wall time to one ready batch on the device, synchronised -- the
    host index draw + index upload + one launch, against Pt_sdf_img.get_batch (the same draw after two file reads
    per sample) + feed_from_batch.  Figures: DESIGN §4t."""
    objects = [(TF.CHAIR if i % 2 else TF.CAR, "o%02d" % i, 32768, 32768) for i in range(40)]
    info, listinfo = TF.write_tree(tmp_path, objects, views=(0,), seed=1)
    fl = TF.flags(20, 2048)
    loader = D.Pt_sdf_img(fl, listinfo=listinfo, info=info, shuffle=True, seed=0)
    t0 = time.perf_counter()
    rset = R.ResidentSet.from_tree(listinfo, info, workers=8)
    t1 = time.perf_counter()
    rset.to("cuda:0")
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    stream = R.PlanStream(rset, 20, 1, 2048, seed=0)

    def resident(index):
        feed = rset.assemble(stream.work(index))
        torch.cuda.synchronize()
        return feed

    def thread(index):
        feed = T.feed_from_batch(loader.work(0, index), "cuda:0")
        torch.cuda.synchronize()
        return feed

    def clock(fn):
        fn(0)                                   # warm-up: the first launch, the page cache
        ts = []
        for index in (0, 20, 0, 20, 0):
            t = time.perf_counter()
            fn(index)
            ts.append(time.perf_counter() - t)
        return float(np.median(ts))
    t_res, t_thr = clock(resident), clock(thread)
    t = time.perf_counter()
    for index in (0, 20, 0, 20, 0):
        stream.work(index)
    t_draw = (time.perf_counter() - t) / 5
    print("ready batch 20 x 2048: resident %.3f ms (host draw alone %.3f ms), loader %.3f ms, ratio %.1f; "
          "set read in %.2f s, %d bytes uploaded in %.3f s"
          % (t_res * 1e3, t_draw * 1e3, t_thr * 1e3, t_thr / t_res, t1 - t0, rset.device_bytes(), t2 - t1))
    assert t_res < t_thr

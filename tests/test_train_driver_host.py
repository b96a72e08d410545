"""Host side of the SDF training driver (``python -m disn_amd.train_sdf``) and of the device-resident training set
(``disn_amd.data_resident``): the batch stream against the loader thread's, the pack files, data-parallel slices,
flag checks, the save rule, the C signature -- no device needed."""
import os
import re

import numpy as np
import pytest

import train_driver_fixtures as TF
from disn_amd import data_resident as R
from disn_amd import data_sdf as D
from disn_amd import train_sdf as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUMERIC = ("sdf_pt", "sdf_pt_rot", "sdf_val", "img", "trans_mat", "norm_params", "sdf_params")
NAMES = ("cat_id", "obj_nm", "view_id")


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("train_tree")
    info, listinfo = TF.write_tree(root, TF.SMALL_OBJECTS, views=(0, 3, 7), seed=5)     # 15 views
    return info, listinfo, R.ResidentSet.from_tree(listinfo, info, workers=4)


def _assert_same_batch(got, want):
    for k in NUMERIC:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    for k in NAMES:
        assert got[k] == want[k], k


# batch 4 of 15 views: 3 batches per epoch; with cat_limit 4 (5) the epoch holds 8 (10) samples and the third batch
# (index 8 + 4 > 8) wraps to index 4 (2)
@pytest.mark.parametrize("seed, kw", [
    (0, dict()),
    (1, dict(rot=True)),
    (2, dict(backcolorwhite=True)),
    (3, dict(rot=True, backcolorwhite=True, cat_limit=4)),
    (4, dict(cat_limit=5, num_points=5)),
])
def test_stream_is_the_loaders(tree, seed, kw):
    info, listinfo, rset = tree
    B, S = 4, 64            # objects of 40 rows (< S: with replacement), 64 (== S), 65, 300, 500 (without)
    fl = TF.flags(B, S, **kw)
    loader = D.Pt_sdf_img(fl, listinfo=listinfo, info=info, shuffle=True, seed=seed)
    stream = R.PlanStream(rset, B, fl.num_points, S, cat_limit=fl.cat_limit, shuffle=True, seed=seed)
    assert len(stream) == len(loader) and stream.num_batches == loader.num_batches == 3
    per_epoch = loader.num_batches * B
    wrapped = False
    for bno in range(0, 2 * per_epoch, B):                  # two epochs, as Pt_sdf_img.run walks them
        index = bno % per_epoch
        wrapped |= index + B > len(loader)
        want = loader.work(bno // per_epoch, index)
        plan = stream.work(index)
        _assert_same_batch(rset.host_batch(plan, rot=fl.rot, backcolorwhite=fl.backcolorwhite), want)
        assert plan.choice.dtype == np.int32 and plan.choice.shape == (B, S)
    assert wrapped == ("cat_limit" in kw)
    if fl.rot:                                               # the fixture's rotations are not the identity
        assert not np.array_equal(want["sdf_pt"], want["sdf_pt_rot"])
    if fl.backcolorwhite:                                    # ... and 30 % of their pixels have alpha 0
        assert not np.array_equal(rset.host_batch(plan, rot=fl.rot)["img"], want["img"])


def test_explicit_cats_limit_and_the_loader_thread(tree):
    """the driver's call: cats_limit given (24 per object in the reference, here the true counts) and the plans
    fetched from the one-batch-ahead thread"""
    info, listinfo, rset = tree
    fl = TF.flags(5, 48, cat_limit=7, max_epoch=2)
    cats_limit = {TF.CHAIR: 9, TF.CAR: 6}
    loader = D.Pt_sdf_img(fl, listinfo=listinfo, info=info, cats_limit=dict(cats_limit), shuffle=True, seed=11)
    rl = R.ResidentLoader(R.PlanStream(rset, 5, 1, 48, cats_limit=cats_limit, cat_limit=7, seed=11), max_epoch=2)
    rl.start()
    per_epoch = loader.num_batches * 5
    for bno in range(0, 2 * per_epoch, 5):
        want = loader.work(bno // per_epoch, bno % per_epoch)
        _assert_same_batch(rset.host_batch(rl.fetch(timeout=30)), want)
    rl.join(timeout=30)
    assert not rl.is_alive()                                 # max_epoch epochs, then the thread ends
    with pytest.raises(RuntimeError, match="ended"):
        rl.fetch(timeout=1)
    rl.shutdown()


def test_pack_round_trip(tree, tmp_path):
    _, listinfo, rset = tree
    d = str(tmp_path / "pack")
    assert not R.ResidentSet.is_pack(d)
    rset.save(d)
    assert R.ResidentSet.is_pack(d)
    assert sorted(os.listdir(d)) == sorted([k + ".npy" for k in R._ARRAYS] + ["index.json"])    # no temporary left
    back = R.ResidentSet.load(d)
    assert back.listinfo == rset.listinfo == [tuple(e) for e in listinfo] and back.objects == rset.objects
    for k in R._ARRAYS:
        a, b = getattr(rset, k), getattr(back, k)
        assert isinstance(b, np.memmap) and a.dtype == b.dtype and np.array_equal(a, b), k
    assert rset.sample_off.tolist() == [0, 300, 340, 404, 904, 969] and rset.ori_n.tolist() == [50, 70, 20, 90, 33]
    plan = R.PlanStream(back, 4, 1, 64, seed=9).work(0)
    _assert_same_batch(back.host_batch(plan, rot=True), rset.host_batch(plan, rot=True))
    assert back.device_bytes() == rset.device_bytes() == 969 * 16 + 6 * 8 + 15 * (137 * 137 * 4 + 48 + 36)


def test_world_size_invariance(tree):
    _, _, rset = tree
    plan = R.PlanStream(rset, 8, 1, 32, seed=2).work(0)
    whole = rset.host_batch(plan, rot=True, backcolorwhite=True)
    for world in (2, 4):
        parts = [rset.host_batch(plan.shard(world, r), rot=True, backcolorwhite=True) for r in range(world)]
        for k in NUMERIC:
            assert np.array_equal(np.concatenate([p[k] for p in parts], 0), whole[k]), (world, k)
        for k in NAMES:
            assert sum((p[k] for p in parts), []) == whole[k]
    with pytest.raises(ValueError):
        plan.shard(3, 0)


def test_plan_outside_the_set_is_refused(tree):
    _, _, rset = tree
    plan = R.PlanStream(rset, 4, 1, 16, seed=0).work(0)
    bad = plan.choice.copy()
    bad[2, 5] = int(rset.sample_off[plan.obj_idx[2] + 1] - rset.sample_off[plan.obj_idx[2]])   # one past the object's rows
    with pytest.raises(IndexError):
        rset.host_batch(R.BatchPlan(plan.entries, plan.obj_idx, bad))
    with pytest.raises(ValueError):
        R.ResidentSet.from_tree([(TF.CHAIR, "a0", 0), (TF.CHAIR, "a0", 0)], {}, workers=1)
    with pytest.raises(ValueError):
        R.ResidentSet.from_tree([], {}, workers=17)


# ---- the driver ------------------------------------------------------------------------------------------------
def _no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("device work began before the arguments were checked")
    import disn_amd.engine as engine
    monkeypatch.setattr(engine, "SdfEngine", refuse)
    monkeypatch.setattr(T, "Trainer", refuse)


@pytest.mark.parametrize("flag", ["--binary", "--threedcnn", "--img_feat_onestream", "--multi_view", "--alpha",
                                  "--volimp"])
def test_unsupported_flags_raise(tmp_path, monkeypatch, flag):
    _no_device(monkeypatch)
    with pytest.raises(NotImplementedError, match="out of scope"):
        T.main(["--train_lst_dir", str(tmp_path), "--log_dir", str(tmp_path / "log"), flag])
    assert not os.path.exists(str(tmp_path / "log"))


def test_momentum_and_tanh_raise(tmp_path, monkeypatch):
    _no_device(monkeypatch)
    with pytest.raises(NotImplementedError, match="momentum"):
        T.main(["--train_lst_dir", str(tmp_path), "--optimizer", "momentum"])
    with pytest.raises(NotImplementedError, match="tanh"):
        T.main(["--train_lst_dir", str(tmp_path), "--tanh"])


def test_reference_flags_parse():
    a = T.parse_args([])
    assert (a.category, a.num_points, a.num_sample_points, a.max_epoch, a.batch_size) == ("all", 1, 256, 200, 32)
    assert (a.learning_rate, a.beta1, a.decay_step, a.decay_rate, a.mask_weight, a.cat_limit) == \
        (1e-4, 0.5, 200000, 0.9, 4.0, 168000)
    assert (a.loader, a.precision, a.seed, a.wd) == ("auto", "f32", 0, 1e-5)
    a = T.parse_args(["--rot", "--backcolorwhite", "--cam_est", "--img_feat_twostream", "--augcolorfore",
                      "--augcolorback", "--restore_modelpn", "p", "--restore_modelcnn", "c", "--restore_model", "m",
                      "--sdf_dir", "s", "--rendered_dir", "r", "--pack_dir", "k", "--loader", "resident"])
    T.check_flags(a)
    assert a.rot and a.backcolorwhite and a.loader == "resident"


def test_missing_list_or_checkpoint_raises_before_device_work(tmp_path, monkeypatch):
    _no_device(monkeypatch)
    log = str(tmp_path / "log")
    with pytest.raises(FileNotFoundError, match="_train.lst"):
        T.main(["--train_lst_dir", str(tmp_path), "--category", "chair", "--log_dir", log])
    lst = TF.write_lists(tmp_path, [(TF.CHAIR, "a0", 0, 0)])
    base = ["--train_lst_dir", lst, "--category", "chair", "--log_dir", log, "--batch_size", "4"]
    with pytest.raises(FileNotFoundError, match="_train.lst"):
        T.main(base[:2] + ["--category", "chair,car"] + base[4:])       # the car list is missing
    for flag in ("--restore_modelcnn", "--restore_modelpn"):
        with pytest.raises(FileNotFoundError, match=flag):
            T.main(base + [flag, str(tmp_path / "nothing.ckpt")])
    os.makedirs(str(tmp_path / "empty"))
    for d in ("empty", "absent"):
        with pytest.raises(FileNotFoundError, match="--restore_model"):
            T.main(base + ["--restore_model", str(tmp_path / d)])
    for loader in ("auto", "resident", "thread"):
        with pytest.raises(FileNotFoundError, match="sdf_dir"):
            T.main(base + ["--sdf_dir", str(tmp_path / "no_sdf"), "--rendered_dir", str(tmp_path / "no_img"),
                           "--loader", loader])
    with pytest.raises(ValueError, match="fewer than one batch"):
        T.main(base[:-1] + ["25"])
    assert not os.path.exists(log)


def test_train_listinfo(tmp_path):
    objs = [(TF.CAR, "c0", 0, 0), (TF.CHAIR, "a0", 0, 0), (TF.CAR, "c1", 0, 0)]
    lst = TF.write_lists(tmp_path, objs)
    listinfo, cats_limit = T.train_listinfo(lst, "car,chair")
    want = [(c, o, v) for c, o in ((TF.CHAIR, "a0"), (TF.CAR, "c0"), (TF.CAR, "c1")) for v in range(24)]
    assert listinfo == want and cats_limit == {TF.CHAIR: 24, TF.CAR: 48}      # CATS_ALL order: chair before car
    assert T.train_listinfo(lst, "car")[0] == want[24:]


def test_save_policy():
    """train/train_sdf.py:314-328: best_acc starts at 0; a strictly better epoch saves model.ckpt, otherwise every
    tenth epoch saves model_epoch_%03d.ckpt"""
    acc = [0.0, 0.5, 0.4, 0.5, 0.6, 0.1, 0.1, 0.1, 0.1, 0.1, 0.2, 0.7, 0.7, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3, 0.7]
    best, got = 0.0, []
    for epoch, a in enumerate(acc):
        name, best = T.save_decision(epoch, a, best)
        got.append(name)
    want = [None] * len(acc)
    want[0] = "model_epoch_000.ckpt"          # 0.0 is not better than the initial 0
    want[1] = want[4] = want[11] = "model.ckpt"
    want[10] = "model_epoch_010.ckpt"
    want[20] = "model_epoch_020.ckpt"         # a tie with the best is not better
    assert got == want and best == 0.7


def test_choose_loader():
    lines = []
    assert T.choose_loader("thread", 1, 10, lines.append) == "thread"
    assert T.choose_loader("auto", 10, 10, lines.append) == "resident"
    assert T.choose_loader("resident", 9, 10, lines.append) == "resident" and not lines
    assert T.choose_loader("auto", 11, 10, lines.append) == "thread"
    assert len(lines) == 1 and "11" in lines[0] and "10" in lines[0]
    with pytest.raises(MemoryError):
        T.choose_loader("resident", 11, 10, lines.append)


def test_assemble_batch_signature():
    """the header, the binding and the library agree on disn_assemble_batch; the ABI number did not move"""
    import ctypes as C

    from disn_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "disn_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+disn_assemble_batch\s*\(([^)]*)\)\s*;", hdr)
    assert m, "include/disn_amd.h does not declare disn_assemble_batch"
    ctype = {"const float*": C.c_void_p, "float*": C.c_void_p, "const int64_t*": C.c_void_p, "void*": C.c_void_p,
             "const uint8_t*": C.c_void_p, "const int32_t*": C.c_void_p, "int32_t*": C.c_void_p,
             "int64_t": C.c_int64, "int": C.c_int}
    args = [ctype[" ".join(a.split()[:-1])] for a in m.group(1).split(",")]
    res, sig = _lib.SIGNATURES["disn_assemble_batch"]
    assert res is C.c_int and sig == args and len(args) == 21
    assert _lib.ABI_VERSION == 10 and _lib.lib().disn_abi_version() == 10
    assert re.search(r"#define\s+DISN_ABI_VERSION\s+10\b", hdr)
    assert hasattr(_lib.lib(), "disn_assemble_batch")

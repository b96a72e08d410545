"""CPU tests of the surface sampler: ``metrics.sample_surface_arrays``, the host function that IS the specification of
mesh_sample.hip, checked against geometry and statistics; ``surface_scores``' arithmetic; ``mesh_seed``;
``evaluate surface`` and ``create_sdf --score`` with the device calls replaced; the fourth header of the C ABI.
Bars used below, all the issue's:
  * two triangles of areas 0.5 and 1.5: weights exactly [715827882, 2147483648]; the share of face 0 among 65 536
    samples within 5 sigma = 5 sqrt(0.25 0.75 / 65536) = 0.0085 of 0.25;
  * uniformity on the uneven unit square: chi^2 of an 8 x 8 histogram of 65 536 points below 103.4, the 0.999 quantile
    at 63 degrees of freedom;
  * a point lies in its face's plane and inside the face to 1e-6 max|coordinate|, a normal is unit to 1e-6.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_sample_fixtures as XF  # noqa: E402
import reconstruct_fixtures as RF  # noqa: E402
from disn_amd import create_sdf as cs  # noqa: E402
from disn_amd import evaluate as E  # noqa: E402
from disn_amd import metrics as M  # noqa: E402

SF = XF.SF
MF = SF.MF
NEW = ("disn_mesh_sample_workspace_bytes", "disn_mesh_sample_batch")


@pytest.fixture(scope="module", autouse=True)
def _built():
    from disn_amd.csrc import build
    build.build()


# ------------------------------------------------------------------ the rule
def test_weights_are_the_integers_of_the_rule_and_the_shares_follow_the_areas():
    v, f = XF.two_triangles()
    q = M.surface_face_weights(v, f)
    assert q.dtype == np.uint64 and q.tolist() == [715827882, 2147483648]
    sigma5 = 5 * np.sqrt(0.25 * 0.75 / 65536)
    assert abs(sigma5 - 0.0085) < 1e-4
    for seed in (0, 1, 12345):
        p, nrm, face, status = M.sample_surface_arrays(v, f, 65536, seed)
        share = float((face == 0).mean())
        print("seed %d: share of face 0 = %.4f" % (seed, share))
        assert status == 0 and p.dtype == nrm.dtype == np.float32 and face.dtype == np.int32
        assert abs(share - 0.25) < sigma5
        assert np.array_equal(nrm[face == 0], np.tile(np.float32([0, 0, 1]), ((face == 0).sum(), 1)))
        assert np.array_equal(nrm[face == 1], np.tile(np.float32([0, -1, 0]), ((face == 1).sum(), 1)))


def test_isqrt_and_mulhi_are_exact():
    x = np.array([0, 1, 2, 3, 4, 2 ** 31 - 1, 2 ** 32, 2 ** 62 - 1, 2 ** 62, (2 ** 31 - 1) ** 2, (2 ** 31 - 1) ** 2 - 1,
                  (2 ** 30 + 12345) ** 2 + 2 * (2 ** 30 + 12345)], np.uint64)
    import math
    assert M._isqrt64(x).tolist() == [math.isqrt(int(t)) for t in x]
    a = np.array([2 ** 64 - 1, 12345678901234567, 3, 0, 2 ** 63], np.uint64)
    for b in (0, 1, 2 ** 63 - 1, 12345, 2 ** 40 + 7, 70000 * 2 ** 31):
        assert M._mulhi64(a, b).tolist() == [(int(t) * b) >> 64 for t in a]
    r0, r1 = M._sample_words(2 ** 64 - 3, 4)
    G = 0x9E3779B97F4A7C15
    assert [int(t) for t in r0] == [M.mix64(2 ** 64 - 3 + G * (2 * i + 1)) for i in range(4)]
    assert [int(t) for t in r1] == [M.mix64(2 ** 64 - 3 + G * (2 * i + 2)) for i in range(4)]


def test_faces_without_area_are_never_drawn():
    v, f = XF.with_undrawable_faces()
    assert M.surface_face_weights(v, f).tolist() == [715827882, 0, 2147483648, 0]
    _, _, face, status = M.sample_surface_arrays(v, f, 65536, 7)
    counts = np.bincount(face, minlength=4)
    assert status == 0 and counts[1] == 0 and counts[3] == 0 and counts[0] > 0 and counts[2] > 0
    # below about 2^-31 of the largest area: weight 0 as well
    tiny = np.concatenate([v, np.float32([[0, 0, 0], [2.0 ** -17, 0, 0], [0, 2.0 ** -17, 0]])])
    q = M.surface_face_weights(tiny, np.concatenate([f, np.int32([[6, 7, 8]])]))
    assert q[4] == 0 and q[2] == 2 ** 31


def test_scaling_by_a_power_of_two_leaves_every_face():
    v, f = XF.with_undrawable_faces()
    a = M.sample_surface_arrays(v, f, 65536, 7)
    b = M.sample_surface_arrays(v * np.float32(1024), f, 65536, 7)
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[0] * np.float32(1024), b[0])
    sv, sf = XF.uneven_square()
    assert np.array_equal(M.sample_surface_arrays(sv, sf, 4096, 3)[2],
                          M.sample_surface_arrays(sv * np.float32(1024), sf, 4096, 3)[2])


def test_points_are_uniform_on_the_uneven_square():
    v, f = XF.uneven_square()
    p, _, _, status = M.sample_surface_arrays(v, f, 65536, 3)
    h, _, _ = np.histogram2d(p[:, 0], p[:, 1], bins=8, range=[[0, 1], [0, 1]])
    e = 65536 / 64
    chi2 = float(((h - e) ** 2 / e).sum())
    vertex_mean = v[np.random.default_rng(0).integers(len(v), size=65536)].mean(0)
    print("chi2 (63 dof) = %.1f; mean of the samples %s, of 65 536 vertex samples %s" % (chi2, p.mean(0), vertex_mean))
    assert status == 0 and h.sum() == 65536
    assert chi2 < 103.4


@pytest.mark.parametrize("name", ["two_triangles", "uneven_square", "box", "soup"])
def test_every_sample_lies_on_its_face_with_its_unit_normal(name):
    v, f = {"two_triangles": XF.two_triangles, "uneven_square": XF.uneven_square, "box": lambda: SF.box_mesh(32),
            "soup": XF.soup}[name]()
    p, nrm, face, status = M.sample_surface_arrays(v, f, 4096, 9)
    assert status == 0 and face.min() >= 0 and face.max() < len(f)
    tol = 1e-6 * float(np.abs(v).max())
    a, b, c = (v[f[face, k]].astype(np.float64) for k in range(3))
    n64 = np.cross(b - a, c - a)
    n64 /= np.linalg.norm(n64, axis=1, keepdims=True)
    assert np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1).max() < 1e-6
    assert np.abs(nrm - n64).max() < 1e-6
    d = p.astype(np.float64) - a
    assert np.abs((d * n64).sum(1)).max() <= tol                                   # in the plane
    for p0, p1 in ((a, b), (b, c), (c, a)):                                        # inside: left of every edge
        inward = np.cross(n64, p1 - p0)
        inward /= np.linalg.norm(inward, axis=1, keepdims=True)
        assert ((p.astype(np.float64) - p0) * inward).sum(1).min() >= -tol


def test_a_sample_does_not_depend_on_n():
    v, f = SF.box_mesh(32)
    many, one = M.sample_surface_arrays(v, f, 1000, 21), M.sample_surface_arrays(v, f, 1, 21)
    for a, b in zip(many[:3], one[:3]):
        assert np.array_equal(a[:1], b)
    assert not np.array_equal(many[2], M.sample_surface_arrays(v, f, 1000, 22)[2])


def test_statuses_and_zeros():
    v, f = XF.two_triangles()
    bad = f.copy()
    bad[1, 2] = 5
    nan = v.copy()
    nan[3, 1] = np.nan
    for vv, ff, want in ((v, bad, 2), (v, -f - 1, 2), (nan, f, 4), (nan, bad, 4), XF.empty() + (6,),
                         XF.all_degenerate() + (6,), (v, XF.empty()[1], 6), (nan, XF.empty()[1], 4),
                         (XF.empty()[0], f, 2)):
        p, nrm, face, status = M.sample_surface_arrays(vv, ff, 5, 1)
        assert status == want
        assert p.shape == nrm.shape == (5, 3) and face.shape == (5,) and not p.any() and not nrm.any() and not face.any()
    assert M.STATUS_NO_AREA == 6 and M.STATUS_NO_AREA not in (1, 2, 3, 4, 5)       # no stage's word uses it yet
    for n in (0, -1, 2 ** 20 + 1):
        with pytest.raises(ValueError):
            M.sample_surface_arrays(v, f, n, 0)


def test_mesh_seed_is_stable_and_tells_names_apart():
    import zlib
    assert M.mesh_seed(0, "03001627_obj_a_00.obj") == M.mesh_seed(0, "03001627_obj_a_00.obj")
    assert M.mesh_seed(5, "a") == M.mix64(5 ^ zlib.crc32(b"a")) and M.mix64(0) == 0
    assert M.mix64(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF          # SplitMix64's first output from state 0
    names = ["%s_%s_%02d.obj" % (c, o, k) for c in ("03001627", "02958343") for o in ("obj_a", "obj_b") for k in range(24)]
    seeds = {M.mesh_seed(s, nm) for s in (0, 1) for nm in names}
    assert len(seeds) == 2 * len(names) and all(0 <= s < 2 ** 64 for s in seeds)


# ------------------------------------------------------------------ surface_scores
def _scores_numpy(pp, pn, gp, gn, thresholds):
    out = {k: [] for k in ("accuracy", "completeness", "chamfer_l1", "chamfer_l2", "normal_consistency", "precision",
                           "recall", "f_score")}
    for v in range(len(pp)):
        d1, i1, d2, i2 = XF.nn_brute(pp[v], gp[v])
        acc, comp = np.sqrt(d1).mean(), np.sqrt(d2).mean()
        nc = 0.5 * (np.abs((pn[v] * gn[v][i1]).sum(1)).mean() + np.abs((gn[v] * pn[v][i2]).sum(1)).mean())
        pre = np.array([(np.sqrt(d1) < t).mean() for t in thresholds])
        rec = np.array([(np.sqrt(d2) < t).mean() for t in thresholds])
        with np.errstate(invalid="ignore"):
            fs = np.where(pre + rec > 0, 2 * pre * rec / (pre + rec), 0.0)
        for k, x in zip(out, (acc, comp, 0.5 * (acc + comp), d1.mean() + d2.mean(), nc, pre, rec, fs)):
            out[k].append(x)
    return {k: np.asarray(x) for k, x in out.items()}


def test_surface_scores_arithmetic(monkeypatch):
    import torch
    rng = np.random.default_rng(4)
    unit = lambda x: (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)
    pp, gp = rng.normal(size=(3, 64, 3)).astype(np.float32), rng.normal(size=(3, 64, 3)).astype(np.float32)
    pn, gn = unit(rng.normal(size=(3, 64, 3))), unit(rng.normal(size=(3, 64, 3)))
    thresholds = np.float32([0.0, 0.2, 0.4, 0.8, 10.0])              # none, some, all of the points
    want = _scores_numpy(pp.astype(np.float64), pn.astype(np.float64), gp.astype(np.float64), gn.astype(np.float64),
                         thresholds)

    def nn(a, b):                                                    # nn_distance's outputs from the brute force
        r = [XF.nn_brute(x, y) for x, y in zip(a.numpy(), b.numpy())]
        f = lambda k, dt: torch.from_numpy(np.stack([x[k] for x in r]).astype(dt))
        return f(0, np.float32), f(1, np.int32), f(2, np.float32), f(3, np.int32)

    monkeypatch.setattr(M, "nn_distance", nn)
    monkeypatch.setattr(M.ops, "_chk", lambda t, name: t.contiguous())
    t = torch.from_numpy
    got = M.surface_scores(t(pp), t(pn), t(gp), t(gn), thresholds)
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == np.float64 and got[k].shape == want[k].shape == ((3,) if want[k].ndim == 1 else (3, 5))
        np.testing.assert_allclose(got[k], want[k], rtol=2e-6, atol=1e-7, err_msg=k)   # float32 sqrt, float64 means
    assert (got["precision"][:, 0] == 0).all() and (got["f_score"][:, 0] == 0).all() and (got["recall"][:, 4] == 1).all()
    assert 0 < got["precision"][0, 2] < 1
    # one ground truth [M,3] is tiled to every view
    tiled = M.surface_scores(t(pp), t(pn), t(gp[0]), t(gn[0]), thresholds)
    np.testing.assert_allclose(tiled["chamfer_l1"][0], want["chamfer_l1"][0], rtol=2e-6)
    with pytest.raises(ValueError):
        M.surface_scores(t(pp), t(pn[:, :32]), t(gp), t(gn), thresholds)


# ------------------------------------------------------------------ the drivers, with the device calls replaced
def _fake_device(monkeypatch, calls):
    import torch

    def sample(meshes, n, seeds):
        calls.append(("sample", len(meshes), n, [int(s) for s in seeds]))
        B = len(meshes)
        status = torch.tensor([0 if len(m[1]) else 6 for m in meshes], dtype=torch.int32)
        pts = torch.arange(B, dtype=torch.float32).reshape(B, 1, 1).expand(B, n, 3).contiguous()
        return pts, torch.ones(B, n, 3), torch.zeros(B, n, dtype=torch.int32), status

    def scores(pp, pn, gp, gn, thresholds):
        v, T = pp.shape[0], len(thresholds)
        calls.append(("scores", tuple(pp.shape), tuple(gp.shape), T))
        out = {k: np.arange(v, dtype=np.float64) + j for j, k in enumerate(M.SURFACE_SCORES)}
        out.update({k: np.full((v, T), 0.5) for k in ("precision", "recall", "f_score")})
        return out

    monkeypatch.setattr(M, "sample_surface_meshes_device", sample)
    monkeypatch.setattr(M, "surface_scores", scores)


def test_evaluate_surface_parses_and_samples_each_object_once(monkeypatch, tmp_path):
    import torch
    a = E.parser().parse_args(["surface", "--pred_dir", "p", "--gt_dir", "g", "--test_lst_dir", "l"])
    assert (a.view_num, a.num_sample_points, a.seed, a.truethreshold, a.category) == (24, 2048, 0, 2.5, "all")
    with pytest.raises(SystemExit):
        E.parser().parse_args(["surface", "--cal_dir", "p", "--gt_dir", "g", "--test_lst_dir", "l"])
    pred, gt, lst = tmp_path / "pred", tmp_path / "gt", tmp_path / "lst"
    OBJS = {"03001627": ["a1", "b2"], "02958343": ["c3", "d4"]}    # (a prediction's object is field 1 of its file name)
    RF.write_lists(str(lst), objs=OBJS)
    for _, cat_id in RF.CATS:
        for obj in OBJS[cat_id]:
            os.makedirs(str(gt / cat_id / obj))
            (gt / cat_id / obj / "isosurf.obj").write_text("")
            os.makedirs(str(pred / cat_id), exist_ok=True)
            for view in range(3):
                (pred / cat_id / ("%s_%s_%02d.obj" % (cat_id, obj, view))).write_text("")
    calls, read = [], []
    _fake_device(monkeypatch, calls)
    v, f = XF.two_triangles()
    monkeypatch.setattr(E, "_device_mesh", lambda path, device=None: read.append(path) or (torch.from_numpy(v),
                                                                                          torch.from_numpy(f)))
    lines = []

    class Out:
        write = staticmethod(lines.append)

    res = E.surface_all(dict(RF.CATS), str(pred), str(gt), str(lst), view_num=2, num_sample_points=16, seed=3, out=Out)
    objs = [(c, o) for _, c in RF.CATS for o in OBJS[c]]
    assert [c[0] for c in calls] == ["sample", "sample", "scores"] * len(objs)
    gt_calls, pred_calls, score_calls = calls[0::3], calls[1::3], calls[2::3]
    assert all(c[1:3] == (1, 16) for c in gt_calls) and all(c[1:3] == (2, 16) for c in pred_calls)
    assert [c[3] for c in gt_calls] == [[M.mesh_seed(3, "%s/%s/isosurf.obj" % co)] for co in objs]
    assert all(c[1:] == ((2, 16, 3), (16, 3), 6) for c in score_calls)
    assert len(read) == 3 * len(objs) and sum(p.endswith("isosurf.obj") for p in read) == len(objs)
    for (c, o), call in zip(objs, pred_calls):
        views = res["categories"][c]["objects"][o]["views"]
        assert call[3] == [M.mesh_seed(3, os.path.basename(p)) for p in views] and len(set(views)) == 2
    assert res["chamfer_l1"] == pytest.approx(0.5 + 2) and res["accuracy"] == pytest.approx(0.5)
    assert res["f_score"].shape == (6,) and "".join(lines).count("cat_nm:") == 2 and "done!" in "".join(lines)
    assert res["categories"]["03001627"]["no_area"] == [] and "WARNING" not in "".join(lines)
    # a mesh with a bad index is an error; one without area is scored on zeros, and named
    monkeypatch.setattr(M, "sample_surface_meshes_device", lambda m, n, s: (None, None, None, torch.tensor([0, 2])))
    with pytest.raises(ValueError, match="index"):
        E._sampled([None, None], ["a", "b"], 4, 0)
    monkeypatch.setattr(M, "sample_surface_meshes_device", lambda m, n, s: (1, 2, None, torch.tensor([0, 6, 0])))
    said = []
    assert E._sampled([None] * 3, ["a", "flat.obj", "c"], 4, 0, said.append)[2].tolist() == [0, 6, 0]
    assert len(said) == 1 and "flat.obj" in said[0] and "WARNING" in said[0] and "4 points at the origin" in said[0]


def test_evaluate_surface_names_the_meshes_without_area(monkeypatch, tmp_path, capsys):
    import torch
    pred, gt, lst = tmp_path / "pred", tmp_path / "gt", tmp_path / "lst"
    cats, OBJS = (("chair", "03001627"),), {"03001627": ["a1"]}
    RF.write_lists(str(lst), cats=cats, objs=OBJS)
    os.makedirs(str(gt / "03001627" / "a1"))
    os.makedirs(str(pred / "03001627"))
    for view in range(2):
        (pred / "03001627" / ("03001627_a1_%02d.obj" % view)).write_text("")
    calls = []
    _fake_device(monkeypatch, calls)
    v, f = XF.two_triangles()
    flat = lambda path, device=None: (torch.from_numpy(v), torch.from_numpy(f[:0] if path.endswith("_01.obj") else f))
    monkeypatch.setattr(E, "_device_mesh", flat)
    res = E.surface_all(dict(cats), str(pred), str(gt), str(lst), view_num=2, num_sample_points=4)
    text = capsys.readouterr().out
    assert [os.path.basename(p) for p in res["categories"]["03001627"]["no_area"]] == ["03001627_a1_01.obj"]
    assert res["categories"]["03001627"]["objects"]["a1"]["no_area"] == res["categories"]["03001627"]["no_area"]
    assert text.count("WARNING") == 2 and "03001627_a1_01.obj has no area" in text and "1 mesh(es) without area" in text


def test_score_flags_and_score_group(monkeypatch, tmp_path):
    import torch
    base = ["--test_lst_dir", str(tmp_path / "none"), "--log_dir", str(tmp_path / "log")]
    a = cs.parser().parse_args(base)
    assert a.score is None and a.score_points is None and cs.score_from_flags(a) is None
    assert cs.score_from_flags(cs.parser().parse_args(base + ["--score", "gt"])) == ("gt", 2048)
    assert cs.score_from_flags(cs.parser().parse_args(base + ["--score", "gt", "--score_points", "7"])) == ("gt", 7)

    def boom(*a, **k):
        raise AssertionError("device work was reached")

    for bad in (["--score_points", "5"], ["--score", "gt", "--score_points", "0"],
                ["--score", "gt", "--score_points", str(2 ** 20 + 1)], ["--score", ""]):
        with pytest.raises(ValueError, match="--score"):
            cs.main(base + bad, reconstruct_fn=boom)
    assert not os.path.exists(str(tmp_path / "log"))

    calls, gts = [], []
    _fake_device(monkeypatch, calls)
    monkeypatch.setattr(cs, "score_ground_truth", lambda gt_dir, c, o, n, seed, device=None, log=None: gts.append(
        (gt_dir, c, o, n, seed)) or (torch.zeros(n, 3), torch.ones(n, 3), 6 if o == "flat" else 0))
    t = lambda m: tuple(torch.from_numpy(np.ascontiguousarray(x)) for x in m)
    meshes = [t(MF.fans()), t(MF.empty()), t(MF.fans()) + (torch.zeros(8, 3),), t(MF.fans())]
    keys = [("03001627", "obj_a", 0), ("03001627", "obj_a", 1), ("03001627", "obj_a", 5), ("02958343", "obj_c", 2)]
    cache = {}
    rows = cs.score_group(meshes, keys, ("gt", 16), seed=9, cache=cache)
    assert gts == [("gt", "03001627", "obj_a", 16, 9), ("gt", "02958343", "obj_c", 16, 9)]      # once per object
    assert calls == [("sample", 3, 16, [M.mesh_seed(9, "03001627_obj_a_00.obj"), M.mesh_seed(9, "03001627_obj_a_05.obj"),
                                        M.mesh_seed(9, "02958343_obj_c_02.obj")]),
                     ("scores", (3, 16, 3), (3, 16, 3), 6)]
    assert [r["status"] for r in rows] == [0, None, 0, 0] and "chamfer_l1" not in rows[1]
    assert [r.get("gt_status") for r in rows] == [0, None, 0, 0]
    assert [r["chamfer_l1"] for r in rows if r["status"] == 0] == [2.0, 3.0, 4.0] and rows[3]["f_score"] == [0.5] * 6
    assert [(r["cat_id"], r["obj"], r["view"]) for r in rows] == keys and all(r["points"] == 16 for r in rows)
    cs.score_group(meshes[:1], keys[:1], ("gt", 16), seed=9, cache=cache)
    assert len(gts) == 2                                                             # cached
    assert cs.score_group([t(MF.empty())], keys[:1], ("gt", 16)) == [
        {"cat_id": "03001627", "obj": "obj_a", "view": 0, "points": 16, "status": None}] and len(calls) == 4
    # a group of more objects than the cache keeps between groups: every one of them is there when it is needed
    for count in (cs.SCORE_CACHE, cs.SCORE_CACHE + 1, 24):
        many = [("c", "o%d" % k, 0) for k in range(count)]
        del gts[:]
        fresh = [k[1] for k in many if k[:2] not in cache]
        rows = cs.score_group([meshes[0]] * count, many, ("gt", 4), cache=cache)
        assert [r["status"] for r in rows] == [0] * count and [g[2] for g in gts] == fresh     # each sampled once
        assert set(k[:2] for k in many) <= set(cache) and len(cache) <= max(count, cs.SCORE_CACHE)
    del gts[:]
    rows = cs.score_group(meshes[:1] * 2, [("c", "o23", 0), ("c", "flat", 1)], ("gt", 4), cache=cache)
    assert [g[2] for g in gts] == ["flat"] and [r["gt_status"] for r in rows] == [0, 6]         # o23 was kept
    assert set(cache) == {("c", "o23"), ("c", "flat")}                     # beyond the bound: only what the group needs


def test_a_ground_truth_without_area_is_logged(monkeypatch):
    import torch
    monkeypatch.setattr(E, "_device_mesh", lambda path, device=None: (torch.zeros(3, 3), torch.zeros((0, 3), dtype=torch.int32)))
    monkeypatch.setattr(M, "sample_surface_meshes_device", lambda m, n, s: (
        torch.zeros(1, n, 3), torch.zeros(1, n, 3), None, torch.tensor([6], dtype=torch.int32)))
    said = []
    pts, nrm, status = cs.score_ground_truth("gt", "03001627", "a1", 5, 0, log=said.append)
    assert status == 6 and pts.shape == nrm.shape == (5, 3)
    assert len(said) == 1 and "03001627/a1/isosurf.obj has no area" in said[0]


def test_driver_appends_one_score_line_per_mesh(monkeypatch, tmp_path):
    import torch
    view_num, seed = 3, 4
    entries = RF.expected_entries(seed, view_num)
    sdf_dir, rendered_dir = RF.build_dataset(str(tmp_path / "data"), entries, n_samples=32)
    lst_dir, log_dir = str(tmp_path / "lst"), str(tmp_path / "log")
    RF.write_lists(lst_dir)
    argv = ["--log_dir", log_dir, "--test_lst_dir", lst_dir, "--sdf_dir", sdf_dir, "--rendered_dir", rendered_dir,
            "--category", "chair,car", "--view_num", str(view_num), "--sdf_res", "8", "--seed", str(seed),
            "--batch_size", "5"]
    v, f = MF.fans()
    n = [0]

    def run(imgs, trans_mats, sdf_params):
        out = [MF.empty() if (n[0] + b) == 2 else (v, f) for b in range(imgs.shape[0])]
        n[0] += imgs.shape[0]
        return out

    plain = cs.main(argv, reconstruct_fn=run)
    assert "scored" not in plain and not os.path.exists(os.path.join(plain["out_dir"], "scores.jsonl"))
    calls = []
    _fake_device(monkeypatch, calls)
    monkeypatch.setattr(cs, "score_ground_truth", lambda gt_dir, c, o, k, s, device=None, log=None: (
        torch.zeros(k, 3), torch.ones(k, 3), 0))
    n[0] = 0
    res = cs.main(argv + ["--score", "gt", "--score_points", "8"], reconstruct_fn=run)
    assert res == dict(plain, scored=11)                                             # the same tree, the same counts
    rows = [json.loads(l) for l in open(os.path.join(res["out_dir"], "scores.jsonl"))]
    assert [(r["cat_id"], r["obj"], r["view"]) for r in rows] == [tuple(e) for e in entries]
    assert [r["status"] for r in rows] == [0, 0, None] + [0] * 9 and all(r["points"] == 8 for r in rows)
    assert all(set(M.SURFACE_SCORES) < set(r) for r in rows if r["status"] == 0)
    assert [c[1] for c in calls if c[0] == "sample"] == [4, 5, 2]                    # one call per group of 5, 5, 2
    # a run that scores every mesh again starts the file afresh; --skip_existing appends what it does now
    n[0] = 0
    cs.main(argv + ["--score", "gt", "--score_points", "8"], reconstruct_fn=run)
    assert [json.loads(l) for l in open(os.path.join(res["out_dir"], "scores.jsonl"))] == rows
    os.remove(cs.obj_path(res["out_dir"], *entries[0]))
    again = cs.main(argv + ["--score", "gt", "--score_points", "8", "--skip_existing"],
                    reconstruct_fn=lambda i, t, s: [(v, f)] * i.shape[0])
    assert again["scored"] == 2 and again["skipped"] == 10        # the removed file and the empty one (<= 200 bytes)
    lines = [json.loads(l) for l in open(os.path.join(res["out_dir"], "scores.jsonl"))]
    assert lines[:12] == rows and [(r["cat_id"], r["obj"], r["view"]) for r in lines[12:]] == [tuple(entries[0]),
                                                                                               tuple(entries[2])]


# ------------------------------------------------------------------ the fourth header
def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return re.findall(r"\b(disn_[a-z0-9_]+)\s*\(", text)


def test_fourth_header_equals_the_fourth_table_and_the_others_stay():
    from disn_amd import _lib
    assert _declared("disn_amd_sample.h") == list(NEW) == list(_lib.SIGNATURES_SAMPLE)
    assert not set(NEW) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_SIMPLIFY) | set(_lib.SIGNATURES_COLOUR))
    assert set(_declared("disn_amd.h")) == set(_lib.SIGNATURES)
    assert _declared("disn_amd_simplify.h") == list(_lib.SIGNATURES_SIMPLIFY)
    assert _declared("disn_amd_colour.h") == list(_lib.SIGNATURES_COLOUR)
    header = open(os.path.join(ROOT, "include", "disn_amd.h")).read()
    assert re.search(r"#define DISN_ABI_VERSION 10\b", header)
    assert not any(name in header for name in NEW) and "disn_mesh_sample" not in header
    assert '#include "disn_amd.h"' in open(os.path.join(ROOT, "include", "disn_amd_sample.h")).read()
    assert _lib.ABI_VERSION == 10 and _lib.lib().disn_abi_version() == 10
    h = _lib.lib()
    for name in NEW:
        fn = getattr(h, name)
        assert fn.restype is _lib.SIGNATURES_SAMPLE[name][0] and list(fn.argtypes) == _lib.SIGNATURES_SAMPLE[name][1]
    ws = h.disn_mesh_sample_workspace_bytes
    assert ws(24, 100000, 200000, 2048) >= 200000 * 8 and ws(1, 0, 0, 1) > 0 and ws(1, 10, 10, 2 ** 20) > 0
    assert ws(5, 10, 10 ** 6, 7) > ws(5, 10, 10, 7) == ws(5, 10 ** 6, 10, 2 ** 20)   # the faces' scan alone grows it
    for bad in ((0, 10, 10, 16), (-1, 10, 10, 16), (1, 10, 10, 0), (1, 10, 10, -5), (1, 10, 10, 2 ** 20 + 1),
                (1, 2 ** 31, 10, 16), (1, 10, (2 ** 31 - 1) // 3 + 1, 16), (1, -1, 10, 16), (1, 10, -1, 16)):
        assert ws(*bad) == 0, bad
    # argument checks that need no device
    off, bad_off = np.zeros(2, np.int64), np.array([0, -1], np.int64)
    seeds = np.zeros(1, np.uint64)
    o, s = off.ctypes.data, seeds.ctypes.data
    call = h.disn_mesh_sample_batch
    assert call(None, None, o, o, 1, s, 16, None, None, None, None, None, 0, None) == -1
    assert call(None, None, o, o, 1, None, 16, 1, None, None, 1, 1, 1 << 30, None) == -1        # no seeds
    assert call(None, None, bad_off.ctypes.data, o, 1, s, 16, 1, None, None, 1, 1, 1 << 30, None) == -1
    assert call(None, None, o, o, 0, s, 16, 1, None, None, 1, 1, 1 << 30, None) == -1
    some = np.array([0, 3], np.int64)
    assert call(None, None, some.ctypes.data, o, 1, s, 16, 1, None, None, 1, 1, 1 << 30, None) == -1   # no verts
    for n in (0, -1, 2 ** 20 + 1):
        assert call(None, None, o, o, 1, s, n, 1, None, None, 1, 1, 1 << 30, None) == -2
    assert call(None, None, o, o, 1, s, 16, 1, None, None, 1, 1, 16, None) == -3


def test_fourth_header_compiles_as_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "disn_amd_sample.h"\n'
                   "int main(void) {\n"
                   "  size_t (*ws)(int, int64_t, int64_t, int) = disn_mesh_sample_workspace_bytes;\n"
                   "  int (*run)(const float*, const int32_t*, const int64_t*, const int64_t*, int, const uint64_t*, int,\n"
                   "             float*, float*, int32_t*, int32_t*, void*, size_t, void*) = disn_mesh_sample_batch;\n"
                   "  return ws == 0 || run == 0 || DISN_ABI_VERSION != 10 || DISN_SAMPLE_NO_AREA != 6 ||\n"
                   "         DISN_SAMPLE_MAX_N != 1048576;\n"
                   "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I",
                        os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_build_lists_the_source_without_contraction_and_the_header():
    from disn_amd.csrc import build
    assert build.SOURCES["mesh_sample.hip"] == ["-ffp-contract=off"]
    assert any(h.endswith(os.path.join("include", "disn_amd_sample.h")) for h in build.HEADERS)

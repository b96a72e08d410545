"""GPU tests of the evaluation metrics (csrc/metrics.hip via disn_amd/metrics.py): nn_distance bit for bit
against the float32 restatement, approx_match / match_cost / emd against the float64 restatement, determinism,
batch invariance, an analytic case, and image-free end to end: SDF grid -> marching cubes -> sampled points ->
scores, and the evaluation driver on a small tree."""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import metrics_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _clouds(seed, b, n, m):
    rng = np.random.default_rng(seed)
    # a surface-like cloud pair: points near a unit sphere, the second perturbed
    def one(k):
        v = rng.standard_normal((b, k, 3))
        v /= np.linalg.norm(v, axis=2, keepdims=True)
        return (0.4 * v + 0.02 * rng.standard_normal((b, k, 3))).astype(np.float32)
    return one(n), one(m)


@pytest.mark.parametrize("b,n,m", [(1, 1, 1), (3, 2048, 2048), (2, 1000, 37), (1, 5000, 70000)])
def test_nn_distance_is_bit_exact(b, n, m):
    from disn_amd import metrics
    x1, x2 = _clouds(b * 7 + n + m, b, n, m)
    got = [t.cpu().numpy() for t in metrics.nn_distance(_dev(x1), _dev(x2))]
    ref = R.nn_distance(x1, x2)
    for name, g, r in zip(("dist1", "idx1", "dist2", "idx2"), got, ref):
        assert g.shape == r.shape, name
        assert np.array_equal(g, r), "%s: %d of %d differ" % (name, int((g != r).sum()), g.size)


def test_nn_ties_go_to_the_lowest_index_across_splits():
    from disn_amd import metrics
    m = 70000                                     # several workgroups split the reference set
    x1, x2 = _clouds(5, 1, 3000, m)
    x2[0, m - 3] = x2[0, 5]
    x1[0, :64] = x2[0, 5]
    d1, i1, _, _ = [t.cpu().numpy() for t in metrics.nn_distance(_dev(x1), _dev(x2))]
    assert (i1[0, :64] == 5).all() and (d1[0, :64] == 0).all()
    # the other direction: a query equidistant to two points of xyz1 far apart in index
    y1, y2 = _clouds(6, 1, 70000, 10)
    y1[0, 7] = y2[0, 0] + np.float32(0.25)
    y1[0, 69990] = y2[0, 0] + np.float32(0.25)
    y1[0, 69991] = y2[0, 0] - np.float32(0.25)
    _, _, d2, i2 = [t.cpu().numpy() for t in metrics.nn_distance(_dev(y1), _dev(y2))]
    ref = R.nn_distance(y1, y2)
    assert np.array_equal(i2, ref[3]) and np.array_equal(d2, ref[2])


def _check_match(match, x1, x2, cost_gpu=None):
    """the bar of the issue: cost rel <= 1e-5, L1 <= 1e-4 of sum, marginals within 1e-4 (float64 restatement)"""
    from disn_amd import metrics
    ref = R.approx_match(x1, x2)
    ref_cost = R.match_cost(x1, x2, ref)
    g = match.cpu().numpy().astype(np.float64)
    assert np.isfinite(g).all()
    for i in range(len(ref)):
        l1 = np.abs(g[i] - ref[i]).sum()
        assert l1 <= 1e-4 * ref[i].sum(), "pair %d: match L1 %g of %g" % (i, l1, ref[i].sum())
        assert np.abs(g[i].sum(0) - ref[i].sum(0)).max() <= 1e-4, "pair %d: row sums" % i
        assert np.abs(g[i].sum(1) - ref[i].sum(1)).max() <= 1e-4, "pair %d: column sums" % i
    cost = metrics.match_cost(_dev(x1), _dev(x2), match).cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(cost, ref_cost, rtol=1e-5)
    if cost_gpu is not None:
        np.testing.assert_allclose(cost_gpu.cpu().numpy().astype(np.float64), ref_cost, rtol=1e-5)
    return cost


@pytest.mark.parametrize("b,n,m", [(24, 512, 512), (2, 2048, 2048), (3, 2048, 1000), (2, 300, 2048), (1, 1, 1),
                                   (1, 7, 5)])
def test_approx_match_against_float64(b, n, m):
    from disn_amd import metrics
    x1, x2 = _clouds(b + n * 3 + m, b, n, m)
    match = metrics.approx_match(_dev(x1), _dev(x2))
    assert tuple(match.shape) == (b, m, n)
    _check_match(match, x1, x2)


@pytest.mark.parametrize("b,n,m", [(4, 2048, 2048), (2, 2048, 1000), (2, 300, 2048), (1, 7, 5), (1, 1, 1)])
def test_fused_emd_equals_match_cost_of_approx_match(b, n, m):
    from disn_amd import metrics
    x1, x2 = _clouds(11 + n + m, b, n, m)
    a, c = _dev(x1), _dev(x2)
    fused = metrics.emd(a, c)
    match = metrics.approx_match(a, c)
    two = _check_match(match, x1, x2, cost_gpu=fused)
    np.testing.assert_allclose(fused.cpu().numpy().astype(np.float64), two, rtol=1e-6)


def test_deterministic_and_batch_invariant():
    from disn_amd import metrics
    x1, x2 = _clouds(21, 24, 2048, 2048)
    a, c = _dev(x1), _dev(x2)
    nn1 = [t.cpu().numpy() for t in metrics.nn_distance(a, c)]
    nn2 = [t.cpu().numpy() for t in metrics.nn_distance(a, c)]
    m1, m2 = metrics.approx_match(a, c).cpu().numpy(), metrics.approx_match(a, c).cpu().numpy()
    e1, e2 = metrics.emd(a, c).cpu().numpy(), metrics.emd(a, c).cpu().numpy()
    k1 = metrics.match_cost(a, c, torch.from_numpy(m1).cuda()).cpu().numpy()
    assert all(np.array_equal(u, v) for u, v in zip(nn1, nn2))
    assert np.array_equal(m1, m2) and np.array_equal(e1, e2)
    for i in (0, 13, 23):
        ai, ci = a[i:i + 1].contiguous(), c[i:i + 1].contiguous()
        nn = [t.cpu().numpy() for t in metrics.nn_distance(ai, ci)]
        assert all(np.array_equal(u[i:i + 1], v) for u, v in zip(nn1, nn)), "nn pair %d" % i
        mi = metrics.approx_match(ai, ci).cpu().numpy()
        assert np.array_equal(mi, m1[i:i + 1]), "match pair %d" % i
        assert np.array_equal(metrics.emd(ai, ci).cpu().numpy(), e1[i:i + 1]), "emd pair %d" % i
        ki = metrics.match_cost(ai, ci, torch.from_numpy(mi).cuda()).cpu().numpy()
        assert np.array_equal(ki, k1[i:i + 1]), "match_cost pair %d" % i


def test_translated_lattice_analytic():
    """spacing 0.05 >> |t| ~ 2.7e-3: every point's neighbour is its own translate; Chamfer = 2|t|^2 * 1000,
    EMD = n |t| -- independent of the restatements"""
    from disn_amd import metrics
    ax = np.arange(16) * 0.05 - 0.4
    g = np.stack(np.meshgrid(ax, ax, ax[:8], indexing="ij"), -1).reshape(-1, 3)       # 2048 points
    t = np.array([1e-3, -2e-3, 1.5e-3])
    gt = g.astype(np.float32)
    pred = (g + t).astype(np.float32)
    d1, i1, d2, i2 = [u.cpu().numpy() for u in metrics.nn_distance(_dev(pred[None]), _dev(gt[None]))]
    assert np.array_equal(i1[0], np.arange(2048)) and np.array_equal(i2[0], np.arange(2048))
    cf = metrics.chamfer_views(_dev(pred[None]), _dev(gt)).cpu().numpy()[0]
    exact = 2 * ((pred.astype(np.float64) - gt) ** 2).sum(1).mean() * 1000          # of the float32 coordinates
    assert cf == pytest.approx(exact, rel=1e-5)
    assert cf == pytest.approx(2 * (t ** 2).sum() * 1000, rel=1e-3)
    cost = metrics.emd(_dev(gt[None]), _dev(pred[None])).cpu().numpy()[0]
    assert cost == pytest.approx(2048 * np.linalg.norm(t), rel=1e-3)
    assert metrics.emd_views(_dev(pred[None]), _dev(gt)).cpu().numpy()[0] == pytest.approx(cost * 0.01, rel=1e-6)


def _sphere_grid(R_, r, c=(0.0, 0.0, 0.0)):
    ax = np.linspace(-1, 1, R_ + 1)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    return (np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r).astype(np.float32)


BOX = [-1, -1, -1, 1, 1, 1]


def test_mesh_to_scores_end_to_end():
    from disn_amd import isosurface, metrics
    vg, _ = isosurface.marching_cubes(_dev(_sphere_grid(40, 0.5)), BOX, 40)
    preds = [isosurface.marching_cubes(_dev(_sphere_grid(32, 0.5 + 0.01 * i, (0.01 * i, 0, 0))), BOX, 32)[0]
             for i in range(3)]
    rng = np.random.default_rng(3)
    gt = metrics.sample_vertices(vg, 2048, rng)
    pred = torch.stack([metrics.sample_vertices(v, 2048, rng) for v in preds])
    assert gt.is_cuda and pred.is_cuda and pred.shape == (3, 2048, 3)
    # the same indices drawn on the host
    rng = np.random.default_rng(3)
    vg_h = vg.cpu().numpy()
    gt_h = vg_h[rng.integers(len(vg_h), size=2048)]
    pred_h = np.stack([v.cpu().numpy()[rng.integers(v.shape[0], size=2048)] for v in preds])
    assert np.array_equal(gt.cpu().numpy(), gt_h) and np.array_equal(pred.cpu().numpy(), pred_h)
    cf = metrics.chamfer_views(pred, gt).cpu().numpy()
    gt_t = np.repeat(gt_h[None], 3, 0)
    d1, _, d2, _ = R.nn_distance(pred_h, gt_t)
    np.testing.assert_allclose(cf, R.chamfer_views(d1, d2), rtol=1e-12)
    em = metrics.emd_views(pred, gt).cpu().numpy()
    np.testing.assert_allclose(em, R.match_cost(gt_t, pred_h, R.approx_match(gt_t, pred_h)) * 0.01, rtol=1e-5)
    # an empty mesh samples to zeros
    assert not metrics.sample_vertices(torch.zeros((0, 3), device="cuda"), 16, rng).any()


def _write_tree(root):
    from disn_amd import isosurface
    cat = "03001627"
    gt_dir, cal_dir, lst_dir = root / "gt", root / "cal", root / "lst"
    objs = ["objA", "objB"]
    for j, obj in enumerate(objs):
        v, f = isosurface.marching_cubes(_dev(_sphere_grid(32, 0.45 + 0.05 * j)), BOX, 32)
        isosurface.write_obj(str(gt_dir / cat / obj / "isosurf.obj"), v, f)
        for view in range(4):
            isosurface.create_obj(_dev(_sphere_grid(24, 0.45 + 0.05 * j + 0.01 * view, (0.01 * view, 0, 0))),
                                  BOX, str(cal_dir), cat, obj, view, 0.0)
    lst_dir.mkdir()
    (lst_dir / (cat + "_test.lst")).write_text("\n".join(objs) + "\n")
    return cat, str(gt_dir), str(cal_dir), str(lst_dir), objs


def test_driver_matches_direct_api_calls(tmp_path, capsys):
    from disn_amd import evaluate, isosurface, metrics
    cat, gt_dir, cal_dir, lst_dir, objs = _write_tree(tmp_path)
    args = ["--cal_dir", cal_dir, "--gt_dir", gt_dir, "--test_lst_dir", lst_dir, "--category", "chair",
            "--view_num", "3", "--num_sample_points", "512", "--seed", "7"]
    res = evaluate.main(["cd_emd"] + args)[cat]
    out = capsys.readouterr().out
    assert "cat_nm:chair, cat_id:%s" % cat in out and "avg cf:" in out
    rng, pyrng = np.random.default_rng(7), random.Random(7)
    fd = evaluate.build_file_dict(os.path.join(cal_dir, cat))
    sums = []
    for obj in objs:
        gt = metrics.sample_vertices(isosurface.read_obj_verts(os.path.join(gt_dir, cat, obj, "isosurf.obj")), 512, rng)
        views = pyrng.sample(fd[obj], 3)
        pred = torch.stack([metrics.sample_vertices(isosurface.read_obj_verts(p), 512, rng) for p in views])
        cf = metrics.chamfer_views(pred, gt).cpu().numpy()
        em = metrics.emd_views(pred, gt).cpu().numpy()
        r = res["objects"][obj]
        assert r["views"] == views
        assert np.array_equal(r["cf_views"], cf) and np.array_equal(r["emd_views"], em)
        assert (r["avg_cf"], r["min_cf"], r["arg_cf"]) == metrics.view_stats(cf)
        assert (r["avg_emd"], r["min_emd"], r["arg_emd"]) == metrics.view_stats(em)
        sums.append((cf.mean(), em.mean()))
    assert res["avg_cf"] == pytest.approx(sum(s[0] for s in sums) / 2, rel=1e-12)
    assert res["avg_emd"] == pytest.approx(sum(s[1] for s in sums) / 2, rel=1e-12)

    # F-score: objA from the reference's point files, objB sampled from its meshes
    pnt_dir = os.path.join(cal_dir, "pnt_512_%s" % cat)
    os.makedirs(pnt_dir)
    prng = np.random.default_rng(1)
    np.savetxt(os.path.join(gt_dir, cat, "objA", "pnt_512.txt"), prng.uniform(-.5, .5, (512, 3)), delimiter=",")
    for p in fd["objA"]:
        np.savetxt(os.path.join(pnt_dir, "pnt_objA_%s.txt" % p[-6:-4]), prng.uniform(-.5, .5, (512, 3)), delimiter=",")
    fres = evaluate.main(["f_score"] + args)
    t = metrics.f_score_thresholds(2.5)
    rng = np.random.default_rng(7)
    pres, recs = [], []
    for obj in objs:
        if obj == "objA":
            gt = np.loadtxt(os.path.join(gt_dir, cat, obj, "pnt_512.txt"), delimiter=",").astype(np.float32)
            pred = np.stack([np.loadtxt(os.path.join(pnt_dir, "pnt_objA_%s.txt" % p[-6:-4]), delimiter=",")
                             for p in fd[obj]]).astype(np.float32)
        else:
            v = isosurface.read_obj_verts(os.path.join(gt_dir, cat, obj, "isosurf.obj"))
            gt = v[rng.integers(len(v), size=512)]
            pred = []
            for p in fd[obj]:
                v = isosurface.read_obj_verts(p)
                pred.append(v[rng.integers(len(v), size=512)])
            pred = np.stack(pred)
        d1, _, d2, _ = [u.cpu().numpy() for u in
                        metrics.nn_distance(_dev(pred), _dev(np.repeat(gt[None], len(pred), 0)))]
        pre, rec = R.precision_recall(d1, d2, t)
        r = fres["categories"][cat]["objects"][obj]
        assert r["points"] == ("files" if obj == "objA" else "meshes")
        np.testing.assert_array_equal(r["precision"], pre)
        np.testing.assert_array_equal(r["recall"], rec)
        pres.append(pre)
        recs.append(rec)
    P, Rc = np.mean(pres, 0), np.mean(recs, 0)
    np.testing.assert_allclose(fres["precision"], P, rtol=1e-12)
    np.testing.assert_allclose(fres["f_score"], 2 * P * Rc / (P + Rc), rtol=1e-12)


def test_missing_prediction_names_the_object(tmp_path):
    from disn_amd import evaluate
    cat, gt_dir, cal_dir, lst_dir, objs = _write_tree(tmp_path)
    with open(os.path.join(lst_dir, cat + "_test.lst"), "a") as f:
        f.write("objMissing\n")
    with pytest.raises(FileNotFoundError, match="objMissing"):
        evaluate.main(["cd_emd", "--cal_dir", cal_dir, "--gt_dir", gt_dir, "--test_lst_dir", lst_dir,
                       "--category", "chair", "--view_num", "2", "--num_sample_points", "64"])

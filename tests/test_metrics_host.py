"""CPU tests of the evaluation metrics (disn_amd/metrics.py, disn_amd/evaluate.py): the numpy restatements
against brute-force loops, the scripts' aggregation arithmetic, the driver's parsing and the C entries' argument
checks.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import metrics_reference as R  # noqa: E402


def _cloud(rng, n):
    return rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)


def test_nn_restatement_equals_brute_force_loops():
    rng = np.random.default_rng(1)
    for n, m in ((1, 1), (7, 5), (13, 29)):
        a, c = _cloud(rng, n), _cloud(rng, m)
        c[m - 1] = c[0]                                         # a tie: the lowest index wins
        d, i = R.nn_one_way(a, c)
        for j in range(n):
            best, bi = np.float32(np.inf), -1
            for k in range(m):
                dx, dy, dz = c[k] - a[j]
                v = np.float32(np.float32(dx * dx + dy * dy) + dz * dz)
                if v < best:
                    best, bi = v, k
            assert d[j] == best and i[j] == bi


def _brute_match(x1, x2):
    n, m = len(x1), len(x2)
    mL, mR = (1.0, float(n // m)) if n >= m else (float(m // n), 1.0)
    remL, remR = [mL] * n, [mR] * m
    match = [[0.0] * n for _ in range(m)]
    d2 = [[float(sum((x2[l][t] - x1[k][t]) ** 2 for t in range(3))) for k in range(n)] for l in range(m)]
    for j in range(7, -3, -1):
        level = 0.0 if j == -2 else -(4.0 ** j)
        E = [[np.exp(level * d2[l][k]) for k in range(n)] for l in range(m)]
        ratioL = [remL[k] / (1e-9 + sum(E[l][k] * remR[l] for l in range(m))) for k in range(n)]
        ratioR = [0.0] * m
        for l in range(m):
            s = remR[l] * sum(E[l][k] * ratioL[k] for k in range(n))
            ratioR[l] = min(remR[l] / (s + 1e-9), 1.0) * remR[l]
            remR[l] = max(0.0, remR[l] - s)
        for k in range(n):
            tot = 0.0
            for l in range(m):
                w = E[l][k] * ratioL[k] * ratioR[l]
                match[l][k] += w
                tot += w
            remL[k] = max(0.0, remL[k] - tot)
    cost = sum(np.sqrt(d2[l][k]) * match[l][k] for l in range(m) for k in range(n))
    return np.asarray(match), cost


def test_approx_match_restatement_equals_brute_force_loops():
    rng = np.random.default_rng(2)
    for n, m in ((1, 1), (7, 5), (3, 8), (6, 6)):
        a, c = _cloud(rng, n), _cloud(rng, m)
        ref, cost = _brute_match(a.astype(np.float64), c.astype(np.float64))
        got = R.approx_match(a[None], c[None])[0]
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-15)
        assert abs(R.match_cost(a[None], c[None], got[None])[0] - cost) <= 1e-12 * max(1.0, cost)


@pytest.mark.parametrize("n,m", [(40, 40), (64, 25), (25, 64), (1, 9)])
def test_float64_match_respects_the_masses(n, m):
    rng = np.random.default_rng(n * 100 + m)
    a, c = _cloud(rng, n), _cloud(rng, m)
    mt = R.approx_match(a[None], c[None])[0]                     # [m, n]
    mL, mR = R.masses(n, m)
    assert (mt >= 0).all()
    assert (mt.sum(0) <= mL + 1e-9).all()                        # rows k: what xyz1[k] gave
    assert (mt.sum(1) <= mR + 1e-9).all()                        # columns l: what xyz2[l] received
    assert mt.sum() > 0.5 * min(n * mL, m * mR)                  # and most of the mass is matched


def test_masses_use_integer_division():
    assert R.masses(2048, 1000) == (1.0, 2.0)
    assert R.masses(300, 2048) == (6.0, 1.0)
    assert R.masses(7, 5) == (1.0, 1.0)
    assert len(R.LEVELS) == 10 and R.LEVELS[0] == -16384.0 and R.LEVELS[-2] == -0.25 and R.LEVELS[-1] == 0.0


def test_chamfer_precision_and_f_score_aggregation_by_hand():
    from disn_amd import metrics
    # two views of four points each: squared distances
    fwd = np.array([[0.0, 1e-4, 4e-4, 1.0], [1e-4, 1e-4, 9e-4, 0.25]], np.float32)
    bwd = np.array([[1e-4, 1e-4, 1e-4, 1e-4], [0.0, 0.0, 0.04, 0.01]], np.float32)
    cf = R.chamfer_views(fwd, bwd)
    assert cf[0] == pytest.approx((np.mean([0, 1e-4, 4e-4, 1.0]) + 1e-4) * 1000, rel=1e-6)
    assert cf[1] == pytest.approx((np.mean([1e-4, 1e-4, 9e-4, 0.25]) + np.mean([0, 0, 0.04, 0.01])) * 1000, rel=1e-6)
    # sqrt: fwd -> 0, .01, .02, 1, .01, .01, .03, .5 ; bwd -> .01 x4, 0, 0, .2, .1   (pooled over both views)
    t = np.array([0.01, 0.02, 0.1], np.float32)
    pre, rec = R.precision_recall(fwd, bwd, t)
    # strict <: a distance equal to the threshold (0.01 = sqrt(1e-4) in float32) is not counted
    s = np.sqrt(np.float32(1e-4))
    n_lt = lambda v, th: int((np.sqrt(np.asarray(v, np.float32)) < np.float32(th)).sum())   # noqa: E731
    assert pre[0] == n_lt(fwd, 0.01) / 8 and rec[2] == n_lt(bwd, 0.1) / 8
    assert pre[1] == (1 + 3 * (s < np.float32(0.02))) / 8           # 0 and the three 0.01's
    # categories: per-object averages, then averaged with weights = object counts
    cat_p = [np.array([0.5, 1.0]), np.array([0.25, 0.5])]
    cat_r = [np.array([1.0, 1.0]), np.array([0.5, 0.75])]
    p = metrics.weighted_category_average(cat_p, [3, 1])
    r = metrics.weighted_category_average(cat_r, [3, 1])
    np.testing.assert_allclose(p, [(3 * 0.5 + 0.25) / 4, (3 * 1.0 + 0.5) / 4])
    np.testing.assert_allclose(r, [(3 * 1.0 + 0.5) / 4, (3 * 1.0 + 0.75) / 4])
    np.testing.assert_allclose(metrics.f_score(p, r), 2 * p * r / (p + r))
    assert metrics.view_stats([3.0, 1.0, 2.0, 1.0]) == (1.75, 1.0, 1)    # argmin: the first minimum


def test_thresholds_scale_like_the_script():
    from disn_amd import metrics
    t = metrics.f_score_thresholds(2.5)
    assert t.dtype == np.float32
    ref = np.asarray([[0.5], [1], [2], [5], [10], [20]], dtype=np.float32) * 0.01 * 2.5
    assert np.array_equal(t, ref.reshape(-1))
    assert metrics.f_score_thresholds(1.0)[1] == np.float32(0.01)


def test_build_file_dict_and_categories(tmp_path):
    from disn_amd import evaluate
    d = tmp_path / "03001627"
    d.mkdir()
    for fn in ("03001627_objA_00.obj", "03001627_objA_01.obj", "03001627_objB_00.obj"):
        (d / fn).write_text("v 0 0 0\n")
    (d / "sub_objC_00").mkdir()                                # directories are not predictions
    fd = evaluate.build_file_dict(str(d))
    assert sorted(fd) == ["objA", "objB"]
    assert [os.path.basename(p) for p in fd["objA"]] == ["03001627_objA_00.obj", "03001627_objA_01.obj"]
    assert len(evaluate.categories("all")) == 13
    assert set(evaluate.categories("clean").values()) == {"02933112", "03211117", "03691459", "04090263", "04530566"}
    assert evaluate.categories("chair") == {"chair": "03001627"}
    with pytest.raises(ValueError):
        evaluate.categories("teapot")
    with pytest.raises(FileNotFoundError, match="objZ"):
        evaluate._predictions(fd, "objZ", "03001627", str(d))
    lst = tmp_path / "l.lst"
    lst.write_text("objA\r\nobjB\n\n")
    assert evaluate.read_list(str(lst)) == ["objA", "objB"]


def test_evaluate_help_runs_without_a_gpu():
    for args in ([], ["cd_emd"], ["f_score"]):
        r = subprocess.run([sys.executable, "-m", "disn_amd.evaluate"] + args + ["--help"], cwd=ROOT,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
    assert "--truethreshold" in r.stdout and "--num_sample_points" in r.stdout


def test_metrics_entries_validate_arguments_without_gpu():
    from disn_amd import _lib
    h = _lib.lib()
    assert h.disn_metrics_workspace_bytes(0, 5, 5) == 0
    assert h.disn_metrics_workspace_bytes(24, 2048, 2048) >= 24 * 4096 * 8
    assert h.disn_metrics_workspace_bytes(2, 1000, 2000) > h.disn_metrics_workspace_bytes(1, 1000, 2000)
    ws = h.disn_metrics_workspace_bytes(2, 10, 20)
    assert h.disn_nn_distance(None, 1, 2, 10, 20, 1, 1, 1, 1, 1, ws, None) == -1
    assert h.disn_nn_distance(1, 1, 2, 0, 20, 1, 1, 1, 1, 1, ws, None) == -1
    assert h.disn_nn_distance(1, 1, 2, 10, 20, 1, 1, 1, 1, 1, ws - 1, None) == -3
    assert h.disn_approx_match(1, 1, 2, 10, -1, 1, 1, ws, None) == -1
    assert h.disn_approx_match(1, 1, 2, 10, 20, 1, 1, 16, None) == -3
    assert h.disn_approx_match(1, 1, 70000, 10, 20, 1, 1, 1 << 40, None) == -2
    assert h.disn_match_cost(1, 1, None, 2, 10, 20, 1, 1, ws, None) == -1
    assert h.disn_match_cost(1, 1, 1, 2, 10, 20, 1, 1, 0, None) == -3
    assert h.disn_emd(1, 1, 2, 10, 20, None, 1, ws, None) == -1
    assert h.disn_emd(1, 1, 2, 10, 20, 1, 1, ws // 2, None) == -3
    assert h.disn_read_obj_verts(b"/nonexistent/x.obj", None, 0) == -1


def test_obj_vertex_reader_matches_read_obj(tmp_path):
    from disn_amd import isosurface
    rng = np.random.default_rng(3)
    v = rng.standard_normal((1000, 3)).astype(np.float32)
    f = rng.integers(0, 1000, (500, 3)).astype(np.int32)
    p = str(tmp_path / "m.obj")
    isosurface.write_obj(p, v, f)
    got = isosurface.read_obj_verts(p)
    assert np.array_equal(got, isosurface.read_obj(p)[0]) and np.array_equal(got, v)
    (tmp_path / "e.obj").write_text("# nothing\n")
    assert isosurface.read_obj_verts(str(tmp_path / "e.obj")).shape == (0, 3)
    (tmp_path / "b.obj").write_text("v 1 2\n")
    with pytest.raises(OSError):
        isosurface.read_obj_verts(str(tmp_path / "b.obj"))


def test_cpu_tensors_are_refused():
    import torch
    from disn_amd import metrics
    a = torch.zeros((1, 4, 3))
    for fn, args in ((metrics.nn_distance, (a, a)), (metrics.approx_match, (a, a)), (metrics.emd, (a, a)),
                     (metrics.match_cost, (a, a, torch.zeros((1, 4, 4)))), (metrics.chamfer_views, (a, a[0]))):
        with pytest.raises(TypeError):
            fn(*args)


def test_driver_names_a_missing_prediction_before_any_work(tmp_path):
    from disn_amd import evaluate
    cat = "03001627"
    (tmp_path / "cal" / cat).mkdir(parents=True)
    (tmp_path / "cal" / cat / (cat + "_objA_00.obj")).write_text("v 0 0 0\n")
    (tmp_path / "lst").mkdir()
    (tmp_path / "lst" / (cat + "_test.lst")).write_text("objA\nobjMissing\n")
    for cmd in ("cd_emd", "f_score"):
        with pytest.raises(FileNotFoundError, match="objMissing"):
            evaluate.main([cmd, "--cal_dir", str(tmp_path / "cal"), "--gt_dir", str(tmp_path / "gt"),
                           "--test_lst_dir", str(tmp_path / "lst"), "--category", "chair", "--view_num", "1"])

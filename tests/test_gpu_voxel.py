"""GPU tests of voxel IoU (csrc/voxel.hip via disn_amd/voxel.py): surface bits, index grid and filled bits bit for
bit against tests/voxel_reference.py, the IoU counts, determinism, the key-range error, the evaluation driver in
both modes, and the file-free chain marching cubes -> small-part cleanup -> IoU."""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import voxel_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BOX = [-1, -1, -1, 1, 1, 1]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _blob_grid(res, blobs):
    """the SDF of a union of spheres [(radius, centre), ...] at the (res+1)^3 nodes of [-1, 1]^3, .dist order"""
    ax = np.linspace(-1, 1, res + 1)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    d = [np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r for r, c in blobs]
    return np.minimum.reduce(d).astype(np.float32)


def _mc(res, blobs):
    from disn_amd import isosurface
    v, f = isosurface.marching_cubes(_dev(_blob_grid(res, blobs)), BOX, res)
    return v, f


def _soup(seed, n_small, n_big):
    """small triangles (about a cell wide) and very large ones (spanning much of the grid) mixed"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-0.8, 0.8, (n_small, 1, 3))
    small = c + rng.normal(0.0, 0.012, (n_small, 3, 3))
    big = rng.uniform(-0.95, 0.95, (n_big, 3, 3))
    tri = np.concatenate([small, big])[rng.permutation(n_small + n_big)].astype(np.float32)
    return tri.reshape(-1, 3), np.arange(3 * tri.shape[0], dtype=np.int32).reshape(-1, 3)


def _degenerate():
    """repeated vertices, collinear vertices, a point triangle, among ordinary ones"""
    v = np.array([[0.1, 0.1, 0.1], [0.5, 0.12, 0.1], [0.3, 0.4, 0.15],
                  [-0.5, -0.5, -0.5], [0.5, 0.5, 0.5], [0.0, 0.0, 0.0],          # collinear
                  [0.3, -0.3, 0.2], [-0.4, 0.6, -0.1]], np.float32)
    f = np.array([[0, 1, 2], [3, 4, 5], [3, 3, 4], [6, 6, 6], [7, 6, 7], [0, 2, 1], [5, 5, 5]], np.int32)
    return v, f


def _cases():
    h = R.cell_size(110)
    yield "soup", _soup(1, 3000, 6), 110
    yield "soup_dim64", _soup(2, 500, 3), 64
    yield "cube_27.2", R.cube(np.float32(27.2) * h), 110
    yield "cube_20.2", R.cube(np.float32(20.2) * h), 110
    v, f = _mc(64, [(0.55, (0.0, 0.0, 0.0))])
    yield "mc_sphere", (v.cpu().numpy(), f.cpu().numpy()), 110
    yield "degenerate", _degenerate(), 110
    yield "empty", (np.zeros((4, 3), np.float32), np.zeros((0, 3), np.int32)), 110
    yield "one_triangle", (np.array([[0.1, 0.2, 0.3], [0.4, 0.2, 0.3], [0.1, 0.5, 0.35]], np.float32),
                           np.array([[0, 1, 2]], np.int32)), 110        # nv = 3, nf = 1: the smallest soup with a face


@pytest.mark.parametrize("case", ["soup", "soup_dim64", "cube_27.2", "cube_20.2", "mc_sphere", "degenerate", "empty",
                                  "one_triangle"])
def test_bits_equal_the_restatement(case):
    from disn_amd import voxel
    (v, f), dim = next((m, d) for n, m, d in _cases() if n == case)
    ref, ovf = R.surface_voxels(v, f, dim)
    assert not ovf
    vox = voxel.surface_voxels(_dev(v), torch.from_numpy(f).cuda(), dim)
    got = voxel.to_dense(vox)
    assert got.shape == ref.shape == (vox.n,) * 3 and (vox.kmin, vox.n) == R.key_range(dim)
    print("%s: %d triangles, %d surface voxels" % (case, f.shape[0], int(ref.sum())))
    assert np.array_equal(got, ref), "%d surface bits differ" % int((got != ref).sum())
    idx = voxel.to_dense(voxel.index_grid(vox))
    assert idx.shape == (dim,) * 3 and np.array_equal(idx, R.index_grid(ref, dim))
    assert np.array_equal(voxel.to_dense(voxel.fill(vox)), R.fill(ref))
    if case == "empty":
        assert not got.any() and not idx.any()
    if case.startswith("cube"):
        shell, solid = {"cube_27.2": (17498, 166375), "cube_20.2": (9602, 68921)}[case]
        assert int(got.sum()) == shell and voxel.fill(vox).count() == solid
    # the padding bits of every row stay clear
    w = vox.words.cpu().numpy().view(np.uint32).reshape(-1, vox.wpr)
    assert not (w[:, -1] >> np.uint32(vox.n & 31)).any()
    # host arrays are accepted too, and give the same bits
    assert torch.equal(voxel.surface_voxels(v, f, dim).words, vox.words)


def test_solid_iou_of_the_two_cubes():
    from disn_amd import voxel
    h = R.cell_size(110)
    big, small = R.cube(np.float32(27.2) * h), R.cube(np.float32(20.2) * h)
    iou, inter, union = voxel.iou_views(big, [small, big], mode="solid")
    assert inter.tolist() == [68921, 166375] and union.tolist() == [166375, 166375]
    assert iou[0] == 68921 / 166375 and iou[1] == 1.0
    assert inter.dtype == np.int64 and union.dtype == np.int64 and iou.dtype == np.float64


def _perturbed_views(n):
    v, f = _mc(40, [(0.5, (0.0, 0.0, 0.0)), (0.25, (0.45, 0.1, 0.0))])
    v, f = v.cpu().numpy(), f.cpu().numpy()
    rng = np.random.default_rng(11)
    views = []
    for i in range(n):
        s = np.float32(1.0 + 0.02 * rng.standard_normal())
        t = (0.02 * rng.standard_normal(3)).astype(np.float32)
        views.append(((v * s + t + (0.004 * rng.standard_normal(v.shape)).astype(np.float32)).astype(np.float32), f))
    return (v, f), views


def _mode_grid(surface, dim, mode):
    return R.index_grid(surface, dim) if mode == "reference" else R.fill(surface)


def test_iou_of_24_views_equals_the_restatement_and_repeats():
    from disn_amd import voxel
    gt, views = _perturbed_views(24)
    sg, ovf = R.surface_voxels(gt[0], gt[1], 110)
    assert not ovf
    sv = [R.surface_voxels(v, f, 110)[0] for v, f in views]       # (restated once, counted in both modes)
    dev = [(_dev(v), torch.from_numpy(f).cuda()) for v, f in views]
    for mode in ("reference", "solid"):
        g = _mode_grid(sg, 110, mode)
        want = [R.iou_counts(g, _mode_grid(s, 110, mode)) for s in sv]
        iou, inter, union = voxel.iou_views(gt, views, mode=mode)
        print(mode, "iou min %.4f max %.4f" % (iou.min(), iou.max()))
        assert inter.tolist() == [w[0] for w in want] and union.tolist() == [w[1] for w in want]
        assert iou.tolist() == [float(a) / b for a, b in want]
        assert 0.0 < iou.min() and iou.max() < 1.0                # perturbed copies: neither disjoint nor equal
        # device tensors in, a second run: identical results
        iou2, inter2, union2 = voxel.iou_views((_dev(gt[0]), torch.from_numpy(gt[1]).cuda()), dev, mode=mode)
        assert np.array_equal(iou, iou2) and np.array_equal(inter, inter2) and np.array_equal(union, union2)
        # a mesh against itself
        iou1, inter1, union1 = voxel.iou_views(gt, [gt], mode=mode)
        assert iou1[0] == 1.0 and inter1[0] == union1[0] > 0
    a = voxel.surface_voxels(*dev[0])
    b = voxel.surface_voxels(*dev[0])
    assert torch.equal(a.words, b.words) and torch.equal(voxel.index_grid(a).words, voxel.index_grid(b).words)
    assert torch.equal(voxel.fill(a).words, voxel.fill(b).words)


def test_errors_name_the_mesh():
    from disn_amd import voxel
    v, f = R.cube(0.5)
    kmin, n = voxel.key_range(110)
    assert (kmin, n) == (-60, 131)
    far = (v + np.array([1.0, 0, 0], np.float32), f)            # reaches x = 1.5, past key 70 (x <= 1.28)
    with pytest.raises(ValueError, match="view_07.*key range"):
        voxel.iou_views((v, f), [(v, f), far], names=["gt.obj", "view_03.obj", "view_07.obj"])
    with pytest.raises(ValueError, match="prediction 1"):
        voxel.iou_views((v, f), [(v, f), far], mode="solid")
    with pytest.raises(ValueError, match="the ground truth"):
        voxel.iou_views(far, [(v, f)])
    with pytest.raises(ValueError, match="odd.obj"):
        voxel.surface_voxels(v - np.float32(0.7), f, name="odd.obj")      # reaches -1.2, below key -60 (x >= -1.1)
    nan = v.copy()
    nan[3, 1] = np.nan
    with pytest.raises(ValueError, match="key range"):
        voxel.surface_voxels(nan, f)
    with pytest.raises(ValueError, match="face index"):
        voxel.surface_voxels(v, f + 1)
    # the restatement calls the same meshes out of range, and the ones just inside in range
    assert R.surface_voxels(far[0], f, 110)[1] and R.surface_voxels(v - np.float32(0.7), f, 110)[1]
    edge = (v * np.float32(2.0) + np.float32(0.09), f)           # -0.91 .. 1.09
    assert not R.surface_voxels(edge[0], f, 110)[1]
    assert np.array_equal(voxel.to_dense(voxel.surface_voxels(*edge)), R.surface_voxels(edge[0], f, 110)[0])
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    with pytest.raises(ValueError, match="occupy no voxel"):
        voxel.iou_views(empty, [empty])
    with pytest.raises(ValueError, match="mode"):
        voxel.iou_views((v, f), [(v, f)], mode="shell")


def _write_tree(root):
    from disn_amd import isosurface
    cats = {"chair": "03001627", "lamp": "03636649"}
    gt_dir, cal_dir, lst_dir = root / "gt", root / "cal", root / "lst"
    lst_dir.mkdir()
    for ci, cat in enumerate(cats.values()):
        objs = ["objA", "objB"]
        for j, obj in enumerate(objs):
            r = 0.4 + 0.05 * j + 0.03 * ci
            v, f = _mc(32, [(r, (0.0, 0.0, 0.0))])
            isosurface.write_obj(str(gt_dir / cat / obj / "isosurf.obj"), v, f)
            for view in range(4):
                isosurface.create_obj(_dev(_blob_grid(24, [(r + 0.01 * view, (0.01 * view, 0, 0))])), BOX,
                                      str(cal_dir), cat, obj, view, 0.0)
        # a stub below the reference's 200-byte filter is not a prediction
        (cal_dir / cat / ("%s_objA_09.obj" % cat)).write_text("v 0 0 0\n")
        (lst_dir / (cat + "_test.lst")).write_text("\n".join(objs) + "\n")
    return cats, str(gt_dir), str(cal_dir), str(lst_dir)


def test_iou_command_reproduces_the_restatement(tmp_path, capsys):
    from disn_amd import evaluate, mesh_sdf
    cats, gt_dir, cal_dir, lst_dir = _write_tree(tmp_path)
    surfaces = {}

    def grid(path, mode):
        if path not in surfaces:
            surfaces[path], ovf = R.surface_voxels(*mesh_sdf.read_obj_mesh(path), 110)
            assert not ovf
        return _mode_grid(surfaces[path], 110, mode)

    for mode in ("reference", "solid"):
        res = {}
        for name in cats:                                        # (one category per call, as --category allows)
            res.update(evaluate.main(["iou", "--cal_dir", cal_dir, "--gt_dir", gt_dir, "--test_lst_dir", lst_dir,
                                      "--category", name, "--view_num", "3", "--mode", mode, "--seed", "5"]))
        out = capsys.readouterr().out
        assert out.count("obj_id iou avg: ") == 4 and out.count("done!") == 2
        for name, cat in cats.items():
            pyrng = random.Random(5)
            fd = evaluate.build_file_dict(os.path.join(cal_dir, cat), min_size=200)
            assert all(len(v) == 4 for v in fd.values())
            sums = []
            for obj in ("objA", "objB"):
                views = pyrng.sample(fd[obj], 3)
                r = res[cat]["objects"][obj]
                assert r["views"] == views
                g = grid(os.path.join(gt_dir, cat, obj, "isosurf.obj"), mode)
                want = [R.iou_counts(g, grid(p, mode)) for p in views]
                assert [(int(a), int(b)) for a, b in zip(r["inter"], r["union"])] == want
                v64 = [float(a) / b for a, b in want]
                v32 = np.asarray(v64, dtype=np.float32)
                ind = int(np.argmax(v32))
                assert r["avg_iou"] == float(np.mean(v32)) and r["best"] == [v64[ind], views[ind]]
                sums.append(float(np.sum(v32)))
            want_avg = (sums[0] + sums[1]) / 6.0
            assert res[cat]["iou_avg"] == want_avg and res[cat]["count"] == 6
            assert "cat_nm: %s, cat_id: %s, iou_avg: %s" % (name, cat, want_avg) in out
    with pytest.raises(ValueError, match="view_num"):
        evaluate.main(["iou", "--cal_dir", cal_dir, "--gt_dir", gt_dir, "--test_lst_dir", lst_dir,
                       "--category", "chair", "--view_num", "5"])
    # the older sub-commands parse what they parsed
    a = evaluate.parser().parse_args(["cd_emd", "--cal_dir", "c", "--gt_dir", "g", "--test_lst_dir", "l",
                                      "--view_num", "3", "--num_sample_points", "512", "--seed", "7"])
    assert (a.command, a.category, a.view_num, a.num_sample_points, a.truethreshold, a.seed) == \
        ("cd_emd", "all", 3, 512, 2.5, 7)
    assert not hasattr(a, "dim") and not hasattr(a, "mode")
    a = evaluate.parser().parse_args(["f_score", "--cal_dir", "c", "--gt_dir", "g", "--test_lst_dir", "l"])
    assert (a.view_num, a.num_sample_points, a.truethreshold, a.seed) == (24, 2048, 2.5, 0)


@pytest.mark.parametrize("mode", ["reference", "solid"])
def test_marching_cubes_to_cleanup_to_iou_without_files(mode):
    from disn_amd import postprocess, voxel
    big = (0.45, (0.0, 0.0, 0.0))
    both_v, both_f = _mc(48, [big, (0.1, (0.75, 0.0, 0.0))])    # two blobs of unequal size, apart
    labels, counts = postprocess.separate_mesh(both_v, both_f)
    assert counts.size == 2 and counts.min() < 0.3 * counts.max()
    cv, cf, kept = postprocess.clean_arrays(both_v, both_f)     # through host arrays; the small blob goes
    assert len(kept) == 1 and cv.shape[0] == counts.max()
    gv, gf = _mc(48, [big])                                     # device tensors, as marching_cubes returns them
    iou, inter, union = voxel.iou_views((gv, gf), [(cv, cf), (both_v, both_f)], mode=mode)
    assert iou[0] == 1.0 and inter[0] == union[0]
    assert iou[1] < 1.0 and inter[1] == inter[0] and union[1] > union[0]

"""CPU tests of the voxel IoU definitions (tests/voxel_reference.py, disn_amd/voxel.py's host parts) and of the
small-part cleanup (disn_amd/postprocess.py, disn_mesh_components): analytic voxel counts, the float32 overlap test
against its float64 twin, the corner lookup table against the reference's literal expression, component labelling
and the keep rule, and the clean command on a small tree."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import voxel_reference as R  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _built():
    from disn_amd.csrc import build
    build.build()


def test_cube_voxel_counts_are_the_analytic_ones():
    """half side 27.2 h: keys -27..27 touch the faces -> 55^3 - 53^3 shell voxels, 55^3 solid; 20.2 h: 41^3 - 39^3, 41^3"""
    h = R.cell_size(110)
    solids = []
    for half, shell, solid in ((27.2, 17498, 166375), (20.2, 9602, 68921)):
        v, f = R.cube(np.float32(half) * h)
        s32, ovf = R.surface_voxels(v, f, 110, np.float32)
        s64, _ = R.surface_voxels(v, f, 110, np.float64)
        assert not ovf and np.array_equal(s32, s64)
        assert int(s32.sum()) == shell
        filled = R.fill(s32)
        assert int(filled.sum()) == solid
        solids.append(filled)
    inter, union = R.iou_counts(solids[0], solids[1])
    assert (inter, union) == (68921, 166375)


def test_float32_overlap_agrees_with_float64_outside_the_borderline_cells():
    """20 000 seeded triangles, the 8x8x8 block of keys from one below the rounded minimum corner: a cell is
    borderline when some float64 axis has |min - r| or |max + r| < 1e-7; elsewhere float32 == float64 exactly,
    and at most 1 % of the cells are left out"""
    dim, T = 110, 20000
    rng = np.random.default_rng(0)
    centre = rng.uniform(-0.9, 0.9, (T, 1, 3))
    tri = (centre + rng.normal(0.0, 0.03, (T, 3, 3))).astype(np.float32)
    h = float(R.cell_size(dim, np.float64))
    start = np.rint(tri.min(1).astype(np.float64) / h).astype(np.int64) - 1
    off = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3)
    cells = border = differ = differ_inside = occupied = 0
    for s in range(0, T, 500):
        keys = start[s:s + 500, None, :] + off[None]
        t = tri[s:s + 500, None]
        a32 = R.overlap(t, keys, dim, np.float32)
        a64 = R.overlap(t, keys, dim, np.float64)
        b = R.borderline(t, keys, dim)
        cells += a32.size
        border += int(b.sum())
        differ += int(((a32 != a64) & ~b).sum())
        differ_inside += int(((a32 != a64) & b).sum())
        occupied += int(a64.sum())
    share = border / cells
    print("borderline share %.4f %% of %d cells (%d occupied); float32 != float64: %d outside, %d inside"
          % (100 * share, cells, occupied, differ, differ_inside))
    assert cells == T * 512 and occupied > T
    assert differ == 0
    assert share <= 0.01


@pytest.mark.parametrize("dim", [110, 64, 32])
def test_corner_table_is_the_reference_expression(dim):
    from disn_amd import voxel
    kmin, lut = voxel.corner_lut(dim)
    assert (kmin, lut.size - 1) == R.key_range(dim) == voxel.key_range(dim)
    keys = np.arange(kmin, kmin + lut.size - 1)
    for j, s in enumerate((-0.5, 0.5)):
        corners = (keys + s) * (2.0 / dim)                       # explicit float64 corner coordinates
        val = (corners + 1.1) / 2.4 * dim
        assert (val >= 0).all() and (val < dim).all()
        assert np.array_equal(((corners + 1.1) / 2.4 * dim).astype(int), lut[keys - kmin + j])
    # one key further on either side, a corner leaves the array
    for k, s in ((kmin - 1, -0.5), (kmin + lut.size - 1, 0.5)):
        val = ((k + s) * (2.0 / dim) + 1.1) / 2.4 * dim
        assert val < 0 or val >= dim
    assert lut.min() >= 0 and lut.max() < dim and (np.diff(lut) >= 0).all()
    if dim == 110:
        # meshes inside the unit sphere: the 115 corner numbers -57 .. 57 (coordinates -1.045 .. 1.027)
        n = np.arange(-57, 58)
        inner = lut[n - kmin]
        assert inner.size == 115 and (inner.min(), inner.max()) == (2, 97)
        assert np.bincount(inner).max() <= 2
        n = n.astype(np.float64)                                 # other ways to form the corner coordinate
        for c in ((n - 0.5) * (2.0 / dim), n * (2.0 / dim) - 1.0 / dim, (2.0 * n - 1.0) / dim):
            assert np.array_equal(((c + 1.1) / 2.4 * dim).astype(int), inner)


def _two_spheres():
    v0, f0 = R.icosphere(0.3, 2)                                # 162 vertices
    v1, f1 = R.icosphere(0.05, 1, (0.6, 0.0, 0.0))              # 42 vertices, apart from the first
    return v0, f0, v1, f1


def test_components_of_two_separated_spheres_and_the_keep_rule():
    from disn_amd import postprocess
    v0, f0, v1, f1 = _two_spheres()
    v = np.concatenate([v1, v0])
    f = np.concatenate([f1, f0 + v1.shape[0]])
    labels, counts = postprocess.separate_mesh(v, f)
    assert counts.tolist() == [42, 162]
    assert (labels[:f1.shape[0]] == 0).all() and (labels[f1.shape[0]:] == 1).all()
    cv, cf, kept = postprocess.clean_arrays(v, f)               # 42 < 0.3 * 162: the small sphere goes
    assert kept == [1] and np.array_equal(cv, v0) and np.array_equal(cf, f0)
    cv, cf, kept = postprocess.clean_arrays(v, f, num_thresh=0.2)        # 42 > 32.4, but its centroid is 0.6 away
    assert kept == [1]
    cv, cf, kept = postprocess.clean_arrays(v, f, dist_thresh=0.7, num_thresh=0.2)
    assert kept == [0, 1] and np.array_equal(cv, v) and np.array_equal(cf, f)
    with pytest.raises(ValueError, match="no part is kept"):
        postprocess.clean_arrays(v + np.float32(2.0), f)
    with pytest.raises(ValueError, match="out of range"):
        postprocess.separate_mesh(v, f + 1)


def test_fans_meeting_in_one_vertex_and_an_unreferenced_vertex():
    from disn_amd import postprocess
    # vertex 0 is shared by two fans; vertex 7 is referenced by nothing
    v = np.array([[0, 0, 0], [0.1, 0, 0], [0.1, 0.1, 0], [0, 0.1, 0], [-0.1, 0, 0], [-0.1, -0.1, 0], [0, -0.1, 0],
                  [0.4, 0.4, 0.4]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3], [0, 4, 5], [0, 5, 6]], np.int32)
    labels, counts = postprocess.separate_mesh(v, f, "face")
    assert labels.tolist() == [0, 0, 1, 1] and counts.tolist() == [4, 4]
    labels, counts = postprocess.separate_mesh(v, f, "vertex")
    assert labels.tolist() == [0, 0, 0, 0] and counts.tolist() == [7]
    cv, cf, kept = postprocess.clean_arrays(v, f)
    assert kept == [0, 1]
    assert cv.shape == (8, 3)                                   # vertex 0 once per part, vertex 7 dropped
    assert np.array_equal(cv, v[[0, 1, 2, 3, 0, 4, 5, 6]])
    assert cf.tolist() == [[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]]
    cv, cf, kept = postprocess.clean_arrays(v, f, connectivity="vertex")
    assert kept == [0] and np.array_equal(cv, v[:7]) and np.array_equal(cf, f)
    with pytest.raises(ValueError):
        postprocess.separate_mesh(v, f, "auto")
    labels, counts = postprocess.separate_mesh(v, np.zeros((0, 3), np.int32))
    assert labels.size == 0 and counts.size == 0


@pytest.mark.parametrize("connectivity", ["face", "vertex"])
def test_native_labelling_equals_the_python_union_find(connectivity):
    from disn_amd import postprocess
    rng = np.random.default_rng(5)
    for nv, nf in ((40, 30), (300, 150), (2000, 1500), (50, 400)):
        f = rng.integers(0, nv, (nf, 3)).astype(np.int32)       # a soup: repeated vertices and shared edges occur
        f[::7, 1] = f[::7, 0]
        labels, counts = postprocess.separate_mesh(np.zeros((nv, 3), np.float32), f, connectivity)
        ref, n = R.components(f, nv, connectivity)
        assert np.array_equal(labels, ref) and counts.size == n
        assert counts.tolist() == [np.unique(f[ref == c]).size for c in range(n)]
    v0, f0, v1, f1 = _two_spheres()
    perm = rng.permutation(f0.shape[0] + f1.shape[0])
    f = np.concatenate([f0, f1 + v0.shape[0]])[perm]
    labels, _ = postprocess.separate_mesh(np.concatenate([v0, v1]), f, connectivity)
    ref, n = R.components(f, v0.shape[0] + v1.shape[0], connectivity)
    assert n == 2 and np.array_equal(labels, ref) and labels[0] == 0


def test_clean_command_on_a_small_tree(tmp_path, capsys):
    from disn_amd import evaluate, isosurface, mesh_sdf, postprocess
    v0, f0, v1, f1 = _two_spheres()
    both_v, both_f = np.concatenate([v0, v1]), np.concatenate([f0, f1 + v0.shape[0]])
    src, tar = tmp_path / "src", tmp_path / "tar"
    cats = evaluate.CATS_CLEAN
    for cat_id in cats.values():
        isosurface.write_obj(str(src / cat_id / ("%s_obj1_00.obj" % cat_id)), both_v, both_f)
        isosurface.write_obj(str(src / cat_id / ("%s_obj1_01.obj" % cat_id)), v0, f0)
    n = postprocess.main(["--src_dir", str(src), "--tar_dir", str(tar)])
    out = capsys.readouterr().out
    assert n == 2 * len(cats) and out.count("threshes:") == n and out.rstrip().endswith("done!")
    for cat_id in cats.values():
        for view in ("00", "01"):
            v, f = mesh_sdf.read_obj_mesh(str(tar / cat_id / ("%s_obj1_%s.obj" % (cat_id, view))))
            assert np.array_equal(v, v0) and np.array_equal(f, f0)
    # a mesh of which nothing is kept is an error and leaves no file
    far = tmp_path / "far"
    isosurface.write_obj(str(far / "03211117" / "03211117_obj2_00.obj"), v0 + np.float32(2.0), f0)
    with pytest.raises(ValueError, match="obj2_00.obj"):
        postprocess.main(["--src_dir", str(far), "--tar_dir", str(tmp_path / "far_out"), "--category", "display"])
    assert not os.path.exists(str(tmp_path / "far_out" / "03211117" / "03211117_obj2_00.obj"))

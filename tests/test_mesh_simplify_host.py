"""CPU tests of the mesh simplification: ``postprocess.simplify_arrays``, the host function that IS the specification
of mesh_simplify.hip, the ``--simplify`` flag of ``create_sdf`` and ``demo``, the result directory, and the
second header of the C ABI.  Bounds used below:
  * displacement: a vertex and its cluster's output lie in the same closed cell after the clips, so they differ by at
    most h per axis; float32 rounding of the output adds at most 2^-24 of a coordinate of magnitude < 2^4 h here:
    |v' - v|_inf <= h (1 + 2^-20);
  * box fixture: the one-third and one-half bars are the issue's (a throwaway prototype gave a ratio of about 7).
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_simplify_fixtures as SF  # noqa: E402
import reconstruct_fixtures as RF  # noqa: E402
from disn_amd import create_sdf as cs  # noqa: E402
from disn_amd import postprocess as P  # noqa: E402

MF = SF.MF
NEW = ("disn_mesh_simplify_workspace_bytes", "disn_mesh_simplify_count_batch", "disn_mesh_simplify_emit_batch")


@pytest.fixture(scope="module", autouse=True)
def _built():
    from disn_amd.csrc import build
    build.build()


def _triples(faces):
    return [tuple(t) for t in np.sort(np.asarray(faces), 1).tolist()]


# ------------------------------------------------------------------ hand-made cases
def test_fans_by_hand():
    """h = 1/8 on [-1,1]^3: vertices 0..3 (0 and 0.1) fall into cell (8,8,8), 4, 5, 6 into cells of their own (-0.1 is
    cell 7), 7 is unreferenced.  The first fan collapses; the second keeps its two faces.  Every face lies in z = 0:
    the quadric fixes z, the regulariser leaves x, y at the members' mean (0.05, 0.05)."""
    v, f = MF.fans()
    qv, qf, vmap, first = P.simplify_arrays(v, f, SF.UNIT, 16)
    assert qv.dtype == np.float32 and qf.dtype == np.int32 and vmap.dtype == np.int32 and first.dtype == np.int32
    assert vmap.tolist() == [0, 0, 0, 0, 1, 2, 3, 4] and first.tolist() == [0, 4, 5, 6, 7]
    assert qf.tolist() == [[0, 1, 2], [0, 2, 3]]
    want = np.array([[0.05, 0.05, 0], [-0.1, 0, 0], [-0.1, -0.1, 0], [0, -0.1, 0], [0.4, 0.4, 0.4]], np.float32)
    assert np.array_equal(qv, want), qv - want
    # the cluster-mean placement: the same faces, cluster 0 on its members' mean
    mv, mf, _, _ = P.simplify_arrays(v, f, SF.UNIT, 16, placement="mean")
    assert np.array_equal(mf, qf) and np.array_equal(mv, want)


def test_two_cluster_quad_by_hand():
    """vertices 0, 3 in cell (0,0,0), 1, 2 in cell (1,0,0) of [0,2]^3 with two cells per axis: both faces collapse,
    each cluster lands in the plane z = 0.1 at its members' mean"""
    v, f, box, cells = SF.quad()
    qv, qf, vmap, first = P.simplify_arrays(v, f, box, cells)
    assert vmap.tolist() == [0, 1, 1, 0] and first.tolist() == [0, 1] and qf.shape == (0, 3)
    assert np.array_equal(qv, np.array([[0.5, 0.5, 0.1], [1.5, 0.5, 0.1]], np.float32))
    # one more vertex in a third cell: the face through all three clusters survives with its orientation
    v3 = np.concatenate([v, np.array([[0.5, 1.5, 0.1]], np.float32)])
    f3 = np.array([[0, 1, 2], [0, 2, 3], [3, 2, 4], [4, 1, 0]], np.int32)
    qv, qf, vmap, first = P.simplify_arrays(v3, f3, box, cells)
    assert vmap.tolist() == [0, 1, 1, 0, 2] and first.tolist() == [0, 1, 4]
    assert qf.tolist() == [[0, 1, 2]]                                  # face 2; face 3 = (2,1,0) is its duplicate
    assert P.simplify_arrays(v3, f3, box, cells, dedup=False)[1].tolist() == [[0, 1, 2], [2, 1, 0]]


# ------------------------------------------------------------------ displacement
def test_displacement_is_at_most_one_cell():
    cases = SF.device_cases()
    for name, (v, f, box, cells) in cases.items():
        qv, _, vmap, first = SF.host_simplify(name)
        origin, h = P.simplify_lattice(box, cells)
        inside = ((v >= origin) & (v <= origin + h * cells)).all(1)
        assert inside.sum() >= 0.9 * len(v), name
        d = np.abs(qv[vmap].astype(np.float64) - v.astype(np.float64)).max(1)
        assert (d[inside] <= h * (1.0 + 2.0 ** -20)).all(), (name, d[inside].max() / h)
        assert np.array_equal(vmap[first], np.arange(first.size)) and (np.diff(first) > 0).all(), name
        assert np.array_equal(first, np.array([np.nonzero(vmap == c)[0][0] for c in range(first.size)])), name


# ------------------------------------------------------------------ face order
@pytest.mark.parametrize("name", ["soup 50 4000", "box", "crowd"])
def test_face_order_does_not_reach_the_positions(name):
    v, f, box, cells = SF.device_cases()[name]
    qv, qf, vmap, first = SF.host_simplify(name)
    perm = np.random.default_rng(11).permutation(f.shape[0])
    sv, sf, svmap, sfirst = P.simplify_arrays(v, f[perm], box, cells)
    assert np.array_equal(sv.view(np.uint32), qv.view(np.uint32))
    assert np.array_equal(svmap, vmap) and np.array_equal(sfirst, first)
    assert sorted(_triples(sf)) == sorted(_triples(qf))
    # without dedup: exactly the shuffled faces, filtered
    g = vmap[f[perm]]
    keep = (g[:, 0] != g[:, 1]) & (g[:, 1] != g[:, 2]) & (g[:, 0] != g[:, 2])
    assert np.array_equal(P.simplify_arrays(v, f[perm], box, cells, dedup=False)[1], g[keep])
    # with it: the first face of every unordered triple in the shuffled order, in that order
    seen, want = set(), []
    for row in g[keep].tolist():
        if tuple(sorted(row)) not in seen:
            seen.add(tuple(sorted(row)))
            want.append(row)
    assert sf.tolist() == want


# ------------------------------------------------------------------ soups
def test_soups_have_no_collapsed_and_no_duplicate_face():
    total_dropped = 0
    for nv, nf in MF.SOUPS:
        name = "soup %d %d" % (nv, nf)
        v, f, box, cells = SF.device_cases()[name]
        qv, qf, vmap, first = SF.host_simplify(name)
        assert ((qf[:, 0] != qf[:, 1]) & (qf[:, 1] != qf[:, 2]) & (qf[:, 0] != qf[:, 2])).all(), name
        assert len(set(_triples(qf))) == qf.shape[0], name
        nd = SF.host_simplify(name, dedup=False)
        assert np.array_equal(nd[0].view(np.uint32), qv.view(np.uint32)) and np.array_equal(nd[2], vmap)
        assert set(_triples(nd[1])) == set(_triples(qf)) and nd[1].shape[0] >= qf.shape[0], name
        total_dropped += nd[1].shape[0] - qf.shape[0]
    v, f, box, cells = SF.device_cases()["soup 50 4000"]
    nd, q = SF.host_simplify("soup 50 4000", dedup=False), SF.host_simplify("soup 50 4000")
    assert nd[1].shape[0] - q[1].shape[0] >= 100, "the densest soup exercises the duplicate path"
    assert total_dropped > 0


# ------------------------------------------------------------------ the box fixture
def test_box_quadric_placement_beats_the_cluster_mean():
    from oracle import mc_oracle as M
    v, f = SF.box_mesh(32)
    assert M.mesh_is_closed_and_oriented(f)[0]
    qv, qf, vmap, first = SF.host_simplify("box")
    mv, mf, _, _ = P.simplify_arrays(v, f, SF.UNIT, 8, placement="mean")
    assert np.array_equal(qf, mf)
    assert M.mesh_is_closed_and_oriented(qf) == (True, 0)
    h = 2.0 / 8
    dq, dm = SF.box_surface_distance(qv).max() / h, SF.box_surface_distance(mv).max() / h
    true = float(8 * np.prod(SF.BOX_HALF))
    vq, vm = SF.volume(qv, qf) / true, SF.volume(mv, mf) / true
    print("box R=32 cells=8: %d -> %d triangles, %d -> %d vertices; max distance to the true surface: quadric %.4f h, "
          "cluster mean %.4f h; volume / true volume: quadric %.4f, cluster mean %.4f"
          % (f.shape[0], qf.shape[0], v.shape[0], qv.shape[0], dq, dm, vq, vm))
    assert qf.shape[0] < f.shape[0] // 8
    assert dq <= dm / 3.0, (dq, dm)
    assert abs(vq - 1.0) <= abs(vm - 1.0) / 2.0, (vq, vm)
    assert vq > 0 and vm > 0                                            # the orientation survived


# ------------------------------------------------------------------ limits
def test_limits():
    v, f = MF.icosphere(0.3, 2)
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    qv, qf, vmap, first = P.simplify_arrays(v, f, SF.UNIT, 1)
    assert qv.shape == (1, 3) and qf.shape == (0, 3) and not vmap.any() and first.tolist() == [0]
    assert (np.abs(qv) <= 1.0).all()
    qv, qf, vmap, first = P.simplify_arrays(v, f, SF.UNIT, 1024)        # h = 2^-9: every vertex a cluster of its own
    assert qv.shape == v.shape and np.array_equal(qf, f) and np.array_equal(vmap, np.arange(len(v)))
    assert np.abs(qv.astype(np.float64) - v).max() <= 2.0 / 1024
    for bad in (0, 1025, 2.5):
        with pytest.raises(ValueError, match="1..1024"):
            P.simplify_arrays(v, f, SF.UNIT, bad)
    with pytest.raises(ValueError, match="extent"):
        P.simplify_arrays(v, f, [0, 0, 0, 0, 0, 0], 4)
    # out-of-lattice vertices clamp to the border cell and stay inside it
    far = np.array([[-5, 0.1, 0.1], [-7, 0.1, 0.1], [9, 0.1, 0.1], [0.1, 0.1, 0.1]], np.float32)
    ff = np.array([[0, 2, 3], [1, 2, 3]], np.int32)
    qv, qf, vmap, first = P.simplify_arrays(far, ff, SF.UNIT, 4)
    assert vmap.tolist() == [0, 0, 1, 2] and first.tolist() == [0, 2, 3] and qf.tolist() == [[0, 1, 2]]
    assert (qv[0] >= [-1, 0, 0]).all() and (qv[0] <= [-0.5, 0.5, 0.5]).all()
    assert (qv[1] >= [0.5, 0, 0]).all() and (qv[1] <= [1, 0.5, 0.5]).all()
    for poison in (np.nan, np.inf, -np.inf):
        bad = v.copy()
        bad[5, 1] = poison
        with pytest.raises(ValueError, match="not finite"):
            P.simplify_arrays(bad, f, SF.UNIT, 8)
    with pytest.raises(ValueError, match="out of range"):
        P.simplify_arrays(v, np.array([[0, 1, len(v)]], np.int32), SF.UNIT, 8)
    e = P.simplify_arrays(*MF.empty(), SF.UNIT, 8)
    assert e[0].shape == (0, 3) and e[1].shape == (0, 3) and e[2].size == 0 and e[3].size == 0
    # a degenerate face contributes nothing and a cluster without a contributing face lands on its members' mean
    pts = np.array([[0.1, 0.1, 0.1], [0.2, 0.3, 0.15], [0.4, 0.2, 0.3]], np.float32)
    qv, qf, _, _ = P.simplify_arrays(pts, np.array([[0, 0, 1]], np.int32), SF.UNIT, 2)
    assert qf.shape == (0, 3) and np.array_equal(qv, pts.astype(np.float64).mean(0, keepdims=True).astype(np.float32))


# ------------------------------------------------------------------ flags, tree, header
def test_simplify_flag_and_tree_name(tmp_path):
    from disn_amd import demo
    base = ["--test_lst_dir", "lists"]
    a = cs.parser().parse_args(base)
    assert a.simplify is None and cs.simplify_from_flags(a) is None
    a = cs.parser().parse_args(base + ["--simplify", "32", "--clean", "clean", "--band", "4", "--refine", "2", "--normals"])
    assert cs.simplify_from_flags(a) == 32 and cs.check_flags(a) is None
    a = cs.parser().parse_args(base + ["--simplify", "8", "--fuse_views", "2", "--view_num", "4"])
    assert cs.check_flags(a) == (2, "max")
    d = demo.parser().parse_args(["--img", "x.png", "--simplify", "16"])
    assert cs.simplify_from_flags(d) == 16 and demo.parser().parse_args(["--img", "x.png"]).simplify is None
    assert cs.simplify_args(None) is None and cs.simplify_args(1) == 1 and cs.simplify_args(1024) == 1024
    for bad in (0, -3, 1025, 2.5, "many"):
        with pytest.raises(ValueError, match="--simplify"):
            cs.simplify_args(bad)
    j = os.path.join
    assert cs.result_obj_path("log", 64, 0.0, simplify=32) == j("log", "test_objs", "65_0.0_s32")
    assert cs.result_obj_path("log", 64, 0.0, clean=True, simplify=4) == j("log", "test_objs", "65_0.0_comb_s4")
    assert cs.result_obj_path("log", 64, 0.0, True, (3, "mean"), clean=True, simplify=7) == \
        j("log", "test_objs", "camest_fuse3mean_65_0.0_comb_s7")
    assert cs.result_obj_path("log", 64, 0.0, clean=True) == j("log", "test_objs", "65_0.0_comb")

    def boom(*a, **k):
        raise AssertionError("device work was reached")

    for bad in ("0", "1025", "-1"):
        with pytest.raises(ValueError, match="--simplify"):
            cs.main(["--test_lst_dir", str(tmp_path / "none"), "--log_dir", str(tmp_path / "log"), "--simplify", bad],
                    reconstruct_fn=boom)
        with pytest.raises(ValueError, match="--simplify"):
            demo.main(["--img", str(tmp_path / "missing.png"), "--simplify", bad])      # never opened
    assert not os.path.exists(str(tmp_path / "log"))


def test_driver_writes_the_s_tree_and_counts(tmp_path):
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

    def fake(imgs, trans_mats, sdf_params):
        out = [MF.empty() if (n[0] + b) == 2 else (v, f) for b in range(imgs.shape[0])]
        n[0] += imgs.shape[0]
        return out

    res = cs.main(argv + ["--simplify", "4"], reconstruct_fn=fake)
    assert res == {"written": 12, "skipped": 0, "empty": 1, "simplified": 11,
                   "out_dir": os.path.join(log_dir, "test_objs", "9_0.0_s4")}
    n[0] = 0
    res = cs.main(argv, reconstruct_fn=fake)
    assert res == {"written": 12, "skipped": 0, "empty": 1, "out_dir": os.path.join(log_dir, "test_objs", "9_0.0")}


def test_simplify_group_picks_the_meshes_with_triangles(monkeypatch):
    calls = []

    def fake(meshes, boxes, cells, dedup=True):
        calls.append((len(meshes), np.asarray(boxes).tolist(), cells))
        return [(m[0] + 1, m[1]) for m in meshes], [None] * len(meshes)

    monkeypatch.setattr(P, "simplify_meshes_device", fake)
    meshes = [MF.fans(), MF.empty(), MF.fans()]
    boxes = np.arange(18, dtype=np.float64).reshape(3, 6)
    out = cs.simplify_group(meshes, 5, boxes)
    assert calls == [(2, boxes[[0, 2]].tolist(), 5)]
    assert np.array_equal(out[0][0], meshes[0][0] + 1) and out[1] is meshes[1]
    assert cs.simplify_group(meshes, None, boxes) == meshes and len(calls) == 1


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return re.findall(r"\b(disn_[a-z0-9_]+)\s*\(", text)


def test_second_header_equals_the_second_table_and_the_first_stays():
    from disn_amd import _lib
    assert _declared("disn_amd_simplify.h") == list(NEW) == list(_lib.SIGNATURES_SIMPLIFY)
    assert not set(NEW) & set(_lib.SIGNATURES) and set(_declared("disn_amd.h")) == set(_lib.SIGNATURES)
    header = open(os.path.join(ROOT, "include", "disn_amd.h")).read()
    assert re.search(r"#define DISN_ABI_VERSION 10\b", header) and "simplify" not in header
    assert _lib.ABI_VERSION == 10 and _lib.lib().disn_abi_version() == 10
    h = _lib.lib()
    for name in NEW:
        fn = getattr(h, name)
        assert fn.restype is _lib.SIGNATURES_SIMPLIFY[name][0] and list(fn.argtypes) == _lib.SIGNATURES_SIMPLIFY[name][1]
    assert h.disn_mesh_simplify_workspace_bytes(24, 100000, 200000) > 0
    assert h.disn_mesh_simplify_workspace_bytes(1, 0, 0) > 0
    assert h.disn_mesh_simplify_workspace_bytes(0, 10, 10) == 0
    assert h.disn_mesh_simplify_workspace_bytes(1, 10, (2 ** 31 - 1) // 3 + 1) == 0
    assert h.disn_mesh_simplify_workspace_bytes(1, 2 ** 31, 10) == 0
    # argument checks that need no device
    off = np.zeros(2, np.int64)
    lat, cells = np.array([0.0, 0.0, 0.0, 0.5]), np.array([4], np.int32)
    assert h.disn_mesh_simplify_count_batch(None, None, off.ctypes.data, off.ctypes.data, lat.ctypes.data,
                                            cells.ctypes.data, 1, 1, None, None, 0, None) == -1
    for bad_lat, bad_cells in ((np.array([0.0, 0.0, 0.0, 0.0]), cells), (np.array([0.0, 0.0, 0.0, np.nan]), cells),
                               (np.array([np.inf, 0.0, 0.0, 0.5]), cells), (lat, np.array([0], np.int32)),
                               (lat, np.array([1025], np.int32))):
        assert h.disn_mesh_simplify_count_batch(None, None, off.ctypes.data, off.ctypes.data, bad_lat.ctypes.data,
                                                bad_cells.ctypes.data, 1, 1, 1, 1, 1 << 20, None) == -2
    assert h.disn_mesh_simplify_count_batch(None, None, off.ctypes.data, off.ctypes.data, lat.ctypes.data,
                                            cells.ctypes.data, 1, 1, 1, 1, 16, None) == -3
    bad = np.array([0, -1], np.int64)
    assert h.disn_mesh_simplify_emit_batch(None, None, bad.ctypes.data, off.ctypes.data, 1, off.ctypes.data, None, None,
                                           None, None, None, 0, None) == -1


def test_second_header_compiles_as_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "disn_amd_simplify.h"\n'
                   "int main(void) {\n"
                   "  size_t (*ws)(int, int64_t, int64_t) = disn_mesh_simplify_workspace_bytes;\n"
                   "  int (*count)(const float*, const int32_t*, const int64_t*, const int64_t*, const double*,\n"
                   "               const int32_t*, int, int, int64_t*, void*, size_t, void*) = disn_mesh_simplify_count_batch;\n"
                   "  return ws == 0 || count == 0 || DISN_ABI_VERSION != 10;\n"
                   "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I",
                        os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

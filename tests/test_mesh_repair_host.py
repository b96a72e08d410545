"""The mesh repair on the host: ``postprocess.repair_arrays`` (the specification of mesh_repair.hip) against the hand
values of mesh_repair_fixtures.py, its postcondition under ``postprocess.check_arrays``, the argument and size checks of
the C entries (all made on the host, before anything is enqueued: no device is needed) and the drivers' ``--repair``
flags.  (-m "not gpu")"""
import json
import os

import numpy as np
import pytest

import mesh_check_fixtures as X
import mesh_repair_fixtures as RX
from abi_table import FAKE
from disn_amd import create_sdf as cs
from disn_amd import postprocess as P

E_ARG, E_SHAPE, E_WS = -1, -2, -3
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
NOISE = ["dc0", "dcs0", "dc1", "dcs1"]
EVERY = list(RX.FIXTURES) + list(X.FIXTURES) + NOISE + [n + "_simplified" for n in NOISE]


def _mesh(name):
    if name in RX.FIXTURES:
        return RX.FIXTURES[name][:2]
    return X.FIXTURES[name][:2] if name in X.FIXTURES else RX.noise_meshes()[name]


def _repaired(name, **kw):
    return RX.repaired(name, **kw) if name in RX.FIXTURES or name in RX.noise_meshes() else P.repair_arrays(
        *_mesh(name), **kw)


# ------------------------------------------------------------------ 1. the rule
@pytest.mark.parametrize("name", list(RX.FIXTURES))
def test_repair_arrays_equals_the_hand_values(name):
    v, f, (faces, vmap, kept, report) = RX.FIXTURES[name]
    gv, gf, gm, gk, gr = RX.repaired(name)
    assert gr == report, (gr, report)
    assert set(report) == {"status", "nv", "nf"} | set(P.REPAIR_FIELDS)
    for got, want in ((gf, faces), (gm, vmap), (gk, kept)):
        assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), (got, want)
    assert gv.dtype == np.float32 and RX.same_bits(gv, v[vmap])           # the positions are a gather


def test_named_properties_of_the_fixtures():
    r = {n: (P.check_arrays(*RX.repaired(n)[:2]), RX.repaired(n)[4]) for n in RX.FIXTURES}
    on_edge, cut, pinched = r["two_tetrahedra_on_an_edge"], r["three_triangles_on_an_edge"], r["pinched_edge"]
    assert on_edge[0]["watertight"] and (on_edge[0]["nv"], on_edge[0]["boundary_edges"], on_edge[0]["euler"]) == (8, 0, 4)
    assert (cut[0]["nv"], cut[0]["boundary_edges"]) == (9, 9)
    assert pinched[0]["closed"] and pinched[0]["manifold"] and pinched[0]["euler"] == 4
    assert r["two_tetrahedra_touching"][0]["watertight"] and r["two_tetrahedra_at_a_vertex"][0]["watertight"]
    assert r["fan_of_18"][0]["boundary_edges"] == 3 * 18 and r["coplanar_four_face_edge"][0]["boundary_edges"] == 12
    # without the weld the +-0 pair stays two vertices, the two faces share vertex 1 alone and it is split: 5 + 1.  Without the stitch the four-face edge is cut, yet each solid's
    # corners at 0 and at 1 stay one class through its third face (a path whose two ends lie on the cut edge): the same
    # two closed tetrahedra
    assert P.repair_arrays(*_mesh("plus_minus_zero"), weld=False)[4]["nv_out"] == 6
    cut_too = P.repair_arrays(*_mesh("two_tetrahedra_on_an_edge"), stitch=False)
    assert np.array_equal(cut_too[1], RX.repaired("two_tetrahedra_on_an_edge")[1]) and cut_too[4]["stitched_edges"] == 0


def test_the_angular_rule_on_one_edge():
    e = np.array([4.0, 0, 0])
    d = [np.array(x, np.float64) for x in ([0, 4, 0], [0, 0, 4], [0, -4, 0], [0, 0, -4])]
    assert P.repair_stitch_edge(e, d, [False, True, False, True]) == [(0, 1), (2, 3)]
    assert P.repair_stitch_edge(e, d, [True, False, True, False]) == [(1, 2), (3, 0)]
    assert P.repair_stitch_edge(e, d, [True, True, False, False]) is None          # the directions do not alternate
    assert P.repair_stitch_edge(e, [d[0], d[2], d[2], d[3]], [False, True, False, True]) is None      # a tie
    assert P.repair_stitch_edge(e, [d[0], e, d[2], d[3]], [False, True, False, True]) is None         # s = c = 0
    # the order of the faces in the row does not matter beyond the choice of the reference
    assert P.repair_stitch_edge(e, [d[0], d[3], d[1], d[2]], [False, True, True, False]) == [(0, 2), (3, 1)]


@pytest.mark.parametrize("name", EVERY)
def test_the_result_is_manifold_and_repairing_it_again_changes_nothing(name):
    v, f = _mesh(name)
    for kw in ({}, {"stitch": False}, {"weld": False}):
        v2, f2, vmap, kept, report = _repaired(name, **kw)
        if report["status"]:
            assert RX.same_bits(v2, v) and np.array_equal(f2, f) and report["nv_out"] == len(v)
            continue
        c = P.check_arrays(v2, f2, max_pairs=0)
        for k in ("nonmanifold_edges", "nonmanifold_vertices", "index_degenerate_faces", "unreferenced_vertices"):
            assert c[k] == 0, (name, kw, k, c[k])
        assert (c["nv"], c["nf"]) == (report["nv_out"], report["nf_out"]) == (len(vmap), len(kept))
        assert report["nv_out"] == report["nv"] - report["dropped_vertices"] + report["added_vertices"] <= 3 * report["nf_out"]
        assert report["nf_out"] == report["nf"] - report["repeated_faces"] - report["duplicate_faces"] - report["pillow_faces"]
        assert report["pinched_edges"] <= report["stitched_edges"] <= report["singular_edges"]
        assert RX.same_bits(v2, np.asarray(v, np.float32).reshape(-1, 3)[vmap])
        assert np.all(np.diff(kept) > 0)                                         # the survivors keep their order
        v3, f3, vmap3, kept3, again = P.repair_arrays(v2, f2, weld=False)
        assert RX.same_bits(v3, v2) and np.array_equal(f3, f2)
        assert np.array_equal(vmap3, np.arange(len(v2))) and np.array_equal(kept3, np.arange(len(f2)))
        assert all(again[k] == 0 for k in P.REPAIR_FIELDS if k not in ("nv_out", "nf_out"))


@pytest.mark.parametrize("name", ["dc0", "dc1"])
def test_stitching_leaves_a_tenth_of_the_boundary_that_cutting_leaves(name):
    """a condition on the rule (the prototype with atan2 gave 28 against 1416 and 0 against 1404)"""
    before = P.check_arrays(*_mesh(name), max_pairs=0)
    stitched = P.check_arrays(*RX.repaired(name)[:2], max_pairs=0)["boundary_edges"]
    cut = P.check_arrays(*RX.repaired(name, stitch=False)[:2], max_pairs=0)["boundary_edges"]
    print(name, "non-manifold edges before", before["nonmanifold_edges"], "boundary edges stitched", stitched, "cut", cut,
          RX.repaired(name)[4])
    assert before["boundary_edges"] == 0 and before["nonmanifold_edges"] > 300
    assert cut > 1000 and 10 * stitched <= cut


def test_statuses():
    tv, tf = X.FIXTURES["tetrahedron"][:2]
    both = tf.copy()
    both[0, 0] = -1
    nan = tv.copy()
    nan[2, 1] = np.nan
    assert P.repair_arrays(tv, both)[4]["status"] == 2 and P.repair_arrays(nan, tf)[4]["status"] == 4
    v, f, vmap, kept, report = P.repair_arrays(nan, both)                       # of both the larger
    assert report["status"] == 4 and RX.same_bits(v, nan) and np.array_equal(f, both)
    assert np.array_equal(vmap, np.arange(4)) and np.array_equal(kept, np.arange(4))
    assert all(report[k] == 0 for k in P.REPAIR_FIELDS if k not in ("nv_out", "nf_out", "status"))


# ------------------------------------------------------------------ 2. the C entries' checks, without a device
def _args(**over):
    from disn_amd import _lib
    h = _lib.lib()
    counts = np.zeros((1, 12), np.int64)
    counts[0, :2] = 3, 1
    a = dict(verts=FAKE, faces=FAKE, v_off=np.asarray([0, 3], np.int64), f_off=np.asarray([0, 1], np.int64), B=1, flags=3,
             counts=FAKE, counts_host=counts, verts_out=FAKE, faces_out=FAKE, vmap_out=FAKE, kept_out=FAKE, ws=FAKE,
             ws_bytes=h.disn_mesh_repair_workspace_bytes(1, 3, 1), stream=None)
    a.update(over)
    return h, {k: (x.ctypes.data if isinstance(x, np.ndarray) else x) for k, x in a.items()}


def _count(**over):
    h, a = _args(**over)
    return h.disn_mesh_repair_count_batch(a["verts"], a["faces"], a["v_off"], a["f_off"], a["B"], a["flags"], a["counts"],
                                          a["ws"], a["ws_bytes"], a["stream"])


def _emit(**over):
    h, a = _args(**over)
    return h.disn_mesh_repair_emit_batch(a["verts"], a["faces"], a["v_off"], a["f_off"], a["B"], a["flags"],
                                         a["counts_host"], a["verts_out"], a["faces_out"], a["vmap_out"], a["kept_out"],
                                         a["ws"], a["ws_bytes"], a["stream"])


def test_the_entries_refuse_bad_arguments_on_the_host():
    from disn_amd import _lib
    h = _lib.lib()
    assert list(_lib.SIGNATURES_REPAIR) == ["disn_mesh_repair_workspace_bytes", "disn_mesh_repair_count_batch",
                                            "disn_mesh_repair_emit_batch"]
    assert h.disn_abi_version() == 10                                       # additions to the same library
    for call, names in ((_count, ("verts", "faces", "v_off", "f_off", "counts", "ws")),
                        (_emit, ("verts", "faces", "v_off", "f_off", "counts_host", "verts_out", "faces_out", "vmap_out",
                                 "kept_out", "ws"))):
        for name in names:
            assert call(**{name: None}) == E_ARG, (call.__name__, name)
        assert call(B=0) == E_ARG and call(B=-1) == E_ARG
        assert call(flags=4) == E_ARG and call(flags=-1) == E_ARG
        assert call(v_off=np.asarray([1, 3], np.int64)) == E_ARG            # does not start at 0
        assert call(f_off=np.asarray([0, -1], np.int64)) == E_ARG           # descends
        assert call(ws_bytes=h.disn_mesh_repair_workspace_bytes(1, 3, 1) - 1) == E_WS
        assert call(ws_bytes=0) == E_WS
        assert call(v_off=np.asarray([0, 1 << 31], np.int64), ws_bytes=1 << 62) == E_SHAPE
        assert call(f_off=np.asarray([0, (2 ** 31 - 1) // 3 + 1], np.int64), ws_bytes=1 << 62) == E_SHAPE
    # counts_host beyond what the inputs allow: more faces than came in, more vertices than 3 nf_out, a negative size
    for nv_out, nf_out, status in ((3, 2, 0), (4, 1, 0), (-1, 1, 0), (3, -1, 0), (4, 1, 2)):
        bad = np.zeros((1, 12), np.int64)
        bad[0, :3] = nv_out, nf_out, status
        assert _emit(counts_host=bad) == E_ARG, (nv_out, nf_out, status)
    assert _emit(counts_host=np.zeros((1, 12), np.int64)) == 0              # nothing to write: no launch


def test_workspace_bytes_and_the_header():
    from disn_amd import _lib
    from disn_amd.csrc import build
    q = _lib.lib().disn_mesh_repair_workspace_bytes
    assert q(1, 3, 1) > 0 and q(1, 0, 0) > 0
    assert q(0, 3, 1) == 0 and q(1, -1, 1) == 0 and q(1, 3, -1) == 0
    assert q(1, 1 << 31, 1) == 0 and q(1, 3, (2 ** 31 - 1) // 3 + 1) == 0
    assert q(2, 2000, 4000) > q(2, 1000, 2000) > q(1, 3, 1)
    text = open(os.path.join(ROOT, "include", "repair", "disn_amd_repair.h")).read()
    for k, name in enumerate(P.REPAIR_FIELDS):
        assert "#define DISN_REPAIR_%s %d\n" % (name.upper(), k) in text, name
    assert "#define DISN_REPAIR_FIELDS %d\n" % len(P.REPAIR_FIELDS) in text and len(P.REPAIR_FIELDS) == 12
    assert "#define DISN_REPAIR_MAX_FAN %d\n" % P.REPAIR_MAX_FAN in text
    assert "#define DISN_REPAIR_WELD %d " % P.REPAIR_WELD in text and "#define DISN_REPAIR_STITCH %d\n" % P.REPAIR_STITCH in text
    assert build.SOURCES["mesh_repair.hip"] == ["-ffp-contract=off"]
    assert any(h.endswith(os.path.join("include", "repair", "disn_amd_repair.h")) for h in build.HEADERS)
    assert sorted(os.listdir(os.path.join(ROOT, "include", "repair"))) == ["disn_amd_repair.h"]


def test_the_header_compiles_as_c99(tmp_path):
    import subprocess
    src = tmp_path / "use.c"
    src.write_text('#include "repair/disn_amd_repair.h"\n'
                   "int main(void) {\n"
                   "  size_t (*ws)(int, int64_t, int64_t) = disn_mesh_repair_workspace_bytes;\n"
                   "  int (*count)(const float*, const int32_t*, const int64_t*, const int64_t*, int, int, int64_t*, void*,\n"
                   "               size_t, void*) = disn_mesh_repair_count_batch;\n"
                   "  int (*emit)(const float*, const int32_t*, const int64_t*, const int64_t*, int, int, const int64_t*,\n"
                   "              float*, int32_t*, int32_t*, int32_t*, void*, size_t, void*) = disn_mesh_repair_emit_batch;\n"
                   "  return ws == 0 || count == 0 || emit == 0 || DISN_ABI_VERSION != 10 || DISN_REPAIR_FIELDS != 12;\n"
                   "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I",
                        os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------ 3. the stage values, the flags, the paths
def test_repair_args():
    assert cs.repair_args(None) is None and cs.repair_args(False) is None
    assert cs.repair_args(True) == {"weld": True, "stitch": True} == cs.repair_args({})
    assert cs.repair_args({"stitch": False}) == {"weld": True, "stitch": False}
    assert cs.repair_args(cs.repair_args({"weld": False})) == {"weld": False, "stitch": True}      # a checked dict again
    with pytest.raises(ValueError, match="not angle"):
        cs.repair_args({"angle": 1})
    with pytest.raises(ValueError, match="weld must be True or False"):
        cs.repair_args({"weld": 1})
    with pytest.raises(ValueError, match="takes True or a dict"):
        cs.repair_args(3)


def test_repair_flags_and_paths():
    from disn_amd import demo
    for parser, base in ((cs.parser(), ["--test_lst_dir", "x"]), (demo.parser(), ["--img", "x.png"])):
        parse = lambda *flags: parser.parse_args(base + list(flags))
        assert cs.repair_from_flags(parse()) is None
        assert cs.repair_from_flags(parse("--repair")) == {"weld": True, "stitch": True}
        assert cs.repair_from_flags(parse("--repair", "--repair_no_weld")) == {"weld": False, "stitch": True}
        assert cs.repair_from_flags(parse("--repair", "--repair_no_stitch", "--repair_no_weld")) == {
            "weld": False, "stitch": False}
        for flag in ("--repair_no_weld", "--repair_no_stitch"):
            with pytest.raises(ValueError, match="%s needs --repair" % flag):
                cs.repair_from_flags(parse(flag))
        assert "repair" not in cs.stages_from_flags(parse("--repair"), False)    # beside the stages, as --refine is
    path = lambda **kw: os.path.basename(cs.result_obj_path("log", 64, 0.0, **kw))
    assert path() == "65_0.0" and path(repair=True) == "65_0.0_rep"
    assert path(repair=True, colour=True) == "65_0.0_rep_col"
    assert path(mesher="dcs", clean=True, smooth=3, simplify=32, repair=True, colour=True) == "65_0.0_dcs_comb_t3_s32_rep_col"
    assert path(fuse=(2, "max"), repair=True) == "fuse2max_65_0.0_rep"


def test_main_writes_repairs_jsonl(tmp_path):
    import reconstruct_fixtures as RF
    entries = RF.expected_entries(4, 2)
    sdf_dir, rendered_dir = RF.build_dataset(str(tmp_path / "data"), entries, n_samples=32)
    RF.write_lists(str(tmp_path / "lst"))
    argv = ["--log_dir", str(tmp_path / "log"), "--test_lst_dir", str(tmp_path / "lst"), "--sdf_dir", sdf_dir,
            "--rendered_dir", rendered_dir, "--category", "chair,car", "--view_num", "2", "--sdf_res", "8", "--seed", "4",
            "--batch_size", "3"]
    order = ["two_tetrahedra_on_an_edge", "pinched_edge", "empty", "pillow", "two_tetrahedra_touching"]
    calls, reports = [], []

    def fake(imgs, trans_mats, sdf_params):
        base = sum(calls)
        calls.append(imgs.shape[0])
        out = [RX.repaired(order[(base + b) % len(order)]) for b in range(imgs.shape[0])]
        reports.extend(r[4] for r in out)
        return [r[:2] for r in out]

    with pytest.raises(ValueError, match="--repair_no_stitch needs --repair"):
        cs.main(argv + ["--repair_no_stitch"], reconstruct_fn=fake)
    assert calls == []                                                      # refused before any work
    plain = cs.main(argv, reconstruct_fn=fake)
    assert "repaired" not in plain and not os.path.exists(os.path.join(plain["out_dir"], "repairs.jsonl"))
    calls.clear()
    del reports[:]
    res = cs.main(argv + ["--repair"], reconstruct_fn=fake, repair_log=reports)
    assert res["out_dir"] == plain["out_dir"] + "_rep" and res["repaired"] == len(entries) == res["written"]
    rows = [json.loads(l) for l in open(os.path.join(res["out_dir"], "repairs.jsonl"))]
    assert len(rows) == len(entries) and reports == []
    for k, (e, row) in enumerate(zip(entries, rows)):
        assert (row["cat"], row["obj"], row["view"]) == tuple(e)
        want = RX.repaired(order[k % len(order)])[4]
        assert {k2: row[k2] for k2 in want} == want
    # --skip_existing appends; a run without it starts the file afresh
    calls.clear()
    res = cs.main(argv + ["--repair", "--skip_existing"], reconstruct_fn=fake, repair_log=reports)
    rows2 = [json.loads(l) for l in open(os.path.join(res["out_dir"], "repairs.jsonl"))]
    assert len(rows2) == len(rows) + res["repaired"] and res["repaired"] == res["written"]


def test_repair_group_is_off_without_a_device_call(monkeypatch):
    def never(*a, **k):
        raise AssertionError("the stage is off")
    monkeypatch.setattr(P, "repair_meshes_device", never)
    meshes = [X.FIXTURES["tetrahedron"][:2]]
    log = []
    assert cs.repair_group(meshes, None, log) == meshes and log == []
    sig = __import__("inspect").signature
    for fn in (cs.reconstruct, cs.reconstruct_select, cs.reconstruct_fused, cs.reconstruct_fused_select):
        assert sig(fn).parameters["repair"].default is None and sig(fn).parameters["repair_log"].default is None
    assert "5b" in cs._mesh_stages.__doc__ and "2, 3 and 5b" in cs._mesh_stages.__doc__

"""The mesh closing on the host: ``postprocess.close_arrays`` (the specification of mesh_close.hip) against the hand
values of mesh_close_fixtures.py, its guarantee under ``postprocess.check_arrays``, the argument and size checks of the
C entries (all made on the host, before anything is enqueued: no device is needed) and the drivers' ``--close`` flags.
(-m "not gpu")"""
import json
import os

import numpy as np
import pytest

import mesh_check_fixtures as X
import mesh_close_fixtures as CX
from abi_table import FAKE
from disn_amd import create_sdf as cs
from disn_amd import postprocess as P

E_ARG, E_SHAPE, E_WS = -1, -2, -3
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


# ------------------------------------------------------------------ 1. the rule
@pytest.mark.parametrize("name,case", CX.CASES)
def test_close_arrays_equals_the_hand_values(name, case):
    v, f, cases = CX.FIXTURES[name]
    kw, (faces, centres, vmap, kept, report) = cases[case]
    gv, gf, gm, gk, gr = CX.closed(name, case)
    assert gr == report, (kw, gr, report)
    assert set(report) == {"status", "nv", "nf"} | set(P.CLOSE_FIELDS)
    for got, want in ((gf, faces), (gm, vmap), (gk, kept)):
        assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), (kw, got, want)
    assert gv.dtype == np.float32 and CX.same_bits(gv, np.concatenate([v.reshape(-1, 3), centres]))
    assert report["nv_out"] == report["nv"] + report["filled_loops"] == len(vmap)
    assert report["nf_out"] == report["nf"] + report["fill_faces"] == len(kept)


def test_named_properties_of_the_fixtures():
    c = {n: P.check_arrays(*CX.closed(n)[:2]) for n in CX.FIXTURES if CX.closed(n)[4]["status"] == 0}
    for n, r in c.items():
        assert r["closed"] and r["manifold"] and (r["oriented"] or n == "moebius_band"), (n, r)
    assert (c["moebius_band"]["nv"], c["moebius_band"]["nf"], c["moebius_band"]["misoriented_edges"]) == (6, 10, 5)
    assert (c["single_triangle"]["nv"], c["single_triangle"]["nf"], c["single_triangle"]["volume"]) == (4, 4, 0.0)
    assert c["tetrahedron_missing_a_face"]["volume"] == 36.0 and c["cube_missing_its_top_one_side_flipped"]["euler"] == 2
    assert c["cone"]["volume"] > 0 > c["cone_inside_out"]["volume"]
    assert P.check_arrays(*CX.closed("cone_inside_out", 1)[:2])["volume"] == c["cone"]["volume"]
    assert c["sixty_percent_flipped"]["volume"] < 0 < P.check_arrays(*CX.closed("sixty_percent_flipped", 1)[:2])["volume"]
    # the cavity: its volume is subtracted by default, added under ``outward``
    assert c["cavity_in_a_cube"]["volume"] < 512 < P.check_arrays(*CX.closed("cavity_in_a_cube", 1)[:2])["volume"]
    over = P.check_arrays(*CX.closed("cone_inside_out", 2)[:2])
    assert over["boundary_edges"] == CX.RIM and over["volume"] < 0           # over max_hole: open, and not turned


@pytest.mark.parametrize("name", CX.NOISE)
def test_the_guarantee_on_the_repaired_noise_meshes(name):
    v, f = CX.RX.repaired(name)[:2]
    before = P.check_arrays(v, f, max_pairs=0)
    v2, f2, vmap, kept, report = CX.closed(name)
    print(name, "boundary", before["boundary_edges"], "misoriented", before["misoriented_edges"], report)
    after = P.check_arrays(v2, f2, max_pairs=0)
    assert report["status"] == 0 and report["unorientable_components"] == 0
    assert after["boundary_edges"] == 0 and after["nonmanifold_edges"] == 0 and after["misoriented_edges"] == 0
    assert after["nonmanifold_vertices"] == before["nonmanifold_vertices"] == 0
    assert report["fill_faces"] == before["boundary_edges"] and report["loops"] == report["filled_loops"]
    assert (report["flipped_faces"] > 0) == (before["misoriented_edges"] > 0)
    assert CX.same_bits(v2[:len(v)], v) and np.array_equal(vmap[:len(v)], np.arange(len(v)))
    assert np.array_equal(kept[:len(f)], np.arange(len(f))) and np.all(np.diff(kept[len(f):]) >= 0)
    # closing the result again changes nothing
    v3, f3, vmap3, kept3, again = P.close_arrays(v2, f2)
    assert CX.same_bits(v3, v2) and np.array_equal(f3, f2)
    assert np.array_equal(vmap3, np.arange(len(v2))) and np.array_equal(kept3, np.arange(len(f2)))
    assert all(again[k] == 0 for k in P.CLOSE_FIELDS if k not in ("nv_out", "nf_out", "components"))
    assert again["components"] == report["components"]


def test_the_oriented_faces_do_not_depend_on_the_order_of_the_faces():
    """on meshes with n0 != n1 (a tie keeps the root, which is a matter of the order): the cube with one side flipped
    (9 against 1) and the cone with every fifth face turned (240 against 60)"""
    v, f = CX.FIXTURES["cone"][:2]
    turned = np.asarray(f).copy()
    turned[::5] = turned[::5][:, (0, 2, 1)]
    for verts, faces in (CX.FIXTURES["cube_missing_its_top_one_side_flipped"][:2], (v, turned)):
        base = P.close_arrays(verts, faces)
        assert base[4]["flipped_faces"] > 0
        canon = lambda t: {tuple(np.roll(r, -int(np.argmin(r)))) for r in t.tolist()}     # a face up to rotation
        nf = len(faces)
        for seed in (0, 1):
            perm = np.random.default_rng(seed).permutation(nf)
            got = P.close_arrays(verts, np.asarray(faces)[perm])
            assert canon(got[1][:nf]) == canon(base[1][:nf]) and got[4] == base[4]
            # the fill faces name a centre, whose number follows its loop's id: the order of the faces does not enter
            assert canon(got[1][nf:]) == canon(base[1][nf:]) and CX.same_bits(got[0], base[0])
            assert np.array_equal(np.sort(perm[got[3][nf:]]), np.sort(base[3][nf:]))      # the same faces' pairs


def test_statuses():
    tv, tf = X.FIXTURES["tetrahedron"][:2]
    both = tf.copy()
    both[0, 0] = -1
    nan = tv.copy()
    nan[2, 1] = np.nan
    assert P.close_arrays(tv, both)[4]["status"] == 2 and P.close_arrays(nan, tf)[4]["status"] == 4
    v, f, vmap, kept, report = P.close_arrays(nan, both)                        # of both the larger
    assert report["status"] == 4 and CX.same_bits(v, nan) and np.array_equal(f, both)
    assert np.array_equal(vmap, np.arange(4)) and np.array_equal(kept, np.arange(4))
    assert all(report[k] == 0 for k in P.CLOSE_FIELDS if k not in ("nv_out", "nf_out", "status"))
    fan = X.FIXTURES["three_triangles_on_an_edge"]
    inf = fan[0].copy()
    inf[4, 0] = np.inf
    assert P.close_arrays(inf, fan[1])[4]["status"] == 16                       # 16 over 4
    assert P.STATUS_NOT_MANIFOLD == 16 and P.CLOSE_MAX_HOLE == 1 << 22
    # what the repair leaves never has status 16
    for name in ("two_tetrahedra_at_a_vertex", "three_triangles_on_an_edge", "fan_of_18", "repeated_index", "pillow"):
        assert P.close_arrays(*CX.RX.repaired(name)[:2])[4]["status"] == 0, name


def test_argument_errors_of_close_arrays():
    v, f = CX.FIXTURES["single_triangle"][:2]
    with pytest.raises(ValueError, match="outward needs orient"):
        P.close_arrays(v, f, orient=False, outward=True)
    for bad in (-1, (1 << 22) + 1, 2.5, True):
        with pytest.raises(ValueError, match="max_hole must be an integer in 0..4194304"):
            P.close_arrays(v, f, max_hole=bad)
    with pytest.raises(ValueError, match="fill must be True or False"):
        P.close_arrays(v, f, fill=1)
    assert P.close_flags() == (3, 1 << 22) and P.close_flags(True, False, True, 0) == (5, 0)
    assert P.close_arrays(v, f, max_hole=0)[4]["filled_loops"] == 0
    assert P.close_exponent(np.asarray([[0, -6, 1]], np.float32)) == 3 and P.close_exponent(np.zeros((2, 3), np.float32)) == 0
    assert P.close_exponent(np.asarray([[8, 0, 0]], np.float32)) == 4 and P.close_exponent(np.zeros((0, 3), np.float32)) == 0


# ------------------------------------------------------------------ 2. the C entries' checks, without a device
def _args(**over):
    from disn_amd import _lib
    h = _lib.lib()
    counts = np.zeros((1, 9), np.int64)
    counts[0, :2] = 4, 4
    a = dict(verts=FAKE, faces=FAKE, v_off=np.asarray([0, 3], np.int64), f_off=np.asarray([0, 1], np.int64), B=1, flags=3,
             max_hole=1 << 22, counts=FAKE, counts_host=counts, verts_out=FAKE, faces_out=FAKE, vmap_out=FAKE,
             kept_out=FAKE, ws=FAKE, ws_bytes=h.disn_mesh_close_workspace_bytes(1, 3, 1), stream=None)
    a.update(over)
    return h, {k: (x.ctypes.data if isinstance(x, np.ndarray) else x) for k, x in a.items()}


def _count(**over):
    h, a = _args(**over)
    return h.disn_mesh_close_count_batch(a["verts"], a["faces"], a["v_off"], a["f_off"], a["B"], a["flags"], a["max_hole"],
                                         a["counts"], a["ws"], a["ws_bytes"], a["stream"])


def _emit(**over):
    h, a = _args(**over)
    return h.disn_mesh_close_emit_batch(a["verts"], a["faces"], a["v_off"], a["f_off"], a["B"], a["flags"], a["max_hole"],
                                        a["counts_host"], a["verts_out"], a["faces_out"], a["vmap_out"], a["kept_out"],
                                        a["ws"], a["ws_bytes"], a["stream"])


def test_the_entries_refuse_bad_arguments_on_the_host():
    from disn_amd import _lib
    h = _lib.lib()
    assert list(_lib.SIGNATURES_CLOSE) == ["disn_mesh_close_workspace_bytes", "disn_mesh_close_count_batch",
                                           "disn_mesh_close_emit_batch"]
    assert h.disn_abi_version() == 10                                       # additions to the same library
    for call, names in ((_count, ("verts", "faces", "v_off", "f_off", "counts", "ws")),
                        (_emit, ("verts", "faces", "v_off", "f_off", "counts_host", "verts_out", "faces_out", "vmap_out",
                                 "kept_out", "ws"))):
        for name in names:
            assert call(**{name: None}) == E_ARG, (call.__name__, name)
        assert call(B=0) == E_ARG and call(B=-1) == E_ARG
        assert call(flags=8) == E_ARG and call(flags=-1) == E_ARG
        assert call(flags=4) == E_ARG and call(flags=6) == E_ARG            # outward without orient
        assert call(max_hole=-1) == E_ARG and call(max_hole=(1 << 22) + 1) == E_ARG
        assert call(v_off=np.asarray([1, 3], np.int64)) == E_ARG            # does not start at 0
        assert call(f_off=np.asarray([0, -1], np.int64)) == E_ARG           # descends
        assert call(ws_bytes=h.disn_mesh_close_workspace_bytes(1, 3, 1) - 1) == E_WS
        assert call(ws_bytes=0) == E_WS
        assert call(v_off=np.asarray([0, 1 << 31], np.int64), ws_bytes=1 << 62) == E_SHAPE
        assert call(f_off=np.asarray([0, (2 ** 31 - 1) // 3 + 1], np.int64), ws_bytes=1 << 62) == E_SHAPE
    # counts_host beyond what the inputs allow: fewer vertices or faces than came in, more fill faces than pairs, a
    # centre with fewer than three faces, anything gained under a status or without the fill flag
    for nv_out, nf_out, status, flags in ((2, 1, 0, 3), (3, 0, 0, 3), (3, 5, 0, 3), (4, 3, 0, 3), (5, 4, 0, 3),
                                          (4, 4, 16, 3), (4, 4, 0, 1)):
        bad = np.zeros((1, 9), np.int64)
        bad[0, :3] = nv_out, nf_out, status
        assert _emit(counts_host=bad, flags=flags) == E_ARG, (nv_out, nf_out, status, flags)
    assert _emit(v_off=np.asarray([0, 0], np.int64), f_off=np.asarray([0, 0], np.int64),
                 counts_host=np.zeros((1, 9), np.int64)) == 0               # nothing to write: no launch


def test_workspace_bytes_and_the_header():
    from disn_amd import _lib
    from disn_amd.csrc import build
    q = _lib.lib().disn_mesh_close_workspace_bytes
    assert q(1, 3, 1) > 0 and q(1, 0, 0) > 0
    assert q(0, 3, 1) == 0 and q(1, -1, 1) == 0 and q(1, 3, -1) == 0
    assert q(1, 1 << 31, 1) == 0 and q(1, 3, (2 ** 31 - 1) // 3 + 1) == 0
    assert q(2, 2000, 4000) > q(2, 1000, 2000) > q(1, 3, 1)
    text = open(os.path.join(ROOT, "include", "close", "disn_amd_close.h")).read()
    for k, name in enumerate(P.CLOSE_FIELDS):
        assert "#define DISN_CLOSE_%s %d\n" % (name.upper(), k) in text, name
    assert "#define DISN_CLOSE_FIELDS %d\n" % len(P.CLOSE_FIELDS) in text and len(P.CLOSE_FIELDS) == 9
    assert "#define DISN_CLOSE_MAX_HOLE %d " % P.CLOSE_MAX_HOLE in text
    assert "#define DISN_CLOSE_STATUS_NOT_MANIFOLD %d\n" % P.STATUS_NOT_MANIFOLD in text
    for name, bit in (("ORIENT", P.CLOSE_ORIENT), ("FILL", P.CLOSE_FILL), ("OUTWARD", P.CLOSE_OUTWARD)):
        assert "#define DISN_CLOSE_%s %d" % (name, bit) in text
    assert build.SOURCES["mesh_close.hip"] == ["-ffp-contract=off"]
    assert any(h.endswith(os.path.join("include", "close", "disn_amd_close.h")) for h in build.HEADERS)
    assert sorted(os.listdir(os.path.join(ROOT, "include", "close"))) == ["disn_amd_close.h"]
    assert '#include "../disn_amd.h"' in text and "DISN_ABI_VERSION 1" not in text


def test_the_header_compiles_as_c99(tmp_path):
    import subprocess
    src = tmp_path / "use.c"
    src.write_text('#include "close/disn_amd_close.h"\n'
                   "int main(void) {\n"
                   "  size_t (*ws)(int, int64_t, int64_t) = disn_mesh_close_workspace_bytes;\n"
                   "  int (*count)(const float*, const int32_t*, const int64_t*, const int64_t*, int, int, int64_t,\n"
                   "               int64_t*, void*, size_t, void*) = disn_mesh_close_count_batch;\n"
                   "  int (*emit)(const float*, const int32_t*, const int64_t*, const int64_t*, int, int, int64_t,\n"
                   "              const int64_t*, float*, int32_t*, int32_t*, int32_t*, void*, size_t, void*) =\n"
                   "      disn_mesh_close_emit_batch;\n"
                   "  return ws == 0 || count == 0 || emit == 0 || DISN_ABI_VERSION != 10 || DISN_CLOSE_FIELDS != 9;\n"
                   "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I",
                        os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------ 3. the stage values, the flags, the paths
def test_close_args():
    full = {"orient": True, "fill": True, "outward": False, "max_hole": 1 << 22}
    assert cs.close_args(None) is None and cs.close_args(False) is None
    assert cs.close_args(True) == full == cs.close_args({})
    assert cs.close_args({"fill": False, "max_hole": 12}) == dict(full, fill=False, max_hole=12)
    assert cs.close_args(cs.close_args({"outward": True})) == dict(full, outward=True)         # a checked dict again
    with pytest.raises(ValueError, match="not angle"):
        cs.close_args({"angle": 1})
    with pytest.raises(ValueError, match="--close: orient must be True or False"):
        cs.close_args({"orient": 1})
    with pytest.raises(ValueError, match="--close: outward needs orient"):
        cs.close_args({"orient": False, "outward": True})
    with pytest.raises(ValueError, match="--close: max_hole must be an integer"):
        cs.close_args({"max_hole": -3})
    with pytest.raises(ValueError, match="takes True or a dict"):
        cs.close_args(3)


def test_close_flags_and_paths():
    from disn_amd import demo
    full = {"orient": True, "fill": True, "outward": False, "max_hole": 1 << 22}
    for parser, base in ((cs.parser(), ["--test_lst_dir", "x"]), (demo.parser(), ["--img", "x.png"])):
        parse = lambda *flags: parser.parse_args(base + list(flags))
        assert cs.close_from_flags(parse()) is None
        assert cs.close_from_flags(parse("--close")) == full
        assert cs.close_from_flags(parse("--close", "--close_no_orient")) == dict(full, orient=False)
        assert cs.close_from_flags(parse("--close", "--close_no_fill", "--close_outward", "--close_max_hole", "9")) == {
            "orient": True, "fill": False, "outward": True, "max_hole": 9}
        for flags in (["--close_no_orient"], ["--close_no_fill"], ["--close_outward"], ["--close_max_hole", "9"]):
            with pytest.raises(ValueError, match="%s needs --close" % flags[0]):
                cs.close_from_flags(parse(*flags))
        with pytest.raises(ValueError, match="outward needs orient"):
            cs.close_from_flags(parse("--close", "--close_no_orient", "--close_outward"))
        with pytest.raises(ValueError, match="max_hole"):
            cs.close_from_flags(parse("--close", "--close_max_hole", "-1"))
        assert "close" not in cs.stages_from_flags(parse("--close"), False)      # beside the stages, as --repair is
    path = lambda **kw: os.path.basename(cs.result_obj_path("log", 64, 0.0, **kw))
    assert path() == "65_0.0" and path(close=True) == "65_0.0_cls" and path(repair=True, close=True) == "65_0.0_rep_cls"
    assert path(repair=True, close=True, colour=True) == "65_0.0_rep_cls_col" and path(close=True, colour=True) == "65_0.0_cls_col"
    assert path(mesher="dcs", clean=True, smooth=3, simplify=32, repair=True, close=True,
                colour=True) == "65_0.0_dcs_comb_t3_s32_rep_cls_col"
    assert path(fuse=(2, "max"), close=True) == "fuse2max_65_0.0_cls"


def test_main_writes_closes_jsonl(tmp_path):
    import reconstruct_fixtures as RF
    entries = RF.expected_entries(4, 2)
    sdf_dir, rendered_dir = RF.build_dataset(str(tmp_path / "data"), entries, n_samples=32)
    RF.write_lists(str(tmp_path / "lst"))
    argv = ["--log_dir", str(tmp_path / "log"), "--test_lst_dir", str(tmp_path / "lst"), "--sdf_dir", sdf_dir,
            "--rendered_dir", rendered_dir, "--category", "chair,car", "--view_num", "2", "--sdf_res", "8", "--seed", "4",
            "--batch_size", "3"]
    order = ["open_prism", "moebius_band", "empty", "cone", "two_triangles_the_same_way"]
    calls, reports = [], []

    def fake(imgs, trans_mats, sdf_params):
        base = sum(calls)
        calls.append(imgs.shape[0])
        out = [CX.closed(order[(base + b) % len(order)]) for b in range(imgs.shape[0])]
        reports.extend(r[4] for r in out)
        return [r[:2] for r in out]

    with pytest.raises(ValueError, match="--close_no_fill needs --close"):
        cs.main(argv + ["--close_no_fill"], reconstruct_fn=fake)
    assert calls == []                                                      # refused before any work
    plain = cs.main(argv, reconstruct_fn=fake)
    assert "closed" not in plain and not os.path.exists(os.path.join(plain["out_dir"], "closes.jsonl"))
    calls.clear()
    del reports[:]
    res = cs.main(argv + ["--close"], reconstruct_fn=fake, close_log=reports)
    assert res["out_dir"] == plain["out_dir"] + "_cls" and res["closed"] == len(entries) == res["written"]
    rows = [json.loads(l) for l in open(os.path.join(res["out_dir"], "closes.jsonl"))]
    assert len(rows) == len(entries) and reports == []
    for k, (e, row) in enumerate(zip(entries, rows)):
        assert (row["cat"], row["obj"], row["view"]) == tuple(e)
        want = CX.closed(order[k % len(order)])[4]
        assert {k2: row[k2] for k2 in want} == want
    # --skip_existing appends; a run without it starts the file afresh
    calls.clear()
    res = cs.main(argv + ["--close", "--skip_existing"], reconstruct_fn=fake, close_log=reports)
    rows2 = [json.loads(l) for l in open(os.path.join(res["out_dir"], "closes.jsonl"))]
    assert len(rows2) == len(rows) + res["closed"] and res["closed"] == res["written"]
    # with --repair too, the tree is <...>_rep_cls and both files are written
    calls.clear()
    del reports[:]
    both = cs.main(argv + ["--repair", "--close"], reconstruct_fn=fake, close_log=reports)
    assert both["out_dir"] == plain["out_dir"] + "_rep_cls" and os.path.exists(os.path.join(both["out_dir"], "closes.jsonl"))


def test_close_group_is_off_without_a_device_call(monkeypatch):
    def never(*a, **k):
        raise AssertionError("the stage is off")
    monkeypatch.setattr(P, "close_meshes_device", never)
    meshes = [X.FIXTURES["tetrahedron"][:2]]
    log = []
    assert cs.close_group(meshes, None, log) == meshes and log == []
    sig = __import__("inspect").signature
    for fn in (cs.reconstruct, cs.reconstruct_select, cs.reconstruct_fused, cs.reconstruct_fused_select):
        assert sig(fn).parameters["close"].default is None and sig(fn).parameters["close_log"].default is None
    assert "5c" in cs._mesh_stages.__doc__
    src = __import__("inspect").getsource(cs._mesh_stages)
    assert src.index("repair_group(") < src.index("close, close_log)") < src.index("colour_group(meshes")

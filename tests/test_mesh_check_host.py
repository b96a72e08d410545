"""The mesh checks on the host: ``postprocess.check_arrays`` (the specification of mesh_check.hip) against the hand
values of mesh_check_fixtures.py and an independent brute-force restatement; the argument and size checks of the C entry
(all made on the host, before anything is enqueued: no device is needed); the drivers' ``--check`` flags."""
import json
import os

import numpy as np
import pytest

import dual_contour_fixtures as DF
import dual_contour_sheets_fixtures as DS
import mesh_check_fixtures as X
from abi_table import FAKE
from disn_amd import create_sdf as cs
from disn_amd import postprocess as P
from oracle import mc_oracle as O

E_ARG, E_SHAPE, E_WS = -1, -2, -3
_CACHE = {}


def _noise_mesh(R=12):
    if R not in _CACHE:
        v, f = O.marching_cubes(X.noise(R, 0), [-1, -1, -1, 1, 1, 1], 0.0)
        _CACHE[R] = (np.asarray(v, np.float32), np.asarray(f, np.int32))
    return _CACHE[R]


# ------------------------------------------------------------------ 1. the rule
@pytest.mark.parametrize("name", list(X.FIXTURES))
def test_check_arrays_equals_the_hand_values(name):
    v, f, hand = X.FIXTURES[name]
    got = P.check_arrays(v, f)
    for k, want in hand.items():
        assert got[k] == want, (name, k, got[k], want)
    assert got["closed"] == (hand["boundary_edges"] == 0)
    assert got["manifold"] == (hand["nonmanifold_edges"] == 0 and hand["nonmanifold_vertices"] == 0)
    assert got["oriented"] == (hand["misoriented_edges"] == 0)
    assert got["watertight"] == (got["closed"] and got["manifold"] and got["oriented"]
                                 and hand["intersecting_pairs"] == 0)
    flags = P.check_face_flags(v, f)
    assert flags.dtype == np.uint8 and flags.shape == (len(f),)
    assert int((flags & P.FLAG_INTERSECTS != 0).sum()) == hand["intersecting_faces"]
    assert int((flags & P.FLAG_DEGENERATE != 0).sum()) == hand["index_degenerate_faces"] + hand["zero_area_faces"]
    assert bool((flags & P.FLAG_BOUNDARY).any()) == (hand["boundary_edges"] > 0)
    assert bool((flags & P.FLAG_NONMANIFOLD).any()) == (hand["nonmanifold_edges"] > 0)
    assert bool((flags & P.FLAG_MISORIENTED).any()) == (hand["misoriented_edges"] > 0)


def test_named_properties_of_the_fixtures():
    r = {n: P.check_arrays(*X.FIXTURES[n][:2]) for n in X.FIXTURES}
    assert r["tetrahedron"]["watertight"] and r["cube"]["watertight"] and r["tetrahedron"]["euler"] == 2
    assert r["tetrahedron"]["volume"] == 64.0 / 6.0
    assert not r["cube_open"]["closed"] and r["cube_open"]["manifold"] and r["cube_open"]["oriented"]
    assert r["tetrahedron_flipped_face"]["closed"] and not r["tetrahedron_flipped_face"]["oriented"]
    assert not r["two_tetrahedra_at_a_vertex"]["manifold"] and r["two_tetrahedra_at_a_vertex"]["nonmanifold_edges"] == 0
    assert not r["two_tetrahedra_on_an_edge"]["manifold"] and r["two_tetrahedra_on_an_edge"]["nonmanifold_vertices"] == 0
    # orientation is not judged on the four-face edge: both solids are oriented
    assert r["two_tetrahedra_on_an_edge"]["oriented"]
    assert r["two_tetrahedra_interpenetrating"]["closed"] and not r["two_tetrahedra_interpenetrating"]["watertight"]
    assert r["two_tetrahedra_touching"]["watertight"]                       # touching is no intersection
    assert r["empty"]["watertight"] and r["empty"]["status"] == 0


@pytest.mark.parametrize("case", ["noise12", "sphere"])
def test_check_arrays_equals_the_brute_force(case):
    if case == "noise12":
        v, f = _noise_mesh(12)
    else:
        g = np.linspace(-1, 1, 11)
        x, y, z = np.meshgrid(g, g, g, indexing="ij")
        vol = (np.sqrt(x * x + y * y + z * z) - 0.73).astype(np.float32)
        v, f = O.marching_cubes(vol, [-1, -1, -1, 1, 1, 1], 0.0)
        v, f = np.asarray(v, np.float32), np.asarray(f, np.int32)
    got = P.check_arrays(v, f)
    assert got["index_degenerate_faces"] == 0 and got["status"] == 0
    assert (got["candidate_pairs"], got["intersecting_pairs"], got["intersecting_faces"]) == X.brute_force(v, f)
    if case == "noise12":
        # the figures of the rule's trial: marching cubes of white noise does intersect itself under this rule
        assert (got["nf"], got["candidate_pairs"], got["intersecting_pairs"]) == (4696, 54168, 61)
        closed, bad = O.mesh_is_closed_and_oriented(f)
        assert closed and bad == 0 and got["closed"] and got["oriented"] and got["manifold"]
    else:
        assert got["watertight"] and got["euler"] == 2 and got["intersecting_pairs"] == 0
        # outward orientation: a positive volume, the ball's up to (its area) x (the sagitta of a chord as long as a
        # cell's diagonal, r - sqrt(r^2 - 0.03) = 0.021, + the interpolation error of a vertex, h^2 / 8r = 0.007)
        r = 0.73
        assert abs(got["volume"] - 4.0 / 3.0 * np.pi * r ** 3) < 4 * np.pi * r * r * (0.021 + 0.007)
        assert got["volume"] > 0


def test_default_cap_has_room_on_the_noise_meshes():
    for R in (12, 20):
        v, f = _noise_mesh(R)
        got = P.check_arrays(v, f)
        print(R, len(f), got["candidate_pairs"], P.check_max_pairs(None, len(f)))
        assert got["status"] == 0 and 8 * got["candidate_pairs"] < P.check_max_pairs(None, len(f))


def test_per_cell_dual_contouring_is_not_manifold_where_per_sheet_is():
    fx = DS.disc(0.03)                                           # a thin part of test_thin_parts_stay_manifold_and_apart
    _, _, dv, df = DF.mesh(fx)
    _, _, sv, sf = DS.mesh(fx)
    per_cell, per_sheet = P.check_arrays(dv, df), P.check_arrays(sv, sf)
    print("per cell", per_cell, "per sheet", per_sheet)
    assert per_cell["nonmanifold_edges"] + per_cell["nonmanifold_vertices"] > 0 and not per_cell["manifold"]
    assert per_sheet["nonmanifold_edges"] + per_sheet["nonmanifold_vertices"] == 0 and per_sheet["manifold"]
    assert per_sheet["closed"] and per_sheet["oriented"]


def test_statuses_and_the_cap():
    v, f, hand = X.FIXTURES["stack"]
    full = P.check_arrays(v, f)
    capped = P.check_arrays(v, f, max_pairs=2015)
    assert capped["status"] == P.STATUS_CHECK_PAIRS == 8
    assert capped["intersecting_pairs"] == capped["intersecting_faces"] == -1 and not capped["watertight"]
    for k in full:
        if k not in ("status", "intersecting_pairs", "intersecting_faces", "watertight"):
            assert capped[k] == full[k], k
    assert P.check_arrays(v, f, max_pairs=2016)["status"] == 0
    assert P.check_max_pairs(None, 64) == 256 * 64 + 4096
    with pytest.raises(ValueError, match="max_pairs"):
        P.check_arrays(v, f, max_pairs=-1)
    tv, tf, _ = X.FIXTURES["two_tetrahedra_interpenetrating"]
    bad = tf.copy()
    bad[2, 0] = 8
    r = P.check_arrays(tv, bad)
    assert r["status"] == 2 and (r["nv"], r["nf"]) == (8, 8) and r["edges"] == -1 and r["candidate_pairs"] == -1
    assert not (r["closed"] or r["manifold"] or r["oriented"] or r["watertight"])
    assert not P.check_face_flags(tv, bad).any()
    nan = tv.copy()
    nan[0, 0] = np.inf
    r = P.check_arrays(nan, tf)
    assert r["status"] == 4 and r["edges"] == 12 and r["closed"] and r["zero_area_faces"] == -1
    assert r["candidate_pairs"] == r["intersecting_pairs"] == -1 and r["area"] == 0.0 and not r["watertight"]


# ------------------------------------------------------------------ 2. the C entry's checks, without a device
def _call(**over):
    from disn_amd import _lib
    h = _lib.lib()
    v_off, f_off = np.asarray([0, 3], np.int64), np.asarray([0, 1], np.int64)
    caps = np.asarray([10], np.int64)
    need = h.disn_mesh_check_workspace_bytes(1, 3, 1, 10)
    a = dict(verts=FAKE, faces=FAKE, v_off=v_off, f_off=f_off, B=1, caps=caps, counts=FAKE, sums=FAKE, flags=None,
             status=FAKE, ws=FAKE, ws_bytes=need, stream=None)
    a.update(over)
    ptr = lambda x: x.ctypes.data if isinstance(x, np.ndarray) else x
    return h.disn_mesh_check_batch(a["verts"], a["faces"], ptr(a["v_off"]), ptr(a["f_off"]), a["B"], ptr(a["caps"]),
                                   a["counts"], a["sums"], a["flags"], a["status"], a["ws"], a["ws_bytes"], a["stream"])


def test_the_entry_refuses_bad_arguments_on_the_host():
    from disn_amd import _lib
    h = _lib.lib()
    assert set(_lib.SIGNATURES_CHECK) == {"disn_mesh_check_workspace_bytes", "disn_mesh_check_batch"}
    assert h.disn_abi_version() == 10
    for name in ("verts", "faces", "v_off", "f_off", "caps", "counts", "sums", "status", "ws"):
        assert _call(**{name: None}) == E_ARG, name
    assert _call(B=0) == E_ARG
    assert _call(v_off=np.asarray([1, 3], np.int64)) == E_ARG               # does not start at 0
    assert _call(f_off=np.asarray([0, -1], np.int64)) == E_ARG              # descends
    assert _call(caps=np.asarray([-1], np.int64)) == E_ARG                  # a negative cap
    assert _call(ws_bytes=h.disn_mesh_check_workspace_bytes(1, 3, 1, 10) - 1) == E_WS
    assert _call(ws_bytes=0) == E_WS
    big = (1 << 27) + 1                                                     # DISN_CHECK_MAX_FACES + 1
    assert _call(f_off=np.asarray([0, big], np.int64), ws_bytes=1 << 62) == E_SHAPE
    assert _call(v_off=np.asarray([0, 1 << 31], np.int64), ws_bytes=1 << 62) == E_SHAPE
    assert _call(f_off=np.asarray([0, (2 ** 31 - 1) // 3 + 1], np.int64), ws_bytes=1 << 62) == E_SHAPE


def test_workspace_bytes():
    from disn_amd import _lib
    q = _lib.lib().disn_mesh_check_workspace_bytes
    assert q(1, 3, 1, 10) > 0 and q(1, 0, 0, 0) > 0
    assert q(0, 3, 1, 10) == 0 and q(1, -1, 1, 10) == 0 and q(1, 3, -1, 10) == 0 and q(1, 3, 1, -1) == 0
    assert q(1, 1 << 31, 1, 10) == 0 and q(1, 3, (2 ** 31 - 1) // 3 + 1, 10) == 0 and q(1, 3, (1 << 27) + 1, 10) == 0
    assert q(1, 3, 1 << 27, 10) > 0
    assert q(2, 2000, 4000, 10) > q(2, 1000, 2000, 10) > q(1, 3, 1, 10)
    assert q(1, 1000, 2000, 10) == q(1, 1000, 2000, 10 ** 12)               # the workspace holds no pair list
    # the header's field indices are the order of CHECK_FIELDS
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "check", "disn_amd_check.h")).read()
    for k, name in enumerate(P.CHECK_FIELDS):
        assert "#define DISN_CHECK_%s %d\n" % (name.upper(), k) in text, name
    assert "#define DISN_CHECK_FIELDS %d\n" % len(P.CHECK_FIELDS) in text
    assert "#define DISN_CHECK_PAIRS_PER_FACE %d\n" % P.CHECK_PAIRS_PER_FACE in text
    assert cs.CHECK_PAIRS_PER_FACE == P.CHECK_PAIRS_PER_FACE


# ------------------------------------------------------------------ 3. the drivers' flags
def _driver_inputs(tmp_path, view_num=2, seed=4):
    import reconstruct_fixtures as RF
    entries = RF.expected_entries(seed, view_num)
    sdf_dir, rendered_dir = RF.build_dataset(str(tmp_path / "data"), entries, n_samples=32)
    lst_dir = str(tmp_path / "lst")
    RF.write_lists(lst_dir)
    log_dir = str(tmp_path / "log")
    argv = ["--log_dir", log_dir, "--test_lst_dir", lst_dir, "--sdf_dir", sdf_dir, "--rendered_dir", rendered_dir,
            "--category", "chair,car", "--view_num", str(view_num), "--sdf_res", "8", "--seed", str(seed)]
    return entries, argv, log_dir


def _host_checker(meshes, max_pairs):
    return [P.check_arrays(v, f, c) for (v, f), c in zip(meshes, max_pairs)]


def test_check_flags():
    parse = lambda *flags: cs.parser().parse_args(["--test_lst_dir", "x"] + list(flags))
    assert cs.check_from_flags(parse()) is None
    assert cs.check_from_flags(parse("--check")) == 256
    assert cs.check_from_flags(parse("--check", "--check_pairs", "3")) == 3
    with pytest.raises(ValueError, match="--check_pairs needs --check"):
        cs.check_from_flags(parse("--check_pairs", "3"))
    with pytest.raises(ValueError, match="negative"):
        cs.check_from_flags(parse("--check", "--check_pairs", "-1"))
    from disn_amd import demo
    a = demo.parser().parse_args(["--img", "x.png", "--check"])
    assert cs.check_from_flags(a) == 256
    with pytest.raises(ValueError, match="--check_pairs needs --check"):
        cs.check_from_flags(demo.parser().parse_args(["--img", "x.png", "--check_pairs", "2"]))


def test_main_writes_checks_jsonl(tmp_path):
    entries, argv, log_dir = _driver_inputs(tmp_path)
    order = ["tetrahedron", "cube_open", "two_tetrahedra_interpenetrating", "empty", "stack", "cube"]
    calls = []

    def fake(imgs, trans_mats, sdf_params):
        base = sum(calls)
        calls.append(imgs.shape[0])
        return [X.FIXTURES[order[(base + b) % len(order)]][:2] for b in range(imgs.shape[0])]

    with pytest.raises(ValueError, match="--check_pairs needs --check"):
        cs.main(argv + ["--check_pairs", "4"], reconstruct_fn=fake)
    assert calls == []                                                      # refused before any work
    plain = cs.main(argv + ["--batch_size", "3"], reconstruct_fn=fake)
    assert "checked" not in plain and "watertight" not in plain
    assert not os.path.exists(os.path.join(plain["out_dir"], "checks.jsonl"))
    calls.clear()
    res = cs.main(argv + ["--batch_size", "3", "--check"], reconstruct_fn=fake, check_fn=_host_checker)
    assert res["out_dir"] == plain["out_dir"]                               # the tree's name does not change
    n = len(entries)
    rows = [json.loads(l) for l in open(os.path.join(res["out_dir"], "checks.jsonl"))]
    assert res["checked"] == n == len(rows)
    for k, (e, row) in enumerate(zip(entries, rows)):
        name = order[k % len(order)]
        assert (row["cat"], row["obj"], row["view"]) == tuple(e)
        want = P.check_arrays(*X.FIXTURES[name][:2])
        assert {k2: row[k2] for k2 in want} == want, name
        for k2 in ("status", "area", "volume", "closed", "manifold", "oriented", "watertight") + P.CHECK_FIELDS:
            assert k2 in row
    assert res["watertight"] == sum(order[k % len(order)] in ("tetrahedron", "empty", "cube") for k in range(n))
    # --check_pairs 0 leaves the 4096 pairs every mesh has: room for every fixture, the stack's 2016 included
    calls.clear()
    res = cs.main(argv + ["--batch_size", "3", "--check", "--check_pairs", "0"], reconstruct_fn=fake,
                  check_fn=_host_checker)
    rows = [json.loads(l) for l in open(os.path.join(res["out_dir"], "checks.jsonl"))]
    assert len(rows) == n and all(r["status"] == 0 for r in rows)
    # --skip_existing appends; a run without it starts the file afresh
    calls.clear()
    res = cs.main(argv + ["--batch_size", "3", "--check", "--skip_existing"], reconstruct_fn=fake,
                  check_fn=_host_checker)
    rows2 = [json.loads(l) for l in open(os.path.join(res["out_dir"], "checks.jsonl"))]
    assert len(rows2) == n + res["checked"] and res["checked"] == res["written"]


def test_check_without_a_checker_needs_device_meshes(tmp_path):
    """the drivers have no host fallback: host meshes from an injected reconstruct_fn and no injected checker is an
    error, not a silent host run"""
    entries, argv, _ = _driver_inputs(tmp_path)
    fake = lambda i, t, s: [X.FIXTURES["tetrahedron"][:2] for _ in range(i.shape[0])]
    with pytest.raises(TypeError, match="CUDA tensors"):
        cs.main(argv + ["--check"], reconstruct_fn=fake)


def test_evaluate_mesh_check_on_a_tree(tmp_path):
    from disn_amd import evaluate, isosurface
    cats = evaluate.categories("chair")
    (cat_id,) = cats.values()
    os.makedirs(tmp_path / cat_id)
    names = ["tetrahedron", "cube_open", "two_tetrahedra_interpenetrating", "cube", "fold_over_at_a_vertex"]
    for k, n in enumerate(names):
        isosurface.write_obj(str(tmp_path / cat_id / ("m%d.obj" % k)), *X.FIXTURES[n][:2])
    (tmp_path / cat_id / "m9.obj").write_bytes(b"")                         # an empty mesh, as the driver writes it
    lines = []

    class Out:
        def write(self, s):
            lines.append(s)

    res = evaluate.mesh_check_all(cats, str(tmp_path), group=4, out=Out(), check_fn=_host_checker)
    rows = [json.loads(l) for l in open(res["out"])]
    assert res["checked"] == 6 == len(rows) and res["out"] == str(tmp_path / "checks.jsonl")
    for k, n in enumerate(names):
        want = P.check_arrays(*X.FIXTURES[n][:2])
        assert {k2: rows[k][k2] for k2 in want} == want and rows[k]["obj"] == "m%d" % k and rows[k]["cat"] == cat_id
    assert rows[5]["nf"] == 0 and rows[5]["watertight"]
    s = res["categories"]["chair"]
    assert s["meshes"] == 6 and res["watertight"] == 3
    assert s["share"] == {"closed": 4 / 6, "manifold": 5 / 6, "oriented": 1.0, "no_self_intersection": 4 / 6,
                          "watertight": 3 / 6}
    assert s["mean"]["boundary_edges"] == (4 + 6) / 6 and s["mean"]["intersecting_pairs"] == 4 / 6
    assert s["status"] == {"0": 6}
    text = "".join(lines)
    assert "chair" in text and "watertight 50.0%" in text and "mean" in text
    a = evaluate.parser().parse_args(["mesh_check", str(tmp_path), "--category", "chair", "--group", "2"])
    assert (a.command, a.obj_dir, a.group, a.check_pairs) == ("mesh_check", str(tmp_path), 2, None)

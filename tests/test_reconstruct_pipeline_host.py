"""The reconstruction pipeline without a device: ``create_sdf._mesh_stages`` is the ONE stage chain of
``reconstruct_select`` and ``reconstruct_fused_select``, ``reconstruct`` / ``reconstruct_fused`` forward every keyword,
and both drivers hand on exactly what ``stages_from_flags`` makes of their flags.  Everything that would touch the
device is replaced by a recorder on tiny tetrahedra.  (-m "not gpu")"""
import inspect
import os

import numpy as np
import pytest
import torch

import reconstruct_fixtures as RF
from disn_amd import create_sdf as cs, isosurface, postprocess

ORDER = ["mesh", "clean", "simplify", "smooth", "refine", "colour"]       # the order stated at cs._mesh_stages
TET_V = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=torch.float32)
TET_F = torch.tensor([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=torch.int32)
R, B = 8, 4
IMGS = np.zeros((B, 137, 137, 3), np.float32)
CAMS = np.zeros((B, 4, 3), np.float32)
BOXES = np.tile(np.array([[-1, -1, -1, 1, 1, 1]], np.float64), (B, 1))
ALL_ON = {"clean": (3.0, 0.0, "face"), "simplify": 4, "smooth": 2, "colour": True, "mesher": "dcs"}
PLAIN_ONLY = {"band": (4, 0.5, 1), "refine": 1, "normals": True}          # what the fused route does not take


class FakeEngine:
    device = "cpu"

    def __init__(self, log):
        self.log = log

    def encode(self, imgs):
        self.log.append("encode")
        return "enc"

    def query_grid_views(self, enc, run, tm, sp, res, pool, out=None):
        self.log.append("grid_views")
        out.zero_()


@pytest.fixture
def log(monkeypatch):
    """every device entry of the pipeline replaced; -> the list of what was called, in order"""
    seen = []

    def grids(name, extra):
        def fake(engine, imgs, *a):
            seen.append(name)
            return ("enc", torch.zeros((len(imgs), (R + 1) ** 3))) + extra
        return fake

    def mesher(*a, **k):
        seen.append("mesh")
        return [(TET_V, TET_F)] * len(a[0])

    def stage(name, shift):
        def fake(meshes, *a, **k):
            seen.append(name)
            return [(m[0] + shift, m[1]) for m in meshes], [0] * len(meshes)
        return fake

    def refine(engine, enc, b, tm, verts, faces, sp, res, iso, iters):
        seen.append("refine")
        return verts + 1000.0, faces, verts * 0.0

    def colour(meshes, im, tm, views_per_mesh=1, alpha=None, **k):
        seen.append("colour")
        return [torch.full((len(m[0]), 3), views_per_mesh, dtype=torch.uint8) for m in meshes], None

    monkeypatch.setattr(cs, "_encode_grids", grids("grids", ()))
    monkeypatch.setattr(cs, "_encode_grids_band", grids("grids_band", (None,)))
    monkeypatch.setattr(isosurface, "marching_cubes_batch", mesher)
    monkeypatch.setattr(isosurface, "dual_contour_batch", mesher)
    monkeypatch.setattr(isosurface, "refine_mesh", refine)
    monkeypatch.setattr(postprocess, "clean_meshes_device", stage("clean", 1.0))
    monkeypatch.setattr(postprocess, "simplify_meshes_device", stage("simplify", 10.0))
    monkeypatch.setattr(postprocess, "smooth_meshes_device", stage("smooth", 100.0))
    monkeypatch.setattr(postprocess, "colour_meshes_device", colour)
    return seen


def _plain(log, select=True, **kw):
    fn = cs.reconstruct_select if select else cs.reconstruct
    return fn(FakeEngine(log), IMGS, CAMS, BOXES, R, **kw)


def _fused(log, select=True, **kw):
    fn = cs.reconstruct_fused_select if select else cs.reconstruct_fused
    return fn(FakeEngine(log), IMGS, CAMS, BOXES, R, fuse=2, **kw)


def _same_meshes(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and all(torch.equal(s, t) for s, t in zip(x, y))
                                    for x, y in zip(a, b))


# ------------------------------------------------------------------ (a), (b): one chain, one order
def test_both_routes_run_the_stages_in_the_stated_order_once_per_group(log):
    meshes, unclean = _plain(log, **ALL_ON, **PLAIN_ONLY)
    plain = list(log)
    assert plain == ["grids_band", "mesh", "clean", "simplify", "smooth"] + ["refine"] * B + ["colour"]
    assert [s for k, s in enumerate(plain[1:]) if s != plain[k]] == ORDER       # runs of one name, in the stated order
    assert unclean == [False] * B and len(meshes) == B
    for v, f, n, c in meshes:                                       # every stage saw what the one before it left
        assert torch.equal(v, TET_V + 1111.0) and f is TET_F and torch.equal(n, (TET_V + 111.0) * 0.0)
        assert c.dtype == torch.uint8 and c.tolist() == [[1] * 3] * 4             # coloured from ONE view each
    log.clear()
    meshes, unclean = _fused(log, **ALL_ON)
    assert log == ["encode", "grid_views", "grid_views"] + [s for s in ORDER if s != "refine"]
    assert unclean == [False] * 2 and len(meshes) == 2
    for v, f, c in meshes:
        assert torch.equal(v, TET_V + 111.0) and f is TET_F and c.tolist() == [[2] * 3] * 4    # from BOTH views of a run


def test_with_everything_off_no_stage_is_called(log):
    meshes, unclean = _plain(log)
    assert log == ["grids", "mesh"] and unclean == [False] * B
    assert all(m[0] is TET_V and m[1] is TET_F and len(m) == 2 for m in meshes)
    log.clear()
    meshes, unclean = _fused(log)
    assert log == ["encode", "grid_views", "grid_views", "mesh"] and unclean == [False] * 2
    assert all(m[0] is TET_V and m[1] is TET_F and len(m) == 2 for m in meshes)
    log.clear()                                                     # ... and "off" has one spelling per stage or two
    _plain(log, band=None, clean=None, simplify=None, smooth=None, colour=False, mesher="mc", dc=None, refine=0)
    assert log == ["grids", "mesh"]


# ------------------------------------------------------------------ (c): the short forms forward every keyword
KEYWORDS = [{}] + [{k: v} for k, v in sorted(ALL_ON.items())] + [
    {"colour": {"mirror_axis": "x"}, "alpha": np.full((B, 137, 137), 255, np.uint8)}, {"mesher": "dc", "dc": 0.5},
    {"smooth": {"iters": 3, "cap": None}}, ALL_ON]


@pytest.mark.parametrize("kw", KEYWORDS + [{k: v} for k, v in sorted(PLAIN_ONLY.items())] + [dict(ALL_ON, **PLAIN_ONLY)],
                         ids=lambda kw: "+".join(sorted(kw)) or "none")
def test_reconstruct_is_reconstruct_select_0(log, kw):
    want = _plain(log, **kw)[0]
    calls = list(log)
    log.clear()
    assert _same_meshes(_plain(log, select=False, **kw), want) and log == calls


@pytest.mark.parametrize("kw", KEYWORDS, ids=lambda kw: "+".join(sorted(kw)) or "none")
def test_reconstruct_fused_is_reconstruct_fused_select_0(log, kw):
    want = _fused(log, **kw)[0]
    calls = list(log)
    log.clear()
    assert _same_meshes(_fused(log, select=False, **kw), want) and log == calls


def test_the_short_forms_take_every_keyword_of_the_select_forms():
    for short, full in ((cs.reconstruct, cs.reconstruct_select), (cs.reconstruct_fused, cs.reconstruct_fused_select)):
        a, b = inspect.signature(short).parameters, inspect.signature(full).parameters
        assert set(b) - set(a) == {"select", "strict"} and not set(a) - set(b)
        assert all(a[k].default == b[k].default for k in a)


# ------------------------------------------------------------------ (d): the drivers hand on stages_from_flags
@pytest.fixture(scope="module")
def argv(tmp_path_factory):
    root = tmp_path_factory.mktemp("pipeline")
    entries = RF.expected_entries(4, 2)
    sdf_dir, rendered_dir = RF.build_dataset(str(root / "data"), entries, n_samples=32)
    RF.write_lists(str(root / "lst"))
    return ["--log_dir", str(root / "log"), "--test_lst_dir", str(root / "lst"), "--sdf_dir", sdf_dir, "--rendered_dir",
            rendered_dir, "--category", "chair,car", "--view_num", "2", "--sdf_res", "8", "--seed", "4"]


FLAGS = {"clean": ["--clean", "chair", "--clean_dist_thresh", "3"], "simplify": ["--simplify", "4"],
         "smooth": ["--smooth", "2", "--smooth_cap", "1"], "colour": ["--colour", "--colour_mirror", "x"],
         "mesher": ["--mesher", "dcs", "--dc_reg", "0.5"], "band": ["--band", "4"], "refine": ["--refine", "1"],
         "normals": ["--normals"]}
FUSED = ["clean", "simplify", "smooth", "colour", "mesher"]                    # all that --fuse_views admits
MAIN_TABLE = [([], "9_0.0"), (["clean"], "9_0.0_comb"), (["simplify"], "9_0.0_s4"), (["smooth"], "9_0.0_t2"),
              (["colour"], "9_0.0_col"), (["mesher"], "9_0.0_dcs"), (["band"], "9_0.0"), (["refine"], "9_0.0"),
              (["normals"], "9_0.0"), (sorted(FLAGS), "9_0.0_dcs_comb_t2_s4_col"),
              (["fuse"], "fuse2max_9_0.0"), (["fuse"] + FUSED, "fuse2max_9_0.0_dcs_comb_t2_s4_col")]


@pytest.mark.parametrize("names,tree", MAIN_TABLE, ids=lambda x: "+".join(x) or "none" if isinstance(x, list) else None)
def test_main_hands_on_what_stages_from_flags_gives(argv, monkeypatch, names, tree):
    import disn_amd.engine as engine_mod
    fuse = "fuse" in names
    args = argv + (["--fuse_views", "2"] if fuse else []) + [w for n in names if n != "fuse" for w in FLAGS[n]]
    parsed = cs.parser().parse_args(args)
    want = cs.stages_from_flags(parsed, parsed.clean is not None)
    assert sorted(want) == ["band", "clean", "colour", "dc", "mesher", "simplify", "smooth"]
    assert all((want[k] is not None) == (k in names) for k in want if k not in ("mesher", "dc"))
    assert (want["mesher"], want["dc"] is not None) == (("dcs", True) if "mesher" in names else ("mc", False))
    calls = []

    def route(name):
        signature = inspect.signature(getattr(cs, name))

        def fake(*a, **k):
            named = signature.bind(*a, **k)
            named.apply_defaults()
            c = dict(named.arguments, route=name)
            calls.append(c)
            M = len(c["imgs"]) // (2 if fuse else 1)
            mesh = (TET_V.numpy(), TET_F.numpy()) + ((TET_V.numpy(),) if c.get("normals") else ()) \
                + ((np.zeros((4, 3), np.uint8),) if c["colour"] is not None else ())
            return [mesh] * M, [False] * M
        return fake

    monkeypatch.setattr(engine_mod, "SdfEngine", lambda *a, **k: None)
    monkeypatch.setattr(cs, "restore_weights", lambda log_dir, seed: (None, "stub"))
    monkeypatch.setattr(cs, "reconstruct_select", route("reconstruct_select"))
    monkeypatch.setattr(cs, "reconstruct_fused_select", route("reconstruct_fused_select"))
    res = cs.main(args)
    assert len(calls) == 4                                          # four objects, two views each: one group each
    for c in calls:
        assert c["route"] == ("reconstruct_fused_select" if fuse else "reconstruct_select")
        assert {k: c[k] for k in want if k in c} == {k: v for k, v in want.items() if not (fuse and k == "band")}
        assert (c["sdf_res"], c["iso"], c["strict"]) == (8, 0.0, False)
        assert (c["fuse"], c["pool"]) == (2, "max") if fuse else (c["refine"], c["normals"]) == (
            int("refine" in names), "normals" in names)
        assert c["select"] is None or "clean" in names
    chairs_then_cars = [[True]] * 2 + [[False]] * 2 if fuse else [[True] * 2] * 2 + [[False] * 2] * 2
    assert [c["select"] for c in calls] == (chairs_then_cars if "clean" in names else [None] * 4)
    assert res["out_dir"] == os.path.join(parsed.log_dir, "test_objs", tree)
    assert res["written"] == (4 if fuse else 8) and res["empty"] == 0
    assert sorted(set(res) - {"written", "skipped", "empty", "out_dir"}) == sorted(
        {"clean": "unclean", "simplify": "simplified", "smooth": "smoothed", "colour": "coloured"}[n]
        for n in names if n in ("clean", "simplify", "smooth", "colour"))


def test_demo_hands_on_what_stages_from_flags_gives(tmp_path, monkeypatch):
    from PIL import Image

    import disn_amd.engine as engine_mod
    from disn_amd import demo
    png = str(tmp_path / "view.png")
    Image.fromarray(np.full((137, 137, 4), 200, np.uint8), "RGBA").save(png)
    calls = []

    def fake(*a, **k):
        named = inspect.signature(cs.reconstruct_select).bind(*a, **k)      # (reconstruct takes a subset of it)
        calls.append(named.arguments)
        return [(TET_V, TET_F) + ((TET_V,) if k.get("colour") is None else (TET_V, TET_F.to(torch.uint8)))]

    monkeypatch.setattr(engine_mod, "SdfEngine", lambda *a, **k: None)
    monkeypatch.setattr(cs, "restore_weights", lambda log_dir, seed: (None, "stub"))
    monkeypatch.setattr(cs, "reconstruct", fake)
    for names in ([], ["clean"], ["colour"], sorted(FLAGS)):
        flags = [w for n in names for w in (["--clean", "--clean_dist_thresh", "3"] if n == "clean" else FLAGS[n])]
        args = ["--img", png, "--sdf_res", "8", "--out", str(tmp_path / "out.obj")] + flags
        parsed = demo.parser().parse_args(args)
        res = demo.main(args)
        c = calls.pop()
        assert not calls and {k: c[k] for k in cs.stages_from_flags(parsed, parsed.clean)} == cs.stages_from_flags(
            parsed, parsed.clean)
        assert (c["alpha"] is not None) == ("colour" in names) == ("colours" in res)
        assert (res["verts"], res["faces"]) == (4, 4)
        got = isosurface.read_obj(res["out"])
        assert np.array_equal(got[0], TET_V.numpy()) and np.array_equal(got[1], TET_F.numpy())

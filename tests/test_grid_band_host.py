"""Narrow-band grid evaluation without a device: the float32 reference (tests/grid_band_reference.py) on the float64
golden of BASELINE config 1, the drivers' ``--band`` flags, and the C ABI's argument checks.  (-m "not gpu")"""
import ctypes
import os

import numpy as np
import pytest

import grid_band_reference as G
import reconstruct_fixtures as RF
from disn_amd import create_sdf as cs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SURFACE_CELLS = 5971


@pytest.fixture(scope="module")
def cfg1():
    """the stored values pred64 / 10 of the 65^3 grid (the pad point dropped), float32"""
    gold = np.load(os.path.join(GOLDEN, "cfg1_full65.npz"))["pred64"]
    assert gold.size == 65 ** 3 + 1
    return (gold[:65 ** 3] / 10.0).astype(np.float32)


# (stride, margin, dilate) -> (active coarse cells, coarse cells, share of the 65^3 points evaluated, surface cells missed)
TABLE = {(2, 0.5, 0): (3121, 32768, 0.232, 0),
         (4, 0.5, 0): (763, 4096, 0.224, 0),
         (4, 0.5, 1): (1845, 4096, 0.475, 0),
         (4, 0.0, 0): (306, 4096, 0.102, 366)}


@pytest.mark.parametrize("key", sorted(TABLE))
def test_reference_reproduces_the_table(cfg1, key):
    s, margin, rounds = key
    active, cells, share, lost = TABLE[key]
    assert int(G.surface_cells(cfg1, 0.0).sum()) == SURFACE_CELLS
    mask = G.select(cfg1, 64, s, 0.0, margin, rounds)
    assert mask.size == cells and int(mask.sum()) == active
    assert round(G.share(mask, 64, s), 3) == share
    assert G.missed(cfg1, mask, s, 0.0) == lost
    ev = G.evaluated_mask(mask, 64, s)
    assert int(ev.sum()) == int(G.band_mask(mask, 64, s).sum()) + (64 // s + 1) ** 3     # band and lattice are disjoint


def test_filled_grid_has_no_crossing_outside_the_active_cells(cfg1):
    s = 4
    mask = G.select(cfg1, 64, s, 0.0, 0.5, 1)
    filled = G.fill(cfg1, mask, 64, s)
    ev = G.evaluated_mask(mask, 64, s)
    assert np.array_equal(filled[ev], cfg1[ev]) and not np.array_equal(filled, cfg1)
    assert G.missed(filled, mask, s, 0.0) == 0
    # ... and inside them the filled grid IS the dense grid, so the surface cells are the dense grid's
    assert np.array_equal(G.surface_cells(filled, 0.0), G.surface_cells(cfg1, 0.0))
    # a fill never leaves the range of its cell's corners
    lo, hi = G.cell_minmax(cfg1, 64, s)
    up = lambda a: a.repeat(s, 0).repeat(s, 1).repeat(s, 2)
    inner, evaluated = filled.reshape(65, 65, 65)[:64, :64, :64], ev.reshape(65, 65, 65)[:64, :64, :64]
    assert np.all((inner >= up(lo)) | evaluated) and np.all((inner <= up(hi)) | evaluated)


def test_reference_edge_cases():
    n = 17
    const = np.full(n ** 3, 0.25, np.float32)
    assert not G.select(const, 16, 4, 0.25, 0.5, 2).any()           # a constant equal to iso: hi >= iso but lo < iso fails
    assert np.array_equal(G.fill(const, np.zeros((4, 4, 4), bool), 16, 4), const)
    z = np.arange(n, dtype=np.float32)[:, None, None] * np.ones((1, n, n), np.float32)
    plane = (16.0 - z).ravel().astype(np.float32)                   # 0 on the last plane iz = 16, positive below
    m = G.cell_rule(plane, 16, 4, 0.0, 0.0)
    assert not m.any()                                              # lo = 0 is not < iso: nothing is inside
    m = G.cell_rule(-plane, 16, 4, 0.0, 0.0)
    assert m[3].all() and not m[:3].any()                           # hi = 0 >= iso, lo < iso: the last layer of cells
    assert G.dilate(m, 1)[2:].all() and not G.dilate(m, 1)[:2].any()
    with pytest.raises(ValueError):
        G.select(const, 16, 3, 0.0, 0.5, 0)
    with pytest.raises(ValueError):
        G.lattice_mask(18, 4)


# ------------------------------------------------------------------ flags
def test_band_flags_are_checked_before_any_device_work(tmp_path):
    from disn_amd import demo
    base = ["--test_lst_dir", str(tmp_path / "none"), "--log_dir", str(tmp_path / "log")]

    def boom(*a):
        raise AssertionError("device work was reached")

    with pytest.raises(ValueError, match="--band"):
        cs.main(base + ["--band", "3"], reconstruct_fn=boom)
    with pytest.raises(ValueError, match="--band"):
        cs.main(base + ["--sdf_res", "66", "--band", "4"], reconstruct_fn=boom)
    with pytest.raises(ValueError, match="--band_margin"):
        cs.main(base + ["--band", "4", "--band_margin", "-1"], reconstruct_fn=boom)
    with pytest.raises(ValueError, match="--band_dilate"):
        cs.main(base + ["--band", "4", "--band_dilate", "-1"], reconstruct_fn=boom)
    assert not os.path.exists(str(tmp_path / "log"))
    img = str(tmp_path / "missing.png")                             # never opened: the flags are checked first
    with pytest.raises(ValueError, match="--band"):
        demo.main(["--img", img, "--band", "3"])
    with pytest.raises(ValueError, match="--band"):
        demo.main(["--img", img, "--sdf_res", "66", "--band", "4"])
    a = cs.parser().parse_args(base)
    assert (a.band, a.band_margin, a.band_dilate) == (0, 0.5, 1) and cs.band_from_flags(a) is None
    d = demo.parser().parse_args(["--img", img])
    assert (d.band, d.band_margin, d.band_dilate) == (0, 0.5, 1) and cs.band_from_flags(d) is None
    a = cs.parser().parse_args(base + ["--band", "8", "--band_margin", "0.25", "--band_dilate", "2"])
    assert cs.band_from_flags(a) == (8, 0.25, 2)
    assert cs.band_args(None, 66) is None and cs.band_args((2, 0, 0), 66) == (2, 0.0, 0)


def test_band_zero_takes_the_existing_call_path(tmp_path, monkeypatch):
    """``--band 0``: the driver's one call, ``reconstruct_select``, gets ``band=None`` and every other stage off, and
    ``reconstruct`` goes through ``_encode_grids``; ``--band 4``: the same call with ``band=(4, 0.5, 1)``"""
    import inspect

    import disn_amd.engine as engine_mod
    from disn_amd import isosurface
    entries = RF.expected_entries(4, 3)
    sdf_dir, rendered_dir = RF.build_dataset(str(tmp_path / "data"), entries, n_samples=32)
    lst_dir = str(tmp_path / "lst")
    RF.write_lists(lst_dir)
    argv = ["--log_dir", str(tmp_path / "log"), "--test_lst_dir", lst_dir, "--sdf_dir", sdf_dir, "--rendered_dir",
            rendered_dir, "--category", "chair,car", "--view_num", "3", "--sdf_res", "8", "--seed", "4"]
    calls = []

    class FakeEngine:
        def __init__(self, *a, **k):
            pass

    signature = inspect.signature(cs.reconstruct_select)

    def fake_reconstruct(*args, **kwargs):
        named = signature.bind(*args, **kwargs)
        named.apply_defaults()
        calls.append(named.arguments)
        t = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
        B = named.arguments["imgs"].shape[0]
        return [(t, np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32))] * B, [False] * B

    def facts(c):
        return [c[k] for k in ("sdf_res", "iso", "refine", "normals", "band")]

    def rest_is_off(c):
        return all(c[k] is None for k in ("clean", "simplify", "smooth", "colour", "dc")) and c["mesher"] == "mc"

    monkeypatch.setattr(engine_mod, "SdfEngine", FakeEngine)
    monkeypatch.setattr(cs, "restore_weights", lambda log_dir, seed: (None, "stub"))
    monkeypatch.setattr(cs, "reconstruct_select", fake_reconstruct)
    cs.main(argv)
    cs.main(argv + ["--band", "0", "--band_margin", "0.9"])
    assert calls and all(facts(c) == [8, 0.0, 0, False, None] and rest_is_off(c) for c in calls)
    calls.clear()
    cs.main(argv + ["--band", "4"])
    assert calls and all(facts(c) == [8, 0.0, 0, False, (4, 0.5, 1)] and rest_is_off(c) for c in calls)
    monkeypatch.undo()

    # reconstruct(band=None) itself: the dense grids, never the band's
    seen = []
    monkeypatch.setattr(cs, "_encode_grids", lambda *a: seen.append("dense") or ("enc", np.zeros((1, 729), np.float32)))
    monkeypatch.setattr(cs, "_encode_grids_band", lambda *a: seen.append("band") or ("enc", np.zeros((1, 729), np.float32), None))
    monkeypatch.setattr(isosurface, "marching_cubes_batch", lambda grids, sp, res, iso: ["mesh"])
    box = np.array([[-1, -1, -1, 1, 1, 1]], np.float64)
    assert cs.reconstruct(None, None, None, box, 8) == ["mesh"] and seen == ["dense"]
    assert cs.reconstruct(None, None, None, box, 8, band=(4, 0.5, 1)) == ["mesh"] and seen == ["dense", "band"]
    with pytest.raises(ValueError):
        cs.reconstruct(None, None, None, box, 8, band=(3, 0.5, 1))
    with pytest.raises(ValueError):
        cs.create_sdf(None, None, None, box, 6, band=(4, 0.5, 1))
    assert seen == ["dense", "band"]


# ------------------------------------------------------------------ C ABI
def test_band_entries_validate_their_arguments():
    from disn_amd import _lib, ops
    h = _lib.lib()
    big = 1 << 40
    for name in ("disn_query_grid_listed", "disn_query_grid_listed_workspace_bytes", "disn_grid_band_select",
                 "disn_grid_band_select_workspace_bytes", "disn_grid_band_fill"):
        assert name in _lib.SIGNATURES and hasattr(h, name)
    # workspace sizes: pure host arithmetic
    assert h.disn_grid_band_select_workspace_bytes(64, 4) >= 2 * 4 * 65 ** 3
    assert h.disn_grid_band_select_workspace_bytes(64, 3) == 0
    assert h.disn_grid_band_select_workspace_bytes(66, 4) == 0
    assert h.disn_grid_band_select_workspace_bytes(2, 4) == 0
    assert h.disn_grid_band_select_workspace_bytes(1296, 8) == 0          # (R+1)^3 >= 2^31
    assert h.disn_grid_band_select_workspace_bytes(1288, 8) > 0
    assert h.disn_query_grid_listed_workspace_bytes(0) == 0
    per_million = h.disn_query_grid_listed_workspace_bytes(2 << 20) - h.disn_query_grid_listed_workspace_bytes(1 << 20)
    assert per_million == 20 << 20                                        # 20 bytes per listed point: bounded by the chunk

    def select(grid=1, R=64, s=4, margin=0.5, dilate=1, mask=1, idx=1, cap=100, counts=1, ws=1, nbytes=big):
        return h.disn_grid_band_select(grid, R, s, 0.0, margin, dilate, mask, idx, cap, counts, ws, nbytes, None)

    assert select(grid=None) == -1 and select(mask=None) == -1 and select(idx=None) == -1
    assert select(counts=None) == -1 and select(ws=None) == -1
    assert select(s=3) == -1 and select(s=0) == -1 and select(s=16) == -1
    assert select(R=66) == -1 and select(R=0) == -1
    assert select(dilate=-1) == -1 and select(margin=-0.5) == -1 and select(margin=float("nan")) == -1
    assert select(cap=-1) == -1
    assert select(nbytes=16) == -3
    assert h.disn_grid_band_fill(None, 64, 4, 1, None) == -1
    assert h.disn_grid_band_fill(1, 64, 4, None, None) == -1
    assert h.disn_grid_band_fill(1, 64, 3, 1, None) == -1
    assert h.disn_grid_band_fill(1, 66, 4, 1, None) == -1

    w = _lib.MlpWeights()
    for f in _lib.MLP_FIELDS:
        setattr(w, f, 1)
    wr = ctypes.byref(w)
    pr = ctypes.byref((ctypes.c_double * 6)(-1, -1, -1, 1, 1, 1))

    def listed(wp=wr, pmap=1, amax=1, emb=1, tm=1, box=pr, R=64, idx=None, s=4, first=0, n=10, weight=10.0, grid=1,
               ws=1, nbytes=big):
        return h.disn_query_grid_listed(wp, pmap, amax, emb, tm, box, R, idx, s, first, n, weight, grid, ws, nbytes,
                                        None)

    assert listed() == -1                                                  # no fused images in the weights
    for f in _lib.MLP_FUSED_FIELDS:
        setattr(w, f, 1)
    assert listed(wp=None) == -1 and listed(pmap=None) == -1 and listed(amax=None) == -1 and listed(emb=None) == -1
    assert listed(tm=None) == -1 and listed(box=None) == -1 and listed(grid=None) == -1 and listed(ws=None) == -1
    assert listed(s=3) == -1 and listed(s=0) == -1 and listed(R=66) == -1
    assert listed(idx=1, s=4) == -1                                        # a list takes no stride
    assert listed(weight=0.0) == -1 and listed(n=-1) == -1 and listed(first=-1) == -1
    assert listed(first=17 ** 3 - 5, n=6) == -1                            # past the lattice's (64/4 + 1)^3 points
    assert listed(nbytes=16) == -3 and listed(idx=1, s=0, nbytes=16) == -3
    assert listed(n=0) == 0 and listed(idx=1, s=0, n=0) == 0               # nothing listed: no launch
    # the wrappers refuse before they touch a tensor
    with pytest.raises(ValueError):
        ops.band_check(64, 3)
    with pytest.raises(ValueError):
        ops.band_check(66, 4)
    assert ops.band_sizes(64, 4) == (17 ** 3, 16 ** 3, 65 ** 3 - 17 ** 3)

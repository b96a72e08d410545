"""Narrow-band grid evaluation on the device (disn_amd/csrc/grid_band.hip, disn_query_grid_listed,
``SdfEngine.query_grid_band``, ``create_sdf.reconstruct(band=...)``).  Bars: the selection, the point list and the fill
equal the float32 reference (tests/grid_band_reference.py) bit for bit; every evaluated point carries the dense fused
grid's bits; on the config-1 field the default band misses no surface cell and marching cubes gives the dense mesh."""
import numpy as np
import pytest
import torch

import grid_band_reference as G
from oracle import disn_oracle as O

pytestmark = pytest.mark.gpu

BOX = [-1, -0.9, -0.8, 1, 0.9, 0.8]


@pytest.fixture(scope="module")
def eng():
    from disn_amd.engine import SdfEngine
    from disn_amd.weights import WeightStore
    return SdfEngine(WeightStore.random_init(0, mode="he"))


@pytest.fixture(scope="module")
def view(eng):
    """one encoded image and its dense fused grid at R = 32 over an anisotropic box: computed once, never modified"""
    enc = eng.encode(O.synth_inputs(3, 1, 8)["imgs"])
    dense = eng.query_grid(enc, 0, O.DEMO_TRANS_MAT, BOX, 32, fused=True)
    torch.cuda.synchronize()
    return enc, dense, dense.cpu().numpy()


# ------------------------------------------------------------------ 1. the selection kernels, exactly
def _fields(R):
    n = R + 1
    i = np.arange(n, dtype=np.float32)
    z, y, x = np.meshgrid(i, i, i, indexing="ij")
    c = np.float32(R / 2.0)
    sphere = np.sqrt((x - c - np.float32(0.3)) ** 2 + (y - c) ** 2 + (z - c + np.float32(0.7)) ** 2) - np.float32(0.31 * R)
    plane = (x - np.float32(R)) * np.float32(0.1)          # 0 on the last plane ix = R, inside (negative) everywhere else
    far = sphere + np.float32(4.0 * R)                     # no crossing
    const = np.full((n, n, n), 0.25, np.float32)           # a constant equal to iso
    return {"sphere": (sphere, 0.0), "plane": (plane, 0.0), "far": (far, 0.0), "const": (const, 0.25)}


@pytest.mark.parametrize("s", [4, 2])
@pytest.mark.parametrize("name", ["sphere", "plane", "far", "const"])
def test_selection_list_and_fill_equal_the_reference(name, s):
    from disn_amd import ops
    R = 16
    vol, iso = _fields(R)[name]
    vol = np.ascontiguousarray(vol.astype(np.float32)).ravel()
    dev = torch.from_numpy(vol).cuda()
    for margin in (0.0, 0.5):
        for rounds in (0, 1, 2):
            grid = dev.clone()
            mask, idx, counts = ops.grid_band_select(grid, R, s, iso, margin, rounds)
            nband, ncell = (int(v) for v in counts.tolist())
            ref_mask = G.select(vol, R, s, iso, margin, rounds)
            ref_band = np.nonzero(G.band_mask(ref_mask, R, s))[0]
            tag = (name, s, margin, rounds)
            assert np.array_equal(mask.cpu().numpy().reshape(ref_mask.shape), ref_mask.astype(np.int32)), tag
            assert ncell == int(ref_mask.sum()) and nband == ref_band.size, tag
            got = idx[:nband].cpu().numpy()
            assert np.array_equal(np.sort(got), ref_band) and np.array_equal(got, np.sort(got)), tag
            assert torch.equal(grid, dev), "the selection wrote to the grid"
            ops.grid_band_fill(grid, R, s, mask)
            ref = G.fill(vol, ref_mask, R, s)
            assert np.array_equal(grid.cpu().numpy().view(np.uint32), ref.view(np.uint32)), tag
            if name in ("far", "const"):                   # nothing to evaluate: the grid is all lattice and fill
                assert nband == 0 and ncell == 0, tag
            else:
                assert nband > 0, tag
                if margin == 0.0 and rounds == 0:          # the bare rule leaves the cells without a crossing alone
                    assert nband < vol.size - (R // s + 1) ** 3, tag
    if name == "plane":                                    # margin 0, no dilation: the last layer of cells in x, nothing else
        m = G.select(vol, R, s, iso, 0.0, 0).reshape((R // s,) * 3)
        assert m[:, :, -1].all() and not m[:, :, :-1].any()


# ------------------------------------------------------------------ 2. evaluated points are the dense grid's
@pytest.mark.parametrize("s,margin,rounds", [(2, 0.5, 1), (4, 0.5, 0), (4, 0.0, 0)])
def test_evaluated_points_are_the_dense_grid_and_the_rest_is_the_fill(eng, view, s, margin, rounds):
    enc, dense, dense_np = view
    R = 32
    iso = float(np.median(dense_np))
    band, stats = eng.query_grid_band(enc, 0, O.DEMO_TRANS_MAT, BOX, R, iso=iso, stride=s, margin=margin, dilate=rounds)
    torch.cuda.synchronize()
    got = band.cpu().numpy()
    mask = G.select(got, R, s, iso, margin, rounds)        # from the device's own coarse values
    ev = G.evaluated_mask(mask, R, s)
    print("R=32 s=%d margin=%g dilate=%d: %s, evaluated share %.3f" % (s, margin, rounds, stats, ev.mean()))
    assert stats == {"coarse_points": (R // s + 1) ** 3, "band_points": int(ev.sum()) - (R // s + 1) ** 3,
                     "active_cells": int(mask.sum()), "total_points": (R + 1) ** 3}
    assert stats["band_points"] > 0
    evd = torch.from_numpy(ev).cuda()
    assert torch.equal(band[evd], dense[evd]), "an evaluated point differs from the dense fused grid"
    ref = G.fill(got, mask, R, s)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), "a filled point differs from the reference fill"
    if margin == 0.0:
        assert (~ev).any(), "no point was left to fill"


def test_band_needs_the_fused_kernels_and_a_valid_stride(eng, view):
    from disn_amd.engine import SdfEngine
    enc = view[0]
    with pytest.raises(ValueError, match="stride"):
        eng.query_grid_band(enc, 0, O.DEMO_TRANS_MAT, BOX, 32, stride=3)
    with pytest.raises(ValueError, match="multiple"):
        eng.query_grid_band(enc, 0, O.DEMO_TRANS_MAT, BOX, 30, stride=4)
    plain = SdfEngine(None, weights=eng.weights, fused=False)
    with pytest.raises(ValueError, match="fused"):
        plain.query_grid_band(enc, 0, O.DEMO_TRANS_MAT, BOX, 32)


# ------------------------------------------------------------------ 3. everything active is the dense grid
def test_everything_active_is_the_dense_grid(eng, view, monkeypatch):
    enc, dense, _ = view
    band, stats = eng.query_grid_band(enc, 0, O.DEMO_TRANS_MAT, BOX, 32, margin=1e30)
    assert torch.equal(band, dense)
    assert stats["band_points"] + stats["coarse_points"] == stats["total_points"] == 33 ** 3
    assert stats["active_cells"] == 8 ** 3
    # ... and in chunks with a ragged tail (lattice 729 = 600 + 129, band 35208 = 58 x 600 + 408)
    monkeypatch.setattr(eng, "BAND_CHUNK", 600, raising=False)
    out = torch.full((33 ** 3,), float("nan"), device=dense.device)
    band2, stats2 = eng.query_grid_band(enc, 0, O.DEMO_TRANS_MAT, BOX, 32, stride=4, margin=1e30, out=out)
    assert band2 is out and torch.equal(band2, dense) and stats2 == stats


# ------------------------------------------------------------------ 4. recall on the config-1 field
def test_config1_band_misses_nothing_and_meshes_like_the_dense_grid(eng, kat):
    """float64 table (tests/test_grid_band_host.py), stride 4, margin 0.5, dilate 1: 1845 of 4096 cells, share 0.475"""
    from disn_amd import isosurface
    R, box = 64, [-1, -1, -1, 1, 1, 1]
    enc = eng.encode(kat["demo_img"].astype(np.float32) / np.float32(255.0))
    dense = eng.query_grid(enc, 0, O.DEMO_TRANS_MAT, box, R, fused=True)
    band, stats = eng.query_grid_band(enc, 0, O.DEMO_TRANS_MAT, box, R, iso=0.0, stride=4, margin=0.5, dilate=1)
    torch.cuda.synchronize()
    dense_np = dense.cpu().numpy()
    mask = G.select(dense_np, R, 4, 0.0, 0.5, 1)
    share = (stats["band_points"] + stats["coarse_points"]) / float(stats["total_points"])
    lost = G.missed(dense_np, mask, 4, 0.0)
    print("config 1 on the device: %s, share %.4f, surface cells %d, missed %d" % (
        stats, share, int(G.surface_cells(dense_np, 0.0).sum()), lost))
    assert stats["active_cells"] == int(mask.sum())
    assert lost == 0
    assert abs(stats["active_cells"] - 1845) <= 0.01 * 1845
    assert abs(share - 0.475) <= 0.01
    vb, fb = isosurface.marching_cubes(band, box, R, 0.0)
    vd, fd = isosurface.marching_cubes(dense, box, R, 0.0)
    assert len(fd) > 0
    assert torch.equal(vb, vd) and torch.equal(fb, fd)
    assert not torch.equal(band, dense)                    # (the meshes agree although half of the tensor is interpolated)


# ------------------------------------------------------------------ 5. the group path
def test_reconstruct_band_equals_per_view_band_then_marching_cubes(eng):
    from disn_amd import create_sdf as cs, isosurface
    feed = O.synth_inputs(21, 3, 8)
    imgs = feed["imgs"] * np.array([1.0, 0.5, 0.75], np.float32).reshape(3, 1, 1, 1)
    tms = np.stack([O.DEMO_TRANS_MAT[0], O.synth_trans_mat(30.0, 25.0, 0.8), O.synth_trans_mat(80.0, 25.0, 0.8)]
                   ).astype(np.float32)
    boxes = np.asarray([[-1.0, -1.0, -1.0, 1.0, 1.0 + 0.05 * b, 1.0] for b in range(3)], np.float64)
    R, band = 32, (4, 0.5, 1)
    enc = eng.encode(imgs)
    iso = float(eng.query_grid(enc, 0, tms, boxes[0], R, fused=True).median())
    host = lambda m: (m[0].cpu().numpy(), m[1].cpu().numpy())
    dense_before = [host(m) for m in cs.reconstruct(eng, imgs, tms, boxes, R, iso)]
    got = [host(m) for m in cs.reconstruct(eng, imgs, tms, boxes, R, iso, band=band)]
    grids = cs.create_sdf(eng, imgs, tms, boxes, R, band=band, iso=iso)
    dense_after = [host(m) for m in cs.reconstruct(eng, imgs, tms, boxes, R, iso)]
    assert len(got) == 3 and sum(len(f) > 0 for _, f in got) >= 1
    for b in range(3):
        grid, stats = eng.query_grid_band(enc, b, tms, boxes[b], R, iso=iso, stride=4, margin=0.5, dilate=1)
        assert torch.equal(grids[b], grid), "view %d: the group's grid differs from query_grid_band's" % b
        v, f = host(isosurface.marching_cubes(grid, boxes[b], R, iso))
        assert np.array_equal(got[b][1], f) and np.array_equal(got[b][0].view(np.uint32), v.view(np.uint32)), b
        assert np.array_equal(dense_before[b][1], dense_after[b][1])
        assert np.array_equal(dense_before[b][0].view(np.uint32), dense_after[b][0].view(np.uint32))
        d = eng.query_grid(enc, b, tms, boxes[b], R, fused=True)
        vd, fd = host(isosurface.marching_cubes(d, boxes[b], R, iso))
        assert np.array_equal(dense_after[b][1], fd) and np.array_equal(dense_after[b][0], vd)

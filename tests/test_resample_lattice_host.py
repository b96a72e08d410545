"""What the exact pixel lattice (tests/resample_lattice.py) reaches, asserted on the CPU with the oracle alone: the kernels
of tests/test_gpu_resample_lattice.py are only as well tested as this table is complete.  Every assertion is a
condition on the table; none may be relaxed to make the table smaller."""
import numpy as np
import pytest

import resample_lattice as L
import sdf_grad_reference as R
from oracle import disn_oracle as O
from test_gpu_train_edges import _HAND_PLACED

F32 = np.float32


@pytest.fixture(scope="module")
def lat():
    return L.lattice(True)


@pytest.fixture(scope="module")
def finite(lat):
    """(raw, table) without the NaN row"""
    keep = np.arange(len(lat["raw"])) != lat["nan"]
    return lat["raw"][keep], lat["table"][keep]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_size_and_cross_product(lat):
    a = L.axis_values()
    n = len(a)
    assert len(lat["pts"]) <= L.MAX_POINTS and len(np.unique(a)) == n
    cross = lat["raw"][:n * n].reshape(n, n, 2)
    assert np.array_equal(cross[:, :, 0], np.repeat(a[:, None], n, axis=1))      # every x representative with ...
    assert np.array_equal(cross[:, :, 1], np.repeat(a[None, :], n, axis=0))      # ... every y representative
    print("lattice: %d representatives per axis, %d points" % (n, len(lat["pts"])))


def test_projection_is_exact_in_float32_and_float64(lat):
    xy = O.get_img_points(lat["pts"][None], lat["camera"])[0]
    assert np.array_equal(_bits(xy), _bits(lat["table"]))                       # bit for bit, the NaN row included
    assert np.isnan(xy[lat["nan"]]).all() and np.isnan(lat["pts"][lat["nan"], 0])
    assert np.isfinite(np.delete(xy, lat["nan"], axis=0)).all()
    # the raw coordinate itself, before the clamp, in float64 as well: both precisions agree on the cell and the clamp
    p = lat["pts"][:lat["nan"]].astype(np.float64) @ L.CAMERA[:3].astype(np.float64) + L.CAMERA[3]
    assert np.array_equal(p[:, :2] / p[:, 2:3], lat["raw"][:lat["nan"]].astype(np.float64))
    assert np.abs(lat["pts"][:lat["nan"]]).max() < 1.2


def test_nan_point_has_zero_features(lat):
    fm = np.random.default_rng(0).standard_normal((1, 137, 137, 3)).astype(np.float32)
    rows = L.oracle_rows(fm, lat["table"])
    assert not rows[lat["nan"]].any() and rows[:lat["nan"]].any(axis=1).all()


@pytest.mark.parametrize("axis", [0, 1])
def test_cells_fractions_and_clamps_per_axis(finite, axis):
    raw, table = finite
    r, t = raw[:, axis], table[:, axis]
    cell = np.floor(t).astype(np.int64)
    assert set(cell.tolist()) == set(range(137))                               # every cell 0..136
    frac = t - np.floor(t)
    inside = (r > 0) & (r < 136)
    for f in L.FRACTIONS:
        for where, cells in (("interior", range(1, 135)), ("cell 0", (0,)), ("cell 135", (135,))):
            hit = (frac == F32(f)) & np.isin(cell, list(cells)) & ((r >= 0) if f == 0.0 else inside)
            assert hit.any(), "fraction %r in %s" % (f, where)
    assert (r == 0).any() and (r == 136).any() and (t == 136).any()            # 0 and 136 exactly
    assert ((r < 0) & (t == 0)).any() and ((r > 136) & (t == 136)).any()       # the clamp from below and from above


def test_edges_and_corners_are_reached_from_outside(finite):
    raw, _ = finite
    lo, hi = raw < 0, raw > 136
    inside = (raw > 0) & (raw < 136)
    for axis in (0, 1):                                                        # the four edges: one clamp alone
        assert (lo[:, axis] & inside[:, 1 - axis]).any() and (hi[:, axis] & inside[:, 1 - axis]).any()
    for cx in (lo, hi):                                                        # the four corners: both clamps
        for cy in (lo, hi):
            assert (cx[:, 0] & cy[:, 1]).any()


def test_negative_zero_is_in_the_raw_xy_table():
    """68 + (-68) rounds to +0: no point projects to -0.0, so the entries that take pixel coordinates carry it, with
    -1, (-1, 0), (136, 137), 137, NaN and the infinities"""
    xy = L.raw_xy_table(_HAND_PLACED)
    assert len(xy) <= 2048 + 64
    rows = {tuple(r) for r in xy[np.isfinite(xy).all(axis=1)].tolist()}
    for want in ((-1, -1), (-1, 0), (136, 137), (137, 137), (137, 5), (0, 0), (136, 136)) + tuple(map(tuple, _HAND_PLACED)):
        assert tuple(float(v) for v in want) in rows, want
    assert (np.signbit(xy) & (xy == 0)).any()
    assert np.isnan(xy).any() and np.isposinf(xy).any() and np.isneginf(xy).any()
    table = L.lattice(True)["table"]
    assert not (np.signbit(table) & (table == 0)).any()


@pytest.mark.parametrize("k", range(5))
def test_every_tap_row_relation_pair_occurs(finite, k):
    cells = L.cells_of(finite[1])
    want = L.all_relation_pairs(k)
    got = L.relation_pairs(cells, k)
    print("tap %d: %d (row class, column class) pairs exist: %s" % (
        k, len(want), sorted((L.RELATION_NAMES[a], L.RELATION_NAMES[b]) for a, b in want)))
    assert got == want
    per_axis = set(L.tap_relations()[k].tolist())
    assert want == {(a, b) for a in per_axis for b in per_axis}                 # (the classes of the two axes are free)
    # the clamp-only class: where 'same pair' exists only at cell 136 it is reached by the coordinate 136 alone
    if set(np.nonzero(L.tap_relations()[k] == L.SAME)[0].tolist()) == {136}:
        assert (L.SAME, L.SAME) in got


@pytest.mark.parametrize("k", range(5))
def test_last_tap_row_and_column_are_touched(finite, k):
    cells = L.cells_of(finite[1])
    last = L.last_row_cells()[k]
    assert len(last) and np.isin(cells[:, 0], last).any() and np.isin(cells[:, 1], last).any()
    assert (np.isin(cells[:, 0], last) & np.isin(cells[:, 1], last)).any()      # ... and the last corner pixel


# ---- the decoder behind the gather: teeth, and how much of the gradient test remains comparable --------------------
@pytest.fixture(scope="module")
def world():
    lat = L.lattice(False)
    return lat, L.oracle_map(0), L.weight_arrays()


def test_a_one_cell_slip_is_a_hundred_tolerances(world):
    """the float64 decoder on the oracle's rows at the table and at the table shifted by one cell in x: they differ by
    more than 100 x (1e-5 + 1e-5 |ref|), the bar of the random-point tests, at >= 95 % of the interior points"""
    lat, fm, W = world
    ins = L.interior(lat["raw"])
    xy = lat["table"][ins]
    rot = L.mlp_points(len(lat["pts"]))[0][ins]
    emb = L.embedding(0)
    ref = L.decoder64(L.oracle_rows(fm, xy), rot, emb, W)
    off = L.decoder64(L.oracle_rows(fm, xy + np.array([1.0, 0.0], np.float32)), rot, emb, W)
    tol = 1e-5 + 1e-5 * np.abs(ref)
    share = float((np.abs(off - ref) > 100 * tol).mean())
    print("teeth: %d interior points, a one-cell slip exceeds 100 tolerances at %.1f %%, median |d| %.3g, |pred| max "
          "%.3g (tap gain %g)" % (ins.sum(), 100 * share, np.median(np.abs(off - ref)), np.abs(ref).max(), L.TAP_GAIN))
    assert ins.any() and share >= 0.95


def test_gradient_reference_keeps_half_of_the_lattice(world):
    """sdf_grad_reference on the lattice with only the ReLU-kink margin as exclusion (no near_line, no clamped): the
    share of comparable points, and the convention on a line and on a clamp that the reference's text states"""
    lat, fm, W = world
    ref = R.forward_mode(W, L.embedding(0)[0], fm[0], lat["pts"], L.CAMERA, np.float64)
    ok = ref["margin"] >= R.MARGIN
    print("query_grad lattice: %.1f %% of the %d points are off every ReLU kink by %g" % (100 * ok.mean(), len(ok), R.MARGIN))
    assert ok.mean() >= L.GRAD_MIN_SHARE
    assert np.array_equal(ref["uv_raw"], lat["raw"].astype(np.float64))
    # a clamp is active exactly where the raw coordinate is not in the open interval (0, 136) ...
    raw = lat["raw"]
    assert np.array_equal(ref["clamped_uv"], ~((raw > 0) & (raw < 136)))
    # ... and there the gradient does not depend on that axis: both clamped -> only the point MLPs' own gradient, the
    # same for every such point's image part; moving along a clamped axis changes nothing
    both = ref["clamped_uv"].all(axis=1)
    assert both.any() and ref["near_line"].mean() > 0.3                          # most of the table sits on a line

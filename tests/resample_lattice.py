"""The exact pixel lattice (not a test module): a camera and a table of points whose float32 projection is EXACTLY a
chosen pixel coordinate, so that every copy of the projection-and-resampling rule (include/disn_amd.h, disn_project)
can be fed cell lines, the two clamps, the image corners and every tap-row relation of the legacy resize table.
What the table reaches is asserted on the CPU by tests/test_resample_lattice_host.py; the kernels run on it in
tests/test_gpu_resample_lattice.py.

The camera: trans_mat = [[64,0,0],[0,64,0],[0,0,0],[68,68,1]] ([4,3], right-multiply) and the point
((px - 68) / 64, (py - 68) / 64, z).  The pinned float32 expression ((x T0 + y T1) + z T2) + T3 of oracle.get_img_points
gives (px, py, 1) without a rounding for every px, py with at most 16 fractional bits (x * 64 and the sum with 68 are
exact; z meets zeros only), so the projected coordinate is clip(p, 0, 136) in float32 AND in float64: both agree on the
cell.  |x|, |y| stay below 1.2, z is uniform in [-1, 1): inputs of ordinary size for the entries that feed the point to
the MLP as well.

Everything here is derived from the oracle (O.resize_index_table, O.get_img_points, O.resampler); nothing restates a
kernel.  The table is a CROSS PRODUCT of per-axis representatives (``axis_values``: the clamps from either side, 0 and
136, the four fractions in cell 0, an interior cell and cell 135, and the first and the last cell of every tap-row
relation of every tap),
followed by three sweeps that visit every cell 0..136 on either axis, and one point whose x is NaN.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import disn_oracle as O

F32 = np.float32
TAP_SHAPES = ((224, 64), (112, 128), (56, 256), (28, 512), (14, 512))      # conv1_2 .. conv5_3: (hw, channels)
CAMERA = np.array([[64, 0, 0], [0, 64, 0], [0, 0, 0], [68, 68, 1]], np.float32)
EPS = 2.0 ** -10
FRACTIONS = (0.0, EPS, 0.5, 1.0 - EPS)
INTERIOR_CELL = 67
SAME, SHIFTED, DISJOINT = 0, 1, 2
RELATION_NAMES = ("same pair", "shifted by one", "disjoint")
MAX_POINTS = 2048


# ---- the legacy resize table's relation of map pixel i to min(i + 1, 136) ------------------------------------------
@functools.lru_cache(maxsize=None)
def tap_relations() -> np.ndarray:
    """[5, 137] of SAME / SHIFTED / DISJOINT: how the source rows (lower, upper) of map pixel min(i + 1, 136) relate to
    those of map pixel i in tap k, from O.resize_index_table alone"""
    out = np.zeros((len(TAP_SHAPES), O.IMG_H), np.int64)
    nxt = np.minimum(np.arange(O.IMG_H) + 1, O.IMG_H - 1)
    for k, (hw, _) in enumerate(TAP_SHAPES):
        lo, hi, _ = O.resize_index_table(hw, O.IMG_H)
        same = (lo[nxt] == lo) & (hi[nxt] == hi)
        shifted = ~same & (lo[nxt] == hi)
        out[k] = np.where(same, SAME, np.where(shifted, SHIFTED, DISJOINT))
    return out


@functools.lru_cache(maxsize=None)
def last_row_cells() -> tuple:
    """per tap: the cells i whose corner pixels i, i + 1 (inside the image) read the last tap row hw - 1"""
    out = []
    nxt = np.minimum(np.arange(O.IMG_H) + 1, O.IMG_H - 1)
    for hw, _ in TAP_SHAPES:
        _, hi, _ = O.resize_index_table(hw, O.IMG_H)
        out.append(np.nonzero((hi == hw - 1) | (hi[nxt] == hw - 1))[0])
    return tuple(out)


# ---- the per-axis representatives ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def axis_values() -> np.ndarray:
    """the raw (unclamped) coordinates one axis takes in the cross product, float32"""
    vals = [-3.5, -0.25, 136.5, 140.25]                                      # p < 0 and p > 136: the clamp from either side
    for cell in (0, INTERIOR_CELL, 135):
        vals += [cell + f for f in FRACTIONS]
    vals.append(136.0)
    cells = {int(np.floor(min(max(v, 0.0), 136.0))) for v in vals}
    rel = tap_relations()
    for k in range(rel.shape[0]):
        for c in np.unique(rel[k]):
            where = np.nonzero(rel[k] == c)[0]
            for i in (int(where[0]), int(where[-1])):                        # the first and the last cell of the class
                if i not in cells:
                    cells.add(i)
                    vals.append(i + (0.25 if len(vals) % 2 else 0.8125))
    return np.asarray(vals, np.float32)


def _sweeps() -> np.ndarray:
    """three passes over the 137 cells of the x axis, the y cell a different permutation of 0..136 in each (137 is
    prime), fractions with 12 bits: every cell of either axis occurs (cell 136 holds the coordinate 136 only)"""
    rng = np.random.default_rng(137)
    i = np.arange(O.IMG_W)
    out = []
    for mul, add in ((37, 5), (101, 77), (136, 136)):
        j = (i * mul + add) % O.IMG_W
        fx, fy = (rng.integers(1, 4096, O.IMG_W) / 4096.0 for _ in range(2))
        out.append(np.stack([np.where(i == 136, 136.0, i + fx), np.where(j == 136, 136.0, j + fy)], axis=1))
    return np.concatenate(out).astype(np.float32)


@functools.lru_cache(maxsize=None)
def raw_table() -> np.ndarray:
    """[n, 2] float32 raw pixel coordinates (x = column, y = row): axis_values x axis_values, then the sweeps.  Every
    value has at most 16 fractional bits."""
    a = axis_values()
    gx, gy = np.meshgrid(a, a, indexing="ij")
    raw = np.concatenate([np.stack([gx.ravel(), gy.ravel()], axis=1), _sweeps()]).astype(np.float32)
    assert np.array_equal(raw * 65536.0, np.round(raw * 65536.0))
    raw.setflags(write=False)
    return raw


def points_of(raw: np.ndarray, seed: int = 7) -> np.ndarray:
    """raw [n, 2] -> the float32 points [n, 3] that CAMERA projects onto them; z uniform in [-1, 1)"""
    raw = np.asarray(raw, np.float32)
    z = np.random.default_rng(seed).uniform(-1.0, 1.0, len(raw)).astype(np.float32)
    xy = ((raw - F32(68.0)) / F32(64.0)).astype(np.float32)
    return np.concatenate([xy, z[:, None]], axis=1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def lattice(with_nan: bool = True) -> dict:
    """{"raw" [n,2]: the raw coordinates, "table" [n,2]: the intended projected coordinates clip(raw, 0, 136), "pts"
    [n,3], "camera" [1,4,3], "nan": index of the point whose x is NaN (its raw / table rows are NaN) or None}.
    ``with_nan``: for the gather-only entries; the entries that feed the same point to the MLP get the table without it."""
    raw = np.array(raw_table())
    pts = points_of(raw)
    nan = None
    if with_nan:
        nan = len(raw)
        raw = np.concatenate([raw, np.full((1, 2), np.nan, np.float32)])
        pts = np.concatenate([pts, np.array([[np.nan, 0.25, -0.5]], np.float32)])
    table = np.minimum(F32(136.0), np.maximum(F32(0.0), raw)).astype(np.float32)      # (NaN stays NaN)
    assert len(pts) <= MAX_POINTS
    out = {"raw": raw, "table": table, "pts": pts, "camera": CAMERA[None].copy(), "nan": nan}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def raw_xy_extras(hand_placed) -> np.ndarray:
    """what only an entry that takes pixel coordinates can be given: outside the resampler's range (-1, 137 and beyond),
    the half-outside strips, -0.0, NaN and the infinities, on top of the hand-placed list of test_gpu_train_edges.py"""
    inf, nan = np.inf, np.nan
    more = [[-1, -1], [-1, 0], [0, -1], [136, 137], [137, 136], [137, 137], [-0.0, -0.0], [-0.0, 50.5], [50.5, -0.0],
            [nan, 5], [5, nan], [nan, nan], [inf, 5], [5, inf], [-inf, 5], [5, -inf], [inf, -inf], [-EPS, 136 + EPS],
            [-1 + EPS, 137 - 2 * EPS]]
    return np.asarray(list(hand_placed) + more, np.float32)


def raw_xy_table(hand_placed) -> np.ndarray:
    """[m, 2]: the lattice's projected table (the NaN row included) followed by the extras"""
    return np.concatenate([lattice(True)["table"], raw_xy_extras(hand_placed)]).astype(np.float32)


# ---- classification of projected coordinates, by the oracle --------------------------------------------------------
def cells_of(table: np.ndarray) -> np.ndarray:
    """floor of the finite rows of a projected table, int64 [n, 2]"""
    t = np.asarray(table, np.float32)
    return np.floor(t[np.isfinite(t).all(axis=1)]).astype(np.int64)


def relation_pairs(cells: np.ndarray, k: int) -> set:
    """the (row class, column class) pairs of tap k that the cells [n, 2] = (x cell, y cell) reach"""
    rel = tap_relations()[k]
    return set(zip(rel[cells[:, 1]].tolist(), rel[cells[:, 0]].tolist()))


def all_relation_pairs(k: int) -> set:
    """... and those that exist among the 137 x 137 cells"""
    i = np.arange(O.IMG_H)
    gx, gy = np.meshgrid(i, i, indexing="ij")
    return relation_pairs(np.stack([gx.ravel(), gy.ravel()], axis=1), k)


def interior(raw: np.ndarray) -> np.ndarray:
    """bool [n]: points strictly inside the image whose cell has a neighbour cell to the right (x + 1 <= 136)"""
    r = np.asarray(raw, np.float32)
    with np.errstate(invalid="ignore"):
        return (r[:, 0] > 0) & (r[:, 0] <= 135) & (r[:, 1] > 0) & (r[:, 1] < 136)


# ---- the synthetic features and the decoder on them ----------------------------------------------------------------
TAP_GAIN = 1.0            # standard-normal taps as they are: the teeth condition holds (test_resample_lattice_host.py)
WEIGHT_SEED = 0           # WeightStore.random_init(0, "he"): the store of tests/test_gpu_smallest_shapes.py
GRAD_MIN_SHARE = 0.5


@functools.lru_cache(maxsize=None)
def synthetic_taps(image: int = 0) -> tuple:
    """five standard-normal taps [1, hw, hw, ch] float32 (signed: a maximum over views is no maximum of ReLU outputs)"""
    rng = np.random.default_rng(1000 + image)
    taps = tuple((rng.standard_normal((1, hw, hw, ch), dtype=np.float32) * F32(TAP_GAIN)).astype(np.float32)
                 for hw, ch in TAP_SHAPES)
    for t in taps:
        t.setflags(write=False)
    return taps


@functools.lru_cache(maxsize=2)
def oracle_map(image: int = 0) -> np.ndarray:
    """[1, 137, 137, 1472]: concat of O.resize_bilinear_legacy(tap, 137, 137) -- row E of the oracle, built once"""
    fm = np.concatenate([O.resize_bilinear_legacy(t, O.IMG_H, O.IMG_W) for t in synthetic_taps(image)], axis=3)
    fm.setflags(write=False)
    return fm


@functools.lru_cache(maxsize=None)
def embedding(image: int = 0) -> np.ndarray:
    e = np.random.default_rng(2000 + image).standard_normal((1, 1024)).astype(np.float32)
    e.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def mlp_points(n: int) -> np.ndarray:
    """ordinary points for the MLP of the entries that take pts_rot separately"""
    p = np.random.default_rng(3000).uniform(-1.0, 1.0, (1, n, 3)).astype(np.float32)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def weight_arrays(seed: int = WEIGHT_SEED) -> dict:
    """the decoder variables of the suite's He store (oracle.init_weights is what WeightStore.random_init draws)"""
    W = O.init_weights(seed, mode="he")
    return {k: v for k, v in W.items() if k.startswith("sdfprediction")}


def decoder64(feat: np.ndarray, pts_rot: np.ndarray, emb: np.ndarray, W: dict) -> np.ndarray:
    """float64 pred_sdf [n] of the two decoder streams on feature rows [n, 1472]"""
    pc = np.asarray(pts_rot, np.float32).reshape(1, -1, 3)
    g = O.get_sdf_basic2(pc, np.asarray(emb, np.float32).reshape(1, -1), W, dtype=np.float64)
    l = O.get_sdf_basic2_imgfeat_twostream(pc, np.asarray(feat, np.float32)[None, :, None, :], W, dtype=np.float64)
    return (g + l)[0, :, 0]


def oracle_rows(fm: np.ndarray, xy: np.ndarray) -> np.ndarray:
    """O.resampler of one image's map at coordinates [n, 2] -> [n, C]"""
    return O.resampler(np.asarray(fm, np.float32), np.asarray(xy, np.float32)[None])[0]

"""float32 numpy restatement of the narrow-band grid evaluation (disn_amd/csrc/grid_band.hip), in the kernels' order of
operations: the cell rule, the dilation, the evaluated-point mask and the fill.  Everything works on the stored values
v = pred_sdf / sdf_weight of a flat (iz, iy, ix) grid of (res + 1)^3 points; "inside" is v < iso, as marching_cubes.hip's
mc_flags_point has it.  ``surface_cells`` / ``missed`` measure what a selection loses against the dense grid."""
import numpy as np

STRIDES = (2, 4, 8)


def _check(res, s):
    if s not in STRIDES:
        raise ValueError("stride must be one of %s, got %r" % (STRIDES, s))
    if res < s or res % s:
        raise ValueError("res %d is no multiple of the stride %d" % (res, s))


def _cube(grid, res):
    return np.asarray(grid, np.float32).reshape(res + 1, res + 1, res + 1)


def _corners(lat):
    """the 8 corner arrays [C,C,C] of the coarse cells of the lattice values [C+1,C+1,C+1], x fastest: index dz*4 + dy*2 + dx"""
    C = lat.shape[0] - 1
    return [lat[dz:dz + C, dy:dy + C, dx:dx + C] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]


def cell_minmax(grid, res, s):
    _check(res, s)
    c = _corners(_cube(grid, res)[::s, ::s, ::s])
    lo, hi = c[0], c[0]
    for v in c[1:]:
        lo, hi = np.minimum(lo, v), np.maximum(hi, v)
    return lo, hi


def cell_rule(grid, res, s, iso, margin):
    """bool [C,C,C]: lo - t < iso && hi + t >= iso with t = margin * (hi - lo), every step rounded to float32"""
    lo, hi = cell_minmax(grid, res, s)
    iso, margin = np.float32(iso), np.float32(margin)
    with np.errstate(over="ignore", invalid="ignore"):
        t = margin * (hi - lo)
        return ((lo - t) < iso) & ((hi + t) >= iso)


def dilate(mask, rounds):
    """``rounds`` rounds of 26-neighbourhood dilation, clipped at the box"""
    m = np.asarray(mask, bool)
    C = m.shape[0]
    for _ in range(int(rounds)):
        p = np.zeros((C + 2,) * 3, bool)
        p[1:-1, 1:-1, 1:-1] = m
        out = np.zeros_like(m)
        for dz in range(3):
            for dy in range(3):
                for dx in range(3):
                    out |= p[dz:dz + C, dy:dy + C, dx:dx + C]
        m = out
    return m


def select(grid, res, s, iso, margin, rounds):
    return dilate(cell_rule(grid, res, s, iso, margin), rounds)


def lattice_mask(res, s):
    """bool [(res+1)^3]: the coarse lattice (every index a multiple of s)"""
    _check(res, s)
    on = (np.arange(res + 1) % s) == 0
    return (on[:, None, None] & on[None, :, None] & on[None, None, :]).ravel()


def band_mask(mask, res, s):
    """bool [(res+1)^3]: the fine points in the closed box of an active coarse cell, the lattice points left out"""
    _check(res, s)
    n = res + 1
    out = np.zeros((n, n, n), bool)
    for cz, cy, cx in zip(*np.nonzero(np.asarray(mask, bool))):
        out[cz * s:cz * s + s + 1, cy * s:cy * s + s + 1, cx * s:cx * s + s + 1] = True
    return out.ravel() & ~lattice_mask(res, s)


def evaluated_mask(mask, res, s):
    return band_mask(mask, res, s) | lattice_mask(res, s)


def share(mask, res, s):
    return float(evaluated_mask(mask, res, s).sum()) / float((res + 1) ** 3)


def _lerp(a, b, t):
    u = np.float32(1.0) - t
    p = u * a
    q = t * b
    return p + q


def fill(grid, mask, res, s):
    """the filled grid: evaluated points keep ``grid``'s value, every other point gets the trilinear interpolant of the
    8 lattice corners of its coarse cell min(i // s, C - 1) -- x, then y, then z, each lerp (1 - t) * a + t * b in
    float32 -- clamped to the corners' [lo, hi]"""
    g = _cube(grid, res)
    C = res // s
    i = np.arange(res + 1)
    c = np.minimum(i // s, C - 1)
    t = ((i - c * s).astype(np.float32) / np.float32(s)).astype(np.float32)
    cz, cy, cx = c[:, None, None], c[None, :, None], c[None, None, :]
    tz, ty, tx = t[:, None, None], t[None, :, None], t[None, None, :]
    v = [[[g[(cz + dz) * s, (cy + dy) * s, (cx + dx) * s] for dx in (0, 1)] for dy in (0, 1)] for dz in (0, 1)]
    x = [[_lerp(v[dz][dy][0], v[dz][dy][1], tx) for dy in (0, 1)] for dz in (0, 1)]
    y = [_lerp(x[dz][0], x[dz][1], ty) for dz in (0, 1)]
    r = _lerp(y[0], y[1], tz)
    lo, hi = v[0][0][0], v[0][0][0]
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                lo, hi = np.minimum(lo, v[dz][dy][dx]), np.maximum(hi, v[dz][dy][dx])
    r = np.minimum(np.maximum(r, lo), hi).astype(np.float32)
    ev = evaluated_mask(mask, res, s)
    return np.where(ev, g.ravel(), r.ravel()).astype(np.float32)


def _res(grid):
    res = int(round(np.asarray(grid).size ** (1.0 / 3.0))) - 1
    if (res + 1) ** 3 != np.asarray(grid).size:
        raise ValueError("not a cubic grid")
    return res


def surface_cells(grid, iso):
    """bool [res,res,res]: the fine cells whose 8 corners are not all on one side of iso (the cells marching cubes
    emits triangles for)"""
    inside = _cube(grid, _res(grid)) < np.float32(iso)
    c = _corners(inside)
    any_in, all_in = c[0], c[0]
    for v in c[1:]:
        any_in, all_in = any_in | v, all_in & v
    return any_in & ~all_in


def missed(grid, mask, s, iso):
    """number of surface cells of ``grid`` that lie in a coarse cell the selection left inactive"""
    m = np.asarray(mask, bool)
    up = m.repeat(s, 0).repeat(s, 1).repeat(s, 2)
    return int((surface_cells(grid, iso) & ~up).sum())

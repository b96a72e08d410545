"""Dual contouring, host side: the specification ``isosurface.dual_contour_arrays`` checked by independent properties
(Hermite points = marching cubes' vertices, vertices on planes and IN cube corners, a closed oriented sphere, rows that
only count in the mean), the argument checks of the five C entries of include/dc/disn_amd_dc.h, the header itself, and
the flags and paths of the drivers.  No GPU: the device's bits are compared in tests/test_gpu_dual_contour.py."""
import glob
import os
import subprocess

import numpy as np
import pytest

import abi_table
import dual_contour_fixtures as F
from oracle import mc_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REG = 2.0 ** -10


def iso_mod():
    from disn_amd import isosurface
    return isosurface


# ------------------------------------------------------------------ 1. Hermite points
@pytest.mark.parametrize("fixture", [F.sphere(9, F.SKEW, 0.6, 0.05), F.noise(5)], ids=["sphere9", "noise5"])
def test_hermite_points_are_the_marching_cubes_vertices(fixture):
    vol, box, iso, _ = fixture
    n = round(vol.size ** (1.0 / 3.0))
    pts = iso_mod().hermite_points_arrays(vol, box, iso)
    ref, _ = O.marching_cubes(vol.reshape(n, n, n), box, iso)
    assert pts.dtype == np.float32 and pts.shape == ref.shape and len(pts) > 50
    assert np.array_equal(F.bits(pts), F.bits(ref))


def test_the_cell_visits_its_edges_in_the_order_of_the_case_table():
    assert [tuple(e) for e in O.gen.edge_geometry()] == [tuple(e) for e in iso_mod().DC_CUBE_EDGES]


# ------------------------------------------------------------------ 2. plane
def test_every_vertex_of_a_plane_lies_on_it():
    nrm, off = np.array([0.3, -0.5, 0.8]), 0.11
    _, _, v, f = F.mesh(F.plane(6, nrm, off))
    assert len(v) > 20 and len(f) > 20
    dist = np.abs(v.astype(np.float64) @ nrm - off) / np.linalg.norm(nrm)
    # a few float32 ulps of coordinates <= 1 plus the float32 crossing
    assert dist.max() <= 1e-6, dist.max()


# ------------------------------------------------------------------ 3. cube corner
def test_a_cube_keeps_its_corners_and_marching_cubes_cuts_them_off():
    h, c, r = F.CUBE_H, F.CUBE_C, REG
    fx = F.cube(8)
    pts, nrm, v, f = F.mesh(fx, r)
    vol = fx[0]
    assert np.array_equal(np.unique(np.abs(vol * 8)), np.unique(np.abs(vol * 8)).round())     # every value is dyadic
    corners = np.array([[sx, sy, sz] for sx in (-h, h) for sy in (-h, h) for sz in (-h, h)])
    vd = v.astype(np.float64)
    for corner in corners:
        # the mass point of a corner cell is c/3 from the corner and the regulariser pulls by r/(1+r) of that
        assert np.abs(vd - corner).max(1).min() <= r * c / 3 + 1e-6, corner
        near = np.linalg.norm(pts.astype(np.float64) - corner, axis=1).min()      # marching cubes' vertices
        assert abs(near - c / np.sqrt(2.0)) <= 1e-6, near
    q = np.abs(vd) - h                                                            # distance to the surface of the box
    outside = np.linalg.norm(np.maximum(q, 0.0), axis=1)
    dist = np.where((q <= 0).all(1), -q.max(1), outside)
    assert dist.max() <= r * c + 1e-6, dist.max()
    assert len(f) == 2 * len(pts)                                                 # no cut edge on the grid's boundary


# ------------------------------------------------------------------ 4. sphere
def test_a_sphere_is_closed_oriented_and_of_genus_zero():
    fx = F.sphere(12, F.UNIT, 0.6, 0.0, (0.0, 0.0, 0.0))
    vol, box, iso, _ = fx
    pts, _, v, f = F.mesh(fx)
    n = 13
    ins = vol.reshape(n, n, n) < np.float32(iso)
    cnt = sum(ins[dz:dz + 12, dy:dy + 12, dx:dx + 12].astype(int) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1))
    assert len(v) == int(((cnt != 0) & (cnt != 8)).sum())                         # nv = the active cells
    assert len(f) == 2 * len(pts)                                                 # every cut edge here is interior
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).astype(np.int64)
    directed, dcount = np.unique(e[:, 0] * len(v) + e[:, 1], return_counts=True)
    assert (dcount == 1).all()                                                    # once in each direction
    und, ucount = np.unique(np.sort(e, 1) @ np.array([len(v), 1]), return_counts=True)
    assert (ucount == 2).all()                                                    # in exactly two triangles
    assert O.mesh_is_closed_and_oriented(f)[0]
    assert len(v) - len(und) + len(f) == 2
    assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 0] != f[:, 2]).all()
    volume, _ = O.mesh_volume_area(v, f)
    assert volume > 0 and abs(volume - 4.0 / 3.0 * np.pi * 0.6 ** 3) < 0.05       # the normals point along +grad


def test_faces_on_the_boundary_are_left_open_and_counted_by_interior_edges():
    vol, box, iso, nat = F.sphere(6, F.UNIT, 1.1, 0.0, (0.0, 0.0, 0.0))            # the sphere leaves the box
    pts = iso_mod().hermite_points_arrays(vol, box, iso)
    v, f = iso_mod().dual_contour_arrays(vol, box, iso, nat(pts))
    n, R = 7, 6
    E = iso_mod()._DcEdges(vol, box, iso)
    u, w = (E.axis + 1) % 3, (E.axis + 2) % 3
    rows = np.arange(len(E.p))
    inner = ((E.idx[rows, u] >= 1) & (E.idx[rows, u] <= R - 1) & (E.idx[rows, w] >= 1) & (E.idx[rows, w] <= R - 1))
    assert 0 < inner.sum() < len(pts) and len(f) == 2 * inner.sum()


# ------------------------------------------------------------------ 5. rows and degenerate grids
def _reference_vertices(vol, box, iso, pts, nrm, reg):
    """per active cell, an independent statement: numpy.linalg on the rows with a usable normal, the mean over all"""
    iso_m = iso_mod()
    E = iso_m._DcEdges(vol, box, iso)
    n, R = E.n, E.R
    out = []
    for c in range(R ** 3):
        cx, cy, cz = c % R, (c // R) % R, c // (R * R)
        rows = [int(E.eidx[3 * (((cz + dz) * n + cy + dy) * n + cx + dx) + a]) for dx, dy, dz, a in iso_m.DC_CUBE_EDGES
                if E.flat[3 * (((cz + dz) * n + cy + dy) * n + cx + dx) + a]]
        if not rows:
            continue
        corner = np.array([E.ax[0][cx], E.ax[1][cy], E.ax[2][cz]], np.float64)
        hi = np.array([E.ax[0][cx + 1], E.ax[1][cy + 1], E.ax[2][cz + 1]], np.float64) - corner
        d = pts[rows].astype(np.float64) - corner
        g = nrm[rows].astype(np.float64)
        with np.errstate(all="ignore"):
            s = (g * g).sum(1)
        good = np.isfinite(s) & (s > 0)
        gh = g[good] / np.sqrt(s[good])[:, None]
        A = gh.T @ gh
        b = -(gh * (gh * d[good]).sum(1)[:, None]).sum(0)
        m = d.mean(0)
        lam = reg * np.trace(A) / 3 + 2.0 ** -40
        x = np.linalg.solve(A + lam * np.eye(3), lam * m - b)
        out.append((corner, hi, x, m))
    return out


def test_a_row_without_a_usable_normal_changes_nothing_but_the_mean():
    vol, box, iso, nat = F.noise(5)
    pts = iso_mod().hermite_points_arrays(vol, box, iso)
    nrm = nat(pts)
    bad = ~np.isfinite(nrm).all(1) | (nrm == 0).all(1)
    assert np.isnan(nrm).any() and np.isinf(nrm).any() and (nrm == 0).all(1).any() and 0 < bad.sum() < len(nrm) // 2
    v, _ = iso_mod().dual_contour_arrays(vol, box, iso, nrm, REG)
    # NaN, infinite and zero rows are one kind: the same bits whichever stands in a bad row
    for fill in (np.nan, np.inf, 0.0):
        other = nrm.copy()
        other[bad] = fill
        v2, _ = iso_mod().dual_contour_arrays(vol, box, iso, other, REG)
        assert np.array_equal(F.bits(v), F.bits(v2)), fill
    ref = _reference_vertices(vol, box, iso, pts, nrm, REG)
    assert len(ref) == len(v)
    checked = 0
    for (corner, hi, x, m), got in zip(ref, v.astype(np.float64)):
        if (x > 1e-4).all() and (x < hi - 1e-4).all():       # the clip is checked below; here the solve itself
            assert np.abs(corner + x - got).max() <= 1e-5
            checked += 1
        assert (got >= corner - 1e-6).all() and (got <= corner + hi + 1e-6).all()             # clipped to the cell
    assert checked >= 10


def test_a_cell_whose_rows_all_lack_a_normal_sits_at_its_mean():
    vol, box, iso, nat = F.noise(5)
    pts = iso_mod().hermite_points_arrays(vol, box, iso)
    for fill in (0.0, np.nan):
        nrm = np.full_like(pts, fill)
        v, _ = iso_mod().dual_contour_arrays(vol, box, iso, nrm, REG)
        ref = _reference_vertices(vol, box, iso, pts, np.zeros_like(pts), REG)
        want = np.array([corner + m for corner, _, _, m in ref])
        assert np.abs(v.astype(np.float64) - want).max() <= 1e-6


def test_degenerate_grids():
    m = iso_mod()
    for R in (1, 3):
        for value in (1.0, -1.0):                       # an empty grid, an all-inside grid
            vol = np.full((R + 1) ** 3, value, np.float32)
            assert m.hermite_points_arrays(vol, F.UNIT, 0.0).shape == (0, 3)
            assert m.grid_normals_arrays(vol, F.UNIT, 0.0).shape == (0, 3)
            v, f = m.dual_contour_arrays(vol, F.UNIT, 0.0, np.zeros((0, 3), np.float32))
            assert v.shape == (0, 3) and f.shape == (0, 3) and v.dtype == np.float32 and f.dtype == np.int32
    vol = np.array([-1, 1, 1, 1, 1, 1, 1, 1], np.float32)                          # R = 1: one corner inside
    pts = m.hermite_points_arrays(vol, F.UNIT, 0.0)
    v, f = m.dual_contour_arrays(vol, F.UNIT, 0.0, m.grid_normals_arrays(vol, F.UNIT, 0.0))
    assert len(pts) == 3 and v.shape == (1, 3) and f.shape == (0, 3)
    with pytest.raises(ValueError):
        m.dual_contour_arrays(vol, F.UNIT, 0.0, np.zeros((3, 3), np.float32), reg=0.0)
    with pytest.raises(ValueError):
        m.dual_contour_arrays(vol, F.UNIT, 0.0, np.zeros((2, 3), np.float32))


def test_grid_normals_follow_the_field():
    vol, box, iso, nat = F.sphere(12, F.UNIT, 0.6, 0.0, (0.0, 0.0, 0.0))
    pts = iso_mod().hermite_points_arrays(vol, box, iso)
    g = iso_mod().grid_normals_arrays(vol, box, iso).astype(np.float64)
    cos = (g / np.linalg.norm(g, axis=1, keepdims=True) * nat(pts)).sum(1)
    assert cos.min() > 0.99                               # central differences of a distance field at h = 1/6
    # a linear field: the finite differences are exact, whatever the cell sizes
    nrm = np.array([0.25, -0.5, 0.75])
    lin = (F.grid(F.SKEW, 4).astype(np.float64) @ nrm - 0.0625).astype(np.float32).reshape(-1)
    g = iso_mod().grid_normals_arrays(lin, F.SKEW, 0.0)
    assert len(g) > 10 and np.abs(g - nrm).max() <= 1e-5


# ------------------------------------------------------------------ 6. argument checks
ENTRIES = ("disn_dc_count_batch", "disn_dc_points_batch", "disn_dc_grid_normals_batch", "disn_dc_emit_batch")
NEW = ("disn_dc_workspace_bytes",) + ENTRIES


def _case(name, h, box):
    """the smallest legal call as {parameter: value}, in the prototype's order; device pointers are abi_table.FAKE"""
    need = h.disn_dc_workspace_bytes(1, 4)
    fake = abi_table.FAKE
    a = {"sdf": fake}
    if name != "disn_dc_count_batch":
        a["sdf_params_host"] = box.ctypes.data
    a.update(B=1, R=4, iso=0.0)
    if name == "disn_dc_count_batch":
        a["counts"] = fake
    elif name == "disn_dc_points_batch":
        a["points"] = fake
    elif name == "disn_dc_grid_normals_batch":
        a["normals"] = fake
    else:
        a.update(points=fake, normals=fake, reg=REG, verts=fake, faces=fake)
    a.update(ws=fake, ws_bytes=need, stream=None)
    return a


@pytest.mark.parametrize("name", ENTRIES)
def test_every_entry_refuses_bad_arguments_on_the_host(name):
    """every refused call returns its negative code; the device pointers are never mapped and there may be no device at
    all, so a call that got as far as a launch or a dereference would not return one"""
    from disn_amd import _lib
    h = _lib.lib()
    box = np.array([-1, -1, -1, 1, 1, 1], np.float64)
    fn = getattr(h, name)
    base = _case(name, h, box)
    protos = [p for p in _parse_dc_header() if p.name == name]
    assert [pn for _, pn in protos[0].params] == list(base)

    def call(**kw):
        return fn(*dict(base, **kw).values())

    pointers = [k for k in base if k not in ("B", "R", "iso", "reg", "ws_bytes", "stream")]
    assert len(pointers) >= 3
    for p in pointers:
        assert call(**{p: None}) == abi_table.E_ARG, p
    for size in ("B", "R"):
        for bad in (0, -1):
            assert call(**{size: bad}) == abi_table.E_ARG, (size, bad)
    if "reg" in base:
        for bad in (0.0, 1.5, float("nan"), -REG, float("inf")):
            assert call(reg=bad) == abi_table.E_ARG, bad
        assert call(reg=1.0, ws_bytes=base["ws_bytes"] - 1) == abi_table.E_WS       # 1 itself is legal
    assert call(ws_bytes=base["ws_bytes"] - 1) == abi_table.E_WS
    assert call(ws_bytes=0) == abi_table.E_WS
    assert call(R=1291, ws_bytes=1 << 62) == abi_table.E_SHAPE
    assert call(R=1290, B=2, ws_bytes=1 << 62) == abi_table.E_SHAPE
    assert call(B=abi_table.INT_MAX, R=4, ws_bytes=1 << 62) == abi_table.E_SHAPE    # refused before a box is read


def test_the_workspace_query_is_zero_beyond_the_limits():
    from disn_amd import _lib
    h = _lib.lib()
    q = h.disn_dc_workspace_bytes
    for B, R in ((0, 4), (-1, 4), (1, 0), (1, -1), (0, 0), (1, 1291), (2, 1290), (abi_table.INT_MAX, 4),
                 (1, abi_table.INT_MAX), (abi_table.INT_MAX, abi_table.INT_MAX)):
        assert q(B, R) == 0, (B, R)
    n = 5
    assert q(1, 4) >= 4 * (4 * 3 * n ** 3 + 2 * 4 ** 3) and q(2, 4) > q(1, 4) and q(1, 1000) > 0
    # the limits of disn_mc_*_batch: R in 1..1290 and 3 B (R+1)^3 < 2^32
    for B, R in ((1, 1), (1, 1125), (1, 1126), (1, 1290), (2, 1290), (3, 700), (43690, 31), (43691, 31)):
        assert (q(B, R) > 0) == (h.disn_mc_batch_workspace_bytes(B, R) > 0), (B, R)


def _parse_dc_header():
    path = os.path.join(ROOT, "include", "dc", "disn_amd_dc.h")
    text = abi_table.strip_comments(open(path).read())
    text = "\n".join(l for l in text.split("\n") if not l.lstrip().startswith("#"))
    out = []
    for ret, name, params in __import__("re").findall(r"([\w\s\*]+?)\b(disn_\w+)\s*\(([^)]*)\)\s*;", text):
        out.append(abi_table.Proto(" ".join(ret.split()), name, [abi_table.parse_param(p) for p in params.split(",")],
                                   "dc/disn_amd_dc.h"))
    return out


def test_the_header_declares_exactly_the_sixth_table():
    from disn_amd import _lib
    protos = {p.name: p for p in _parse_dc_header()}
    assert set(protos) == set(_lib.SIGNATURES_DC) == set(NEW)
    for name, p in protos.items():
        res, args = _lib.SIGNATURES_DC[name]
        assert abi_table.c_class(p.ret) == abi_table.binding_class(res), name
        assert len(p.params) == len(args), name
        for (ctype, pname), a in zip(p.params, args):
            assert abi_table.c_class(ctype) == abi_table.binding_class(a), (name, pname)
    for t in abi_table.binding_tables():
        assert not set(t) & set(_lib.SIGNATURES_DC)
    assert len(glob.glob(os.path.join(ROOT, "include", "*.h"))) == 5            # the five headers stay five
    assert _lib.ABI_VERSION == 10
    h = _lib.lib()
    for name in NEW:
        assert getattr(h, name).argtypes == _lib.SIGNATURES_DC[name][1]           # lib() binds the sixth table too


def test_the_header_compiles_as_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "dc/disn_amd_dc.h"\n'
                   "int main(void) {\n"
                   "  size_t (*ws)(int, int) = disn_dc_workspace_bytes;\n"
                   "  int (*count)(const float*, int, int, float, uint64_t*, void*, size_t, void*) = disn_dc_count_batch;\n"
                   "  int (*emit)(const float*, const double*, int, int, float, const float*, const float*, double, float*,\n"
                   "              int32_t*, void*, size_t, void*) = disn_dc_emit_batch;\n"
                   "  return ws == 0 || count == 0 || emit == 0 || DISN_ABI_VERSION != 10;\n"
                   "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I",
                        os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_build_lists_the_source_without_contraction_and_the_header():
    from disn_amd.csrc import build
    assert build.SOURCES["dual_contour.hip"] == ["-ffp-contract=off"] == build.SOURCES["marching_cubes.hip"]
    assert "dual_contour_sheets.hip" not in build.SOURCES               # both vertex rules are built from the one file
    for hdr in ("disn_amd_dc.h", "disn_amd_dc_sheets.h"):
        assert any(h.endswith(os.path.join("include", "dc", hdr)) for h in build.HEADERS)
    assert "grid_mesh.hpp" in build.HEADERS and "dual_contour_common.hpp" not in build.HEADERS
    csrc = os.path.join(ROOT, "disn_amd", "csrc")
    users = sorted(os.path.basename(f) for f in glob.glob(os.path.join(csrc, "*.hip"))
                   if '#include "grid_mesh.hpp"' in abi_table.strip_comments(open(f).read()))
    assert users == ["dual_contour.hip", "marching_cubes.hip"]
    assert "atomic" not in abi_table.strip_comments(open(os.path.join(csrc, "dual_contour.hip")).read()).lower()


# ------------------------------------------------------------------ 7. flags and paths
def test_flags_and_paths():
    from disn_amd import create_sdf, demo
    base = ["--test_lst_dir", "lists"]
    a = create_sdf.parser().parse_args(base)
    assert a.mesher == "mc" and a.dc_normals is None and a.dc_reg is None and create_sdf.dc_from_flags(a) is None
    a = create_sdf.parser().parse_args(base + ["--mesher", "dc"])
    assert create_sdf.dc_from_flags(a) == {"normals": "network", "reg": REG}
    a = create_sdf.parser().parse_args(base + ["--mesher", "dc", "--dc_normals", "grid", "--dc_reg", "0.25"])
    assert create_sdf.dc_from_flags(a) == {"normals": "grid", "reg": 0.25}
    d = demo.parser().parse_args(["--img", "x.png", "--mesher", "dc", "--dc_reg", "0.5"])
    assert create_sdf.dc_from_flags(d) == {"normals": "network", "reg": 0.5}
    assert create_sdf.dc_from_flags(demo.parser().parse_args(["--img", "x.png"])) is None
    for bad in (["--dc_reg", "0.5"], ["--dc_normals", "grid"], ["--mesher", "dc", "--dc_reg", "0"],
                ["--mesher", "dc", "--dc_reg", "1.5"], ["--mesher", "dc", "--dc_reg", "nan"]):
        with pytest.raises(ValueError):
            create_sdf.dc_from_flags(create_sdf.parser().parse_args(base + bad))
    with pytest.raises(SystemExit):
        create_sdf.parser().parse_args(base + ["--mesher", "tetra"])
    with pytest.raises(ValueError):
        create_sdf.dc_args("tetra")
    # the paths: unchanged without the flag, _dc directly behind <res+1>_<iso> with it
    old = create_sdf.result_obj_path("log", 64, 0.0)
    assert old == os.path.join("log", "test_objs", "65_0.0") == create_sdf.result_obj_path("log", 64, 0.0, mesher="mc")
    assert create_sdf.result_obj_path("log", 64, 0.0, mesher="dc") == old + "_dc"
    full = dict(cam_est=True, fuse=(3, "max"), clean=True, simplify=32, colour=True, smooth=4)
    assert create_sdf.result_obj_path("log", 64, 0.003, **full) == os.path.join(
        "log", "test_objs", "camest_fuse3max_65_0.003_comb_t4_s32_col")
    assert create_sdf.result_obj_path("log", 64, 0.003, mesher="dc", **full) == os.path.join(
        "log", "test_objs", "camest_fuse3max_65_0.003_dc_comb_t4_s32_col")

"""CPU tests of the Taubin smoothing: ``postprocess.smooth_arrays``, the host function that IS the specification of
mesh_smooth.hip, checked against geometry; the drivers' arguments and flags; the fifth header of the C ABI.
Bars used below, all the issue's:
  * the noisy sphere (sigma 0.01 on radius 0.4), 10 iterations, defaults, no cap: the RMS of |v| - 0.4 at most 0.5 times
    the input's (0.42 measured), the signed volume within [0.98, 1.02] of the input's (1.009 measured);
  * with ``max_move`` = r every coordinate stays within r of its input IN FLOAT64 BEFORE THE CAST: the float32 result is
    the rounding of a float64 in [v0 - r, v0 + r], so it lies between the float32 roundings of the two ends.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_smooth_fixtures as XF  # noqa: E402
from disn_amd import create_sdf as cs  # noqa: E402
from disn_amd import demo  # noqa: E402
from disn_amd import postprocess as P  # noqa: E402

NEW = ("disn_mesh_smooth_workspace_bytes", "disn_mesh_smooth_batch")


@pytest.fixture(scope="module", autouse=True)
def _built():
    from disn_amd.csrc import build
    build.build()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _moved(a, b):
    return (_bits(a) != _bits(b)).any(1)


# ------------------------------------------------------------------ the rule
def test_the_noisy_sphere_is_faired_and_keeps_its_volume():
    v, f = XF.noisy()
    assert v.shape == (642, 3) and f.shape == (1280, 3) and XF.sphere()[0].shape == (642, 3)
    out = P.smooth_arrays(v, f, iters=10)
    assert out.dtype == np.float32 and out.shape == v.shape
    rms = XF.radial_rms(out) / XF.radial_rms(v)
    vol = XF.signed_volume(out, f) / XF.signed_volume(v, f)
    print("radial RMS x %.4f, signed volume x %.5f" % (rms, vol))
    assert rms <= 0.5
    assert 0.98 <= vol <= 1.02
    # the plain Laplacian of the same strength shrinks: what the mu steps are there for
    shrunk = P.smooth_arrays(v, f, iters=10, mu=-1e-9)
    assert XF.signed_volume(shrunk, f) / XF.signed_volume(v, f) < vol - 0.01


@pytest.mark.parametrize("name", ["noisy", "patch", "messy"])
@pytest.mark.parametrize("r", [0.0, 0.003, 0.01])
def test_the_cap_is_a_box_around_the_input(name, r):
    v, f = XF.host_cases()[name]
    free = P.smooth_arrays(v, f, iters=5, pin_boundary=False)
    out = P.smooth_arrays(v, f, iters=5, pin_boundary=False, max_move=r)
    v64 = v.astype(np.float64)
    lo, hi = (v64 - r).astype(np.float32), (v64 + r).astype(np.float32)
    assert (out >= lo).all() and (out <= hi).all()
    if r == 0.0:
        assert np.array_equal(out, v)
    else:
        assert (np.abs(free.astype(np.float64) - v64) > r).any(), "the cap is reached at all"
        assert _moved(out, v).any()


def test_pinned_boundary_vertices_keep_their_bits():
    v, f = XF.patch()
    edge = XF.patch_boundary()
    assert np.array_equal(P.smooth_graph(f, len(v))[2], edge) and edge.sum() == 32
    pinned = P.smooth_arrays(v, f, iters=3)
    assert np.array_equal(_moved(pinned, v), ~edge)                    # every interior vertex moves, no boundary one
    free = P.smooth_arrays(v, f, iters=3, pin_boundary=False)
    assert _moved(free, v)[edge].all()


def test_the_messy_mesh():
    v, f = XF.messy()
    indptr, nbr, boundary = P.smooth_graph(f, len(v))
    assert np.diff(indptr).tolist() == [5, 4, 5, 4, 5, 4, 3, 2, 2, 2, 0]
    assert nbr[indptr[6]:indptr[7]].tolist() == [0, 2, 4]               # (6, 6, 4): the pair (6, 6) counts for nothing
    assert tuple(np.nonzero(boundary)[0]) == XF.MESSY_PINNED            # the duplicated face's edges are no boundary
    for iters in (1, 4):
        out = P.smooth_arrays(v, f, iters=iters)
        assert tuple(np.nonzero(_moved(out, v))[0]) == XF.MESSY_FREE
        kept = list(XF.MESSY_PINNED) + [XF.MESSY_ISOLATED]
        assert np.array_equal(_bits(out)[kept], _bits(v)[kept])
        free = P.smooth_arrays(v, f, iters=iters, pin_boundary=False)
        assert np.array_equal(_bits(free)[XF.MESSY_ISOLATED], _bits(v)[XF.MESSY_ISOLATED])
        assert _moved(free, v)[:10].all()
    assert np.signbit(v[7, 0]) and np.signbit(v[10, 0]) and 0 < v[8, 1] < np.finfo(np.float32).tiny


def test_the_order_and_the_rotation_of_the_faces_change_no_bit():
    for name in ("noisy", "patch", "messy"):
        v, f = XF.host_cases()[name]
        for pin in (True, False):
            want = P.smooth_arrays(v, f, iters=3, pin_boundary=pin, max_move=0.01)
            for seed in (1, 2):
                got = P.smooth_arrays(*XF.permuted(v, f, seed), iters=3, pin_boundary=pin, max_move=0.01)
                assert np.array_equal(_bits(got), _bits(want)), (name, pin, seed)
    # every face twice: nothing changes but the boundary set
    for name in ("patch", "messy", "noisy"):
        v, f = XF.host_cases()[name]
        twice = np.concatenate([f, f])
        assert not P.smooth_graph(twice, len(v))[2].any()
        a, b = P.smooth_graph(f, len(v)), P.smooth_graph(twice, len(v))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(_bits(P.smooth_arrays(v, twice, iters=3)),
                              _bits(P.smooth_arrays(v, f, iters=3, pin_boundary=False)))


def test_statuses_of_the_host_rule():
    v, f = XF.messy()
    bad = f.copy()
    bad[3, 1] = len(v)
    nan = v.copy()
    nan[4, 1] = np.nan
    far = v.copy()
    far[1, 2] = 2000.0
    inf = v.copy()
    inf[1, 2] = np.inf
    for vv, ff, want in ((v, bad, 2), (v, -f - 1, 2), (nan, f, 4), (far, f, 7), (inf, f, 4), (nan, bad, 4), (far, bad, 7),
                         (v, f, 0), XF.empty() + (0,)):
        out, status = P.smooth_arrays_status(vv, ff, iters=2)
        assert status == want == max(P.smooth_status(vv, ff), status)
        if want:
            assert np.array_equal(_bits(out), _bits(vv))
            with pytest.raises(ValueError):
                P.smooth_arrays(vv, ff, iters=2)
    sv, sf = XF.spike()
    assert np.abs(sv).max() <= 1024 and P.smooth_status(sv, sf) == 0
    out, status = P.smooth_arrays_status(sv, sf, **XF.SPIKE_KW)
    assert status == 7 and np.array_equal(out, sv)
    assert P.smooth_arrays_status(sv, sf, iters=1)[1] == 0               # the default factors stay inside
    assert P.smooth_arrays_status(sv, sf, max_move=5.0, **XF.SPIKE_KW)[1] == 0       # and so does the capped run
    assert P.STATUS_SMOOTH_RANGE == 7 and P.SMOOTH_MAX_ITERS == 64


def test_parameter_checks():
    v, f = XF.messy()
    for kw in ({"iters": 0}, {"iters": 65}, {"iters": 2.5}, {"iters": True}, {"lam": 0.0}, {"lam": 1.5}, {"lam": np.nan},
               {"mu": 0.0}, {"mu": -1.6}, {"mu": 0.3}, {"max_move": -1.0}, {"max_move": np.inf}, {"max_move": np.nan},
               {"max_move": [0.1, 0.2]}):
        with pytest.raises(ValueError):
            P.smooth_arrays(v, f, **kw)
    P.smooth_arrays(v, f, iters=64, lam=1.0, mu=-1.5, max_move=0.0)


# ------------------------------------------------------------------ the drivers' arguments and flags
def test_smooth_args_and_flags(tmp_path):
    assert cs.smooth_args(None) is None
    assert cs.smooth_args(3) == {"iters": 3, "lam": 0.5, "mu": -0.53, "cap": 0.5, "pin_boundary": True}
    assert cs.smooth_args({"iters": 7, "cap": None, "pin_boundary": 0, "mu": -0.6}) == {
        "iters": 7, "lam": 0.5, "mu": -0.6, "cap": None, "pin_boundary": False}
    for bad in (0, 65, 2.5, True, {"cap": 1.0}, {"iters": 3, "lam": 0.0}, {"iters": 3, "lam": 1.1}, {"iters": 3, "mu": 0.0},
                {"iters": 3, "mu": -2.0}, {"iters": 3, "cap": -0.5}, {"iters": 3, "cap": float("inf")},
                {"iters": 3, "cap": float("nan")}, {"iters": 3, "radius": 1.0}):
        with pytest.raises(ValueError, match="--smooth"):
            cs.smooth_args(bad)
    boxes = np.array([[-1, -1, -1, 1, 1, 1], [-0.5, -0.25, -0.25, 0.5, 0.25, 0.75]], np.float64)
    assert cs.smooth_cap(cs.smooth_args(3), boxes, 64).tolist() == [0.5 * 2 / 64, 0.5 * 1 / 64]
    assert cs.smooth_cap(cs.smooth_args({"iters": 3, "cap": None}), boxes, 64) is None
    base = ["--test_lst_dir", str(tmp_path / "none"), "--log_dir", str(tmp_path / "log")]
    a = cs.parser().parse_args(base)
    assert a.smooth is None and a.smooth_cap is None and a.smooth_free_boundary is False
    assert cs.smooth_from_flags(a) is None
    assert cs.smooth_from_flags(cs.parser().parse_args(base + ["--smooth", "10"])) == cs.smooth_args(10)
    got = cs.smooth_from_flags(cs.parser().parse_args(base + ["--smooth", "4", "--smooth_cap", "0.25",
                                                              "--smooth_free_boundary"]))
    assert got == {"iters": 4, "lam": 0.5, "mu": -0.53, "cap": 0.25, "pin_boundary": False}

    def boom(*a, **k):
        raise AssertionError("device work was reached")

    for bad in (["--smooth_cap", "0.5"], ["--smooth_free_boundary"], ["--smooth", "0"], ["--smooth", "65"],
                ["--smooth", "3", "--smooth_cap", "-1"], ["--smooth", "3", "--smooth_cap", "nan"],
                ["--smooth", "3", "--smooth_cap", "inf"]):
        with pytest.raises(ValueError, match="--smooth"):
            cs.main(base + bad, reconstruct_fn=boom)
    assert not os.path.exists(str(tmp_path / "log"))
    # demo takes the same flags, with the same refusals before any file is read
    d = demo.parser().parse_args(["--img", "x.png", "--smooth", "3", "--smooth_cap", "1"])
    assert cs.smooth_from_flags(d) == dict(cs.smooth_args(3), cap=1.0)
    for bad in (["--smooth_cap", "0.5"], ["--smooth", "100"]):
        with pytest.raises(ValueError, match="--smooth"):
            demo.main(["--img", str(tmp_path / "missing.png")] + bad)


def test_result_obj_path_puts_the_iterations_between_comb_and_cells():
    plain = cs.result_obj_path("log", 64, 0.0)
    assert cs.result_obj_path("log", 64, 0.0, smooth=None) == plain
    assert cs.result_obj_path("log", 64, 0.0, smooth=10) == plain + "_t10"
    assert cs.result_obj_path("log", 64, 0.0, clean=True, simplify=32, smooth=3, colour=True) == plain + "_comb_t3_s32_col"
    assert cs.result_obj_path("log", 64, 0.0, cam_est=True, fuse=(2, "max"), simplify=8, smooth=1).endswith(
        "camest_fuse2max_65_0.0_t1_s8")


def test_smooth_group_makes_one_call_for_the_meshes_with_triangles(monkeypatch):
    calls = []

    def fake(meshes, iters, lam, mu, pin, cap):
        calls.append((len(meshes), iters, lam, mu, pin, None if cap is None else list(cap)))
        return [("smoothed",) + tuple(m[1:]) for m in meshes], np.zeros(len(meshes), np.int32)

    monkeypatch.setattr(P, "smooth_meshes_device", fake)
    v, f = XF.messy()
    meshes = [(v, f), XF.empty(), (v, f, "normals")]
    boxes = [[-1, -1, -1, 1, 1, 1]] * 2 + [[0, 0, 0, 4, 2, 2]]
    out = cs.smooth_group(meshes, cs.smooth_args({"iters": 2, "cap": 0.25}), boxes, 16)
    assert calls == [(2, 2, 0.5, -0.53, True, [0.25 * 2 / 16, 0.25 * 4 / 16])]
    assert out[0][0] == "smoothed" and out[0][1] is f and out[1] is meshes[1] and out[2] == ("smoothed", f, "normals")
    assert cs.smooth_group(meshes, None, boxes, 16) == meshes and len(calls) == 1
    only_empty = [XF.empty()]
    assert cs.smooth_group(only_empty, cs.smooth_args(2), boxes[:1], 16)[0] is only_empty[0] and len(calls) == 1


# ------------------------------------------------------------------ the fifth header
def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return re.findall(r"\b(disn_[a-z0-9_]+)\s*\(", text)


def test_fifth_header_equals_the_fifth_table_and_the_others_stay():
    from disn_amd import _lib
    assert _declared("disn_amd_smooth.h") == list(NEW) == list(_lib.SIGNATURES_SMOOTH)
    assert not set(NEW) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_SIMPLIFY) | set(_lib.SIGNATURES_COLOUR)
                           | set(_lib.SIGNATURES_SAMPLE))
    assert set(_declared("disn_amd.h")) == set(_lib.SIGNATURES) and len(_declared("disn_amd.h")) == len(_lib.SIGNATURES)
    assert _declared("disn_amd_simplify.h") == list(_lib.SIGNATURES_SIMPLIFY)
    assert _declared("disn_amd_colour.h") == list(_lib.SIGNATURES_COLOUR)
    assert _declared("disn_amd_sample.h") == list(_lib.SIGNATURES_SAMPLE)
    header = open(os.path.join(ROOT, "include", "disn_amd.h")).read()
    assert re.search(r"#define DISN_ABI_VERSION 10\b", header) and "disn_mesh_smooth" not in header
    assert '#include "disn_amd.h"' in open(os.path.join(ROOT, "include", "disn_amd_smooth.h")).read()
    assert _lib.ABI_VERSION == 10 and _lib.lib().disn_abi_version() == 10
    h = _lib.lib()
    for name in NEW:
        fn = getattr(h, name)
        assert fn.restype is _lib.SIGNATURES_SMOOTH[name][0] and list(fn.argtypes) == _lib.SIGNATURES_SMOOTH[name][1]
    ws = h.disn_mesh_smooth_workspace_bytes
    assert ws(24, 100000, 200000) >= 200000 * 6 * 4 + 2 * 100000 * 12 and ws(1, 0, 0) > 0
    assert ws(5, 10, 10 ** 6) > ws(5, 10, 10) and ws(5, 10 ** 6, 10) > ws(5, 10, 10)
    for bad in ((0, 10, 10), (-1, 10, 10), (1, 2 ** 31, 10), (1, 10, (2 ** 31 - 1) // 3 + 1), (1, -1, 10), (1, 10, -1)):
        assert ws(*bad) == 0, bad
    # argument checks that need no device
    off, bad_off, some = np.zeros(2, np.int64), np.array([0, -1], np.int64), np.array([0, 3], np.int64)
    o = off.ctypes.data
    call = h.disn_mesh_smooth_batch
    ok = (10, 0.5, -0.53, 1)
    assert call(None, None, o, o, 1, *ok, None, None, None, None, 0, None) == -1                # no status, no ws
    assert call(None, None, bad_off.ctypes.data, o, 1, *ok, None, None, 1, 1, 1 << 30, None) == -1
    assert call(None, None, o, o, 0, *ok, None, None, 1, 1, 1 << 30, None) == -1
    assert call(None, None, some.ctypes.data, o, 1, *ok, None, None, 1, 1, 1 << 30, None) == -1  # no verts
    for bad in ((0, 0.5, -0.53, 1), (65, 0.5, -0.53, 1), (-3, 0.5, -0.53, 1), (10, 0.0, -0.53, 1), (10, 1.25, -0.53, 1),
                (10, float("nan"), -0.53, 1), (10, 0.5, 0.0, 1), (10, 0.5, -1.75, 1), (10, 0.5, float("nan"), 0)):
        assert call(None, None, o, o, 1, *bad, None, None, 1, 1, 1 << 30, None) == -1, bad
    for r in (float("nan"), float("inf")):
        cap = np.array([r], np.float64)
        assert call(None, None, o, o, 1, *ok, cap.ctypes.data, None, 1, 1, 1 << 30, None) == -1
    assert call(None, None, o, o, 1, *ok, None, None, 1, 1, 16, None) == -3


def test_fifth_header_compiles_as_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "disn_amd_smooth.h"\n'
                   "int main(void) {\n"
                   "  size_t (*ws)(int, int64_t, int64_t) = disn_mesh_smooth_workspace_bytes;\n"
                   "  int (*run)(const float*, const int32_t*, const int64_t*, const int64_t*, int, int, double, double,\n"
                   "             int, const double*, float*, int32_t*, void*, size_t, void*) = disn_mesh_smooth_batch;\n"
                   "  return ws == 0 || run == 0 || DISN_ABI_VERSION != 10 || DISN_SMOOTH_RANGE != 7 ||\n"
                   "         DISN_SMOOTH_MAX_ITERS != 64;\n"
                   "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I",
                        os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_build_lists_the_source_without_contraction_and_the_header():
    from disn_amd.csrc import build
    assert build.SOURCES["mesh_smooth.hip"] == ["-ffp-contract=off"]
    assert any(h.endswith(os.path.join("include", "disn_amd_smooth.h")) for h in build.HEADERS)
    text = open(os.path.join(ROOT, "disn_amd", "csrc", "mesh_batch.hpp")).read()
    assert "mesh_smooth.hip" in text.split("#pragma once")[0]

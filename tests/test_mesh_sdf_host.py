"""CPU tests of mesh-to-SDF preprocessing (disn_amd/mesh_sdf.py, disn_amd/preprocess.py, csrc/mesh_host.cpp): the
OBJ reader, the BVH image, normalisation, sample_sdf on CPU tensors, check_insideout, the flood rule of the
restatement and the C entries' argument checks.  No GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_sdf_reference as R  # noqa: E402

torch = pytest.importorskip("torch")


def _write(tmp_path, name, text, newline="\n"):
    p = tmp_path / name
    p.write_bytes(text.replace("\n", newline).encode())
    return str(p)


OBJ = """# a comment
mtllib x.mtl
o thing
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
vt 0 0
vn 0 0 1
g group
s off
usemtl m
f 1 2 3 4
f 1/1 2/1 3/1
f 1//1 3//1 4//1
f 1/1/1 2/1/1 3/1/1
v 0.5 0.5 1
f -1 -5 -4 -3 -2
"""


@pytest.mark.parametrize("newline", ["\n", "\r\n"])
def test_obj_reader_faces_tokens_polygons(tmp_path, newline):
    from disn_amd import mesh_sdf
    v, f = mesh_sdf.read_obj_mesh(_write(tmp_path, "m.obj", OBJ, newline))
    assert v.dtype == np.float32 and f.dtype == np.int32
    np.testing.assert_array_equal(v, [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1]])
    want = [[0, 1, 2], [0, 2, 3],            # quad, fan in file order
            [0, 1, 2], [0, 2, 3], [0, 1, 2],
            [4, 0, 1], [4, 1, 2], [4, 2, 3]]  # pentagon of negative indices: -1 = vertex 4 (the last read)
    np.testing.assert_array_equal(f, want)


def test_obj_reader_errors(tmp_path):
    from disn_amd import mesh_sdf
    for body in ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n",      # beyond the vertices
                 "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n",      # 0 is not an index
                 "v 0 0 0\nv 1 0 0\nv 0 1 0\nf -4 1 2\n",     # relative, before the first vertex
                 "v 0 0 0\nv 1 0 0\nf 1 2\n",                 # not a polygon
                 "v 0 0\n"):
        with pytest.raises(OSError):
            mesh_sdf.read_obj_mesh(_write(tmp_path, "bad.obj", body))
    with pytest.raises(OSError):
        mesh_sdf.read_obj_mesh(str(tmp_path / "missing.obj"))


def test_read_obj_is_unchanged(tmp_path):
    """isosurface.read_obj keeps its first-three-indices behaviour"""
    from disn_amd import isosurface
    v, f = isosurface.read_obj(_write(tmp_path, "m.obj", "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nf 1 2 3 4\n"))
    np.testing.assert_array_equal(f, [[0, 1, 2]])


def _soup(seed, n=700):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1, 1, (n * 3, 3)).astype(np.float32)
    f = np.arange(n * 3, dtype=np.int32).reshape(n, 3)
    f[n - 1] = f[n - 2]                      # a duplicated triangle
    v[1] = v[0]                              # a degenerate one
    return v, f


def test_bvh_invariants_and_reproducibility():
    from disn_amd import mesh_sdf
    for v, f in (_soup(0), _soup(1, 5), R.icosphere(2), R.box([-1, -1, -1], [1, 1, 1])):
        img = mesh_sdf.build_bvh_host(v, f)
        assert np.array_equal(img, mesh_sdf.build_bvh_host(v.copy(), f.copy()))
        b = R.parse_bvh(img, len(f))
        n = b["n_nodes"]
        assert b["n_tris"] == len(f) and 1 <= n <= 2 * len(f)
        # depth-first walk through the escape links: every node once, leaves cover every triangle slot once
        seen = np.zeros(len(f), int)
        for i in range(n):
            e, leaf = b["escape"][i], b["leaf"][i]
            assert i < e <= n
            if leaf:
                first, cnt = leaf >> 3, leaf & 7
                assert 1 <= cnt <= 4 and e == i + 1
                seen[first:first + cnt] += 1
                tri = b["tris"][first:first + cnt].reshape(-1, 3)
                assert np.all(tri >= b["lo"][i]) and np.all(tri <= b["hi"][i])
            else:
                left, right = i + 1, b["escape"][i + 1]
                assert right < e and b["escape"][right] == e
                for c in (left, right):
                    assert np.all(b["lo"][c] >= b["lo"][i]) and np.all(b["hi"][c] <= b["hi"][i])
        assert np.all(seen == 1)
        # the leaf-ordered triangles are a permutation of the input triangles
        want = np.sort(v[f].reshape(len(f), 9).view([("", np.float32)] * 9), axis=0)
        got = np.sort(b["tris"].reshape(len(f), 9).view([("", np.float32)] * 9), axis=0)
        assert np.array_equal(want, got)


def test_bvh_rejects_bad_indices():
    from disn_amd import mesh_sdf
    v, f = R.box([0, 0, 0], [1, 1, 1])
    f[3, 1] = 8
    with pytest.raises(ValueError):
        mesh_sdf.build_bvh_host(v, f)
    f[3, 1] = -1
    with pytest.raises(ValueError):
        mesh_sdf.build_bvh_host(v, f)


def test_normalisation_matches_restatement():
    from disn_amd import preprocess
    v, f = R.torus()
    v = (v * np.float32(3.0) + np.float32(0.5)).astype(np.float32)
    c, m = preprocess.normalize_params(v, f, np.random.default_rng(7))
    pts = R.sample_surface(v, f, 16384, np.random.default_rng(7))
    c_ref = pts.mean(0)
    m_ref = np.max(np.linalg.norm(pts - c_ref, axis=1))
    np.testing.assert_allclose(c, c_ref, rtol=0, atol=1e-12)
    assert abs(m - m_ref) <= 1e-12
    assert np.allclose(c, [0.5, 0.5, 0.5], atol=0.02)


def _field(res, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.2, 0.2, (res + 1) ** 3).astype(np.float32)


@pytest.mark.parametrize("num_sample,bw,seed", [(400, 0.1, 0), (4000, 0.1, 1), (4000, 0.02, 2)])
def test_sample_sdf_on_cpu_tensors_equals_restatement(num_sample, bw, seed):
    from disn_amd import preprocess
    res = 12
    vals = _field(res, seed)
    params = np.float32([-1, -0.5, -0.25, 1, 0.5, 0.75])
    got, _ = preprocess.sample_sdf("03001627", num_sample, bw, 0.003,
                                   {"param": params, "value": torch.from_numpy(vals)}, res,
                                   np.random.default_rng(seed))
    want, counts = R.sample_sdf(num_sample, bw, 0.003, params, vals, res, np.random.default_rng(seed))
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert len(got) == sum(counts)
    # rows are grid nodes and their values
    ax = [np.linspace(np.float64(params[a]), np.float64(params[a + 3]), res + 1).astype(np.float32) for a in range(3)]
    ix = [np.searchsorted(ax[a], got[:, a]) for a in range(3)]
    for a in range(3):
        assert np.array_equal(ax[a][ix[a]], got[:, a])
    flat = ix[0] + (res + 1) * (ix[1] + (res + 1) * ix[2])
    assert np.array_equal(vals[flat], got[:, 3])
    # bin bounds
    dis = got[:, 3] - np.float32(0.003)
    assert np.all(dis >= np.float32(-bw)) and np.all(dis < np.float32(bw))


def test_sample_sdf_carry_rule_and_starved_last_bin():
    from disn_amd import preprocess
    res = 8
    n = (res + 1) ** 3
    vals = np.full(n, 5.0, np.float32)                       # outside every bin
    vals[:10] = np.float32(-0.08) + 0.003                    # bin 0: 10 nodes
    vals[10:300] = np.float32(-0.01) + 0.003                 # bin 1: 290 nodes
    vals[300:305] = np.float32(0.01) + 0.003                 # bin 2: 5 nodes
    vals[305:307] = np.float32(0.05) + 0.003                 # bin 3: 2 nodes -- starved
    params = np.float32([-1, -1, -1, 1, 1, 1])
    got, _ = preprocess.sample_sdf("03001627", 400, 0.1, 0.003, {"param": params, "value": torch.from_numpy(vals)},
                                   res, np.random.default_rng(3))
    want, counts = R.sample_sdf(400, 0.1, 0.003, params, vals, res, np.random.default_rng(3))
    assert counts == [10, 190, 5, 2]       # bin 0 short by 90 -> bin 1 asks 190; bin 2 short -> bin 3 short, lost
    assert np.array_equal(got, want) and len(got) == 207


def test_check_insideout():
    from disn_amd import preprocess
    res = 4
    ax = np.linspace(-1, 1, res + 1).astype(np.float32)
    vals = np.full((res + 1) ** 3, -1.0, np.float32)
    centre = 2 + 2 * 5 + 2 * 25
    assert not preprocess.check_insideout("02958343", torch.from_numpy(vals), res, ax, ax, ax)
    vals[centre] = 0.5
    for cat in preprocess.INSIDEOUT_CATS:
        assert preprocess.check_insideout(cat, torch.from_numpy(vals), res, ax, ax, ax)
    assert not preprocess.check_insideout("03001627", torch.from_numpy(vals), res, ax, ax, ax)


def test_flood_rule_by_hand():
    n = 9
    u = np.full((n, n, n), 1.0, np.float32)
    bits = np.zeros((n, n, n), np.uint8)
    # a band block [2, 6]^3 in a far box: with no crossing everything floods within 3 steps
    u[2:7, 2:7, 2:7] = 0.05
    out = R.flood(u, bits, 0.1, 3)
    assert out.all()
    assert not R.flood(u, bits, 0.1, 2)[4, 4, 4]         # the centre is 3 steps deep
    b = np.zeros_like(bits)
    # cross every edge between the shell layer (index 2 or 6) and the next node inward
    b[2:7, 2:7, 2] |= 1          # x edges 2->3
    b[2:7, 2:7, 5] |= 1          # x edges 5->6
    b[2:7, 2, 2:7] |= 2
    b[2:7, 5, 2:7] |= 2
    b[2, 2:7, 2:7] |= 4
    b[5, 2:7, 2:7] |= 4
    out = R.flood(u, b, 0.1, 3)
    assert out[2, 2, 2] and out[0, 0, 0]
    assert not out[3:6, 3:6, 3:6].any()                  # the sealed inner block stays inside
    # depth limit: a band corridor longer than the step count is reached only `steps` deep
    u2 = np.full((3, 3, 12), 0.05, np.float32)
    u2[:, :, 0] = 1.0
    out = R.flood(u2, np.zeros(u2.shape, np.uint8), 0.1, 4)
    assert out[1, 1, 4] and not out[1, 1, 5]


def test_mesh_entries_validate_arguments_without_gpu(tmp_path):
    from disn_amd import _lib
    h = _lib.lib()
    assert h.disn_mesh_bvh_bytes(0) == 0 and h.disn_mesh_bvh_bytes(10) > 0
    assert h.disn_mesh_sign_workspace_bytes(1, 4, 4) == 0 and h.disn_mesh_sign_workspace_bytes(4, 4, 4) > 0
    assert h.disn_mesh_udf_points(None, 1, None, 1, 0, None, None) == -1
    one = C.c_void_p(1)
    assert h.disn_mesh_udf_points(one, 0, one, 1, 0, one, None) == -1
    assert h.disn_mesh_udf_grid(one, 1, one, one, one, 1, 4, 4, 0, one, None) == -1
    assert h.disn_mesh_sign(one, 1, one, one, one, 4, 4, 4, one, 0.0, 3, 0.0, one, None, one, 1 << 20, None) == -1
    assert h.disn_mesh_sign(one, 1, one, one, one, 4, 4, 4, one, 0.1, 3, 0.0, one, None, one, 16, None) == -3
    assert h.disn_mesh_sign(one, 1, one, one, one, 4, 4, 4, one, 0.1, -1, 0.0, one, None, one, 1 << 20, None) == -1
    counts = (C.c_int64 * 2)()
    assert h.disn_read_obj_mesh(b"/nonexistent/x.obj", None, 0, None, 0, counts) == -1
    assert h.disn_read_obj_mesh(b"/nonexistent/x.obj", None, 0, None, 0, None) == -1
    v = np.zeros((3, 3), np.float32)
    f = np.array([[0, 1, 3]], np.int32)
    buf = np.zeros(h.disn_mesh_bvh_bytes(1), np.uint8)
    assert h.disn_mesh_bvh_build(v.ctypes.data, 3, f.ctypes.data, 1, buf.ctypes.data, buf.size) == -1
    f[0, 2] = 2
    assert h.disn_mesh_bvh_build(v.ctypes.data, 3, f.ctypes.data, 1, buf.ctypes.data, buf.size - 1) == -3
    assert h.disn_mesh_bvh_build(v.ctypes.data, 3, f.ctypes.data, 1, buf.ctypes.data, buf.size) == 0


def test_seal_params_and_axes():
    from disn_amd import create_sdf, mesh_sdf
    params = np.float32([-0.6, -0.3, -0.1, 0.6, 0.3, 0.7])
    axes = mesh_sdf.grid_axes(params, 16)
    host = create_sdf.grid_points_host(params, 16)
    assert np.array_equal(R.grid_points(axes), host)
    tau, k = mesh_sdf.seal_params(axes, 1.0)
    h = [(float(a[-1]) - float(a[0])) / 16 for a in axes]
    assert tau == np.float32(max(h)) and k == 2 * int(np.ceil(tau / min(h))) + 1 == 5
    with pytest.raises(ValueError):
        mesh_sdf.seal_params(axes, 0.5)
    b = mesh_sdf.default_bbox(np.float32([[0, 0, 0], [1, 2, 4]]), 1.2)
    np.testing.assert_allclose(b, [-0.1, -0.2, -0.4, 1.1, 2.2, 4.4])


def test_preprocess_help_runs_without_a_gpu():
    r = subprocess.run([sys.executable, "-m", "disn_amd.preprocess", "--help"], cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "--category" in r.stdout and "--info" in r.stdout

"""Sphere tracing on the device (disn_amd/csrc/sdf_trace.hip, ``ops.trace_*``, ``render.trace_field``,
``SdfEngine.trace``).  Bars: the per-ray state, the lists (as sets), the points and the shaded outputs equal
the float32 reference (tests/sdf_trace_reference.py) bit for bit after setup and after every iteration; on the sphere
every hit lies where |f| <= eps puts it in float64; on the network every status-1 hit is a root of the fused query
within eps; a view does not depend on the views traced with it."""
import numpy as np
import pytest
import torch

import sdf_trace_reference as T
from oracle import disn_oracle as O

pytestmark = pytest.mark.gpu

BOX = [-1, -0.9, -0.8, 1, 0.9, 0.8]
EPS = 1e-4
ALL = ("rgba", "depth", "normal", "residual", "status")


def look_at(org, W, H, k):
    """a camera row at ``org`` looking at the origin: dir(x, y) = f + (x - W/2) k right + (y - H/2) k up"""
    org = np.asarray(org, np.float64)
    f = -org / np.linalg.norm(org)
    right = np.cross(f, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, f)
    return np.concatenate([org, f - 0.5 * W * k * right - 0.5 * H * k * up, k * right, k * up]).astype(np.float32)


def kernel_cams(W, H, synthetic_inside):
    from disn_amd import render
    demo = render.sdf_ray_cameras(O.DEMO_TRANS_MAT, W, H)[0]
    inside = demo.copy()
    inside[:3] *= np.float32(0.4)                                  # (0.81, 0.55, -0.52): inside the box, outside the shapes
    assert (np.abs(inside[:3]) < np.asarray(BOX[3:], np.float32)).all()
    # a direction with an exactly zero y component (a containment test, no 0 * inf), the origin inside / outside the
    # box's x-y extent
    synth = np.asarray([-0.05, 0.3 if synthetic_inside else 1.5, -2.0, 0, 0, 1, 0.01, 0, 0, 0, 0, 0], np.float32)
    return np.stack([demo, inside, synth])


FIELDS = {
    "sphere": (T.sphere, T.sphere_grad, 0.0),
    "steep": (lambda p: T.sphere(p, 2.5), lambda p: T.sphere_grad(p, 2.5), 0.0),
    "torus": (T.torus, T.torus_grad, 0.0),
    "far": (lambda p: T.sphere(p, 1.0, 4.0), T.sphere_grad, 0.0),
    "inside": (T.constant(-1.0), lambda p: np.zeros_like(p), 0.0),
    "iso": (T.constant(0.25), lambda p: np.zeros_like(p), 0.25),
}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _compare_state(view, ref, tag):
    for name in T.FLOAT_FIELDS + tuple(k for k in T.INT_FIELDS if k != "hit_slot"):
        got = view[name].cpu().numpy()
        assert np.array_equal(_bits(got), _bits(ref[name])), (tag, name, np.nonzero(_bits(got) != _bits(ref[name]))[0][:8])


@pytest.mark.parametrize("synthetic_inside", [True, False])
@pytest.mark.parametrize("name", list(FIELDS))
def test_kernels_equal_the_reference_bit_for_bit(name, synthetic_inside):
    from disn_amd import ops
    field, grad, iso = FIELDS[name]
    W, H = 13, 9
    cams = kernel_cams(W, H, synthetic_inside)
    n = cams.shape[0] * H * W
    assert n == 351                                                # 5.5 waves: a partial last one
    params = dict(T.DEFAULTS, iso=iso)
    cam_d = torch.from_numpy(cams).cuda()
    state = ops.trace_state(n, cam_d.device)
    view = ops.trace_state_view(state, n)
    pts = torch.empty((n, 3), dtype=torch.float32, device=cam_d.device)
    ops.trace_setup(cam_d, (W, H), BOX, state, pts)
    ref, ref_active = T.setup(cams, H, W, BOX)
    per_view = [int((ref_active // (H * W) == v).sum()) for v in range(3)]
    assert per_view[0] == 92 and per_view[1] == H * W and per_view[2] == (H * W if synthetic_inside else 0), per_view
    cur, it, evals = 0, 0, 0
    while True:
        tag = (name, "iteration", it)
        _compare_state(view, ref, tag)
        cnt = int(view["counts"][cur].item())
        lst = view["lists"][cur][:cnt].cpu().numpy().astype(np.int64)
        assert cnt == ref_active.size and np.array_equal(np.sort(lst), ref_active), tag
        p = pts[:cnt].cpu().numpy()
        assert np.array_equal(_bits(p), _bits(T.points(ref["org"], ref["dir"], ref["t"], lst))), tag
        if cnt == 0:
            break
        vals = field(p)                                            # float32 numpy, in the device's order
        ops.trace_advance(cam_d, (W, H), state, torch.from_numpy(vals).cuda(), cnt, cur, pts, **params)
        ref_active = np.sort(T.advance(ref, lst, vals, **params))
        cur, it, evals = 1 - cur, it + 1, evals + cnt
        assert it <= params["max_steps"] + params["refine"], "the loop does not end"
    ops.trace_collect(cam_d, (W, H), state, pts)
    ref_hits = T.collect(ref)
    nh = int(view["counts"][2].item())
    hits = view["lists"][2][:nh].cpu().numpy().astype(np.int64)
    assert nh == ref_hits.size and np.array_equal(np.sort(hits), ref_hits)
    slot = view["hit_slot"].cpu().numpy()
    assert np.array_equal(slot[hits], np.arange(nh)) and (np.delete(slot, hits) == -1).all()
    hp = pts[:nh].cpu().numpy()
    assert np.array_equal(_bits(hp), _bits(T.points(ref["org"], ref["dir"], ref["t"], hits)))
    pred_d = torch.from_numpy(field(hp)).cuda() if nh else None
    grad_d = torch.from_numpy(np.ascontiguousarray(grad(hp))).cuda() if nh else None
    out = ops.trace_shade(cam_d, (W, H), state, pred_d, grad_d, nh, iso=iso, want=ALL)
    rhp = T.points(ref["org"], ref["dir"], ref["t"], ref_hits)
    want = T.shade(ref, ref_hits, field(rhp), grad(rhp), iso=iso)
    for key in ALL:
        got = out[key].cpu().numpy().reshape(want[key].shape)
        assert np.array_equal(_bits(got), _bits(want[key])), (name, key)
    status = np.bincount(ref["status"], minlength=5)
    print("%s (synthetic camera %s): %d iterations, %d evaluations, %d hits, status %s"
          % (name, "inside" if synthetic_inside else "outside", it, evals, nh, status))
    box = sum(per_view)
    if name == "far":
        assert nh == 0 and status[1] == status[2] == status[3] == 0
    elif name == "inside":
        assert nh == box and status[2] == box and evals == box
    elif name == "iso":
        assert nh == box and status[1] == box and evals == box
        assert not out["normal"].any() and (out["rgba"].cpu().numpy().reshape(-1, 4)[hits, 0] == 61).all()   # 0.3 * 0.8 * 255
    else:
        assert 0 < nh < box and status[1] > 0


# ------------------------------------------------------------------ accuracy on the sphere, through trace_field
def _torch_sphere(p):
    q = p - torch.from_numpy(T.CENTRE).to(p.device)
    return torch.sqrt((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) - float(T.RADIUS)


def _torch_sphere_grad(p):
    q = p - torch.from_numpy(T.CENTRE).to(p.device)
    return q / torch.sqrt((q * q).sum(dim=1, keepdim=True))


@pytest.mark.parametrize("size", [(13, 9), (40, 40)])
def test_sphere_hits_lie_where_eps_puts_them(size):
    from disn_amd import render
    W, H = size
    cams = render.sdf_ray_cameras(O.DEMO_TRANS_MAT, W, H)
    calls = []

    def field(p):
        calls.append(p.shape[0])
        return _torch_sphere(p)

    out = render.trace_field(field, cams, size, BOX, grad=_torch_sphere_grad, want=ALL)
    stats = out["stats"]
    assert min(calls) > 0 and stats["rays"] == W * H
    org, d = T.rays(cams, H, W)
    r = float(T.RADIUS)
    b, s_in, _ = T.ray_sphere(org, d, r - EPS)
    _, s_out, _ = T.ray_sphere(org, d, r + EPS)
    depth = out["depth"].cpu().numpy().reshape(-1).astype(np.float64)
    hit = out["rgba"].cpu().numpy().reshape(-1, 4)[:, 3] == 255
    assert np.array_equal(hit, depth > 0)
    assert hit[b < r - EPS].all(), "a ray through the sphere did not hit"
    assert not hit[b > r + EPS].any(), "a ray past the sphere hit"
    s = depth * np.linalg.norm(d.astype(np.float64), axis=1)       # distance along the ray: dir is not unit length
    lo = s_out - 1e-6
    hi = np.where(b < r - EPS, s_in + 1e-6, np.inf)
    worst = float((s[hit] - s_out[hit]).max())
    print("%dx%d sphere: %s, status %s, widest depth slack of a hit %.3g"
          % (W, H, stats, np.bincount(out["status"].cpu().numpy().reshape(-1), minlength=5), worst))
    assert (s[hit] >= lo[hit]).all() and (s[hit] <= hi[hit]).all()
    status = out["status"].cpu().numpy().reshape(-1)
    assert (status[hit] == 1).all(), "a hit of the sphere did not converge"
    assert (out["residual"].cpu().numpy().reshape(-1) <= np.float32(EPS)).all()
    nl = out["normal"].cpu().numpy().reshape(-1, 3)
    assert np.abs(np.linalg.norm(nl[hit], axis=1) - 1).max() < 1e-6 and not nl[~hit].any()


# ------------------------------------------------------------------ the network
@pytest.fixture(scope="module")
def eng():
    from disn_amd.engine import SdfEngine
    from disn_amd.weights import WeightStore
    return SdfEngine(WeightStore.random_init(0, mode="he"))


@pytest.fixture(scope="module")
def view(eng):
    """one encoded image, the median of its coarse grid as the iso value, and its 24 x 24 trace: computed once"""
    enc = eng.encode(O.synth_inputs(3, 1, 8)["imgs"])
    iso = float(np.median(eng.query_grid(enc, 0, O.DEMO_TRANS_MAT, BOX, 16).cpu().numpy()))
    out = eng.trace(enc, 0, O.DEMO_TRANS_MAT, size=(24, 24), sdf_params=BOX, iso=iso, want=ALL)
    torch.cuda.synchronize()
    return enc, iso, out


def test_network_hits_are_roots_of_the_fused_query(eng, view):
    from disn_amd import render
    enc, iso, out = view
    W = H = 24
    stats = out["stats"]
    status = out["status"].cpu().numpy().reshape(-1)
    depth = out["depth"].cpu().numpy().reshape(-1)
    alpha = out["rgba"].cpu().numpy().reshape(-1, 4)[:, 3]
    print("network 24x24, iso %.6f: %s, status %s" % (iso, stats, np.bincount(status, minlength=5)))
    hit = (status >= 1) & (status <= 3)
    assert hit.any() and (~hit).any() and stats["hits"] == int(hit.sum())
    assert np.array_equal(depth > 0, alpha == 255) and np.array_equal(hit, alpha == 255)
    assert set(alpha.tolist()) <= {0, 255}
    one = np.nonzero(status == 1)[0]
    assert one.size > 0
    cams = render.sdf_ray_cameras(O.DEMO_TRANS_MAT, W, H)
    org, d = T.rays(cams, H, W)
    p = T.points(org, d, depth, one)                                # the point the kernel handed out, bit for bit
    pred = eng.query(enc, p[None], O.DEMO_TRANS_MAT, fold=True, fused=True).cpu().numpy().reshape(-1)
    f = np.abs(pred / np.float32(10.0) - np.float32(iso))
    res = out["residual"].cpu().numpy().reshape(-1)[one]
    print("status-1 hits: %d, max |pred/10 - iso| %.3g, max |residual - it| %.3g" % (one.size, f.max(), np.abs(res - f).max()))
    assert (f <= np.float32(EPS)).all()
    assert np.abs(res - f).max() <= 2e-6                           # REFINE_MIN_DECREASE = 2e-5 between query forms, / sdf_weight
    nl = np.linalg.norm(out["normal"].cpu().numpy().reshape(-1, 3), axis=1)
    assert np.abs(nl[hit] - 1).max() < 1e-5 and not nl[~hit].any()


def test_companions_do_not_matter(eng, view, monkeypatch):
    from disn_amd import ops, render
    enc, iso, alone = view
    c = render.sdf_ray_cameras(O.DEMO_TRANS_MAT, 24, 24)
    c2 = look_at([-1.6, 1.2, 1.4], 24, 24, 0.03)[None]
    counts = []
    real = ops.trace_advance

    def recording(cams, size, state, values, n_active, *a, **k):
        counts[-1].append(int(n_active))
        return real(cams, size, state, values, n_active, *a, **k)

    monkeypatch.setattr(ops, "trace_advance", recording)

    def run(cams):
        counts.append([])
        return eng.trace(enc, 0, O.DEMO_TRANS_MAT, cams=cams, size=(24, 24), sdf_params=BOX, iso=iso, want=ALL)

    first, other, pair, twice = run(c), run(c2), run(np.concatenate([c, c2])), run(np.concatenate([c, c]))
    n1, n2, n12, n11 = counts
    print("iterations: %d alone, %d the other view, %d together" % (len(n1), len(n2), len(n12)))
    for key in ALL:
        assert torch.equal(first[key], alone[key]), key           # ... and the same as the fixture's own-camera run
        assert torch.equal(pair[key][0], first[key][0]) and torch.equal(pair[key][1], other[key][0]), key
        assert torch.equal(twice[key][0], first[key][0]) and torch.equal(twice[key][1], first[key][0]), key
    # every iteration evaluated all views' rays in one call: the counts add up, so view 0's rays met another number of
    # companions in every iteration (for as long as the other view had rays left; next to itself: throughout)
    m = max(len(n1), len(n2))
    pad = lambda v: v + [0] * (m - len(v))
    assert n12 == [a + b for a, b in zip(pad(n1), pad(n2))]
    assert all(b > a for a, b in zip(n1[:len(n2)], n12)) and n11 == [2 * a for a in n1]
    assert other["stats"]["hits"] > 0


def test_misuse_and_degenerate_sizes(eng, view):
    from disn_amd import render
    from disn_amd.engine import SdfEngine
    enc, iso, _ = view
    plain = SdfEngine(None, weights=eng.weights, fused=False)
    with pytest.raises(ValueError, match="fused"):
        plain.trace(enc, 0, O.DEMO_TRANS_MAT, size=(8, 8), sdf_params=BOX, iso=iso)
    with pytest.raises(ValueError, match="want"):
        eng.trace(enc, 0, O.DEMO_TRANS_MAT, size=(8, 8), sdf_params=BOX, iso=iso, want=("face",))
    for size in ((1, 1), (1, 137)):
        out = eng.trace(enc, 0, O.DEMO_TRANS_MAT, size=size, sdf_params=BOX, iso=iso, want=ALL)
        assert out["rgba"].shape == (1, size[1], size[0], 4) and out["stats"]["rays"] == size[0] * size[1]
        cams = render.sdf_ray_cameras(O.DEMO_TRANS_MAT, *size)
        sph = render.trace_field(_torch_sphere, cams, size, BOX, want=("depth", "status"))
        ref = T.trace(T.sphere, cams, size[1], size[0], BOX)[2]
        assert sph["stats"]["box_rays"] == ref["box_rays"] and sph["stats"]["hits"] == ref["hits"]


"""Host side of the sphere tracer: the cameras of ``render.sdf_ray_cameras`` against the oracle's projection,
the float32 reference tracer (tests/sdf_trace_reference.py, what the kernels are compared with bit for bit) on analytic
fields, ``render.silhouette_iou`` and the demo's flags.  No GPU."""
import numpy as np
import pytest

import sdf_trace_reference as T
from oracle import disn_oracle as O

BOX = [-1, -0.9, -0.8, 1, 0.9, 0.8]
W, H = 13, 9


def test_cameras_round_trip_through_the_projection():
    from disn_amd import render
    cam = render.sdf_ray_cameras(O.DEMO_TRANS_MAT)
    assert cam.shape == (1, 12) and cam.dtype == np.float32
    assert np.allclose(cam[0, :3], [2.026, 1.384, -1.296], atol=2e-3)
    c = cam[0].astype(np.float64)
    org, d0, dx, dy = c[0:3], c[3:6], c[6:9], c[9:12]
    Tm = O.DEMO_TRANS_MAT[0].astype(np.float64)
    rng = np.random.default_rng(0)
    xy = np.concatenate([[[70.2, 33.7], [0.5, 0.5], [136.5, 136.5]], rng.uniform(1.0, 135.0, (20, 2))])
    t = np.concatenate([[1.3, 0.9, 2.0], rng.uniform(0.8, 2.2, 20)])
    d = d0 + xy[:, :1] * dx + xy[:, 1:] * dy
    p = org + t[:, None] * d
    proj = np.concatenate([p, np.ones((len(p), 1))], axis=1) @ Tm
    assert np.abs(proj[:, 2] - t).max() < 1e-5, "t is not the camera-space depth"
    inside = (xy.min(axis=1) >= 0) & (xy.max(axis=1) <= 136)       # the oracle clamps to the image
    got = O.get_img_points(p[None].astype(np.float32), O.DEMO_TRANS_MAT)[0]
    assert np.abs(got[inside] - xy[inside]).max() < 1e-4
    ln = np.linalg.norm(T.rays(cam, 137, 137)[1].astype(np.float64), axis=1)
    print("|dir| over the image: %.3f .. %.3f" % (ln.min(), ln.max()))
    assert 1.9 < ln.min() and ln.max() < 2.35                      # not unit length: a distance s is s / |dir| in t
    # another image size scales dx and dy alone: pixel (x, y) of W x H is pixel (x 137/W, y 137/H) of the 137 image
    small = render.sdf_ray_cameras(O.DEMO_TRANS_MAT, W=40, H=25).astype(np.float64)[0]
    assert np.array_equal(small[:6], c[:6])
    assert np.allclose(small[6:9], c[6:9] * 137 / 40, rtol=1e-6) and np.allclose(small[9:12], c[9:12] * 137 / 25, rtol=1e-6)
    two = render.sdf_ray_cameras(np.repeat(O.DEMO_TRANS_MAT, 2, axis=0))
    assert two.shape == (2, 12) and np.array_equal(two[0], two[1])


@pytest.fixture(scope="module")
def cam():
    from disn_amd import render
    return render.sdf_ray_cameras(O.DEMO_TRANS_MAT, W, H)


def _closed_form_masks(cam, eps=1e-4):
    org, d = T.rays(cam, H, W)
    b, _, _ = T.ray_sphere(org, d, T.RADIUS)
    return b < float(T.RADIUS) - eps, b > float(T.RADIUS) + eps


def test_reference_tracer_on_analytic_fields(cam):
    st, out, stats = T.trace(T.sphere, cam, H, W, BOX, grad=T.sphere_grad)
    print("sphere:", stats, "status", np.bincount(st["status"], minlength=5))
    assert stats["rays"] == 117 and stats["box_rays"] == 92
    hit = out["rgba"][:, 3] == 255
    must, must_not = _closed_form_masks(cam)
    assert (must | must_not).all(), "a ray of this image grazes the sphere within eps: the masks are not comparable"
    assert np.array_equal(hit, must)
    assert stats["hits"] == 9 and (st["status"][hit] == 1).all() and (st["status"][~hit] == 0).all()
    assert np.array_equal(out["depth"] > 0, hit)
    assert (np.abs(T.sphere(T.points(st["org"], st["dir"], st["t"], np.nonzero(hit)[0]))) <= np.float32(1e-4)).all()
    assert np.abs(np.linalg.norm(out["normal"][hit], axis=1) - 1).max() < 1e-6

    st, out, stats = T.trace(lambda p: T.sphere(p, 2.5), cam, H, W, BOX)
    print("2.5 x sphere:", stats, "status", np.bincount(st["status"], minlength=5))
    assert stats["hits"] == 9 and np.array_equal(out["rgba"][:, 3] == 255, must)
    # ... and without the cap on a step the steep field is stepped through
    st, out, stats = T.trace(lambda p: T.sphere(p, 2.5), cam, H, W, BOX, max_step=10.0)
    print("2.5 x sphere, no step cap:", stats)
    assert stats["hits"] < 9

    st, out, stats = T.trace(T.torus, cam, H, W, BOX)
    print("torus:", stats, "status", np.bincount(st["status"], minlength=5))
    assert stats["hits"] == 14

    st, out, stats = T.trace(lambda p: T.sphere(p, 1.0, 4.0), cam, H, W, BOX)
    assert stats["hits"] == 0 and set(st["status"].tolist()) <= {0, 4}
    st, out, stats = T.trace(T.constant(-1.0), cam, H, W, BOX)
    assert stats["hits"] == 92 and stats["evaluations"] == 92 and (st["status"][st["t1"] > 0] == 2).all()
    st, out, stats = T.trace(T.constant(0.25), cam, H, W, BOX, iso=0.25)
    assert stats["hits"] == 92 and (st["status"][st["t1"] > 0] == 1).all()


def test_reference_evaluation_count_at_the_image_size():
    """the issue's figure for a 137 x 137 view: 0.2 - 0.28 M evaluations, about one 65^3 grid"""
    from disn_amd import render
    c = render.sdf_ray_cameras(O.DEMO_TRANS_MAT, 48, 48)
    _, _, stats = T.trace(T.sphere, c, 48, 48, BOX)
    per_ray = stats["evaluations"] / stats["rays"]
    print("48 x 48 sphere:", stats, "evaluations per ray %.2f" % per_ray)
    assert per_ray * 137 * 137 < 0.3e6


def test_silhouette_iou():
    from disn_amd.render import silhouette_iou
    z = np.zeros((4, 5), np.uint8)
    assert silhouette_iou(z, z) == 1.0
    a = z.copy()
    a[1:3, 1:4] = 255
    assert silhouette_iou(a, a) == 1.0 and silhouette_iou(a, z) == 0.0 and silhouette_iou(z, a) == 0.0
    m = z.copy()
    m[1:3, 2:5] = 1                                      # 4 shared, 8 in the union
    assert silhouette_iou(m, a) == 0.5
    assert silhouette_iou(m.astype(bool), a.astype(np.float32) / 255) == 0.5
    with pytest.raises(ValueError):
        silhouette_iou(np.zeros((4, 4)), np.zeros((4, 5)))
    with pytest.raises(ValueError):
        silhouette_iou(np.zeros(4), np.zeros(4))


def test_demo_preview_flags():
    from disn_amd import demo
    a = demo.parser().parse_args(["--img", "x.png"])
    assert a.preview is None and a.preview_size == 137
    b = demo.parser().parse_args(["--img", "x.png", "--preview", "p.png", "--preview_size", "64"])
    assert b.preview == "p.png" and b.preview_size == 64
    rest = {k: v for k, v in vars(b).items() if k not in ("preview", "preview_size")}
    assert rest == {k: v for k, v in vars(a).items() if k not in ("preview", "preview_size")}


def test_read_alpha(tmp_path):
    from PIL import Image
    from disn_amd import demo
    rgba = np.zeros((5, 4, 4), np.uint8)
    rgba[1:3, :, 3] = 200
    Image.fromarray(rgba).save(tmp_path / "a.png")
    Image.fromarray(rgba[:, :, :3]).save(tmp_path / "b.png")
    assert np.array_equal(demo.read_alpha(str(tmp_path / "a.png")), rgba[:, :, 3])
    assert demo.read_alpha(str(tmp_path / "b.png")) is None


def test_write_preview_with_a_stub_engine(tmp_path, capsys):
    """the demo's preview step around an engine that returns a fixed view: the PNG, the statistics, the IoU against the
    input's alpha sampled at the rays' pixels"""
    import torch
    from PIL import Image
    from disn_amd import demo, render
    rgba = np.zeros((1, 24, 24, 4), np.uint8)
    rgba[0, 4:20, 6:18] = (150, 150, 150, 255)
    stats = {"rays": 576, "box_rays": 500, "evaluations": 9000, "iterations": 40, "hits": 192}
    seen = {}

    class Engine:
        def encode(self, img):
            return "enc"

        def trace(self, enc, image_index, trans_mat, **kw):
            seen.update(kw, enc=enc, image_index=image_index)
            return {"rgba": torch.from_numpy(rgba), "stats": stats}

    alpha = np.zeros((137, 137), np.uint8)
    alpha[30:110, 40:100] = 200
    path = str(tmp_path / "p.png")
    res = demo.write_preview(Engine(), np.zeros((1, 137, 137, 3), np.float32), O.DEMO_TRANS_MAT, path, 24, 0.25, alpha)
    assert seen["enc"] == "enc" and seen["image_index"] == 0 and seen["size"] == (24, 24) and seen["iso"] == 0.25
    assert np.array_equal(np.asarray(Image.open(path)), rgba[0])
    idx = ((np.arange(24) + 0.5) * 137 / 24).astype(np.int64)
    assert res == {"stats": stats, "iou": render.silhouette_iou(rgba[0, :, :, 3], alpha[idx][:, idx])}
    assert 0.0 < res["iou"] < 1.0
    text = capsys.readouterr().out
    assert "silhouette IoU" in text and "'evaluations': 9000" in text
    assert demo.write_preview(Engine(), None, O.DEMO_TRANS_MAT, path, 24, 0.0)["iou"] is None
    with pytest.raises(ValueError):
        demo.write_preview(Engine(), None, O.DEMO_TRANS_MAT, path, 0, 0.0)

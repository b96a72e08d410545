"""CPU checks of the SDF-gradient feature: the numpy reference of tests/sdf_grad_reference.py against the
oracle and against central differences, the .obj writer with normals through the three readers, the new flags."""
import numpy as np
import pytest

import sdf_grad_reference as R
from oracle import disn_oracle as O


@pytest.fixture(scope="module")
def case():
    """He weights of seed 2, synth_inputs(seed=3, n_points=2048): the float64 reference, computed once"""
    w = O.init_weights(2, mode="he")
    feed = O.synth_inputs(seed=3, n_points=2048)
    enc = R.encode(feed["imgs"], w, np.float64)
    ref = R.reference(w, feed["imgs"], feed["sample_pc"], feed["trans_mat"], np.float64, enc)
    return {"w": w, "feed": feed, "enc": enc, "ref": ref}


def test_reference_value_is_the_oracles(case):
    w, feed = case["w"], case["feed"]
    want = np.asarray(O.get_model(feed, w, dtype=np.float64)["pred_sdf"], np.float64)[..., 0]
    got = R.reference(w, feed["imgs"], feed["sample_pc"], feed["trans_mat"], np.float64, case["enc"],
                      oracle_gather=True)
    err = np.abs(got["value"] - want).max()
    print("\n[sdf_grad] reference value vs oracle.get_model(float64): max |d| %.3g" % err)
    assert err <= 1e-9
    # the tangents do not depend on where the value's local term came from
    assert np.array_equal(got["grad"], case["ref"]["grad"])
    # the all-float64 value differs from the oracle's by the oracle's float32 projection and gather only
    assert np.abs(case["ref"]["value"] - want).max() <= 1e-4


def test_inclusion_rates(case):
    ref = case["ref"]
    inc = R.included(ref)
    print("\n[sdf_grad] included %.1f %%: clamped %.1f %%, near a cell line %.1f %%, margin < %g %.1f %%; clamped and "
          "comparable: %d points" % (100 * inc.mean(), 100 * ref["clamped"].mean(), 100 * ref["near_line"].mean(),
                                     R.MARGIN, 100 * (ref["margin"] < R.MARGIN).mean(),
                                     int(R.clamped_comparable(ref).sum())))
    assert inc.mean() >= 0.75
    assert R.clamped_comparable(ref).sum() >= 50


def test_reference_gradient_is_the_central_difference(case):
    """h = 1e-6 in float64.  Between the kinks pred is a smooth function of p (rational projection, bilinear patch,
    linear layers): the central difference errs by eps64 |f| cond / h ~ 1e-16 * 1e2 / 1e-6 = 1e-8 of rounding plus
    h^2 f''' / 6 ~ 1e-12 f''' of truncation -- 1e-6 bounds both with room.  A point whose ReLU pattern changes within
    +-h is not differentiable there and is left out (the margin of 3e-5 leaves next to none)."""
    w, feed, ref = case["w"], case["feed"], case["ref"]
    h = 1e-6
    pts = feed["sample_pc"].astype(np.float64)
    cd = np.zeros_like(ref["grad"])
    same = np.ones(ref["margin"].shape, bool)
    for k in range(3):
        d = np.zeros(3)
        d[k] = h
        hi = R.reference(w, feed["imgs"], pts + d, feed["trans_mat"], np.float64, case["enc"])
        lo = R.reference(w, feed["imgs"], pts - d, feed["trans_mat"], np.float64, case["enc"])
        cd[..., k] = (hi["value"] - lo["value"]) / (2 * h)
        same &= (hi["signs"] == ref["signs"]).all(-1) & (lo["signs"] == ref["signs"]).all(-1)
    inc = R.included(ref)
    sel = inc & same
    err = np.abs(cd - ref["grad"])[sel].max()
    print("\n[sdf_grad] central differences: %d of %d included points keep their ReLU pattern, max |d| %.3g, "
          "|grad| median %.3g" % (sel.sum(), inc.sum(), err, np.median(np.linalg.norm(ref["grad"], axis=-1))))
    assert sel.sum() >= 0.99 * inc.sum()
    assert err <= 1e-6
    # clamped points: the projection's tangents of the clamped coordinate are zero, and so is the central difference's
    cl = R.clamped_comparable(ref) & same
    assert cl.sum() >= 50
    assert np.abs(cd - ref["grad"])[cl].max() <= 1e-6


def test_write_obj_with_normals_round_trips(tmp_path):
    from disn_amd import isosurface, mesh_sdf
    rng = np.random.default_rng(5)
    verts = rng.standard_normal((7, 3)).astype(np.float32)
    normals = rng.standard_normal((7, 3)).astype(np.float32)
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    normals[3] = 0                                                              # a degenerate vertex's normal
    faces = np.asarray([[0, 1, 2], [2, 3, 4], [4, 5, 6], [6, 0, 3]], np.int32)
    plain, withn = str(tmp_path / "plain.obj"), str(tmp_path / "normals.obj")
    isosurface.write_obj(plain, verts, faces)
    isosurface.write_obj(withn, verts, faces, normals)
    want = "".join("v %.9g %.9g %.9g\n" % tuple(v) for v in verts) + "".join("f %d %d %d\n" % tuple(f + 1) for f in faces)
    assert open(plain).read() == want                                           # the plain file is what it always was
    lines = open(withn).read().splitlines()
    assert lines[:7] == want.splitlines()[:7]
    vn = np.asarray([[float(t) for t in l.split()[1:]] for l in lines if l.startswith("vn ")], np.float32)
    assert np.array_equal(vn, normals)                                          # 9 digits: float32 round-trips
    assert lines[14:] == ["f %d//%d %d//%d %d//%d" % (a, a, b, b, c, c) for a, b, c in faces + 1]
    for path in (plain, withn):
        v, f = isosurface.read_obj(path)
        assert np.array_equal(v, verts) and np.array_equal(f, faces)
        assert np.array_equal(isosurface.read_obj_verts(path), verts)
        v, f = mesh_sdf.read_obj_mesh(path)
        assert np.array_equal(v, verts) and np.array_equal(f, faces)
    with pytest.raises(ValueError):
        isosurface.write_obj(withn, verts, faces, normals[:5])


def test_refine_flags_parse_and_default_to_off():
    from disn_amd import create_sdf, demo
    a = create_sdf.parser().parse_args(["--test_lst_dir", "x"])
    assert a.refine == 0 and a.normals is False
    a = create_sdf.parser().parse_args(["--test_lst_dir", "x", "--refine", "2", "--normals"])
    assert a.refine == 2 and a.normals is True
    create_sdf.check_flags(a)
    a.refine = -1
    with pytest.raises(ValueError):
        create_sdf.check_flags(a)
    d = demo.parser().parse_args(["--img", "v.png"])
    assert d.refine == 0 and d.normals is False
    d = demo.parser().parse_args(["--img", "v.png", "--refine", "3", "--normals"])
    assert d.refine == 3 and d.normals is True

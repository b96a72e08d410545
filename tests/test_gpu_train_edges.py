"""The training backward kernels at ragged, odd and tiny shapes (tables: train_edge_shapes.py; what each shape reaches:
its comments, checked on the CPU by test_train_edges_host.py).

Every reference is torch-CPU float64 autograd or numpy float64 of the same operation; every case runs inside
guarded("A") (guarded_alloc.py), so an overrun at a tail shape damages a guard band the test owns and fails g.check()
instead of faulting.  Tolerances are those of test_gpu_train.py / test_gpu_bf16.py for the same kernel and mode.
Each comparison prints an ``EDGE`` line (error and bound relative to max |ref|) before it asserts."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as Fnn

import train_edge_shapes as S
from conftest import report_close
from guarded_alloc import guarded
from oracle import disn_oracle as O
from oracle import train_oracle as T
from train_edge_shapes import bf16_round, host, step_feed

pytestmark = pytest.mark.gpu

_CACHE = {}


def cached(key, make):
    """host-side inputs and float64 references, shared between the modes of a shape: computed once, never modified
    (the three most recent only: a large dense case holds ~0.5 GB)"""
    if key not in _CACHE:
        while len(_CACHE) >= 3:
            _CACHE.pop(next(iter(_CACHE)))
        _CACHE[key] = make()
    return _CACHE[key]


@pytest.fixture(scope="module")
def ops():
    from disn_amd import ops as _ops
    return _ops


def close(name, got, ref, rtol_of_max):
    """|got - ref| <= rtol_of_max * max |ref|; prints the measured figure first"""
    got, ref = np.asarray(got), np.asarray(ref, np.float64)
    scale = max(float(np.abs(ref).max()), 1e-30)
    err = float(np.abs(got.astype(np.float64) - ref).max()) if got.shape == ref.shape else float("nan")
    print("EDGE %s: err %.3g of max|ref|, bound %.3g, ratio %.3f" % (name, err / scale, rtol_of_max,
                                                                     err / scale / rtol_of_max))
    report_close(name, got, ref, atol=rtol_of_max * scale)


def shape_id(s):
    return "x".join(str(v) for v in s)


def f64(a, grad=False):
    return torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=grad)


# ------------------------------------------------------------------ 3x3 conv -------------------
def _conv2d(x, w, b=None):
    return Fnn.conv2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), b, padding=1).permute(0, 2, 3, 1)


def _conv_weight_grad(x, dz, w_shape):
    """float64 dW of sum(conv(x, w) * dz): linear in x and dz"""
    wt = torch.zeros(w_shape, dtype=torch.float64, requires_grad=True)
    (_conv2d(f64(x), wt) * f64(dz)).sum().backward()
    return wt.grad.numpy()


def _conv_case(shape):
    B, H, W, Cin, Cout = shape
    rng = np.random.default_rng(B * 100003 + H * 1009 + W * 101 + Cin + Cout)
    x = rng.standard_normal((B, H, W, Cin)).astype(np.float32)
    w = (rng.standard_normal((3, 3, Cin, Cout)) / math.sqrt(9 * Cin)).astype(np.float32)
    b = (0.1 * rng.standard_normal(Cout)).astype(np.float32)
    # every sample its own gradient scale, as in test_conv3x3_data_gradient_through_conv_h2
    dy = (rng.standard_normal((B, H, W, Cout)) * rng.uniform(0.01, 10.0, (B, 1, 1, 1))).astype(np.float32)
    xt, wt, bt = f64(x, True), f64(w, True), f64(b, True)
    z = _conv2d(xt, wt, bt)
    case = dict(x=x, w=w, dy=dy)
    for relu in (True, False):
        y = torch.relu(z) if relu else z
        gx, gw, gb = torch.autograd.grad((y * f64(dy)).sum(), (xt, wt, bt), retain_graph=True)
        if relu:   # the mask comes from the SAME activations the gradient is checked against
            pos = y.detach().numpy() > 0
            y32 = np.where(pos, np.maximum(y.detach().numpy().astype(np.float32), 1e-30), 0.0).astype(np.float32)
            dz = np.where(pos, dy, 0).astype(np.float32)
        else:
            y32, dz = None, dy
        case[relu] = dict(y=y32, dx=gx.numpy(), dw=gw.numpy(), db=gb.numpy(),
                          dw_bf16=_conv_weight_grad(bf16_round(x), bf16_round(dz), w.shape))
    return case


def _run_conv(ops, c, y, dy, mode, wd=S.CONV_WD):
    need_dx = c["x"].shape[-1] != 3
    with guarded("A") as g:
        dx, dw, db = ops.conv3x3_backward(g.put(c["x"]), g.put(c["w"]), g.put(y) if y is not None else None,
                                          g.put(dy, freeze=False), wd=wd, need_dx=need_dx, compute_bf16=mode)
        g.check()
        return (host(dx) if need_dx else None), host(dw), host(db)


@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("shape", S.CONV_SHAPES + S.CONV_C3_SHAPES, ids=shape_id)
def test_conv3x3_backward_edges(ops, shape, mode):
    """dx (per sample), dw, db against float64 autograd, with the ReLU mask and without.  Modes 0 and 2: 2e-6 of
    max |ref|; mode 1: dx the same (it runs through conv_h2.hip on the unrounded operands), dw against float64 on the
    bf16-rounded operands, 2e-6 where the bf16 form runs (9 Cin and Cout multiples of 128), else 2e-2."""
    B, H, W, Cin, Cout = shape
    c = cached(("conv", shape), lambda: _conv_case(shape))
    for relu in (True, False):
        r = c[relu]
        tag = "conv%s m%d %s" % (shape, mode, "relu" if relu else "lin")
        dx, dw, db = _run_conv(ops, c, r["y"], c["dy"], mode)
        wdw = S.CONV_WD * c["w"].astype(np.float64)
        if Cin != 3:
            if mode == 1:
                close(tag + " dx", dx, r["dx"], 2e-6)
            else:
                for s in range(B):
                    close(tag + " dx[%d]" % s, dx[s], r["dx"][s], 2e-6)
        if mode == 1:
            tol = 2e-6 if ((9 * Cin) % 128 == 0 and Cout % 128 == 0) else 2e-2
            close(tag + " dw(bf16 operands)", dw, r["dw_bf16"] + wdw, tol)
        else:
            close(tag + " dw", dw, r["dw"] + wdw, 2e-6)
        close(tag + " db", db, r["db"], 2e-6)   # one fp32 column sum in every mode


@pytest.mark.parametrize("mode", S.MODES)
def test_conv3x3_backward_zero_gradient(ops, mode):
    """dy all zero: dx and db exactly zero, dw the weight-decay term alone, to one fp32 rounding"""
    c = cached(("conv", S.CONV_ZERO_SHAPE), lambda: _conv_case(S.CONV_ZERO_SHAPE))
    dx, dw, db = _run_conv(ops, c, c[True]["y"], np.zeros_like(c["dy"]), mode)
    assert np.isfinite(dx).all() and np.isfinite(dw).all() and np.isfinite(db).all()
    assert not dx.any() and not db.any()
    ref = np.float64(np.float32(S.CONV_WD)) * c["w"].astype(np.float64)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    err = np.abs(dw.astype(np.float64) - ref)
    print("EDGE conv zero dy m%d: max |dw - wd w| / ulp = %.3f" % (mode, float((err / ulp).max())))
    assert (err <= ulp).all()


@pytest.mark.parametrize("mode", S.MODES)
def test_conv3x3_backward_sample_independence(ops, mode):
    """sample 1's dy zero: its dx is exactly zero and the other samples' dx keep their bits (per-sample operand scales
    of the data gradient), at a shape that is no VGG layer's"""
    c = cached(("conv", S.CONV_ZERO_SHAPE), lambda: _conv_case(S.CONV_ZERO_SHAPE))
    full, _, _ = _run_conv(ops, c, None, c["dy"], mode)
    dy0 = c["dy"].copy()
    dy0[1] = 0
    part, dw, db = _run_conv(ops, c, None, dy0, mode)
    assert not part[1].any()
    assert np.array_equal(part[0], full[0]) and np.array_equal(part[2], full[2])
    assert np.isfinite(dw).all() and np.isfinite(db).all()


# ------------------------------------------------------------------ dense layer ----------------
def _dense_case(shape):
    M, K, N = shape
    rng = np.random.default_rng(M * 7919 + K + N)
    a = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((K, N)) / math.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    dy = rng.standard_normal((M, N)).astype(np.float32)
    a64, w64 = a.astype(np.float64), w.astype(np.float64)
    z = a64 @ w64 + b
    abf, wbf = bf16_round(a), bf16_round(w)
    case = dict(a=a, w=w, dy=dy)
    for relu in (True, False):
        if relu:
            y32 = np.where(z > 0, np.maximum(z.astype(np.float32), 1e-30), 0.0).astype(np.float32)
            dz = np.where(z > 0, dy, 0).astype(np.float32)
        else:
            y32, dz = None, dy
        dz64, dzbf = dz.astype(np.float64), bf16_round(dz)
        case[relu] = dict(y=y32, da=dz64 @ w64.T, dw=a64.T @ dz64, db=dz64.sum(0),
                          da_bf16=dzbf @ wbf.T, dw_bf16=abf.T @ dzbf)
    return case


@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("shape", S.DENSE_SHAPES, ids=shape_id)
def test_dense_backward_edges(ops, shape, mode):
    """modes 0 and 2 as test_dense_backward (2e-6 of max |ref|, float64 on the unrounded operands); mode 1 as
    test_dense_backward_bf16 (float64 on the bf16-rounded operands; dw 2e-6 with the 128 x 128 tile, else 2e-2)"""
    M, K, N = shape
    c = cached(("dense", shape), lambda: _dense_case(shape))
    wdw = S.DENSE_WD * c["w"].astype(np.float64)
    for relu in (True, False):
        r = c[relu]
        tag = "dense%s m%d %s" % (shape, mode, "relu" if relu else "lin")
        with guarded("A") as g:
            da, dw, db = ops.dense_backward(g.put(c["a"]), g.put(c["w"]), g.put(r["y"]) if relu else None,
                                            g.put(c["dy"], freeze=False), wd=S.DENSE_WD, compute_bf16=mode)
            g.check()
            da, dw, db = host(da), host(dw), host(db)
        if mode == 1:
            close(tag + " da(bf16 operands)", da, r["da_bf16"], 2e-6)
            close(tag + " dw(bf16 operands)", dw, r["dw_bf16"] + wdw, 2e-6 if (K % 128 == 0 and N % 128 == 0) else 2e-2)
        else:
            close(tag + " da", da, r["da"], 2e-6)
            close(tag + " dw", dw, r["dw"] + wdw, 2e-6)
        close(tag + " db", db, r["db"], 2e-6)


# ------------------------------------------------------------------ pool -----------------------
def _pool_ref(x, dy):
    xt = f64(x, True)
    p = Fnn.max_pool2d(xt.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    (p * f64(dy)).sum().backward()
    return xt.grad.numpy().astype(np.float32)


def _run_pool(ops, x, dy):
    with guarded("A") as g:
        got = host(ops.maxpool2x2_backward(g.put(x), g.put(dy)))
        g.check()
    return got


@pytest.mark.parametrize("shape", S.POOL_SHAPES, ids=shape_id)
def test_maxpool_backward_routes_ties_to_the_first_maximum(ops, shape):
    """integer-valued input: positive ties in at least a quarter of the windows; the gradient goes to the first maximum
    in scan order, as torch's CPU max_pool2d backward routes it: every element equal"""
    B, H, W, C = shape
    rng = np.random.default_rng(H * 100 + W)
    x = rng.integers(0, 3, (B, H, W, C)).astype(np.float32)
    win = x.reshape(B, H // 2, 2, W // 2, 2, C)                   # a view: writes go to x
    force = rng.random((B, H // 2, W // 2, C)) < 0.5              # tie of scan positions 1 and 2, position 0 below
    force.reshape(-1)[0] = True
    win[:, :, 0, :, 0, :] = np.where(force, rng.integers(0, 2, force.shape), win[:, :, 0, :, 0, :])
    win[:, :, 0, :, 1, :] = np.where(force, 2, win[:, :, 0, :, 1, :])
    win[:, :, 1, :, 0, :] = np.where(force, 2, win[:, :, 1, :, 0, :])
    top = win.max(axis=(2, 4), keepdims=True)
    tied = ((win == top).sum(axis=(2, 4)) >= 2) & (top[:, :, 0, :, 0, :] > 0)
    assert tied.mean() >= 0.25, tied.mean()
    dy = rng.standard_normal((B, H // 2, W // 2, C)).astype(np.float32)
    got = _run_pool(ops, x, dy)
    assert np.array_equal(got, _pool_ref(x, dy))
    assert np.array_equal(got.reshape(B, H // 2, 2, W // 2, 2, C).sum((2, 4)), dy)


def test_maxpool_backward_with_negative_inputs(ops):
    """continuous input of both signs: a window of negatives routes to its true maximum"""
    B, H, W, C = S.POOL_CONTINUOUS_SHAPE
    rng = np.random.default_rng(17)
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    x[0, :2, :2] = -np.abs(x[0, :2, :2]) - 0.5
    assert (x.reshape(B, H // 2, 2, W // 2, 2, C).max(axis=(2, 4)) < 0).any()
    dy = rng.standard_normal((B, H // 2, W // 2, C)).astype(np.float32)
    assert np.array_equal(_run_pool(ops, x, dy), _pool_ref(x, dy))


# ------------------------------------------------------------------ resize ---------------------
@pytest.mark.parametrize("case", S.RESIZE_SHAPES, ids=shape_id)
def test_resize_backward_edges(ops, case):
    B, Hin, Win, C, cs, coff, Hout, Wout = case
    rng = np.random.default_rng(Hin * 1000 + Win + Hout)
    dout = rng.standard_normal((B, Hout, Wout, cs)).astype(np.float32)
    xt = torch.zeros((B, Hin, Win, C), dtype=torch.float64, requires_grad=True)
    (T._resize_legacy(xt, Hout, Wout) * f64(dout[..., coff:coff + C])).sum().backward()
    ref = xt.grad.numpy()
    base = rng.standard_normal((B, Hin, Win, C)).astype(np.float32)
    with guarded("A") as g:
        doutd = g.put(dout)
        got = host(ops.resize_bilinear_backward(doutd, Hin, Win, channels=C, out_coff=coff))
        acc = g.put(base, freeze=False)
        ops.resize_bilinear_backward(doutd, Hin, Win, channels=C, out_coff=coff, din=acc, accumulate=True)
        g.check()
        acc = host(acc)
    close("resize%s din" % (case,), got, ref, 1e-6)
    close("resize%s din+=" % (case,), acc, ref + base, 1e-6)
    if (Hin, Win) == (Hout, Wout):
        assert np.array_equal(got, dout[..., coff:coff + C])


# ------------------------------------------------------------------ gather ---------------------
_HAND_PLACED = [[0, 0], [136, 0], [0, 136], [136, 136], [136, 5], [5, 136], [-1, 5], [5, -1], [137, 5], [5, 137],
                [-0.5, 7], [7, -0.5], [136.5, 3], [3, 136.5], [-0.5, -0.5], [136.5, 136.5], [-0.5, 136.5], [20, 20]]


def _gather_points(B, N, rng):
    xy = rng.uniform(-2.0, 139.0, (B, N, 2)).astype(np.float32)
    if (B, N) == (1, 1):
        xy[0, 0] = [136.5, 3.25]
    elif (B, N) == (1, 64):
        xy[0] = [20, 31]                                    # 64 points on one pixel: the atomics must accumulate
    else:
        xy[0, :len(_HAND_PLACED)] = _HAND_PLACED
        out = rng.uniform(137.0, 140.0, (N, 2)).astype(np.float32)      # sample 1: every point outside the image
        out[::3, 0] = -1.0
        out[1::3, 1] = rng.uniform(-3.0, -1.0, len(out[1::3]))
        out[2::3, 0] = 137.0
        out[2::3, 1] = rng.uniform(0.0, 136.0, len(out[2::3]))
        xy[1] = out
        xy[2, :64] = [20.25, 31.5]
    return xy


@pytest.mark.parametrize("B,N", S.GATHER_SHAPES)
def test_gather_backward_edges(ops, B, N):
    rng = np.random.default_rng(B * 1000 + N)
    xy = _gather_points(B, N, rng)
    dfeat = rng.standard_normal((B, N, 1472)).astype(np.float32)
    refs = []
    for b in range(B):                                      # per sample: a float64 map is 221 MB
        mt = torch.zeros((1, 137, 137, 1472), dtype=torch.float64, requires_grad=True)
        (T._resampler(mt, xy[b:b + 1]) * f64(dfeat[b:b + 1])).sum().backward()
        refs.append(mt.grad.numpy()[0])
    with guarded("A") as g:
        got = host(ops.gather_backward(g.put(dfeat), g.put(xy)))
        g.check()
    scale = max(float(np.abs(r).max()) for r in refs)
    for b in range(B):
        err = float(np.abs(got[b] - refs[b]).max())
        print("EDGE gather(%d,%d)[%d]: err %.3g of max|ref|, bound 1e-06" % (B, N, b, err / scale))
        report_close("dfeatmap[%d]" % b, got[b], refs[b], atol=1e-6 * scale)
    if B == 3:
        assert not refs[1].any() and not got[1].any()       # nothing of the outside sample reaches the map


# ------------------------------------------------------------------ Adam -----------------------
@pytest.mark.parametrize("grad_scale", S.ADAM_GRAD_SCALES)
@pytest.mark.parametrize("n", S.ADAM_SIZES)
def test_adam_update_edges(ops, n, grad_scale):
    """sizes around the 1024-float block and past 2^22, with the two degenerate states mixed in: g = 0 with v = 0 (the
    step is -lr_t m / eps) and v = 0 with a gradient far above sqrt(v) (the largest step Adam takes).
    The absolute tolerances of test_adam_update (1e-7 on m and v) resolve one fp32 rounding only below |m| = 2
    (ulp(2) / 2 = 1.2e-7), so the gradients are clipped to |g| <= 3; and the reference (numpy float64 of the same update)
    takes beta1, beta2, eps, lr_t and grad_scale as the float32 values the C ABI carries: 1 - float32(0.999) differs from
    0.001 by 1.3e-5 of itself, 2e-7 in v at g^2 = 16."""
    rng = np.random.default_rng(n)
    w = rng.standard_normal(n).astype(np.float32)
    m = (0.1 * rng.standard_normal(n)).astype(np.float32)
    v = (0.01 * rng.random(n)).astype(np.float32)
    grad = np.clip(rng.standard_normal(n), -3.0, 3.0).astype(np.float32)
    kind = rng.choice(4, n, p=[0.4, 0.1, 0.1, 0.4])
    kind[:4] = [0, 1, 2, 3]
    grad[kind == 1] = 0
    v[(kind == 1) | (kind == 2)] = 0
    m[kind == 1] *= np.float32(1e-3)       # the step there is lr_t m / eps = 420 m: kept below |w|, whose tolerance is relative
    big = kind == 2
    m[big] = 0
    grad[big] = (rng.uniform(0.25, 1.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)[big]
    t, lr = 7, 1e-4
    lr_t = lr * math.sqrt(1 - 0.999 ** t) / (1 - 0.5 ** t)
    b1, b2, eps, lr32, gs = (float(np.float32(c)) for c in (0.5, 0.999, 1e-8, lr_t, grad_scale))
    gg = gs * grad.astype(np.float64)
    m2 = b1 * m.astype(np.float64) + (1.0 - b1) * gg
    v2 = b2 * v.astype(np.float64) + (1.0 - b2) * gg * gg
    w2 = w.astype(np.float64) - lr32 * m2 / (np.sqrt(v2) + eps)
    assert np.abs(m2).max() < 2.0
    with guarded("A") as g:
        dw, dm, dv = g.put(w, freeze=False), g.put(m, freeze=False), g.put(v, freeze=False)
        ops.adam_update(dw, g.put(grad), dm, dv, lr_t, grad_scale=grad_scale)
        g.check()
        gw, gm, gv = host(dw), host(dm), host(dv)
    assert np.isfinite(gw).all() and np.isfinite(gm).all() and np.isfinite(gv).all()
    report_close("m", gm, m2, atol=1e-7)
    report_close("v", gv, v2, atol=1e-7)
    report_close("w", gw, w2, atol=1e-7, rtol=1e-6)
    assert np.array_equal(gm[kind == 1], (np.float32(0.5) * m[kind == 1])) and not gv[kind == 1].any()


def test_adam_update_large_gradient(ops):
    """v = 0 and m ~ 0.1 under gradients of 1e2 .. 1e4, beyond what the absolute 1e-7 of test_adam_update can resolve
    (m reaches 5e3, v 1e5).  Tolerance from the arithmetic: with beta1 = 0.5 both products of m are exact and the sum
    rounds once; v = c2 (g g) + beta2 0 rounds twice, three times if not contracted; allowed: four half-ulps,
    2.4e-7 of each value.  w moves by lr_t m / (sqrt(v) + eps) ~ 16 lr_t = 1.3e-4, every rounding of which is far below
    the last bit of w: the bound of test_adam_update holds as it is.  Reference as in test_adam_update_edges."""
    n = 1028
    rng = np.random.default_rng(77)
    w = rng.standard_normal(n).astype(np.float32)
    m = (0.1 * rng.standard_normal(n)).astype(np.float32)
    v = np.zeros(n, np.float32)
    grad = (10.0 ** rng.uniform(2.0, 4.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    t, lr = 7, 1e-4
    lr_t = lr * math.sqrt(1 - 0.999 ** t) / (1 - 0.5 ** t)
    b1, b2, eps, lr32 = (float(np.float32(c)) for c in (0.5, 0.999, 1e-8, lr_t))
    gg = grad.astype(np.float64)
    m2 = b1 * m.astype(np.float64) + (1.0 - b1) * gg
    v2 = (1.0 - b2) * gg * gg
    w2 = w.astype(np.float64) - lr32 * m2 / (np.sqrt(v2) + eps)
    with guarded("A") as g:
        dw, dm, dv = g.put(w, freeze=False), g.put(m, freeze=False), g.put(v, freeze=False)
        ops.adam_update(dw, g.put(grad), dm, dv, lr_t, grad_scale=1.0)
        g.check()
        gw, gm, gv = host(dw), host(dm), host(dv)
    assert np.isfinite(gw).all() and np.isfinite(gm).all() and np.isfinite(gv).all()
    report_close("m", gm, m2, atol=0.0, rtol=2.4e-7)
    report_close("v", gv, v2, atol=0.0, rtol=2.4e-7)
    report_close("w", gw, w2, atol=1e-7, rtol=1e-6)
    step = np.abs(gw.astype(np.float64) - w)
    assert (step > 10 * lr32).all() and (step < 20 * lr32).all()      # ~ lr_t * 0.5 / sqrt(0.001) = 15.8 lr_t


# ------------------------------------------------------------------ the whole step --------------
_FEED_KEYS = ("imgs", "trans_mat", "sample_pc", "sample_pc_rot", "sdf")
_UNIT_TOL = 2e-6          # of a variable's max |grad|: what each backward kernel is held to in its unit test


@pytest.fixture(scope="module", params=S.STEP_SHAPES, ids=lambda p: "B%d_N%d" % p)
def edge_step(request):
    """float64 oracle once per shape; per precision three steps on one Trainer: the feed, the feed again (run-to-run
    difference: atomics), the feed with every sample's points permuted"""
    from disn_amd.train_sdf import VARIABLE_ORDER, Trainer
    from disn_amd.weights import WeightStore
    B, N = request.param
    weights = O.init_weights(3, "he")
    feed = step_feed(B, N, 40 + B)
    L, grads, pred = T.loss_and_grads(feed, weights, np.float64)
    rng = np.random.default_rng(B * 100 + N)
    perm = np.stack([rng.permutation(N) for _ in range(B)])
    pfeed = dict(feed)
    for k in ("sample_pc", "sample_pc_rot", "sdf"):
        pfeed[k] = np.stack([feed[k][b][perm[b]] for b in range(B)])
    runs = {}
    for precision in S.STEP_PRECISIONS:
        with guarded("A") as g:
            tr = Trainer(WeightStore(weights), batch_size=B, precision=precision)
            g.frozen(tr.params)
            dfeed = {k: g.put(feed[k]) for k in _FEED_KEYS}
            dpfeed = {k: g.put(pfeed[k]) for k in _FEED_KEYS}
            out = []
            for f in (dfeed, dfeed, dpfeed):
                g.poison(tr.grads)
                p, dl = tr.forward_backward(f)
                torch.cuda.synchronize()
                out.append((host(p).copy(), host(dl).copy(), tr.grads.clone()))
            g.check()
            lay, rows = tr.flat.layout, {}
            for i, name in enumerate(VARIABLE_ORDER):       # per variable: scale, run-to-run and permuted difference
                sl = slice(int(lay.offset[i]), int(lay.offset[i]) + int(lay.count[i]))
                g1 = out[0][2][sl]
                rows[name] = (float(g1.abs().max()), float((out[1][2][sl] - g1).abs().max()),
                              float((out[2][2][sl] - g1).abs().max()), i)
            runs[precision] = dict(pred=out[0][0], dl=out[0][1], pred_perm=out[2][0], dl_perm=out[2][1],
                                   grads=tr.flat.to_arrays(out[0][2]), rows=rows)
            tr.close()
            del tr, out
        torch.cuda.empty_cache()
    return dict(B=B, N=N, L=L, grads=grads, pred=pred, perm=perm, runs=runs)


@pytest.mark.parametrize("precision", S.STEP_PRECISIONS)
def test_step_edges_forward_and_losses(edge_step, precision):
    """bounds of test_train_step_forward_and_losses"""
    from disn_amd.train_sdf import LOSS_NAMES
    s, r = edge_step, edge_step["runs"][precision]
    assert np.isfinite(r["pred"]).all()
    report_close("pred", r["pred"], s["pred"].reshape(r["pred"].shape), atol=2e-5, rtol=1e-5)
    for i, n in enumerate(LOSS_NAMES):
        assert abs(r["dl"][i] - s["L"][n]) <= 1e-5 * max(abs(s["L"][n]), 1.0) + 1e-6, (n, r["dl"][i], s["L"][n])


@pytest.mark.parametrize("precision", S.STEP_PRECISIONS)
def test_step_edges_gradients_vs_oracle(edge_step, precision):
    """the flip-tolerant metric and constants of test_train_step_gradients (why it is flip-tolerant: there)"""
    s, got = edge_step, edge_step["runs"][precision]["grads"]
    rows = []
    for name, ref in s["grads"].items():
        gv = got[name].astype(np.float64).ravel()
        rv = np.asarray(ref, np.float64).ravel()
        l2 = float(np.linalg.norm(gv - rv) / max(np.linalg.norm(rv), 1e-30))
        cos = float(gv @ rv / max(np.linalg.norm(gv) * np.linalg.norm(rv), 1e-30))
        rows.append((l2, cos, name))
    rows.sort(reverse=True)
    print("EDGE step B%d N%d %s worst (rel L2, cos): %s" % (s["B"], s["N"], precision, rows[:4]))
    assert rows[0][0] < 2e-2 and min(c for _, c, _ in rows) > 0.9995, rows[:6]


@pytest.mark.parametrize("precision", S.STEP_PRECISIONS)
def test_step_edges_repeat(edge_step, precision):
    """the same feed twice on one Trainer.  The fc layers and both point MLPs (variables 26 on) have no atomic upstream:
    bit for bit.  The convolutions sit below the gather's backward, whose atomics add in arrival order: capped at the
    unit tolerance, 2e-6 of the variable's max |grad| (measured: exactly zero at these small point sets).  With the
    one-pass fc backward kernel that ran until this test was written, the default mode at B = 3 gave 4.2e-3 on fc6 and
    7.6e-4 on the convolutions here: one to three stray elements of dz6 per step (csrc/backward.hip, fc_bwd_launch)."""
    r = edge_step["runs"][precision]
    worst = max((rr / max(scale, 1e-300), name) for name, (scale, rr, dp, i) in r["rows"].items())
    print("EDGE step B%d N%d %s worst run-to-run / max |grad|: %.3g (%s)" % (edge_step["B"], edge_step["N"], precision,
                                                                              worst[0], worst[1]))
    for name, (scale, rr, dp, i) in r["rows"].items():
        if i >= 26:
            assert rr == 0.0, (name, rr, scale)
        else:
            assert rr <= _UNIT_TOL * scale, (name, rr, scale)


@pytest.mark.parametrize("precision", S.STEP_PRECISIONS)
def test_step_edges_point_permutation(edge_step, precision):
    """A check without flips, which the oracle metric above cannot give: the same feed with every sample's N points
    permuted.  The encoder's forward is unchanged and a point's row does not depend on its position, so the
    predictions are the unpermuted ones bit for bit; every gradient differs by summation order only (rows of the
    point GEMMs, atomics of the gather's backward), over kernels each held to 2e-6 of max |grad|.  Bound per variable:
    four times the larger of that unit tolerance and the measured run-to-run difference of the unpermuted feed (zero on
    the MLP side, atomics on the VGG side).
    Measured on an MI355X, worst ratio = permuted difference / max(unit tolerance, run-to-run), bound 4:
        B = 1, N = 100   f32 0.57 (conv3_2 weights), f32_mfma 0.69 (conv1_1 weights); MLP side 0.10 / 0.12
        B = 3, N = 37    f32 0.49 (conv1_1 weights), f32_mfma 0.90 (conv1_1 weights); MLP side 0.09 / 0.10
    with a run-to-run difference of exactly zero in all four (no two points of these small sets meet in an order that
    matters).  The base cannot absorb a corruption: test_step_edges_repeat caps the run-to-run difference itself.  The
    per-variable figures are printed on every run."""
    s, r = edge_step, edge_step["runs"][precision]
    unperm = np.empty_like(r["pred_perm"])
    for b in range(s["B"]):
        unperm[b, s["perm"][b]] = r["pred_perm"][b]
    assert np.array_equal(unperm, r["pred"])
    for a, b in zip(r["dl_perm"], r["dl"]):         # the losses: sums over the points in another order
        assert abs(float(a) - float(b)) <= 1e-5 * max(abs(float(b)), 1.0) + 1e-6, (r["dl_perm"], r["dl"])
    ratios = []
    for name, (scale, rr, dp, i) in r["rows"].items():
        base = max(_UNIT_TOL * scale, rr)
        ratios.append((dp / max(base, 1e-300), name, dp / max(scale, 1e-300), rr / max(scale, 1e-300)))
    ratios.sort(reverse=True)
    print("EDGE step B%d N%d %s permutation ratio (worst first; ratio, name, perm diff / max, run-to-run / max):" % (
        s["B"], s["N"], precision))
    for row in ratios:
        print("EDGE   %.3f %s %.3g %.3g" % row)
    assert ratios[0][0] <= 4.0, ratios[:6]

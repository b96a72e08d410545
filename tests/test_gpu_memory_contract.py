"""The memory contract of every entry of include/disn_amd.h, asserted under guard bands and poison
(tests/guarded_alloc.py): buffers of exactly the documented size, guards untouched, ``const`` inputs unchanged,
results independent of what the buffers held before.

Every scenario builds its inputs on the host with a fixed seed, calls the project's Python wrappers (the raw C entries
only where no wrapper exists) and returns host arrays plus a closure that compares them with the reference and the
tolerance the entry's own test uses.  One parametrised test runs each scenario under variant A and variant B and
asserts: (a) guards and frozen inputs intact in both runs, (b) every result bit-identical between the runs (results
that go through float atomics: FLOAT_ATOMICS, compared under (c) only), (c) run A within the reference's tolerance,
(d) every entry the table claims for the scenario was really called.

ENTRY_COVERAGE / EXEMPT are checked against the header by tests/test_guarded_alloc_host.py (no GPU needed)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from guarded_alloc import guarded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENARIOS = {}            # name -> function(g) -> (results: dict of host arrays, verify(results))
ENTRY_COVERAGE = {}       # name -> the disn_* entries the scenario proves were called
TOLERANCE_ONLY = {}       # name -> result keys that go through float atomics: not compared bit for bit
# entries whose result depends on the order of float atomicAdds, with the atomic's file:line
_GATHER_BWD = ["disn_amd/csrc/backward_img.hip:%d" % n for n in (48, 49, 50, 51)]      # gather_bwd_kernel's scatter
FLOAT_ATOMICS = {
    "disn_gather_backward": _GATHER_BWD,          # result key "dmap"
    "disn_train_step": _GATHER_BWD,               # result key "grads_vgg": everything upstream of the feature map
}

# The other floating-point atomic of csrc/: mesh_clean.hip's pair_kernel, unsafeAtomicAdd of DOUBLES into a component's
# coordinate sum (disn_mesh_clean_count_batch).  The sum's last bits depend on the order, but it reaches a result only
# through keep_kernel's test `distance of the centroid < dist_thresh`, a discrete decision: the scenario's meshes (two
# fans, an icosphere of radius 0.4 about the origin) have their parts' centroids at distances that differ from the 0.5
# threshold by more than 0.1, 1e14 times the 1e-16 relative spread of a float64 sum, so `kept` and the emitted meshes
# are compared bit for bit (as test_gpu_mesh_clean.py does, under mesh_clean_fixtures.assert_margins' condition).
# Every other atomic in csrc/ is an integer add / min / max / or / CAS: order-independent results, except the ORDER of
# the sphere tracer's ray lists (sdf_trace.hip:90), which the trace scenario therefore compares as sets.
# entries that write no device memory and launch nothing
EXEMPT = {}


def scenario(name, entries, tolerance_only=()):
    def deco(fn):
        assert name not in SCENARIOS
        SCENARIOS[name] = fn
        ENTRY_COVERAGE[name] = tuple(entries)
        if tolerance_only:
            TOLERANCE_ONLY[name] = tuple(tolerance_only)
        return fn
    return deco


def host(t):
    return t.detach().cpu().numpy()


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def close(name, got, ref, atol, rtol=0.0):
    from conftest import report_close
    return report_close(name, got, ref, atol, rtol)


def rel_close(name, got, ref, rtol_of_max):
    ref = np.asarray(ref, np.float64)
    close(name, got, ref, atol=rtol_of_max * max(float(np.abs(ref).max()), 1e-30))


def bf16_round(a):
    return torch.from_numpy(f32(a)).to(torch.bfloat16).to(torch.float64).numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


_CACHE = {}


def cached(key, make):
    """host-side references and inputs shared between scenarios and variants: computed once, never modified"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _ops():
    from disn_amd import ops
    return ops


def _O():
    from oracle import disn_oracle as O
    return O


# =====================================================================================================================
# GEMM-shaped layers
# =====================================================================================================================
def _gemm_case(M, K, N, seed, positive=True, scale_w=2.0):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((M, K)).astype(np.float32)
    if positive:
        a = np.maximum(a, 0)
    w = (rng.standard_normal((K, N)) * np.sqrt(scale_w / K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    return a, w, b


@scenario("fc", ["disn_fc", "disn_fc_t"])
def _fc(g):
    ops, out, refs = _ops(), {}, {}
    for B, K, N in ((1, 1000, 256), (4, 1000, 256), (17, 1024, 512)):      # 17: a second gemv_mfma pass of one row
        x, w, b = _gemm_case(B, K, N, K + N + B)
        refs["fc_%d" % B] = x.astype(np.float64) @ w.astype(np.float64) + b
        out["fc_%d" % B] = host(ops.fc(g.put(x), g.put(w), g.put(b), False))
    x, w, b = _gemm_case(2, 100, 7, 108)
    refs["fc_t"] = x.astype(np.float64) @ w.astype(np.float64) + b
    out["fc_t"] = host(ops.fc_t(g.put(x), g.put(np.ascontiguousarray(w.T)), g.put(b), False))

    def verify(r):
        for k in refs:
            close(k, r[k], refs[k], atol=1e-5, rtol=1e-5)
    return out, verify


@scenario("dense", ["disn_dense", "disn_dense_bf16"])
def _dense(g):
    ops, out, refs = _ops(), {}, {}
    k1, k2, N = 512, 1472, 512
    for M in (1, 777):                                   # f32 MFMA with stream-K slabs in the workspace
        a, w, b = _gemm_case(M, k1 + k2, N, M + k1, positive=False)
        refs["dense_%d" % M] = np.maximum(a.astype(np.float64) @ w.astype(np.float64) + b, 0)
        out["dense_%d" % M] = host(ops.dense(g.put(a[:, :k1]), ops.pack_kn(g.put(w)), g.put(b), N, True,
                                             g.put(a[:, k1:])))
    M = 700
    a, w, b = _gemm_case(M, k1 + k2, N, M + k1, positive=False, scale_w=1.0)
    a1, a2, wd, bd = g.put(a[:, :k1]), g.put(a[:, k1:]), g.put(w), g.put(b)
    out["bf16"] = host(ops.dense_bf16(a1, wd, bd, True, a2))
    out["x3"] = host(ops.dense_bf16(a1, wd, bd, True, a2, nsplit=3))
    ref_bf = np.maximum(bf16_round(a) @ bf16_round(w) + b.astype(np.float64), 0)
    ref_x3 = np.maximum(a.astype(np.float64) @ w.astype(np.float64) + b, 0)

    def verify(r):
        for M in (1, 777):
            close("dense M=%d" % M, r["dense_%d" % M], refs["dense_%d" % M], atol=1e-5, rtol=1e-5)
        close("dense_bf16", r["bf16"], ref_bf, atol=2e-6 * np.abs(ref_bf).max(), rtol=2e-6)
        close("dense 3xbf16", r["x3"], ref_x3, atol=2e-6 * np.abs(ref_x3).max())
    return out, verify


def _h2_case(M, K, N, seed, positive=True):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((M, K)).astype(np.float32)
    if positive:
        a = np.maximum(a, 0) * 1.5
    w = (rng.standard_normal((K, N)) * np.sqrt(2.0 / K)).astype(np.float32)
    b = (rng.standard_normal(N) * 0.1).astype(np.float32)
    return a, w, b


@scenario("dense_h2", ["disn_dense_h2", "disn_pack_dense_h2"])
def _dense_h2(g):
    ops, out, refs = _ops(), {}, {}
    # one row; 700 rows reading two sources in place
    a, w, b = _h2_case(1, 512, 512, 1025)
    refs["one"] = a.astype(np.float64) @ w.astype(np.float64) + b
    o, amax = ops.dense_h2(g.put(a), ops.pack_dense_h2(g.put(w)), g.put(b), 512, False, want_amax=True)
    out["one"], out["one_amax"] = host(o), host(amax)
    M, k1, k2, N = 700, 512, 1472, 512
    a, w, b = _h2_case(M, k1 + k2, N, M + k1)
    a1, a2 = f32(a[:, :k1]), f32(a[:, k1:]) * 4.0
    refs["two"] = np.maximum(np.concatenate([a1, a2], 1).astype(np.float64) @ w.astype(np.float64) + b, 0)
    out["two"] = host(ops.dense_h2(g.put(a1), ops.pack_dense_h2(g.put(w)), g.put(b), N, True, a2=g.put(a2)))
    # deferred bias + ReLU on load
    pre, w, b = _h2_case(333, 512, 256, 5, positive=False)
    ib = (np.random.default_rng(6).standard_normal(512) * 0.7).astype(np.float32)
    refs["defer"] = np.maximum(np.maximum(pre.astype(np.float64) + ib, 0) @ w.astype(np.float64) + b, 0)
    out["defer"] = host(ops.dense_h2(g.put(pre), ops.pack_dense_h2(g.put(w)), g.put(b), 256, True, in_bias=g.put(ib)))
    # the batched form at its smallest: four images of 128 rows; then a K range with an addend, in place
    imgs, rows = 4, 128
    a, w, b = _h2_case(imgs * rows, 128, 512, 777)
    a = f32(a.reshape(imgs, rows, 128) * (0.5 + np.arange(imgs, dtype=np.float32)).reshape(imgs, 1, 1)).reshape(-1, 128)
    refs["batched"] = np.maximum(a.astype(np.float64) @ w.astype(np.float64) + b, 0)
    o, amax = ops.dense_h2(g.put(a), ops.pack_dense_h2(g.put(w)), g.put(b), 512, True, want_amax=True,
                           rows_per_image=rows)
    out["batched"], out["batched_amax"] = host(o), host(amax)
    a, w, b = _h2_case(imgs * rows, 2048, 512, 1234)
    a[:, 1984:] = 0
    point, feat = f32(a[:, :512]), f32(a[:, 512:])
    img = ops.pack_dense_h2(g.put(w))
    pre = ops.dense_h2(g.put(point), img, g.put(np.zeros(512, np.float32)), 512, False, a2=g.put(feat[:, :896]),
                       rows_per_image=rows, image_k=2048, k_begin=0)
    o = ops.dense_h2(g.put(feat[:, 896:]), img, g.put(b), 512, True, rows_per_image=rows, image_k=2048, k_begin=1408,
                     add_in=pre, out=pre)
    refs["krange"] = np.maximum(a.astype(np.float64) @ w.astype(np.float64) + b, 0)
    out["krange"] = host(o)

    def verify(r):
        close("dense_h2 one row", r["one"], refs["one"], atol=1e-5, rtol=1e-5)
        for k in ("one", "two", "defer", "krange"):
            assert np.abs(r[k] - refs[k]).max() <= 2e-6 * np.abs(refs[k]).max(), k
        for i in range(imgs):
            sl = slice(i * rows, (i + 1) * rows)
            assert np.abs(r["batched"][sl] - refs["batched"][sl]).max() <= 2e-6 * np.abs(refs["batched"][sl]).max(), i
        assert float(r["one_amax"][0]) == float(np.abs(r["one"]).max())
        assert float(r["batched_amax"][0]) == float(np.abs(r["batched"]).max())
    return out, verify


# =====================================================================================================================
# convolutions, pooling, resize
# =====================================================================================================================
def _conv_case(B, H, W, Cin, Cout, seed, relu_input=False):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, H, W, Cin)).astype(np.float32)
    if relu_input:
        x = np.maximum(x, 0) * 2.0
    w = (rng.standard_normal((3, 3, Cin, Cout)) * np.sqrt(2.0 / (9 * Cin))).astype(np.float32)
    b = (rng.standard_normal(Cout) * 0.1).astype(np.float32)
    return x, w, b


# tiling ids of disn_conv3x3_h2 at the smallest shapes where disn_conv3x3_h2_plan accepts them
CONV_H2_CASES = [((3, 6, 8, 192, 64), (0, 1, 2, 3, 4, 10)),
                 ((4, 10, 12, 128, 64), (0, 10, 18, 19)),
                 ((3, 28, 28, 192, 128), (5, 6, 7, 8, 9, 12, 13, 18)),
                 ((2, 30, 44, 64, 128), (5, 8))]


@scenario("conv3x3_h2", ["disn_conv3x3_h2", "disn_pack_conv_h2", "disn_conv_h2_gain_span"])
def _conv3x3_h2(g):
    from disn_amd import _lib
    ops, O, out, refs = _ops(), _O(), {}, {}
    for shape, tilings in CONV_H2_CASES:
        B, H, W, Cin, Cout = shape
        x, w, b = _conv_case(B, H, W, Cin, Cout, H + Cin)
        refs[shape] = cached(("conv_h2", shape), lambda: O.conv2d(x, w, b, "SAME", False, dtype=np.float64))
        xd, bd, img = g.put(x), g.put(b), ops.pack_conv_h2(g.put(w))
        g.frozen(img)
        span, warned = ops.conv_h2_gain_span(img, Cin, Cout)
        out["span_%s" % (shape,)] = np.float32([span, warned])
        for t in tilings:
            assert _lib.lib().disn_conv3x3_h2_plan(B, H, W, Cin, Cout, t, None, None) >= 0, (shape, t)
            o, pooled, amax = ops.conv3x3_h2(xd, img, bd, Cout, False, pool=True, want_amax=True, tiling=t)
            out["%s t%d" % (shape, t)] = host(o)
            out["%s t%d pool" % (shape, t)] = host(pooled)
            out["%s t%d amax" % (shape, t)] = host(amax)

    def verify(r):
        for shape, tilings in CONV_H2_CASES:
            B, H, W, Cin, Cout = shape
            assert r["span_%s" % (shape,)][0] < 12 and r["span_%s" % (shape,)][1] == 0
            for t in tilings:
                got = r["%s t%d" % (shape, t)]
                close("conv3x3_h2 tiling %d %s" % (t, shape), got, refs[shape], atol=1e-5, rtol=1e-5)
                assert float(np.abs(got - refs[shape]).max()) <= 2e-6 * float(np.abs(refs[shape]).max())
                assert np.array_equal(r["%s t%d pool" % (shape, t)],
                                      got.reshape(B, H // 2, 2, W // 2, 2, Cout).max(axis=(2, 4)))
                assert float(r["%s t%d amax" % (shape, t)][0]) == float(np.abs(got).max())
    return out, verify


# (BM, BN, workgroups) of test_conv3x3_every_tile_config_and_splitk, on its shape (M = 380 rows, N = 256, 36 k-steps)
CONV_PLANS = ["128,128,6", "128,64,12", "64,128,12", "64,64,24", "64,64,96", "128,128,18", "128,128,7", "64,128,256",
              "64,64,500", "128,64,1", "64,64,864"]


@scenario("conv3x3", ["disn_conv3x3", "disn_conv3x3_planned", "disn_conv1_1", "disn_pack_kn", "disn_conv3x3_x3",
                      "disn_pack_kn_x3", "disn_conv3x3_bf16"])
def _conv3x3(g):
    import torch.nn.functional as Fnn
    ops, O, out, refs = _ops(), _O(), {}, {}
    for shape in ((1, 16, 16, 3, 64), (1, 7, 9, 256, 512)):              # the K = 27 path; M = 63 < one tile
        B, H, W, Cin, Cout = shape
        x, w, b = _conv_case(*shape, seed=B * 1000 + H + Cin)
        refs[shape] = cached(("conv", shape), lambda: O.conv2d(x, w, b, "SAME", True, dtype=np.float64))
        packed = ops.pack_kn(g.put(w.reshape(-1, Cout)))
        if Cin == 3:
            out["pack_kn"] = host(packed)
            pack_w = w.reshape(-1, Cout)
        out["conv %s" % (shape,)] = host(ops.conv3x3(g.put(x), packed, g.put(b), Cout, True))
    shape = (1, 20, 19, 128, 256)
    x, w, b = _conv_case(*shape, seed=11)
    refs[shape] = cached(("conv", shape), lambda: O.conv2d(x, w, b, "SAME", True, dtype=np.float64))
    xd, bd, packed = g.put(x), g.put(b), g.frozen(ops.pack_kn(g.put(w.reshape(-1, 256))))
    for force in CONV_PLANS:
        out["planned " + force] = host(ops.conv3x3(xd, packed, bd, 256, True, plan=tuple(int(v) for v in force.split(","))))
    for B, H, W in ((1, 5, 3), (2, 37, 45)):
        rng = np.random.default_rng(H)
        x1 = rng.random((B, H, W, 3)).astype(np.float32)
        w1 = (rng.standard_normal((3, 3, 3, 64)) * np.sqrt(2.0 / 27)).astype(np.float32)
        b1 = (rng.standard_normal(64) * 0.1).astype(np.float32)
        refs["c11", B] = cached(("c11", B), lambda: O.conv2d(x1, w1, b1, "SAME", True, dtype=np.float64))
        o, amax = ops.conv1_1(g.put(x1), g.put(w1), g.put(b1), True, want_amax=True)
        out["conv1_1 %d" % B], out["conv1_1 %d amax" % B] = host(o), host(amax)
    # three-term bf16 image and the bf16-compute kernel: B = 2, 14 x 14, 64 -> 128
    rng = np.random.default_rng(2 * 100 + 14 + 64)
    x = rng.standard_normal((2, 14, 14, 64)).astype(np.float32)
    w = (rng.standard_normal((3, 3, 64, 128)) / math.sqrt(9 * 64)).astype(np.float32)
    b = (0.1 * rng.standard_normal(128)).astype(np.float32)

    def conv64(xx, ww):
        return torch.relu(Fnn.conv2d(torch.from_numpy(xx).permute(0, 3, 1, 2), torch.from_numpy(ww).permute(3, 2, 0, 1),
                                     torch.from_numpy(b.astype(np.float64)), padding=1)).permute(0, 2, 3, 1).numpy()
    ref_full = cached("conv_x3_ref", lambda: conv64(x.astype(np.float64), w.astype(np.float64)))
    ref_bf = cached("conv_bf_ref", lambda: conv64(bf16_round(x), bf16_round(w)))
    xd, wd, bd = g.put(x), g.put(w), g.put(b)
    out["x3"] = host(ops.conv3x3_x3(xd, ops.pack_kn_x3(g.put(w.reshape(-1, 128))), bd, 128, True))
    out["bf16"] = host(ops.conv3x3_bf16(xd, wd, bd, True))
    out["bf16x3"] = host(ops.conv3x3_bf16(xd, wd, bd, True, nsplit=3))

    def verify(r):
        K, N = pack_w.shape
        kpad = (K + 31) // 32 * 32
        packed = r["pack_kn"].reshape(kpad // 8, N // 32, 64, 4)
        wp = np.zeros((kpad, N), np.float32)
        wp[:K] = pack_w
        lane = np.arange(64)
        for t in range(4):
            k = np.arange(kpad // 8)[:, None, None] * 8 + 4 * (lane >> 5)[None, None, :] + t
            n = np.arange(N // 32)[None, :, None] * 32 + (lane & 31)[None, None, :]
            assert np.array_equal(packed[:, :, :, t], wp[k, n])
        for shape in ((1, 16, 16, 3, 64), (1, 7, 9, 256, 512)):
            close("conv3x3 %s" % (shape,), r["conv %s" % (shape,)], refs[shape], atol=1e-5, rtol=1e-5)
        for force in CONV_PLANS:
            close("conv3x3 force=%s" % force, r["planned " + force], refs[(1, 20, 19, 128, 256)], atol=1e-5, rtol=1e-5)
        for B in (1, 2):
            close("conv1_1 B=%d" % B, r["conv1_1 %d" % B], refs["c11", B], atol=2e-6, rtol=2e-6)
            assert float(r["conv1_1 %d amax" % B][0]) == float(np.abs(r["conv1_1 %d" % B]).max())
        close("conv 3-term image", r["x3"], ref_full, atol=2e-6 * np.abs(ref_full).max())
        close("conv 3xbf16", r["bf16x3"], ref_full, atol=2e-6 * np.abs(ref_full).max())
        close("conv3x3_bf16", r["bf16"], ref_bf, atol=2e-6 * np.abs(ref_bf).max(), rtol=2e-6)
    return out, verify


@scenario("resize_pool", ["disn_resize_bilinear", "disn_maxpool2x2", "disn_build_featmap"])
def _resize_pool(g):
    ops, O, out = _ops(), _O(), {}
    rng = np.random.default_rng(14 * 7 + 4)
    x = rng.standard_normal((2, 14, 14, 4)).astype(np.float32)
    base = rng.standard_normal((2, 137, 137, 16)).astype(np.float32)      # the destination: only channels 4..7 are written
    wide = g.put(base, freeze=False)
    ops.resize_bilinear(g.put(x), 137, 137, out=wide, out_coff=4)
    out["strided"] = host(wide)
    y = rng.random((2, 137, 137, 3)).astype(np.float32)
    out["up224"] = host(ops.resize_bilinear(g.put(y), 224, 224))
    p = rng.standard_normal((2, 6, 10, 8)).astype(np.float32)
    out["pool"] = host(ops.maxpool2x2(g.put(p)))
    out["featmap"] = host(ops.build_featmap([g.put(t) for t in _taps(2)]))

    def verify(r):
        assert np.array_equal(r["strided"][..., 4:8], O.resize_bilinear_legacy(x, 137, 137))
        keep = np.ones(16, bool)
        keep[4:8] = False
        assert same_bits(r["strided"][..., keep], base[..., keep]), "resize wrote outside its channel slice"
        assert np.array_equal(r["up224"], O.resize_bilinear_legacy(y, 224, 224))
        assert np.array_equal(r["pool"], O.max_pool_2x2(p))
        assert np.array_equal(r["featmap"], _featmap_ref())
    return out, verify



def _taps(V):
    """standard-normal taps of the true shapes for V images (signed: max is no maximum of ReLU outputs)"""
    return cached(("taps", V), lambda: [np.random.default_rng(17).standard_normal((V, hw, hw, ch), dtype=np.float32)
                                        for hw, ch in _ops().TAP_SHAPES])


def _maps(V):
    """per view the five up-sampled maps [1,137,137,ch] of _taps(V) (oracle resize)"""
    import multiview_reference as MR
    return cached(("maps", V), lambda: MR.view_maps(_taps(V)))


def _featmap_ref():
    return cached("featmap2", lambda: np.concatenate([np.concatenate(m, axis=3) for m in _maps(2)], axis=0))


def _cams(V):
    O = _O()
    return f32(np.stack([O.DEMO_TRANS_MAT[0], O.synth_trans_mat(30, 25, 0.8), O.synth_trans_mat(201.5, 30, 0.65)])[:V])


# =====================================================================================================================
# projection and gathers
# =====================================================================================================================
@scenario("gather", ["disn_project", "disn_gather", "disn_gather_taps", "disn_gather_taps_split", "disn_gather_fold",
                     "disn_gather_taps_pool", "disn_pool_embedding"])
def _gather(g):
    import fused_emulation as E
    import multiview_reference as MR
    ops, O, out, refs = _ops(), _O(), {}, {}
    B = 2
    taps_h, fm_h, tms = _taps(B), _featmap_ref(), _cams(B)
    taps, fm, tm = [g.put(t) for t in taps_h], g.put(fm_h), g.put(tms)
    amax_h = f32([max(float(np.abs(t[b]).max()) for t in taps_h) for b in range(B)])
    amax = g.put(amax_h)
    rng = np.random.default_rng(3)
    pmap_h = rng.standard_normal((137 * 137, 512)).astype(np.float32)
    pmap, bias_h = g.put(pmap_h), rng.standard_normal(512).astype(np.float32)
    bias = g.put(bias_h)
    taps3_h, cams3 = _taps(3), _cams(3)
    taps3, tm3 = [g.put(t) for t in taps3_h], g.put(cams3)
    w3 = f32([0.7, 0.2, 0.1])
    emb3 = rng.standard_normal((3, 1024)).astype(np.float32)
    for N in (1, 257, 10241):                          # 10241 points: the wave-per-point gather (B = 1)
        Bn = 1 if N == 10241 else B
        pts_h = np.random.default_rng(N).uniform(-1.2, 1.2, (Bn, N, 3)).astype(np.float32)
        pts = g.put(pts_h)
        sub = slice(0, Bn)
        tps = taps if Bn == B else [g.put(t[:1]) for t in taps_h]
        tmn = tm if Bn == B else g.put(tms[:1])
        refs["xy", N] = O.get_img_points(pts_h, tms[sub])
        refs["feat", N] = O.resampler(fm_h[sub], refs["xy", N])
        xy = ops.project(pts, tmn)
        out["xy %d" % N] = host(xy)
        out["taps %d" % N] = host(ops.gather_taps(tps, tmn, pts))
        out["split %d" % N] = host(ops.gather_taps_split(tps, tmn, pts, amax if Bn == B else g.put(amax_h[:1])))
        if N == 10241:
            continue
        out["gather %d" % N] = host(ops.gather(fm, g.frozen(xy)))
        pre_h = np.random.default_rng(N + 1).standard_normal((N, 512)).astype(np.float32)
        refs["fold", N] = (pre_h, O.resampler(pmap_h.reshape(1, 137, 137, 512), refs["xy", N][:1])[0])
        out["fold %d" % N] = host(ops.gather_fold(pmap, g.put(tms[:1]), g.put(pts_h[0]), g.put(pre_h), bias))
        rows = g.put(np.full((N + 3, 1472), -77.0, np.float32), freeze=False)     # rows beyond N stay untouched
        for pool, w in (("max", None), ("mean", w3)):
            ops.gather_taps_pool(taps3, tm3, g.put(pts_h[0]), pool, None if w is None else g.put(w), out=rows)
            out["pool %s %d" % (pool, N)] = host(rows)
            refs["pool", pool, N] = cached(("poolref", pool, N), lambda: MR.pool_views(
                MR.gather_views(_maps(3), cams3, pts_h[0]), pool, w))
    for pool, w in (("max", None), ("mean", w3)):
        out["emb " + pool] = host(ops.pool_embedding(g.put(emb3), pool, None if w is None else g.put(w)))

    def verify(r):
        for N in (1, 257, 10241):
            Bn = 1 if N == 10241 else B
            assert np.array_equal(r["xy %d" % N], refs["xy", N], equal_nan=True)
            assert np.array_equal(r["taps %d" % N], refs["feat", N]), N
            for b in range(Bn):
                assert np.array_equal(r["split %d" % N][b], E.split_rows(refs["feat", N][b], float(amax_h[b]))), (N, b)
            if N == 10241:
                continue
            assert np.array_equal(r["gather %d" % N], refs["feat", N])
            # relu(pre + g + bias): three fp32 terms in the kernel's own association -- within gamma_2 of the exact sum
            pre_h, gth = refs["fold", N]
            exact = pre_h.astype(np.float64) + gth + bias_h
            bound = 3 * 2.0 ** -24 * (np.abs(pre_h) + np.abs(gth) + np.abs(bias_h)).astype(np.float64)
            assert (np.abs(r["fold %d" % N] - np.maximum(exact, 0)) <= bound + 1e-30).all(), N
            for pool in ("max", "mean"):
                got = r["pool %s %d" % (pool, N)]
                assert np.array_equal(got[:N], refs["pool", pool, N]), (pool, N)
                assert (got[N:] == -77.0).all()
        assert np.array_equal(r["emb max"][0], MR.pool_views(emb3, "max", None))
        assert np.array_equal(r["emb mean"][0], MR.pool_views(emb3, "mean", w3))
    return out, verify


# =====================================================================================================================
# the point MLPs on given features (the variables as they are: DeviceWeights(equalise=False))
# =====================================================================================================================
def _store(seed=2):
    from disn_amd.weights import WeightStore
    return cached(("store", seed), lambda: WeightStore.random_init(seed, mode="he"))


def _mlp_ref(W, pts, emb, feat):
    O = _O()
    return (O.get_sdf_basic2(pts, emb, W, dtype=np.float64)
            + O.get_sdf_basic2_imgfeat_twostream(pts, feat[:, :, None, :], W, dtype=np.float64))[..., 0]


QUERY_CASES = ((1, 1), (2, 127), (5, 1000), (1, 8193))      # the last crosses the fused threshold and a chunk boundary


@scenario("sdf_mlp", ["disn_sdf_mlp"])
def _sdf_mlp_query(g):
    from disn_amd.engine import DeviceWeights
    ops, O, out, refs = _ops(), _O(), {}, {}
    store = _store()
    dw = DeviceWeights(store, torch.device("cuda", 0), equalise=False)
    fm_h = cached("fm_relu1", lambda: np.maximum(np.random.default_rng(6).standard_normal((1, 137, 137, 1472), dtype=np.float32), 0))
    fm = g.put(fm_h)
    for B, N in QUERY_CASES:
        rng = np.random.default_rng(B * 100 + N)
        pts_h = rng.uniform(-1, 1, (B, N, 3)).astype(np.float32)
        emb_h = rng.standard_normal((B, 1024)).astype(np.float32)
        feat_h = np.maximum(rng.standard_normal((B, N, 1472)), 0).astype(np.float32)
        sdf, gl, lo = ops.sdf_mlp(dw.mlp, g.put(pts_h), g.put(emb_h), g.put(feat_h), want_streams=True)
        out["mlp %d %d" % (B, N)], out["mlp g %d %d" % (B, N)], out["mlp l %d %d" % (B, N)] = host(sdf), host(gl), host(lo)
        refs["mlp", B, N] = cached(("mlpref", B, N), lambda: _mlp_ref(store.arrays, pts_h, emb_h, feat_h))
        if B == 1:                                     # disn_query on a given map: == project + gather + sdf_mlp
            tm_h = _cams(1)
            out["query %d" % N] = host(ops.query(dw.mlp, fm, g.put(emb_h), g.put(tm_h), g.put(pts_h)))
            refs["query", N] = cached(("queryref", N), lambda: _mlp_ref(
                store.arrays, pts_h, emb_h, O.resampler(fm_h, O.get_img_points(pts_h, tm_h))))

    def verify(r):
        for B, N in QUERY_CASES:
            close("mlp sum %s" % ((B, N),), r["mlp %d %d" % (B, N)], refs["mlp", B, N], atol=1e-5, rtol=1e-5)
            assert np.array_equal(r["mlp %d %d" % (B, N)], r["mlp g %d %d" % (B, N)] + r["mlp l %d %d" % (B, N)])
            if B == 1:
                close("query N=%d" % N, r["query %d" % N], refs["query", N], atol=1e-5, rtol=1e-5)
    return out, verify


# =====================================================================================================================
# the engine: encoder, query family, grids (weights, engines and encodings are created under the guards)
# =====================================================================================================================
def _imgs(B, seed=9):
    return cached(("imgs", B, seed), lambda: np.random.default_rng(seed).random((B, 137, 137, 3), dtype=np.float32))


def _engine(store=None, **kw):
    from disn_amd.engine import SdfEngine
    return SdfEngine(store or _store(), **kw)


def _fresh(eng):
    """drop the engine's cached workspaces: the next call allocates each at exactly the size its query returns (a cached
    larger one would hide an overrun)"""
    eng._ws.clear()
    return eng


def _internal(store):
    from conftest import internal_arrays
    return internal_arrays(store)


def _oracle_on_featmap(store, featmap_h, emb_h, pts, tms):
    """the float64 oracle decoder on the engine's own (equalised-unit) feature map and embedding"""
    O = _O()
    feat = O.resampler(featmap_h, O.get_img_points(pts, tms))
    return _mlp_ref(_internal(store), pts, emb_h, feat)


@scenario("encode", ["disn_encode", "disn_vgg16_forward", "disn_vgg16_conv_stack", "disn_scale_channels"])
def _encode(g):
    ops, O, out = _ops(), _O(), {}
    store, imgs_h = _store(0), _imgs(2)
    eng = _engine(store)
    imgs = g.put(imgs_h)
    enc = eng.encode(imgs)
    out["resized"], out["emb"] = host(enc.resized), host(enc.embedding)
    for k, t in enumerate(eng.true_taps(enc)):
        out["tap%d" % k] = host(t)
    out["featmap"] = host(eng.true_features(enc.featmap))
    resized, taps, emb = ops.vgg16_forward(eng._vgg, imgs)
    out["fwd_emb"] = host(emb)
    for k, t in enumerate(taps):
        out["fwd_tap%d" % k] = host(t)
    run = ops.ConvStackRun(eng._vgg, imgs)
    run.run()
    for k, t in enumerate(run.taps):
        out["stack_tap%d" % k] = host(t)
    out["pool5"] = host(run.pool5)
    pts_h = np.random.default_rng(2 * 100 + 700).uniform(-1, 1, (2, 700, 3)).astype(np.float32)
    tms = _cams(2)
    enc_q, sdf = _fresh(eng).encode_query(imgs, g.put(pts_h), g.put(tms))
    out["eq_sdf"], out["eq_emb"] = host(sdf), host(enc_q.embedding)
    ref = cached("encode_ref", lambda: O.encode(imgs_h, store.arrays, dtype=np.float64))

    def verify(r):
        resized, emb64, maps, eps = ref
        assert np.array_equal(r["resized"], resized)
        for k, nm in enumerate(O.TAP_NAMES):
            close(nm, r["tap%d" % k], eps["vgg_16/%s/%s" % (nm[:5], nm)], 1e-5, 1e-5)
            assert same_bits(r["fwd_tap%d" % k], r["stack_tap%d" % k]), nm      # the same kernels on the same image
        close("embedding", r["emb"], emb64, 1e-5, 1e-5)
        close("embedding (vgg16_forward)", r["fwd_emb"], emb64, 1e-5, 1e-5)
        close("featmap", r["featmap"], np.concatenate(maps, axis=3), 1e-5, 1e-5)
        assert np.array_equal(r["pool5"], O.max_pool_2x2(r["stack_tap4"]))
        assert same_bits(r["eq_emb"], r["emb"])
        feat = O.resampler(np.concatenate(maps, axis=3), O.get_img_points(pts_h, tms))
        close("encode_query vs oracle", r["eq_sdf"], _mlp_ref(store.arrays, pts_h, emb64, feat), 1e-5)
    return out, verify


QUERY_FAMILY_PER_CASE = ("disn_query", "disn_query_folded", "disn_query_fused", "disn_query_taps_fused", "disn_query_grad",
                         "disn_encode_query")


@scenario("query_family", ["disn_fold_local", "disn_amax"] + list(QUERY_FAMILY_PER_CASE))
def _query_family(g):
    ops, out, refs, grad_inputs = _ops(), {}, {}, {}
    store, imgs_h = _store(), _imgs(5, 11)
    eng = _engine(store)
    enc = eng.encode(g.put(imgs_h))
    fm_h, emb_h = host(eng.featmap_of(enc)), host(enc.embedding)
    out["pmap0"] = host(eng.pmap_of(enc, 0))
    out["pmap_amax0"] = host(eng.pmap_amax_of(enc, 0))
    tms_all = f32(np.stack([_O().DEMO_TRANS_MAT[0] if b % 2 == 0 else _O().synth_trans_mat(30 + 20 * b, 25, 0.8)
                            for b in range(5)]))
    for B, N in QUERY_CASES:
        pts_h = np.random.default_rng(B * 11 + N).uniform(-1, 1, (B, N, 3)).astype(np.float32)
        tms = tms_all[:B]
        sub = type(enc)(enc.resized[:B], [t[:B] for t in enc.taps], enc.embedding[:B], enc.featmap[:B])
        sub.pmap, sub.pmap_amax = enc.pmap, enc.pmap_amax
        pts, tm = g.put(pts_h), g.put(tms)
        first = len(g.called)
        out["plain %d %d" % (B, N)] = host(_fresh(eng).query(sub, pts, tm, fold=False))
        out["folded %d %d" % (B, N)] = host(_fresh(eng).query(sub, pts, tm, fold=True, fused=False))
        out["fused %d %d" % (B, N)] = host(_fresh(eng).query(sub, pts, tm, fold=True, fused=True))
        out["taps %d %d" % (B, N)] = host(ops.query_taps_fused(eng.weights.mlp, sub.taps, sub.embedding, tm, pts))
        sdf, grad = _fresh(eng).query_grad(sub, pts, tm)
        out["grad_sdf %d %d" % (B, N)], out["grad %d %d" % (B, N)] = host(sdf), host(grad)
        idx = np.unique(np.concatenate([np.arange(0, N, max(1, N // 300)), [N - 1]]))
        refs[B, N] = (idx, cached(("qfam", B, N), lambda: _oracle_on_featmap(store, fm_h[:B], emb_h[:B], pts_h[:, idx], tms)))
        grad_inputs[B, N] = (pts_h, tms)
        # rows A..H in one call on the first B images: its own encoder state (a call of one or two images runs the
        # single-image kernel forms, five the batched ones), so the oracle continues from ITS taps and embedding
        enc_q, sdf_q = _fresh(eng).encode_query(g.put(imgs_h[:B]), pts, tm)
        out["eq %d %d" % (B, N)] = host(sdf_q)
        fq, eq = host(eng.featmap_of(enc_q)), host(enc_q.embedding)
        refs["eq", B, N] = cached(("qfam_eq", B, N), lambda: _oracle_on_featmap(store, fq, eq, pts_h[:, idx], tms))
        ran = set(g.called[first:])                       # (d) per shape: no case fell back to another entry
        assert set(QUERY_FAMILY_PER_CASE) <= ran, ((B, N), sorted(set(QUERY_FAMILY_PER_CASE) - ran))

    def verify(r):
        w = _internal(store)["sdfprediction_imgfeat/fold2/conv1/weights"][0, 0].astype(np.float64)
        ref = fm_h[0].reshape(-1, 1472).astype(np.float64) @ w[512:]
        assert np.abs(r["pmap0"] - ref).max() / np.abs(ref).max() < 4e-6
        assert float(r["pmap_amax0"][0]) == float(np.abs(r["pmap0"]).max())
        for B, N in QUERY_CASES:
            idx, want = refs[B, N]
            close("query %s" % ((B, N),), r["plain %d %d" % (B, N)][:, idx], want, 1e-5, 1e-5)
            close("encode_query %s" % ((B, N),), r["eq %d %d" % (B, N)][:, idx], refs["eq", B, N], 1e-5)
            close("folded %s" % ((B, N),), r["folded %d %d" % (B, N)][:, idx], want, 1e-5, 1e-5)
            close("fused %s" % ((B, N),), r["fused %d %d" % (B, N)][:, idx], want, 1e-5)
            close("taps fused %s" % ((B, N),), r["taps %d %d" % (B, N)][:, idx], want, 1e-5)
            close("pred_sdf of query_grad %s" % ((B, N),), r["grad_sdf %d %d" % (B, N)][:, idx], want, 1e-5, 1e-5)
            assert np.isfinite(r["grad %d %d" % (B, N)]).all()
        # the gradients against the float64 forward-mode reference on the engine's own feature map and embedding, where
        # a gradient is comparable (sdf_grad_reference.included); the bound is test_gpu_sdf_grad.py's rule on these
        # points: twice the error of the same reference run in numpy float32
        import sdf_grad_reference as SG
        Wi = _internal(store)
        e32 = None
        for B, N in ((5, 1000), (2, 127), (1, 1), (1, 8193)):
            pts_h, tms = grad_inputs[B, N]
            sel = refs[B, N][0] if N > 1000 else np.arange(N)      # past the chunk boundary: the strided sample of pred_sdf
            pts_h = np.ascontiguousarray(pts_h[:, sel])
            ref = SG.reference(Wi, None, pts_h, tms, np.float64, (emb_h[:B].astype(np.float64), fm_h[:B]))
            inc = SG.included(ref)
            if e32 is None:
                run32 = SG.reference(Wi, None, pts_h, tms, np.float32, (emb_h[:B], fm_h[:B]))
                e32 = float(np.abs(run32["grad"].astype(np.float64) - ref["grad"])[inc].max())
                print("[query_grad] (%d, %d): %.1f %% of the points comparable, e32 = %.3g (float32 run of the reference "
                      "vs float64)" % (B, N, 100 * inc.mean(), e32))
                assert inc.mean() >= 0.5                     # the comparison is not vacuous
            if inc.any():
                err = np.abs(r["grad %d %d" % (B, N)][:, sel].astype(np.float64) - ref["grad"])[inc].max()
                print("[query_grad] (%d, %d): gradient max |gpu - f64| %.3g on %d points" % (B, N, err, inc.sum()))
                assert err <= 2 * e32, ((B, N), err, e32)
    return out, verify


GRID_R = 12
GRID_BOX = [-1, -0.9, -0.8, 1, 0.9, 0.8]
BAND_CASES = ((2, 2), (4, 4), (12, 2), (12, 4))       # (R, stride): the smallest grid band_check takes for either stride
VIEW_POINTS = tuple(N for _, N in QUERY_CASES)        # 1, 127, 1000, 8193


@scenario("grids", ["disn_grid_points", "disn_query_grid", "disn_query_grid_folded", "disn_query_grid_fused",
                    "disn_query_grid_ctx", "disn_query_grid_listed", "disn_grid_band_select", "disn_grid_band_fill",
                    "disn_query_views", "disn_query_grid_views"])
def _grids(g):
    import grid_band_reference as G
    ops, O, out = _ops(), _O(), {}
    store, imgs_h = _store(), _imgs(2, 13)
    eng = _engine(store)
    enc = eng.encode(g.put(imgs_h))
    fm_h, emb_h = host(eng.featmap_of(enc)), host(enc.embedding)
    R, box, total = GRID_R, GRID_BOX, (GRID_R + 1) ** 3
    k0, k1 = 5, total - 7                               # a flat range inside the grid
    tm_h = _cams(1)
    tm = g.put(tm_h)
    out["points"] = host(ops.grid_points(box, R, k0, k1, "cuda"))
    out["plain"] = host(_fresh(eng).query_grid(enc, 0, tm, box, R, k0, k1, fold=False))
    out["folded"] = host(_fresh(eng).query_grid(enc, 0, tm, box, R, k0, k1, fused=False))
    out["fused"] = host(_fresh(eng).query_grid(enc, 0, tm, box, R, k0, k1, fused=True))
    _fresh(eng)
    out["ctx"] = host(eng.query_grid(enc, 0, tm, box, R, k0, k1, pipelined=True))
    dense = _fresh(eng).query_grid(enc, 0, tm, box, R, fused=True)
    out["dense"] = host(dense)
    isos = {}
    for Rb, s in BAND_CASES:
        if Rb not in isos:
            out["dense R%d" % Rb] = host(_fresh(eng).query_grid(enc, 0, tm, box, Rb, fused=True))
            isos[Rb] = float(np.median(out["dense R%d" % Rb]))
        band, stats = _fresh(eng).query_grid_band(enc, 0, tm, box, Rb, iso=isos[Rb], stride=s, margin=0.5, dilate=1)
        out["band R%d s%d" % (Rb, s)] = host(band)
        out["band R%d s%d stats" % (Rb, s)] = np.int64([stats[k] for k in sorted(stats)])
    # the selection alone on an analytic field, with the grid as a const input
    n = R + 1
    i = np.arange(n, dtype=np.float32)
    z, y, x = np.meshgrid(i, i, i, indexing="ij")
    c = np.float32(R / 2.0)
    vol = f32(np.sqrt((x - c - np.float32(0.3)) ** 2 + (y - c) ** 2 + (z - c + np.float32(0.7)) ** 2)
              - np.float32(0.31 * R)).ravel()
    grid = g.put(vol)
    mask, idx, counts = ops.grid_band_select(grid, R, 4, 0.0, 0.5, 1)
    out["sel_mask"], out["sel_counts"] = host(mask), host(counts)
    out["sel_idx"] = host(idx)[:int(out["sel_counts"][0])]
    filled = g.put(vol, freeze=False)
    ops.grid_band_fill(filled, R, 4, mask)
    out["sel_fill"] = host(filled)
    # pooled over two views
    tm2_h = _cams(2)
    view_pts = {N: np.random.default_rng(5 + N).uniform(-1, 1, (N, 3)).astype(np.float32) for N in VIEW_POINTS}
    for N in VIEW_POINTS:
        first = len(g.called)
        for pool in ("max", "mean"):
            out["views %s %d" % (pool, N)] = host(_fresh(eng).query_views(enc, (0, 2), g.put(tm2_h), g.put(view_pts[N]), pool))
        assert g.called[first:].count("disn_query_views") == 2, N
    for pool in ("max", "mean"):
        out["grid_views " + pool] = host(_fresh(eng).query_grid_views(enc, (0, 2), g.put(tm2_h), box, R, pool, k0=k0, k1=k1))
        out["grid_views_pts " + pool] = host(_fresh(eng).query_views(enc, (0, 2), g.put(tm2_h), ops.grid_points(box, R, k0, k1, "cuda"), pool))

    def verify(r):
        import multiview_reference as MR
        pts = O.grid_points(np.asarray(box, np.float64), R)
        assert np.array_equal(r["points"], pts[k0:k1])
        want = cached("gridref", lambda: _oracle_on_featmap(store, fm_h[:1], emb_h[:1], pts[None, k0:k1].astype(np.float32), tm_h)[0] / 10.0)
        for k in ("plain", "folded", "fused", "ctx"):
            close("grid " + k, r[k], want, 1e-6, 1e-5)
        assert same_bits(r["fused"], r["dense"][k0:k1]), "a range of the fused grid differs from the whole grid"
        assert same_bits(r["dense R%d" % R], r["dense"])
        for Rb, s in BAND_CASES:
            got, dense_b = r["band R%d s%d" % (Rb, s)], r["dense R%d" % Rb]
            mask = G.select(got, Rb, s, isos[Rb], 0.5, 1)
            ev = G.evaluated_mask(mask, Rb, s)
            stats = dict(zip(sorted(("coarse_points", "band_points", "active_cells", "total_points")),
                             r["band R%d s%d stats" % (Rb, s)].tolist()))
            assert stats == {"coarse_points": (Rb // s + 1) ** 3, "band_points": int(ev.sum()) - (Rb // s + 1) ** 3,
                             "active_cells": int(mask.sum()), "total_points": (Rb + 1) ** 3}, (Rb, s)
            assert same_bits(got[ev], dense_b[ev]), "an evaluated point differs from the dense fused grid: %s" % ((Rb, s),)
            assert same_bits(got, G.fill(got, mask, Rb, s)), "a filled point differs from the reference fill: %s" % ((Rb, s),)
        ref_mask = G.select(vol, R, 4, 0.0, 0.5, 1)
        ref_band = np.nonzero(G.band_mask(ref_mask, R, 4))[0]
        assert np.array_equal(r["sel_mask"].reshape(ref_mask.shape), ref_mask.astype(np.int32))
        assert r["sel_counts"].tolist() == [ref_band.size, int(ref_mask.sum())]
        assert np.array_equal(r["sel_idx"], ref_band)
        assert same_bits(r["sel_fill"], G.fill(vol, ref_mask, R, 4))
        maps = [fm_h[:, :, :, o:o + ch] for o, ch in zip((0, 64, 192, 448, 960), (64, 128, 256, 512, 512))]
        per_view = [[mp[v:v + 1] for mp in maps] for v in range(2)]
        for pool in ("max", "mean"):
            for N in VIEW_POINTS:                         # (a strided sample past 1000 points: a point's value is its own)
                sel = np.unique(np.concatenate([np.arange(0, N, max(1, N // 300)), [N - 1]]))
                ref = MR.pred_views(per_view, emb_h, tm2_h, view_pts[N][sel], _internal(store), pool, None, dtype=np.float64)
                assert r["views %s %d" % (pool, N)].shape == (N,)
                assert np.abs(r["views %s %d" % (pool, N)][sel] - ref).max() <= 1e-5, (pool, N)
            assert np.array_equal(r["grid_views " + pool], r["grid_views_pts " + pool] / np.float32(10.0))
    return out, verify


# =====================================================================================================================
# marching cubes, metrics, meshes
# =====================================================================================================================
@scenario("marching_cubes", ["disn_mc_count", "disn_mc_emit", "disn_mc_count_batch", "disn_mc_emit_batch"])
def _marching_cubes(g):
    import reconstruct_fixtures as RF
    from disn_amd import isosurface
    from oracle import mc_oracle as M
    out = {}
    R = 4                                               # 5^3 nodes
    box = np.asarray([-1.0, -0.9, -1.0, 1.0, 1.0, 0.8], np.float64)
    vols = [RF.noise(R, 3), np.ones((R + 1,) * 3, np.float32), RF.sphere(R, 0.6)]
    for k, vol in enumerate(vols[:2]):                  # a noise grid and an empty one
        v, f = isosurface.marching_cubes(g.put(vol.reshape(-1)), box, R, 0.0)
        out["v%d" % k], out["f%d" % k] = host(v), host(f)
    boxes = np.stack([box, box, box * 0.5])
    got = isosurface.marching_cubes_batch(g.put(np.stack([v.reshape(-1) for v in vols])), boxes, R, 0.0)
    for k, (v, f) in enumerate(got):
        out["bv%d" % k], out["bf%d" % k] = host(v), host(f)

    def verify(r):
        for k in range(3):
            vr, fr = M.marching_cubes(vols[k], boxes[k], 0.0)
            assert same_bits(r["bv%d" % k].reshape(-1, 3), f32(vr).reshape(-1, 3)) and np.array_equal(r["bf%d" % k].reshape(-1, 3), fr.reshape(-1, 3)), k
            if k < 2:
                assert same_bits(r["v%d" % k], r["bv%d" % k]) and same_bits(r["f%d" % k], r["bf%d" % k]), k
        assert len(r["f0"]) > 0 and len(r["f1"]) == 0 and len(r["bf2"]) > 0
    return out, verify


def _clouds(seed, b, n, m):
    rng = np.random.default_rng(seed)

    def one(k):
        v = rng.standard_normal((b, k, 3))
        v /= np.linalg.norm(v, axis=2, keepdims=True)
        return (0.4 * v + 0.02 * rng.standard_normal((b, k, 3))).astype(np.float32)
    return one(n), one(m)


@scenario("metrics", ["disn_nn_distance", "disn_approx_match", "disn_match_cost", "disn_emd"])
def _metrics(g):
    import metrics_reference as R
    from disn_amd import metrics
    out, inputs = {}, {}
    for b, n, m in ((1, 1, 1), (2, 1000, 37)):
        x1, x2 = _clouds(b * 7 + n + m, b, n, m)
        inputs["nn", n] = (x1, x2)
        for name, t in zip(("dist1", "idx1", "dist2", "idx2"), metrics.nn_distance(g.put(x1), g.put(x2))):
            out["%s %d" % (name, n)] = host(t)
    for b, n, m in ((1, 7, 5), (2, 300, 129)):
        x1, x2 = _clouds(b + n * 3 + m, b, n, m)
        inputs["emd", n] = (x1, x2)
        a, c = g.put(x1), g.put(x2)
        match = metrics.approx_match(a, c)
        out["match %d" % n] = host(match)
        out["cost %d" % n] = host(metrics.match_cost(a, c, g.frozen(match)))
        out["emd %d" % n] = host(metrics.emd(a, c))

    def verify(r):
        for n in (1, 1000):
            for name, want in zip(("dist1", "idx1", "dist2", "idx2"), R.nn_distance(*inputs["nn", n])):
                assert np.array_equal(r["%s %d" % (name, n)], want), (name, n)
        for n in (7, 300):
            x1, x2 = inputs["emd", n]
            ref = R.approx_match(x1, x2)
            ref_cost = R.match_cost(x1, x2, ref)
            gm = r["match %d" % n].astype(np.float64)
            assert np.isfinite(gm).all()
            for i in range(len(ref)):
                assert np.abs(gm[i] - ref[i]).sum() <= 1e-4 * ref[i].sum()
                assert np.abs(gm[i].sum(0) - ref[i].sum(0)).max() <= 1e-4
                assert np.abs(gm[i].sum(1) - ref[i].sum(1)).max() <= 1e-4
            np.testing.assert_allclose(r["cost %d" % n].astype(np.float64), ref_cost, rtol=1e-5)
            np.testing.assert_allclose(r["emd %d" % n].astype(np.float64), ref_cost, rtol=1e-5)
            np.testing.assert_allclose(r["emd %d" % n].astype(np.float64), r["cost %d" % n].astype(np.float64), rtol=1e-6)
    return out, verify


def _soup300():
    rng = np.random.default_rng(3)
    n = 300
    v = rng.uniform(-0.8, 0.8, (3 * n, 3)).astype(np.float32)
    f = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    f[n - 1] = f[n - 2]
    v[1] = v[0]
    v[5] = v[3] + np.float32(0.5) * (v[4] - v[3])
    return v, f


@scenario("mesh_sdf", ["disn_mesh_udf_points", "disn_mesh_udf_grid", "disn_mesh_sign", "disn_render_views"])
def _mesh_sdf(g):
    import mesh_sdf_reference as R
    import render_reference as RR
    from disn_amd import mesh_sdf, render
    out = {}
    v, f = _soup300()
    m = mesh_sdf.MeshBvh(v, f)
    pts = np.random.default_rng(0).uniform(-1, 1, (257, 3)).astype(np.float32)
    pts[:50] = v[f[:50, 0]]
    out["udf"] = host(mesh_sdf.unsigned_distance(m, None, g.put(pts)))
    out["udf_brute"] = host(mesh_sdf.unsigned_distance(m, None, g.put(pts), brute=True))
    res = 5                                             # 6^3 nodes: ragged 4^3 bricks
    axes = mesh_sdf.grid_axes(np.float32([-1, -1, -1, 1, 1, 1]), res)
    tau, steps = mesh_sdf.seal_params(axes, 1.0)
    u = mesh_sdf.unsigned_distance_grid(m, None, axes)
    out["u"] = host(u)
    sdf, outside = mesh_sdf.sign_grid(m, None, axes, g.frozen(u), tau, steps, 0.01)
    out["sdf"], out["outside"] = host(sdf), host(outside)
    cv, cf = RR.unit_cube()
    cams = render.ray_cameras([[30.0, 27.0, 0.0, 0.8, 25.0], [0.0, 0.0, 0.0, 0.9, 25.0], [200.0, 25.0, 0.0, 0.7, 25.0]], 33, 33)
    img = render.render_views(mesh_sdf.MeshBvh(cv, cf), None, None, size=(33, 33), samples=1, want=("rgba", "depth", "face"),
                              cams=cams)
    for k in ("rgba", "depth", "face"):
        out["render " + k] = host(img[k])

    def verify(r):
        assert np.array_equal(r["udf"], r["udf_brute"]) and np.array_equal(r["udf"], R.udf(pts, v, f))
        assert np.array_equal(r["u"], R.udf(R.grid_points(axes), v, f))
        n = res + 1
        u3 = r["u"].reshape(n, n, n)
        want = R.flood(u3, R.crossing_bits(axes, u3, tau, v, f), tau, steps)
        assert np.array_equal(r["outside"].reshape(n, n, n).astype(bool), want)
        assert np.array_equal(r["sdf"].reshape(n, n, n), R.signed(u3, want, 0.01))
        want_rgba, want_depth, want_face = RR.render(cv, cf, cams, 33, 33, 1)
        assert np.array_equal(r["render face"], want_face) and np.array_equal(r["render depth"], want_depth)
        assert np.array_equal(r["render rgba"], want_rgba)
    return out, verify


def _voxel_soup(seed, n_small, n_big):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-0.8, 0.8, (n_small, 1, 3))
    small = c + rng.normal(0.0, 0.012, (n_small, 3, 3))
    big = rng.uniform(-0.95, 0.95, (n_big, 3, 3))
    tri = np.concatenate([small, big])[rng.permutation(n_small + n_big)].astype(np.float32)
    return tri.reshape(-1, 3), np.arange(3 * tri.shape[0], dtype=np.int32).reshape(-1, 3)


def _voxel_cases():
    v = np.array([[0.1, 0.1, 0.1], [0.5, 0.12, 0.1], [0.3, 0.4, 0.15], [-0.5, -0.5, -0.5], [0.5, 0.5, 0.5], [0.0, 0.0, 0.0],
                  [0.3, -0.3, 0.2], [-0.4, 0.6, -0.1]], np.float32)
    f = np.array([[0, 1, 2], [3, 4, 5], [3, 3, 4], [6, 6, 6], [7, 6, 7], [0, 2, 1], [5, 5, 5]], np.int32)
    return {"soup_dim64": (_voxel_soup(2, 500, 3), 64), "degenerate": ((v, f), 110),
            "empty": ((np.zeros((4, 3), np.float32), np.zeros((0, 3), np.int32)), 110)}


@scenario("voxel", ["disn_voxel_surface", "disn_voxel_fill", "disn_voxel_index_grid", "disn_voxel_iou"])
def _voxel(g):
    import voxel_reference as R
    from disn_amd import voxel
    out = {}
    cases = _voxel_cases()
    for name, ((v, f), dim) in cases.items():
        vox = voxel.surface_voxels(g.put(v), g.put(f), dim)
        out[name + " surface"] = voxel.to_dense(vox)
        out[name + " index"] = voxel.to_dense(voxel.index_grid(vox))
        out[name + " fill"] = voxel.to_dense(voxel.fill(vox))
        out[name + " words"] = host(vox.words)
    (gv, gf), idim = cases["soup_dim64"]
    shifted = (gv + np.float32(0.03)).astype(np.float32)
    for mode in ("reference", "solid"):
        iou, inter, union = voxel.iou_views((gv, gf), [(shifted, gf), (gv, gf)], dim=idim, mode=mode)
        out["iou " + mode] = np.stack([inter, union])

    def verify(r):
        for name, ((v, f), dim) in cases.items():
            ref, ovf = R.surface_voxels(v, f, dim)
            assert not ovf
            assert np.array_equal(r[name + " surface"], ref), name
            assert np.array_equal(r[name + " index"], R.index_grid(ref, dim)), name
            assert np.array_equal(r[name + " fill"], R.fill(ref)), name
        sg = R.surface_voxels(gv, gf, idim)[0]
        ss = R.surface_voxels(shifted, gf, idim)[0]
        for mode in ("reference", "solid"):
            grid = (lambda s: R.index_grid(s, idim)) if mode == "reference" else R.fill
            want = [R.iou_counts(grid(sg), grid(s)) for s in (ss, sg)]
            assert r["iou " + mode][0].tolist() == [w[0] for w in want], mode
            assert r["iou " + mode][1].tolist() == [w[1] for w in want], mode
    return out, verify


@scenario("mesh_clean", ["disn_mesh_components_device", "disn_mesh_clean_count_batch", "disn_mesh_clean_emit_batch"])
def _mesh_clean(g):
    import mesh_clean_fixtures as MF
    import voxel_reference as VR
    from disn_amd import postprocess
    out = {}
    ico = VR.icosphere(0.4, 1)
    meshes = [MF.fans(), (np.zeros((3, 3), np.float32), np.zeros((0, 3), np.int32)), (f32(ico[0]), np.asarray(ico[1], np.int32))]
    for k, (v, f) in enumerate(meshes):
        for conn in ("face", "vertex"):
            labels, counts = postprocess.separate_mesh_device(g.put(v), g.put(f) if len(f) else torch.from_numpy(f).cuda(), conn)
            out["labels %d %s" % (k, conn)], out["counts %d %s" % (k, conn)] = host(labels), host(counts)
    dev = [(g.put(v), g.put(f) if len(f) else torch.from_numpy(f).cuda()) for v, f in meshes]
    cleaned, kept = postprocess.clean_meshes_device(dev, 0.5, 0.0, strict=False)
    for k in range(3):
        if cleaned[k] is not None:
            out["clean v%d" % k], out["clean f%d" % k] = host(cleaned[k][0]), host(cleaned[k][1])
        out["kept %d" % k] = host(kept[k])

    def verify(r):
        for k, (v, f) in enumerate(meshes):
            for conn in ("face", "vertex"):
                hl, hc = postprocess.separate_mesh(v, f, conn)
                assert np.array_equal(r["labels %d %s" % (k, conn)], hl) and np.array_equal(r["counts %d %s" % (k, conn)], hc)
            if len(f) == 0:
                assert r["kept %d" % k].size == 0
                continue
            want = MF.host_clean(v, f, 0.5, 0.0)
            assert same_bits(r["clean v%d" % k], np.ascontiguousarray(want[0])) and np.array_equal(r["clean f%d" % k], want[1])
            assert r["kept %d" % k].tolist() == list(want[2])
    return out, verify


# =====================================================================================================================
# sphere tracing
# =====================================================================================================================
@scenario("trace", ["disn_trace_setup", "disn_trace_advance", "disn_trace_collect", "disn_trace_shade"])
def _trace(g):
    import sdf_trace_reference as T
    from disn_amd import render
    ops, O, out = _ops(), _O(), {}
    W, H = 13, 9
    box = [-1, -0.9, -0.8, 1, 0.9, 0.8]
    demo = render.sdf_ray_cameras(O.DEMO_TRANS_MAT, W, H)[0]
    inside = demo.copy()
    inside[:3] *= np.float32(0.4)
    synth = np.asarray([-0.05, 0.3, -2.0, 0, 0, 1, 0.01, 0, 0, 0, 0, 0], np.float32)
    cams = np.stack([demo, inside, synth])
    n = cams.shape[0] * H * W
    cam_d = g.put(cams)
    state = ops.trace_state(n, cam_d.device)
    view = ops.trace_state_view(state, n)
    pts = torch.empty((n, 3), dtype=torch.float32, device=cam_d.device)
    ops.trace_setup(cam_d, (W, H), box, state, pts)
    ref, ref_active = T.setup(cams, H, W, box)
    names = T.FLOAT_FIELDS + tuple(k for k in T.INT_FIELDS if k != "hit_slot")
    cur, it = 0, 0
    while True:
        for name in names:
            assert same_bits(host(view[name]), ref[name]), (it, name)
        cnt = int(view["counts"][cur].item())
        lst = host(view["lists"][cur][:cnt]).astype(np.int64)
        assert cnt == ref_active.size and np.array_equal(np.sort(lst), ref_active), it
        p = host(pts[:cnt])
        assert same_bits(p, T.points(ref["org"], ref["dir"], ref["t"], lst)), it
        if cnt == 0:
            break
        vals = T.sphere(p)
        ops.trace_advance(cam_d, (W, H), state, g.put(vals), cnt, cur, pts, **T.DEFAULTS)
        ref_active = np.sort(T.advance(ref, lst, vals, **T.DEFAULTS))
        cur, it = 1 - cur, it + 1
        assert it <= T.DEFAULTS["max_steps"] + T.DEFAULTS["refine"]
    ops.trace_collect(cam_d, (W, H), state, pts)
    nh = int(view["counts"][2].item())
    hits = host(view["lists"][2][:nh]).astype(np.int64)
    hp = host(pts[:nh])
    shaded = ops.trace_shade(cam_d, (W, H), state, g.put(T.sphere(hp)), g.put(np.ascontiguousarray(T.sphere_grad(hp))), nh)
    for k, t in shaded.items():
        out[k] = host(t)
    # (the lists are filled through an integer atomic counter: their ORDER is not part of the result, the sets are)
    out["hits"], out["iterations"] = np.sort(hits), np.int64([it])
    for name in names:
        out["state " + name] = host(view[name])

    def verify(r):
        ref_hits = T.collect(ref)
        assert np.array_equal(r["hits"], ref_hits) and 0 < ref_hits.size < n
        rhp = T.points(ref["org"], ref["dir"], ref["t"], ref_hits)
        want = T.shade(ref, ref_hits, T.sphere(rhp), T.sphere_grad(rhp))
        for key in ("rgba", "depth", "normal", "residual", "status"):
            assert same_bits(r[key].reshape(want[key].shape), want[key]), key
    return out, verify


# =====================================================================================================================
# training: the backward building blocks, the two steps, the batch assembly
# =====================================================================================================================
@scenario("train_kernels", ["disn_dense_backward", "disn_conv3x3_backward", "disn_maxpool2x2_backward",
                            "disn_resize_bilinear_backward", "disn_gather_backward", "disn_adam_update",
                            "disn_get_loss"],
          tolerance_only=("dmap",))
def _train_kernels(g):
    import torch.nn.functional as Fnn
    from oracle import train_oracle as T
    ops, O, out, refs = _ops(), _O(), {}, {}
    wd = 1e-3
    t64 = lambda a, grad=False: torch.tensor(a, dtype=torch.float64, requires_grad=grad)

    # dense layer, M = 777 (ragged), K = 1472, N = 512
    M, K, N = 777, 1472, 512
    rng = np.random.default_rng(M + K + N)
    a = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((K, N)) / math.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    dy = rng.standard_normal((M, N)).astype(np.float32)

    def dense_ref():
        at, wt, bt = t64(a, True), t64(w, True), t64(b, True)
        y = torch.relu(at @ wt + bt)
        (y * t64(dy)).sum().backward()
        y32 = np.where(y.detach().numpy() > 0, np.maximum(y.detach().numpy().astype(np.float32), 1e-30), 0.0)
        return f32(y32), at.grad.numpy(), wt.grad.numpy() + wd * w.astype(np.float64), bt.grad.numpy()
    y32, *refs["dense"] = cached("dense_bwd_ref", dense_ref)
    da, dw, db = ops.dense_backward(g.put(a), g.put(w), g.put(y32), g.put(dy, freeze=False), wd=wd)    # dy: masked in place
    out["dense da"], out["dense dw"], out["dense db"] = host(da), host(dw), host(db)

    # 3x3 convolution: conv1_1's shape without a data gradient, and 64 -> 128 at 14 x 14
    for B, H, Cin, Cout in ((3, 20, 3, 64), (2, 14, 64, 128)):
        rng = np.random.default_rng(B * 1000 + H + Cin)
        x = rng.standard_normal((B, H, H, Cin)).astype(np.float32)
        w = (rng.standard_normal((3, 3, Cin, Cout)) / math.sqrt(9 * Cin)).astype(np.float32)
        b = (0.1 * rng.standard_normal(Cout)).astype(np.float32)
        dy = rng.standard_normal((B, H, H, Cout)).astype(np.float32)

        def conv_ref():
            xt, wt, bt = t64(x, True), t64(w, True), t64(b, True)
            y = torch.relu(Fnn.conv2d(xt.permute(0, 3, 1, 2), wt.permute(3, 2, 0, 1), bt, padding=1).permute(0, 2, 3, 1))
            (y * t64(dy)).sum().backward()
            y32 = np.where(y.detach().numpy() > 0, np.maximum(y.detach().numpy().astype(np.float32), 1e-30), 0.0)
            return f32(y32), xt.grad.numpy(), wt.grad.numpy() + wd * w.astype(np.float64), bt.grad.numpy()
        y32, *refs["conv", Cin] = cached(("conv_bwd_ref", Cin), conv_ref)
        dx, dw, db = ops.conv3x3_backward(g.put(x), g.put(w), g.put(y32), g.put(dy, freeze=False), wd=wd,
                                          need_dx=Cin != 3)
        if Cin != 3:
            out["conv%d dx" % Cin] = host(dx)
        out["conv%d dw" % Cin], out["conv%d db" % Cin] = host(dw), host(db)

    # max pool
    rng = np.random.default_rng(5)
    xp = np.maximum(rng.standard_normal((2, 6, 10, 8)), 0).astype(np.float32)
    dyp = rng.standard_normal((2, 3, 5, 8)).astype(np.float32)
    out["pool dx"] = host(ops.maxpool2x2_backward(g.put(xp), g.put(dyp)))

    # resize: plain, and a channel slice of a wider gradient accumulated into a pre-filled destination
    for hin, c, coff, cs in ((28, 4, 0, 4), (56, 8, 4, 16)):
        rng = np.random.default_rng(hin + c)
        dout = rng.standard_normal((2, 137, 137, cs)).astype(np.float32)
        base = rng.standard_normal((2, hin, hin, c)).astype(np.float32)

        def resize_ref():
            xt = torch.zeros((2, hin, hin, c), dtype=torch.float64, requires_grad=True)
            (T._resize_legacy(xt, 137, 137) * t64(dout[..., coff:coff + c])).sum().backward()
            return xt.grad.numpy()
        refs["resize", hin] = (cached(("resize_bwd_ref", hin), resize_ref), base)
        dd = g.put(dout)
        out["resize%d" % hin] = host(ops.resize_bilinear_backward(dd, hin, hin, channels=c, out_coff=coff))
        acc = g.put(base, freeze=False)
        ops.resize_bilinear_backward(dd, hin, hin, channels=c, out_coff=coff, din=acc, accumulate=True)
        out["resize%d acc" % hin] = host(acc)

    # gather, B = 1: float atomics into the map (compared by tolerance only)
    rng = np.random.default_rng(9)
    Ng = 300
    xy = rng.uniform(-2.0, 139.0, (1, Ng, 2)).astype(np.float32)
    xy[0, :8] = [[0, 0], [136, 136], [136.5, 3], [-0.5, 7], [5, 136.9], [-1, 5], [137, 5], [20, 20]]
    xy[0, 100:140] = xy[0, 140:141]                     # many points on one pixel: the atomics must accumulate
    dfeat = rng.standard_normal((1, Ng, 1472)).astype(np.float32)

    def gather_ref():
        mt = torch.zeros((1, 137, 137, 1472), dtype=torch.float64, requires_grad=True)
        (T._resampler(mt, xy) * t64(dfeat)).sum().backward()
        return mt.grad.numpy()
    refs["dmap"] = cached("gather_bwd_ref", gather_ref)
    out["dmap"] = host(ops.gather_backward(g.put(dfeat), g.put(xy)))

    # Adam on 1004 floats (the entry takes multiples of four): three whole blocks of 256 and a ragged one
    rng = np.random.default_rng(11)
    n = 1004
    aw, am = rng.standard_normal(n).astype(np.float32), (0.1 * rng.standard_normal(n)).astype(np.float32)
    av, ag = (0.01 * rng.random(n)).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    t, lr = 7, 1e-4
    dwt, dm, dv = g.put(aw, freeze=False), g.put(am, freeze=False), g.put(av, freeze=False)
    ops.adam_update(dwt, g.put(ag), dm, dv, lr * math.sqrt(1 - 0.999 ** t) / (1 - 0.5 ** t), grad_scale=0.5)
    out["adam w"], out["adam m"], out["adam v"] = host(dwt), host(dm), host(dv)

    # get_loss
    rng = np.random.default_rng(1)
    pred = rng.standard_normal((3, 257)).astype(np.float32)
    gt = (rng.standard_normal((3, 257)) * 0.05).astype(np.float32)
    out["loss"] = host(ops.get_loss(g.put(pred), g.put(gt), 10.0, 4.0, regularization=0.25))

    def verify(r):
        for k, ref in zip(("da", "dw", "db"), refs["dense"]):
            rel_close("dense " + k, r["dense " + k], ref, 2e-6)
        for Cin in (3, 64):
            dxr, dwr, dbr = refs["conv", Cin]
            if Cin != 3:
                rel_close("conv dx", r["conv%d dx" % Cin], dxr, 2e-6)
            rel_close("conv dw", r["conv%d dw" % Cin], dwr, 2e-6)
            rel_close("conv db", r["conv%d db" % Cin], dbr, 2e-6)
        xt = t64(xp, True)
        (Fnn.max_pool2d(xt.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1) * t64(dyp)).sum().backward()
        nz = xp > 0
        assert np.array_equal(r["pool dx"][nz], xt.grad.numpy()[nz].astype(np.float32))
        assert np.array_equal(r["pool dx"].reshape(2, 3, 2, 5, 2, 8).sum((2, 4)), dyp)
        for hin in (28, 56):
            ref, base = refs["resize", hin]
            rel_close("din", r["resize%d" % hin], ref, 1e-6)
            rel_close("din+=", r["resize%d acc" % hin], ref + base, 1e-6)
        rel_close("dfeatmap", r["dmap"], refs["dmap"], 1e-6)
        w2, m2, v2 = T.adam_step(aw.astype(np.float64), 0.5 * ag.astype(np.float64), am.astype(np.float64),
                                 av.astype(np.float64), t, lr)
        close("m", r["adam m"], m2, atol=1e-7)
        close("v", r["adam v"], v2, atol=1e-7)
        close("w", r["adam w"], w2, atol=1e-7, rtol=1e-6)
        want = O.get_loss(pred, gt)
        for i, nm in enumerate(("accuracy", "sdf_loss_realvalue", "sdf_loss")):
            assert abs(float(r["loss"][i]) - want[nm]) <= 1e-4 * max(1.0, abs(want[nm])), nm
        assert float(r["loss"][3]) == 0.25
        assert abs(float(r["loss"][4]) - (want["sdf_loss"] + 0.25)) <= 1e-4 * max(1.0, want["sdf_loss"])
    return out, verify


def _in_variables(flat):
    """True for the floats of a flat parameter / gradient buffer that belong to a variable (the layout pads between
    variables; the steps write the variables' gradients, never the padding)"""
    m = np.zeros(flat.total, bool)
    for name in flat.index:
        o, c = flat._span(name)
        m[o:o + c] = True
    return m


def _train_feed(B, N, seed):
    O = _O()
    feed = O.synth_inputs(seed=seed, batch=B, n_points=N)
    rng = np.random.default_rng(seed + 1)
    feed["sample_pc_rot"] = (feed["sample_pc"] @ np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], np.float32)).astype(np.float32)
    feed["sdf"] = (0.05 * rng.standard_normal((B, N, 1))).astype(np.float32)
    return feed


@scenario("train_step", ["disn_train_step"], tolerance_only=("grads_vgg",))
def _train_step(g):
    """the ``small_step`` inputs of test_gpu_train.py (B = 2, N = 256, He weights of seed 3); the gradient buffer is
    poisoned before the step: the step writes every gradient, it does not add to what was there"""
    from disn_amd.train_sdf import LOSS_NAMES, Trainer
    from disn_amd.weights import WeightStore
    from oracle import train_oracle as T
    O = _O()
    weights = cached("train_weights", lambda: O.init_weights(3, "he"))
    feed = _train_feed(2, 256, 21)
    ref = cached("train_ref", lambda: T.loss_and_grads(feed, weights, np.float64))
    tr = Trainer(WeightStore(weights), batch_size=2)
    g.frozen(tr.params)
    g.poison(tr.grads)
    pred, losses = tr.forward_backward({k: g.put(feed[k]) for k in ("imgs", "trans_mat", "sample_pc", "sample_pc_rot", "sdf")})
    o = int(tr.flat.layout.offset[32])
    grads, flat = host(tr.grads), tr.flat
    tr.close()
    var = _in_variables(flat)
    out = {"pred": host(pred), "losses": host(losses), "grads_vgg": grads[:o][var[:o]], "grads_mlp": grads[o:][var[o:]]}

    def verify(r):
        L, ref_grads, ref_pred = ref
        close("pred", r["pred"], ref_pred.reshape(r["pred"].shape), atol=2e-5, rtol=1e-5)
        for i, n in enumerate(LOSS_NAMES):
            assert abs(r["losses"][i] - L[n]) <= 1e-5 * max(abs(L[n]), 1.0) + 1e-6, (n, r["losses"][i], L[n])
        whole = np.zeros(flat.total, np.float32)
        whole[var] = np.concatenate([r["grads_vgg"], r["grads_mlp"]])
        got = flat.to_arrays(torch.from_numpy(whole))
        rows = []
        for name, rg in ref_grads.items():               # flip-tolerant, as test_train_step_gradients
            a, b = got[name].astype(np.float64).ravel(), np.asarray(rg, np.float64).ravel()
            rows.append((float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)),
                         float(a @ b / max(np.linalg.norm(a) * np.linalg.norm(b), 1e-30)), name))
        rows.sort(reverse=True)
        assert rows[0][0] < 2e-2 and min(c for _, c, _ in rows) > 0.9995, rows[:6]
    return out, verify


def _cam_head_weights(seed):
    from oracle import cam_oracle as CO
    w = CO.init_weights(seed)
    w["cameraprediction/scale/fc3/weights"] *= 0.05
    w["cameraprediction/scale/fc3/biases"][:] = 1.0
    w["cameraprediction/translation/fc3/weights"] *= 0.05
    w["cameraprediction/translation/fc3/biases"][:] = 0.0
    return w


@scenario("cam", ["disn_cam_head", "disn_cam_loss_backward", "disn_cam_train_step"])
def _cam(g):
    """the head alone at the smallest case of test_gpu_cam_train.py (B = 4, N = 2048), then its ``step_case``"""
    import cam_train_reference as R
    from disn_amd import posenet
    from disn_amd.train_cam import LOSS_NAMES, CamTrainer
    ops, O, out = _ops(), _O(), {}
    w = _cam_head_weights(5)
    rng = np.random.default_rng(7)
    B, N = 4, 2048
    RT, tm = R.synth_camera(rng, B)
    emb = rng.standard_normal((B, 1024)).astype(np.float32)
    pts = ((rng.random((B, N, 3)) - 0.5) * 0.9).astype(np.float32)
    head = posenet.CameraHead(w)
    embd = g.put(emb)
    res = ops.cam_loss_backward(head.w, embd, g.put(pts), g.put(RT), g.put(tm), "ALL")
    for k, v in res.items():
        out["head " + k] = host(v)
    out["cam_head"] = host(head.run(embd)[3])
    head_ref = cached("cam_head_ref", lambda: R.head_loss_and_grads(emb, w, pts, RT, tm, "ALL"))
    # the whole step
    weights = cached("cam_weights", lambda: dict([(k, v) for k, v in O.init_weights(3, "he").items() if k.startswith("vgg_16/")]
                                                + list(_cam_head_weights(11).items())))
    feed = cached("cam_feed", lambda: R.synth_feed(21, 2, 256))
    step_ref = cached("cam_step_ref", lambda: R.loss_and_grads(feed, weights, "3D"))
    tr = CamTrainer(weights, batch_size=2, loss_mode="3D", precision="f32")
    g.frozen(tr.params)
    g.poison(tr.grads)
    tmat, losses, dists = tr.forward_backward({k: g.put(feed[k]) for k in ("imgs", "sample_pc", "RT", "trans_mat")})
    flat = tr.flat
    var = _in_variables(flat)
    out["step tm"], out["step losses"], out["step dists"], out["step grads"] = host(tmat), host(losses), host(dists), host(tr.grads)[var]
    tr.close()

    def verify(r):
        ref, gr, ptm = head_ref
        for i, n in enumerate(("rotpc_loss", "rot2d_loss", "rotmatrix_loss", "rot2d_dist", "rot3d_dist")):
            assert abs(r["head losses"][i] - ref[n]) <= 1e-5 * abs(ref[n]) + 1e-12, n
        assert r["head losses"][5] == 0.0
        assert abs(r["head losses"][6] - ref["overall_loss"]) <= 1e-5 * abs(ref["overall_loss"])
        close("rot2d_dist_all", r["head dists"][0], ref["rot2d_dist_all"], atol=0, rtol=1e-5)
        close("rot3d_dist_all", r["head dists"][1], ref["rot3d_dist_all"], atol=0, rtol=1e-5)
        close("pred_trans_mat", r["head pred_trans_mat"], ptm, atol=1e-5 * np.abs(ptm).max())
        near = lambda name, a, b: close(name, a, b, atol=1e-5 * max(float(np.abs(b).max()), 1e-30))
        near("dRT", r["head dRT"], gr["pred_RT"])
        near("demb", r["head demb"], gr["embedding"])
        L = ops.cam_param_layout()
        for j, (name, shp) in enumerate(posenet.variable_shapes().items()):
            o = int(L.offset[32 + j] - L.offset[32])
            near(name, r["head head_grads"][o:o + int(L.count[32 + j])].reshape(shp), gr[name])
        assert same_bits(r["cam_head"], r["head pred_trans_mat"])      # the training forward is the inference head
        sref, sgrads, stm = step_ref
        w3, w2, wm = R.mode_weights("3D")
        for i, n in enumerate(LOSS_NAMES):
            want = (w2 * sref["rot2d_loss"] + w3 * sref["rotpc_loss"] + wm * sref["rotmatrix_loss"]
                    + sref["regularization"]) if n == "overall_loss" else sref[n]
            assert abs(r["step losses"][i] - want) <= 1e-5 * abs(want) + 1e-9, (n, r["step losses"][i], want)
        close("rot3d_dist_all", r["step dists"][1], sref["rot3d_dist_all"], atol=0, rtol=1e-5)
        close("pred_trans_mat", r["step tm"], stm, atol=1e-5 * np.abs(r["step tm"]).max())
        whole = np.zeros(flat.total, np.float32)
        whole[var] = r["step grads"]
        got = flat.to_arrays(torch.from_numpy(whole))
        rows = []
        for name, rg in sgrads.items():
            a, b = got[name].astype(np.float64).ravel(), np.asarray(rg, np.float64).ravel()
            rows.append((float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)),
                         float(a @ b / max(np.linalg.norm(a) * np.linalg.norm(b), 1e-30)), name))
        rows.sort(reverse=True)
        assert rows[0][0] < 2e-2 and min(c for _, c, _ in rows) > 0.9995, rows[:6]
    return out, verify


@scenario("assemble_batch", ["disn_assemble_batch"])
def _assemble_batch(g):
    import tempfile
    import train_driver_fixtures as TF
    from disn_amd import data_resident as R

    def tree():
        with tempfile.TemporaryDirectory(prefix="disn_memory_contract_") as root:     # the set holds everything in memory
            info, listinfo = TF.write_tree(root, TF.SMALL_OBJECTS, views=(0, 3, 7), seed=5)
            return R.ResidentSet.from_tree(listinfo, info, workers=4)
    host_set = cached("resident_host", tree)
    rset = host_set.to("cuda:0")                        # the device copies are allocated under the guards
    g.frozen(*[t for t in rset._dev.values() if isinstance(t, torch.Tensor)])
    plan = R.PlanStream(rset, 7, 1, 77, seed=3).work(0)
    out = {k: host(v) for k, v in rset.assemble(plan, rot=True, backcolorwhite=True).items()}
    rset.raise_on_flags()
    want = rset.host_batch(plan, rot=True, backcolorwhite=True)

    def verify(r):
        assert np.array_equal(r["imgs"], want["img"]) and np.array_equal(r["sample_pc"], want["sdf_pt"])
        assert np.array_equal(r["sdf"], want["sdf_val"] - np.float32(0.003)) and r["sdf"].shape == (7, 77, 1)
        assert np.array_equal(r["trans_mat"], want["trans_mat"])
        p = want["sdf_pt"].astype(np.float64)
        Rm = np.stack([np.asarray(rset.obj_rot_mat[e]) for e in plan.entries]).astype(np.float64)
        u = 2.0 ** -24
        bound = 2 * (3 * u / (1 - 3 * u)) * np.einsum("bsk,bkj->bsj", np.abs(p), np.abs(Rm))
        assert (np.abs(r["sample_pc_rot"].astype(np.float64) - want["sdf_pt_rot"].astype(np.float64)) <= bound).all()
    return out, verify


# =====================================================================================================================
# weight images and host-side helpers
# =====================================================================================================================
@scenario("packers", ["disn_mlp_fused_pack", "disn_mlp_fused_feat_pack", "disn_equalise_weights", "disn_crc32c",
                      "disn_mesh_components", "disn_write_obj", "disn_write_obj_normals", "disn_read_obj_verts",
                      "disn_read_obj_mesh", "disn_mesh_bvh_build", "disn_mesh_bvh_build_order"])
def _packers(g):
    import tempfile
    import fused_emulation as E
    import mesh_clean_fixtures as MF
    from disn_amd import isosurface, mesh_sdf, postprocess, tf_checkpoint
    from disn_amd._lib import lib
    ops, out = _ops(), {}
    store = _store()
    W = lambda scope, l: f32(store["%s/%s/weights" % (scope, l)][0, 0])
    ws = (W("sdfprediction", "fold1/conv2"), W("sdfprediction", "fold1/conv3"), W("sdfprediction", "fold2/conv1")[:512],
          W("sdfprediction", "fold2/conv2"))
    out["fused"] = host(ops.mlp_fused_pack(*[g.put(w) for w in ws]))
    lw = tuple(W("sdfprediction_imgfeat", l) for l in ("fold1/conv2", "fold1/conv3", "fold2/conv1", "fold2/conv2"))
    out["feat"] = host(ops.mlp_fused_feat_pack(*[g.put(w) for w in lw]))
    # host-side entries: they take host pointers and launch nothing; run here so that the table covers the header
    eq, tap_scale, span = store.equalised()
    out["tap_scale"] = f32(tap_scale)
    data = bytes(range(256)) * 64
    out["crc"] = np.uint32([lib().disn_crc32c(data, len(data), 0), lib().disn_crc32c(b"123456789", 9, 0)])
    v, f = MF.fans()
    labels, counts = postprocess.separate_mesh(v, f, "face")
    out["labels"], out["counts"] = labels, counts
    with tempfile.TemporaryDirectory(prefix="disn_memory_contract_") as d:
        isosurface.write_obj(os.path.join(d, "a.obj"), v, f)
        isosurface.write_obj(os.path.join(d, "n.obj"), v, f, normals=np.ones_like(v))
        out["obj_verts"] = isosurface.read_obj_verts(os.path.join(d, "a.obj"))
        rv, rf = mesh_sdf.read_obj_mesh(os.path.join(d, "n.obj"))
        out["obj_v"], out["obj_f"] = rv, rf
    out["bvh"], out["bvh_order"] = mesh_sdf.build_bvh_host_order(v, f)
    plain = np.empty(out["bvh"].size, np.uint8)         # no wrapper: the image alone
    assert lib().disn_mesh_bvh_build(v.ctypes.data, v.shape[0], f.ctypes.data, f.shape[0], plain.ctypes.data, plain.size) == 0
    out["bvh_plain"] = plain

    def verify(r):
        ref_img, ref_meta = E.pack_image(*ws)
        nb = E.PAIRS * 2048
        meta = r["fused"][nb:nb + 4 * E.META].view(np.float32)
        assert np.array_equal(meta[64:], ref_meta[64:])
        np.testing.assert_allclose(meta[8:10], ref_meta[8:10], rtol=1e-5)
        assert np.array_equal(r["fused"][:nb].view(np.uint16).reshape(E.PAIRS, 2, 64, 8), ref_img.view(np.uint16))
        ref_img, ref_meta = E.pack_image(*lw)
        nb = E.PAIRS_FEAT * 2048
        meta = r["feat"][nb:nb + 4 * E.META].view(np.float32)
        assert np.array_equal(meta[64:], ref_meta[64:]) and meta[11] == ref_meta[11]
        np.testing.assert_allclose(meta[8:11], ref_meta[8:11], rtol=1e-5)
        assert np.array_equal(r["feat"][:nb].view(np.uint16).reshape(E.PAIRS_FEAT, 2, 64, 8), ref_img.view(np.uint16))
        assert r["crc"][1] == 0xE3069283                 # the CRC-32C check value
        assert r["labels"].tolist() == [0, 0, 1, 1] and r["counts"].tolist() == [4, 4]
        assert same_bits(r["bvh"], r["bvh_plain"]) and sorted(r["bvh_order"].tolist()) == [0, 1, 2, 3]
        assert np.array_equal(r["obj_verts"], v) and np.array_equal(r["obj_v"], v) and np.array_equal(r["obj_f"], f)
        m = np.log2(r["tap_scale"])
        assert np.array_equal(m, np.round(m))            # powers of two
    return out, verify


EXEMPT.update({
    "disn_abi_version": "returns a constant",
    "disn_pack_kn_x3_bytes": "size query: host arithmetic",
    "disn_pack_conv_h2_bytes": "size query: host arithmetic",
    "disn_pack_dense_h2_bytes": "size query: host arithmetic",
    "disn_mlp_fused_image_bytes": "size query: host arithmetic",
    "disn_mlp_fused_feat_image_bytes": "size query: host arithmetic",
    "disn_mesh_bvh_bytes": "size query: host arithmetic",
    "disn_trace_state_bytes": "size query: host arithmetic",
    "disn_voxel_grid_words": "size query: host arithmetic",
    "disn_conv3x3_h2_plan": "kernel selection on the host: needs no device",
    "disn_param_layout": "fills a host struct",
    "disn_cam_param_layout": "fills a host struct",
    "disn_stream_create": "creates a stream: writes no device memory",
    "disn_stream_destroy": "destroys a stream: writes no device memory",
    "disn_ctx_create": "creates a stream and events: writes no device memory",
    "disn_ctx_destroy": "destroys a context: writes no device memory",
    "disn_ctx_pipeline": "stores two event handles in the host context",
})
EXEMPT.update({name: "workspace size query: host arithmetic" for name in (
    "disn_conv3x3_x3_workspace_bytes", "disn_conv1_1_workspace_bytes", "disn_conv3x3_h2_workspace_bytes",
    "disn_vgg16_workspace_bytes", "disn_conv3x3_workspace_bytes", "disn_conv3x3_planned_workspace_bytes",
    "disn_fc_workspace_bytes", "disn_dense_h2_workspace_bytes", "disn_dense_workspace_bytes",
    "disn_query_taps_fused_workspace_bytes", "disn_query_fused_workspace_bytes", "disn_query_grid_fused_workspace_bytes",
    "disn_query_grid_listed_workspace_bytes", "disn_grid_band_select_workspace_bytes", "disn_sdf_mlp_workspace_bytes",
    "disn_query_workspace_bytes", "disn_encode_workspace_bytes", "disn_encode_query_workspace_bytes",
    "disn_query_grid_ctx_workspace_bytes", "disn_dense_bf16_workspace_bytes", "disn_conv3x3_bf16_workspace_bytes",
    "disn_cam_train_workspace_bytes", "disn_cam_loss_backward_workspace_bytes", "disn_train_workspace_bytes",
    "disn_dense_backward_workspace_bytes", "disn_conv3x3_backward_workspace_bytes",
    "disn_resize_bilinear_backward_workspace_bytes", "disn_mc_workspace_bytes", "disn_mc_batch_workspace_bytes",
    "disn_mesh_sign_workspace_bytes", "disn_voxel_surface_workspace_bytes", "disn_voxel_fill_workspace_bytes",
    "disn_metrics_workspace_bytes", "disn_query_grid_workspace_bytes", "disn_fold_local_workspace_bytes",
    "disn_query_views_workspace_bytes", "disn_query_grid_views_workspace_bytes", "disn_query_grad_workspace_bytes",
    "disn_mesh_clean_workspace_bytes", "disn_mesh_simplify_workspace_bytes", "disn_mesh_colour_workspace_bytes",
    "disn_mesh_sample_workspace_bytes", "disn_mesh_smooth_workspace_bytes")})
EXEMPT["disn_write_obj_colours"] = "host file writer: reads host arrays, no device work"

# The launching entries of the mesh modules' own headers (include/disn_amd_{simplify,colour,sample,smooth}.h) run under
# guards in their own files, not in a scenario here: entry -> file::test.  tests/test_guarded_alloc_host.py checks that
# the test exists, that the file's NEW tuple lists the entry and that the test asserts set(NEW) <= set(called).
MESH_MODULE_COVERAGE = {
    "disn_mesh_simplify_count_batch": "test_gpu_mesh_simplify.py::test_memory_contract_of_the_simplify_entries",
    "disn_mesh_simplify_emit_batch": "test_gpu_mesh_simplify.py::test_memory_contract_of_the_simplify_entries",
    "disn_mesh_zbuffer_batch": "test_gpu_mesh_colour.py::test_memory_contract_of_the_colour_entries",
    "disn_mesh_colour_batch": "test_gpu_mesh_colour.py::test_memory_contract_of_the_colour_entries",
    "disn_mesh_sample_batch": "test_gpu_mesh_sample.py::test_memory_contract_of_both_entries",
    "disn_mesh_smooth_batch": "test_gpu_mesh_smooth.py::test_memory_contract_of_the_smooth_entries",
}


# =====================================================================================================================
# the test
# =====================================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_memory_contract(name):
    fn = SCENARIOS[name]
    results, verify = {}, None
    for variant in ("A", "B"):
        with guarded(variant) as g:
            with g.recording() as called:
                out, check_reference = fn(g)
            g.check()                                              # (a) guards and const inputs
        missing = sorted(set(ENTRY_COVERAGE[name]) - set(called))
        assert not missing, "variant %s: the scenario never called %s" % (variant, missing)      # (d)
        results[variant] = out
        verify = verify or check_reference
    a, b = results["A"], results["B"]
    assert sorted(a) == sorted(b)
    excused = set(TOLERANCE_ONLY.get(name, ()))
    differ = [k for k in a if k not in excused and not same_bits(a[k], b[k])]                   # (b)
    assert not differ, "results depend on what the buffers held before, or on memory outside them: %s" % [
        (k, int((np.ascontiguousarray(a[k]).view(np.uint8) != np.ascontiguousarray(b[k]).view(np.uint8)).sum())
         if a[k].shape == b[k].shape else "shape") for k in differ]
    verify(a)                                                      # (c) the entry's own reference and tolerance
    for k in excused:                                              # float atomics: run B within the tolerance too
        assert a[k].shape == b[k].shape
    if excused:
        verify(b)

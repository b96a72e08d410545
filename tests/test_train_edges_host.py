"""The tables of train_edge_shapes.py still reach the code paths they were chosen for (CPU; no GPU needed).

gemm_tn_launch's selection (csrc/gemm_tn_mfma.hip: tile form, stream-K split) is restated here in a few lines; if someone
edits a shape of the tables -- or the rule, then this restatement with it -- a named path cannot silently drop out of
test_gpu_train_edges.py."""
import os
import re

import train_edge_shapes as S

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "disn_amd", "csrc")
K_TN_MAX_W = 512           # kTnMaxW
INTERLEAVE_FROM_TILES = 18


def tn_plan(M, P, Q, mode):
    """gemm_tn_launch + tn_launch_tile: mode 0 f32-input MFMA, 1 bf16, 2 two-term f16 (the last two stage transposed)"""
    p128, q128 = P % 128 == 0, Q % 128 == 0
    if mode == 1 and not (p128 and q128):
        mode = 0                                       # the bf16 form exists with the 128 x 128 tile only
    bp, bq = 128 if p128 else 64, 128 if q128 else 64
    T, msteps = (P // bp) * (Q // bq), (M + 31) // 32
    units = T * msteps
    plan = dict(mode=mode, tile=(bp, bq), T=T, msteps=msteps, units=units, W=min(units, K_TN_MAX_W), kt=0, clamped=False)
    if mode != 0 and T >= INTERLEAVE_FROM_TILES:
        kt = K_TN_MAX_W // T
        clamped = kt > msteps
        kt = max(min(kt, msteps), 1)
        if T * kt <= 2 * K_TN_MAX_W:                    # the slab capacity
            plan.update(kt=kt, W=T * kt, clamped=clamped)
    return plan


def all_plans():
    out = []
    for shape in S.CONV_SHAPES + S.CONV_C3_SHAPES:
        for mode in S.MODES:
            M, P, Q, m, conv = S.conv_tn_problem(shape, mode)
            out.append(dict(tn_plan(M, P, Q, m), M=M, conv=conv, shape=shape, entry="conv"))
    for shape in S.DENSE_SHAPES:
        for mode in S.MODES:
            M, P, Q, m, conv = S.dense_tn_problem(shape, mode)
            out.append(dict(tn_plan(M, P, Q, m), M=M, conv=conv, shape=shape, entry="dense"))
    return out


def where(plans, **eq):
    return [p for p in plans if all(p[k] == v for k, v in eq.items())]


def _source_int(text, pattern, what):
    m = re.search(pattern, text)
    assert m is not None, "%s: pattern %r no longer matches the source; restate the rule here as the source now has it" % (
        what, pattern)
    return int(m.group(1))


def test_the_restated_constants_are_the_sources():
    """a tripwire on the source text: a reformat turns it red with the message above, and the restatement is re-read"""
    tn = open(os.path.join(CSRC, "gemm_tn_mfma.hip")).read()
    assert _source_int(tn, r"kTnMaxW\s*=\s*(\d+)", "gemm_tn_mfma.hip kTnMaxW") == K_TN_MAX_W
    assert _source_int(tn, r"p\.bf16\s*!=\s*0\s*&&\s*T\s*>=\s*(\d+)", "tn_launch_tile's interleaving rule") == INTERLEAVE_FROM_TILES
    assert _source_int(tn, r"\(long\)T\s*\*\s*kt\s*<=\s*(\d+)\s*\*\s*kTnMaxW", "tn_launch_tile's slab capacity") == 2
    hpp = open(os.path.join(CSRC, "kernels.hpp")).read()
    assert _source_int(hpp, r"kConvWideMinImages\s*=\s*(\d+)", "kernels.hpp kConvWideMinImages") == S.CONV_BATCHED_FROM
    img = open(os.path.join(CSRC, "backward_img.hip")).read()
    assert _source_int(img, r"Hout\s*<\s*(\d+)\s*\*\s*Hin\s*\|\|\s*Wout\s*<\s*\1\s*\*\s*Win", "resize_bwd_ws_bytes' threshold") == 2


def test_every_tile_form_in_every_mode_that_can_run_it():
    plans = all_plans()
    forms = {(128, 128), (128, 64), (64, 128), (64, 64)}
    assert {p["tile"] for p in where(plans, mode=0)} == forms
    assert {p["tile"] for p in where(plans, mode=1)} == {(128, 128)}
    assert {p["tile"] for p in where(plans, mode=2)} == forms
    # ... with implicit im2col, where the loader's tap validity matters
    assert {p["tile"] for p in where(plans, mode=2, conv=True)} == forms
    assert where(plans, mode=1, conv=True) and where(plans, mode=1, conv=False)


def test_the_table_quotes_the_plan_of_each_conv_shape():
    """the comments of CONV_SHAPES, as numbers"""
    def plan(shape, mode):
        return tn_plan(*S.conv_tn_problem(shape, mode)[:4])
    assert plan((1, 1, 1, 64, 64), 2)["tile"] == (64, 64) and plan((1, 1, 1, 64, 64), 2)["units"] == 9
    assert plan((1, 1, 7, 128, 64), 2)["tile"] == (128, 64) and plan((1, 1, 7, 128, 64), 1)["mode"] == 0
    assert plan((1, 7, 1, 64, 128), 2)["tile"] == (64, 128)
    for mode in S.MODES:
        p = plan((1, 7, 5, 128, 128), mode)
        assert p["tile"] == (128, 128) and p["T"] == 9 and p["kt"] == 0 and p["mode"] == mode
    for mode in (1, 2):
        p = plan((3, 3, 3, 128, 256), mode)
        assert p["T"] == 18 and p["msteps"] == 1 and p["kt"] == 1 and p["clamped"]
        p = plan((5, 9, 11, 128, 256), mode)
        assert p["msteps"] == 16 and p["kt"] == 16 and p["clamped"] and p["W"] == 288
    p = plan((4, 13, 6, 192, 192), 2)
    assert p["tile"] == (64, 64) and p["T"] == 81 and p["kt"] == 6 and not p["clamped"]
    assert plan((4, 13, 6, 192, 192), 1)["mode"] == 0
    p = plan((2, 33, 31, 64, 64), 0)
    assert p["units"] == 576 and p["T"] == 9 and p["kt"] == 0
    p = plan((1, 2, 2, 512, 512), 2)
    assert p["T"] == 144 and p["msteps"] == 1 and p["kt"] == 1


def test_stream_k_bookkeeping_paths():
    plans = all_plans()
    for mode in (0, 2):                                 # one row step only (M < 32), contiguous and interleaved
        assert any(p["msteps"] == 1 and p["kt"] == 0 and p["units"] < K_TN_MAX_W for p in where(plans, mode=mode))
    for mode in (1, 2):
        assert any(p["kt"] > 0 and p["clamped"] and p["msteps"] == 1 for p in where(plans, mode=mode))
        assert any(p["kt"] > 1 and p["clamped"] for p in where(plans, mode=mode))
    # interleaved in a tile form other than 128 x 128, with several slabs per tile
    assert any(p["kt"] > 1 and p["tile"] != (128, 128) for p in where(plans, mode=2))
    # the slab capacity: exactly full, and exceeded (back to the contiguous split)
    assert any(p["kt"] > 0 and p["T"] * p["kt"] == 2 * K_TN_MAX_W and p["tile"] == (128, 128) for p in plans)
    assert any(p["mode"] != 0 and p["T"] > 2 * K_TN_MAX_W and p["kt"] == 0 for p in plans)
    # contiguous segments that cross tile boundaries: more units than workgroups, too few tiles to interleave
    for mode in (0, 2):
        assert any(p["units"] > K_TN_MAX_W and p["T"] < INTERLEAVE_FROM_TILES and p["kt"] == 0 and p["msteps"] > 1
                   for p in where(plans, mode=mode))
    assert any(p["units"] > K_TN_MAX_W and p["kt"] == 0 and p["msteps"] % 2 for p in where(plans, mode=0, entry="dense"))


def test_ragged_rows_reach_the_transposed_staging():
    plans = all_plans()
    for mode in (1, 2):
        conv = where(plans, mode=mode, conv=True)
        # an odd M: the last row has no partner inside the last 32-row step (also with more than one step)
        assert any(p["M"] % 2 == 1 and p["M"] > 32 for p in conv)
        assert any(p["M"] % 2 == 1 and p["M"] < 32 for p in conv)
        # an odd W and an odd H * W with several images: row pairs lie across image rows and across images
        assert any(p["shape"][2] % 2 and (p["shape"][1] * p["shape"][2]) % 2 and p["shape"][0] > 1 and p["shape"][2] > 1
                   for p in conv)
    assert any(p["M"] % 2 == 1 and p["M"] > 32 for p in where(plans, mode=1, conv=False))
    assert any(p["M"] % 2 == 1 for p in where(plans, mode=0, conv=False))
    # one-row and one-column images
    assert any(s[1] == 1 and s[2] > 1 for s in S.CONV_SHAPES) and any(s[2] == 1 and s[1] > 1 for s in S.CONV_SHAPES)
    assert S.CONV_ZERO_SHAPE in S.CONV_SHAPES and S.CONV_ZERO_SHAPE[0] == 3


def test_the_data_gradient_runs_on_both_sides_of_the_batched_switch():
    at = [s for s in S.CONV_SHAPES if s[0] == S.CONV_BATCHED_FROM]
    assert at and all((S.CONV_BATCHED_FROM - 1,) + s[1:] in S.CONV_SHAPES for s in at)
    assert any(s[0] > S.CONV_BATCHED_FROM for s in S.CONV_SHAPES)
    assert all(s[3] == 3 for s in S.CONV_C3_SHAPES) and {s[0] * s[1] * s[2] for s in S.CONV_C3_SHAPES} >= {1, 105, 2046}


def test_conv_h2_plan_takes_the_batched_form_from_four_samples_on():
    """the data gradient of the table's shapes is conv(dz, mirrored kernel) with the channels swapped, under the training
    step's tiling: conv_h2_plan (a host function) must pick another form than the single-image one exactly from
    CONV_BATCHED_FROM samples on -- that the B values lie on both sides of 4 is not enough"""
    import ctypes
    from disn_amd import _lib
    h = _lib.lib()
    TRAIN, STRICT = 18, 11               # kConvTilingTrain, kConvTilingStrict (the single-image forms whatever B)

    def form(tiling, B, H, W, cin, cout):
        f = h.disn_conv3x3_h2_plan(B, H, W, cin, cout, tiling, None, None)
        assert f >= 0, (tiling, B, H, W, cin, cout, f)
        return f
    seen = set()
    for B, H, W, Cin, Cout in S.CONV_SHAPES:
        batched = form(TRAIN, B, H, W, Cout, Cin) != form(STRICT, B, H, W, Cout, Cin)
        assert batched == (B >= S.CONV_BATCHED_FROM), (B, H, W, Cin, Cout)
        seen.add(batched)
    assert seen == {True, False}


def test_resize_cases_sit_on_both_sides_of_the_separable_threshold():
    def sep(n_in, n_out):
        return n_out >= 2 * n_in
    at137 = [s for s in S.RESIZE_SHAPES if s[6:] == (137, 137)]
    for axis in (1, 2):                                 # Hin, Win
        assert any(s[axis] == 137 // 2 for s in at137)          # the largest separable size
        assert any(s[axis] == 137 // 2 + 1 for s in at137)      # the first that is not
    kinds = {(sep(s[1], s[6]), sep(s[2], s[7])) for s in S.RESIZE_SHAPES}
    assert kinds == {(True, True), (True, False), (False, True), (False, False)}
    assert any(s[1] == s[6] and s[2] == s[7] for s in S.RESIZE_SHAPES)           # identity
    assert any(s[6:] != (137, 137) for s in S.RESIZE_SHAPES)
    assert all(s[3] % 4 == 0 and s[4] % 4 == 0 and s[5] % 4 == 0 and s[5] + s[3] <= s[4] for s in S.RESIZE_SHAPES)


def test_the_step_shapes_have_ragged_row_counts():
    rows = [b * n for b, n in S.STEP_SHAPES]
    assert all(r % 32 for r in rows) and any(b == 1 for b, _ in S.STEP_SHAPES)
    assert any(b % 2 and b > 1 for b, _ in S.STEP_SHAPES) and any(r % 2 for r in rows)

"""CPU test of conv_h2_plan() through disn_conv3x3_h2_plan: which convolution kernel a call runs, with which grid.

Most of the plan's choices are speed-only -- two workgroups per CU or one, the parked or the two-k-wave segmented form,
whole-image or two-row patches: siblings with the same bits, which no bit test can tell apart.  tests/conv_plan_table.json
pins them: (tiling, B, H, W, Cin, Cout) -> (form, grid, block) as the launchers chose BEFORE the plan function existed
(recorded from the parent commit's launchers with their launch calls replaced by prints; see the file's comment)."""
import ctypes
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_SHAPE = -2

# (hw, Cin, Cout) of conv1_2 .. conv5_3
LAYERS = [(224, 64, 64), (112, 64, 128), (112, 128, 128), (56, 128, 256), (56, 256, 256), (56, 256, 256),
          (28, 256, 512), (28, 512, 512), (28, 512, 512), (14, 512, 512), (14, 512, 512), (14, 512, 512)]


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(ROOT, "tests", "conv_plan_table.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def plan():
    from disn_amd import _lib
    h = _lib.lib()

    def call(tiling, B, H, W, Cin, Cout):
        g, b = ctypes.c_int(-1), ctypes.c_int(-1)
        form = h.disn_conv3x3_h2_plan(B, H, W, Cin, Cout, tiling, ctypes.byref(g), ctypes.byref(b))
        return form, g.value, b.value
    return call


def _key(r):
    return (r["tiling"], r["B"], r["H"], r["W"], r["Cin"], r["Cout"])


def test_table_names_are_the_enumerators(table):
    """the table's form names are enum ConvForm of kernels.hpp, in order (the ids the export returns)"""
    src = open(os.path.join(ROOT, "disn_amd", "csrc", "kernels.hpp")).read()
    body = re.search(r"enum ConvForm \{(.*?)\};", src, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    names = [n for n in re.findall(r"\b(CONVW?_[A-Z0-9_]+)\b\s*(?:=\s*0\s*)?,", body) if n != "CONV_FORMS"]
    assert names == table["forms"] and len(names) == 20


def test_plan_equals_the_recorded_table(table, plan):
    ids = {n: i for i, n in enumerate(table["forms"])}
    wrong = []
    for r in table["rows"]:
        got = plan(*_key(r))
        want = (E_SHAPE, -1, -1) if r["form"] is None else (ids[r["form"]], r["grid"], r["block"])
        if got != want:
            wrong.append((_key(r), want, got))
    assert not wrong, wrong[:10]


def test_table_covers_the_issue_cases(table):
    rows = {_key(r): r for r in table["rows"]}
    # the twelve 3x3 layers at every batch size, by shape / strict / the training step: 17 forms
    base = set()
    for tiling in (0, 11, 18):
        for B in (1, 2, 3, 4, 8, 12, 13, 16):
            for hw, cin, cout in LAYERS:
                base.add(rows[(tiling, B, hw, hw, cin, cout)]["form"])
    assert None not in base and len(base) == 17
    # forced rows that reach the rest
    for k in [(1, 3, 6, 8, 192, 64), (2, 3, 6, 8, 192, 64), (7, 2, 30, 44, 64, 128)]:
        assert rows[k]["form"] is not None
    assert {r["form"] for r in table["rows"]} - {None} == set(table["forms"])     # every enumerator occurs
    # two workgroups per CU: three images take them, one image their one-per-CU siblings
    occ2 = [((1, 16, 14, 128, 512), "CONV_P14_K8_OCC2", 384, "CONV_P14_K8", 128),
            ((3, 32, 28, 64, 512), "CONV_P28_N2_OCC2", 384, "CONV_P28_N2", 128),
            ((4, 64, 64, 64, 512), "CONV_P16H_N2_OCC2", 1536, "CONV_P16_N2", 256)]
    for (tiling, H, W, cin, cout), f3, g3, f1, g1 in occ2:
        r3, r1 = rows[(tiling, 3, H, W, cin, cout)], rows[(tiling, 1, H, W, cin, cout)]
        assert (r3["form"], r3["grid"]) == (f3, g3) and (r1["form"], r1["grid"]) == (f1, g1)


def test_invalid_combinations_return_e_shape(plan):
    """what disn_conv3x3_h2 rejected before the plan held the rules"""
    for tiling in (14, 15, 16, 17, -1, 20):
        for B in (1, 4):
            assert plan(tiling, B, 56, 56, 256, 256)[0] == E_SHAPE
    for tiling in (6, 8, 12):                                   # four n-waves = 128 channels per workgroup
        assert plan(tiling, 4, 56, 56, 128, 192)[0] == E_SHAPE
        assert plan(tiling, 4, 56, 56, 128, 256)[0] >= 0
    for tiling in (12, 13):                                     # two K halves of whole segments
        assert plan(tiling, 4, 56, 56, 64, 128)[0] == E_SHAPE
    for hw in ((14, 28), (28, 14), (16, 16)):                   # the whole-image tilings: at most 14 x 14
        assert plan(19, 2, hw[0], hw[1], 512, 512)[0] == E_SHAPE
        assert plan(10, 2, hw[0], hw[1], 512, 512)[0] == E_SHAPE
    assert plan(19, 2, 14, 14, 64, 64)[0] == E_SHAPE and plan(10, 2, 14, 14, 64, 64)[0] >= 0   # segments: Cin % 128
    for tiling in (5, 6, 7, 8, 9, 12, 13):                      # the batched forms: 28 x 28 pixels and more
        assert plan(tiling, 4, 14, 14, 512, 512)[0] == E_SHAPE
        assert plan(tiling, 4, 27, 28, 256, 256)[0] == E_SHAPE
        assert plan(tiling, 4, 28, 28, 256, 256)[0] >= 0
    for tiling in range(20):                                    # channel multiples of 64, whatever the tiling
        assert plan(tiling, 1, 28, 28, 96, 64)[0] == E_SHAPE and plan(tiling, 1, 28, 28, 64, 32)[0] == E_SHAPE


def test_conv3x3_h2_rejects_what_the_plan_rejects(plan):
    """disn_conv3x3_h2 answers DISN_E_SHAPE from the plan, before any device call"""
    from disn_amd import _lib
    h = _lib.lib()
    for tiling, H, W, cin, cout in [(14, 56, 56, 256, 256), (12, 56, 56, 128, 192), (19, 14, 28, 512, 512), (5, 14, 14, 512, 512)]:
        assert plan(tiling, 4, H, W, cin, cout)[0] == E_SHAPE   # first: only a shape the plan rejects goes into the call
        # host buffers as stand-ins (never touched: the shape check comes before any device call); ws_bytes = 0 would
        # stop an accepted shape at DISN_E_WS, still in front of the first launch
        buf = (ctypes.c_float * 16)()
        p = ctypes.cast(buf, ctypes.c_void_p)
        assert h.disn_conv3x3_h2(p, 4, H, W, cin, p, p, cout, 1, p, None, None, tiling, p, 0, None) == E_SHAPE

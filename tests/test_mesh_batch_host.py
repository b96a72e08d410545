"""The workspace sizes of the batched-mesh stages and of the two layouts that share their cursor are pinned:
mesh_batch_workspace_table.json holds what the queries returned from the library built at the commit BEFORE the stages'
building blocks moved to csrc/mesh_batch.hpp and the layouts to kernels.hpp's WsCursor -- recorded from that build,
never from the code under test.  A buffer lost, doubled, resized or taken in another order by a change of the layout
code shows here, without a device; so does a limit (3 nf and nv within int32, B <= 65535, S in {1, 2, 4}) that moved:
a refused batch is a 0 in the table."""
import json
import os

import pytest

from disn_amd import _lib

TABLE = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "mesh_batch_workspace_table.json")))
INT32_MAX = 2 ** 31 - 1


@pytest.mark.parametrize("stage", ["clean", "simplify"])
def test_mesh_workspace_bytes(stage):
    fn = getattr(_lib.lib(), "disn_mesh_%s_workspace_bytes" % stage)
    assert len(TABLE[stage]) == 9
    for B, nv, nf, want in TABLE[stage]:
        assert fn(B, nv, nf) == want, (B, nv, nf)


@pytest.mark.parametrize("stage", ["clean", "simplify"])
def test_mesh_workspace_limits(stage):
    fn = getattr(_lib.lib(), "disn_mesh_%s_workspace_bytes" % stage)
    assert fn(1, 3, INT32_MAX // 3) > 0 and fn(1, 3, INT32_MAX // 3 + 1) == 0
    assert fn(1, INT32_MAX, 1) > 0 and fn(1, INT32_MAX + 1, 1) == 0


def test_mesh_colour_workspace_bytes():
    fn = _lib.lib().disn_mesh_colour_workspace_bytes
    assert len(TABLE["colour"]) == 9 * 2 * 3 + 4
    for B, V, nv, nf, S, want in TABLE["colour"]:
        assert fn(B, V, nv, nf, S) == want, (B, V, nv, nf, S)


def test_mesh_colour_workspace_limits():
    fn = _lib.lib().disn_mesh_colour_workspace_bytes
    for V in (1, 4):
        for S in (1, 2, 4):
            assert fn(1, V, 3, INT32_MAX // 3, S) > 0 and fn(1, V, 3, INT32_MAX // 3 + 1, S) == 0
    assert fn(5, 1, 1000, 2000, 3) == 0
    assert fn(65535, 1, 1000, 2000, 1) > 0 and fn(65536, 1, 1000, 2000, 1) == 0


@pytest.mark.parametrize("name, key", [("disn_mc_workspace_bytes", "mc"), ("disn_mc_batch_workspace_bytes", "mc_batch"),
                                       ("disn_grid_band_select_workspace_bytes", "grid_band")])
def test_cursor_layouts_elsewhere(name, key):
    assert len(TABLE[key]) >= 2
    for *args, want in TABLE[key]:
        assert want > 0 and getattr(_lib.lib(), name)(*args) == want, args

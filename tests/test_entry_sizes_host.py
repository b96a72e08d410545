"""The size queries and the first argument check of the utility modules' C entries (metrics, mesh-to-SDF, rendering,
sphere tracing, voxel IoU, batch assembly, marching cubes, the narrow-band selection) are pinned, without a device.
entry_size_table.json holds what the size queries returned from the library built at the commit BEFORE those entries
moved from csrc/api.hip to the end of their modules' own files -- recorded from that build, never from the code under
test.  (disn_mc_*_workspace_bytes and disn_grid_band_select_workspace_bytes: mesh_batch_workspace_table.json.)
A limit that moved shows as a row that changed between a size and 0; which rows are in range is restated here from
include/disn_amd.h, not read off the table."""
import ctypes as C
import json
import os

import pytest

from disn_amd import _lib

TABLE = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "entry_size_table.json")))
INT32_MAX = 2 ** 31 - 1
DISN_E_ARG = -1

# the calls the table must hold, and whether the query takes them (else it returns 0)
IN_RANGE = {
    # every size positive; b <= 65535 is the entries' DISN_E_SHAPE, not the query's
    "disn_metrics_workspace_bytes": lambda b, n, m: b >= 1 and n >= 1 and m >= 1,
    # every axis >= 2 and the point count within int32 (1290^3 = 2 146 689 000 fits, 1291^3 does not)
    "disn_mesh_sign_workspace_bytes": lambda nx, ny, nz: min(nx, ny, nz) >= 2 and nx * ny * nz <= INT32_MAX,
    "disn_trace_state_bytes": lambda n: 1 <= n <= 2 ** 27,
    "disn_voxel_grid_words": lambda n: 1 <= n <= 1024,
    "disn_voxel_surface_workspace_bytes": lambda nf: nf >= 0,
    "disn_voxel_fill_workspace_bytes": lambda n: 1 <= n <= 1024,
}
CALLS = {
    "disn_metrics_workspace_bytes": [(1, 1, 1), (2, 2048, 2048), (24, 4096, 1000), (65535, 1, 1), (65536, 1, 1),
                                     (0, 1, 1), (1, 0, 1), (1, 1, 0)],
    "disn_mesh_sign_workspace_bytes": [(2, 2, 2), (65, 65, 65), (257, 257, 257), (1290, 1290, 1290),
                                       (1291, 1291, 1291), (1, 2, 2)],
    "disn_trace_state_bytes": [(1,), (137 * 137,), (2 ** 27,), (2 ** 27 + 1,), (0,)],
    "disn_voxel_grid_words": [(1,), (32,), (33,), (1024,), (1025,), (0,)],
    "disn_voxel_surface_workspace_bytes": [(0,), (1,), (100000,), (-1,)],
    "disn_voxel_fill_workspace_bytes": [(1,), (32,), (1024,), (1025,)],
}

# every moved entry that returns a status
STATUS_ENTRIES = [
    "disn_mc_count", "disn_mc_emit", "disn_mc_count_batch", "disn_mc_emit_batch",
    "disn_nn_distance", "disn_approx_match", "disn_match_cost", "disn_emd",
    "disn_mesh_udf_points", "disn_mesh_udf_grid", "disn_mesh_sign",
    "disn_render_views",
    "disn_trace_setup", "disn_trace_advance", "disn_trace_collect", "disn_trace_shade",
    "disn_voxel_surface", "disn_voxel_fill", "disn_voxel_index_grid", "disn_voxel_iou",
    "disn_assemble_batch",
    "disn_grid_band_select", "disn_grid_band_fill",
]


def test_table_covers_exactly_the_calls():
    assert sorted(TABLE) == sorted(CALLS)
    for name, calls in CALLS.items():
        assert [tuple(row[:-1]) for row in TABLE[name]] == calls, name


@pytest.mark.parametrize("name", sorted(CALLS))
def test_size_query(name):
    fn = getattr(_lib.lib(), name)
    for *args, want in TABLE[name]:
        got = fn(*args)
        assert (got > 0) == bool(IN_RANGE[name](*args)), (args, got)
        assert got == want, (args, got, want)


@pytest.mark.parametrize("name", STATUS_ENTRIES)
def test_all_null_call_is_an_argument_error(name):
    """Every pointer NULL, every integer 1, every float 1.0: the entry's first check refuses the call, before any HIP
    call (so this is safe on a machine with a device too)."""
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is C.c_int
    args = []
    for t in argtypes:
        if t in (C.c_int, C.c_int64, C.c_size_t):
            args.append(1)
        elif t in (C.c_float, C.c_double):
            args.append(1.0)
        else:
            assert t is C.c_void_p or issubclass(t, C._Pointer), (name, t)
            args.append(None)
    assert any(a is None for a in args), name
    assert getattr(_lib.lib(), name)(*args) == DISN_E_ARG

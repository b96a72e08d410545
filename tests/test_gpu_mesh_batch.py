"""The three batched-mesh stages on a batch whose FIRST and LAST meshes are empty (csrc/mesh_batch.hpp: ``mesh_of`` steps
over empty meshes; the batches of the stages' own tests have their empty mesh in the middle only).  Each stage's result
for the batch is compared bit for bit with the same call on every mesh alone and, for the meshes that have triangles,
with the host rule (``clean_arrays``, ``simplify_arrays``, ``colour_arrays``)."""
import numpy as np
import pytest
import torch

import mesh_clean_fixtures as MF
import mesh_colour_fixtures as CF

pytestmark = pytest.mark.gpu

TRIANGLE = (np.array([[-0.3, -0.2, 0.1], [0.3, -0.2, 0.0], [0.0, 0.3, -0.1]], np.float32),       # inside the unit ball
            np.array([[0, 1, 2]], np.int32))
BATCH = [MF.empty(), MF.fans(), MF.empty(), MF.empty(), TRIANGLE, MF.empty()]
BOX = np.array([-0.4, -0.4, -0.4, 0.4, 0.4, 0.4], np.float64)


def _dev(v, f):
    return torch.from_numpy(np.ascontiguousarray(v)).cuda(), torch.from_numpy(np.ascontiguousarray(f)).cuda()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8),
                                                                     b.contiguous().view(torch.uint8))


def _host_bits(t, want):
    g = t.cpu().numpy()
    want = np.ascontiguousarray(want)
    return g.dtype == want.dtype and g.shape == want.shape and g.tobytes() == want.tobytes()


def test_empty_meshes_at_both_ends_of_a_batch():
    from disn_amd import postprocess
    dev = [_dev(v, f) for v, f in BATCH]
    B = len(BATCH)
    empty = [b for b, (v, f) in enumerate(BATCH) if len(f) == 0]
    assert empty == [0, 2, 3, 5]

    # ---- cleanup, both connectivities
    for conn in ("face", "vertex"):
        cleaned, kept = postprocess.clean_meshes_device(dev, connectivity=conn, strict=False)
        assert len(cleaned) == B and len(kept) == B
        for b, (v, f) in enumerate(BATCH):
            alone, kept_alone = postprocess.clean_meshes_device([dev[b]], connectivity=conn, strict=False)
            assert cleaned[b] is not None and alone[0] is not None, (conn, b)          # status 0, not "nothing kept"
            assert _same_bits(cleaned[b][0], alone[0][0]) and _same_bits(cleaned[b][1], alone[0][1]), (conn, b)
            assert _same_bits(kept[b], kept_alone[0]), (conn, b)
            if b in empty:
                assert cleaned[b][0].shape == (0, 3) and cleaned[b][1].shape == (0, 3) and kept[b].numel() == 0
                continue
            want = MF.host_clean(v, f, connectivity=conn)
            assert want is not None and len(want[2]) > 0
            assert _host_bits(cleaned[b][0], want[0]) and _host_bits(cleaned[b][1], want[1]), (conn, b)
            assert kept[b].tolist() == list(want[2]), (conn, b)

    # ---- simplification, 4 cells, with and without the duplicate-face pass
    boxes = np.tile(BOX, (B, 1))
    for dedup in (True, False):
        simplified, maps = postprocess.simplify_meshes_device(dev, boxes, 4, dedup=dedup)      # raises on a status
        assert len(simplified) == B and len(maps) == B
        for b, (v, f) in enumerate(BATCH):
            alone, maps_alone = postprocess.simplify_meshes_device([dev[b]], boxes[b:b + 1], 4, dedup=dedup)
            for got, one in zip(simplified[b] + maps[b], alone[0] + maps_alone[0]):
                assert _same_bits(got, one), (dedup, b)
            if b in empty:
                assert simplified[b][0].shape == (0, 3) and simplified[b][1].shape == (0, 3)
                assert maps[b][0].numel() == 0 and maps[b][1].numel() == 0
                continue
            want = postprocess.simplify_arrays(v, f, BOX, 4, dedup=dedup)
            assert want[1].shape[0] > 0, "the lattice keeps a face of mesh %d" % b
            for got, w in zip(simplified[b] + maps[b], want):
                assert _host_bits(got, w), (dedup, b)

    # ---- colours: one view, one sample per pixel, the same constant picture and camera for every mesh
    cam, img = CF.pinhole(), CF.flat_image((0.2, 0.5, 0.8))
    cams, imgs = np.tile(cam, (B, 1, 1, 1)), torch.from_numpy(np.tile(img, (B, 1, 1, 1, 1))).cuda()
    cols, seen, status = postprocess.colour_meshes_device(dev, imgs, cams, views_per_mesh=1, S=1, strict=False)
    assert status.tolist() == [0] * B
    for b, (v, f) in enumerate(BATCH):
        c1, s1, st1 = postprocess.colour_meshes_device([dev[b]], imgs[b:b + 1], cams[b:b + 1], views_per_mesh=1, S=1,
                                                       strict=False)
        assert st1.tolist() == [0] and _same_bits(cols[b], c1[0]) and _same_bits(seen[b], s1[0]), b
        if b in empty:
            assert cols[b].shape == (0, 3) and seen[b].shape == (0,)
            continue
        want = postprocess.colour_arrays(v, f, img[None], cam[None], S=1)
        assert (want[1] == 1).any(), "a vertex of mesh %d is seen" % b
        assert _host_bits(cols[b], want[0]) and _host_bits(seen[b], want[1]), b

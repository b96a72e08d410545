"""The workspace sizes of the two training steps are pinned: train_workspace_table.json holds what
disn_train_workspace_bytes / disn_cam_train_workspace_bytes returned before the encoder half of the two steps was
written once (csrc/train.hip, EncTrainWs) -- a buffer lost, doubled or resized by a change of the layout code shows
here, without a device."""
import json
import os

import pytest

from disn_amd import _lib

TABLE = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "train_workspace_table.json")))


@pytest.mark.parametrize("B, N, want", TABLE["sdf"])
def test_sdf_train_workspace_bytes(B, N, want):
    assert _lib.lib().disn_train_workspace_bytes(B, N) == want


@pytest.mark.parametrize("B, N, want", TABLE["cam"])
def test_cam_train_workspace_bytes(B, N, want):
    assert _lib.lib().disn_cam_train_workspace_bytes(B, N) == want

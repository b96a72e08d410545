"""One rank of `python -m disn_amd.train_sdf` under the torchrun environment, for the two-rank test of
tests/test_gpu_train_driver.py: runs train_sdf.main(argv) -- which creates and destroys the process group itself, as
under torchrun -- and prints a digest of the parameters the rank ended with, so that the test can compare the ranks
(every rank applies the same all-reduced gradient to the same initial weights: bit for bit the same parameters).
Prints DDP_TRAIN_OK <rank> <json>.
env: RANK WORLD_SIZE LOCAL_RANK MASTER_ADDR MASTER_PORT;  argv: the driver's arguments"""
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from disn_amd import train_sdf as T  # noqa: E402

kept = {}


class KeepParams(T.Trainer):
    def close(self):
        if self.ctx:
            torch.cuda.synchronize(self.params.device)
            kept["params"], kept["steps"], kept["world"] = self.params.cpu(), self.step_count, self.world
        super().close()


T.Trainer = KeepParams
assert not torch.distributed.is_initialized()
res = T.main(sys.argv[1:])
assert not torch.distributed.is_initialized(), "main left its process group behind"
assert kept["steps"] >= 1, "no step was taken"
print("DDP_TRAIN_OK %d %s" % (int(os.environ["RANK"]), json.dumps({
    "saved": res["saved"], "steps": kept["steps"], "loader": res["loader"], "world": kept["world"],
    "params_sha256": hashlib.sha256(kept["params"].numpy().tobytes()).hexdigest()})))

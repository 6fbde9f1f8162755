"""The manifest of the reference's shipped weight files: for every file under the reference's models/ (not its epoch_save/
directory), the name, dtype and shape of every tensor of its state_dict -- names and shapes only, no weights.
TEST INFRASTRUCTURE ONLY; runs only where a reference checkout is at hand (oracle.gen_golden.REF).

    python -m oracle.gen_golden_checkpoints         # writes tests/golden/g16_reference_checkpoint_manifest.json

tests/test_evaluators_golden.py::test_every_shipped_pc_checkpoint_loads builds each state_dict from it and loads it into get_model.
"""
import glob
import json
import os

import torch

from oracle.gen_golden import GOLDEN, REF

OUT = os.path.join(GOLDEN, "g16_reference_checkpoint_manifest.json")


def main():
    files = []
    for path in sorted(glob.glob(os.path.join(REF, "models", "*"))):
        if os.path.isdir(path):
            continue
        sd = torch.load(path, map_location="cpu")
        files.append({"name": os.path.basename(path),
                      "tensors": [[k, str(v.dtype).replace("torch.", ""), list(v.shape)] for k, v in sd.items()]})
    with open(OUT, "w") as f:
        json.dump({"source": "the reference's models/ directory: tensor names, dtypes and shapes of every state_dict", "files": files}, f,
                  indent=0)
    print(OUT, len(files), "files")


if __name__ == "__main__":
    main()

"""Writes tests/golden/g17_knn_kl/g17_knn_kl.npz: three pairs of fp32 Gaussian clouds and the value the REFERENCE'S OWN `KLdivergence`
(utils/training_evaluation.py:240-284: two scipy cKDTrees queried with eps=.01) returns for each.

    MCPC_REFERENCE_DIR=<a checkout of the reference> python scripts/make_knn_kl_golden.py

The function is imported, not restated: the engine finder is installed (montecarlopredictivecoding_amd/run.py), the checkout goes on
sys.path, and `utils.training_evaluation.KLdivergence` resolves through `run.script_own_attr` to the checkout's own module, executed
where it lies; third-party packages it imports and this machine lacks become empty stand-in modules, as in tests/test_launcher.py.
Needs scipy and no GPU.  The fixture holds data only: the clouds (seeded here) and three numbers.  It lies in a folder of its own:
every `*.npz` directly under tests/golden/ is taken for an oracle-format fixture by tests/golden_util.py (`fixture_names`).
"""
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, n, m, d, shift and scale of y against x)
CASES = (("a", 1200, 1000, 5, 0.5, 1.3), ("b", 700, 900, 1, -1.0, 0.7), ("c", 600, 600, 17, 0.2, 1.1))


def clouds(seed, n, m, d, shift, scale):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    y = (shift + scale * rng.standard_normal((m, d))).astype(np.float32)
    return x, y


def reference_kl():
    from oracle import ref_stage
    ref = os.environ.get("MCPC_REFERENCE_DIR", ref_stage.REF)
    if not os.path.isfile(os.path.join(ref, "utils", "training_evaluation.py")):
        raise SystemExit("no checkout of the reference at %s (set MCPC_REFERENCE_DIR)" % ref)
    # what utils/training_evaluation.py and utils/data.py import from torchvision, as names that only exist
    stand_ins = {"torchvision": (), "torchvision.utils": ("save_image",), "torchvision.transforms": (), "torchvision.datasets": ()}
    try:
        importlib.import_module("torchvision")
    except ImportError:
        for name, attrs in stand_ins.items():
            sys.modules[name] = types.ModuleType(name)
            for a in attrs:
                setattr(sys.modules[name], a, None)
            if "." in name:
                setattr(sys.modules["torchvision"], name.rpartition(".")[2], sys.modules[name])
    from montecarlopredictivecoding_amd import run
    run.install()
    sys.path.insert(0, ref)
    te = importlib.import_module("utils.training_evaluation")
    fn = te.KLdivergence
    assert fn.__module__.startswith("_mcpc_script_own."), fn.__module__
    return fn


def main():
    kl = reference_kl()
    out = {}
    for j, (name, n, m, d, shift, scale) in enumerate(CASES):
        x, y = clouds(1700 + j, n, m, d, shift, scale)
        out["x_" + name], out["y_" + name] = x, y
        out["kl_" + name] = np.float64(kl(x, y))
        print("%s: n=%d m=%d d=%d  KLdivergence=%.17g" % (name, n, m, d, out["kl_" + name]))
    path = os.path.join(ROOT, "tests", "golden", "g17_knn_kl", "g17_knn_kl.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()

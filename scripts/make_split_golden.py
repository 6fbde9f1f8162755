#!/usr/bin/env python3
"""Record the cases of tests/split_bitwise_cases.py on the library the process loads, or compare two such recordings.

  MCPC_LIB=scripts/bin/libmcpc_parent.so python3 scripts/make_split_golden.py record tests/golden/split_bitwise_parent.golden
  python3 scripts/make_split_golden.py record out/split_new.npz            # the tree's own library
  python3 scripts/make_split_golden.py diff tests/golden/split_bitwise_parent.golden out/split_new.npz

scripts/make_split_golden.sh builds the parent commit's library and runs the first line.  The recording names the library's csrc hash
and commit (meta/csrc, meta/commit; also written to <file>.txt beside it): tests/test_gpu_split_bitwise.py compares the loaded
library's results with it, so it must come from the commit BEFORE the change under test, never from the tree's own library.
The recording is an .npz archive under the extension .golden: every *.npz under tests/golden/ is taken for a fixture of the oracle
(tests/golden_util.py: fixture_names)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


FORMAT_NOTE = """%s is a NumPy .npz archive (np.load reads it) under another extension: tests/golden_util.py takes every *.npz of
this folder for a fixture of the oracle.  Read by tests/test_gpu_split_bitwise.py; cases in tests/split_bitwise_cases.py.  Re-record
(only when a change moves results on purpose, from the commit before it): scripts/make_split_golden.sh build <commit>, then `record` on a GPU.
"""


def record(path):
    import torch
    from montecarlopredictivecoding_amd import _lib as L
    from tests import split_bitwise_cases as sc
    info = L.build_info()
    dev = torch.device("cuda", 0)
    store = {"meta/csrc": np.array(info["csrc"]), "meta/commit": np.array(info["commit"])}
    for case in sc.cases():
        got = sc.run_case(case, dev)
        store[f"{case['name']}/kernel"] = np.array(got.pop("kernel"))
        store[f"{case['name']}/flush"] = np.array(got.pop("flush"))
        for name, a in got.items():
            if sc.keeps_raw(name, a):
                store[f"{case['name']}/{name}"] = a
            else:
                store[f"{case['name']}/{name}#sha256"] = sc.digest(a)
        print(f"{case['name']:<28} {store[case['name'] + '/kernel']}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:         # (a file object: NumPy appends no ".npz" to the name)
        np.savez_compressed(f, **store)
    note = f"recorded from libmcpc csrc={info['csrc']} commit={info['commit']} ({os.path.basename(info['path'])}) by scripts/make_split_golden.py\n"
    with open(os.path.splitext(path)[0] + ".txt", "w") as f:
        f.write(note + FORMAT_NOTE % os.path.basename(path))
    print(note, end="")


def diff(a_path, b_path):
    from tests import split_bitwise_cases as sc
    a, b = np.load(a_path), np.load(b_path)
    print(f"{a_path}: csrc {a['meta/csrc']}   {b_path}: csrc {b['meta/csrc']}")
    n_bad = n = 0
    for key in a.files:
        if key.startswith("meta/"):
            continue
        if key not in b.files:
            print(f"  {key}: missing in {b_path}")
            n_bad += 1
            continue
        n += 1
        same = str(a[key]) == str(b[key]) if key.endswith(("/kernel", "/flush")) else np.array_equal(a[key], b[key], equal_nan=a[key].dtype.kind == "f")
        if not same:
            n_bad += 1
            print(f"  {key}: DIFFERS" + (f" ({a[key]} | {b[key]})" if key.endswith(("/kernel", "/flush")) else ""))
    print(f"{n} entries compared, {n_bad} differing" + ("" if n_bad else ": every array bitwise equal"))
    return 1 if n_bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "record":
        record(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "diff":
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)

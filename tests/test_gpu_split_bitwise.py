"""The step kernels, the flush and the evaluators' shared operand split against results recorded from the PARENT commit's library.

csrc/mcpc_gemm_f16.h: split2_pair serves every kernel form, so the form-against-form tests of this suite cannot see a change in it.
tests/golden/split_bitwise_parent.golden (an .npz archive; every *.npz there is an oracle fixture, hence the name) holds what the library of the commit before the single-rounding split computed
(split_bitwise_parent.txt names its csrc hash; recorded by scripts/make_split_golden.sh) for the cases of
tests/split_bitwise_cases.py -- the small net of profiles/step_math_ab.txt on four kernel forms, two activations and two read-outs;
cfg-M's net at batch 48 with rows spanning more than 2^17 (second pieces that are fp16 subnormals), with and without an Inf and a NaN
chain; the same net on the round schedule with the spill at system scope -- and the loaded library must reproduce them bit for bit:
final states, one recorded step, all energies, the flat gradient bucket (`np.array_equal`, NaNs by position; arrays too large to keep
are compared by the SHA-256 of their bytes).

When a later change moves results ON PURPOSE, the recording is made anew from the commit before THAT change
(`scripts/make_split_golden.sh build <commit>` where the history is, `scripts/make_split_golden.sh record` on the GPU) and the reason
goes into the commit; tests/golden/split_bitwise_parent.txt says which library the present one came from and why the file is not
called .npz."""
import os

import numpy as np
import pytest
import torch

from tests import split_bitwise_cases as sc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "split_bitwise_parent.golden")
CASES = sc.cases()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_the_recording_is_not_of_this_tree(golden):
    from montecarlopredictivecoding_amd import _lib as L
    assert str(golden["meta/csrc"]) != L.csrc_sha(), "the golden file must be recorded from the parent commit's library"
    names = {k.split("/")[0] for k in golden.files} - {"meta"}
    assert names == {c["name"] for c in CASES}, names ^ {c["name"] for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c["name"].replace(" ", "-") for c in CASES])
def test_bitwise_equal_to_the_parent(case, golden):
    got = sc.run_case(case, torch.device("cuda", 0))
    kernel, flush = got.pop("kernel"), got.pop("flush")
    name = case["name"]
    print(f"[split bitwise] {name}: ran {kernel!r}; flush {flush!r}")
    assert kernel == str(golden[f"{name}/kernel"]), (kernel, str(golden[f"{name}/kernel"]))
    if name == "B":
        assert "mcpc_steps_ws2_spec_kernel" in kernel and "hot" in kernel, kernel
        # the flush instantiations the case is there to reach (mcpc_last_flush_plan names what was launched)
        assert all(k in flush for k in ("heb7<2,2,T>", "heb7<16,2>", "heb7<17,2>")), flush
    if name == "C":
        assert "hot+spill" in kernel, kernel
    if case["init"] != "special":
        assert all(np.isfinite(a).all() for a in got.values()) and got["flat"].any() and got["energies"].any(), name
    else:
        # the two poisoned chains stay poisoned and stay alone (their tile neighbours and the wide-range chains are finite)
        assert np.isnan(got["x1"][21]).any() and not np.isfinite(got["x0"][5]).all(), name
        assert all(np.isfinite(got[f"x{l}"][[0, 3, 4, 6, 19, 20, 22, 35, 47]]).all() for l in range(3)), name
    differing = []
    for key, a in got.items():
        if sc.keeps_raw(key, a):
            want = golden[f"{name}/{key}"]
            if not (want.dtype == a.dtype and np.array_equal(a, want, equal_nan=True)):
                n = int((~((a == want) | (np.isnan(a) & np.isnan(want)))).sum()) if want.shape == a.shape else -1
                differing.append(f"{key}: {n} of {a.size} elements")
        elif not np.array_equal(sc.digest(a), golden[f"{name}/{key}#sha256"]):
            differing.append(f"{key}: digest")
    assert not differing, (name, differing)

"""The table of tests/stream_cases.py against include/mcpc.h, without a device: every function whose last parameter is `void* stream`
is named by a case or excluded by name, the table holds the cases it is meant to hold, and the poison of every index tensor is a
valid index."""
import os
import re

import numpy as np

from tests import stream_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# a case that leaves the table fails here, also where another case names the same entry points
EXPECTED = {
    "run[small]", "run[small,no_overlap=1]", "run[small,ws=0]", "run[small,ws=4]", "run[more]", "run[ws=3,adam,tanh]",
    "run[update_x=False]", "params_changed", "param_grads", "chain_energies", "prediction_errors", "sample_prior",
    "philox_normals", "box_muller", "moments_accumulate", "cov_accumulate[pooled]", "cov_accumulate[per chain]",
    "hist_accumulate[pooled]", "hist_accumulate[per chain]", "hist2d_accumulate", "acov_accumulate[fresh]", "acov_accumulate[continued]",
    "roll_accumulate", "probe_accumulate", "probe_records", "knn_accumulate", "loglik_accumulate", "ais_increment", "mala_propose",
    "mala_accept", "hmc_trajectory", "smc_ancestors", "smc_gather",
    "train_on_batch[moments_side_stream=False]", "train_on_batch[moments_side_stream=True]", "mcpc_ais[plain]",
    "mcpc_ais[mala,leapfrog=2]", "mcpc_ais[systematic]",
}


def stream_functions(header_text):
    """The functions of a header whose last parameter is `void* stream`."""
    text = re.sub(r"/\*.*?\*/", " ", header_text, flags=re.S)
    return sorted(set(re.findall(r"\b(mcpc_\w+)\s*\([^;{}]*?\bvoid\s*\*\s*stream\s*\)\s*;", text)))


def _header():
    with open(os.path.join(ROOT, "include", "mcpc.h")) as f:
        return f.read()


def uncovered(functions, cases, excluded=sc.EXCLUDED):
    named = {e for c in cases for e in c.entries}
    return sorted(set(functions) - named - set(excluded))


def test_every_stream_entry_point_has_a_case_or_is_excluded():
    fns = stream_functions(_header())
    assert len(fns) == 35 and "mcpc_run" in fns and "mcpc_smc_gather" in fns and "mcpc_create" not in fns, fns
    assert sc.EXCLUDED == ("mcpc_sync_check", "mcpc_debug_poison_lds", "mcpc_allreduce_grads")
    assert set(sc.EXCLUDED) <= set(fns)
    assert uncovered(fns, sc.CASES) == []
    named = {e for c in sc.CASES for e in c.entries}
    assert named <= set(fns), sorted(named - set(fns))              # a case names functions of the header, nothing else
    assert not named & set(sc.EXCLUDED)


def test_a_new_entry_point_without_a_case_is_found():
    grown = _header() + "\nint mcpc_new_reducer(int device, const float* rec,\n                     double* sum, void* stream);\n"
    assert uncovered(stream_functions(grown), sc.CASES) == ["mcpc_new_reducer"]


def test_the_table_holds_its_cases():
    assert {c.name for c in sc.CASES} == EXPECTED
    for c in sc.CASES:
        assert c.entries or c.facade, c.name
    # the only case that names an entry point alone is missed by the first test when it goes
    lone = [c for c in sc.CASES if c.name == "moments_accumulate"]
    assert uncovered(stream_functions(_header()), [c for c in sc.CASES if c not in lone]) == ["mcpc_moments_accumulate"]


def test_the_poison_of_every_index_tensor_is_in_range_and_differs():
    seen = 0
    for c in sc.CASES:
        for name, (lo, hi, step) in c.index.items():
            real = c.inputs()[name]
            assert real.dtype.kind in "iu" and name in c.pending_names(), (c.name, name)
            assert real.min() >= lo and real.max() < hi, (c.name, name)
            p = sc.poison_of(c, name, real)
            assert p.dtype == real.dtype and p.shape == real.shape
            assert p.min() >= lo and p.max() < hi, (c.name, name)
            assert (p != real).all(), (c.name, name)
            seen += 1
    assert seen >= 3                                                   # box_muller's two bit patterns, smc_gather's ancestors
    gather = sc.BY_NAME["smc_gather"]
    assert gather.index["ancestors"][:2] == (0, gather.ROWS)        # the range IS the rows of the state it gathers from


def test_float_poison_is_nan_and_other_data_must_be_declared():
    c = sc.BY_NAME["moments_accumulate"]
    assert np.isnan(sc.poison_of(c, "rec", c.inputs()["rec"])).all()
    try:
        sc.poison_of(c, "count", np.arange(3, dtype=np.int32))
    except TypeError:
        pass
    else:
        raise AssertionError("integer data without a declared range got a poison")

"""Sample clouds and the nearest-neighbour KL estimate, the host side: the request's validation, the row order of a cloud, which rows of
a slice are samples, the estimator's fp64 arithmetic against numpy and against the reference's recorded values, and the C entry point's
argument checks.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from montecarlopredictivecoding_amd import _lib
from montecarlopredictivecoding_amd import cloud as K
from montecarlopredictivecoding_amd.covariance import sample_steps
from tests import knn_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (20, 128, 128)
GOLDEN = os.path.join(ROOT, "tests", "golden", "g17_knn_kl", "g17_knn_kl.npz")
FIXTURE_CASES = (("a", 1200, 1000, 5), ("b", 700, 900, 1), ("c", 600, 600, 17))


def _ok(**kw):
    spec = dict(begin=500, stride=1, layer=2, units=(3, 17, 40, 77, 101))
    spec.update(kw)
    return K.validate_spec(spec, 10000, 3, SIZES, 256, 1 << 30)


def test_a_good_request_and_its_defaults():
    s = _ok()
    assert (s.begin, s.stride, s.layer, s.units, s.T, s.n, s.d) == (500, 1, 2, (3, 17, 40, 77, 101), 10000, 9500, 5)
    s = K.validate_spec(dict(layer=0), 7, 3, SIZES, 4, 1 << 30)
    assert (s.begin, s.stride, s.units, s.n) == (0, 1, tuple(range(20)), 7)           # units=None: every unit of a layer of at most 32
    assert _ok(units=[5]).units == (5,) and _ok(units=9).units == (9,)
    assert _ok(units=(101, 3)).units == (101, 3)                                      # the order given is the order of the columns
    assert len(_ok(units=tuple(range(32))).units) == 32


@pytest.mark.parametrize("spec, word", [
    ("cloud", "expected a dict or None, got str"),
    (dict(layer=2, unit=(1,)), r"unknown keys \['unit'\]"),
    (dict(layer=2, units=(1,), begin=10000), r"begin=10000 outside \[0, T=10000\)"),
    (dict(layer=2, units=(1,), begin=-1), "begin=-1 outside"),
    (dict(layer=2, units=(1,), begin=1.0), "begin must be an int"),
    (dict(layer=2, units=(1,), begin=True), "begin must be an int"),
    (dict(layer=2, units=(1,), stride=0), "stride=0, must be at least 1"),
    (dict(layer=2, units=(1,), stride="2"), "stride must be an int"),
    (dict(units=(1,)), "layer is required"),
    (dict(layer=None, units=(1,)), "layer is required"),
    (dict(layer=3, units=(1,)), "layer index 3 out of range"),
    (dict(layer=-1, units=(1,)), "layer index -1 out of range"),
    (dict(layer=1.0, units=(1,)), "layer must be an int"),
    (dict(layer=2), "units=None asks for every unit of layer 2, which is 128 wide"),
    (dict(layer=2, units=()), "0 units, expected 1..32"),
    (dict(layer=2, units=tuple(range(33))), "33 units, expected 1..32"),
    (dict(layer=2, units=(1, 128)), "unit index 128 out of range, layer 2 has 128 units"),
    (dict(layer=0, units=(20,)), "unit index 20 out of range, layer 0 has 20 units"),
    (dict(layer=2, units=(-1,)), "unit index -1 out of range"),
    (dict(layer=2, units=(1.5,)), "unit index 1.5 out of range"),
    (dict(layer=2, units=(True,)), "unit index True out of range"),
    (dict(layer=2, units=(4, 9, 4)), r"units \[4, 9, 4\] are not distinct"),
    (dict(layer=2, units=1.5), "units must be a sequence"),
])
def test_bad_requests(spec, word):
    with pytest.raises(ValueError, match="mcpc_cloud: .*" + word):
        K.validate_spec(spec, 10000, 3, SIZES, 256, 1 << 30)


def test_the_byte_budget():
    need = 4 * 9500 * 256 * 5                                                         # figure 5: 48.6 MB
    spec = dict(begin=500, layer=2, units=(3, 17, 40, 77, 101))
    assert K.validate_spec(spec, 10000, 3, SIZES, 256, need).n == 9500
    with pytest.raises(ValueError, match=r"mcpc_cloud: the cloud \(9500 samples x 256 chains x 5 units fp32\) takes 46.4 MiB, more than "
                                         r"mcpc_cloud_max_bytes = 46.4 MiB"):
        K.validate_spec(spec, 10000, 3, SIZES, 256, need - 1)
    assert K.validate_spec(dict(spec, stride=2), 10000, 3, SIZES, 256, need // 2).n == 4750


@pytest.mark.parametrize("begin, stride, T", [(0, 1, 40), (13, 3, 40), (39, 5, 40), (7, 40, 40), (20, 7, 61)])
def test_chunk_agrees_with_sample_steps(begin, stride, T):
    s = K.validate_spec(dict(begin=begin, stride=stride, layer=0, units=(0,)), T, 3, SIZES, 2, 1 << 30)
    steps = list(sample_steps(begin, T, stride))
    assert s.n == len(steps)
    for per in (1, 4, 9, T):
        got = []
        for t0 in range(0, T, per):
            first, cnt = s.chunk(t0, min(per, T - t0))
            got += [t0 + first + j * stride for j in range(cnt)]
            assert cnt == 0 or (0 <= first and first + (cnt - 1) * stride < min(per, T - t0))
        assert got == steps, (per, got)


def test_the_row_order_of_a_cloud():
    n, B, d = 7, 3, 2
    pts = torch.arange(n * B * d, dtype=torch.float32).reshape(n, B, d)
    c = K.Cloud(points=pts, units=(4, 9), layer=2)
    assert (c.n, c.B, c.d, c.units, c.layer) == (n, B, d, (4, 9), 2)
    xs = [[None, None, pts[t]] for t in range(n)]                                     # the reference's res["xs"][t][layer]
    assert torch.equal(c.flat(), torch.concatenate([r[2] for r in xs]))               # step-major, then chain
    assert c.flat().data_ptr() == pts.data_ptr()                                      # a view
    assert torch.equal(c.thin(4), torch.concatenate([r[2] for r in xs])[::4]) and tuple(c.thin(4).shape) == (6, d)
    assert torch.equal(c.cpu().points, pts) and c.cpu().units == (4, 9)
    other = K.Cloud(points=pts + 100, units=(4, 9), layer=2)
    both = K.Cloud.cat([c, other])
    assert (both.n, both.B, both.d) == (n, 2 * B, d)
    assert torch.equal(both.points[:, :B], pts) and torch.equal(both.points[:, B:], pts + 100)       # along the chains, in order
    for bad in (K.Cloud(points=pts[:5], units=(4, 9), layer=2), K.Cloud(points=pts, units=(4, 8), layer=2),
                K.Cloud(points=pts, units=(4, 9), layer=1)):
        with pytest.raises(ValueError, match="different requests"):
            K.Cloud.cat([c, bad])


def test_kl_from_sqdist_is_the_references_formula():
    rng = np.random.default_rng(3)
    n, m, d = 400, 300, 5
    r2, s2 = rng.uniform(1e-3, 2.0, n), rng.uniform(1e-3, 2.0, n)
    want = -np.log(np.sqrt(r2) / np.sqrt(s2)).sum() * d / n + np.log(m / (n - 1.0))
    got = K.kl_from_sqdist(torch.from_numpy(r2.astype(np.float32)), torch.from_numpy(s2.astype(np.float32)), n, m, d)
    assert got.dtype == torch.float64 and got.dim() == 0 and got.device.type == "cpu"
    want32 = R.kl_from_sqdist(r2.astype(np.float32), s2.astype(np.float32), n, m, d)
    assert abs(float(got) - want32) <= 1e-12 * max(1.0, abs(want32))                  # the same fp32 inputs: fp64 rounding alone
    assert abs(float(got) - want) <= d * 2.0 ** -23                                   # the fp32 rounding of the inputs, d * 2 u
    # duplicates: what the arithmetic gives, as in the reference
    z = K.kl_from_sqdist(torch.tensor([0.0, 1.0]), torch.tensor([1.0, 1.0]), 2, 2, 1)
    assert float(z) == float("inf")


@pytest.mark.parametrize("name, n, m, d", FIXTURE_CASES)
def test_exact_distances_reproduce_the_references_recorded_value(name, n, m, d):
    """The reference's own KLdivergence (eps=.01 trees) against this module's formula on exact fp64 brute-force distances of the same
    fp32 clouds: within d log 1.01 (tests/knn_cases.py)."""
    g = np.load(GOLDEN)
    x, y, ref = g["x_" + name], g["y_" + name], float(g["kl_" + name])
    assert x.dtype == y.dtype == np.float32 and x.shape == (n, d) and y.shape == (m, d)
    r2, s2 = R.kbest(x, x, 2), R.kbest(x, y, 1)
    assert bool((r2[:, 0] == 0).all()) and bool((r2[:, 1] > 0).all())                 # the nearest row of x to x_i is x_i itself
    got = float(K.kl_from_sqdist(torch.from_numpy(r2[:, 1]), torch.from_numpy(s2[:, 0]), n, m, d))
    print("%s: reference %.12g, exact %.12g, difference %.3g (bound %.3g)" % (name, ref, got, abs(got - ref), d * np.log(1.01)))
    assert abs(got - R.kl_exact(x, y)) <= 1e-12
    assert abs(got - ref) <= d * np.log(1.01)


def test_without_a_device_the_search_raises():
    if torch.cuda.is_available():
        pytest.skip("a HIP device is visible")
    x = np.zeros((4, 3), dtype=np.float32)
    with pytest.raises(_lib.MCPCLibraryError, match="no HIP device is visible"):
        K.knn_sqdist(x, x, 2)
    with pytest.raises(_lib.MCPCLibraryError, match="no HIP device is visible"):
        K.kl_divergence(torch.zeros(4, 3), x)
    from montecarlopredictivecoding_amd.utils import training_evaluation as te
    with pytest.raises(_lib.MCPCLibraryError, match="no HIP device is visible"):
        te.knn_kl_divergence(x, x)
    assert "KLdivergence" not in vars(te)                                             # that name stays the script's own


def test_the_trainer_has_the_opt_in_attributes_and_they_are_off():
    import montecarlopredictivecoding_amd.predictive_coding as pc
    model = torch.nn.Sequential(torch.nn.Linear(2, 2), pc.PCLayer(), torch.nn.Linear(2, 3))
    tr = pc.PCTrainer(model, T=4, plot_progress_at=[])
    assert tr.mcpc_cloud is None and tr.mcpc_last_cloud is None and tr.mcpc_cloud_max_bytes == 1 << 30
    import montecarlopredictivecoding_amd.utils.model as um
    assert callable(um.get_posterior_cloud)


def test_header_declares_the_entry_point_and_the_binding_binds_it():
    header = open(os.path.join(ROOT, "include", "mcpc.h")).read()
    assert re.search(r"\bint\s+mcpc_knn_accumulate\s*\(", header) and re.search(r"\bint64_t\s+mcpc_knn_workspace_bytes\s*\(", header)
    assert re.search(r"#define\s+MCPC_KNN_MAX_DIM\s+32\b", header) and re.search(r"#define\s+MCPC_KNN_MAX_K\s+4\b", header)
    assert (_lib.KNN_MAX_DIM, _lib.KNN_MAX_K, K.MAX_UNITS) == (32, 4, 32)
    assert re.search(r"#define\s+MCPC_ABI_VERSION\s+4\b", header) and _lib.ABI_VERSION == 4
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, n_args, res in (("mcpc_knn_accumulate", 12, C.c_int), ("mcpc_knn_workspace_bytes", 4, C.c_int64)):
        decl = re.search(name + r"\s*\(([^)]*)\)", code).group(1)
        assert len(_lib.SYMBOLS[name][1]) == len(decl.split(",")) == n_args and _lib.SYMBOLS[name][0] is res
    from montecarlopredictivecoding_amd import engine
    assert callable(engine.knn_accumulate) and callable(engine.knn_workspace_bytes)
    lib = _lib.load()
    assert lib.mcpc_abi_version() == 4 and hasattr(lib, "mcpc_knn_accumulate")
    preamble = open(os.path.join(ROOT, "montecarlopredictivecoding_amd", "csrc", "mcpc_knn.h")).read().split("#pragma once")[0]
    assert "MFMA" in preamble and "cancels" in preamble                               # why the pair loop is not on the matrix unit


def test_argument_errors_are_refused_before_any_device_work():
    """Every MCPC_EINVAL case returns -1 with a message and touches no device: the pointers are never dereferenced (this machine need
    not have a GPU)."""
    lib = _lib.load()
    p = [C.c_void_p(0x1000 * (i + 1)) for i in range(4)]             # never dereferenced: every call below is refused
    need = lib.mcpc_knn_workspace_bytes(1000, 4099, 5, 2)
    assert need > 0 and need % (1000 * 2 * 4) == 0 and need == lib.mcpc_knn_workspace_bytes(1000, 4099, 5, 2)
    assert lib.mcpc_knn_workspace_bytes(1000, 4099, 5, 3) == lib.mcpc_knn_workspace_bytes(1000, 4099, 5, 4) == 2 * need
    assert lib.mcpc_knn_workspace_bytes(0, 4099, 5, 2) == 0 and lib.mcpc_knn_workspace_bytes(1000, 0, 5, 2) == 0

    def call(q=p[0], nq=1000, ref=p[1], nr=4099, d=5, k=2, best=p[2], accumulate=0, ws=p[3], ws_bytes=need):
        rc = lib.mcpc_knn_accumulate(0, q, nq, ref, nr, d, k, best, accumulate, ws, ws_bytes, None)
        return rc, lib.mcpc_last_error().decode()

    for kw, word in [(dict(d=33), "d=33 outside 1..32"), (dict(d=0), "d=0 outside"), (dict(k=5), "k=5 outside 1..4"),
                     (dict(k=0), "k=0 outside"), (dict(nq=-1), "nq=-1 outside"), (dict(nr=-1), "nr=-1 outside"),
                     (dict(nq=1 << 31), "nq=2147483648 outside"), (dict(nr=1 << 31), "nr=2147483648 outside"),
                     (dict(q=None), "q is null with nq=1000"), (dict(ref=None), "ref is null with nr=4099"),
                     (dict(best=None), "best is null with nq=1000"), (dict(ws=None), "workspace is null"),
                     (dict(ws_bytes=need - 1), "workspace of %d bytes is too small, %d needed" % (need - 1, need))]:
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("knn:") and word in msg, (kw, rc, msg)
        args = {"nq": 1000, "nr": 4099, "d": 5, "k": 2}
        if set(kw) & set(args):
            args.update(kw)
            assert lib.mcpc_knn_workspace_bytes(args["nq"], args["nr"], args["d"], args["k"]) == -1
    # nothing to do: accepted without a device, and nothing is read
    assert call(nq=0, q=None, best=None, ws=None, ws_bytes=0)[0] == 0
    assert call(nr=0, ref=None, accumulate=1, ws=None, ws_bytes=0)[0] == 0

"""Posterior covariances, host side (no GPU): the `mcpc_covariance` request, the sample count, the fp64 arithmetic from sums to
covariance and correlation, and the C entry points' declaration and binding."""
import os
import re

import numpy as np
import pytest
import torch

from montecarlopredictivecoding_amd import _lib
from montecarlopredictivecoding_amd import covariance as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (6, 16, 16)
KW = dict(T=60, n_layers=3, n_out=24, sizes=SIZES, B=37, max_bytes=2 << 30)


def test_defaults():
    spec = V.validate_spec({}, **KW)
    assert (spec.begin, spec.stride, spec.layers, spec.outputs, spec.pooled, spec.T) == (0, 1, (0, 1, 2), None, False, 60)
    assert spec.columns == (("x0", 0, 6), ("x1", 6, 16), ("x2", 22, 16)) and spec.D == 38 and spec.n == 60
    spec = V.validate_spec(dict(begin=13, stride=3, layers=(2, 0, 2), outputs="sigmoid", pool="chains"), **KW)
    assert spec.layers == (0, 2) and spec.pooled and spec.n == len(range(13, 60, 3))
    assert spec.columns == (("x0", 0, 6), ("x2", 6, 16), ("out", 22, 24)) and spec.D == 46
    assert V.validate_spec(dict(layers=1), **KW).columns == (("x1", 0, 16),)
    assert V.validate_spec(dict(layers=(), outputs="identity"), **KW).columns == (("out", 0, 24),)


@pytest.mark.parametrize("spec, word", [
    (dict(begin=5, strid=2), "unknown keys"),
    (dict(begin=-1), "begin"),
    (dict(begin=60), "begin"),
    (dict(begin=1.0), "begin must be an int"),
    (dict(begin=True), "begin must be an int"),
    (dict(stride=0), "stride"),
    (dict(stride="2"), "stride must be an int"),
    (dict(layers=(0, 3)), "layer index"),
    (dict(layers=(-1,)), "layer index"),
    (dict(layers=(True,)), "layer index"),
    (dict(layers=1.5), "sequence of layer indices"),
    (dict(layers=()), "no columns"),
    (dict(outputs="softmax"), "outputs"),
    (dict(pool="records"), "pool"),
    (dict(pool=True), "pool"),
    ([("begin", 0)], "expected a dict"),
])
def test_invalid_requests_are_value_errors(spec, word):
    with pytest.raises(ValueError, match=word):
        V.validate_spec(spec, **KW)


def test_outputs_need_a_read_out():
    with pytest.raises(ValueError, match="read-out"):
        V.validate_spec(dict(outputs="identity"), **dict(KW, n_layers=2, n_out=0))
    assert V.validate_spec(dict(layers=(1,)), **dict(KW, n_layers=2, n_out=0)).layers == (1,)


def test_the_size_guard_names_the_size_and_the_ways_out():
    need = 8 * (38 * 38 + 38) * 37
    assert V.result_bytes(38, 37, False) == need and V.result_bytes(38, 37, True) == 8 * (38 * 38 + 38)
    assert V.validate_spec({}, **dict(KW, max_bytes=need)).D == 38
    with pytest.raises(ValueError, match=r"37 chains x 38 x 38.*KiB.*fewer layers or pool='chains'"):
        V.validate_spec({}, **dict(KW, max_bytes=need - 1))
    assert V.validate_spec(dict(pool="chains"), **dict(KW, max_bytes=need - 1)).pooled
    with pytest.raises(ValueError, match=r"one 38 x 38.*fewer layers$"):
        V.validate_spec(dict(pool="chains"), **dict(KW, max_bytes=1000))
    # the reference's 20-128-128 net at batch 256, every layer, per chain: 156 MB of sums pass the default of 2 GiB; 20000 chains do not
    big = dict(T=8000, n_layers=3, n_out=784, sizes=(20, 128, 128), max_bytes=2 << 30)
    assert V.validate_spec({}, B=256, **big).D == 276
    with pytest.raises(ValueError, match="GiB"):
        V.validate_spec({}, B=20000, **big)


@pytest.mark.parametrize("begin, stride, T", [(0, 1, 1), (13, 3, 60), (59, 7, 60), (200, 1, 1000), (3, 4, 5), (0, 60, 60)])
def test_sample_count_and_chunks(begin, stride, T):
    spec = V.validate_spec(dict(begin=begin, stride=stride), **dict(KW, T=T))
    steps = list(range(begin, T, stride))
    assert spec.n == len(steps)
    for S in (1, 5, 7, T):                               # however the call is sliced, the chunks name exactly the sample steps
        got = []
        for t0 in range(0, T, S):
            n = min(S, T - t0)
            first, cnt = spec.chunk(t0, n)
            assert cnt == 0 or (0 <= first and first + (cnt - 1) * stride < n)
            got += [t0 + first + k * stride for k in range(cnt)]
        assert got == steps


COLUMNS = [("x0", 0, 3), ("x2", 3, 4), ("out", 7, 2)]


def _sums(v, pooled):
    """v: [n, B, D] fp64 -> Covariance of its raw sums."""
    n, B, _ = v.shape
    if pooled:
        flat = v.reshape(n * B, -1)
        return V.Covariance(n=n, B=B, pooled=True, columns=list(COLUMNS), sum=flat.sum(0), outer=flat.T @ flat)
    return V.Covariance(n=n, B=B, pooled=False, columns=list(COLUMNS), sum=v.sum(0), outer=torch.einsum("nbi,nbj->bij", v, v))


@pytest.mark.parametrize("pooled", [False, True])
def test_cov_corr_block_against_numpy(pooled):
    g = torch.Generator().manual_seed(0)
    v = torch.randn(11, 5, 9, generator=g, dtype=torch.float64) * 2.0 + 0.5
    c = _sums(v, pooled)
    vn = v.numpy()
    groups = [vn.reshape(-1, 9)] if pooled else [vn[:, b] for b in range(5)]
    assert c.N == (55 if pooled else 11)
    for ddof in (0, 1):
        want = np.stack([np.cov(x, rowvar=False, ddof=ddof) for x in groups])
        got = c.cov(ddof=ddof).numpy().reshape(want.shape)
        assert c.cov(ddof=ddof).dtype == torch.float64
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(c.mean.numpy().reshape(len(groups), 9), np.stack([x.mean(0) for x in groups]), rtol=0, atol=1e-14)
    want = np.stack([np.corrcoef(x, rowvar=False) for x in groups])
    np.testing.assert_allclose(c.corr().numpy().reshape(want.shape), want, rtol=0, atol=1e-12)
    full = c.cov(ddof=1)
    assert torch.equal(c.block("x0", "out"), full[..., 0:3, 7:9]) and torch.equal(c.block("x2", "x2"), full[..., 3:7, 3:7])
    assert torch.equal(c.block("out", "x0", ddof=0), c.cov(ddof=0)[..., 7:9, 0:3])
    with pytest.raises(KeyError, match="x1"):
        c.block("x1", "x0")


@pytest.mark.parametrize("pooled", [False, True])
def test_merge_and_too_few_samples(pooled):
    g = torch.Generator().manual_seed(1)
    v = torch.randn(12, 4, 9, generator=g, dtype=torch.float64)
    both = _sums(v[:5], pooled).merge(_sums(v[5:], pooled))
    whole = _sums(v, pooled)
    assert both.n == 12 and both.B == 4 and both.pooled == pooled and both.columns == whole.columns
    torch.testing.assert_close(both.cov(), whole.cov(), rtol=0, atol=1e-12)
    torch.testing.assert_close(both.sum, whole.sum, rtol=0, atol=1e-12)
    with pytest.raises(ValueError, match="different requests"):
        whole.merge(_sums(v[:, :3], pooled))
    one = _sums(v[:1, :1], pooled)                       # one sample: no unbiased covariance, as torch.var of one sample
    assert one.N == 1 and torch.isnan(one.cov(ddof=1)).all() and torch.isfinite(one.cov(ddof=0)).all()
    assert torch.isnan(one.cov(ddof=2)).all()


def test_the_trainer_has_the_opt_in_attributes_and_they_are_off():
    import montecarlopredictivecoding_amd.predictive_coding as pc
    model = torch.nn.Sequential(torch.nn.Linear(2, 2), pc.PCLayer(), torch.nn.Linear(2, 3))
    tr = pc.PCTrainer(model, T=4, plot_progress_at=[])
    assert tr.mcpc_covariance is None and tr.mcpc_last_covariance is None and tr.mcpc_covariance_max_bytes == 2 << 30


def test_header_declares_the_entry_points_and_the_binding_binds_them():
    header = open(os.path.join(ROOT, "include", "mcpc.h")).read()
    assert re.search(r"\bint\s+mcpc_cov_accumulate\s*\(", header)
    assert re.search(r"\bint64_t\s+mcpc_cov_workspace_bytes\s*\(", header)
    assert re.search(r"#define\s+MCPC_ABI_VERSION\s+4\b", header) and _lib.ABI_VERSION == 4
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("mcpc_cov_accumulate", "mcpc_cov_workspace_bytes"):
        decl = re.search(name + r"\s*\(([^)]*)\)", code).group(1)
        res, args = _lib.SYMBOLS[name]
        assert len(args) == len(decl.split(",")), name
    assert len(_lib.SYMBOLS["mcpc_cov_accumulate"][1]) == 15 and len(_lib.SYMBOLS["mcpc_cov_workspace_bytes"][1]) == 4
    lib = _lib.load()
    assert lib.mcpc_abi_version() == 4 and hasattr(lib, "mcpc_cov_accumulate")
    # no device work: the size of the pooled workspace is host arithmetic, [groups][Dpad][Dpad] fp64, and depends on B and the widths alone
    import ctypes as C
    w = (C.c_int32 * 3)(15, 1, 33)
    need = lib.mcpc_cov_workspace_bytes(70, w, 3, 1)
    assert need > 0 and need % (8 * 80 * 80) == 0 and need == lib.mcpc_cov_workspace_bytes(70, w, 3, 1)
    assert lib.mcpc_cov_workspace_bytes(70, w, 3, 0) == 0
    assert lib.mcpc_cov_workspace_bytes(70, w, 0, 1) == -1 and b"n_blocks=0" in lib.mcpc_last_error()
    # one launch holds every job (64 lanes each, fewer than 2^32 threads): 2^26 chains, one matrix each, are refused by name
    one = (C.c_int32 * 1)(8)                                 # (one tile: one job per chain)
    assert lib.mcpc_cov_workspace_bytes((1 << 26) - 1, one, 1, 0) == 0
    assert lib.mcpc_cov_workspace_bytes(1 << 26, one, 1, 0) == -1 and b"jobs" in lib.mcpc_last_error()

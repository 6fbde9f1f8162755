"""Prediction errors and predictions of recorded states, host side (no GPU): the `mcpc_errors` request, which steps are samples however
the call is sliced, the byte bound, the fp64 arithmetic from sums to mean / var / rms, merging, and the C entry point's declaration,
binding and the one argument check that needs no engine."""
import ctypes as C
import os
import re

import pytest
import torch

from montecarlopredictivecoding_amd import _lib
from montecarlopredictivecoding_amd import errors as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (6, 33, 16)
KW = dict(T=60, n_layers=3, n_out=24, sizes=SIZES, B=37, has_loss=True, max_bytes=2 << 30)


def test_defaults_and_columns():
    spec = E.validate_spec(dict(layers=(1,)), **KW)
    assert (spec.begin, spec.stride, spec.layers, spec.quantity, spec.outputs, spec.variance, spec.covariance, spec.T, spec.n) == \
        (0, 1, (1,), "error", None, True, None, 60, 60)
    assert spec.columns == (("e1", 0, 33),) and spec.D == 33 and spec.reads == (0, 1) and not spec.pooled
    spec = E.validate_spec(dict(begin=13, stride=3, layers=(2, 0, 2), quantity="prediction", outputs="error", covariance="chains"), **KW)
    assert spec.layers == (0, 2) and spec.n == len(range(13, 60, 3)) == 16 and spec.pooled
    assert spec.columns == (("mu0", 0, 6), ("mu2", 6, 16), ("eout", 22, 24)) and spec.reads == (0, 1, 2)
    spec = E.validate_spec(dict(outputs="prediction", variance=False, covariance="chain"), **KW)       # the read-out alone
    assert spec.layers == () and spec.columns == (("out", 0, 24),) and spec.reads == (2,) and not spec.variance and not spec.pooled
    assert E.validate_spec(dict(layers=0), **KW).reads == (0,)                                           # layer 0 reads no layer below
    assert E.validate_spec(dict(layers=2, outputs="prediction"), **dict(KW, has_loss=False)).columns == (("e2", 0, 16), ("out", 16, 24))


@pytest.mark.parametrize("spec, word", [
    ([("begin", 0)], "expected a dict"),
    (dict(layers=(0,), strid=2), "unknown keys"),
    (dict(layers=(0,), pool="chains"), "unknown keys"),
    (dict(layers=(0,), begin=-1), "begin"),
    (dict(layers=(0,), begin=60), "begin"),
    (dict(layers=(0,), begin=1.0), "begin must be an int"),
    (dict(layers=(0,), begin=True), "begin must be an int"),
    (dict(layers=(0,), stride=0), "stride"),
    (dict(layers=(0,), stride="2"), "stride must be an int"),
    (dict(layers=(0, 3)), "layer index"),
    (dict(layers=(-1,)), "layer index"),
    (dict(layers=(True,)), "layer index"),
    (dict(layers=1.5), "sequence of layer indices"),
    (dict(), "no columns"),
    (dict(layers=()), "no columns"),
    (dict(layers=(0,), quantity="both"), "quantity"),
    (dict(layers=(0,), quantity=None), "quantity"),
    (dict(outputs="sigmoid"), "outputs"),
    (dict(layers=(0,), covariance="pool"), "covariance"),
    (dict(layers=(0,), covariance=True), "covariance"),
])
def test_invalid_requests_are_value_errors(spec, word):
    with pytest.raises(ValueError, match=word):
        E.validate_spec(spec, **KW)


def test_outputs_need_a_read_out_and_its_error_needs_a_loss():
    for outputs in ("error", "prediction"):
        with pytest.raises(ValueError, match="read-out"):
            E.validate_spec(dict(outputs=outputs), **dict(KW, n_layers=2, n_out=0))
    with pytest.raises(ValueError, match="without a loss"):
        E.validate_spec(dict(layers=(0,), outputs="error"), **dict(KW, has_loss=False))
    assert E.validate_spec(dict(outputs="prediction"), **dict(KW, has_loss=False)).outputs == "prediction"
    assert E.validate_spec(dict(layers=(1,)), **dict(KW, n_layers=2, n_out=0)).layers == (1,)


def test_the_byte_bound_covers_derived_buffers_sums_and_covariance():
    B, D = 37, 6 + 33 + 24
    spec = dict(layers=(0, 1), outputs="error")
    sums = 8 * B * D * 2
    assert E.request_bytes(D, B, 1, True, None) == 4 * B * D + sums
    assert E.request_bytes(D, B, 9, False, None) == 4 * 9 * B * D + sums // 2
    assert E.request_bytes(D, B, 9, True, "chain") == 4 * 9 * B * D + sums + 8 * (D * D + D) * B
    assert E.request_bytes(D, B, 9, True, "chains") == 4 * 9 * B * D + sums + 8 * (D * D + D)
    # validation bounds the request with derived buffers of ONE sample; the trainer checks again with the samples of a slice
    need = 4 * B * D + sums + 8 * (D * D + D) * B
    ok = E.validate_spec(dict(spec, covariance="chain"), **dict(KW, max_bytes=need))
    assert ok.bytes(B, 1) == need
    with pytest.raises(ValueError, match=r"63 columns x 37 chains.*derived records of 1 sample, sums, covariance\) takes 1.2 MiB.*mcpc_errors_max_bytes.*fewer layers or covariance='chains'"):
        E.validate_spec(dict(spec, covariance="chain"), **dict(KW, max_bytes=need - 1))
    assert E.validate_spec(dict(spec, covariance="chains"), **dict(KW, max_bytes=need - 1)).pooled
    E.check_bytes(ok, B, 1, need)
    with pytest.raises(ValueError, match="derived records of 20 samples"):
        E.check_bytes(ok, B, 20, need + 4 * 19 * B * D - 1)
    E.check_bytes(ok, B, 20, need + 4 * 19 * B * D)
    # a slice of S steps holds at most ceil(S / stride) samples, and never more than the call has
    s = E.validate_spec(dict(layers=(0,), begin=7, stride=3), **dict(KW, T=40))
    assert s.n == 11 and [s.max_samples(S) for S in (1, 3, 4, 12, 40, 400)] == [1, 1, 2, 4, 11, 11]


@pytest.mark.parametrize("begin, stride, T", [(0, 1, 1), (7, 3, 40), (59, 7, 60), (200, 1, 1000), (3, 4, 5), (0, 60, 60)])
def test_sample_count_and_chunks(begin, stride, T):
    spec = E.validate_spec(dict(layers=(0,), begin=begin, stride=stride), **dict(KW, T=T))
    steps = list(range(begin, T, stride))
    assert spec.n == len(steps)
    for S in (1, 5, 7, T):                               # however the call is sliced, the chunks name exactly the sample steps, in order
        got = []
        for t0 in range(0, T, S):
            n = min(S, T - t0)
            first, cnt = spec.chunk(t0, n)
            assert cnt <= spec.max_samples(n)
            assert cnt == 0 or (0 <= first and first + (cnt - 1) * stride < n)
            got += [t0 + first + k * stride for k in range(cnt)]
        assert got == steps


def test_result_arithmetic_and_merge():
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn(9, 4, 5, generator=g, dtype=torch.float64), torch.randn(6, 4, 5, generator=g, dtype=torch.float64) + 2.0

    def result(v):
        return E.Errors(n=v.shape[0], sum={"e1": v.sum(0)}, sumsq={"e1": (v * v).sum(0)})
    r = result(a)
    assert r.names == ["e1"]
    torch.testing.assert_close(r.mean("e1"), a.mean(0), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(r.var("e1"), a.var(0, unbiased=True), rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(r.var("e1", ddof=0), a.var(0, unbiased=False), rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(r.rms("e1"), (a * a).mean(0).sqrt(), rtol=1e-13, atol=1e-13)
    both = r.merge(result(b))
    ab = torch.cat([a, b])
    assert both.n == 15
    torch.testing.assert_close(both.mean("e1"), ab.mean(0), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(both.var("e1"), ab.var(0, unbiased=True), rtol=1e-12, atol=1e-13)
    assert torch.isnan(result(a[:1]).var("e1")).all()
    with pytest.raises(KeyError, match="no block 'e0'"):
        r.mean("e0")
    lean = E.Errors(n=9, sum={"e1": a.sum(0)}, sumsq={"e1": None})
    with pytest.raises(ValueError, match="variance=False"):
        lean.rms("e1")
    assert lean.merge(lean).sumsq["e1"] is None
    with pytest.raises(ValueError, match="different requests"):
        r.merge(E.Errors(n=1, sum={"mu1": a[0]}, sumsq={"mu1": a[0]}))


def test_the_trainer_has_the_opt_in_attributes_and_they_are_off():
    import montecarlopredictivecoding_amd.predictive_coding as pc
    model = torch.nn.Sequential(torch.nn.Linear(2, 2), pc.PCLayer(), torch.nn.Linear(2, 3))
    tr = pc.PCTrainer(model, T=4, plot_progress_at=[])
    assert tr.mcpc_errors is None and tr.mcpc_last_errors is None and tr.mcpc_errors_max_bytes == 2 << 30
    assert tr.mcpc_errors_max_bytes == tr.mcpc_covariance_max_bytes == tr.mcpc_rolling_max_bytes
    assert callable(tr.mcpc_state_errors)
    import montecarlopredictivecoding_amd.utils.model as um
    assert callable(um.get_posterior_error_statistics)
    from montecarlopredictivecoding_amd.engine import Engine
    assert callable(Engine.prediction_errors)


def _args(text, name):
    """The parameter list of `name` in C text, comments removed: [(type, identifier)]."""
    code = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1)
    out = []
    for a in decl.split(","):
        a = " ".join(a.split())
        m = re.match(r"(.*?)(\w+)$", a)
        out.append((m.group(1).replace(" ", ""), m.group(2).rstrip("_")))
    return out


def test_header_source_and_binding_agree_on_the_signature():
    header = open(os.path.join(ROOT, "include", "mcpc.h")).read()
    source = open(os.path.join(ROOT, "montecarlopredictivecoding_amd", "csrc", "mcpc_eval.hip")).read()       # the unit of the evaluators
    assert re.search(r"#define\s+MCPC_ABI_VERSION\s+4\b", header) and _lib.ABI_VERSION == 4
    name = "mcpc_prediction_errors"
    h, s = _args(header, name), _args(source, name)
    assert h == s and len(h) == 13
    assert [i for _, i in h] == ["e", "inputs", "x_rec", "n_rec", "loss_kind", "loss_var", "mask_start", "err", "pred", "err_out", "pred_out",
                                 "max_rows", "stream"]
    restype, argtypes = _lib.SYMBOLS[name]
    assert restype is C.c_int and len(argtypes) == 13
    scalar = {"int32_t": C.c_int32, "double": C.c_double}
    for (t, ident), a in zip(h, argtypes):
        if t.endswith("*const*"):
            assert a is C.POINTER(C.c_void_p), (ident, t)
        elif t.endswith("*"):
            assert a is C.c_void_p, (ident, t)
        else:
            assert a is scalar[t], (ident, t)
    lib = _lib.load()
    assert lib.mcpc_abi_version() == 4 and hasattr(lib, name)


def test_a_null_engine_is_refused_before_any_device_work():
    lib = _lib.load()
    p = C.c_void_p(0x1000)                                               # never dereferenced: the call is refused
    arr = (C.c_void_p * 3)(p, p, p)
    rc = lib.mcpc_prediction_errors(None, p, arr, 1, 0, 1.0, 0, arr, None, None, None, 0, None)
    assert rc == -1 and "prediction errors: null engine" in lib.mcpc_last_error().decode()

"""The posterior of a linear probe, host side (no GPU): the `mcpc_probe` request, the sample count, the fp64 arithmetic on the sums, and
the C entry point's declaration, binding and argument checks."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from montecarlopredictivecoding_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (6, 16, 16)
KW = dict(T=60, n_layers=3, sizes=SIZES, B=37)
W0 = torch.arange(30, dtype=torch.float32).reshape(5, 6)


def _P():
    from montecarlopredictivecoding_amd import probe
    return probe


def test_defaults():
    P = _P()
    spec = P.validate_spec(dict(layer=0, weight=W0), **KW)
    assert (spec.begin, spec.stride, spec.layer, spec.link, spec.T, spec.C, spec.n) == (0, 1, 0, "softmax", 60, 5, 60)
    assert spec.bias is None and torch.equal(spec.weight, W0)
    lin = torch.nn.Linear(16, 10)
    spec = P.validate_spec(dict(begin=13, stride=3, layer=2, linear=lin, link="sigmoid"), **KW)
    assert (spec.layer, spec.C, spec.link, spec.n) == (2, 10, "sigmoid", len(range(13, 60, 3)))
    assert not spec.weight.requires_grad and torch.equal(spec.weight, lin.weight.detach()) and torch.equal(spec.bias, lin.bias.detach())
    w, b = spec.on("cpu")
    assert w.dtype == b.dtype == torch.float32 and w.is_contiguous() and tuple(w.shape) == (10, 16)
    spec = P.validate_spec(dict(layer=1, weight=torch.zeros(64, 16, dtype=torch.float64).t().contiguous().t(),
                                bias=torch.zeros(64), link="identity"), **KW)
    w, _ = spec.on("cpu")
    assert spec.C == 64 and w.dtype == torch.float32 and w.is_contiguous()
    assert P.MAX_CLASSES == _lib.PROBE_MAX_CLASSES == 64
    assert (_lib.PROBE_IDENTITY, _lib.PROBE_SIGMOID, _lib.PROBE_SOFTMAX) == (0, 1, 2)


@pytest.mark.parametrize("spec, word", [
    ([("layer", 0)], "expected a dict"),
    (dict(layer=0, weight=W0, strid=2), "unknown keys"),
    (dict(layer=0, weight=W0, begin=-1), "begin"),
    (dict(layer=0, weight=W0, begin=60), "begin"),
    (dict(layer=0, weight=W0, begin=1.0), "begin must be an int"),
    (dict(layer=0, weight=W0, begin=True), "begin must be an int"),
    (dict(layer=0, weight=W0, stride=0), "stride"),
    (dict(layer=0, weight=W0, stride="2"), "stride must be an int"),
    (dict(weight=W0), "layer is required"),
    (dict(layer=None, weight=W0), "layer is required"),
    (dict(layer=(0,), weight=W0), "layer must be an int"),
    (dict(layer=True, weight=W0), "layer must be an int"),
    (dict(layer=3, weight=W0), "layer index"),
    (dict(layer=-1, weight=W0), "layer index"),
    (dict(layer=0, weight=torch.zeros(6)), "2-D"),
    (dict(layer=0, weight=[[0.0] * 6]), "2-D"),
    (dict(layer=1, weight=W0), r"expected \[classes, 16\]"),
    (dict(layer=0, weight=torch.zeros(0, 6)), "outside 1..64"),
    (dict(layer=0, weight=torch.zeros(65, 6)), "65 classes, outside 1..64"),
    (dict(layer=0, weight=W0, bias=torch.zeros(6)), "bias"),
    (dict(layer=0, weight=W0, bias=torch.zeros(5, 1)), "bias"),
    (dict(layer=0, weight=W0, linear=torch.nn.Linear(6, 5)), "both linear and weight"),
    (dict(layer=0, bias=torch.zeros(5), linear=torch.nn.Linear(6, 5)), "both linear and weight"),
    (dict(layer=0), "neither linear nor weight"),
    (dict(layer=0, bias=torch.zeros(5)), "neither linear nor weight"),
    (dict(layer=0, linear=torch.nn.ReLU()), "torch.nn.Linear"),
    (dict(layer=0, weight=W0, link="tanh"), "link"),
    (dict(layer=0, weight=W0, link=None), "link"),
])
def test_invalid_requests_are_value_errors(spec, word):
    with pytest.raises(ValueError, match="mcpc_probe: .*" + word):
        _P().validate_spec(spec, **KW)


@pytest.mark.parametrize("begin, stride, T", [(0, 1, 1), (13, 3, 60), (59, 7, 60), (200, 1, 1000), (3, 4, 5), (0, 60, 60)])
def test_sample_count_and_chunks(begin, stride, T):
    spec = _P().validate_spec(dict(layer=0, weight=W0, begin=begin, stride=stride), **dict(KW, T=T))
    steps = list(range(begin, T, stride))
    assert spec.n == len(steps)
    for S in (1, 5, 7, T):                               # however the call is sliced, the chunks name exactly the sample steps, in order
        got = []
        for t0 in range(0, T, S):
            n = min(S, T - t0)
            first, cnt = spec.chunk(t0, n)
            assert cnt == 0 or (0 <= first and first + (cnt - 1) * stride < n)
            got += [t0 + first + k * stride for k in range(cnt)]
        assert got == steps


def _probe(link="softmax"):
    """Two chains, three classes, n = 4: chain 0 always (0.5, 0.5, 0), chain 1 one-hot on class 0, 1, 1, 2."""
    P = _P()
    p = torch.tensor([[[0.5, 0.5, 0.0]] * 4, [[1.0, 0, 0], [0, 1.0, 0], [0, 1.0, 0], [0, 0, 1.0]]], dtype=torch.float64)   # [B, n, C]
    votes = torch.tensor([[4, 0, 0, 0], [1, 2, 1, 0]], dtype=torch.int64)
    ent = torch.tensor([4 * math.log(2.0), 0.0], dtype=torch.float64) if link == "softmax" else None
    return P.Probe(n=4, B=2, C=3, link=link, psum=p.sum(1), psumsq=(p * p).sum(1), votes=votes, entsum=ent)


def test_probe_arithmetic_on_hand_made_sums():
    r = _probe()
    assert torch.equal(r.mean(), torch.tensor([[0.5, 0.5, 0.0], [0.25, 0.5, 0.25]], dtype=torch.float64))
    assert torch.equal(r.var(), torch.tensor([[0.0, 0.0, 0.0], [0.1875, 0.25, 0.1875]], dtype=torch.float64))
    assert torch.equal(r.var(ddof=1), r.var() * (4 / 3))
    assert torch.equal(r.vote_share(), torch.tensor([[1.0, 0, 0], [0.25, 0.5, 0.25]], dtype=torch.float64))
    assert r.predict().tolist() == [0, 1] and r.predict().dtype == torch.int64
    h = r.entropy()                                                                  # 0 log 0 = 0: no NaN from the zero probability
    assert h.dtype == torch.float64 and abs(float(h[0]) - math.log(2.0)) <= 1e-15 and abs(float(h[1]) - 1.5 * math.log(2.0)) <= 1e-15
    assert torch.equal(r.expected_entropy(), torch.tensor([math.log(2.0), 0.0], dtype=torch.float64))
    mi = r.mutual_information()
    assert bool((mi >= -1e-12).all()) and abs(float(mi[0])) <= 1e-15 and abs(float(mi[1]) - 1.5 * math.log(2.0)) <= 1e-15


def test_the_entropy_family_is_for_the_softmax_link():
    for link in ("identity", "sigmoid"):
        r = _probe(link)
        assert r.entsum is None and tuple(r.mean().shape) == (2, 3) and tuple(r.var().shape) == (2, 3)
        for f in (r.entropy, r.expected_entropy, r.mutual_information):
            with pytest.raises(ValueError, match="link is '%s'" % link):
                f()


def test_cat_and_merge():
    P = _P()
    r = _probe()
    both = P.Probe.cat([r, r])
    assert (both.n, both.B, both.C, both.link) == (4, 4, 3, "softmax")
    assert torch.equal(both.psum[2:], r.psum) and torch.equal(both.votes[:2], r.votes) and tuple(both.entsum.shape) == (4,)
    more = r.merge(r)
    assert (more.n, more.B) == (8, 2) and torch.equal(more.psum, 2 * r.psum) and torch.equal(more.votes, 2 * r.votes)
    assert torch.equal(more.mean(), r.mean()) and torch.equal(more.entsum, 2 * r.entsum)
    ident = P.Probe.cat([_probe("identity")] * 2)
    assert ident.entsum is None and ident.B == 4 and _probe("identity").merge(_probe("identity")).entsum is None
    other_n = P.Probe(n=5, B=2, C=3, link="softmax", psum=r.psum, psumsq=r.psumsq, votes=r.votes, entsum=r.entsum)
    with pytest.raises(ValueError, match="different requests"):
        P.Probe.cat([r, other_n])
    with pytest.raises(ValueError, match="different requests"):
        P.Probe.cat([r, _probe("sigmoid")])
    with pytest.raises(ValueError, match="different chains or requests"):
        r.merge(both)
    with pytest.raises(ValueError, match="different chains or requests"):
        r.merge(_probe("identity"))
    assert r.merge(other_n).n == 9                                                   # more samples of the same chains: any count


def test_the_trainer_has_the_opt_in_attributes_and_they_are_off():
    import montecarlopredictivecoding_amd.predictive_coding as pc
    model = torch.nn.Sequential(torch.nn.Linear(2, 2), pc.PCLayer(), torch.nn.Linear(2, 3))
    tr = pc.PCTrainer(model, T=4, plot_progress_at=[])
    assert tr.mcpc_probe is None and tr.mcpc_last_probe is None and callable(tr.mcpc_state_probe)
    import montecarlopredictivecoding_amd.utils.model as um
    assert callable(um.get_posterior_class_probabilities)


def test_header_declares_the_entry_point_and_the_binding_binds_it():
    header = open(os.path.join(ROOT, "include", "mcpc.h")).read()
    assert re.search(r"\bint\s+mcpc_probe_accumulate\s*\(", header)
    assert re.search(r"#define\s+MCPC_PROBE_MAX_CLASSES\s+64\b", header)
    for name, val in (("IDENTITY", 0), ("SIGMOID", 1), ("SOFTMAX", 2)):
        assert re.search(r"#define\s+MCPC_PROBE_%s\s+%d\b" % (name, val), header)
    assert re.search(r"#define\s+MCPC_ABI_VERSION\s+4\b", header) and _lib.ABI_VERSION == 4
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = re.search(r"mcpc_probe_accumulate\s*\(([^)]*)\)", code).group(1)
    res, args = _lib.SYMBOLS["mcpc_probe_accumulate"]
    assert len(args) == len(decl.split(",")) == 17 and res is C.c_int
    from montecarlopredictivecoding_amd import engine
    assert callable(engine.probe_accumulate)
    lib = _lib.load()
    assert lib.mcpc_abi_version() == 4 and hasattr(lib, "mcpc_probe_accumulate")


def test_argument_errors_are_refused_before_any_device_work():
    """Every MCPC_EINVAL case returns -1 with a message and touches no device: the pointers are never dereferenced (this machine need
    not have a GPU)."""
    lib = _lib.load()
    p = [C.c_void_p(0x1000 * (i + 1)) for i in range(7)]             # never dereferenced: every call below is refused

    def call(rec=p[0], B=3, width=5, first=0, stride=1, n=4, W=p[1], bias=p[2], n_classes=10, link=2, psum=p[3], psumsq=p[4],
             votes=p[5], entsum=p[6], accumulate=1):
        rc = lib.mcpc_probe_accumulate(0, rec, B, width, first, stride, n, W, bias, n_classes, link, psum, psumsq, votes, entsum,
                                       accumulate, None)
        return rc, lib.mcpc_last_error().decode()

    for kw, word in [(dict(rec=None), "rec is null with n=4"), (dict(W=None), "W is null"), (dict(psum=None), "psum is null"),
                     (dict(votes=None), "votes is null"), (dict(entsum=None), "entsum is null"), (dict(B=0), "B=0"),
                     (dict(width=0), "width=0"), (dict(stride=0), "stride=0"), (dict(first=-1), "first=-1"), (dict(n=-1), "n=-1"),
                     (dict(n_classes=0), "n_classes=0"), (dict(n_classes=65), "n_classes=65"), (dict(link=3), "unknown link 3"),
                     (dict(link=-1), "unknown link -1"), (dict(link=3, entsum=None), "unknown link 3")]:
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("probe:") and word in msg, (kw, rc, msg)
    # nothing to add: accepted without a device, and nothing is read; entsum and psumsq are not needed by the other links
    assert call(n=0, rec=None)[0] == 0
    assert call(n=0, rec=None, link=0, entsum=None, psumsq=None, bias=None)[0] == 0
    assert call(n=0, rec=None, link=1, entsum=None)[0] == 0

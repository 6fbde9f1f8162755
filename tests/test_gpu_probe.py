"""The linear probe on the device, the kernel: `engine.probe_accumulate` against the numpy reference on the same fp32 data
(tests/probe_cases.py).  The logits are bitwise the sequential fp64 loop, so with the identity link psum, psumsq and votes are compared
BITWISE and the votes of every link are; the softmax probabilities and entropies are held to the bounds derived in tests/probe_cases.py
(per sample |p - p_ref| <= (C + 16) 2^-24 against the fp64 softmax of the same fp32 logits; the entropy bound `h_bound`), which rest on
the header's arithmetic and were written before the kernel first ran.  The records sit at FIRST + j * STRIDE of a buffer whose other
rows are NaN."""
import numpy as np
import pytest
import torch

from tests import probe_cases as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIRST, STRIDE = 2, 3
BS = (1, 3, 37)
NS = (1, 8, 9, 37)                       # both sides of the block of 8 samples
# 64 | 65: W resident in one k-tile of 64 columns | restaged per block; 128 | 129: two | three tiles
WIDTHS = (1, 5, 20, 33, 64, 65, 128, 129)
CLASSES = (1, 2, 3, 10, 16, 17, 64)      # every Cpad 1..64, at and above a power of two
LINKS = ("identity", "sigmoid", "softmax")


def _records(g):
    """fp32 [n, B, w] samples -> a record buffer on the device whose rows FIRST + j * STRIDE are the samples; every other row NaN."""
    n = g.shape[0]
    rec = torch.full((FIRST + STRIDE * max(n - 1, 0) + 2,) + tuple(g.shape[1:]), float("nan"), dtype=torch.float32, device=DEV)
    if n:
        rec[FIRST:FIRST + STRIDE * (n - 1) + 1:STRIDE] = torch.from_numpy(g).to(DEV)
    return rec


def _state(B, C, link, poison=True):
    """Outputs of a call; poisoned, so that an overwriting call shows what it leaves alone."""
    f = float("nan") if poison else 0.0
    return dict(psum=torch.full((B, C), f, dtype=torch.float64, device=DEV), psumsq=torch.full((B, C), f, dtype=torch.float64, device=DEV),
                votes=torch.full((B, C + 1), -7 if poison else 0, dtype=torch.int64, device=DEV),
                entsum=torch.full((B,), f, dtype=torch.float64, device=DEV) if link == "softmax" else None)


def _feed(rec, st, W, bias, link, chunks, offset=0, accumulate=False):
    from montecarlopredictivecoding_amd.engine import probe_accumulate
    for c in chunks:
        probe_accumulate(rec, FIRST + STRIDE * offset, STRIDE, c, W, bias, link, st["psum"], st["psumsq"], st["votes"], st["entsum"],
                         accumulate=accumulate)
        offset += c
        accumulate = True
    return st


def _np(st):
    return {k: (None if t is None else t.cpu().numpy()) for k, t in st.items()}


def _same_bits(a, b):
    for k in a:
        if a[k] is not None:
            assert torch.equal(a[k].view(torch.int64), b[k].view(torch.int64)), k


def _data(B, w, C, n, seed):
    rng = np.random.default_rng(seed)
    g = (rng.standard_normal((n, B, w)) * 1.5 + 0.3).astype(np.float32)
    W = (rng.standard_normal((C, w)) / np.sqrt(w)).astype(np.float32)
    b = (rng.standard_normal(C) * 0.5).astype(np.float32)
    return g, W, b


def _sigmoid_of(v):
    return R.device_sigmoid(v, DEV)


def _check(got, v, link, C, n, what, sig=None):
    """`got` (numpy outputs of n samples whose fp32 logits are v [n, B, C]) against the reference; `sig`: `_sigmoid_of(v)` if at hand."""
    assert np.array_equal(got["votes"], R.votes(v)), ("votes", what)
    assert (got["votes"].sum(axis=1) == n).all(), ("votes add up to n", what)
    if link == "identity":
        s, q = R.sums(v)
        assert np.array_equal(got["psum"], s, equal_nan=True) and np.array_equal(got["psumsq"], q, equal_nan=True), what
    elif link == "sigmoid":
        s, q = R.sums(_sigmoid_of(v) if sig is None else sig)
        assert np.array_equal(got["psum"], s) and np.array_equal(got["psumsq"], q), what
    else:
        p, H = R.softmax64(v)
        ep = np.abs(got["psum"] - p.sum(axis=0)).max()
        eq = np.abs(got["psumsq"] - (p * p).sum(axis=0)).max()
        eh = np.abs(got["entsum"] - H.sum(axis=0)).max()
        print("%s: |psum - ref| = %.3g (bound %.3g), |psumsq - ref| = %.3g, |entsum - ref| = %.3g (bound %.3g)"
              % (what, ep, n * R.p_bound(C), eq, eh, n * R.h_bound(C)))
        assert ep <= n * R.p_bound(C) and eq <= 2 * n * R.p_bound(C) and eh <= n * R.h_bound(C), what


@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("w", WIDTHS)
def test_every_shape_against_the_reference(w, C):
    """One reference per (width, classes): the logits of 37 samples of 37 chains; fewer chains and samples are slices of it."""
    g, W, b = _data(37, w, C, 37, seed=1000 * w + C)
    v = R.logits(g, W, b)
    sig = _sigmoid_of(v)
    Wd, bd = torch.from_numpy(W).to(DEV), torch.from_numpy(b).to(DEV)
    for B in BS:
        for n in NS:
            rec = _records(np.ascontiguousarray(g[:n, :B]))
            for link in LINKS:
                st = _feed(rec, _state(B, C, link), Wd, bd, link, [n])
                _check(_np(st), v[:n, :B], link, C, n, f"B={B} w={w} C={C} n={n} {link}", sig=sig[:n, :B])
                if n == 37:                                  # 1 + 5 + 31 with accumulate = 1: the same bits in every output
                    _same_bits(_feed(rec, _state(B, C, link), Wd, bd, link, [1, 5, 31]), st)


@pytest.mark.parametrize("C", CLASSES)
def test_softmax_per_sample(C):
    """One sample per call: psum is p, psumsq its exact square, entsum the sample's entropy, votes the one-hot argmax."""
    B, w, n = 37, 20, 9
    g, W, b = _data(B, w, C, n, seed=77 + C)
    g *= 3                                                   # logits a few units apart: probabilities from 1e-6 to almost 1
    v = R.logits(g, W, b)
    p, H = R.softmax64(v)
    rec = _records(g)
    Wd, bd = torch.from_numpy(W).to(DEV), torch.from_numpy(b).to(DEV)
    worst_p = worst_h = 0.0
    for j in range(n):
        got = _np(_feed(rec, _state(B, C, "softmax"), Wd, bd, "softmax", [1], offset=j))
        worst_p = max(worst_p, np.abs(got["psum"] - p[j]).max())
        worst_h = max(worst_h, np.abs(got["entsum"] - H[j]).max())
        p32 = got["psum"].astype(np.float32)
        assert np.array_equal(p32.astype(np.float64), got["psum"])                        # an fp32 value, added to 0
        assert np.array_equal(got["psumsq"], got["psum"] * got["psum"])
        assert np.array_equal(got["votes"], R.votes(v[j:j + 1]))
        assert np.abs(got["psum"].sum(axis=1) - 1).max() <= C * R.p_bound(C)
    print("C=%d: max |p - p_ref| = %.3g (bound %.3g), max |H - H_ref| = %.3g (bound %.3g)"
          % (C, worst_p, R.p_bound(C), worst_h, R.h_bound(C)))
    assert worst_p <= R.p_bound(C) and worst_h <= R.h_bound(C)


def test_a_row_of_many_workgroups():
    """2051 chains x 16 class lanes: 513 workgroups, the last one with 3 chains of 4."""
    B, w, C, n = 2051, 20, 10, 9
    g, W, b = _data(B, w, C, n, seed=5)
    v = R.logits(g, W, b)
    rec = _records(g)
    Wd, bd = torch.from_numpy(W).to(DEV), torch.from_numpy(b).to(DEV)
    for link in ("identity", "softmax"):
        st = _feed(rec, _state(B, C, link), Wd, bd, link, [4, 5])
        _check(_np(st), v, link, C, n, f"B={B} {link}")


def test_exact_ties_go_to_the_lowest_index():
    B, w, C, n = 5, 7, 6, 12
    g, W, b = _data(B, w, C, n, seed=11)
    W[4], b[4] = W[1], b[1]                                  # classes 1 and 4 always tie, bitwise
    W[5], b[5] = W[0], b[0]
    v = R.logits(g, W, b)
    assert np.array_equal(v[..., 1], v[..., 4])
    for link in LINKS:
        got = _np(_feed(_records(g), _state(B, C, link), torch.from_numpy(W).to(DEV), torch.from_numpy(b).to(DEV), link, [n]))
        assert np.array_equal(got["votes"], R.votes(v))
        assert (got["votes"][:, 4:] == 0).all() and got["votes"][:, :2].sum() > 0
    # all logits equal (W = 0): class 0 takes every vote, the softmax is uniform and its entropy log C within the bound
    Z = torch.zeros(C, w, device=DEV)
    got = _np(_feed(_records(g), _state(B, C, "softmax"), Z, None, "softmax", [n]))
    assert (got["votes"][:, 0] == n).all() and (got["votes"][:, 1:] == 0).all()
    assert np.abs(got["psum"] - n / C).max() <= n * R.p_bound(C) and np.abs(got["entsum"] - n * np.log(C)).max() <= n * R.h_bound(C)


def test_logits_of_ten_thousand():
    B, w, C, n = 3, 5, 10, 9
    g, W, b = _data(B, w, C, n, seed=13)
    W *= 1e4
    v = R.logits(g, W, b)
    assert np.abs(v).max() > 1e4
    got = _np(_feed(_records(g), _state(B, C, "softmax"), torch.from_numpy(W).to(DEV), torch.from_numpy(b).to(DEV), "softmax", [n]))
    assert np.isfinite(got["psum"]).all() and np.isfinite(got["psumsq"]).all() and np.isfinite(got["entsum"]).all()
    assert np.abs(got["psum"].sum(axis=1) - n).max() <= n * C * R.p_bound(C)
    _check(got, v, "softmax", C, n, "1e4")


@pytest.mark.parametrize("w", [5, 65])
def test_one_class(w):
    B, n = 7, 9
    g, W, b = _data(B, w, 1, n, seed=17)
    got = _np(_feed(_records(g), _state(B, 1, "softmax"), torch.from_numpy(W).to(DEV), torch.from_numpy(b).to(DEV), "softmax", [n]))
    assert (got["psum"] == n).all() and (got["psumsq"] == n).all() and (got["entsum"] == 0).all()
    assert (got["votes"][:, 0] == n).all() and (got["votes"][:, 1] == 0).all()


@pytest.mark.parametrize("link", LINKS)
def test_special_values_stay_in_their_chain(link):
    """A NaN in one sample of chain 3 and a +Inf in one sample of chain 20."""
    B, w, C, n = 37, 20, 10, 12
    g, W, b = _data(B, w, C, n, seed=19)
    bad = g.copy()
    bad[4, 3, 11] = np.nan
    bad[9, 20, 0] = np.inf
    Wd, bd = torch.from_numpy(W).to(DEV), torch.from_numpy(b).to(DEV)
    clean = _feed(_records(g), _state(B, C, link), Wd, bd, link, [n])
    hit = _feed(_records(bad), _state(B, C, link), Wd, bd, link, [3, 9])
    v = R.logits(bad, W, b)
    got = _np(hit)
    assert np.array_equal(got["votes"], R.votes(v))
    assert got["votes"][3, C] == 1 and got["votes"][3, :C].sum() == n - 1             # the NaN sample casts no vote
    assert got["votes"][:, C].sum() == 1 and got["votes"][20].sum() == n              # +-Inf logits and no NaN: it votes
    assert np.isnan(got["psum"][3]).all() and np.isnan(got["psumsq"][3]).all()       # every logit of the sample is NaN
    if link == "identity":
        s, q = R.sums(v)
        assert np.array_equal(got["psum"], s, equal_nan=True) and np.array_equal(got["psumsq"], q, equal_nan=True)
        assert np.isinf(got["psum"][20]).all()
    if link == "softmax":
        assert np.isnan(got["entsum"][3]) and np.isnan(got["psum"][20]).all()        # Inf - Inf in the chain that holds it
    keep = torch.ones(B, dtype=torch.bool, device=DEV)
    keep[3] = keep[20] = False
    for k in clean:
        if clean[k] is not None:
            assert torch.equal(hit[k][keep], clean[k][keep]), k                       # every other chain: the bits of the clean run


@pytest.mark.parametrize("link", LINKS)
def test_no_bias_is_a_zero_bias(link):
    B, w, C, n = 5, 33, 17, 9
    g, W, _ = _data(B, w, C, n, seed=23)
    rec, Wd = _records(g), torch.from_numpy(W).to(DEV)
    none = _feed(rec, _state(B, C, link), Wd, None, link, [n])
    _same_bits(none, _feed(rec, _state(B, C, link), Wd, torch.zeros(C, device=DEV), link, [n]))


def test_psumsq_is_optional_and_an_empty_call_zeroes():
    from montecarlopredictivecoding_amd.engine import probe_accumulate
    B, w, C, n = 5, 20, 10, 9
    g, W, b = _data(B, w, C, n, seed=29)
    rec, Wd, bd = _records(g), torch.from_numpy(W).to(DEV), torch.from_numpy(b).to(DEV)
    full = _feed(rec, _state(B, C, "softmax"), Wd, bd, "softmax", [n])
    st = _state(B, C, "softmax")
    probe_accumulate(rec, FIRST, STRIDE, n, Wd, bd, "softmax", st["psum"], None, st["votes"], st["entsum"], accumulate=False)
    assert torch.equal(st["psum"], full["psum"]) and torch.equal(st["entsum"], full["entsum"]) and bool(torch.isnan(st["psumsq"]).all())
    before = {k: t.clone() for k, t in full.items()}
    _feed(rec, full, Wd, bd, "softmax", [0], accumulate=True)                        # nothing to add
    _same_bits(full, before)
    _feed(rec, full, Wd, bd, "softmax", [0])                                         # an overwriting empty call
    assert all(bool((t == 0).all()) for t in full.values())


def test_the_binding_checks_its_tensors():
    from montecarlopredictivecoding_amd.engine import probe_accumulate
    B, w, C = 3, 5, 4
    g, W, b = _data(B, w, C, 6, seed=1)
    rec = _records(g)
    base = dict(_state(B, C, "softmax", poison=False), W=torch.from_numpy(W).to(DEV), bias=torch.from_numpy(b).to(DEV))

    def call(n=6, link="softmax", **kw):
        a = dict(base, **kw)
        probe_accumulate(rec, FIRST, STRIDE, n, a["W"], a["bias"], link, a["psum"], a["psumsq"], a["votes"], a["entsum"])
    with pytest.raises(ValueError, match="last one asked for"):
        call(n=7)
    with pytest.raises(ValueError, match="link"):
        call(link="tanh")
    with pytest.raises(ValueError, match="W: expected shape"):
        call(W=torch.zeros(C, w + 1, device=DEV))
    with pytest.raises(ValueError, match="65 classes"):
        call(W=torch.zeros(65, w, device=DEV))
    with pytest.raises(ValueError, match="bias: expected shape"):
        call(bias=torch.zeros(C + 1, device=DEV))
    with pytest.raises(TypeError, match="psum: expected torch.float64"):
        call(psum=torch.zeros(B, C, device=DEV))
    with pytest.raises(ValueError, match="votes: expected shape"):
        call(votes=torch.zeros(B, C, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="psumsq: expected device"):
        call(psumsq=torch.zeros(B, C, dtype=torch.float64))
    with pytest.raises(TypeError, match="entsum"):
        call(entsum=None)
    with pytest.raises(ValueError, match="entsum"):
        call(link="identity")
    call()
    assert float(base["psum"].sum()) > 0

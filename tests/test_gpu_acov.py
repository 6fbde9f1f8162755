"""Lagged products on the device, the kernel: `engine.acov_accumulate` against the sequential fp64 host loop on the same fp32 data
(tests/acov_cases.py).  A product of two fp32 values is exact in fp64 and one thread walks an element's samples in order, so lagged,
sum, head and the final window are compared BITWISE, whatever the shape, the capacity instantiated, and the chunking of the stream."""
import numpy as np
import pytest
import torch

from tests.acov_cases import ref_stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIRST, STRIDE = 2, 3
SHAPES = [(3, 5), (4, 8), (5, 52)]       # E odd: scalar loads, a partial wave; vector loads; two workgroups with a tail
LAGS = [0, 1, 5, 8, 9, 32, 33, 64]       # both sides of every capacity (8, 16, 32, 64)
BIG = (2051, 257)                        # E = 527107: 2060 workgroups of 256 threads (beyond 64 Ki elements), scalar form


def _records(g):
    """fp32 [n, B, w] samples -> a record buffer on the device whose rows FIRST + j * STRIDE are the samples; every other row NaN."""
    n = g.shape[0]
    rec = torch.full((FIRST + STRIDE * max(n - 1, 0) + 2,) + tuple(g.shape[1:]), float("nan"), dtype=torch.float32, device=DEV)
    if n:
        rec[FIRST:FIRST + STRIDE * (n - 1) + 1:STRIDE] = torch.from_numpy(g).to(DEV)
    return rec


def _state(B, w, K, poison=False):
    fill = float("nan") if poison else 0.0
    return dict(lagged=torch.full((B, w, K + 1), fill, dtype=torch.float64, device=DEV),
                sum=torch.full((B, w), fill, dtype=torch.float64, device=DEV),
                window=torch.full((K, B, w), fill, dtype=torch.float32, device=DEV),
                head=torch.full((K, B, w), fill, dtype=torch.float32, device=DEV))


def _feed(rec, st, K, chunks, transform="identity", n_seen=0, offset=0):
    """Feed samples offset .. of `rec` to the stream `st` as calls of `chunks` samples each."""
    from montecarlopredictivecoding_amd.engine import acov_accumulate
    for c in chunks:
        acov_accumulate(rec, FIRST + STRIDE * offset, STRIDE, c, K, n_seen, st["lagged"], st["sum"], st["window"], st["head"],
                        transform=transform)
        n_seen += c
        offset += c
    return n_seen


def _check(st, want, K, what=""):
    """Bitwise, NaN equal to NaN; head and window in their valid rows."""
    lag, s, head, win = want
    B, w = st["sum"].shape
    v = head.shape[0]
    got = {k: t.cpu().numpy() for k, t in st.items()}
    assert np.array_equal(got["lagged"].reshape(-1, K + 1), lag, equal_nan=True), ("lagged", what)
    assert np.array_equal(got["sum"].reshape(-1), s, equal_nan=True), ("sum", what)
    assert np.array_equal(got["head"][:v].reshape(v, B * w), head, equal_nan=True), ("head", what)
    assert np.array_equal(got["window"][:v].reshape(v, B * w), win, equal_nan=True), ("window", what)


def _samples(B, w, n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, B, w)) * 1.5 + 0.7).astype(np.float32)


def _counts(K):
    return sorted({m for m in (1, K - 1, K, K + 1, 3 * K + 2) if m >= 1})


@pytest.mark.parametrize("K", LAGS)
@pytest.mark.parametrize("B, w", SHAPES)
def test_one_call_is_the_host_loop_bitwise(B, w, K):
    g = _samples(B, w, 3 * K + 2, seed=K)
    rec = _records(g)
    want = ref_stream(g.reshape(g.shape[0], -1), K, stops=_counts(K))
    for n in _counts(K):
        st = _state(B, w, K)
        _feed(rec, st, K, [n])
        _check(st, want[n], K, what=f"n={n}")
        v = min(K, n)
        assert bool((st["head"][v:] == 0).all()) and bool((st["window"][v:] == 0).all())      # slots not valid yet are left alone


@pytest.mark.parametrize("K", LAGS)
@pytest.mark.parametrize("B, w", SHAPES)
def test_chunked_stream_equals_the_single_call_bitwise(B, w, K):
    n = max(3 * K + 2, 2 * K + 8)
    g = _samples(B, w, n, seed=100 + K)
    rec = _records(g)
    whole, cut = _state(B, w, K), _state(B, w, K)
    _feed(rec, whole, K, [n])
    chunks = [c for c in (1, 1, 2, K - 1, K + 3) if c > 0]
    chunks.append(n - sum(chunks))
    assert chunks[-1] > 0
    seen = _feed(rec, cut, K, chunks[:3])
    before = {k: t.clone() for k, t in cut.items()}
    _feed(rec, cut, K, [0], n_seen=seen, offset=seen)                                # n = 0 mid-stream changes nothing
    assert all(torch.equal(before[k].view(torch.int32), cut[k].view(torch.int32)) for k in cut)
    assert _feed(rec, cut, K, chunks[3:], n_seen=seen, offset=seen) == n
    _check(whole, ref_stream(g.reshape(n, -1), K)[n], K)
    for k in cut:
        assert torch.equal(cut[k].view(torch.int32), whole[k].view(torch.int32)), k   # the bits, NaN payloads included


@pytest.mark.parametrize("K", [5, 33])
@pytest.mark.parametrize("B, w", SHAPES)
def test_sigmoid_is_the_moments_kernels_g(B, w, K):
    """g per row from `moments_accumulate` with n = 1 (sum = 0 + g, exact), which uses the same device function."""
    from montecarlopredictivecoding_amd.engine import moments_accumulate
    n = 3 * K + 2
    x = _samples(B, w, n, seed=200 + K) * 2
    rec = _records(x)
    g = np.empty_like(x)
    one = torch.zeros(B, w, dtype=torch.float64, device=DEV)
    for j in range(n):
        moments_accumulate(rec, FIRST + STRIDE * j, STRIDE, 1, one, None, transform="sigmoid", accumulate=False)
        g[j] = one.cpu().numpy().astype(np.float32)
    assert 0 <= g.min() and g.max() <= 1 and g.std() > 0.1
    st, cut = _state(B, w, K), _state(B, w, K)
    _feed(rec, st, K, [n], transform="sigmoid")
    _check(st, ref_stream(g.reshape(n, -1), K)[n], K)
    _feed(rec, cut, K, [2, K, n - K - 2], transform="sigmoid")
    for k in cut:
        assert torch.equal(cut[k], st[k]), k


def test_a_row_of_many_workgroups():
    B, w = BIG
    K, n = 3, 12                                                                     # the first K one at a time, a block of 8, one more
    rng = np.random.default_rng(7)
    g = rng.standard_normal((n, B, w), dtype=np.float32)
    rec = _records(g)
    st = _state(B, w, K, poison=True)
    _feed(rec, st, K, [5, 7])
    _check(st, ref_stream(g.reshape(n, -1), K)[n], K)


@pytest.mark.parametrize("K", [8, 33])
def test_a_fresh_stream_overwrites_poisoned_state(K):
    B, w = 5, 52
    g = _samples(B, w, K + 3, seed=300)
    rec = _records(g)
    want = ref_stream(g.reshape(K + 3, -1), K, stops=[0, K + 3])
    st = _state(B, w, K, poison=True)
    _feed(rec, st, K, [K + 3])
    _check(st, want[K + 3], K)
    # an empty call that starts a stream zeroes lagged and sum; window and head hold nothing valid and are left alone
    st = _state(B, w, K, poison=True)
    _feed(rec, st, K, [0])
    assert bool((st["lagged"] == 0).all()) and bool((st["sum"] == 0).all())
    assert bool(torch.isnan(st["window"]).all()) and bool(torch.isnan(st["head"]).all())
    _feed(rec, st, K, [K + 3])                                                       # still n_seen = 0
    _check(st, want[K + 3], K)


def test_an_absent_term_is_not_a_zero():
    """Inf in sample 0 of one element, n = 3, K = 8: with a zero-filled window Inf * 0 = NaN would land in the lags >= 3."""
    B, w, K, n = 4, 8, 8, 3
    g = _samples(B, w, n, seed=400)
    g[0, 1, 2] = np.inf
    st = _state(B, w, K, poison=True)
    _feed(_records(g), st, K, [n])
    want = ref_stream(g.reshape(n, -1), K)[n]
    _check(st, want, K)
    row = st["lagged"][1, 2].cpu().numpy()
    assert (row[3:] == 0.0).all() and np.isinf(row[:3]).all()
    assert bool(torch.isfinite(st["lagged"]).cpu().reshape(-1, K + 1)[torch.arange(B * w) != 10].all())
    assert bool((st["lagged"][..., 3:] == 0).all())


@pytest.mark.parametrize("K", [5, 33])
def test_a_nan_stays_in_its_element(K):
    B, w = 5, 52
    n = 3 * K + 2
    g = _samples(B, w, n, seed=500 + K)
    bad = g.copy()
    bad[K + 2, 3, 17] = np.nan
    clean, hit = _state(B, w, K), _state(B, w, K)
    _feed(_records(g), clean, K, [n])
    _feed(_records(bad), hit, K, [K, 4, n - K - 4])
    _check(hit, ref_stream(bad.reshape(n, -1), K)[n], K)
    assert bool(torch.isnan(hit["lagged"][3, 17]).all()) and bool(torch.isnan(hit["sum"][3, 17]))
    keep = torch.ones(B, w, dtype=torch.bool, device=DEV)
    keep[3, 17] = False
    assert torch.equal(hit["lagged"][keep], clean["lagged"][keep]) and torch.equal(hit["sum"][keep], clean["sum"][keep])
    assert torch.equal(hit["window"][:, keep], clean["window"][:, keep]) and torch.equal(hit["head"][:, keep], clean["head"][:, keep])
    assert int(torch.isnan(hit["lagged"]).sum()) == K + 1


def test_the_binding_checks_its_tensors():
    from montecarlopredictivecoding_amd.engine import acov_accumulate
    B, w, K = 3, 5, 4
    rec = _records(_samples(B, w, 6, seed=1))
    st = _state(B, w, K)

    def call(n=6, K=K, **kw):
        a = dict(st, **kw)
        acov_accumulate(rec, FIRST, STRIDE, n, K, 0, a["lagged"], a["sum"], a["window"], a["head"])
    with pytest.raises(ValueError, match="last one asked for"):
        call(n=7)
    with pytest.raises(ValueError, match="max_lag=65"):
        call(K=65)
    with pytest.raises(ValueError, match="lagged: expected shape"):
        call(lagged=torch.zeros(B, w, K, dtype=torch.float64, device=DEV))
    with pytest.raises(TypeError, match="sum: expected torch.float64"):
        call(sum=torch.zeros(B, w, device=DEV))
    with pytest.raises(ValueError, match="window: expected shape"):
        call(window=torch.zeros(B, w, K, device=DEV))
    with pytest.raises(ValueError, match="head: expected device"):
        call(head=torch.zeros(K, B, w))
    with pytest.raises(ValueError, match="contiguous"):
        call(lagged=torch.zeros(B, K + 1, w, dtype=torch.float64, device=DEV).transpose(1, 2))
    with pytest.raises(ValueError, match="transform"):
        acov_accumulate(rec, FIRST, STRIDE, 6, K, 0, st["lagged"], st["sum"], st["window"], st["head"], transform="tanh")
    call()
    assert float(st["sum"].abs().sum()) > 0

"""Posterior histograms on the device, the kernel: `hist_accumulate` against the numpy definition (tests/hist_cases.py), exactly.
Counts are integers: every comparison is `np.array_equal`; only the sigmoid case has values whose bin the fp32 sigmoid may decide
otherwise than the fp64 one, and it bounds them by count."""
import numpy as np
import pytest
import torch

from tests.hist_cases import ref_hist, table

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32


def _uniform(lo, hi, nb):
    return np.linspace(lo, hi, nb + 1).astype(F32)


def _nonuniform(nb, seed=4):
    """Sorted distinct fp32 normals, nb + 1 of them."""
    e = np.unique((4.0 * np.random.default_rng(seed).standard_normal(4 * nb + 8)).astype(F32))
    e = e[np.abs(e) >= 1.17549435e-38]
    e = np.sort(np.random.default_rng(seed + 1).choice(e, nb + 1, replace=False))
    assert e.size == nb + 1 and (np.diff(e) > 0).all()
    return e


EDGE_SETS = {"u1": _uniform(-1.5, 2.5, 1), "u2": _uniform(-1.5, 2.5, 2), "u19": _uniform(-1.5, 2.5, 19), "u64": _uniform(-1.5, 2.5, 64),
             "u256": _uniform(-1.5, 2.5, 256), "w19": _uniform(-12, 12, 19), "w256": _uniform(-12, 12, 256), "n64": _nonuniform(64)}


def _planted(e32):
    """Every edge, the value one ulp below each, and the one above the last edge (so that `over` is never empty by chance)."""
    return np.concatenate([e32, np.nextafter(e32, F32(-np.inf)), np.nextafter(e32[-1:], F32(np.inf))]).astype(F32)


def _values(n_rec, B, width, rows, e32, seed):
    """[n_rec, B, width] fp32: 3 N(0,1) + 1.5 with the planted values at random places of the records taken.  Returns (host, all planted
    values fit)."""
    rng = np.random.default_rng(seed)
    host = (3.0 * rng.standard_normal((n_rec, B * width)) + 1.5).astype(F32)
    plant = _planted(e32)
    places = [(r, i) for r in rows for i in range(B * width)]
    fit = len(places) >= 2 * plant.size
    take = rng.permutation(len(places))[:min(plant.size, len(places))]
    for v, k in zip(rng.permutation(plant), take):
        host[places[k]] = v
    return host.reshape(n_rec, B, width), fit


def _on_device(host, offset):
    """The records on the device, `offset` floats into their allocation."""
    alloc = torch.empty(host.size + offset, dtype=torch.float32, device=DEV)
    rec = alloc[offset:].view(*host.shape)
    rec.copy_(torch.from_numpy(host))
    assert rec.is_contiguous() and rec.data_ptr() == alloc.data_ptr() + 4 * offset
    return rec


def _garbage(shape, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2 ** 62, 2 ** 62, shape, generator=g, dtype=torch.int64)


WINDOWS = [(0, 1, 1), (0, 1, 2), (3, 2, 7), (5, 7, 8), (0, 1, 37)]
SHAPES = [(1, 1), (3, 5), (16, 15), (37, 20), (5, 784), (256, 1)]
CASES = [(B, w, off, win) for (B, w) in SHAPES for off in (0, 1) for win in WINDOWS] + \
        [(B, w, off, (0, 1, 300)) for (B, w) in ((256, 1), (3, 5)) for off in (0, 1)]


@pytest.mark.parametrize("B, width, offset, window", CASES)
def test_counts_are_the_numpy_definition(B, width, offset, window):
    """Overwrite onto garbage, accumulate onto known counts, and pool = 1 against pool = 0 summed over the chains, for every edge set."""
    from montecarlopredictivecoding_amd.engine import hist_accumulate
    first, stride, n = window
    rows = [first + k * stride for k in range(n)]
    n_rec = rows[-1] + 3
    for name, e32 in EDGE_SETS.items():
        nb = e32.size - 1
        host, fit = _values(n_rec, B, width, rows, e32, seed=B * width + n + nb)
        want = table(host[rows], e32)                                        # [B, width, nb + 3]
        assert (want.sum(-1) == n).all()
        if fit:                                                              # (asserted on the host, before the device is touched)
            assert want[..., nb].sum() > 0 and want[..., nb + 1].sum() > 0, name
        rec = _on_device(host, offset)
        counts = _garbage((B, width, nb + 3)).to(DEV)
        hist_accumulate(rec, first, stride, n, e32, counts, accumulate=False)
        assert np.array_equal(counts.cpu().numpy(), want), (name, "overwrite")
        known = torch.randint(0, 1000, (B, width, nb + 3), generator=torch.Generator().manual_seed(2), dtype=torch.int64)
        counts = known.to(DEV)
        hist_accumulate(rec, first, stride, n, torch.from_numpy(e32), counts, accumulate=True)
        assert np.array_equal(counts.cpu().numpy(), known.numpy() + want), (name, "accumulate")
        pooled = _garbage((width, nb + 3)).to(DEV)
        hist_accumulate(rec, first, stride, n, e32, pooled, pool=True, accumulate=False)
        assert np.array_equal(pooled.cpu().numpy(), want.sum(0)), (name, "pool, overwrite")
        pooled = known[0].to(DEV)
        hist_accumulate(rec, first, stride, n, e32, pooled, pool=True, accumulate=True)
        assert np.array_equal(pooled.cpu().numpy(), known[0].numpy() + want.sum(0)), (name, "pool, accumulate")


@pytest.mark.parametrize("name", ["u19", "u256", "n64"])
def test_every_edge_in_one_unit(name):
    """One chain, one unit, and a window long enough for every planted value: each edge opens its bin, the value below closes the one
    before."""
    from montecarlopredictivecoding_amd.engine import hist_accumulate
    e32 = EDGE_SETS[name]
    nb = e32.size - 1
    n = 4 * _planted(e32).size
    host, fit = _values(n + 2, 1, 1, list(range(n)), e32, seed=nb)
    want = table(host[:n], e32)
    assert fit and want[0, 0, nb] >= 1 and want[0, 0, nb + 1] >= 1 and (want[0, 0, :nb] >= 1).all()
    for offset in (0, 1):
        counts = _garbage((1, 1, nb + 3)).to(DEV)
        hist_accumulate(_on_device(host, offset), 0, 1, n, e32, counts, accumulate=False)
        assert np.array_equal(counts.cpu().numpy(), want)


@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("B, width, offset", [(3, 5, 0), (37, 20, 1), (5, 784, 0), (256, 1, 0)])
def test_chunking_the_records_does_not_change_a_count(B, width, offset, pool):
    from montecarlopredictivecoding_amd.engine import hist_accumulate
    for name in ("u19", "w256", "n64"):
        e32 = EDGE_SETS[name]
        nb = e32.size - 1
        host, _ = _values(40, B, width, list(range(37)), e32, seed=7)
        rec = _on_device(host, offset)
        shape = (width, nb + 3) if pool else (B, width, nb + 3)
        once = _garbage(shape).to(DEV)
        hist_accumulate(rec, 0, 1, 37, e32, once, pool=pool, accumulate=False)
        parts = _garbage(shape, seed=3).to(DEV)
        hist_accumulate(rec, 0, 1, 1, e32, parts, pool=pool, accumulate=False)
        hist_accumulate(rec, 1, 1, 5, e32, parts, pool=pool, accumulate=True)
        hist_accumulate(rec, 6, 1, 31, e32, parts, pool=pool, accumulate=True)
        assert torch.equal(once, parts), name
        want = table(host[:37], e32)
        assert np.array_equal(once.cpu().numpy(), want.sum(0) if pool else want), name


@pytest.mark.parametrize("offset", [0, 1])
def test_pooled_row_long_enough_for_runs_of_tiles(offset):
    """6000 chains x 96 units: the row has more tiles than a pooled launch has workgroups, so a workgroup counts a run of tiles that hold
    the same units (four or five, the last tile of the row ragged) before it flushes once: 4500 tiles over 1026 workgroups."""
    from montecarlopredictivecoding_amd.engine import hist_accumulate
    B, width, n = 6000, 96, 2
    e32 = EDGE_SETS["u64"]
    rng = np.random.default_rng(11)
    host = (3.0 * rng.standard_normal((n + 1, B, width)) + 1.5).astype(F32)
    plant = _planted(e32)
    host[0].reshape(-1)[rng.permutation(B * width)[:plant.size]] = plant
    want = table(host[:n].reshape(n * B, width), e32)                       # [width, 67]: the chains are samples of the unit
    assert (want.sum(-1) == n * B).all() and want[:, 64].sum() > 0 and want[:, 65].sum() > 0
    rec = _on_device(host, offset)
    pooled = _garbage((width, 67)).to(DEV)
    hist_accumulate(rec, 0, 1, n, e32, pooled, pool=True, accumulate=False)
    assert np.array_equal(pooled.cpu().numpy(), want)
    hist_accumulate(rec, 0, 1, n, e32, pooled, pool=True, accumulate=True)
    assert np.array_equal(pooled.cpu().numpy(), 2 * want)


@pytest.mark.parametrize("B, width, offset", [(3, 5, 0), (3, 5, 1), (16, 16, 0), (64, 4, 1)])
def test_special_values(B, width, offset):
    """Huge values, infinities, NaN, denormals and both zeros, with an edge exactly at 0.0."""
    from montecarlopredictivecoding_amd.engine import hist_accumulate
    vals = np.array([3e38, -3e38, np.inf, -np.inf, np.nan, 1e-40, -1e-42, 1.17549435e-38, 0.0, -0.0], dtype=F32)
    n = 41
    rng = np.random.default_rng(B + width)
    host = vals[rng.integers(0, vals.size, (n, B, width))]
    host[:vals.size, 0, 0] = vals                                            # every one of them at least once
    assert np.signbit(host[vals.size - 1, 0, 0]) and host[vals.size - 1, 0, 0] == 0
    for e32 in (np.array([-1.0, 0.0, 1.0], dtype=F32), np.array([0.0, 1e-41, 1.0], dtype=F32), np.array([-2.0, -1e-44, 0.0], dtype=F32)):
        nb = e32.size - 1
        want = table(host, e32)
        counts = _garbage((B, width, nb + 3)).to(DEV)
        hist_accumulate(_on_device(host, offset), 0, 1, n, e32, counts, accumulate=False)
        got = counts.cpu().numpy()
        assert np.array_equal(got, want)
        assert (got.sum(-1) == n).all()
        assert np.array_equal(got[..., nb + 2], np.isnan(host).sum(0))       # NaN goes to the NaN column, and only NaN does
    # one value at a time against the edges [-1, 0, 1]: where each one lands
    e32 = np.array([-1.0, 0.0, 1.0], dtype=F32)
    col = {}
    for v in vals:
        counts = torch.zeros(1, 1, 5, dtype=torch.int64, device=DEV)
        hist_accumulate(_on_device(np.full((1, 1, 1), v, dtype=F32), offset), 0, 1, 1, e32, counts, accumulate=False)
        got = counts.cpu().numpy()[0, 0]
        assert got.sum() == 1
        col[repr(float(v))] = int(np.argmax(got))
    assert col[repr(float(F32(-1e-42)))] == 0 and col["-0.0"] == 1 and col["0.0"] == 1           # under the edge / at it
    assert col[repr(float(F32(1e-40)))] == 1 and col[repr(float(F32(1.17549435e-38)))] == 1
    assert col["inf"] == 3 and col[repr(float(F32(3e38)))] == 3 and col["-inf"] == 2 and col[repr(float(F32(-3e38)))] == 2 and col["nan"] == 4
    # with the first edge at 0.0: -1e-42 is UNDER it, -0.0 is not
    e32 = np.array([0.0, 1.0], dtype=F32)
    for v, c in ((F32(-1e-42), 1), (F32(-0.0), 0), (F32(1e-40), 0)):
        counts = torch.zeros(1, 1, 4, dtype=torch.int64, device=DEV)
        hist_accumulate(_on_device(np.full((1, 1, 1), v, dtype=F32), 0), 0, 1, 1, e32, counts, accumulate=False)
        assert int(np.argmax(counts.cpu().numpy()[0, 0])) == c, (v, c)


@pytest.mark.parametrize("pool", [False, True])
def test_no_records(pool):
    from montecarlopredictivecoding_amd.engine import hist_accumulate
    e32 = EDGE_SETS["u19"]
    rec = _on_device(np.ones((2, 3, 5), dtype=F32), 0)
    shape = (5, 22) if pool else (3, 5, 22)
    keep = _garbage(shape)
    counts = keep.to(DEV)
    hist_accumulate(rec, 0, 1, 0, e32, counts, pool=pool, accumulate=True)
    assert torch.equal(counts.cpu(), keep)
    hist_accumulate(rec, 0, 1, 0, e32, counts, pool=pool, accumulate=False)
    assert not counts.any()


def test_wrapper_checks_its_arguments():
    from montecarlopredictivecoding_amd.engine import hist_accumulate
    e32 = EDGE_SETS["u19"]
    rec = _on_device(np.ones((4, 3, 5), dtype=F32), 0)
    counts = torch.zeros(3, 5, 22, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="shape"):
        hist_accumulate(rec, 0, 1, 2, e32, counts, pool=True)
    with pytest.raises(TypeError, match="int64"):
        hist_accumulate(rec, 0, 1, 2, e32, counts.to(torch.int32))
    with pytest.raises(ValueError, match="device"):
        hist_accumulate(rec, 0, 1, 2, e32, counts.cpu())
    with pytest.raises(ValueError, match="last one asked for"):
        hist_accumulate(rec, 0, 2, 3, e32, counts)
    with pytest.raises(TypeError, match="edges"):
        hist_accumulate(rec, 0, 1, 2, e32.astype(np.float64), torch.zeros(3, 5, 22, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="transform"):
        hist_accumulate(rec, 0, 1, 2, e32, counts, transform="softmax")
    with pytest.raises(ValueError, match="contiguous"):
        hist_accumulate(rec.transpose(1, 2), 0, 1, 2, e32, torch.zeros(5, 3, 22, dtype=torch.int64, device=DEV))
    from montecarlopredictivecoding_amd._lib import MCPCError
    bad = e32.copy()
    bad[3] = bad[2]
    with pytest.raises(MCPCError, match="strictly ascending"):
        hist_accumulate(rec, 0, 1, 2, bad, counts)
    assert not counts.any()


def test_sigmoid_transform():
    """The read-out's Bernoulli mean, 20 uniform bins on [0, 1].  sigmoid_f is within 4.8e-7 of the fp64 sigmoid
    (tests/test_gpu_moments.py::test_sigmoid_transform); with tol = 1e-6, twice that, a value whose fp64 sigmoid lies within tol of an
    interior edge may fall on either side of it, and every other value may not.  Per unit and bin:
        (unambiguous values in the bin) <= count <= (that + ambiguous values in the bin or next to it)."""
    from montecarlopredictivecoding_amd.engine import hist_accumulate
    g = torch.Generator().manual_seed(6)
    logits = 3.0 * torch.randn(64, 2310, generator=g)
    e32 = _uniform(0.0, 1.0, 20)
    e64 = e32.astype(np.float64)
    ref = 1.0 / (1.0 + np.exp(-logits.numpy().astype(np.float64)))
    tol = 1e-6
    near = np.abs(ref[..., None] - e64[1:-1]) <= tol                          # [64, 2310, 19]: interior edge i + 1
    amb = near.any(-1)
    assert amb.sum() <= 1e-3 * amb.size, int(amb.sum())                      # the condition (4 of 147 840 for this input)
    idx = np.clip(np.searchsorted(e64, ref, side="right") - 1, 0, 19)
    sure = np.zeros((2310, 20), np.int64)
    maybe = np.zeros((2310, 20), np.int64)
    for i in range(20):
        sure[:, i] = ((idx == i) & ~amb).sum(0)
        # ambiguous at interior edge j (between bins j - 1 and j): it may be counted in either
        touch = np.zeros_like(amb)
        if i >= 1:
            touch |= near[..., i - 1]
        if i <= 18:
            touch |= near[..., i]
        maybe[:, i] = touch.sum(0)
    counts = _garbage((1, 2310, 23)).to(DEV)
    hist_accumulate(logits.to(DEV).view(64, 1, 2310), 0, 1, 64, e32, counts, transform="sigmoid", accumulate=False)
    got = counts.cpu().numpy()[0]
    assert (got.sum(-1) == 64).all() and not got[:, 20:].any()               # a sigmoid is in [0, 1] and no NaN
    assert (sure <= got[:, :20]).all() and (got[:, :20] <= sure + maybe).all()
    print(f"sigmoid histogram: {int(amb.sum())} ambiguous of {amb.size}; bins that differ from the fp64 ones: "
          f"{int((got[:, :20] != table(ref.astype(F32), e32)[:, :20]).sum())}")

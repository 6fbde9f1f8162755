"""Posterior histograms, host side (no GPU): the `mcpc_histogram` request, the sample count, the fp64 arithmetic from counts to
density, cdf and quantiles, the numpy definition the device tests compare against, and the C entry point's declaration, binding and
argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from montecarlopredictivecoding_amd import _lib
from montecarlopredictivecoding_amd import histogram as H
from tests.hist_cases import ref_hist, table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (6, 16, 16)
KW = dict(T=60, n_layers=3, n_out=24, sizes=SIZES, B=37, max_bytes=2 << 30)
BINS = dict(bins=20, range=(-3.0, 3.0))


def test_defaults_and_edges():
    spec = H.validate_spec(dict(BINS, layers=(0,)), **KW)
    assert (spec.begin, spec.stride, spec.layers, spec.outputs, spec.pooled, spec.T, spec.n) == (0, 1, (0,), None, False, 60, 60)
    assert spec.columns == (("x0", 6),)
    assert spec.edges[0].dtype == np.float32 and np.array_equal(spec.edges[0], np.linspace(-3.0, 3.0, 21).astype(np.float32))
    # layers defaults to (): the read-out alone
    spec = H.validate_spec(dict(BINS, outputs="sigmoid"), **KW)
    assert spec.layers == () and spec.columns == (("out", 24),)
    spec = H.validate_spec(dict(begin=13, stride=3, layers=(2, 0, 2), outputs="identity", pool="chains", bins=[-1.0, 0.0, 0.5, 4.0]), **KW)
    assert spec.layers == (0, 2) and spec.pooled and spec.n == len(range(13, 60, 3))
    assert spec.columns == (("x0", 6), ("x2", 16), ("out", 24))
    assert all(np.array_equal(e, np.float32([-1.0, 0.0, 0.5, 4.0])) for e in spec.edges)
    assert H.validate_spec(dict(BINS, layers=1), **KW).columns == (("x1", 16),)
    # per block, either form
    spec = H.validate_spec(dict(layers=(0, 1), outputs="sigmoid", bins={"x0": 4, "x1": [0.0, 1.0, 3.0], "out": 10},
                                range={"x0": (-1, 1), "out": (0, 1)}), **KW)
    assert [len(e) for e in spec.edges] == [5, 3, 11]
    assert np.array_equal(spec.edges[2], np.linspace(0, 1, 11).astype(np.float32)) and np.array_equal(spec.edges[1], np.float32([0, 1, 3]))
    assert H.validate_spec(dict(layers=(0,), bins=256, range=(0, 1)), **KW).edges[0].size == 257
    assert H.validate_spec(dict(layers=(0,), bins=1, range=(0, 1)), **KW).edges[0].size == 2


@pytest.mark.parametrize("spec, word", [
    (dict(BINS, layers=(0,), strid=2), "unknown keys"),
    (dict(BINS, layers=(0,), begin=-1), "begin"),
    (dict(BINS, layers=(0,), begin=60), "begin"),
    (dict(BINS, layers=(0,), begin=1.0), "begin must be an int"),
    (dict(BINS, layers=(0,), begin=True), "begin must be an int"),
    (dict(BINS, layers=(0,), stride=0), "stride"),
    (dict(BINS, layers=(0,), stride="2"), "stride must be an int"),
    (dict(BINS, layers=(0, 3)), "layer index"),
    (dict(BINS, layers=(-1,)), "layer index"),
    (dict(BINS, layers=(True,)), "layer index"),
    (dict(BINS, layers=1.5), "sequence of layer indices"),
    (dict(BINS), "no columns"),
    (dict(BINS, layers=()), "no columns"),
    (dict(BINS, outputs="softmax"), "outputs"),
    (dict(BINS, layers=(0,), pool="records"), "pool"),
    (dict(BINS, layers=(0,), pool=True), "pool"),
    ([("begin", 0)], "expected a dict"),
    (dict(layers=(0,)), "bins is required"),
    (dict(layers=(0,), bins=20), "needs range"),
    (dict(layers=(0,), bins=0, range=(0, 1)), "bins=0"),
    (dict(layers=(0,), bins=257, range=(0, 1)), "bins=257"),
    (dict(layers=(0,), bins=True, range=(0, 1)), "bins"),
    (dict(layers=(0,), bins=4, range=(1, 1)), "lo < hi"),
    (dict(layers=(0,), bins=4, range=(0, float("inf"))), "finite"),
    (dict(layers=(0,), bins=4, range=3), "range"),
    (dict(layers=(0,), bins=[0.0]), "2..257"),
    (dict(layers=(0,), bins=[0.0, 1.0, 1.0]), "strictly ascending"),
    (dict(layers=(0,), bins=[0.0, 2.0, 1.0]), "strictly ascending"),
    (dict(layers=(0,), bins=[0.0, float("nan")]), "finite"),
    (dict(layers=(0,), bins=[0.0, 1e39]), "finite"),
    (dict(layers=(0,), bins=[1.0, 1.0 + 1e-9, 2.0]), "strictly ascending in fp32"),       # distinct in fp64, one value in fp32
    (dict(layers=(0,), bins=4, range=(1.0, 1.0 + 1e-7)), "strictly ascending in fp32"),
    (dict(layers=(0,), bins="many", range=(0, 1)), "bins"),
    (dict(layers=(0,), bins={"x1": 4}, range=(0, 1)), "does not have"),
    (dict(layers=(0, 1), bins={"x0": 4}, range=(0, 1)), "no entry for block 'x1'"),
    (dict(layers=(0,), bins=4, range={"x2": (0, 1)}), "does not have"),
])
def test_invalid_requests_are_value_errors(spec, word):
    with pytest.raises(ValueError, match=word):
        H.validate_spec(spec, **KW)


def test_outputs_need_a_read_out():
    with pytest.raises(ValueError, match="read-out"):
        H.validate_spec(dict(BINS, outputs="identity"), **dict(KW, n_layers=2, n_out=0))
    assert H.validate_spec(dict(BINS, layers=(1,)), **dict(KW, n_layers=2, n_out=0)).layers == (1,)


def test_the_size_guard_names_the_size_and_the_ways_out():
    spec = dict(BINS, layers=(0, 1, 2))
    need = 8 * 38 * 23 * 37
    ok = H.validate_spec(spec, **dict(KW, max_bytes=need))
    assert H.result_bytes(ok.columns, ok.edges, 37, False) == need and H.result_bytes(ok.columns, ok.edges, 37, True) == 8 * 38 * 23
    with pytest.raises(ValueError, match=r"37 chains x 38 units.*KiB.*mcpc_histogram_max_bytes.*fewer layers or fewer bins or pool='chains'"):
        H.validate_spec(spec, **dict(KW, max_bytes=need - 1))
    assert H.validate_spec(dict(spec, pool="chains"), **dict(KW, max_bytes=need - 1)).pooled
    with pytest.raises(ValueError, match=r"38 units.*fewer layers or fewer bins$"):
        H.validate_spec(dict(spec, pool="chains"), **dict(KW, max_bytes=1000))
    big = dict(T=8000, n_layers=3, n_out=784, sizes=(20, 128, 128), max_bytes=2 << 30)
    assert H.validate_spec(dict(layers=(0, 1, 2), bins=256, range=(-5, 5)), B=256, **big).n == 8000
    with pytest.raises(ValueError, match="GiB"):
        H.validate_spec(dict(layers=(0, 1, 2), outputs="sigmoid", bins=256, range=(-5, 5)), B=20000, **big)


@pytest.mark.parametrize("begin, stride, T", [(0, 1, 1), (13, 3, 60), (59, 7, 60), (200, 1, 1000), (3, 4, 5), (0, 60, 60)])
def test_sample_count_and_chunks(begin, stride, T):
    spec = H.validate_spec(dict(BINS, layers=(0,), begin=begin, stride=stride), **dict(KW, T=T))
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


def _edge_values(e32):
    """Every edge, the fp32 value one ulp below it, and the one above the last edge."""
    return np.concatenate([e32, np.nextafter(e32, np.float32(-np.inf)), np.nextafter(e32[-1:], np.float32(np.inf))]).astype(np.float32)


EDGE_SETS = [np.linspace(-1.5, 2.5, 20).astype(np.float32), np.linspace(-12, 12, 65).astype(np.float32),
             np.float32([-3.0, -1.0, -0.99999994, 0.0, 1e-30, 0.3, 0.30000004, 7.5]), np.float32([0.0, 1.0])]


@pytest.mark.parametrize("e32", EDGE_SETS, ids=["uniform19", "uniform64", "nonuniform", "one_bin"])
def test_ref_hist_is_numpy_histogram_with_explicit_edges(e32):
    rng = np.random.default_rng(0)
    v = np.concatenate([(3 * rng.standard_normal(500) + 1.5).astype(np.float32), _edge_values(e32)])
    v = np.stack([v, v[::-1]], axis=1)                       # [n, 2]
    bins, under, over, nan = ref_hist(v, e32)
    for j in range(2):
        want = np.histogram(v[:, j].astype(np.float64), bins=e32.astype(np.float64))[0]
        assert np.array_equal(bins[j], want)
        assert under[j] == (v[:, j] < e32[0]).sum() > 0 and over[j] == (v[:, j] > e32[-1]).sum() > 0 and nan[j] == 0
        assert bins[j].sum() + under[j] + over[j] == v.shape[0]
    # the value on an edge opens the bin above it, the value one ulp below closes the bin below; the last edge closes the last bin
    for i, edge in enumerate(e32):
        b, u, o, _ = ref_hist(np.float32([edge])[:, None], e32)
        assert (u[0], o[0]) == (0, 0) and b[0, min(i, e32.size - 2)] == 1
        b, u, o, _ = ref_hist(np.nextafter(np.float32([edge]), np.float32(-np.inf))[:, None], e32)
        assert (u[0] == 1) if i == 0 else (b[0, i - 1] == 1)
    b, u, o, n = ref_hist(np.float32([np.nan, np.inf, -np.inf, -0.0, -1e-42])[:, None], np.float32([0.0, 1.0]))
    assert (b[0, 0], u[0], o[0], n[0]) == (1, 2, 1, 1)
    assert table(v, e32).shape == (2, e32.size + 2) and (table(v, e32).sum(-1) == v.shape[0]).all()


def _hist(values, e32, pooled=False):
    """values: fp32 [n, B, w] -> Histogram of block "x0"."""
    n, B, _ = values.shape
    b, u, o, na = ref_hist(values, e32)
    h = H.Histogram(n=n, B=B, pooled=False, names=["x0"], edges={"x0": torch.from_numpy(e32.copy())}, counts={"x0": torch.from_numpy(b)},
                    under={"x0": torch.from_numpy(u)}, over={"x0": torch.from_numpy(o)}, nan={"x0": torch.from_numpy(na)})
    return h.pool() if pooled else h


@pytest.mark.parametrize("e32", EDGE_SETS[:3], ids=["uniform19", "uniform64", "nonuniform"])
def test_density_and_cdf_against_numpy(e32):
    rng = np.random.default_rng(1)
    v = (3 * rng.standard_normal((400, 3, 2)) + 1.5).astype(np.float32)
    h = _hist(v, e32)
    d, c = h.density("x0"), h.cdf("x0")
    assert d.dtype == c.dtype == torch.float64 and tuple(d.shape) == (3, 2, e32.size - 1)
    for b in range(3):
        for u in range(2):
            want = np.histogram(v[:, b, u].astype(np.float64), bins=e32.astype(np.float64), density=True)[0]
            np.testing.assert_allclose(d[b, u].numpy(), want, rtol=4 * 2.0 ** -52, atol=0)
            cnt = np.histogram(v[:, b, u].astype(np.float64), bins=e32.astype(np.float64))[0]
            np.testing.assert_allclose(c[b, u].numpy(), np.cumsum(cnt) / cnt.sum(), rtol=2.0 ** -52, atol=0)
    p = h.pool()
    want = np.histogram(v[:, :, 1].astype(np.float64).ravel(), bins=e32.astype(np.float64), density=True)[0]
    np.testing.assert_allclose(p.density("x0")[1].numpy(), want, rtol=4 * 2.0 ** -52, atol=0)
    with pytest.raises(KeyError, match="x1"):
        h.density("x1")


def test_quantile_of_a_step_distribution():
    e = np.float32([0.0, 1.0, 2.0, 4.0])
    counts = torch.tensor([[[2, 0, 2]], [[0, 4, 4]], [[0, 0, 0]]])                   # [B=3, w=1, nb=3]
    z = torch.zeros(3, 1, dtype=torch.int64)
    h = H.Histogram(n=8, B=3, pooled=False, names=["x0"], edges={"x0": torch.from_numpy(e)}, counts={"x0": counts},
                    under={"x0": z + 1}, over={"x0": z}, nan={"x0": z})
    q = h.quantile("x0", [0.0, 0.25, 0.5, 0.75, 1.0])
    assert q.dtype == torch.float64 and tuple(q.shape) == (3, 1, 5)
    assert q[0, 0].tolist() == [0.0, 0.5, 1.0, 3.0, 4.0]       # mass 2 on [0, 1), none on [1, 2), 2 on [2, 4]
    assert q[1, 0].tolist() == [1.0, 1.5, 2.0, 3.0, 4.0]
    assert torch.isnan(q[2]).all()                             # nothing in range
    assert h.quantile("x0", 0.5).shape == (3, 1) and h.quantile("x0", 0.5)[1, 0] == 2.0
    with pytest.raises(ValueError, match="q must lie"):
        h.quantile("x0", 1.5)
    # against the sorted sample: the q-quantile lies in the bin that holds the sample of that rank
    rng = np.random.default_rng(2)
    v = rng.standard_normal((1000, 1, 1)).astype(np.float32)
    e = np.linspace(-5, 5, 41).astype(np.float32)
    hh = _hist(v, e)
    for qv in (0.05, 0.5, 0.95):
        got = float(hh.quantile("x0", qv)[0, 0])
        assert abs(got - np.quantile(v.astype(np.float64), qv)) <= 0.25      # one bin width


@pytest.mark.parametrize("pooled", [False, True])
def test_pool_merge_and_the_invariant(pooled):
    rng = np.random.default_rng(3)
    e32 = np.linspace(-1.5, 2.5, 20).astype(np.float32)
    v = (3 * rng.standard_normal((12, 4, 5)) + 1.5).astype(np.float32)
    v[3, 1, 2] = np.nan
    whole, a, b = _hist(v, e32, pooled), _hist(v[:5], e32, pooled), _hist(v[5:], e32, pooled)
    both = a.merge(b)
    assert (both.n, both.B, both.pooled, both.names) == (12, 4, pooled, ["x0"])
    for f in ("counts", "under", "over", "nan"):
        assert torch.equal(getattr(both, f)["x0"], getattr(whole, f)["x0"])
    assert torch.equal(whole.total("x0"), torch.full((5,) if pooled else (4, 5), 48 if pooled else 12))
    assert whole.N == (48 if pooled else 12) and int(whole.nan["x0"].sum()) == 1
    pool = _hist(v, e32).pool()
    assert pool.pooled and pool.pool() is pool and tuple(pool.counts["x0"].shape) == (5, 19)
    want = np.histogram(v[:, :, 0].astype(np.float64).ravel(), bins=e32.astype(np.float64))[0]
    assert np.array_equal(pool.counts["x0"][0].numpy(), want)
    with pytest.raises(ValueError, match="different requests"):
        whole.merge(_hist(v[:, :, :3], e32, pooled))
    with pytest.raises(ValueError, match="different requests"):
        whole.merge(_hist(v, np.linspace(-1.5, 2.0, 20).astype(np.float32), pooled))


def test_the_trainer_has_the_opt_in_attributes_and_they_are_off():
    import montecarlopredictivecoding_amd.predictive_coding as pc
    model = torch.nn.Sequential(torch.nn.Linear(2, 2), pc.PCLayer(), torch.nn.Linear(2, 3))
    tr = pc.PCTrainer(model, T=4, plot_progress_at=[])
    assert tr.mcpc_histogram is None and tr.mcpc_last_histogram is None and tr.mcpc_histogram_max_bytes == 2 << 30


def test_header_declares_the_entry_point_and_the_binding_binds_it():
    header = open(os.path.join(ROOT, "include", "mcpc.h")).read()
    assert re.search(r"\bint\s+mcpc_hist_accumulate\s*\(", header)
    assert re.search(r"#define\s+MCPC_HIST_MAX_BINS\s+256\b", header) and _lib.HIST_MAX_BINS == H.MAX_BINS == 256
    assert re.search(r"#define\s+MCPC_ABI_VERSION\s+4\b", header) and _lib.ABI_VERSION == 4
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = re.search(r"mcpc_hist_accumulate\s*\(([^)]*)\)", code).group(1)
    res, args = _lib.SYMBOLS["mcpc_hist_accumulate"]
    assert len(args) == len(decl.split(",")) == 14
    from montecarlopredictivecoding_amd import engine
    assert callable(engine.hist_accumulate)
    lib = _lib.load()
    assert lib.mcpc_abi_version() == 4 and hasattr(lib, "mcpc_hist_accumulate")


def test_argument_errors_are_refused_before_any_device_work():
    """Every MCPC_EINVAL case returns -1 with a message and touches no device: the pointers are never dereferenced (this machine need
    not have a GPU)."""
    lib = _lib.load()
    good = np.linspace(-1, 1, 5).astype(np.float32)
    rec, counts = C.c_void_p(0x1000), C.c_void_p(0x2000)         # never dereferenced: every call below is refused

    def call(rec=rec, B=3, width=5, first=0, stride=1, n=4, transform=0, edges=good, n_bins=4, pool=0, counts=counts):
        ptr = None if edges is None else edges.ctypes.data_as(C.POINTER(C.c_float))
        rc = lib.mcpc_hist_accumulate(0, rec, B, width, first, stride, n, transform, ptr, n_bins, pool, counts, 1, None)
        return rc, lib.mcpc_last_error().decode()

    many = np.arange(300, dtype=np.float32)
    for kw, word in [(dict(counts=None), "counts is null"), (dict(edges=None), "edges is null"), (dict(rec=None), "rec is null with n=4"),
                     (dict(B=0), "B=0"), (dict(width=0), "width=0"), (dict(stride=0), "stride=0"), (dict(first=-1), "first=-1"),
                     (dict(n=-1), "n=-1"), (dict(n_bins=0), "n_bins=0"), (dict(n_bins=257, edges=many), "n_bins=257"),
                     (dict(pool=2), "pool=2"), (dict(pool=-1), "pool=-1"), (dict(transform=2), "unknown transform 2"),
                     (dict(edges=np.float32([0, 1, np.inf, 3, 4])), "edges[2] is not finite"),
                     (dict(edges=np.float32([0, 1, np.nan, 3, 4])), "edges[2] is not finite"),
                     (dict(edges=np.float32([0, 1, 1, 3, 4])), "not strictly ascending at 2"),
                     (dict(edges=np.float32([0, 1, 0.5, 3, 4])), "not strictly ascending at 2"),
                     (dict(edges=np.float32([-0.0, 0.0, 0.5, 3, 4])), "not strictly ascending at 1")]:
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("hist:") and word in msg, (kw, rc, msg)
    # nothing to add: accepted without a device, and nothing is read
    assert call(n=0, rec=None)[0] == 0

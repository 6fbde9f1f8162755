"""Joint histograms on the device, the trainer: `PCTrainer.mcpc_histogram2d` against the recorded trajectory of the same call.  Counts
are integers and a cell is decided by fp32 comparison alone, so the counts of the call equal the numpy definition
(tests/hist2d_cases.py) on the trajectory the same call returns, exactly -- in the probe form after `engine.probe_records` twice, and
within the samples the fp32 link can move across an edge of the fp64 softmax."""
import warnings

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from tests import hist2d_cases as hc
from tests import probe_cases as pcs
from tests.test_gpu_hist_facade import N_OUT, SIZES, B, T, _net

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS = list(range(20, T, 3))
UNITS = dict(begin=20, stride=3, x=(0, (0, 3, 5, 3)), y=(2, (1, 1, 15, 0)), bins=(19, 12), range=((-1.5, 2.5), (-4.0, 4.0)))
C = 10
EDGES = np.linspace(-1.03, 1.01, 38).astype(np.float32)                               # no multiple of a vertex coordinate of the polygon


def _classifier():
    g = torch.Generator().manual_seed(11)
    return 1.5 * torch.randn(C, SIZES[0], generator=g), 0.3 * torch.randn(C, generator=g)


def _probe_spec(**kw):
    W, b = _classifier()
    return dict(dict(begin=20, stride=3, probe=dict(layer=0, weight=W, bias=b, link="softmax"), bins=(EDGES, EDGES)), **kw)


def _call(um, model, data, inputs, hist2d, chunk=None, xs=True, update_p_at="never", histogram=None, probe=None, max_bytes=None):
    import montecarlopredictivecoding_amd.predictive_coding as pc
    import montecarlopredictivecoding_amd.predictive_coding.pc_trainer as pt
    tr = pc.PCTrainer(model, T=T, optimizer_x_fn=torch.optim.SGD, optimizer_x_kwargs={"lr": 0.05}, update_p_at=update_p_at,
                      accumulate_p_at="never", optimizer_p_fn=torch.optim.Adam, optimizer_p_kwargs={"lr": 0.01}, plot_progress_at=[])
    tr.mcpc_seed = 5
    tr.mcpc_histogram2d, tr.mcpc_histogram, tr.mcpc_probe = hist2d, histogram, probe
    if chunk is not None:
        tr.mcpc_moments_chunk_bytes = chunk
    if max_bytes is not None:
        tr.mcpc_histogram2d_max_bytes = max_bytes
    base = pt._PHILOX_STEPS[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = tr.train_on_batch(inputs=inputs, callback_after_t=um.random_step, callback_after_t_kwargs={"_pc_trainer": tr},
                                is_log_progress=False, is_return_results_every_t=True, is_return_xs=xs, is_return_outputs=False,
                                loss_fn=um.bernoulli_fn, loss_fn_kwargs={"_target": data, "_var": None})
    pt._PHILOX_STEPS[0] = base                               # the next run replays the same noise
    return tr, res


def _trajectory(res, layer):
    return np.stack([res["xs"][t][layer].detach().cpu().numpy() for t in STEPS])


def _same(a, b):
    assert (a.n, a.B, a.pooled, a.pairs) == (b.n, b.B, b.pooled, b.pairs)
    assert torch.equal(a.edges_x, b.edges_x) and torch.equal(a.edges_y, b.edges_y) and torch.equal(a.full, b.full)


@pytest.fixture(scope="module")
def reference_calls():
    """One call per form and pooling: its result and the trajectory the same call returned.  Shared, never modified."""
    out = {}
    for form, spec in (("units", UNITS), ("probe", _probe_spec())):
        for pool in (None, "chains"):
            um, model, data, inputs = _net(DEV)
            tr, res = _call(um, model, data, inputs, dict(spec, pool=pool))
            assert tr.last_call_mode == "fused" and tr.last_record_slices == 1
            out[form, pool] = (tr.mcpc_last_histogram2d, _trajectory(res, 0), _trajectory(res, 2))
    return out


@pytest.mark.parametrize("pool", [None, "chains"])
def test_unit_pairs_equal_the_joint_histogram_of_the_recorded_trajectory(reference_calls, pool):
    h, x0, x2 = reference_calls["units", pool]
    assert (h.n, h.B, h.pooled, h.pairs) == (14, B, pool == "chains", [(0, 1), (3, 1), (5, 15), (3, 0)])
    assert h.full.dtype == torch.int64 and h.full.device.type == "cuda" and tuple(h.counts.shape)[-3:] == (4, 19, 12)
    assert np.array_equal(h.edges_x.cpu().numpy(), np.linspace(-1.5, 2.5, 20).astype(np.float32))
    want = hc.ref_pairs(x0, x2, h.pairs, h.edges_x.cpu().numpy(), h.edges_y.cpu().numpy(), pool=bool(pool))
    assert np.array_equal(h.full.cpu().numpy(), want)
    assert bool((h.total() == h.N).all()) and int(h.nan.sum()) == 0 and int(h.outside.sum()) > 0    # the ranges cut the data
    d = h.density()
    assert d.device.type == "cuda" and d.dtype == torch.float64


def test_pool_method_is_the_pooled_request(reference_calls):
    for form in ("units", "probe"):
        _same(reference_calls[form, None][0].pool(), reference_calls[form, "chains"][0])


@pytest.mark.parametrize("form", ["units", "probe"])
@pytest.mark.parametrize("steps", [10, 23])
def test_the_result_does_not_depend_on_how_the_call_is_sliced(reference_calls, form, steps):
    um, model, data, inputs = _net(DEV)
    spec = UNITS if form == "units" else _probe_spec()
    step_bytes = 4 * B * (SIZES[0] + SIZES[2]) if form == "units" else 4 * B * SIZES[0] + -(-4 * B * (C + 2) // 3)
    cut, _ = _call(um, model, data, inputs, dict(spec), chunk=steps * step_bytes + step_bytes // 2, xs=False)
    assert cut.last_record_slices == -(-T // steps) > 1
    _same(cut.mcpc_last_histogram2d, reference_calls[form, None][0])


def _plane64(v32, P32):
    """The fp64 reference of the plane: the fp64 softmax of the fp32 logits, then the fp64 dot with the fp32 plane."""
    p64, _ = pcs.softmax64(v32)
    return p64 @ P32.astype(np.float64).T


def test_the_edges_keep_the_fp64_reference_clear_of_ambiguity_on_the_host():
    """The condition of the probe test below, checked without a device on a cloud like the trajectory's: at most 1 % of the samples
    lie within delta(C) of an edge."""
    W, b = _classifier()
    rng = np.random.default_rng(0)
    x = rng.normal(0.0, 1.5, size=(14 * B, SIZES[0])).astype(np.float32)
    xy = _plane64(pcs.logits(x, W.numpy(), b.numpy()), _polygon())
    delta = (C * (C + 16) + 2) * 2.0 ** -24
    near = (np.abs(xy[..., None] - EDGES.astype(np.float64)) <= delta).any(-1).any(-1)
    assert near.mean() <= 0.01


def _polygon():
    from montecarlopredictivecoding_amd.histogram2d import polygon
    return polygon(C)


@pytest.mark.parametrize("pool", [None, "chains"])
def test_probe_plane(reference_calls, pool):
    from montecarlopredictivecoding_amd.engine import probe_records
    h, x0, _ = reference_calls["probe", pool]
    W, b = _classifier()
    P = _polygon()
    assert h.pairs == [(0, 1)] and tuple(h.full.shape) == ((1, 40, 40) if pool else (B, 1, 40, 40))
    # exactly: the two derived records of the same trajectory
    rec = torch.from_numpy(x0).to(DEV)
    p = probe_records(rec, 0, 1, 14, W.to(DEV), b.to(DEV), "softmax")
    xy = probe_records(p, 0, 1, 14, torch.from_numpy(P).to(DEV), None, "identity").cpu().numpy()
    want = hc.ref_pairs(xy, xy, [(0, 1)], EDGES, EDGES, pool=bool(pool))
    assert np.array_equal(h.full.cpu().numpy(), want) and bool((h.total() == h.N).all())
    # against fp64: a sample is ambiguous when either fp64 coordinate lies within delta(C) of an edge -- each p_i is off by at most
    # p_bound(C), |P| <= 1 over C terms, and one final fp32 rounding of a value of magnitude at most 1
    xy64 = _plane64(pcs.logits(x0, W.numpy(), b.numpy()), P)
    delta = (C * (C + 16) + 2) * 2.0 ** -24
    ambiguous = (np.abs(xy64[..., None] - EDGES.astype(np.float64)) <= delta).any(-1).any(-1)      # [n, B]
    print("ambiguous samples:", int(ambiguous.sum()), "of", ambiguous.size)
    assert ambiguous.mean() <= 0.01
    ref = _ref64(xy64, pool)
    l1 = int(np.abs(h.full.cpu().numpy() - ref).sum())
    print("L1 distance of the count grids:", l1)
    assert l1 <= 2 * int(ambiguous.sum())
    assert int(h.outside.sum()) == 0 and int(h.counts.sum()) == 14 * B                # the plane's polygon lies inside the edges


def _ref64(xy64, pool):
    """The grids of fp64 coordinates against the fp32 edges, compared in fp64 (the classes of tests/hist2d_cases.py take fp32 values:
    here the comparison is written out)."""
    e = EDGES.astype(np.float64)

    def cls(v):
        idx = np.searchsorted(e, v, side="right") - 1
        idx = np.where(v == e[-1], e.size - 2, idx)
        idx = np.where(v < e[0], e.size - 1, idx)
        return np.where(v > e[-1], e.size, idx)
    flat = cls(xy64[..., 0]) * 40 + cls(xy64[..., 1])                                 # [n, B]
    out = np.stack([np.bincount(flat[:, c], minlength=1600).reshape(1, 40, 40) for c in range(flat.shape[1])]).astype(np.int64)
    return out.sum(0) if pool else out


def test_composes_with_histogram_and_probe_and_its_marginal_is_the_histogram():
    um, model, data, inputs = _net(DEV)
    W, b = _classifier()
    hist = dict(begin=20, stride=3, layers=(0,), bins=19, range=(-1.5, 2.5))
    probe = dict(begin=13, stride=2, layer=0, weight=W, bias=b, link="softmax")
    kw = dict(xs=False)
    alone_h = _call(um, model, data, inputs, None, histogram=hist, **kw)[0]
    alone_p = _call(um, model, data, inputs, None, probe=probe, **kw)[0]
    alone_2 = _call(um, model, data, inputs, dict(UNITS), **kw)[0]
    every = _call(um, model, data, inputs, dict(UNITS), histogram=hist, probe=probe, **kw)[0]
    assert alone_h.mcpc_last_histogram2d is None and alone_2.mcpc_last_histogram is None and alone_2.mcpc_last_probe is None
    _same(every.mcpc_last_histogram2d, alone_2.mcpc_last_histogram2d)
    a, e = alone_h.mcpc_last_histogram, every.mcpc_last_histogram
    for f in ("counts", "under", "over", "nan"):
        assert torch.equal(getattr(a, f)["x0"], getattr(e, f)["x0"])
    a, e = alone_p.mcpc_last_probe, every.mcpc_last_probe
    assert torch.equal(a.psum, e.psum) and torch.equal(a.psumsq, e.psumsq) and torch.equal(a.votes, e.votes) and torch.equal(a.entsum, e.entsum)
    # the x marginal of pair k is the 1-D histogram of its unit, side columns included
    h2, h1 = every.mcpc_last_histogram2d, every.mcpc_last_histogram
    assert torch.equal(h2.edges_x, h1.edges["x0"])
    units = [px for px, _ in h2.pairs]
    m = h2.marginal("x", sides=True)                                                  # [B, pairs, 22]
    assert torch.equal(m[..., :19], h1.counts["x0"][:, units]) and torch.equal(h2.marginal("x"), h1.counts["x0"][:, units])
    assert torch.equal(m[..., 19], h1.under["x0"][:, units]) and torch.equal(m[..., 20], h1.over["x0"][:, units])
    assert torch.equal(m[..., 21], h1.nan["x0"][:, units])


def test_calls_that_are_not_fused_are_rejected():
    import montecarlopredictivecoding_amd.predictive_coding as pc
    um, model, data, inputs = _net(DEV)
    small = dict(x=(0, (0,)), y=(0, (1,)), bins=4, range=(0, 1))
    with pytest.raises(NotImplementedError, match="mcpc_histogram2d is set.*step by step.*joint histograms are counted by the fused HIP loop only"):
        _call(um, model, data, inputs, small, update_p_at="all")
    assert all(m.get_x() is None for m in model if hasattr(m, "get_x"))      # before any work
    masked = torch.nn.Sequential(torch.nn.Linear(3, 3), pc.PCLayer(M=torch.ones(3, device=DEV)), torch.nn.Linear(3, 2)).to(DEV)
    masked.train()
    tr = pc.PCTrainer(masked, T=3, update_p_at="never", plot_progress_at=[])
    tr.mcpc_histogram2d = small
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(NotImplementedError, match="mcpc_histogram2d is set.*generic torch loop.*joint histograms are counted by the fused HIP loop only"):
            tr.train_on_batch(inputs=torch.zeros(2, 3, device=DEV), is_log_progress=False, is_return_results_every_t=False)
    with pytest.raises(ValueError, match="unit 6 of x out of range"):
        _call(um, model, data, inputs, dict(small, x=(0, (6,))))
    need = 8 * B * 4 * 22 * 15
    with pytest.raises(ValueError, match=r"mcpc_histogram2d_max_bytes.*fewer pairs or fewer bins or pool='chains'"):
        _call(um, model, data, inputs, dict(UNITS), max_bytes=need - 1)
    assert all(m.get_x() is None for m in model if hasattr(m, "get_x"))
    assert _call(um, model, data, inputs, dict(UNITS), max_bytes=need, xs=False)[0].mcpc_last_histogram2d.n == 14


def test_get_posterior_class_density():
    import montecarlopredictivecoding_amd.predictive_coding.pc_trainer as pt
    import montecarlopredictivecoding_amd.utils.model as um
    from montecarlopredictivecoding_amd.histogram2d import Histogram2D
    from montecarlopredictivecoding_amd.utils.training_evaluation import get_mcpc_trainer, get_pc_trainer
    torch.manual_seed(5)
    cfg = dict(input_size=SIZES[0], hidden_size=SIZES[1], hidden2_size=SIZES[2], output_size=N_OUT, activation_fn="relu",
               loss_fn=um.bernoulli_fn, input_var=0.3, T_pc=40, optimizer_x_fn_pc=torch.optim.Adam, optimizer_x_kwargs_pc={"lr": 0.1},
               mixing=20, sampling=40, optimizer_x_kwargs_mcpc={"lr": 0.03},
               optimizer_p_fn_mcpc=torch.optim.Adam, optimizer_p_kwargs_mcpc={"lr": 0.01})
    model = um.get_model(cfg, True, sample_x_fn=um.sample_x_fn_normal)
    g = torch.Generator().manual_seed(2)
    data = (torch.rand(32, N_OUT, generator=g) < 0.3).float()
    loader = DataLoader(TensorDataset(data, torch.arange(32) % 10), batch_size=16)
    classifier = torch.nn.Sequential(torch.nn.Linear(SIZES[0], C)).to(DEV)
    trainers = [get_pc_trainer(model, cfg, is_mcpc=True, training=False), get_mcpc_trainer(model, cfg, training=False)]
    marker = dict(x=(0, (0,)), y=(0, (1,)), bins=4, range=(0, 1))
    trainers[1].mcpc_histogram2d = marker
    base = pt._PHILOX_STEPS[0]
    halves, orig = [], trainers[1].train_on_batch

    def spy(*a, **k):
        r = orig(*a, **k)
        halves.append(trainers[1].mcpc_last_histogram2d)
        return r
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(7)
        trainers[1].train_on_batch = spy
        per = um.get_posterior_class_density(model, cfg, trainers, loader, classifier, bins=12, range=(-1.1, 1.1))
        trainers[1].train_on_batch = orig
        pt._PHILOX_STEPS[0] = base
        torch.manual_seed(7)
        pooled = um.get_posterior_class_density(model, cfg, trainers, loader, classifier, bins=12, range=(-1.1, 1.1), pool="chains")
        pt._PHILOX_STEPS[0] = base
    assert trainers[1].mcpc_histogram2d is marker                                     # the trainer's own request is back
    assert isinstance(per, Histogram2D) and (per.n, per.B, per.pooled, per.pairs) == (40, 32, False, [(0, 1)])
    assert len(halves) == 2 and halves[0].B == halves[1].B == 16 and tuple(per.full.shape) == (32, 1, 15, 15)
    assert torch.equal(per.full, torch.cat([halves[0].full, halves[1].full])) and bool((per.total() == 40).all())
    assert int(per.outside.sum()) == 0                                                # the polygon lies inside (-1.1, 1.1)
    assert (pooled.n, pooled.B, pooled.pooled) == (80, 16, True) and torch.equal(pooled.full, per.full.sum(0))

"""Posterior histograms on the device, the trainer: `PCTrainer.mcpc_histogram` against the recorded trajectory of the same call.
Counts are integers and a bin is decided by fp32 comparison alone, so the counts of the call equal the numpy definition
(tests/hist_cases.py) on the trajectory the same call returns, exactly."""
import warnings

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from tests.hist_cases import ref_hist

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES, N_OUT, B, T = (6, 16, 16), 24, 37, 60
SPEC = dict(begin=20, stride=3, layers=(0, 2), outputs="identity", bins={"x0": 19, "x2": 64, "out": [-30.0, -4.0, -1.0, 0.0, 0.5, 2.0, 30.0]},
            range={"x0": (-1.5, 2.5), "x2": (-4.0, 4.0)})
STEPS = list(range(20, T, 3))
NAMES = ["x0", "x2", "out"]


def _net(device, kind="relu_bernoulli"):
    """6-16-16 -> 24, ReLU (Bernoulli loss) or Tanh (Gaussian loss); the same weights, data and x0 on whichever device."""
    import montecarlopredictivecoding_amd.utils.model as um
    torch.manual_seed(3)
    cfg = dict(input_size=SIZES[0], hidden_size=SIZES[1], hidden2_size=SIZES[2], output_size=N_OUT,
               activation_fn="relu" if kind == "relu_bernoulli" else "tanh")
    model = um.get_model(cfg, False)
    g = torch.Generator().manual_seed(8)
    x0 = [torch.randn(B, n, generator=g) for n in SIZES]
    for layer, x in zip([m for m in model if hasattr(m, "get_x")], x0):
        layer._sample_x_fn = lambda inp, _x=x: _x.clone().to(inp["mu"].device)
    if kind == "relu_bernoulli":
        data = (torch.rand(B, N_OUT, generator=g) < 0.3).float()
    else:
        data = torch.randn(B, N_OUT, generator=g)
    model.to(device)
    return um, model, data.to(device), torch.zeros(B, SIZES[0], device=device)


def _call(um, model, data, inputs, hist, kind="relu_bernoulli", chunk=None, every_t=True, update_p_at="never", xs=True, outputs=True,
          moments=None, chain_energies=None, covariance=None, max_bytes=None):
    import montecarlopredictivecoding_amd.predictive_coding as pc
    import montecarlopredictivecoding_amd.predictive_coding.pc_trainer as pt
    tr = pc.PCTrainer(model, T=T, optimizer_x_fn=torch.optim.SGD, optimizer_x_kwargs={"lr": 0.05}, update_p_at=update_p_at,
                      accumulate_p_at=list(range(40, T)) if update_p_at == "last" else "never",
                      optimizer_p_fn=torch.optim.Adam, optimizer_p_kwargs={"lr": 0.01}, plot_progress_at=[])
    tr.mcpc_seed = 5
    tr.mcpc_histogram = hist
    tr.mcpc_moments = moments
    tr.mcpc_chain_energies = chain_energies
    tr.mcpc_covariance = covariance
    if chunk is not None:
        tr.mcpc_moments_chunk_bytes = chunk
    if max_bytes is not None:
        tr.mcpc_histogram_max_bytes = max_bytes
    base = pt._PHILOX_STEPS[0]
    loss = dict(loss_fn=um.bernoulli_fn, loss_fn_kwargs={"_target": data, "_var": None}) if kind == "relu_bernoulli" else \
        dict(loss_fn=um.fe_fn, loss_fn_kwargs={"_target": data, "_var": 0.3})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = tr.train_on_batch(inputs=inputs, callback_after_t=um.random_step, callback_after_t_kwargs={"_pc_trainer": tr},
                                is_log_progress=False, is_return_results_every_t=every_t, is_return_xs=xs,
                                is_return_outputs=outputs, **loss)
    pt._PHILOX_STEPS[0] = base                               # the next run replays the same noise
    return tr, res


def _trajectory(res):
    """Per block of SPEC: fp32 [n, B, w] from the records of the sample steps."""
    out = {f"x{l}": np.stack([res["xs"][t][l].detach().cpu().numpy() for t in STEPS]) for l in (0, 2)}
    out["out"] = np.stack([res["outputs"][t].detach().cpu().numpy() for t in STEPS])
    return out


def _same(a, b):
    assert (a.n, a.B, a.pooled, a.names) == (b.n, b.B, b.pooled, b.names)
    for nm in a.names:
        assert torch.equal(a.edges[nm], b.edges[nm])
        for f in ("counts", "under", "over", "nan"):
            assert torch.equal(getattr(a, f)[nm], getattr(b, f)[nm]), (nm, f)


@pytest.fixture(scope="module")
def reference_call():
    """One call per pooling: its histogram and the trajectory the same call returned.  Shared, never modified."""
    out = {}
    for pool in (None, "chains"):
        um, model, data, inputs = _net(DEV)
        tr, res = _call(um, model, data, inputs, dict(SPEC, pool=pool))
        assert tr.last_call_mode == "fused" and tr.last_record_slices == 1
        out[pool] = (tr.mcpc_last_histogram, _trajectory(res))
    return out


@pytest.mark.parametrize("pool", [None, "chains"])
def test_counts_equal_the_histogram_of_the_recorded_trajectory(reference_call, pool):
    h, traj = reference_call[pool]
    assert h.names == NAMES and h.n == len(STEPS) == 14 and h.B == B and h.pooled == (pool == "chains")
    assert h.N == (14 * B if pool else 14)
    some_outside = 0
    for nm, nb in zip(NAMES, (19, 64, 6)):
        e = h.edges[nm]
        assert e.dtype == torch.float32 and e.numel() == nb + 1 and e.device.type == "cuda" and h.counts[nm].dtype == torch.int64
        bins, under, over, nan = ref_hist(traj[nm].reshape(len(STEPS), -1), e.cpu().numpy())
        w = traj[nm].shape[2]
        bins, under, over, nan = bins.reshape(B, w, nb), under.reshape(B, w), over.reshape(B, w), nan.reshape(B, w)
        if pool:
            bins, under, over, nan = bins.sum(0), under.sum(0), over.sum(0), nan.sum(0)
        assert np.array_equal(h.counts[nm].cpu().numpy(), bins) and np.array_equal(h.under[nm].cpu().numpy(), under)
        assert np.array_equal(h.over[nm].cpu().numpy(), over) and np.array_equal(h.nan[nm].cpu().numpy(), nan)
        assert bool((h.total(nm) == h.N).all()) and int(h.nan[nm].sum()) == 0
        some_outside += int(under.sum() + over.sum())
    assert some_outside > 0                                  # the ranges cut the data: under / over are exercised
    assert np.array_equal(h.edges["x0"].cpu().numpy(), np.linspace(-1.5, 2.5, 20).astype(np.float32))
    # the arithmetic on the model's device
    d = h.density("x2")
    assert d.device.type == "cuda" and d.dtype == torch.float64
    q = h.quantile("x2", [0.25, 0.5, 0.75])
    ok = ~torch.isnan(q).any(-1)
    assert bool(ok.any()) and bool((q[ok][:, 0] <= q[ok][:, 1]).all()) and bool((q[ok][:, 1] <= q[ok][:, 2]).all())


def test_pool_method_is_the_pooled_request(reference_call):
    _same(reference_call[None][0].pool(), reference_call["chains"][0])


@pytest.mark.parametrize("every_t", [True, False])
def test_nothing_else_moves_in_a_learning_call(every_t):
    um, model, data, inputs = _net(DEV)
    w0 = {k: v.clone() for k, v in model.state_dict().items() if "_x" not in k}

    def state(tr, res):
        xs = [x.detach().clone() for x in tr.get_model_xs()]
        lin = [p for m in model if isinstance(m, torch.nn.Linear) for p in m.parameters()]
        return xs, [p.grad.clone() for p in lin], [p.detach().clone() for p in lin], {k: res[k] for k in ("loss", "energy", "overall")}
    runs = []
    for hist in (None, dict(SPEC), dict(SPEC, pool="chains", outputs="sigmoid", bins=20, range=(-2.0, 2.0))):
        model.load_state_dict(w0, strict=False)
        for p in model.parameters():
            p.grad = None
        tr, res = _call(um, model, data, inputs, hist, every_t=every_t, update_p_at="last")
        assert tr.last_call_mode == "fused"
        runs.append((tr, res, state(tr, res)))
    assert runs[0][0].mcpc_last_histogram is None and runs[1][0].mcpc_last_histogram.n == 14
    xs0, g0, p0, e0 = runs[0][2]
    assert len(g0) == len(p0) == 8
    for _, res, (xs, g, p, e) in runs[1:]:
        assert e == e0
        for a, b in zip(xs0 + g0 + p0, xs + g + p):
            assert torch.equal(a, b)
        assert len(res["outputs"]) == len(runs[0][1]["outputs"]) >= 1
        for t in range(len(res["outputs"])):
            assert torch.equal(res["outputs"][t], runs[0][1]["outputs"][t])
            for a, b in zip(res["xs"][t], runs[0][1]["xs"][t]):
                assert torch.equal(a, b)


@pytest.mark.parametrize("pool", [None, "chains"])
def test_sliced_call_gives_equal_counts(reference_call, pool):
    um, model, data, inputs = _net(DEV)
    step_bytes = 4 * B * (SIZES[0] + SIZES[2] + N_OUT)
    cut, _ = _call(um, model, data, inputs, dict(SPEC, pool=pool), chunk=10 * step_bytes, xs=False, outputs=False)
    assert cut.last_record_slices > 1
    _same(cut.mcpc_last_histogram, reference_call[pool][0])


def test_composes_with_moments_chain_energies_and_covariance(reference_call):
    um, model, data, inputs = _net(DEV)
    cov = dict(begin=13, stride=3, layers=(0, 2), outputs="identity")
    mom, ce = dict(begin=20, stride=3, layers=(0, 2), outputs="identity"), dict(begin=7, stride=5)
    kw = dict(xs=False, outputs=False)
    alone_c = _call(um, model, data, inputs, None, covariance=cov, **kw)[0]
    alone_m = _call(um, model, data, inputs, None, moments=mom, **kw)[0]
    alone_e = _call(um, model, data, inputs, None, chain_energies=ce, **kw)[0]
    alone_h = _call(um, model, data, inputs, dict(SPEC), **kw)[0]
    every = _call(um, model, data, inputs, dict(SPEC), moments=mom, chain_energies=ce, covariance=cov, **kw)[0]
    assert alone_m.mcpc_last_histogram is None and alone_h.mcpc_last_moments is None and alone_h.mcpc_last_covariance is None
    _same(alone_h.mcpc_last_histogram, reference_call[None][0])              # with and without the caller's records
    _same(every.mcpc_last_histogram, alone_h.mcpc_last_histogram)            # exact
    m, k = alone_m.mcpc_last_moments, every.mcpc_last_moments
    for p, q in ((m.out_sum, k.out_sum), (m.out_sumsq, k.out_sumsq), (m.x_sum[0], k.x_sum[0]), (m.x_sumsq[2], k.x_sumsq[2])):
        assert torch.equal(p, q)                             # bitwise
    e, f = alone_e.mcpc_last_chain_energies, every.mcpc_last_chain_energies
    assert e.steps == f.steps and torch.equal(e.loss, f.loss) and torch.equal(e.energy, f.energy) and torch.equal(e.overall, f.overall)
    a, b = alone_c.mcpc_last_covariance, every.mcpc_last_covariance          # as tests/test_gpu_cov_facade.py states it: bitwise
    assert torch.equal(a.sum, b.sum) and torch.equal(a.outer, b.outer) and a.columns == b.columns


def test_read_out_paths():
    """outputs="sigmoid" on a Bernoulli call; the outputs binned out of the caller's own buffer (every step's outputs are returned:
    the slices write them in place) and out of the ring give equal counts."""
    um, model, data, inputs = _net(DEV)
    spec = dict(begin=20, stride=3, outputs="sigmoid", bins=20, range=(0.0, 1.0))
    direct, res = _call(um, model, data, inputs, spec, xs=False, outputs=True, every_t=True)
    ring, _ = _call(um, model, data, inputs, spec, xs=False, outputs=False, every_t=True)
    last, _ = _call(um, model, data, inputs, spec, xs=False, outputs=True, every_t=False)
    h = direct.mcpc_last_histogram
    assert h.names == ["out"] and tuple(h.counts["out"].shape) == (B, N_OUT, 20)
    assert bool((h.total("out") == 14).all()) and int(h.under["out"].sum() + h.over["out"].sum() + h.nan["out"].sum()) == 0
    _same(h, ring.mcpc_last_histogram)
    _same(h, last.mcpc_last_histogram)
    # against the fp64 sigmoid of the recorded logits, away from the edges (the kernel test bounds the values next to one)
    logits = np.stack([res["outputs"][t].detach().cpu().numpy() for t in STEPS]).astype(np.float64)
    ref = 1.0 / (1.0 + np.exp(-logits))
    e64 = h.edges["out"].cpu().numpy().astype(np.float64)
    clear = (np.abs(ref[..., None] - e64[1:-1]) > 1e-6).all(-1).all(0)       # [B, N_OUT]: no sample of this histogram near an edge
    want = ref_hist(ref.astype(np.float32), e64.astype(np.float32))[0]
    assert clear.mean() > 0.9 and np.array_equal(h.counts["out"].cpu().numpy()[clear], want[clear])


def test_calls_that_are_not_fused_are_rejected():
    import montecarlopredictivecoding_amd.predictive_coding as pc
    um, model, data, inputs = _net(DEV)
    with pytest.raises(NotImplementedError, match="mcpc_histogram is set.*step by step.*update_p_at"):
        _call(um, model, data, inputs, dict(layers=(0,), bins=4, range=(0, 1)), update_p_at="all")
    assert all(m.get_x() is None for m in model if hasattr(m, "get_x"))      # before any work
    masked = torch.nn.Sequential(torch.nn.Linear(3, 3), pc.PCLayer(M=torch.ones(3, device=DEV)), torch.nn.Linear(3, 2)).to(DEV)
    masked.train()
    tr = pc.PCTrainer(masked, T=3, update_p_at="never", plot_progress_at=[])
    tr.mcpc_histogram = dict(layers=(0,), bins=4, range=(0, 1))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(NotImplementedError, match="mcpc_histogram is set.*generic torch loop.*S/M masks"):
            tr.train_on_batch(inputs=torch.zeros(2, 3, device=DEV), is_log_progress=False, is_return_results_every_t=False)
    # a bad request on a call that would be fused: ValueError, before any work
    with pytest.raises(ValueError, match="layer index"):
        _call(um, model, data, inputs, dict(layers=(3,), bins=4, range=(0, 1)))
    with pytest.raises(ValueError, match="needs range"):
        _call(um, model, data, inputs, dict(layers=(0,), bins=4))
    need = 8 * 37 * (6 * 22 + 16 * 67 + 24 * 9)
    with pytest.raises(ValueError, match=r"mcpc_histogram_max_bytes.*fewer layers or fewer bins or pool='chains'"):
        _call(um, model, data, inputs, dict(SPEC), max_bytes=need - 1)
    assert all(m.get_x() is None for m in model if hasattr(m, "get_x"))
    tr, _ = _call(um, model, data, inputs, dict(SPEC), max_bytes=need, xs=False, outputs=False)
    assert tr.mcpc_last_histogram.n == 14


def test_cpu_built_model():
    results = []
    for device in (DEV, "cpu"):
        um, model, data, inputs = _net(device)
        results.append(_call(um, model, data, inputs, dict(SPEC), xs=False, outputs=False)[0].mcpc_last_histogram)
    dev, cpu = results
    assert all(cpu.counts[nm].device.type == cpu.edges[nm].device.type == cpu.under[nm].device.type == "cpu" for nm in NAMES)
    assert cpu.density("x0").device.type == "cpu" and dev.counts["x0"].device.type == "cuda"
    for nm in NAMES:
        for f in ("counts", "under", "over", "nan", "edges"):
            assert torch.equal(getattr(cpu, f)[nm], getattr(dev, f)[nm].cpu())


def test_get_posterior_histogram():
    import montecarlopredictivecoding_amd.predictive_coding.pc_trainer as pt
    import montecarlopredictivecoding_amd.utils.model as um
    from montecarlopredictivecoding_amd.utils.training_evaluation import get_mcpc_trainer, get_pc_trainer
    torch.manual_seed(5)
    cfg = dict(input_size=SIZES[0], hidden_size=SIZES[1], hidden2_size=SIZES[2], output_size=N_OUT, activation_fn="relu",
               loss_fn=um.bernoulli_fn, input_var=0.3, T_pc=40, optimizer_x_fn_pc=torch.optim.Adam, optimizer_x_kwargs_pc={"lr": 0.1},
               mixing=20, sampling=40, optimizer_x_kwargs_mcpc={"lr": 0.03},
               optimizer_p_fn_mcpc=torch.optim.Adam, optimizer_p_kwargs_mcpc={"lr": 0.01})
    model = um.get_model(cfg, True, sample_x_fn=um.sample_x_fn_normal)
    g = torch.Generator().manual_seed(2)
    data = (torch.rand(32, N_OUT, generator=g) < 0.3).float()
    labels = torch.arange(32) % 10
    loader = DataLoader(TensorDataset(data, labels), batch_size=16)
    trainers = [get_pc_trainer(model, cfg, is_mcpc=True, training=False), get_mcpc_trainer(model, cfg, training=False)]
    base = pt._PHILOX_STEPS[0]
    kw = dict(layers=(0, 1), bins=30, range=(-3.0, 3.0))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(7)
        per, lab = um.get_posterior_histogram(model, cfg, trainers, loader, **kw)
        pt._PHILOX_STEPS[0] = base
        torch.manual_seed(7)
        pooled, plab = um.get_posterior_histogram(model, cfg, trainers, loader, pool="chains", **kw)
        # the same run again, keeping what every batch's call left behind
        pt._PHILOX_STEPS[0] = base
        torch.manual_seed(7)
        halves, orig = [], trainers[1].train_on_batch

        def spy(*a, **k):
            r = orig(*a, **k)
            halves.append(trainers[1].mcpc_last_histogram)
            return r
        trainers[1].train_on_batch = spy
        again, _ = um.get_posterior_histogram(model, cfg, trainers, loader, pool="chains", **kw)
        trainers[1].train_on_batch = orig
        pt._PHILOX_STEPS[0] = base
    assert trainers[1].mcpc_histogram is None
    assert torch.equal(lab.cpu(), labels) and torch.equal(plab, lab)
    assert (per.n, per.B, per.pooled, per.names) == (40, 32, False, ["x0", "x1"]) and tuple(per.counts["x1"].shape) == (32, 16, 30)
    assert bool((per.total("x0") == 40).all())
    assert (pooled.n, pooled.B, pooled.pooled) == (80, 16, True) and bool((pooled.total("x1") == 80 * 16).all())
    assert len(halves) == 2 and halves[0].n == halves[1].n == 40 and halves[0].pooled
    _same(again, halves[0].merge(halves[1]))
    _same(pooled, again)
    for nm in per.names:                                     # pooled over the chains of every batch = all data summed
        for f in ("counts", "under", "over", "nan"):
            assert torch.equal(getattr(per, f)[nm].sum(0), getattr(pooled, f)[nm])

"""The posterior of a linear probe on the device, the trainer: `PCTrainer.mcpc_probe` against the recorded trajectory of the same call.
The logits are bitwise the sequential fp64 loop, so with the identity link the sums and votes of the call equal the host loop
(tests/probe_cases.py) on the trajectory the same call returns, exactly, however the call is sliced; the softmax sums are held to the
bounds derived in tests/probe_cases.py."""
import warnings

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from tests import probe_cases as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES, N_OUT, B, T = (6, 16, 16), 24, 37, 60
C = 5
BEGIN = 20
ACOV = dict(begin=20, stride=1, layers=(0, 2), outputs="identity", max_lag=8)
HIST = dict(begin=20, stride=3, layers=(0, 2), outputs="identity", bins=19, range=(-3.0, 3.0))
COV = dict(begin=13, stride=3, layers=(0, 2), outputs="identity")
MOM = dict(begin=20, stride=1, layers=(0, 2), outputs="identity")
CE = dict(begin=7, stride=5)


def _readout(layer, sizes=SIZES):
    """The probe's read-out on `layer`: fp32 W [C, width] and bias [C], the same on every call."""
    g = torch.Generator().manual_seed(40 + layer)
    w = sizes[layer]
    return torch.randn(C, w, generator=g) / w ** 0.5, torch.randn(C, generator=g) * 0.5


def _spec(layer, link="softmax", sizes=SIZES, **kw):
    W, b = _readout(layer, sizes)
    return dict(dict(begin=BEGIN, stride=1, layer=layer, weight=W, bias=b, link=link), **kw)


def _net(device, sizes=SIZES, batch=B):
    """6-16-16 -> 24, ReLU, Bernoulli loss; the same weights, data and x0 on whichever device."""
    import montecarlopredictivecoding_amd.utils.model as um
    torch.manual_seed(3)
    cfg = dict(input_size=sizes[0], hidden_size=sizes[1], hidden2_size=sizes[2], output_size=N_OUT, activation_fn="relu")
    model = um.get_model(cfg, False)
    g = torch.Generator().manual_seed(8)
    x0 = [torch.randn(batch, n, generator=g) for n in sizes]
    for layer, x in zip([m for m in model if hasattr(m, "get_x")], x0):
        layer._sample_x_fn = lambda inp, _x=x: _x.clone().to(inp["mu"].device)
    data = (torch.rand(batch, N_OUT, generator=g) < 0.3).float()
    model.to(device)
    return um, model, data.to(device), torch.zeros(batch, sizes[0], device=device)


def _call(um, model, data, inputs, probe, chunk=None, every_t=True, update_p_at="never", xs=True, outputs=False, moments=None,
          chain_energies=None, covariance=None, histogram=None, autocovariance=None, steps=T, noise=True):
    import montecarlopredictivecoding_amd.predictive_coding as pc
    import montecarlopredictivecoding_amd.predictive_coding.pc_trainer as pt
    tr = pc.PCTrainer(model, T=steps, optimizer_x_fn=torch.optim.SGD, optimizer_x_kwargs={"lr": 0.05}, update_p_at=update_p_at,
                      accumulate_p_at=list(range(40, steps)) if update_p_at == "last" else "never",
                      optimizer_p_fn=torch.optim.Adam, optimizer_p_kwargs={"lr": 0.01}, plot_progress_at=[])
    tr.mcpc_seed = 5
    tr.mcpc_probe = probe
    tr.mcpc_moments = moments
    tr.mcpc_chain_energies = chain_energies
    tr.mcpc_covariance = covariance
    tr.mcpc_histogram = histogram
    tr.mcpc_autocovariance = autocovariance
    if chunk is not None:
        tr.mcpc_moments_chunk_bytes = chunk
    base = pt._PHILOX_STEPS[0]
    kick = dict(callback_after_t=um.random_step, callback_after_t_kwargs={"_pc_trainer": tr}) if noise else {}
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = tr.train_on_batch(inputs=inputs, is_log_progress=False, is_return_results_every_t=every_t, is_return_xs=xs,
                                is_return_outputs=outputs, loss_fn=um.bernoulli_fn, loss_fn_kwargs={"_target": data, "_var": None}, **kick)
    pt._PHILOX_STEPS[0] = base                               # the next run replays the same noise
    tr.caught = caught
    return tr, res


def _trajectory(res, layer, steps):
    return np.stack([res["xs"][t][layer].detach().cpu().numpy() for t in steps])


def _same(a, b):
    assert (a.n, a.B, a.C, a.link) == (b.n, b.B, b.C, b.link)
    for f in ("psum", "psumsq", "votes", "entsum"):
        if getattr(a, f) is not None:
            assert torch.equal(getattr(a, f), getattr(b, f)), f


def _against_the_host_loop(p, g, spec, batch=B):
    """`p`: the call's Probe; `g`: fp32 [n, batch, w], the samples of its layer as the same call returned them."""
    n, link = g.shape[0], spec["link"]
    v = R.logits(g, spec["weight"].numpy(), None if spec["bias"] is None else spec["bias"].numpy())
    assert (p.n, p.B, p.C, p.link) == (n, batch, C, link)
    assert p.psum.dtype == p.psumsq.dtype == torch.float64 and p.votes.dtype == torch.int64 and p.psum.device.type == "cuda"
    assert tuple(p.psum.shape) == tuple(p.psumsq.shape) == (batch, C) and tuple(p.votes.shape) == (batch, C + 1)
    assert np.array_equal(p.votes.cpu().numpy(), R.votes(v)) and bool((p.votes.sum(dim=1) == n).all())
    if link != "softmax":
        s, q = R.sums(v if link == "identity" else R.device_sigmoid(v, DEV))
        assert p.entsum is None
        assert np.array_equal(p.psum.cpu().numpy(), s) and np.array_equal(p.psumsq.cpu().numpy(), q)
    else:
        pr, H = R.softmax64(v)
        ep = np.abs(p.psum.cpu().numpy() - pr.sum(axis=0)).max()
        eq = np.abs(p.psumsq.cpu().numpy() - (pr * pr).sum(axis=0)).max()
        eh = np.abs(p.entsum.cpu().numpy() - H.sum(axis=0)).max()
        print("n=%d: |psum - ref| = %.3g (bound %.3g), |psumsq - ref| = %.3g, |entsum - ref| = %.3g (bound %.3g)"
              % (n, ep, n * R.p_bound(C), eq, eh, n * R.h_bound(C)))
        assert ep <= n * R.p_bound(C) and eq <= 2 * n * R.p_bound(C) and eh <= n * R.h_bound(C)
        assert tuple(p.entsum.shape) == (batch,)
        mean = p.mean()
        assert mean.dtype == torch.float64 and float((mean.sum(dim=1) - 1).abs().max()) <= C * R.p_bound(C)
        assert bool(torch.isfinite(p.mutual_information()).all()) and bool((p.entropy() <= np.log(C) + 1e-12).all())
        assert bool((p.var() >= 0).all()) and tuple(p.predict().shape) == (batch,)
        assert float((p.vote_share().sum(dim=1) - 1).abs().max()) <= 1e-12


@pytest.fixture(scope="module")
def reference_calls():
    """Per (layer, link) the call's result and the samples of the layer as the same call returned them.  Shared, never modified."""
    out = {}
    for layer in (0, 2):
        for link in ("identity", "softmax"):
            um, model, data, inputs = _net(DEV)
            tr, res = _call(um, model, data, inputs, _spec(layer, link))
            assert tr.last_call_mode == "fused" and tr.last_record_slices == 1
            out[layer, link] = (tr.mcpc_last_probe, _trajectory(res, layer, range(BEGIN, T)))
    return out


@pytest.mark.parametrize("link", ["identity", "softmax"])
@pytest.mark.parametrize("layer", [0, 2])
def test_the_sums_are_the_host_loop_on_the_recorded_trajectory(reference_calls, layer, link):
    p, g = reference_calls[layer, link]
    _against_the_host_loop(p, g, _spec(layer, link))


def test_stride_a_linear_and_no_bias():
    um, model, data, inputs = _net(DEV)
    W, b = _readout(2)
    lin = torch.nn.Linear(16, C).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(W)
        lin.bias.copy_(b)
    tr, res = _call(um, model, data, inputs, dict(begin=13, stride=3, layer=2, linear=lin, link="identity"))
    steps = range(13, T, 3)
    _against_the_host_loop(tr.mcpc_last_probe, _trajectory(res, 2, steps), _spec(2, "identity"))
    tr, res = _call(um, model, data, inputs, _spec(0, "sigmoid", bias=None))
    _against_the_host_loop(tr.mcpc_last_probe, _trajectory(res, 0, range(BEGIN, T)), _spec(0, "sigmoid", bias=None))


@pytest.mark.parametrize("per_slice, slices", [(T, 1), (30, 2), (7, 9)])
@pytest.mark.parametrize("layer", [0, 2])
def test_a_sliced_call_gives_the_same_bits(reference_calls, layer, per_slice, slices):
    um, model, data, inputs = _net(DEV)
    cut, _ = _call(um, model, data, inputs, _spec(layer), chunk=per_slice * 4 * B * SIZES[layer], xs=False)
    assert cut.last_record_slices == slices
    _same(cut.mcpc_last_probe, reference_calls[layer, "softmax"][0])


def test_all_six_features_compose_in_a_learning_call(reference_calls):
    um, model, data, inputs = _net(DEV)
    w0 = {k: v.clone() for k, v in model.state_dict().items() if "_x" not in k}
    runs = []
    for probe in (None, _spec(2)):
        model.load_state_dict(w0, strict=False)
        for p in model.parameters():
            p.grad = None
        tr, res = _call(um, model, data, inputs, probe, update_p_at="last", xs=False, outputs=True, every_t=False, moments=dict(MOM),
                        chain_energies=dict(CE), covariance=dict(COV), histogram=dict(HIST), autocovariance=dict(ACOV))
        assert tr.last_call_mode == "fused"
        lin = [p for m in model if isinstance(m, torch.nn.Linear) for p in m.parameters()]
        runs.append((tr, [p.grad.clone() for p in lin], [p.detach().clone() for p in lin],
                     [x.detach().clone() for x in tr.get_model_xs()], {k: res[k] for k in ("loss", "energy", "overall")},
                     [o.detach().clone() for o in res["outputs"]]))
    (t0, g0, p0, x0, e0, o0), (t1, g1, p1, x1, e1, o1) = runs
    assert t0.mcpc_last_probe is None and len(g0) == 8
    _same(t1.mcpc_last_probe, reference_calls[2, "softmax"][0])                      # the steps before the learning window's end: the same
    assert e0 == e1 and len(o0) == len(o1)
    for a, b in zip(g0 + p0 + x0 + o0, g1 + p1 + x1 + o1):
        assert torch.equal(a, b)                                                     # param.grad, the parameters, x, outputs: bitwise
    m, k = t0.mcpc_last_moments, t1.mcpc_last_moments
    for p, q in ((m.out_sum, k.out_sum), (m.out_sumsq, k.out_sumsq), (m.x_sum[0], k.x_sum[0]), (m.x_sumsq[2], k.x_sumsq[2])):
        assert torch.equal(p, q)
    e, f = t0.mcpc_last_chain_energies, t1.mcpc_last_chain_energies
    assert e.steps == f.steps and torch.equal(e.loss, f.loss) and torch.equal(e.energy, f.energy) and torch.equal(e.overall, f.overall)
    a, b = t0.mcpc_last_covariance, t1.mcpc_last_covariance
    assert torch.equal(a.sum, b.sum) and torch.equal(a.outer, b.outer) and a.columns == b.columns
    h, i = t0.mcpc_last_histogram, t1.mcpc_last_histogram
    for nm in h.names:
        for fld in ("counts", "under", "over", "nan"):
            assert torch.equal(getattr(h, fld)[nm], getattr(i, fld)[nm])
    a, b = t0.mcpc_last_autocovariance, t1.mcpc_last_autocovariance
    for nm in a.names:
        for fld in ("lagged", "sum", "head", "tail"):
            assert torch.equal(getattr(a, fld)[nm], getattr(b, fld)[nm])


def test_the_state_probe_is_the_kernel_on_the_current_x():
    from montecarlopredictivecoding_amd.engine import probe_accumulate
    from montecarlopredictivecoding_amd.probe import new_state
    um, model, data, inputs = _net(DEV)
    tr, _ = _call(um, model, data, inputs, None, xs=False, every_t=False, noise=False)           # a MAP call
    assert tr.last_call_mode == "fused" and tr.mcpc_last_probe is None
    xs = [x.detach().clone() for x in tr.get_model_xs()]
    for layer in (0, 2):
        for link in ("softmax", "identity"):
            spec = _spec(layer, link)
            p = tr.mcpc_state_probe(spec)
            st = new_state(B, C, link, DEV)
            probe_accumulate(xs[layer].unsqueeze(0).contiguous(), 0, 1, 1, spec["weight"].to(DEV), spec["bias"].to(DEV), link,
                             st["psum"], st["psumsq"], st["votes"], st["entsum"], accumulate=False)
            assert (p.n, p.B, p.C, p.link) == (1, B, C, link) and p.psum.device.type == "cuda"
            for f in ("psum", "psumsq", "votes", "entsum"):
                if st[f] is not None:
                    assert torch.equal(getattr(p, f), st[f]), f
            _against_the_host_loop(p, xs[layer].cpu().numpy()[None], spec)
    assert all(torch.equal(a, b) for a, b in zip(xs, tr.get_model_xs()))                           # nothing moved
    with pytest.raises(ValueError, match="mcpc_probe: layer index"):
        tr.mcpc_state_probe(dict(_spec(0), layer=3))


def test_calls_that_are_not_fused_are_rejected():
    import montecarlopredictivecoding_amd.predictive_coding as pc
    um, model, data, inputs = _net(DEV)
    with pytest.raises(NotImplementedError, match="mcpc_probe is set.*step by step.*update_p_at"):
        _call(um, model, data, inputs, _spec(0), update_p_at="all")
    assert all(m.get_x() is None for m in model if hasattr(m, "get_x"))              # before any work
    masked = torch.nn.Sequential(torch.nn.Linear(3, 3), pc.PCLayer(M=torch.ones(3, device=DEV)), torch.nn.Linear(3, 2)).to(DEV)
    masked.train()
    tr = pc.PCTrainer(masked, T=3, update_p_at="never", plot_progress_at=[])
    tr.mcpc_probe = dict(layer=0, weight=torch.zeros(2, 3))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(NotImplementedError, match="mcpc_probe is set.*generic torch loop.*S/M masks"):
            tr.train_on_batch(inputs=torch.zeros(2, 3, device=DEV), is_log_progress=False, is_return_results_every_t=False)
    # a bad request on a call that would be fused: ValueError, before any work
    with pytest.raises(ValueError, match="mcpc_probe: layer index"):
        _call(um, model, data, inputs, dict(_spec(0), layer=3))
    with pytest.raises(ValueError, match=r"mcpc_probe: weight is \(5, 6\), layer 1 is 16 wide"):
        _call(um, model, data, inputs, dict(_spec(0), layer=1))
    assert all(m.get_x() is None for m in model if hasattr(m, "get_x"))


def test_a_wide_layer_on_the_layer_wise_path():
    """6-1024-1024 -> 24: no LDS plan holds the hidden width, the call runs on the layer-wise step kernels; the probe reads the ring
    alone, and W goes through LDS in 16 k-tiles."""
    sizes, batch, steps = (6, 1024, 1024), 8, 12
    um, model, data, inputs = _net(DEV, sizes, batch)
    spec = _spec(2, "identity", sizes, begin=3)
    tr, res = _call(um, model, data, inputs, spec, steps=steps)
    assert tr.last_call_mode == "fused"
    assert any("layer-wise kernels" in str(w.message) for w in tr.caught), [str(w.message) for w in tr.caught]
    g = _trajectory(res, 2, range(3, steps))
    _against_the_host_loop(tr.mcpc_last_probe, g, spec, batch)
    soft = dict(spec, link="softmax")
    tr, res = _call(um, model, data, inputs, soft, steps=steps)
    _against_the_host_loop(tr.mcpc_last_probe, _trajectory(res, 2, range(3, steps)), soft, batch)


def test_cpu_built_model(reference_calls):
    um, model, data, inputs = _net("cpu")
    tr, _ = _call(um, model, data, inputs, _spec(2), xs=False)
    cpu, dev = tr.mcpc_last_probe, reference_calls[2, "softmax"][0]
    assert all(getattr(cpu, f).device.type == "cpu" for f in ("psum", "psumsq", "votes", "entsum")) and cpu.entropy().device.type == "cpu"
    for f in ("psum", "psumsq", "votes", "entsum"):
        assert torch.equal(getattr(cpu, f), getattr(dev, f).cpu()), f
    state = tr.mcpc_state_probe(_spec(2))
    assert state.psum.device.type == "cpu" and state.n == 1 and int(state.votes.sum()) == B


def test_get_posterior_class_probabilities():
    import montecarlopredictivecoding_amd.predictive_coding.pc_trainer as pt
    import montecarlopredictivecoding_amd.utils.model as um
    from montecarlopredictivecoding_amd.probe import Probe
    from montecarlopredictivecoding_amd.utils.training_evaluation import get_mcpc_trainer, get_pc_trainer
    torch.manual_seed(5)
    cfg = dict(input_size=SIZES[0], hidden_size=SIZES[1], hidden2_size=SIZES[2], output_size=N_OUT, activation_fn="relu",
               loss_fn=um.bernoulli_fn, input_var=0.3, T_pc=40, optimizer_x_fn_pc=torch.optim.Adam, optimizer_x_kwargs_pc={"lr": 0.1},
               mixing=20, sampling=40, optimizer_x_kwargs_mcpc={"lr": 0.03},
               optimizer_p_fn_mcpc=torch.optim.Adam, optimizer_p_kwargs_mcpc={"lr": 0.01})
    model = um.get_model(cfg, True, sample_x_fn=um.sample_x_fn_normal)

    class Classifier(torch.nn.Module):                                               # the shape of MNIST_LinearClassifier: one Linear inside
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(SIZES[0], 10)

        def forward(self, x):
            return self.lin(x)

    clf = Classifier().to(next(model.parameters()).device)
    g = torch.Generator().manual_seed(2)
    data = (torch.rand(32, N_OUT, generator=g) < 0.3).float()
    labels = torch.arange(32) % 10
    loader = DataLoader(TensorDataset(data, labels), batch_size=16)
    trainers = [get_pc_trainer(model, cfg, is_mcpc=True, training=False), get_mcpc_trainer(model, cfg, training=False)]

    def run(fn):
        base = pt._PHILOX_STEPS[0]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            torch.manual_seed(7)
            out = fn()
        pt._PHILOX_STEPS[0] = base
        return out

    trainers[1].mcpc_probe = "kept"
    p, lab = run(lambda: um.get_posterior_class_probabilities(model, cfg, trainers, loader, clf, layer=0))
    assert trainers[1].mcpc_probe == "kept"                                          # the previous setting is back
    trainers[1].mcpc_probe = None
    assert torch.equal(lab.cpu(), labels)
    assert (p.n, p.B, p.C, p.link) == (40, 32, 10, "softmax") and tuple(p.psum.shape) == (32, 10) and tuple(p.entsum.shape) == (32,)
    assert bool((p.votes.sum(dim=1) == 40).all()) and float((p.mean().sum(dim=1) - 1).abs().max()) <= 10 * R.p_bound(10)

    def two_calls():
        """The helper's protocol by hand, one batch at a time."""
        dev = next(model.parameters()).device
        trainers[1].mcpc_probe = dict(begin=20, stride=1, layer=0, linear=clf.lin, link="softmax")
        parts = []
        for d, _ in loader:
            d = d.to(dev)
            kw = dict(inputs=torch.zeros(d.shape[0], SIZES[0], device=dev), loss_fn=cfg["loss_fn"],
                      loss_fn_kwargs={"_target": d, "_var": cfg["input_var"]}, is_log_progress=False, is_return_results_every_t=False,
                      is_checking_after_callback_after_t=False)
            trainers[0].train_on_batch(**kw)
            trainers[1].train_on_batch(callback_after_t=um.random_step, callback_after_t_kwargs={"_pc_trainer": trainers[1]},
                                       is_sample_x_at_batch_start=False, **kw)
            parts.append(trainers[1].mcpc_last_probe)
        trainers[1].mcpc_probe = None
        return parts

    parts = run(two_calls)
    assert [q.B for q in parts] == [16, 16]
    _same(p, Probe.cat(parts))
    with pytest.raises(ValueError, match="exactly one"):
        um.get_posterior_class_probabilities(model, cfg, trainers, loader, torch.nn.Sequential(clf, torch.nn.Linear(10, 10)))

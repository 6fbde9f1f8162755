"""Lagged autocovariances on the device, the trainer: `PCTrainer.mcpc_autocovariance` against the recorded trajectory of the same call.
The kernel is bitwise the sequential fp64 loop over the samples in step order, so lagged, sum, head and tail of the call equal the host
loop (tests/acov_cases.py) on the trajectory the same call returns, exactly, however the call is sliced."""
import math
import warnings

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from tests.acov_cases import direct_acov, ref_stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES, N_OUT, B, T = (6, 16, 16), 24, 37, 60
K = 8
SPEC = dict(begin=20, stride=1, layers=(0, 2), outputs="identity", max_lag=K)
NAMES = ["x0", "x2", "out"]
HIST = dict(begin=20, stride=3, layers=(0, 2), outputs="identity", bins=19, range=(-3.0, 3.0))
COV = dict(begin=13, stride=3, layers=(0, 2), outputs="identity")
MOM = dict(begin=20, stride=1, layers=(0, 2), outputs="identity")
CE = dict(begin=7, stride=5)


def _net(device):
    """6-16-16 -> 24, ReLU, Bernoulli loss; the same weights, data and x0 on whichever device."""
    import montecarlopredictivecoding_amd.utils.model as um
    torch.manual_seed(3)
    cfg = dict(input_size=SIZES[0], hidden_size=SIZES[1], hidden2_size=SIZES[2], output_size=N_OUT, activation_fn="relu")
    model = um.get_model(cfg, False)
    g = torch.Generator().manual_seed(8)
    x0 = [torch.randn(B, n, generator=g) for n in SIZES]
    for layer, x in zip([m for m in model if hasattr(m, "get_x")], x0):
        layer._sample_x_fn = lambda inp, _x=x: _x.clone().to(inp["mu"].device)
    data = (torch.rand(B, N_OUT, generator=g) < 0.3).float()
    model.to(device)
    return um, model, data.to(device), torch.zeros(B, SIZES[0], device=device)


def _call(um, model, data, inputs, acov, chunk=None, every_t=True, update_p_at="never", xs=True, outputs=True, moments=None,
          chain_energies=None, covariance=None, histogram=None, max_bytes=None):
    import montecarlopredictivecoding_amd.predictive_coding as pc
    import montecarlopredictivecoding_amd.predictive_coding.pc_trainer as pt
    tr = pc.PCTrainer(model, T=T, optimizer_x_fn=torch.optim.SGD, optimizer_x_kwargs={"lr": 0.05}, update_p_at=update_p_at,
                      accumulate_p_at=list(range(40, T)) if update_p_at == "last" else "never",
                      optimizer_p_fn=torch.optim.Adam, optimizer_p_kwargs={"lr": 0.01}, plot_progress_at=[])
    tr.mcpc_seed = 5
    tr.mcpc_autocovariance = acov
    tr.mcpc_moments = moments
    tr.mcpc_chain_energies = chain_energies
    tr.mcpc_covariance = covariance
    tr.mcpc_histogram = histogram
    if chunk is not None:
        tr.mcpc_moments_chunk_bytes = chunk
    if max_bytes is not None:
        tr.mcpc_autocovariance_max_bytes = max_bytes
    base = pt._PHILOX_STEPS[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = tr.train_on_batch(inputs=inputs, callback_after_t=um.random_step, callback_after_t_kwargs={"_pc_trainer": tr},
                                is_log_progress=False, is_return_results_every_t=every_t, is_return_xs=xs,
                                is_return_outputs=outputs, loss_fn=um.bernoulli_fn, loss_fn_kwargs={"_target": data, "_var": None})
    pt._PHILOX_STEPS[0] = base                               # the next run replays the same noise
    return tr, res


def _trajectory(res, steps, sigmoid=False):
    """Per block of SPEC: fp32 [n, B, w] from the records of the sample steps; the read-out through the device's own sigmoid."""
    out = {f"x{l}": np.stack([res["xs"][t][l].detach().cpu().numpy() for t in steps]) for l in (0, 2)}
    logits = torch.stack([res["outputs"][t].detach() for t in steps]).contiguous()
    if sigmoid:
        from montecarlopredictivecoding_amd.engine import moments_accumulate
        one = torch.zeros(B, N_OUT, dtype=torch.float64, device=DEV)
        rows = []
        for j in range(len(steps)):
            moments_accumulate(logits, j, 1, 1, one, None, transform="sigmoid", accumulate=False)     # 0 + g: exact
            rows.append(one.cpu().numpy().astype(np.float32))
        out["out"] = np.stack(rows)
    else:
        out["out"] = logits.cpu().numpy()
    return out


def _same(a, b):
    assert (a.n, a.B, a.max_lag, a.names) == (b.n, b.B, b.max_lag, b.names)
    for nm in a.names:
        for f in ("lagged", "sum", "head", "tail"):
            assert torch.equal(getattr(a, f)[nm], getattr(b, f)[nm]), (nm, f)


def _against_the_host_loop(a, traj, n):
    assert a.names == NAMES and a.n == n and a.B == B and a.max_lag == K
    for nm in NAMES:
        g = traj[nm]
        w = g.shape[2]
        lag, s, head, win = ref_stream(g.reshape(n, -1), K)[n]
        assert a.lagged[nm].dtype == a.sum[nm].dtype == torch.float64 and a.head[nm].dtype == a.tail[nm].dtype == torch.float32
        assert a.lagged[nm].device.type == "cuda" and tuple(a.lagged[nm].shape) == (B, w, K + 1) and tuple(a.tail[nm].shape) == (K, B, w)
        assert np.array_equal(a.lagged[nm].cpu().numpy().reshape(-1, K + 1), lag), nm
        assert np.array_equal(a.sum[nm].cpu().numpy().reshape(-1), s), nm
        v = head.shape[0]
        assert np.array_equal(a.head[nm].cpu().numpy()[:v].reshape(v, -1), head), nm
        assert np.array_equal(a.tail[nm].cpu().numpy()[:v].reshape(v, -1), win), nm
        want = direct_acov(g.reshape(n, -1), K)
        c = a.acov(nm)
        assert c.dtype == torch.float64 and c.device.type == "cuda"
        err = np.abs(c.cpu().numpy().reshape(-1, K + 1) - want).max()
        print("%s: max |acov - direct| = %.3g, max c_0 = %.3g" % (nm, err, want[:, 0].max()))
        assert err <= 1e-11 * want[:, 0].max(), nm


@pytest.fixture(scope="module")
def reference_call():
    """The call of SPEC: its result and the trajectory the same call returned.  Shared, never modified."""
    um, model, data, inputs = _net(DEV)
    tr, res = _call(um, model, data, inputs, dict(SPEC))
    assert tr.last_call_mode == "fused" and tr.last_record_slices == 1
    return tr.mcpc_last_autocovariance, _trajectory(res, range(20, T))


def test_the_state_is_the_host_loop_on_the_recorded_trajectory(reference_call):
    a, traj = reference_call
    _against_the_host_loop(a, traj, 40)
    tau, ess = a.tau("x2"), a.ess("x2")
    assert tau.device.type == "cuda" and tuple(tau.shape) == (B, 16) and tuple(a.acf("out").shape) == (B, N_OUT, K + 1)
    ok = torch.isfinite(ess)
    assert bool(ok.any()) and bool((ess[ok] > 0).all()) and bool((ess[ok] <= 40 * math.log10(40) * (1 + 1e-15)).all())


@pytest.mark.parametrize("stride, outputs", [(3, "identity"), (1, "sigmoid"), (3, "sigmoid")])
def test_stride_and_the_sigmoid_read_out(stride, outputs):
    um, model, data, inputs = _net(DEV)
    tr, res = _call(um, model, data, inputs, dict(SPEC, stride=stride, outputs=outputs))
    steps = range(20, T, stride)
    _against_the_host_loop(tr.mcpc_last_autocovariance, _trajectory(res, steps, sigmoid=outputs == "sigmoid"), len(steps))


@pytest.mark.parametrize("per_slice", [1, 5, 7])
def test_a_sliced_call_gives_the_same_bits(reference_call, per_slice):
    """Slices of fewer than K = 8 steps: every lag crosses slice boundaries through the kernel's window."""
    um, model, data, inputs = _net(DEV)
    step_bytes = 4 * B * (SIZES[0] + SIZES[2] + N_OUT)
    cut, _ = _call(um, model, data, inputs, dict(SPEC), chunk=per_slice * step_bytes, xs=False, outputs=False)
    assert cut.last_record_slices == -(-T // per_slice) > 2
    _same(cut.mcpc_last_autocovariance, reference_call[0])


def test_read_out_paths_and_moments_agree(reference_call):
    """The read-out taken out of the caller's own buffer (every step's outputs are returned) and out of the ring; the last step only;
    and `sum` is bitwise the x_sum of `mcpc_moments` on the same begin and stride."""
    um, model, data, inputs = _net(DEV)
    ring, _ = _call(um, model, data, inputs, dict(SPEC), xs=False, outputs=False, moments=dict(MOM))
    last, _ = _call(um, model, data, inputs, dict(SPEC), xs=False, outputs=True, every_t=False)
    _same(ring.mcpc_last_autocovariance, reference_call[0])
    _same(last.mcpc_last_autocovariance, reference_call[0])
    a, m = ring.mcpc_last_autocovariance, ring.mcpc_last_moments
    assert torch.equal(a.sum["x0"], m.x_sum[0]) and torch.equal(a.sum["x2"], m.x_sum[2]) and torch.equal(a.sum["out"], m.out_sum)
    assert torch.equal(a.lagged["x2"][..., 0], m.x_sumsq[2])                         # lag 0 is the sum of squares, the same bits


def test_all_five_features_compose_in_a_learning_call():
    um, model, data, inputs = _net(DEV)
    w0 = {k: v.clone() for k, v in model.state_dict().items() if "_x" not in k}
    runs = []
    for acov in (None, dict(SPEC)):
        model.load_state_dict(w0, strict=False)
        for p in model.parameters():
            p.grad = None
        tr, res = _call(um, model, data, inputs, acov, update_p_at="last", xs=False, outputs=False, every_t=False, moments=dict(MOM),
                        chain_energies=dict(CE), covariance=dict(COV), histogram=dict(HIST))
        assert tr.last_call_mode == "fused"
        lin = [p for m in model if isinstance(m, torch.nn.Linear) for p in m.parameters()]
        runs.append((tr, [p.grad.clone() for p in lin], [p.detach().clone() for p in lin],
                     [x.detach().clone() for x in tr.get_model_xs()], {k: res[k] for k in ("loss", "energy", "overall")}))
    (t0, g0, p0, x0, e0), (t1, g1, p1, x1, e1) = runs
    assert t0.mcpc_last_autocovariance is None and len(g0) == 8
    a = t1.mcpc_last_autocovariance
    assert (a.n, a.names) == (40, NAMES) and torch.equal(a.sum["x2"], t1.mcpc_last_moments.x_sum[2])
    assert torch.equal(a.lagged["out"][..., 0], t1.mcpc_last_moments.out_sumsq)
    assert e0 == e1
    for a, b in zip(g0 + p0 + x0, g1 + p1 + x1):
        assert torch.equal(a, b)                                                     # param.grad, the parameters, x: bitwise
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


def test_calls_that_are_not_fused_are_rejected():
    import montecarlopredictivecoding_amd.predictive_coding as pc
    um, model, data, inputs = _net(DEV)
    with pytest.raises(NotImplementedError, match="mcpc_autocovariance is set.*step by step.*update_p_at"):
        _call(um, model, data, inputs, dict(layers=(0,), max_lag=4), update_p_at="all")
    assert all(m.get_x() is None for m in model if hasattr(m, "get_x"))              # before any work
    masked = torch.nn.Sequential(torch.nn.Linear(3, 3), pc.PCLayer(M=torch.ones(3, device=DEV)), torch.nn.Linear(3, 2)).to(DEV)
    masked.train()
    tr = pc.PCTrainer(masked, T=3, update_p_at="never", plot_progress_at=[])
    tr.mcpc_autocovariance = dict(layers=(0,), max_lag=2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(NotImplementedError, match="mcpc_autocovariance is set.*generic torch loop.*S/M masks"):
            tr.train_on_batch(inputs=torch.zeros(2, 3, device=DEV), is_log_progress=False, is_return_results_every_t=False)
    # a bad request on a call that would be fused: ValueError, before any work
    with pytest.raises(ValueError, match="layer index"):
        _call(um, model, data, inputs, dict(layers=(3,), max_lag=4))
    with pytest.raises(ValueError, match="max_lag is required"):
        _call(um, model, data, inputs, dict(layers=(0,)))
    need = B * (SIZES[0] + SIZES[2] + N_OUT) * (8 * (K + 1) + 8 + 8 * K)
    with pytest.raises(ValueError, match=r"mcpc_autocovariance_max_bytes.*fewer layers or fewer lags"):
        _call(um, model, data, inputs, dict(SPEC), max_bytes=need - 1)
    assert all(m.get_x() is None for m in model if hasattr(m, "get_x"))
    tr, _ = _call(um, model, data, inputs, dict(SPEC), max_bytes=need, xs=False, outputs=False)
    assert tr.mcpc_last_autocovariance.n == 40


def test_cpu_built_model(reference_call):
    um, model, data, inputs = _net("cpu")
    cpu = _call(um, model, data, inputs, dict(SPEC), xs=False, outputs=False)[0].mcpc_last_autocovariance
    dev = reference_call[0]
    assert all(getattr(cpu, f)[nm].device.type == "cpu" for nm in NAMES for f in ("lagged", "sum", "head", "tail"))
    assert cpu.tau("x0").device.type == "cpu"
    for nm in NAMES:
        for f in ("lagged", "sum", "head", "tail"):
            assert torch.equal(getattr(cpu, f)[nm], getattr(dev, f)[nm].cpu())


def test_get_posterior_ess():
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
    trainers[1].mcpc_autocovariance = "kept"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(7)
        a, lab = um.get_posterior_ess(model, cfg, trainers, loader, layers=(0, 1), max_lag=12)
    pt._PHILOX_STEPS[0] = base
    assert trainers[1].mcpc_autocovariance == "kept"                                 # the previous setting is back
    trainers[1].mcpc_autocovariance = None
    assert torch.equal(lab.cpu(), labels)
    assert (a.n, a.B, a.max_lag, a.names) == (40, 32, 12, ["x0", "x1"])
    assert tuple(a.lagged["x1"].shape) == (32, 16, 13) and tuple(a.sum["x0"].shape) == (32, 6) and tuple(a.head["x1"].shape) == (12, 32, 16)
    for nm in a.names:
        ess, tau = a.ess(nm), a.tau(nm)
        assert tuple(ess.shape) == tuple(a.sum[nm].shape) and ess.dtype == torch.float64
        assert bool(torch.isfinite(ess).all()) and bool((ess > 0).all()) and bool((ess <= 40 * math.log10(40) * (1 + 1e-15)).all())
        assert torch.equal(ess, 40 / tau) and tuple(a.truncated(nm).shape) == tuple(ess.shape)
        assert bool(torch.isfinite(a.mcse(nm)).all())

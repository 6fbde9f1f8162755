"""Prediction errors through the trainer: `mcpc_errors` on a fused Langevin call against `Engine.prediction_errors` on the returned
trajectory with sequential fp64 sums on the host (bitwise), slicing, the covariance within `mcpc_cov_accumulate`'s documented bound,
composition with `mcpc_moments` and `mcpc_chain_energies`, `mcpc_state_errors`, the calls that must refuse the request, and the
posterior mean of the error units of the linear-Gaussian toy against its analytic value within the call's own Monte Carlo error."""
import warnings

import numpy as np
import pytest
import torch

from oracle import mcpc_oracle as mo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES, N_OUT, B, T = (6, 33, 17), 24, 20, 40            # ragged widths, a read-out with a Bernoulli loss
BEGIN, STRIDE = 7, 3
STEPS = list(range(BEGIN, T, STRIDE))
STEP_BYTES = 4 * B * sum(SIZES)


def _net(device=DEV):
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


def _call(um, model, data, inputs, spec, moments=None, chain_energies=None, chunk=None, **kw):
    import montecarlopredictivecoding_amd.predictive_coding as pc
    import montecarlopredictivecoding_amd.predictive_coding.pc_trainer as pt
    tr = pc.PCTrainer(model, T=T, optimizer_x_fn=torch.optim.SGD, optimizer_x_kwargs={"lr": 0.05}, update_p_at="never",
                      plot_progress_at=[])
    tr.mcpc_seed = 5
    tr.mcpc_errors = spec
    tr.mcpc_moments = moments
    tr.mcpc_chain_energies = chain_energies
    if chunk is not None:
        tr.mcpc_moments_chunk_bytes = chunk
    base = pt._PHILOX_STEPS[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = tr.train_on_batch(inputs=inputs, loss_fn=um.bernoulli_fn, loss_fn_kwargs={"_target": data, "_var": None},
                                callback_after_t=um.random_step, callback_after_t_kwargs={"_pc_trainer": tr}, is_log_progress=False,
                                is_return_results_every_t=True, **kw)
    pt._PHILOX_STEPS[0] = base                               # the next run replays the same noise
    return tr, res


def _engine(model, data):
    """An engine of the test's own with the model's parameters and the call's target."""
    from montecarlopredictivecoding_amd.engine import Engine
    lins = [m for m in model if isinstance(m, torch.nn.Linear)]
    eng = Engine(list(SIZES), [mo.ACT_RELU] * 3, SIZES[0], N_OUT, B, device=torch.device(DEV))
    eng.bind_params([m.weight.detach().contiguous() for m in lins], [m.bias.detach().contiguous() for m in lins])
    eng.bind_target(data.contiguous())
    return eng


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int64)


def _host_sums(rec):
    """Sequential fp64 sums over the records, in order: what moments_accumulate is bitwise held to."""
    v = rec.cpu().numpy().astype(np.float64)
    s, q = np.zeros(v.shape[1:]), np.zeros(v.shape[1:])
    for k in range(v.shape[0]):
        s += v[k]
        q += v[k] * v[k]
    return s, q


@pytest.fixture(scope="module")
def runs():
    """One fused call per quantity with the trajectory returned, the derived records of its sample steps from Engine.prediction_errors,
    and the same call in slices; computed once, never modified."""
    um, model, data, inputs = _net()
    out = {}
    for quantity in ("error", "prediction"):
        spec = dict(begin=BEGIN, stride=STRIDE, layers=(0, 1, 2), quantity=quantity, outputs=quantity, covariance="chain")
        tr, res = _call(um, model, data, inputs, spec, is_return_xs=True)
        assert tr.last_call_mode == "fused"
        traj = [torch.stack([res["xs"][t][l] for t in STEPS]).to(DEV).contiguous() for l in range(3)]
        eng = _engine(model, data)
        derived = eng.prediction_errors(None, traj, quantity=quantity, outputs=quantity, loss_kind=mo.LOSS_BERNOULLI)
        eng.sync_check()
        eng.close()
        sliced, _ = _call(um, model, data, inputs, spec, chunk=14 * STEP_BYTES)
        out[quantity] = dict(result=tr.mcpc_last_errors, derived=derived, sliced=sliced)
    return out


@pytest.mark.parametrize("quantity", ["error", "prediction"])
def test_sums_are_the_sequential_fp64_sums_of_the_derived_records(runs, quantity):
    r, derived = runs[quantity]["result"], runs[quantity]["derived"]
    names = ["e0", "e1", "e2", "eout"] if quantity == "error" else ["mu0", "mu1", "mu2", "out"]
    assert r.names == names == list(derived) and r.n == len(STEPS) == 11
    for name, w in zip(names, SIZES + (N_OUT,)):
        s, q = _host_sums(derived[name])
        assert r.sum[name].shape == (B, w) and r.sum[name].dtype == torch.float64 and r.sum[name].device.type == "cuda"
        assert np.array_equal(_bits(r.sum[name]), s.view(np.int64)), name
        assert np.array_equal(_bits(r.sumsq[name]), q.view(np.int64)), name
        assert (q > 0).any()
        np.testing.assert_allclose(r.rms(name).cpu().numpy(), np.sqrt(q / 11), rtol=1e-15)
        np.testing.assert_allclose(r.mean(name).cpu().numpy(), s / 11, rtol=1e-15)


@pytest.mark.parametrize("quantity", ["error", "prediction"])
def test_slicing_changes_no_bit_of_the_sums_and_the_covariance_stays_within_its_bound(runs, quantity):
    r, sliced, derived = runs[quantity]["result"], runs[quantity]["sliced"], runs[quantity]["derived"]
    assert sliced.last_record_slices >= 3
    s = sliced.mcpc_last_errors
    for name in r.names:
        assert np.array_equal(_bits(r.sum[name]), _bits(s.sum[name])) and np.array_equal(_bits(r.sumsq[name]), _bits(s.sumsq[name])), name
    # mcpc_cov_accumulate (include/mcpc.h): chunkings agree per entry within (R + G + 2) * 2^-52 * sum |v_i v_j|, R = n rows, G = 0
    v = np.concatenate([derived[name].cpu().numpy().astype(np.float64) for name in r.names], axis=-1)          # [n, B, D]
    scale = np.einsum("nbi,nbj->bij", np.abs(v), np.abs(v))
    bound = (len(STEPS) + 2) * 2.0 ** -52 * scale
    a, b = r.covariance.outer.cpu().numpy(), s.covariance.outer.cpu().numpy()
    assert a.shape == (B, v.shape[-1], v.shape[-1]) and (np.abs(a - b) <= bound).all()
    assert np.array_equal(_bits(r.covariance.sum), _bits(s.covariance.sum))


@pytest.mark.parametrize("quantity", ["error", "prediction"])
def test_covariance_is_a_covariance_over_the_same_blocks(runs, quantity):
    from montecarlopredictivecoding_amd.covariance import Covariance
    r = runs[quantity]["result"]
    c = r.covariance
    assert isinstance(c, Covariance) and c.n == 11 and c.B == B and not c.pooled
    assert [nm for nm, _, _ in c.columns] == r.names and c.outer.shape == (B, 80, 80)
    # the diagonal against sumsq, and the first-order sums: the bound the header states for mcpc_cov_accumulate
    q = torch.cat([r.sumsq[name] for name in r.names], dim=1).cpu().numpy()
    diag = torch.diagonal(c.outer, dim1=-2, dim2=-1).cpu().numpy()
    assert (np.abs(diag - q) <= (11 + 2) * 2.0 ** -52 * q).all()
    assert np.array_equal(_bits(c.sum), _bits(torch.cat([r.sum[name] for name in r.names], dim=1)))
    first, last = r.names[0], r.names[-1]
    assert c.block(first, last).shape == (B, SIZES[0], N_OUT) and c.corr().shape == (B, 80, 80)
    var = torch.diagonal(c.block(first, first), dim1=-2, dim2=-1)
    torch.testing.assert_close(var, r.var(first), rtol=1e-9, atol=1e-12)


def test_a_pooled_covariance_and_a_request_for_one_layer():
    um, model, data, inputs = _net()
    tr, _ = _call(um, model, data, inputs, dict(begin=BEGIN, stride=STRIDE, layers=(2,), covariance="chains", variance=False))
    r = tr.mcpc_last_errors
    assert r.names == ["e2"] and r.sumsq["e2"] is None and r.covariance.pooled and r.covariance.outer.shape == (17, 17)
    assert r.covariance.N == 11 * B
    full, _ = _call(um, model, data, inputs, dict(begin=BEGIN, stride=STRIDE, layers=(0, 1, 2)))
    assert full.mcpc_last_errors.covariance is None
    assert np.array_equal(_bits(r.sum["e2"]), _bits(full.mcpc_last_errors.sum["e2"])), "layer 2 alone (layers 1 and 2 through the ring)"


def test_the_request_leaves_moments_and_chain_energies_bit_identical():
    um, model, data, inputs = _net()
    mom = dict(begin=4, stride=2, layers=(0, 2), outputs="sigmoid")
    ce = dict(begin=2, stride=3)
    spec = dict(begin=BEGIN, stride=STRIDE, layers=(1,), outputs="error")
    both, res = _call(um, model, data, inputs, spec, moments=mom, chain_energies=ce)
    without, res0 = _call(um, model, data, inputs, None, moments=mom, chain_energies=ce)
    alone, _ = _call(um, model, data, inputs, spec)
    assert both.last_call_mode == "fused" and without.mcpc_last_errors is None
    a, b = both.mcpc_last_chain_energies, without.mcpc_last_chain_energies
    for p, q in ((a.loss, b.loss), (a.energy, b.energy), (a.overall, b.overall)):
        assert np.array_equal(_bits(p), _bits(q))
    m, n = both.mcpc_last_moments, without.mcpc_last_moments
    for p, q in ((m.out_sum, n.out_sum), (m.out_sumsq, n.out_sumsq), (m.x_sum[0], n.x_sum[0]), (m.x_sumsq[2], n.x_sumsq[2])):
        assert np.array_equal(_bits(p), _bits(q))
    for k in ("loss", "energy", "overall"):
        assert res[k] == res0[k]
    for p, q in zip(both.get_model_xs(), without.get_model_xs()):
        assert torch.equal(p, q)
    e, f = both.mcpc_last_errors, alone.mcpc_last_errors
    assert e.names == f.names == ["e1", "eout"]
    for name in e.names:
        assert np.array_equal(_bits(e.sum[name]), _bits(f.sum[name])) and np.array_equal(_bits(e.sumsq[name]), _bits(f.sumsq[name]))


def test_state_errors_are_the_record_path_on_the_same_state():
    um, model, data, inputs = _net()
    tr, _ = _call(um, model, data, inputs, None)
    kw = dict(inputs=inputs, loss_fn=um.bernoulli_fn, loss_fn_kwargs={"_target": data, "_var": None})
    xs = [x.detach().clone() for x in tr.get_model_xs()]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        st = tr.mcpc_state_errors(quantity="both", outputs="both", **kw)
        one = tr.mcpc_state_errors(layers=(1,), quantity="prediction", **kw)
    for a, b in zip(xs, tr.get_model_xs()):
        assert torch.equal(a, b.detach())                    # evaluating moves nothing
    eng = _engine(model, data)
    want = eng.prediction_errors(None, [x.contiguous() for x in xs], quantity="both", outputs="both", loss_kind=mo.LOSS_BERNOULLI)
    eng.sync_check()
    eng.close()
    assert sorted(st) == sorted(want) and len(st) == 8 and list(one) == ["mu1"]
    for k, v in st.items():
        assert v.shape == want[k].shape[1:] and v.dtype == torch.float32
        assert np.array_equal(v.cpu().numpy().view(np.int32), want[k][0].cpu().numpy().view(np.int32)), k
    assert torch.equal(one["mu1"], st["mu1"])
    assert torch.equal(st["e1"], xs[1] - st["mu1"])


def test_calls_that_are_not_fused_are_rejected():
    import montecarlopredictivecoding_amd.predictive_coding as pc
    um, model, data, inputs = _net()
    spec = dict(layers=(0,))
    with pytest.raises(NotImplementedError, match="mcpc_errors.*step by step.*callback_after_backward is set"):
        _call(um, model, data, inputs, spec, callback_after_backward=lambda **kw: None)
    assert all(m.get_x() is None for m in model if hasattr(m, "get_x"))      # before any work
    masked = torch.nn.Sequential(torch.nn.Linear(3, 3), pc.PCLayer(M=torch.ones(3, device=DEV)), torch.nn.Linear(3, 2)).to(DEV)
    masked.train()
    tr = pc.PCTrainer(masked, T=3, update_p_at="never", plot_progress_at=[])
    tr.mcpc_errors = spec
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(NotImplementedError, match="mcpc_errors.*generic torch loop.*S/M masks"):
            tr.train_on_batch(inputs=torch.zeros(2, 3, device=DEV), is_log_progress=False, is_return_results_every_t=False)
    with pytest.raises(ValueError, match="begin"):
        _call(um, model, data, inputs, dict(layers=(0,), begin=T))
    with pytest.raises(ValueError, match="unknown keys"):
        _call(um, model, data, inputs, dict(layers=(0,), pool="chains"))
    # the byte bound with the samples a slice holds: refused before anything runs
    import montecarlopredictivecoding_amd.predictive_coding.pc_trainer as pt
    tr = pc.PCTrainer(model, T=T, optimizer_x_fn=torch.optim.SGD, optimizer_x_kwargs={"lr": 0.05}, update_p_at="never", plot_progress_at=[])
    tr.mcpc_errors = dict(layers=(1,))
    tr.mcpc_errors_max_bytes = 4 * B * 33 * 2 + 16 * B * 33                 # derived buffers of two samples; the call's slice holds 40
    base = pt._PHILOX_STEPS[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match="derived records of 40 samples.*mcpc_errors_max_bytes"):
            tr.train_on_batch(inputs=inputs, loss_fn=um.bernoulli_fn, loss_fn_kwargs={"_target": data, "_var": None},
                              callback_after_t=um.random_step, callback_after_t_kwargs={"_pc_trainer": tr}, is_log_progress=False,
                              is_return_results_every_t=False)
    pt._PHILOX_STEPS[0] = base


def test_posterior_mean_of_the_error_units_of_the_linear_gaussian_toy():
    """Prior x ~ N(0.2, 1), y = 2 x + N(0, 1), y = 1: the posterior is N(0.44, 0.2), so E[eps_0] = 0.44 - 0.2 = 0.24 and the read-out
    error (2 x - 1) / var has mean -0.12 (a linear drift: the Euler discretisation does not bias the mean).  The tolerance is five
    Monte Carlo standard errors of the same call, from mcpc_autocovariance's .mcse of x_0 (eps_0 = x_0 - 0.2 has the same error; the
    read-out error twice that)."""
    import torch.nn as nn
    import montecarlopredictivecoding_amd.predictive_coding as pc
    import montecarlopredictivecoding_amd.utils.model as um
    chains, steps, mixing = 16, 2000, 200
    model = nn.Sequential(nn.Linear(1, 1), pc.PCLayer(sample_x_fn=um.sample_x_fn_cte), nn.Linear(1, 1, bias=False))
    model.train()
    nn.init.constant_(model[0].bias, 0.2)
    nn.init.constant_(model[2].weight, 2.0)
    model.to(DEV)
    tr = pc.PCTrainer(model, T=steps, optimizer_x_fn=torch.optim.SGD, optimizer_x_kwargs={"lr": 0.05}, update_p_at="never", plot_progress_at=[])
    tr.mcpc_seed = 11
    tr.mcpc_errors = dict(begin=mixing, layers=(0,), outputs="error")
    tr.mcpc_autocovariance = dict(begin=mixing, layers=(0,), max_lag=64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tr.train_on_batch(inputs=torch.zeros(chains, 1, device=DEV), loss_fn=um.fe_fn, loss_fn_kwargs={"_target": torch.ones(chains, 1, device=DEV), "_var": 1.0},
                          callback_after_t=um.random_step, callback_after_t_kwargs={"_pc_trainer": tr}, is_log_progress=False,
                          is_return_results_every_t=False)
    assert tr.last_call_mode == "fused"
    e, ac = tr.mcpc_last_errors, tr.mcpc_last_autocovariance
    assert e.n == ac.n == steps - mixing
    mcse = ac.mcse("x0")
    assert not ac.truncated("x0").any() and torch.isfinite(mcse).all() and (mcse > 0).all() and (mcse < 0.1).all()
    d0, do = (e.mean("e0") - 0.24).abs(), (e.mean("eout") + 0.12).abs()
    print(f"linear-Gaussian toy: |mean eps_0 - 0.24| / mcse max {float((d0 / mcse).max()):.2f}, "
          f"|mean eps_out + 0.12| / (2 mcse) max {float((do / (2 * mcse)).max()):.2f}, mcse {float(mcse.mean()):.4f}")
    assert (d0 <= 5 * mcse).all()
    assert (do <= 5 * 2 * mcse).all()
    # and eps_0 is x_0 shifted by the constant prediction: the same spread
    torch.testing.assert_close(e.var("e0"), ac.acov("x0")[..., 0] * e.n / (e.n - 1), rtol=1e-5, atol=1e-8)

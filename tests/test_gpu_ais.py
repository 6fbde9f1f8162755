"""Annealed importance sampling of the log marginal likelihood through PCTrainer.mcpc_ais (montecarlopredictivecoding_amd/ais.py)
against the NumPy restatement of tests/ais_cases.py, what the call promises bitwise (chunking, repetition, merging), what it must leave
untouched -- also when it raises -- and the known-answer case against its exact value."""
import functools
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import ais_cases as A
from tests import parity_log

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ACTS = {"tanh": nn.Tanh, "relu": nn.ReLU, "identity": None}


def _mods():
    from montecarlopredictivecoding_amd import predictive_coding as pc
    from montecarlopredictivecoding_amd.utils import model as um
    return pc, um


def build(W, b, act, lr=0.03, T=20):
    """(model on the device with these weights, an SGD trainer of it)."""
    pc, _ = _mods()
    mods = []
    for j, w in enumerate(W):
        lin = nn.Linear(w.shape[1], w.shape[0], bias=b[j] is not None)
        with torch.no_grad():
            lin.weight.copy_(torch.tensor(w))
            if b[j] is not None:
                lin.bias.copy_(torch.tensor(b[j]))
        mods.append(lin)
        if j < len(W) - 1:
            mods.append(pc.PCLayer())
            if ACTS[act] is not None:
                mods.append(ACTS[act]())
    model = nn.Sequential(*mods).to(DEV)
    model.train()
    trainer = pc.PCTrainer(model, T=T, optimizer_x_fn=torch.optim.SGD, optimizer_x_kwargs={"lr": lr}, update_p_at="never", plot_progress_at=[])
    return model, trainer


def case_trainer(name):
    c = A.ESTIMATOR_CASES[name]
    W, b, data = A.estimator_params(name)
    model, trainer = build(W, b, c["act"], lr=A.ESTIMATOR_RUN["lr"])
    _, um = _mods()
    if c["loss"] == "gaussian":
        loss_fn, kw = um.fe_fn, {"_var": c["var"]}
    else:
        loss_fn, kw = um.bernoulli_fn_mask, {"perc": c["perc"]}
    return model, trainer, loss_fn, kw, torch.tensor(data).to(DEV)


def run_kw(**over):
    r = dict(A.ESTIMATOR_RUN)
    r.pop("lr")                                       # the trainer's own
    r.update(over)
    return r


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int64).numpy()


@functools.lru_cache(maxsize=None)
def device_result(name):
    """(LogLikelihood, logw) of a case in one chunk; never modified."""
    from montecarlopredictivecoding_amd import ais
    _, trainer, loss_fn, kw, data = case_trainer(name)
    return ais.run(trainer, data, loss_fn, kw, return_logw=True, **run_kw())


# ---- against the restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(A.ESTIMATOR_CASES))
def test_log_weights_follow_the_restatement(name):
    ll, logw = device_result(name)
    want_logw, want_state = A.estimator_reference(name, "float32")
    tol = A.estimator_tolerance(name)
    got = logw.cpu().numpy()
    print(f"{name}: max |logw - restatement| = {np.abs(got - want_logw).max():.3g} (tolerance {tol:.3g}), "
          f"max |log_p - restatement| = {np.abs(ll.log_p.cpu().numpy() - A.log_p(want_state)).max():.3g}")
    np.testing.assert_array_equal(ll.n_samples.cpu().numpy(), want_state[:, 3])
    parity_log.close("ais_estimator", f"{name} logw", got, want_logw, atol=tol)
    parity_log.close("ais_estimator", f"{name} log_p", ll.log_p.cpu().numpy(), A.log_p(want_state), atol=tol)
    assert ll.state.device.type == "cuda" and ll.state.dtype == torch.float64 and tuple(ll.state.shape) == (A.N_DATA, 4)
    assert len(ll) == A.N_DATA and np.isfinite(ll.mean()) and (ll.ess >= 1).all() and (ll.ess <= A.ESTIMATOR_RUN["replicas"]).all()


# ---- bitwise --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(A.ESTIMATOR_CASES))
def test_the_result_does_not_depend_on_the_chunking_or_the_run(name):
    one, _ = device_result(name)
    _, trainer, loss_fn, kw, data = case_trainer(name)
    for max_chains in (80, 32, 16):
        got = trainer.mcpc_ais(data, loss_fn, kw, max_chains=max_chains, **run_kw())
        assert np.array_equal(bits(got.state), bits(one.state)), f"max_chains={max_chains} moves the state"


@pytest.mark.parametrize("name", sorted(A.ESTIMATOR_CASES))
def test_two_calls_with_disjoint_chains_merge_to_the_call_over_their_union(name):
    _, trainer, loss_fn, kw, data = case_trainer(name)
    one = data[:1]
    whole = trainer.mcpc_ais(one, loss_fn, kw, **run_kw(replicas=80))
    lo = trainer.mcpc_ais(one, loss_fn, kw, **run_kw(replicas=40, chain_base=0))
    hi = trainer.mcpc_ais(one, loss_fn, kw, **run_kw(replicas=40, chain_base=40))
    both = lo.merge(hi)
    assert float(both.n_samples[0]) == 80.0 == float(whole.n_samples[0])
    # the merge rule rescales two sums by one exp each: a few ulp of log s1 (include/mcpc.h: (n_samp + 64) 2^-52 for the summation)
    tol = (80 + 64) * 2.0 ** -52
    assert abs(float(both.log_p[0] - whole.log_p[0])) <= tol * max(1.0, abs(float(whole.log_p[0])))
    assert abs(float(both.ess[0] - whole.ess[0])) <= 1e-12 * float(whole.ess[0])
    assert float(lo.log_p[0]) != float(hi.log_p[0])


# ---- what the call leaves untouched ------------------------------------------------------------------------------------------------------
def _train(trainer, um, target):
    from montecarlopredictivecoding_amd.predictive_coding import pc_trainer as pt
    trainer.mcpc_seed = 77
    pt._PHILOX_STEPS[0] = 900
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = trainer.train_on_batch(inputs=torch.zeros(target.shape[0], A.ESTIMATOR_CASES["bern_relu"]["n_in"], device=DEV),
                                     loss_fn=um.bernoulli_fn, loss_fn_kwargs={"_target": target, "_var": None},
                                     callback_after_t=um.random_step, callback_after_t_kwargs={"_pc_trainer": trainer},
                                     is_log_progress=False, is_return_results_every_t=True)
    assert trainer.last_call_mode == "fused"
    xs = [x.detach().clone() for x in trainer.get_model_xs()]
    return xs, np.asarray(res["overall"], dtype=np.float64)


def _snapshot(model, trainer):
    from montecarlopredictivecoding_amd.predictive_coding import pc_trainer as pt
    return dict(params=[p.detach().clone() for p in model.parameters()], versions=[p._version for p in model.parameters()],
                grads=[None if p.grad is None else p.grad.detach().clone() for p in model.parameters()],
                xs=[x.detach().clone() for x in trainer.get_model_xs()], steps=pt._PHILOX_STEPS[0],
                engine_steps=[e.step_counter for e in pt._ENGINES.values()], opt_x=trainer.get_optimizer_x(), opt_p=trainer.get_optimizer_p())


def _assert_untouched(model, trainer, before):
    now = _snapshot(model, trainer)
    for a, b in zip(now["params"], before["params"]):
        assert torch.equal(a, b)
    assert now["versions"] == before["versions"]
    for a, b in zip(now["grads"], before["grads"]):
        assert (a is None) == (b is None) and (a is None or np.array_equal(a.cpu().numpy().view(np.int32), b.cpu().numpy().view(np.int32)))
    assert len(now["xs"]) == len(before["xs"])
    for a, b in zip(now["xs"], before["xs"]):
        assert np.array_equal(a.cpu().numpy().view(np.int32), b.cpu().numpy().view(np.int32))
    assert now["steps"] == before["steps"]
    assert now["engine_steps"][:len(before["engine_steps"])] == before["engine_steps"]
    assert now["opt_x"] is before["opt_x"] and now["opt_p"] is before["opt_p"]


@pytest.mark.parametrize("fails", [False, True])
def test_a_call_leaves_the_trainer_and_a_later_fused_call_as_they_were(fails, monkeypatch):
    _, um = _mods()
    target = torch.tensor(np.repeat(A.estimator_params("bern_relu")[2], 16, axis=0)).to(DEV)      # 80 chains: the engine the AIS call uses
    # the yardstick: a fresh trainer that never ran AIS
    _, fresh, _, _, _ = case_trainer("bern_relu")
    _train(fresh, um, target)                          # (leaves x and, below, grads: a state worth keeping)
    want_xs, want_overall = _train(fresh, um, target)

    model, trainer, loss_fn, kw, data = case_trainer("bern_relu")
    _train(trainer, um, target)
    for p in model.parameters():
        p.grad = torch.full_like(p, 0.25)
    before = _snapshot(model, trainer)
    if fails:
        from montecarlopredictivecoding_amd import engine as E
        real, calls = E.ais_increment, []

        def third_rung_fails(*a, **k):
            calls.append(1)
            if len(calls) == 3:
                raise RuntimeError("the third rung fails")
            return real(*a, **k)
        monkeypatch.setattr(E, "ais_increment", third_rung_fails)
        with pytest.raises(RuntimeError, match="third rung"):
            trainer.mcpc_ais(data, loss_fn, kw, **run_kw())
        monkeypatch.undo()
    else:
        trainer.mcpc_ais(data, loss_fn, kw, **run_kw())
    _assert_untouched(model, trainer, before)
    for p in model.parameters():
        p.grad = None
    got_xs, got_overall = _train(trainer, um, target)
    assert np.array_equal(got_overall.view(np.int64), want_overall.view(np.int64))
    for a, b in zip(got_xs, want_xs):
        assert np.array_equal(a.cpu().numpy().view(np.int32), b.cpu().numpy().view(np.int32))


def test_refusals_and_an_lr_of_ones_own():
    _, um = _mods()
    pc, _ = _mods()
    W, b, data = A.estimator_params("gauss_tanh")
    model, _ = build(W, b, "tanh")
    adam = pc.PCTrainer(model, T=4, optimizer_x_fn=torch.optim.Adam, optimizer_x_kwargs={"lr": 0.03}, update_p_at="never", plot_progress_at=[])
    d = torch.tensor(data).to(DEV)
    with pytest.raises(ValueError, match="lr"):
        adam.mcpc_ais(d, um.fe_fn, {"_var": 0.7}, **run_kw())
    got = adam.mcpc_ais(d, um.fe_fn, {"_var": 0.7}, lr=A.ESTIMATOR_RUN["lr"], **run_kw())
    assert np.array_equal(bits(got.state), bits(device_result("gauss_tanh")[0].state))
    with pytest.raises(ValueError):
        adam.mcpc_ais(d, um.fe_fn, {"_var": 0.7}, lr=0.03, betas=[0.0, 0.5, 0.4, 1.0])
    # data on the host are taken too, and land on the model's device
    host = adam.mcpc_ais(data, um.fe_fn, {"_var": 0.7}, lr=A.ESTIMATOR_RUN["lr"], **run_kw())
    assert np.array_equal(bits(host.state), bits(got.state))


# ---- the known-answer case ---------------------------------------------------------------------------------------------------------------
def test_kat_annealing_beats_prior_sampling_and_meets_the_exact_value():
    _, um = _mods()
    W, b, data = A.kat_params()
    _, trainer = build(W, b, "identity", lr=A.KAT["lr"])
    d = torch.tensor(data).to(DEV)
    kw = dict(replicas=A.KAT["replicas"], steps_per_stage=A.KAT["steps_per_stage"], noise_var=A.KAT["noise_var"], seed=0)
    ll = trainer.mcpc_ais(d, um.bernoulli_fn, {}, stages=A.KAT["stages"], power=A.KAT["power"], **kw)
    prior = trainer.mcpc_ais(d, um.bernoulli_fn, {}, betas=[0.0, 1.0], **kw)
    exact = A.kat_exact()
    err = ll.log_p.cpu().numpy() - exact
    print("KAT device: err", np.round(err, 4), "ESS ais", np.round(ll.ess.cpu().numpy(), 1), "ESS prior", np.round(prior.ess.cpu().numpy(), 1),
          "tol", A.KAT_TOL, "restatement", np.round(A.log_p(A.kat_run(0)[1]) - exact, 4))
    assert (ll.n_samples == A.KAT["replicas"]).all() and (prior.n_samples == A.KAT["replicas"]).all(), "a replica is not finite"
    assert (ll.ess > prior.ess).all()
    parity_log.close("ais_kat", "log_p against the quadrature", ll.log_p.cpu().numpy(), exact, atol=A.KAT_TOL)


# ---- the evaluator -------------------------------------------------------------------------------------------------------------------------
def test_get_marginal_likelihood_ais_walks_the_loader_in_order():
    from montecarlopredictivecoding_amd.likelihood import LogLikelihood
    from montecarlopredictivecoding_amd.utils.training_evaluation import get_marginal_likelihood_ais
    _, um = _mods()
    c = A.ESTIMATOR_CASES["gauss_tanh"]
    W, b, data = A.estimator_params("gauss_tanh")
    model, _ = build(W, b, c["act"])
    config = dict(loss_fn=um.fe_fn, input_var=c["var"], input_size=c["n_in"], mixing=3, sampling=2,
                  optimizer_x_kwargs_mcpc={"lr": A.ESTIMATOR_RUN["lr"]})
    d = torch.tensor(data)
    loader = [(d[:3], None), (d[3:], None)]
    r = run_kw()
    got = get_marginal_likelihood_ais(model, config, loader, True, replicas=r["replicas"], stages=r["stages"],
                                      steps_per_stage=r["steps_per_stage"], seed=r["seed"], step_base=r["step_base"], noise_var=r["noise_var"])
    assert isinstance(got, LogLikelihood) and len(got) == A.N_DATA
    assert np.array_equal(bits(got.state), bits(device_result("gauss_tanh")[0].state)), "the loader's batches are not the call's chunks"
    swapped = get_marginal_likelihood_ais(model, config, [(d[3:], None), (d[:3], None)], True, replicas=r["replicas"], stages=r["stages"],
                                          steps_per_stage=r["steps_per_stage"], seed=r["seed"], step_base=r["step_base"], noise_var=r["noise_var"])
    assert not np.array_equal(bits(swapped.state[:2]), bits(got.state[:2]))
    with pytest.raises(NotImplementedError):
        get_marginal_likelihood_ais(model, dict(config, loss_fn=um.zero_fn), loader, True)

"""The facade of mcpc_state_gradients: PCTrainer.mcpc_state_gradients after a MAP call, and PCTrainer.mcpc_ais(adjust="mala",
gradients="evaluator") -- the adjusted transitions with ONE Engine.state_gradients call per proposal -- against the restatement of
tests/mala_cases.py, against gradients="run" bit for bit on the layer-wise kernels, and every bitwise and untouched-state promise."""
import warnings

import numpy as np
import pytest
import torch

from oracle import mcpc_oracle as mo
from tests import ais_cases as A
from tests import mala_cases as M
from tests import parity_log
from tests import state_grad_cases as sg
from tests.test_gpu_ais import DEV, _assert_untouched, _mods, _snapshot, _train, bits, build, case_trainer

pytestmark = pytest.mark.gpu
NAMES = sorted(A.ESTIMATOR_CASES)
_RESULTS = {}


@pytest.fixture(autouse=True)
def philox_steps_as_found():
    """The fused calls of `_train` take their noise from a process-wide step counter: leave it as it was found."""
    from montecarlopredictivecoding_amd.predictive_coding import pc_trainer as pt
    before = pt._PHILOX_STEPS[0]
    yield
    pt._PHILOX_STEPS[0] = before


def run_kw(**over):
    r = dict(M.ESTIMATOR_RUN, adjust="mala", gradients="evaluator")
    r.update(over)
    return r


def device_result(name):
    """(LogLikelihood, logw, accepted [K - 1, B], the trainer's acceptance) of a case in one chunk; computed once, never modified."""
    if name not in _RESULTS:
        from montecarlopredictivecoding_amd import ais
        _, trainer, loss_fn, kw, data = case_trainer(name)
        ll, logw, acc = ais.run(trainer, data, loss_fn, kw, return_logw=True, return_accepted=True, **run_kw())
        _RESULTS[name] = (ll, logw, acc, trainer.mcpc_last_ais_acceptance)
    return _RESULTS[name]


# ---- 11. mcpc_state_gradients -----------------------------------------------------------------------------------------------------------
def _map_call(trainer, um, inputs, target):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = trainer.train_on_batch(inputs=inputs, loss_fn=um.bernoulli_fn, loss_fn_kwargs={"_target": target, "_var": None},
                                     is_log_progress=False, is_return_results_every_t=True)
    assert trainer.last_call_mode == "fused"
    return [x.detach().clone() for x in trainer.get_model_xs()], np.asarray(res["overall"], dtype=np.float64)


@pytest.mark.parametrize("device", [DEV, "cpu"])
def test_state_gradients_of_the_trainer(device):
    from montecarlopredictivecoding_amd.chain_energies import ChainEnergies
    from montecarlopredictivecoding_amd.engine import Engine
    _, um = _mods()
    name = "bern_relu"
    c = A.ESTIMATOR_CASES[name]
    W, b, data = A.estimator_params(name)
    B = 48
    target = torch.tensor(np.repeat(data, 10, axis=0)[:B]).to(device)
    inputs = torch.tensor(np.random.RandomState(3).randn(B, c["n_in"]).astype(np.float32)).to(device)
    model, trainer = build(W, b, c["act"], T=6)
    model.to(device)
    kw = dict(inputs=inputs, loss_fn=um.bernoulli_fn, loss_fn_kwargs={"_target": target, "_var": None})
    xs, _ = _map_call(trainer, um, inputs, target)
    for p in model.parameters():
        p.grad = torch.full_like(p, 0.25)
    before = _snapshot(model, trainer)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        grads = trainer.mcpc_state_gradients(**kw)
        both, ce = trainer.mcpc_state_gradients(energies=True, **kw)
        st = trainer.mcpc_state_energies(**kw)
    _assert_untouched(model, trainer, before)
    assert len(grads) == 2 and isinstance(ce, ChainEnergies)
    for g, g2, x in zip(grads, both, xs):
        assert g.shape == x.shape and g.dtype == torch.float32 and g.device.type == torch.device(device).type
        assert np.array_equal(g.cpu().numpy().view(np.int32), g2.cpu().numpy().view(np.int32))
    assert np.array_equal(bits(ce.overall), bits(st.overall)) and np.array_equal(bits(ce.loss), bits(st.loss))
    # the engine's own call on the same x, bitwise
    eng = Engine(list(c["sizes"]), [mo.ACT_RELU] * 2, c["n_in"], c["n_out"], B, device=torch.device(DEV))
    eng.bind_params([torch.tensor(w).to(DEV) for w in W], [torch.tensor(v).to(DEV) for v in b])
    eng.bind_target(target.to(DEV))
    want, _ = eng.state_gradients(inputs.to(DEV), [x.to(DEV).contiguous() for x in xs], loss_kind=mo.LOSS_BERNOULLI)
    eng.sync_check()
    for g, w in zip(grads, want):
        assert np.array_equal(g.cpu().numpy().view(np.int32), w[0].cpu().numpy().view(np.int32))
    eng.close()
    # the fp64 oracle, one chain at a time
    case = dict(sizes=c["sizes"], n_in=c["n_in"], n_out=c["n_out"], act=mo.ACT_RELU, loss=mo.LOSS_BERNOULLI, var=1.0, mask_start=0)
    d = dict(W=W, b=b, inputs=inputs.cpu().numpy(), target=target.cpu().numpy())
    ref, bound = sg.oracle_rows(case, [x.cpu().numpy()[None] for x in xs], d=d)
    sg.log_against_bound(parity_log, f"mcpc_state_gradients after MAP vs oracle per chain ({device})", [g.cpu().numpy()[None] for g in grads],
                         ref, bound)
    # the next fused call is what it is on a trainer that never evaluated
    for p in model.parameters():
        p.grad = None
    model2, fresh = build(W, b, c["act"], T=6)
    model2.to(device)
    _map_call(fresh, um, inputs, target)
    want_xs, want_overall = _map_call(fresh, um, inputs, target)
    got_xs, got_overall = _map_call(trainer, um, inputs, target)
    assert np.array_equal(got_overall.view(np.int64), want_overall.view(np.int64))
    for a, w in zip(got_xs, want_xs):
        assert np.array_equal(a.cpu().numpy().view(np.int32), w.cpu().numpy().view(np.int32))


def test_state_gradients_refuses_what_the_engine_does_not_express():
    _, um = _mods()
    W, b, data = A.estimator_params("bern_relu")
    model, trainer = build(W, b, "relu", T=4)
    target = torch.tensor(np.repeat(data, 4, axis=0)).to(DEV)
    inputs = torch.zeros(target.shape[0], 5, device=DEV)
    _map_call(trainer, um, inputs, target)
    with pytest.raises(NotImplementedError):
        trainer.mcpc_state_gradients(inputs, loss_fn=lambda out, _target: ((out - _target) ** 4).sum(), loss_fn_kwargs={"_target": target})


# ---- 12. against the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_log_weights_and_decisions_follow_the_restatement(name):
    """The criteria of tests/test_gpu_mala_ais.py: a chain whose accepted proposals per rung are the fp32 restatement's is held to
    10 x max |logw32 - logw64|; one that decided differently somewhere is left out, at most MAX_FLIPPED of 80 (the fp32 restatement
    itself stays within that cap by construction: FP32_VS_FP64_FLIPS is 0)."""
    assert M.FP32_VS_FP64_FLIPS[name] == 0
    ll, logw, acc, share = device_result(name)
    want_logw, want_state, want_acc, margin = M.estimator_reference(name, "float32")
    steps, B = M.ESTIMATOR_RUN["steps_per_stage"], want_logw.shape[0]
    got_acc = acc.cpu().numpy()
    assert got_acc.shape == want_acc.shape == (M.ESTIMATOR_RUN["stages"] - 1, B) and acc.dtype == torch.int32
    flipped = (got_acc != want_acc).any(0)
    tol = M.estimator_tolerance(name)
    got = logw.cpu().numpy()
    print(f"{name}: {int(flipped.sum())} of {B} chains decide differently (the restatement's smallest margin: {margin:.3g}), "
          f"max |logw - restatement| over the others = {np.abs(got - want_logw)[~flipped].max():.3g} (tolerance {tol:.3g}), "
          f"accepted {got_acc.mean() / steps:.3f} against {want_acc.mean() / steps:.3f}")
    assert int(flipped.sum()) <= M.MAX_FLIPPED
    parity_log.close("mala_estimator (gradients=evaluator)", f"{name} logw", got[~flipped], want_logw[~flipped], atol=tol)
    np.testing.assert_array_equal(ll.n_samples.cpu().numpy(), want_state[:, 3])
    if not flipped.any():
        parity_log.close("mala_estimator (gradients=evaluator)", f"{name} log_p", ll.log_p.cpu().numpy(), A.log_p(want_state), atol=tol)
    np.testing.assert_allclose(share.cpu().numpy(), got_acc.sum(1) / (B * steps), rtol=0, atol=1e-15)
    np.testing.assert_array_equal(got_acc[:, ~flipped].sum(1), want_acc[:, ~flipped].sum(1))
    assert (got_acc < steps).any() and (got_acc > 0).any(), "one of the two branches is never taken"


# ---- 13. on the layer-wise kernels the two are one call -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("extra", [dict(), dict(leapfrog=2, steps_per_stage=1), dict(resample="systematic")],
                         ids=["mala", "leapfrog2", "systematic"])
def test_evaluator_and_run_agree_bitwise_on_the_layerwise_kernels(name, extra, monkeypatch):
    from montecarlopredictivecoding_amd import ais
    monkeypatch.setenv("MCPC_TUNING", "ws=4")                           # (the engine cache keys on it)
    _, trainer, loss_fn, kw, data = case_trainer(name)
    res = {}
    for how in ("run", "evaluator"):
        out = ais.run(trainer, data, loss_fn, kw, return_logw=True, return_accepted=True, return_ancestors=True, **run_kw(gradients=how, **extra))
        trace = trainer.mcpc_last_ais_resampling
        res[how] = out + (trainer.mcpc_last_ais_acceptance,) + ((trace.ess, trace.share) if trace is not None else ())
    ll_r, ll_e = res["run"][0], res["evaluator"][0]
    assert np.array_equal(bits(ll_r.state), bits(ll_e.state)), "the state"
    for i, (a, e) in enumerate(zip(res["run"][1:], res["evaluator"][1:])):
        assert (a is None) == (e is None)
        if a is not None:
            assert torch.equal(a, e) and a.dtype == e.dtype, f"output {i + 1}"
            if a.dtype == torch.float64:
                assert np.array_equal(bits(a), bits(e)), f"output {i + 1}"
    assert (res["run"][3] is not None) == ("resample" in extra)


# ---- 14. chunking and defaults -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_result_does_not_depend_on_the_chunking_or_the_run(name):
    one, _, _, share = device_result(name)
    _, trainer, loss_fn, kw, data = case_trainer(name)
    for max_chains in (80, 32, 16):
        got = trainer.mcpc_ais(data, loss_fn, kw, max_chains=max_chains, **run_kw())
        assert np.array_equal(bits(got.state), bits(one.state)), f"max_chains={max_chains} moves the state"
        assert np.array_equal(bits(trainer.mcpc_last_ais_acceptance), bits(share)), f"max_chains={max_chains} moves the acceptance"


def test_gradients_run_is_the_call_without_the_keyword():
    _, trainer, loss_fn, kw, data = case_trainer("bern_relu")
    r = run_kw()
    r.pop("gradients")
    plain = trainer.mcpc_ais(data, loss_fn, kw, **r)
    share = trainer.mcpc_last_ais_acceptance
    named = trainer.mcpc_ais(data, loss_fn, kw, gradients="run", **r)
    assert np.array_equal(bits(named.state), bits(plain.state)) and np.array_equal(bits(trainer.mcpc_last_ais_acceptance), bits(share))
    unadjusted = dict(r, adjust=None)
    a = trainer.mcpc_ais(data, loss_fn, kw, **unadjusted)
    b = trainer.mcpc_ais(data, loss_fn, kw, gradients="run", **unadjusted)
    assert np.array_equal(bits(a.state), bits(b.state))
    with pytest.raises(ValueError, match="gradients"):
        trainer.mcpc_ais(data, loss_fn, kw, gradients="evaluator", **unadjusted)
    with pytest.raises(ValueError, match="gradients"):
        trainer.mcpc_ais(data, loss_fn, kw, gradients="engine", **r)


def test_the_evaluator_call_does_not_load_the_engines_state(monkeypatch):
    from montecarlopredictivecoding_amd.engine import Engine
    _, trainer, loss_fn, kw, data = case_trainer("gauss_tanh")
    calls = []
    real = Engine.load_state
    monkeypatch.setattr(Engine, "load_state", lambda self, xs: (calls.append(1), real(self, xs))[1])
    trainer.mcpc_ais(data, loss_fn, kw, **run_kw())
    assert not calls, "gradients='evaluator' loaded a state into the engine"
    trainer.mcpc_ais(data, loss_fn, kw, **run_kw(gradients="run"))
    assert calls


@pytest.mark.parametrize("fails", [False, True])
def test_a_call_leaves_the_trainer_and_a_later_fused_call_as_they_were(fails, monkeypatch):
    _, um = _mods()
    target = torch.tensor(np.repeat(A.estimator_params("bern_relu")[2], 16, axis=0)).to(DEV)      # 80 chains: the engine the AIS call uses
    _, fresh, _, _, _ = case_trainer("bern_relu")                        # the yardstick: a trainer that never ran AIS
    _train(fresh, um, target)
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
        assert trainer.mcpc_last_ais_acceptance is None                  # a call that raises leaves no acceptance behind
    else:
        trainer.mcpc_ais(data, loss_fn, kw, **run_kw())
    _assert_untouched(model, trainer, before)
    for p in model.parameters():
        p.grad = None
    # the engines hold the model's own read-out again: the next fused call is the fresh trainer's
    got_xs, got_overall = _train(trainer, um, target)
    assert np.array_equal(got_overall.view(np.int64), want_overall.view(np.int64))
    for a, b in zip(got_xs, want_xs):
        assert np.array_equal(a.cpu().numpy().view(np.int32), b.cpu().numpy().view(np.int32))


# ---- 15. the known-answer case --------------------------------------------------------------------------------------------------------------
def test_kat_meets_the_exact_value():
    """|log_p - exact| <= M.KAT_TOL[0.15], 2 x the largest error of the fp32 MALA restatement over seeds 0..7; seed 0 only."""
    lr = 0.15
    _, um = _mods()
    W, b, data = A.kat_params()
    _, trainer = build(W, b, "identity", lr=A.KAT["lr"])
    d = torch.tensor(data).to(DEV)
    kw = dict(replicas=A.KAT["replicas"], steps_per_stage=A.KAT["steps_per_stage"], noise_var=A.KAT["noise_var"], seed=0,
              stages=A.KAT["stages"], power=A.KAT["power"], lr=lr)
    ll = trainer.mcpc_ais(d, um.bernoulli_fn, {}, adjust="mala", gradients="evaluator", **kw)
    share = trainer.mcpc_last_ais_acceptance.cpu().numpy()
    exact = A.kat_exact()
    err = ll.log_p.cpu().numpy() - exact
    print(f"KAT device, MALA through the evaluator, lr {lr}: err", np.round(err, 4), "ESS", np.round(ll.ess.cpu().numpy(), 1),
          f"acceptance {share.min():.3f} .. {share.max():.3f}, tol {M.KAT_TOL[lr]:.4f}")
    assert (ll.n_samples == A.KAT["replicas"]).all(), "a replica is not finite"
    assert (share > 0.5).all() and (share <= 1.0).all()
    parity_log.close("mala_kat (gradients=evaluator)", f"log_p against the quadrature, lr {lr}", ll.log_p.cpu().numpy(), exact, atol=M.KAT_TOL[lr])

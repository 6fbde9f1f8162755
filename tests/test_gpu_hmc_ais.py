"""Annealed importance sampling with Hamiltonian transitions of L leapfrog steps, PCTrainer.mcpc_ais(adjust="mala", leapfrog=L)
(montecarlopredictivecoding_amd/ais.py), against the restatement of tests/hmc_cases.py: log-weights and accepted trajectories on
ais_cases' two estimator nets at lr = 0.1 and L = 3, every bitwise and untouched-state promise of the adjusted call, the known-answer
case, and the closed-form case on which one trajectory of five leapfrog steps meets a bound that five MALA steps miss."""
import numpy as np
import pytest
import torch

from tests import ais_cases as A
from tests import hmc_cases as H
from tests import parity_log
from tests import smc_cases as S
from tests.test_gpu_ais import DEV, _assert_untouched, _mods, _snapshot, _train, bits, build, case_trainer

pytestmark = pytest.mark.gpu
NAMES = sorted(A.ESTIMATOR_CASES)
_RESULTS = {}


@pytest.fixture(autouse=True)
def philox_steps_as_found():
    """The fused calls of `_train` take their noise from a process-wide step counter.  Tests that run later in the process and check
    a statistic of their own noise were written for the stream they meet without this file: leave the counter as it was found."""
    from montecarlopredictivecoding_amd.predictive_coding import pc_trainer as pt
    before = pt._PHILOX_STEPS[0]
    yield
    pt._PHILOX_STEPS[0] = before


def run_kw(**over):
    r = dict(H.ESTIMATOR_RUN, adjust="mala")                            # lr = 0.1 and leapfrog = 3 are passed
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


# ---- against the restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_log_weights_and_decisions_follow_the_restatement(name):
    """A chain whose accepted trajectories per rung are the fp32 restatement's is held to 10 x max |logw32 - logw64|; one that decided
    differently somewhere is left out, at most 4 of 80."""
    ll, logw, acc, share = device_result(name)
    want_logw, want_state, want_acc, margin = H.estimator_reference(name, "float32")
    steps, B = H.ESTIMATOR_RUN["steps_per_stage"], want_logw.shape[0]
    got_acc = acc.cpu().numpy()
    assert got_acc.shape == want_acc.shape == (H.ESTIMATOR_RUN["stages"] - 1, B) and acc.dtype == torch.int32
    flipped = (got_acc != want_acc).any(0)
    tol = H.estimator_tolerance(name)
    got = logw.cpu().numpy()
    print(f"{name}: {int(flipped.sum())} of {B} chains decide differently (the restatement's smallest margin: {margin:.3g}), "
          f"max |logw - restatement| over the others = {np.abs(got - want_logw)[~flipped].max():.3g} (tolerance {tol:.3g}), "
          f"accepted {got_acc.mean() / steps:.3f} against {want_acc.mean() / steps:.3f}")
    assert int(flipped.sum()) <= H.MAX_FLIPPED
    parity_log.close("hmc_estimator", f"{name} logw", got[~flipped], want_logw[~flipped], atol=tol)
    np.testing.assert_array_equal(ll.n_samples.cpu().numpy(), want_state[:, 3])
    if not flipped.any():
        parity_log.close("hmc_estimator", f"{name} log_p", ll.log_p.cpu().numpy(), A.log_p(want_state), atol=tol)
    # the acceptance: the trainer's attribute is the share of the device's counts, and over the chains kept it is the restatement's
    assert share.dtype == torch.float64 and tuple(share.shape) == (H.ESTIMATOR_RUN["stages"] - 1,)
    np.testing.assert_allclose(share.cpu().numpy(), got_acc.sum(1) / (B * steps), rtol=0, atol=1e-15)
    np.testing.assert_array_equal(got_acc[:, ~flipped].sum(1), want_acc[:, ~flipped].sum(1))
    if not flipped.any():
        np.testing.assert_allclose(share.cpu().numpy(), want_acc.sum(1) / (B * steps), rtol=0, atol=1e-15)
    assert (got_acc < steps).any() and (got_acc > 0).any(), "one of the two branches is never taken"


# ---- bitwise ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_result_does_not_depend_on_the_chunking_or_the_run(name):
    one, _, _, share = device_result(name)
    _, trainer, loss_fn, kw, data = case_trainer(name)
    for max_chains in (80, 80, 32, 16):
        got = trainer.mcpc_ais(data, loss_fn, kw, max_chains=max_chains, **run_kw())
        assert np.array_equal(bits(got.state), bits(one.state)), f"max_chains={max_chains} moves the state"
        assert np.array_equal(bits(trainer.mcpc_last_ais_acceptance), bits(share)), f"max_chains={max_chains} moves the acceptance"


@pytest.mark.parametrize("name", NAMES)
def test_two_calls_with_disjoint_chains_merge_to_the_call_over_their_union(name):
    _, trainer, loss_fn, kw, data = case_trainer(name)
    one = data[:1]
    whole = trainer.mcpc_ais(one, loss_fn, kw, **run_kw(replicas=80))
    lo = trainer.mcpc_ais(one, loss_fn, kw, **run_kw(replicas=40, chain_base=0))
    hi = trainer.mcpc_ais(one, loss_fn, kw, **run_kw(replicas=40, chain_base=40))
    both = lo.merge(hi)
    assert float(both.n_samples[0]) == 80.0 == float(whole.n_samples[0])
    tol = (80 + 64) * 2.0 ** -52                                         # tests/test_gpu_ais.py's merge tolerance
    assert abs(float(both.log_p[0] - whole.log_p[0])) <= tol * max(1.0, abs(float(whole.log_p[0])))
    assert abs(float(both.ess[0] - whole.ess[0])) <= 1e-12 * float(whole.ess[0])
    assert float(lo.log_p[0]) != float(hi.log_p[0])


def test_one_leapfrog_step_is_the_call_without_the_keyword_and_three_move_the_state():
    _, trainer, loss_fn, kw, data = case_trainer("bern_relu")
    r = run_kw()
    r.pop("leapfrog")
    plain = trainer.mcpc_ais(data, loss_fn, kw, **r)
    share = trainer.mcpc_last_ais_acceptance.clone()
    one = trainer.mcpc_ais(data, loss_fn, kw, leapfrog=1, **r)
    assert np.array_equal(bits(one.state), bits(plain.state)) and np.array_equal(bits(trainer.mcpc_last_ais_acceptance), bits(share))
    three = trainer.mcpc_ais(data, loss_fn, kw, leapfrog=3, **r)
    assert not np.array_equal(bits(three.state), bits(plain.state))
    assert np.array_equal(bits(three.state), bits(device_result("bern_relu")[0].state))
    # unadjusted, leapfrog=1 is still the call without it
    r.pop("adjust")
    assert np.array_equal(bits(trainer.mcpc_ais(data, loss_fn, kw, leapfrog=1, **r).state), bits(trainer.mcpc_ais(data, loss_fn, kw, **r).state))


def test_the_three_value_errors_fire_before_any_device_work(monkeypatch):
    from montecarlopredictivecoding_amd import engine as E
    _, trainer, loss_fn, kw, data = case_trainer("gauss_tanh")

    def never(*a, **k):
        raise AssertionError("device work before the refusal")
    for name in ("ais_increment", "hmc_begin", "mala_propose"):
        monkeypatch.setattr(E, name, never)
    monkeypatch.setattr(trainer, "_engine_for", never)
    for over in (dict(leapfrog=0), dict(leapfrog=2.0), dict(leapfrog=True), dict(leapfrog=2, adjust=None), dict(leapfrog=2, noise_var=1.0)):
        with pytest.raises(ValueError, match="leapfrog"):
            trainer.mcpc_ais(data, loss_fn, kw, **run_kw(**over))
    assert trainer.mcpc_last_ais_acceptance is None


@pytest.mark.parametrize("name", NAMES)
def test_a_vanishing_step_size_accepts_every_trajectory(name):
    _, trainer, loss_fn, kw, data = case_trainer(name)
    ll = trainer.mcpc_ais(data, loss_fn, kw, **run_kw(lr=1e-8))
    assert (trainer.mcpc_last_ais_acceptance == 1.0).all(), trainer.mcpc_last_ais_acceptance
    assert (ll.n_samples == H.ESTIMATOR_RUN["replicas"]).all()


# ---- what the call leaves untouched ------------------------------------------------------------------------------------------------------
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
    got_xs, got_overall = _train(trainer, um, target)
    assert np.array_equal(got_overall.view(np.int64), want_overall.view(np.int64))
    for a, b in zip(got_xs, want_xs):
        assert np.array_equal(a.cpu().numpy().view(np.int32), b.cpu().numpy().view(np.int32))


# ---- the known-answer case ---------------------------------------------------------------------------------------------------------------
def test_kat_meets_the_exact_value_with_two_trajectories_of_five_steps_per_rung():
    """|log_p - exact| <= 2 x the largest error of the fp32 leapfrog restatement over seeds 0..7 (tests/hmc_cases.py: 2 x 0.422875) at
    lr 0.15, where the unadjusted restatement errs by 0.874 .. 1.016 on every seed: a test of exactness, not of gain."""
    _, um = _mods()
    W, b, data = A.kat_params()
    _, trainer = build(W, b, "identity", lr=A.KAT["lr"])
    d = torch.tensor(data).to(DEV)
    kw = dict(replicas=A.KAT["replicas"], noise_var=A.KAT["noise_var"], seed=0, stages=A.KAT["stages"], power=A.KAT["power"], **H.KAT_RUN)
    ll = trainer.mcpc_ais(d, um.bernoulli_fn, {}, adjust="mala", **kw)
    share = trainer.mcpc_last_ais_acceptance.cpu().numpy()
    exact = A.kat_exact()
    err = ll.log_p.cpu().numpy() - exact
    print("KAT device,", H.KAT_RUN, ": err", np.round(err, 4), "ESS", np.round(ll.ess.cpu().numpy(), 1), f"acceptance {share.min():.3f} .. "
          f"{share.max():.3f}, tol {H.KAT_TOL:.4f}, restatement", np.round(A.log_p(H.kat_run(0)[1]) - exact, 4))
    assert (ll.n_samples == A.KAT["replicas"]).all(), "a replica is not finite"
    assert share.shape == (A.KAT["stages"] - 1,) and (share > 0.5).all() and (share <= 1.0).all()
    parity_log.close("hmc_kat", "log_p against the quadrature", ll.log_p.cpu().numpy(), exact, atol=H.KAT_TOL)


# ---- the closed-form case -----------------------------------------------------------------------------------------------------------------
def test_one_trajectory_of_five_steps_meets_a_bound_on_the_closed_form_case_that_five_mala_steps_miss():
    """smc_cases.CF without resampling, leapfrog=5, steps_per_stage=1, seeds 0..7 (tests/hmc_cases.py).  Every |log_p - exact| <= 2 x
    the largest error of the fp32 restatement (2 x 1.497337), and the pooled rms error <= sqrt(0.687456 x 2.551402) = 1.3244, the
    geometric mean of the restatement's rms with one trajectory of five leapfrog steps and with five MALA steps per rung: a device
    that quietly runs one leapfrog step, or plain MALA (2.55), misses it."""
    _, um = _mods()
    W, b, data = S.cf_params()
    c = S.CF
    _, trainer = build(W, b, "identity", lr=c["lr"])
    d = torch.tensor(data).to(DEV)
    exact = S.cf_exact()
    errs, final, shares = [], [], []
    for seed in H.CF_SEEDS:
        ll = trainer.mcpc_ais(d, um.fe_fn, {"_var": c["var"]}, replicas=c["replicas"], stages=c["stages"], power=c["power"],
                              noise_var=c["noise_var"], seed=seed, adjust="mala", **H.CF_RUNS["hmc"])
        assert (ll.n_samples == c["replicas"]).all(), "a replica is not finite"
        errs.append(ll.log_p.cpu().numpy() - exact)
        final.append(ll.ess.cpu().numpy())
        shares.append(float(trainer.mcpc_last_ais_acceptance.mean()))
    errs, final = np.stack(errs), np.stack(final)
    rms = float(np.sqrt((errs ** 2).mean()))
    want = H.cf_errors("hmc")[0]
    print(f"closed form, device: rms {rms:.4f} (bound {H.cf_rms_bound():.4f}; restatement {np.sqrt((want ** 2).mean()):.4f}), max |err| "
          f"{np.abs(errs).max():.4f} (tolerance {H.cf_tol():.4f}), mean {errs.mean():.4f}, final ESS {final.min():.1f} .. {final.max():.1f}, "
          f"acceptance {np.mean(shares):.3f}, max |err - restatement's| {np.abs(errs - want).max():.3g}")
    parity_log.close("hmc_closed_form", "log_p against the exact value", errs, np.zeros_like(errs), atol=H.cf_tol())
    assert rms <= H.cf_rms_bound()


# ---- with resampling ------------------------------------------------------------------------------------------------------------------------
def test_trajectories_compose_with_resampling():
    _, trainer, loss_fn, kw, data = case_trainer("bern_relu")
    r = run_kw(resample="systematic", ess_threshold=0.5)
    one = trainer.mcpc_ais(data, loss_fn, kw, **r)
    trace, share = trainer.mcpc_last_ais_resampling, trainer.mcpc_last_ais_acceptance
    K = H.ESTIMATOR_RUN["stages"]
    assert torch.isfinite(one.log_p).all() and (one.n_samples == H.ESTIMATOR_RUN["replicas"]).all()
    assert trace is not None and tuple(trace.ess.shape) == (K - 1, A.N_DATA) and tuple(trace.resampled.shape) == (K - 1, A.N_DATA)
    assert tuple(trace.share.shape) == (K - 1,) and torch.isfinite(trace.ess).all() and tuple(share.shape) == (K - 1,)
    for max_chains in (80, 80, 32, 16):
        got = trainer.mcpc_ais(data, loss_fn, kw, max_chains=max_chains, **r)
        t = trainer.mcpc_last_ais_resampling
        assert np.array_equal(bits(got.state), bits(one.state)), f"max_chains={max_chains} moves the state"
        assert np.array_equal(bits(t.ess), bits(trace.ess)) and torch.equal(t.resampled, trace.resampled)
        assert np.array_equal(bits(trainer.mcpc_last_ais_acceptance), bits(share))
    # resampling at every rung moves the chains: the state is not that of the call without it
    every = trainer.mcpc_ais(data, loss_fn, kw, **run_kw(resample="systematic", ess_threshold=1.0))
    assert trainer.mcpc_last_ais_resampling.resampled.any()
    assert not np.array_equal(bits(every.state), bits(device_result("bern_relu")[0].state))

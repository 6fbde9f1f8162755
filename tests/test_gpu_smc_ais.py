"""Annealed importance sampling with resampling, PCTrainer.mcpc_ais(resample="systematic") (montecarlopredictivecoding_amd/ais.py),
against the restatement of tests/smc_cases.py: decisions, ancestors and log-weights on ais_cases' two estimator nets at thresholds 0.5
and 1.0 with both kinds of transition, every bitwise and untouched-state promise of the plain call, and the closed-form linear-Gaussian
case, where the plain estimator misses the bound the resampled one is held to."""
import numpy as np
import pytest
import torch

from tests import ais_cases as A
from tests import parity_log
from tests import smc_cases as S
from tests.test_gpu_ais import DEV, _assert_untouched, _mods, _snapshot, _train, bits, build, case_trainer

pytestmark = pytest.mark.gpu
NAMES = sorted(A.ESTIMATOR_CASES)
R = S.ESTIMATOR_RUN["replicas"]
K = S.ESTIMATOR_RUN["stages"]
_RESULTS = {}


@pytest.fixture(autouse=True)
def philox_steps_as_found():
    """The fused calls of `_train` take their noise from a process-wide step counter: leave it as it was found."""
    from montecarlopredictivecoding_amd.predictive_coding import pc_trainer as pt
    before = pt._PHILOX_STEPS[0]
    yield
    pt._PHILOX_STEPS[0] = before


def run_kw(**over):
    r = dict(S.ESTIMATOR_RUN)                                           # lr = 0.03 is passed: also the trainers' own
    r.update(over)
    return r


def device_result(name, threshold, adjust):
    """(LogLikelihood, logw, accepted, ancestors, the trainer's trace) of a case in one chunk; computed once, never modified."""
    key = (name, threshold, adjust)
    if key not in _RESULTS:
        from montecarlopredictivecoding_amd import ais
        _, trainer, loss_fn, kw, data = case_trainer(name)
        ll, logw, acc, anc = ais.run(trainer, data, loss_fn, kw, return_logw=True, return_accepted=True, return_ancestors=True,
                                     **run_kw(adjust=adjust, resample="systematic", ess_threshold=threshold))
        _RESULTS[key] = (ll, logw, acc, anc, trainer.mcpc_last_ais_resampling)
    return _RESULTS[key]


# ---- against the restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adjust", S.ADJUSTS)
@pytest.mark.parametrize("threshold", S.THRESHOLDS)
@pytest.mark.parametrize("name", NAMES)
def test_decisions_ancestors_and_log_weights_follow_the_restatement(name, threshold, adjust):
    """A datum whose decisions, ancestors and (adjusted) accepted counts are the fp32 restatement's is held to 10 x max |logw32 -
    logw64| (tests/smc_cases.py: ESTIMATOR_FIGURES); at most 1 of the 5 data may disagree and is left out.  The restatement's margins
    (0.022 R and 2.6e-5 S at the closest) make none expected."""
    ll, logw, acc, anc, trace = device_result(name, threshold, adjust)
    want_logw, want_state, want = S.estimator_reference(name, threshold, adjust, "float32")
    got = SimpleTrace(trace.resampled.cpu().numpy(), anc.cpu().numpy().astype(np.int64), None if acc is None else acc.cpu().numpy().astype(np.int64))
    assert got.resampled.shape == (K - 1, A.N_DATA) and got.resampled.dtype == np.bool_ and got.ancestors.shape == (K - 1, A.N_DATA * R)
    assert anc.dtype == torch.int32 and trace.ess.dtype == torch.float64 and tuple(trace.ess.shape) == (K - 1, A.N_DATA)
    assert (acc is None) == (adjust is None)
    same = S.data_that_agree(got, want, R)
    rows = np.repeat(same, R)
    tol = S.estimator_tolerance(name, threshold, adjust)
    glw = logw.cpu().numpy()
    print(f"{name} threshold {threshold} adjust {adjust}: {int((~same).sum())} of {A.N_DATA} data disagree, resampled "
          f"{int(got.resampled.sum())} of {got.resampled.size} pairs (restatement {int(want.resampled.sum())}), "
          f"max |logw - restatement| over the others = {np.abs(glw - want_logw)[rows].max():.3g} (tolerance {tol:.3g}), "
          f"max |ess trace - restatement| = {np.nanmax(np.abs(trace.ess.cpu().numpy() - want.ess)[:, same]):.3g}")
    assert int((~same).sum()) <= S.MAX_DATA_LEFT_OUT
    parity_log.close("smc_estimator", f"{name} {threshold} {adjust} logw", glw[rows], want_logw[rows], atol=tol)
    np.testing.assert_array_equal(ll.n_samples.cpu().numpy(), want_state[:, 3])
    parity_log.close("smc_estimator", f"{name} {threshold} {adjust} log_p", ll.log_p.cpu().numpy()[same], A.log_p(want_state)[same], atol=tol)
    # the trace: ESS before resampling.  ess = S^2 / q with S = sum e, q = sum e^2: log-weights that move by d move S by a factor
    # e^d and q by e^2d at the most, so ess by 4 d relative, and ess <= R: 4 R tol.  And the share of the device's own decisions.
    np.testing.assert_allclose(trace.ess.cpu().numpy()[:, same], want.ess[:, same], rtol=0, atol=4.0 * R * tol)
    np.testing.assert_allclose(trace.share.cpu().numpy(), got.resampled.mean(1), rtol=0, atol=1e-15)
    assert tuple(trace.share.shape) == (K - 1,)
    # a resampled datum's ancestors stay inside the datum; one that is not resampled keeps the identity
    datum = got.ancestors // R
    assert (datum == np.arange(A.N_DATA * R) // R).all()
    ident = np.repeat(~got.resampled, R, axis=1)
    assert (got.ancestors[ident] == np.tile(np.arange(A.N_DATA * R), (K - 1, 1))[ident]).all()


class SimpleTrace:
    def __init__(self, resampled, ancestors, accepted):
        self.resampled, self.ancestors, self.accepted = resampled, ancestors, accepted


def test_both_branches_are_taken():
    trace = device_result("gauss_tanh", 0.5, None)[4]
    n = int(trace.resampled.sum())
    assert 0 < n < trace.resampled.numel(), n
    assert (device_result("gauss_tanh", 1.0, None)[4].resampled).all()
    assert (trace.share > 0).any() and (trace.share < 1).any()


# ---- bitwise ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adjust", S.ADJUSTS)
@pytest.mark.parametrize("name", NAMES)
def test_threshold_zero_is_the_plain_call_bit_for_bit_and_still_fills_the_trace(name, adjust):
    _, trainer, loss_fn, kw, data = case_trainer(name)
    plain = trainer.mcpc_ais(data, loss_fn, kw, **run_kw(adjust=adjust))
    assert trainer.mcpc_last_ais_resampling is None
    zero = trainer.mcpc_ais(data, loss_fn, kw, **run_kw(adjust=adjust, resample="systematic", ess_threshold=0.0))
    trace = trainer.mcpc_last_ais_resampling
    assert np.array_equal(bits(zero.state), bits(plain.state))
    assert not trace.resampled.any() and (trace.share == 0).all()
    ess = trace.ess.cpu().numpy()
    assert np.isfinite(ess).all() and (ess >= 1.0).all() and (ess <= R).all() and (ess < R).any()
    none = trainer.mcpc_ais(data, loss_fn, kw, **run_kw(adjust=adjust, resample=None, ess_threshold=1.0))
    assert trainer.mcpc_last_ais_resampling is None
    assert np.array_equal(bits(none.state), bits(plain.state))
    some = trainer.mcpc_ais(data, loss_fn, kw, **run_kw(adjust=adjust, resample="systematic", ess_threshold=1.0))
    assert not np.array_equal(bits(some.state), bits(plain.state))


@pytest.mark.parametrize("adjust", S.ADJUSTS)
@pytest.mark.parametrize("name", NAMES)
def test_the_result_and_the_trace_do_not_depend_on_the_chunking_or_the_run(name, adjust):
    one, _, _, _, trace = device_result(name, 0.5, adjust)
    _, trainer, loss_fn, kw, data = case_trainer(name)
    for max_chains in (80, 80, 32, 16):
        got = trainer.mcpc_ais(data, loss_fn, kw, max_chains=max_chains, **run_kw(adjust=adjust, resample="systematic", ess_threshold=0.5))
        t = trainer.mcpc_last_ais_resampling
        assert np.array_equal(bits(got.state), bits(one.state)), f"max_chains={max_chains} moves the state"
        assert np.array_equal(bits(t.ess), bits(trace.ess)), f"max_chains={max_chains} moves the ESS trace"
        assert torch.equal(t.resampled, trace.resampled) and np.array_equal(bits(t.share), bits(trace.share))


def test_ancestors_of_a_chunked_call_index_the_chains_of_the_call():
    from montecarlopredictivecoding_amd import ais
    anc = device_result("gauss_tanh", 1.0, None)[3]
    _, trainer, loss_fn, kw, data = case_trainer("gauss_tanh")
    _, got = ais.run(trainer, data, loss_fn, kw, return_ancestors=True, max_chains=32,
                     **run_kw(resample="systematic", ess_threshold=1.0))
    assert torch.equal(got, anc)
    assert ais.run(trainer, data, loss_fn, kw, return_ancestors=True, **run_kw())[1] is None


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
    call = run_kw(resample="systematic", ess_threshold=1.0)
    if fails:
        trainer.mcpc_ais(data, loss_fn, kw, **call)
        assert trainer.mcpc_last_ais_resampling is not None
        from montecarlopredictivecoding_amd import engine as E
        real, calls = E.ais_increment, []

        def third_rung_fails(*a, **k):
            calls.append(1)
            if len(calls) == 3:
                raise RuntimeError("the third rung fails")
            return real(*a, **k)
        monkeypatch.setattr(E, "ais_increment", third_rung_fails)
        with pytest.raises(RuntimeError, match="third rung"):
            trainer.mcpc_ais(data, loss_fn, kw, **call)
        monkeypatch.undo()
        assert trainer.mcpc_last_ais_resampling is None                  # a call that raises leaves no trace behind
    else:
        trainer.mcpc_ais(data, loss_fn, kw, **call)
    _assert_untouched(model, trainer, before)
    for p in model.parameters():
        p.grad = None
    got_xs, got_overall = _train(trainer, um, target)
    assert np.array_equal(got_overall.view(np.int64), want_overall.view(np.int64))
    for a, b in zip(got_xs, want_xs):
        assert np.array_equal(a.cpu().numpy().view(np.int32), b.cpu().numpy().view(np.int32))


# ---- the closed-form case -----------------------------------------------------------------------------------------------------------------
def test_resampling_meets_a_bound_on_the_closed_form_case_that_plain_ais_misses():
    """Identity net, 16 latent units, 24 Gaussian outputs, 4 data x 64 replicas, 16 rungs x 5 unadjusted steps, seeds 0..7, threshold
    0.5 (tests/smc_cases.py: CF).  Every |log_p - exact| <= 2 x the largest error of the fp32 restatement (2 x 2.377614), and the
    pooled rms error <= sqrt(2.911399 x 1.083925) = 1.776, the geometric mean of the restatement's plain and resampled rms: the
    plain estimator (2.91) misses it."""
    _, um = _mods()
    W, b, data = S.cf_params()
    c = S.CF
    _, trainer = build(W, b, "identity", lr=c["lr"])
    d = torch.tensor(data).to(DEV)
    exact = S.cf_exact()
    errs, final = [], []
    for seed in S.CF_SEEDS:
        ll = trainer.mcpc_ais(d, um.fe_fn, {"_var": c["var"]}, replicas=c["replicas"], stages=c["stages"], power=c["power"],
                              steps_per_stage=c["steps_per_stage"], noise_var=c["noise_var"], seed=seed, resample="systematic",
                              ess_threshold=c["threshold"])
        assert (ll.n_samples == c["replicas"]).all(), "a replica is not finite"
        errs.append(ll.log_p.cpu().numpy() - exact)
        final.append(ll.ess.cpu().numpy())
    errs, final = np.stack(errs), np.stack(final)
    rms = float(np.sqrt((errs ** 2).mean()))
    want = S.cf_errors(c["threshold"])[0]
    print(f"closed form, device: rms {rms:.4f} (bound {S.cf_rms_bound():.4f}; restatement {np.sqrt((want ** 2).mean()):.4f}), max |err| "
          f"{np.abs(errs).max():.4f} (tolerance {S.cf_tol():.4f}), mean {errs.mean():.4f}, final ESS {final.min():.1f} .. {final.max():.1f}, "
          f"max |err - restatement's| {np.abs(errs - want).max():.3g}")
    parity_log.close("smc_closed_form", "log_p against the exact value", errs, np.zeros_like(errs), atol=S.cf_tol())
    assert rms <= S.cf_rms_bound()

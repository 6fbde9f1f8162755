"""The host logic of annealed importance sampling (montecarlopredictivecoding_amd/ais.py; PCTrainer.mcpc_ais): the ladder, the scalars
per rung, the normalising constants, the chunking and its chain ids, the calls the ladder of one chunk makes on its engine in both
modes, the fold of log-weights into a LogLikelihood state, everything the call refuses -- and the algorithm itself, on the NumPy restatement of tests/ais_cases.py against an exact value.  No device."""
import math
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from montecarlopredictivecoding_amd import _lib as L
from montecarlopredictivecoding_amd import ais
from montecarlopredictivecoding_amd import predictive_coding as pc
from montecarlopredictivecoding_amd.likelihood import LogLikelihood
from montecarlopredictivecoding_amd.utils import model as um
from tests import ais_cases as A


# ---- the ladder ---------------------------------------------------------------------------------------------------------------------
def test_default_schedule_is_a_power_of_k_over_stages():
    b = ais.schedule(8, 2.0)
    assert b == [(k / 8) ** 2 for k in range(9)] and b[0] == 0.0 and b[-1] == 1.0
    assert ais.schedule(64) == A.schedule(64)
    assert ais.schedule(1) == [0.0, 1.0]
    assert ais.schedule(5, 0.5)[1] == (1 / 5) ** 0.5
    assert ais.schedule(3, betas=(0, 0.25, 1)) == [0.0, 0.25, 1.0]          # an explicit ladder wins over stages / power


@pytest.mark.parametrize("kw", [dict(betas=[0.1, 1.0]), dict(betas=[0.0, 0.9]), dict(betas=[0.0, 0.5, 0.5, 1.0]), dict(betas=[0.0, 0.7, 0.6, 1.0]),
                                dict(betas=[1.0]), dict(betas=[]), dict(betas=[0.0, math.nan, 1.0]), dict(betas="ab"), dict(betas=3),
                                dict(betas=[0.0, 1.0, 1.0]), dict(stages=0), dict(stages=2.5), dict(stages=True), dict(power=0.0),
                                dict(power=-1.0), dict(power=math.inf), dict(stages=4, power=5000.0)])
def test_a_bad_ladder_is_a_value_error(kw):
    with pytest.raises(ValueError):
        ais.schedule(**kw)


def test_scalars_per_loss_and_rung():
    b = ais.schedule(4)
    assert [ais.rung_scalars(L.LOSS_BERNOULLI, b[k - 1], b[k]) for k in (1, 2, 4)] == [
        (0.0, 1.0, 1 / 16, 1.0), (1 / 16, 1.0, 1 / 4, 1.0), (9 / 16, 1.0, 1.0, 1.0)]
    assert [ais.rung_scalars(L.LOSS_GAUSSIAN, b[k - 1], b[k]) for k in (1, 2, 4)] == [
        (1.0, 0.0, 1.0, 1 / 16), (1.0, 1 / 16, 1.0, 1 / 4), (1.0, 9 / 16, 1.0, 1.0)]
    with pytest.raises(ValueError):
        ais.rung_scalars(L.LOSS_NONE, 0.0, 1.0)
    # what the transitions of rung k run: the read-out's scale and the loss variance
    assert ais.rung_run(L.LOSS_BERNOULLI, 1.0, 0.25) == (0.25, 1.0)
    assert ais.rung_run(L.LOSS_GAUSSIAN, 0.7, 0.25) == (1.0, 2.8)


def test_the_increments_telescope_to_the_likelihood():
    """Summed over the ladder at a fixed x, the increments are log f_K - log f_0: -BCE(o, y) + n_active log 2, or -(0.5 / var) |o - y|^2."""
    x, W, b, y, _ = A.increment_inputs("relu_bern_masked")
    ladder = ais.schedule(6)
    logw = np.zeros(x.shape[0])
    for k in range(1, 7):
        logw, _ = A.increment(x, W, b, y, "relu", "bernoulli", None, 21, *ais.rung_scalars(L.LOSS_BERNOULLI, ladder[k - 1], ladder[k]), logw=logw)
    o = (np.maximum(x.astype(np.float64), 0) @ W.astype(np.float64).T + b)[:, 21:]
    bce = (A.softplus(o) - y[:, 21:] * o).sum(1)
    np.testing.assert_allclose(logw - ais.log_norm(L.LOSS_BERNOULLI, 19), -bce, rtol=0, atol=1e-11)
    x, W, b, y, _ = A.increment_inputs("tanh_gauss")
    logw = np.zeros(x.shape[0])
    for k in range(1, 7):
        logw, _ = A.increment(x, W, b, y, "tanh", "gaussian", 0.7, 0, *ais.rung_scalars(L.LOSS_GAUSSIAN, ladder[k - 1], ladder[k]), logw=logw)
    o = np.tanh(x.astype(np.float64)) @ W.astype(np.float64).T + b
    np.testing.assert_allclose(logw, -(0.5 / 0.7) * ((o - y) ** 2).sum(1), rtol=0, atol=1e-11)


def test_normalising_constants():
    assert ais.log_norm(L.LOSS_BERNOULLI, 784) == 784 * math.log(2.0)
    assert ais.log_norm(L.LOSS_BERNOULLI, 19, var=3.0) == 19 * math.log(2.0)
    assert ais.log_norm(L.LOSS_GAUSSIAN, 24, 0.7) == 0.5 * 24 * math.log(2.0 * math.pi * 0.7)
    assert ais.log_norm(L.LOSS_GAUSSIAN, 24, 0.7) == A.log_norm("gaussian", 24, 0.7)


# ---- chunks and chain ids -------------------------------------------------------------------------------------------------------------
def test_chunks_hold_whole_data_and_count_chains_over_the_call():
    assert ais.chunks(5, 16, 80) == [(0, 5, 0)]
    assert ais.chunks(5, 16, 6000, chain_base=7) == [(0, 5, 7)]
    assert ais.chunks(5, 16, 32, chain_base=100) == [(0, 2, 100), (2, 2, 132), (4, 1, 164)]
    assert ais.chunks(5, 16, 31) == [(i, 1, 16 * i) for i in range(5)]
    assert ais.chunks(0, 16, 80) == []
    for kw in (dict(replicas=0), dict(replicas=17, max_chains=16), dict(max_chains=0), dict(chain_base=-1), dict(replicas=2.0),
               dict(chain_base=(1 << 32) - 79)):
        with pytest.raises(ValueError):
            ais.chunks(**dict(dict(n_data=5, replicas=16, max_chains=80, chain_base=0), **kw))


def _words(calls, steps_per_stage):
    """Every (what, chain id, step) an engine call list consumes normals for."""
    out = set()
    for what, g0, sb, n in calls:
        for c in range(g0, g0 + n):
            for t in range(1 if what == "prior" else steps_per_stage):
                w = (what, c, sb + t)
                assert w not in out, f"{w} is consumed twice"
                out.add(w)
    return out


def test_two_chunkings_consume_the_same_normals_and_none_twice():
    kw = dict(n_data=5, replicas=16, n_rungs=8, steps_per_stage=4, step_base=100, chain_base=40)
    one = ais.engine_calls(max_chains=80, **kw)
    assert one == [("prior", 40, 100, 80)] + [("run", 40, 101 + 4 * (k - 1), 80) for k in range(1, 8)]
    words = _words(one, 4)
    assert len(words) == 80 * (1 + 7 * 4)
    # the prior's step and the transitions' steps never meet, whatever the layer: step_base, then step_base + 1 ...
    assert {w[2] for w in words if w[0] == "prior"} == {100} and min(w[2] for w in words if w[0] == "run") == 101
    for max_chains in (32, 16, 79):
        assert _words(ais.engine_calls(max_chains=max_chains, **kw), 4) == words
    parts = ais.engine_calls(max_chains=32, **kw)
    assert [c[:3] for c in parts if c[0] == "prior"] == [("prior", 40, 100), ("prior", 72, 100), ("prior", 104, 100)]


# ---- the ladder of one chunk: every call it makes, in order ---------------------------------------------------------------------------
class LadderRecorder:
    """Stands in for the engine of one chunk and for engine.ais_increment / mala_propose / mala_accept.  Every call is noted as
    ``(name, Philox step, chain_base, update_x, x_next given)``, None where the call has no such argument (``run`` carries its step
    count in the name; a ``run`` that is not told ``update_x`` updates).  No device, no library."""

    def __init__(self, batch, sizes):
        self.batch, self.sizes, self.calls = batch, sizes, []

    def note(self, name, step=None, chain_base=None, update_x=None, x_next=None):
        self.calls.append((name, step, chain_base, update_x, x_next))

    def store_state(self, xs):
        self.note("store_state")

    def load_state(self, xs):
        self.note("load_state")

    def params_changed(self):
        self.note("params_changed")

    def run(self, T, **kw):
        self.note(f"run({T})", kw["step_base"], kw.get("chain_base"), kw.get("update_x", True))
        return types.SimpleNamespace(xgrad=[torch.zeros(self.batch, n) for n in self.sizes])

    def chain_energies(self, inputs, xs, **kw):
        self.note("chain_energies")
        return torch.zeros(1, self.batch, len(self.sizes) + 2, dtype=torch.float64)

    def ais_increment(self, x, W, bias, y, act, loss, var, mask_start, a0, c0, a1, c1, logw, accumulate=True):
        self.note("ais_increment")

    def mala_propose(self, xs, gs, lr, noise_var, seed, step, chain_base=0, out=None):
        self.note("mala_propose", step, chain_base)
        return out

    def mala_accept(self, xs, gs, E, xps, gps, Ep, lr, noise_var, seed, step, chain_base=0, diag=None, n_accepted=None, x_next=None):
        self.note("mala_accept", step, chain_base, None, x_next is not None)


# K = 3 rungs of 2 steps, step_base = 100, the chunk's first chain 40.  The lists were recorded with LadderRecorder over the two separate
# ladders this loop replaced (an inline one for the unadjusted transitions, a function for the adjusted ones), not over the code under test.
_EVALUATE = [("load_state", None, None, None, None), ("run(1)", 0, None, False, None), ("chain_energies", None, None, None, None)]
LADDER_CALLS = {
    None: [
        ("store_state", None, None, None, None), ("ais_increment", None, None, None, None),
        ("params_changed", None, None, None, None), ("run(2)", 101, 40, True, None),
        ("store_state", None, None, None, None), ("ais_increment", None, None, None, None),
        ("params_changed", None, None, None, None), ("run(2)", 103, 40, True, None),
        ("store_state", None, None, None, None), ("ais_increment", None, None, None, None)],
    "mala": [
        ("ais_increment", None, None, None, None), ("params_changed", None, None, None, None),
        *_EVALUATE, ("mala_propose", 101, 40, None, None),
        *_EVALUATE, ("mala_accept", 101, 40, None, True),
        *_EVALUATE, ("mala_accept", 102, 40, None, False),
        ("ais_increment", None, None, None, None), ("params_changed", None, None, None, None),
        *_EVALUATE, ("mala_propose", 103, 40, None, None),
        *_EVALUATE, ("mala_accept", 103, 40, None, True),
        *_EVALUATE, ("mala_accept", 104, 40, None, False),
        ("ais_increment", None, None, None, None)],
}       # the Bernoulli read-out's calls; the Gaussian ladder re-packs nothing: the same without params_changed


def ladder_chunk(rec, loss_kind, adjust):
    """The arguments of ``ais._ladder`` for one chunk of 5 chains on a 4-6 net with 3 outputs, driven by ``rec``."""
    g = torch.Generator().manual_seed(3)
    W_L, b_L = torch.randn(3, 6, generator=g), torch.randn(3, generator=g)
    call = types.SimpleNamespace(adjust=adjust, ladder=ais.schedule(3), steps_per_stage=2, lr=0.05, noise_var=2.0, seed=7, step_base=100,
                                 act=L.ACT_TANH, loss=types.SimpleNamespace(kind=loss_kind, var=0.7, mask_start=1))
    chunk = types.SimpleNamespace(eng=rec, xs=[torch.zeros(5, n) for n in rec.sizes], y=torch.zeros(5, 3),
                                  logw=torch.zeros(5, dtype=torch.float64), g0=40, W_L=W_L, b_L=b_L,
                                  scaled=(W_L.clone(), b_L.clone()) if loss_kind == L.LOSS_BERNOULLI else None)
    return call, chunk


@pytest.mark.parametrize("adjust", [None, "mala"])
@pytest.mark.parametrize("loss_kind", [L.LOSS_BERNOULLI, L.LOSS_GAUSSIAN])
def test_the_ladder_of_a_chunk_makes_these_calls_in_this_order(monkeypatch, loss_kind, adjust):
    from montecarlopredictivecoding_amd import engine as E
    rec = LadderRecorder(5, [4, 6])
    for name in ("ais_increment", "mala_propose", "mala_accept"):
        monkeypatch.setattr(E, name, getattr(rec, name))
    call, chunk = ladder_chunk(rec, loss_kind, adjust)
    accepted = ais._ladder(call, chunk)
    want = [c for c in LADDER_CALLS[adjust] if loss_kind == L.LOSS_BERNOULLI or c[0] != "params_changed"]
    assert rec.calls == want, "\n".join(f"{g} | {w}" for g, w in zip(rec.calls, want))
    assert (accepted is None) if adjust is None else (tuple(accepted.shape) == (2, 5) and accepted.dtype == torch.int32)
    if loss_kind == L.LOSS_BERNOULLI:
        # the last re-pack is that of rung K - 1: the engine is left on the read-out scaled by beta_2
        assert torch.equal(chunk.scaled[0], chunk.W_L * call.ladder[2]) and torch.equal(chunk.scaled[1], chunk.b_L * call.ladder[2])


# ---- the fold -------------------------------------------------------------------------------------------------------------------------
def test_fold_is_a_log_mean_exp_over_the_finite_replicas():
    rng = np.random.default_rng(5)
    logw = 30.0 * rng.standard_normal(6 * 13) - 400.0
    logw[3], logw[14], logw[15] = math.nan, math.inf, -math.inf            # data 0 and 1 lose replicas
    logw[26:39] = math.nan                                                 # datum 2 loses all of them
    const = 19 * math.log(2.0)
    st = ais.fold(torch.tensor(logw), 13, const).numpy()
    want = A.state_from_logw(logw, 13, const)
    np.testing.assert_array_equal(st[:, 3], [12, 11, 0, 13, 13, 13])
    np.testing.assert_array_equal(st[:, 0], want[:, 0])
    np.testing.assert_allclose(st[[0, 1, 3, 4, 5], 1:3], want[[0, 1, 3, 4, 5], 1:3], rtol=1e-14)
    assert st[2].tolist() == [math.inf, 0.0, 0.0, 0.0]
    ll = LogLikelihood(torch.tensor(st))
    finite = np.isfinite(logw.reshape(6, 13))
    for i in (0, 1, 3):
        w = logw.reshape(6, 13)[i][finite[i]] - const
        direct = w.max() + math.log(np.exp(w - w.max()).mean())
        assert abs(float(ll.log_p[i]) - direct) < 1e-12
        assert abs(float(ll.ess[i]) - np.exp(w - w.max()).sum() ** 2 / (np.exp(w - w.max()) ** 2).sum()) < 1e-10
    assert math.isnan(float(ll.log_p[2])) and math.isnan(float(ll.ess[2]))


def test_fold_of_a_datum_does_not_depend_on_the_other_data():
    rng = np.random.default_rng(6)
    logw = torch.tensor(10.0 * rng.standard_normal(7 * 24))
    whole = ais.fold(logw, 24, 1.5)
    parts = torch.cat([ais.fold(logw[:24 * 3], 24, 1.5), ais.fold(logw[24 * 3:24 * 4], 24, 1.5), ais.fold(logw[24 * 4:], 24, 1.5)])
    assert np.array_equal(whole.numpy().view(np.int64), parts.numpy().view(np.int64))


# ---- what the call refuses, before any device is asked for -----------------------------------------------------------------------------
def _trainer(sizes=(6, 16, 16), n_out=24, act=nn.Tanh, optimizer_x_fn=torch.optim.SGD, **kw):
    mods = []
    for i, o in zip(sizes[:-1], sizes[1:]):
        mods += [nn.Linear(i, o), pc.PCLayer(), act()]
    if n_out:
        mods.append(nn.Linear(sizes[-1], n_out))
    else:
        mods.pop()
    model = nn.Sequential(*mods)
    model.train()
    return pc.PCTrainer(model, T=4, optimizer_x_fn=optimizer_x_fn, optimizer_x_kwargs={"lr": 0.03}, update_p_at="never", plot_progress_at=[],
                        **kw)


DATA = torch.zeros(3, 24)


@pytest.mark.parametrize("kw", [dict(betas=[0.0, 0.5]), dict(betas=[0.0, 0.6, 0.4, 1.0]), dict(stages=0), dict(power=-2.0),
                                dict(replicas=0), dict(replicas=1.5), dict(steps_per_stage=0), dict(noise_var=0.0), dict(noise_var=math.nan),
                                dict(lr=0.0), dict(lr=-0.1), dict(lr=math.inf), dict(seed=0.5), dict(step_base=-1), dict(chain_base=-1),
                                dict(max_chains=3, replicas=4), dict(data=torch.zeros(3, 23)), dict(data=torch.zeros(24)),
                                dict(loss_fn_kwargs={"_var": 0.7, "_target": torch.zeros(3, 24)})])
def test_bad_arguments_are_value_errors(kw):
    kw = dict(dict(data=DATA, loss_fn=um.fe_fn, loss_fn_kwargs={"_var": 0.7}), **kw)
    with pytest.raises(ValueError):
        _trainer().mcpc_ais(**kw)


def test_an_adam_trainer_needs_an_lr():
    tr = _trainer(optimizer_x_fn=torch.optim.Adam)
    with pytest.raises(ValueError, match="lr"):
        tr.mcpc_ais(DATA, um.bernoulli_fn)
    tr = _trainer(optimizer_x_fn=torch.optim.SGD)
    tr._optimizer_x_kwargs = {"lr": 0.03, "momentum": 0.9}
    with pytest.raises(ValueError, match="lr"):
        tr.mcpc_ais(DATA, um.bernoulli_fn)


def test_what_the_engine_does_not_express_is_not_implemented():
    with pytest.raises(NotImplementedError):
        _trainer(n_out=0).mcpc_ais(torch.zeros(3, 16), um.fe_fn, {"_var": 0.7})                  # no read-out
    with pytest.raises(NotImplementedError):
        _trainer().mcpc_ais(DATA, None)                                                          # no read-out distribution
    with pytest.raises(NotImplementedError):
        _trainer().mcpc_ais(DATA, um.zero_fn)
    with pytest.raises(NotImplementedError):
        _trainer().mcpc_ais(DATA, um.fe_fn, {})                                                  # a Gaussian without its variance
    with pytest.raises(NotImplementedError):
        _trainer().mcpc_ais(DATA, lambda output, _target: (output ** 4).sum())                   # neither Gaussian nor Bernoulli
    with pytest.raises(NotImplementedError):
        pc.PCTrainer(nn.Linear(3, 3), T=1, update_p_at="never", plot_progress_at=[]).mcpc_ais(torch.zeros(1, 3), um.bernoulli_fn)


def test_valid_calls_reach_the_device():
    if torch.cuda.is_available():
        return                                                   # (tests/test_gpu_ais.py runs them)
    for loss_fn, kw in ((um.fe_fn, {"_var": 0.7}), (um.bernoulli_fn, {}), (um.bernoulli_fn_mask, {"perc": 0.25}), (um.fe_fn_mask, {"_var": 2.0})):
        with pytest.raises(L.MCPCLibraryError):
            _trainer().mcpc_ais(DATA, loss_fn, kw, replicas=4, stages=3)
    with pytest.raises(L.MCPCLibraryError):
        _trainer(optimizer_x_fn=torch.optim.Adam).mcpc_ais(DATA, um.bernoulli_fn, lr=0.05)         # an Adam trainer with its own lr


# ---- the restatement: the tolerances it sets and the algorithm itself -------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(A.ESTIMATOR_CASES))
def test_the_fp32_restatement_stays_where_it_was_measured(name):
    l32, s32 = A.estimator_reference(name, "float32")
    l64, s64 = A.estimator_reference(name, "float64")
    diff = float(np.abs(l32 - l64).max())
    print(f"{name}: max |logw32 - logw64| = {diff:.6g}, recorded {A.FP32_VS_FP64[name]:.6g}")
    assert abs(diff - A.FP32_VS_FP64[name]) <= 1e-3 * A.FP32_VS_FP64[name]
    assert np.isfinite(l32).all() and (s32[:, 3] == A.ESTIMATOR_RUN["replicas"]).all()


def test_kat_tolerance_is_twice_the_largest_recorded_error():
    assert len(A.KAT_ERRORS) == 8 and A.KAT_TOL == 2.0 * max(A.KAT_ERRORS)
    assert np.abs(A.kat_exact(901) - A.kat_exact()).max() < 1e-10           # the quadrature has converged


def test_kat_annealing_beats_prior_sampling_and_meets_the_exact_value():
    exact = A.kat_exact()
    logw, st = A.kat_run(0)
    _, st1 = A.kat_run(0, stages=1)
    err = A.log_p(st) - exact
    print("KAT restatement: err", np.round(err, 4), "ESS ais", np.round(A.ess(st), 1), "ESS prior", np.round(A.ess(st1), 1), "tol", A.KAT_TOL)
    assert np.isfinite(logw).all() and (st[:, 3] == A.KAT["replicas"]).all(), "a replica is not finite"
    assert (A.ess(st) > A.ess(st1)).all(), (A.ess(st), A.ess(st1))
    assert (np.abs(err) <= A.KAT_TOL).all(), err
    assert abs(float(np.abs(err).max()) - A.KAT_ERRORS[0]) < 1e-4           # seed 0 of the recorded list

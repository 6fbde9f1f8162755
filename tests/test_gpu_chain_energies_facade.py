"""Per-chain energies through the trainer: `mcpc_chain_energies` on a fused Langevin call, against the reference's per-datapoint
fixture, `mcpc_state_energies` after a MAP call, and the calls that must refuse the request."""
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import gen_golden_generic as gg
from oracle import mcpc_oracle as mo
from tests import chain_energy_cases as cc
from tests import parity_log

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES, N_OUT, B, T = (6, 16, 16), 24, 40, 12
SPEC = dict(begin=2, stride=3)
STEPS = [2, 5, 8, 11]


def _net(device):
    """6-16-16 -> 24, ReLU; the same weights, data and x0 on whichever device."""
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


def _call(um, model, data, inputs, spec, moments=None, update_p_at="never", chunk=None, **kw):
    import montecarlopredictivecoding_amd.predictive_coding as pc
    import montecarlopredictivecoding_amd.predictive_coding.pc_trainer as pt
    tr = pc.PCTrainer(model, T=T, optimizer_x_fn=torch.optim.SGD, optimizer_x_kwargs={"lr": 0.05}, update_p_at=update_p_at,
                      accumulate_p_at=list(range(6, T)) if update_p_at == "last" else "never",
                      optimizer_p_fn=torch.optim.Adam, optimizer_p_kwargs={"lr": 0.01}, plot_progress_at=[])
    tr.mcpc_seed = 5
    tr.mcpc_chain_energies = spec
    tr.mcpc_moments = moments
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


def _bits(t):
    return t.detach().cpu().numpy().view(np.int64)


def _state(tr, model, res):
    xs = [x.detach().clone() for x in tr.get_model_xs()]
    lin = [p for m in model if isinstance(m, torch.nn.Linear) for p in m.parameters()]
    return xs, [None if p.grad is None else p.grad.clone() for p in lin], [p.detach().clone() for p in lin], {k: res[k] for k in ("loss", "energy", "overall")}


# ---- 5. a fused Langevin call ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nonzero_inputs", [False, True])
def test_fused_call_leaves_the_trace_and_nothing_else_moves(nonzero_inputs):
    um, model, data, inputs = _net(DEV)
    if nonzero_inputs:
        # the engine is handed the inputs themselves, not None: one tensor serves the step kernels and the evaluator of the ring
        inputs = torch.randn(B, SIZES[0], generator=torch.Generator().manual_seed(12)).to(DEV)
    tr, res = _call(um, model, data, inputs, SPEC, is_return_xs=True)
    assert tr.last_call_mode == "fused"
    ce = tr.mcpc_last_chain_energies
    # the last recorded row (step T - 1 holds x before that step's update) is mcpc_state_energies of the state it recorded, bit for bit
    left = [x.detach().clone() for x in tr.get_model_xs()]
    for x, rec in zip(tr.get_model_xs(), res["xs"][STEPS[-1]]):
        x.data.copy_(rec)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        st = tr.mcpc_state_energies(inputs=inputs, loss_fn=um.bernoulli_fn, loss_fn_kwargs={"_target": data, "_var": None})
    for p, q in ((st.loss[0], ce.loss[-1]), (st.energy[0], ce.energy[-1]), (st.overall[0], ce.overall[-1])):
        assert np.array_equal(_bits(p), _bits(q))
    for x, was in zip(tr.get_model_xs(), left):
        x.data.copy_(was)
    assert ce.steps == STEPS
    assert ce.loss.shape == (4, B) and ce.energy.shape == (4, B, 3) and ce.overall.shape == (4, B)
    for t in (ce.loss, ce.energy, ce.overall):
        assert t.dtype == torch.float64 and t.device.type == "cuda"
    group = "mcpc_chain_energies (trainer) summed over chains vs the call's results"
    parity_log.close(group, "loss", ce.loss.sum(1).cpu().numpy(), [res["loss"][t] for t in STEPS], rtol=1e-6)
    parity_log.close(group, "energy", ce.energy.sum((1, 2)).cpu().numpy(), [res["energy"][t] for t in STEPS], rtol=1e-6)
    parity_log.close(group, "overall", ce.overall.sum(1).cpu().numpy(), [res["overall"][t] for t in STEPS], rtol=1e-6)
    # the same call without the request, same seed and x0: final states and results bitwise
    xs, _, _, e = _state(tr, model, res)
    tr0, res0 = _call(um, model, data, inputs, None)
    assert tr0.mcpc_last_chain_energies is None and tr0.last_call_mode == "fused" and tr0.last_record_slices == 0
    xs0, _, _, e0 = _state(tr0, model, res0)
    assert e == e0
    for a, b in zip(xs, xs0):
        assert torch.equal(a, b)


def test_learning_call_leaves_param_grad_bitwise():
    um, model, data, inputs = _net(DEV)
    w0 = {k: v.clone() for k, v in model.state_dict().items() if "_x" not in k}
    step_bytes = 4 * B * sum(SIZES)
    runs = []
    for spec, chunk in ((None, None), (SPEC, None), (SPEC, 2 * step_bytes)):
        model.load_state_dict(w0, strict=False)
        for p in model.parameters():
            p.grad = None
        tr, res = _call(um, model, data, inputs, spec, update_p_at="last", chunk=chunk)
        assert tr.last_call_mode == "fused"
        runs.append((tr, _state(tr, model, res)))
    # (slices of at most 2 steps; the 6 steps that accumulate parameter gradients stay one slice)
    assert runs[1][0].last_record_slices == 1 and runs[2][0].last_record_slices == 4
    xs0, g0, p0, e0 = runs[0][1]
    assert all(g is not None for g in g0) and len(g0) == 8
    for _, (xs, g, p, e) in runs[1:]:
        assert e == e0
        for a, b in zip(xs0 + g0 + p0, xs + g + p):
            assert torch.equal(a, b)
    a, b = runs[1][0].mcpc_last_chain_energies, runs[2][0].mcpc_last_chain_energies
    assert a.steps == b.steps == STEPS
    for p, q in ((a.loss, b.loss), (a.energy, b.energy), (a.overall, b.overall)):
        assert np.array_equal(_bits(p), _bits(q))


# ---- 6. pinned to the reference's per-datapoint values ---------------------------------------------------------------------
class _WithSpec:
    """The package's predictive_coding with the request set on every trainer it builds."""

    def __init__(self):
        import montecarlopredictivecoding_amd.predictive_coding as pc
        self.PCLayer = pc.PCLayer
        self._Trainer = pc.PCTrainer

    def PCTrainer(self, *a, **kw):
        tr = self._Trainer(*a, **kw)
        tr.mcpc_chain_energies = dict(begin=0, stride=1)
        return tr


def test_last_step_matches_the_reference_fixture_per_datapoint():
    # the data of g15_batchelement (the draws of seed 107 do not depend on the layer keywords), without the keywords that leave the kernels
    got, trainer = gg._standard(_WithSpec(), DEV, 107)
    assert trainer.last_call_mode == "fused"
    want = np.load(os.path.join(GOLDEN, "g15_batchelement.npz"))
    ce = trainer.mcpc_last_chain_energies
    assert ce.steps == list(range(7)) and ce.overall.shape == (7, 6) and ce.energy.shape == (7, 6, 3)
    group = "mcpc_chain_energies vs g15_batchelement (the reference's per-datapoint values)"

    def close(q, g, w):
        scale = max(1.0, float(np.abs(w).max()))
        parity_log.close(group, q, g, w, rtol=3e-5, atol=3e-6 * scale)

    close("overall_elementwise", ce.overall[-1].cpu().numpy(), want["overall_elementwise"].reshape(-1))
    for i in range(3):
        assert want[f"epd{i}"].shape == (6, 1)
        close(f"epd{i}", ce.energy[-1, :, i:i + 1].cpu().numpy(), want[f"epd{i}"])
    for key in ("loss", "energy", "overall"):
        close(key, got[key], want[key])
    # and the trace sums to the call's own lists at every step
    parity_log.close(group, "sum over chains of overall[t]", ce.overall.sum(1).cpu().numpy(), got["overall"], rtol=1e-6)


# ---- 7. the state a MAP call leaves -----------------------------------------------------------------------------------
def _map_state(device, energy_coefficient=1.0):
    import montecarlopredictivecoding_amd.predictive_coding as pc
    um, model, data, inputs = _net(device)
    tr = pc.PCTrainer(model, T=20, optimizer_x_fn=torch.optim.Adam, optimizer_x_kwargs={"lr": 0.1}, update_p_at="never",
                      energy_coefficient=energy_coefficient, plot_progress_at=[])
    kw = dict(inputs=inputs, loss_fn=um.bernoulli_fn, loss_fn_kwargs={"_target": data, "_var": None})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = tr.train_on_batch(is_log_progress=False, is_return_results_every_t=False, **kw)
        xs_before = [x.detach().clone() for x in tr.get_model_xs()]
        st = tr.mcpc_state_energies(**kw)
    assert tr.last_call_mode == "fused" and len(res["overall"]) == 1
    for a, b in zip(xs_before, tr.get_model_xs()):
        assert torch.equal(a, b.detach())                    # evaluating moves nothing
    lins = [m for m in model if isinstance(m, torch.nn.Linear)]
    case = dict(sizes=SIZES, n_in=SIZES[0], n_out=N_OUT, act=mo.ACT_RELU, loss=mo.LOSS_BERNOULLI, var=1.0, mask_start=0)
    d = dict(W=[m.weight.detach().cpu().numpy() for m in lins], b=[m.bias.detach().cpu().numpy() for m in lins],
             inputs=inputs.cpu().numpy(), target=data.cpu().numpy())
    want, bound = cc.oracle_rows(case, [x.cpu().numpy()[None] for x in xs_before], d=d, ecoef=[energy_coefficient] * 3)
    return st, want, bound


@pytest.mark.parametrize("device, coef", [(DEV, 1.0), ("cpu", 1.0), (DEV, 0.5)])
def test_state_energies_after_a_map_call(device, coef):
    st, want, bound = _map_state(device, coef)
    assert st.steps == [] and st.loss.shape == (1, B) and st.energy.shape == (1, B, 3) and st.overall.shape == (1, B)
    for t in (st.loss, st.energy, st.overall):
        assert t.dtype == torch.float64 and t.device.type == torch.device(device).type
    # energy is reported divided by the coefficient, as results["energy"] is; overall = loss + coefficient * energy
    got = np.concatenate([st.loss.cpu().numpy()[..., None], st.energy.cpu().numpy() * coef, st.overall.cpu().numpy()[..., None]], axis=-1)
    cc.log_against_bound(parity_log, f"mcpc_state_energies after MAP vs oracle per chain ({device}, energy_coefficient={coef})", got, want,
                         bound, ["loss", "E_1", "E_2", "E_3", "overall"])


def test_get_map_free_energy():
    from torch.utils.data import DataLoader, TensorDataset
    import montecarlopredictivecoding_amd.utils.model as um
    from montecarlopredictivecoding_amd.utils import training_evaluation as te
    torch.manual_seed(5)
    cfg = dict(input_size=SIZES[0], hidden_size=SIZES[1], hidden2_size=SIZES[2], output_size=N_OUT, activation_fn="relu",
               loss_fn=um.bernoulli_fn, input_var=0.3, T_pc=20, optimizer_x_fn_pc=torch.optim.Adam, optimizer_x_kwargs_pc={"lr": 0.1})
    model = um.get_model(cfg, True, sample_x_fn=um.sample_x_fn_normal)
    g = torch.Generator().manual_seed(2)
    data = (torch.rand(32, N_OUT, generator=g) < 0.3).float()
    loader = DataLoader(TensorDataset(data, torch.arange(32) % 10), batch_size=16)
    results = []

    import montecarlopredictivecoding_amd.predictive_coding as pc
    orig = pc.PCTrainer.train_on_batch

    def spy(self, *a, **kw):
        r = orig(self, *a, **kw)
        results.append(r["overall"][0])
        return r

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(7)
        pc.PCTrainer.train_on_batch = spy
        try:
            fe = te.get_map_free_energy(model, cfg, loader, True)
        finally:
            pc.PCTrainer.train_on_batch = orig
    assert fe.shape == (32,) and fe.dtype == torch.float64 and fe.device.type == "cuda" and len(results) == 2
    # the PCLayers hold the MAP state of the last batch: its data against the oracle, chain by chain
    lins = [m for m in model if isinstance(m, torch.nn.Linear)]
    xs = [m.get_x().detach().cpu().numpy()[None] for m in model if hasattr(m, "get_x")]
    case = dict(sizes=SIZES, n_in=SIZES[0], n_out=N_OUT, act=mo.ACT_RELU, loss=mo.LOSS_BERNOULLI, var=1.0, mask_start=0)
    d = dict(W=[m.weight.detach().cpu().numpy() for m in lins], b=[m.bias.detach().cpu().numpy() for m in lins],
             inputs=np.zeros((16, SIZES[0]), np.float32), target=data[16:].numpy())
    want, bound = cc.oracle_rows(case, xs, d=d)
    cc.log_against_bound(parity_log, "get_map_free_energy vs oracle per datum (last batch)", fe[16:].cpu().numpy()[None, :, None],
                         want[..., -1:], bound[..., -1:], ["overall"])
    assert (fe[:16] > 0).all()
    with pytest.raises(AttributeError):
        te.no_such_name_of_the_reference


# ---- 8. calls that leave the fused path; the combination with mcpc_moments ------------------------------------------------------
def test_calls_that_are_not_fused_are_rejected():
    import montecarlopredictivecoding_amd.predictive_coding as pc
    um, model, data, inputs = _net(DEV)
    with pytest.raises(NotImplementedError, match="mcpc_chain_energies.*step by step.*callback_after_backward is set"):
        _call(um, model, data, inputs, SPEC, callback_after_backward=lambda **kw: None)
    assert all(m.get_x() is None for m in model if hasattr(m, "get_x"))      # before any work
    masked = torch.nn.Sequential(torch.nn.Linear(3, 3), pc.PCLayer(M=torch.ones(3, device=DEV)), torch.nn.Linear(3, 2)).to(DEV)
    masked.train()
    tr = pc.PCTrainer(masked, T=3, update_p_at="never", plot_progress_at=[])
    tr.mcpc_chain_energies = dict()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(NotImplementedError, match="mcpc_chain_energies.*generic torch loop.*S/M masks"):
            tr.train_on_batch(inputs=torch.zeros(2, 3, device=DEV), is_log_progress=False, is_return_results_every_t=False)
    with pytest.raises(ValueError, match="begin"):
        _call(um, model, data, inputs, dict(begin=T))
    with pytest.raises(ValueError, match="unknown keys"):
        _call(um, model, data, inputs, dict(layers=(0,)))


def test_one_ring_serves_moments_and_chain_energies():
    um, model, data, inputs = _net(DEV)
    mom = dict(begin=4, stride=2, layers=(0, 2), outputs="sigmoid")
    both, _ = _call(um, model, data, inputs, SPEC, moments=mom)
    only_ce, _ = _call(um, model, data, inputs, SPEC)
    only_mom, _ = _call(um, model, data, inputs, None, moments=mom)
    assert both.last_call_mode == "fused" and only_mom.mcpc_last_chain_energies is None and only_ce.mcpc_last_moments is None
    a, b = both.mcpc_last_chain_energies, only_ce.mcpc_last_chain_energies
    for p, q in ((a.loss, b.loss), (a.energy, b.energy), (a.overall, b.overall)):
        assert np.array_equal(_bits(p), _bits(q))
    m, n = both.mcpc_last_moments, only_mom.mcpc_last_moments
    assert m.n == n.n == 4
    for p, q in ((m.out_sum, n.out_sum), (m.out_sumsq, n.out_sumsq), (m.x_sum[0], n.x_sum[0]), (m.x_sumsq[2], n.x_sumsq[2])):
        assert np.array_equal(_bits(p), _bits(q))
    assert m.x_sum[1] is None

"""Wide networks through PCLayer / PCTrainer: the facade creates the engine again with tuning wide=1 when mcpc_create rejects the
network's widths, says so once per trainer, and the call -- fused, step-wise or staged from a CPU-built model -- matches the oracle at
the contract of the engine tests (energies rtol 1e-6, states 1e-5, param.grad rtol 2e-4 + 2e-5 max|want|)."""
import warnings

import numpy as np
import pytest
import torch

from oracle import gen_golden, philox
from oracle import mcpc_oracle as mo
from oracle.cases import make_case_inputs
from tests import parity_log
from tests import wide_cases as wc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED, STEP_BASE, LR_P = 4242, 9000, 0.05


def _mods():
    import montecarlopredictivecoding_amd.predictive_coding as pc
    import montecarlopredictivecoding_amd.utils.model as um
    return pc, um


def _wide_warnings(caught):
    return [w for w in caught if issubclass(w.category, RuntimeWarning) and "layer-wise kernels" in str(w.message)]


def _trainer(pc, model, T, acc):
    return pc.PCTrainer(model, T=T, update_x_at="all", optimizer_x_fn=torch.optim.SGD, optimizer_x_kwargs={"lr": wc.LR}, update_p_at="last",
                        accumulate_p_at=acc, optimizer_p_fn=torch.optim.SGD, optimizer_p_kwargs={"lr": LR_P}, plot_progress_at=[])


def _call(trainer, um, case, inputs, target, device, callback, cb_kw):
    from montecarlopredictivecoding_amd.predictive_coding import pc_trainer as pt
    trainer.mcpc_seed = SEED
    pt._PHILOX_STEPS[0] = STEP_BASE
    loss_fn, loss_kw = gen_golden.reference_loss(um, case, target, device)
    inp = torch.from_numpy(inputs).to(device)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = trainer.train_on_batch(inputs=inp, loss_fn=loss_fn, loss_fn_kwargs=loss_kw, is_log_progress=False, is_return_results_every_t=True,
                                     is_checking_after_callback_after_t=False, callback_after_t=callback, callback_after_t_kwargs=cb_kw)
    return res, caught


def _check(group, res, trainer, lins, ref, W):
    scale = max(1.0, float(np.abs(ref.overall).max()))
    parity_log.close(group, "overall[t]", res["overall"], ref.overall, rtol=1e-6, atol=1e-6 * scale)
    parity_log.close(group, "energy[t]", res["energy"], ref.energy, rtol=1e-6, atol=1e-6 * scale)
    parity_log.close(group, "loss[t]", res["loss"], ref.loss, rtol=1e-6, atol=1e-6 * scale)
    for l, x in enumerate(trainer.get_model_xs()):
        parity_log.close(group, "x final", x.detach().cpu().numpy(), ref.xs[l], rtol=0, atol=1e-5)
    for j, lin in enumerate(lins):
        g = lin.weight.grad.detach().cpu().numpy()
        parity_log.close(group, "param.grad (W)", g, ref.gW[j], rtol=2e-4, atol=2e-5 * float(np.abs(ref.gW[j]).max()))
        if lin.bias is not None:
            parity_log.close(group, "param.grad (b)", lin.bias.grad.detach().cpu().numpy(), ref.gb[j], rtol=2e-4,
                             atol=1e-4 * max(1e-3, float(np.abs(ref.gb[j]).max())))


def _oracle(case, data, acc, noise, W=None, b=None):
    W0, b0, X0, inputs, target = data
    W, b = (W0 if W is None else W), (b0 if b is None else b)
    T = case["T"]
    nz = (lambda t, l: philox.layer_normals(SEED, STEP_BASE + t, l, 0, case["B"], case["sizes"][l])) if noise else None
    return mo.run(wc.net_spec(case, W, b), inputs, X0, wc.loss_spec(case, target), mo.XOpt(mo.OPT_SGD, wc.LR), T, noise=nz, noise_var=wc.NOISE_VAR,
                  update_p_at=[T - 1], accumulate_p_at=acc)


@pytest.mark.parametrize("name", ["clf512", "b512"])
def test_wide_model_through_the_facade(name):
    pc, um = _mods()
    case = wc.CASES[name]
    data = make_case_inputs(case)
    W, b, X0, inputs, target = data
    T = case["T"]
    acc = list(range(4, T))
    ref = _oracle(case, data, acc, noise=True)
    model, lins = gen_golden.build_reference_model(pc, case, W, b, X0, device=DEV)
    trainer = _trainer(pc, model, T, acc)
    kick = {"_pc_trainer": trainer, "var": wc.NOISE_VAR}
    res, caught = _call(trainer, um, case, inputs, target, DEV, um.random_step, kick)
    said = _wide_warnings(caught)
    assert len(said) == 1, [str(w.message) for w in caught]
    assert "mcpc_lw_fwd_kernel" in str(said[0].message) and "LDS" in str(said[0].message)
    assert trainer.last_call_mode == "fused"
    _check("wide facade, fused: " + name, res, trainer, lins, ref, W)
    # the second call of the same trainer says nothing (its weights have moved by one optimizer_p step: no parity check here)
    res, caught = _call(trainer, um, case, inputs, target, DEV, um.random_step, kick)
    assert not _wide_warnings(caught) and trainer.last_call_mode == "fused"


def test_wide_model_stepwise_with_a_logging_callback():
    pc, um = _mods()
    case = wc.CASES["clf512"]
    data = make_case_inputs(case)
    W, b, X0, inputs, target = data
    T = case["T"]
    acc = list(range(4, T))
    ref = _oracle(case, data, acc, noise=False)
    model, lins = gen_golden.build_reference_model(pc, case, W, b, X0, device=DEV)
    trainer = _trainer(pc, model, T, acc)
    seen = []

    def log_step(t, _pc_trainer):                    # reads the state every step: nothing the fused loop can do
        seen.append((t, float(list(_pc_trainer.get_model_xs())[0].detach().abs().max())))

    res, caught = _call(trainer, um, case, inputs, target, DEV, log_step, {"_pc_trainer": trainer})
    assert trainer.last_call_mode == "stepwise" and len(seen) == T
    assert len(_wide_warnings(caught)) == 1
    _check("wide facade, step-wise: clf512", res, trainer, lins, ref, W)


def test_wide_model_built_on_the_cpu_is_staged():
    pc, um = _mods()
    case = wc.CASES["b512"]
    data = make_case_inputs(case)
    W, b, X0, inputs, target = data
    T = case["T"]
    acc = list(range(4, T))
    ref = _oracle(case, data, acc, noise=True)
    model, lins = gen_golden.build_reference_model(pc, case, W, b, X0, device="cpu")
    trainer = _trainer(pc, model, T, acc)
    res, caught = _call(trainer, um, case, inputs, target, "cpu", um.random_step, {"_pc_trainer": trainer, "var": wc.NOISE_VAR})
    assert trainer.last_call_mode == "fused" and len(_wide_warnings(caught)) == 1
    assert all(x.device.type == "cpu" for x in trainer.get_model_xs())
    _check("wide facade, staged CPU model: b512", res, trainer, lins, ref, W)


def test_three_training_iterations_of_the_classifier():
    """Every iteration is its own parity check against the oracle started from the model's CURRENT weights and the freshly drawn x, so
    nothing compounds; between them the trainer's own optimizer_p (SGD) moves the weights, and the wide path packs them again."""
    pc, um = _mods()
    case = wc.CASES["clf512"]
    data = make_case_inputs(case)
    W, b, X0, inputs, target = data
    T = case["T"]
    acc = list(range(4, T))
    model, lins = gen_golden.build_reference_model(pc, case, W, b, X0, device=DEV)
    trainer = _trainer(pc, model, T, acc)
    kick = {"_pc_trainer": trainer, "var": wc.NOISE_VAR}
    moved = []
    for it in range(3):
        Wc = [lin.weight.detach().cpu().numpy().copy() for lin in lins]
        bc = [None if lin.bias is None else lin.bias.detach().cpu().numpy().copy() for lin in lins]
        ref = _oracle(case, data, acc, noise=True, W=Wc, b=bc)
        res, _ = _call(trainer, um, case, inputs, target, DEV, um.random_step, kick)
        assert trainer.last_call_mode == "fused"
        _check("wide facade, training iteration %d: clf512" % it, res, trainer, lins, ref, Wc)
        moved.append(float(np.abs(lins[1].weight.detach().cpu().numpy() - Wc[1]).max()))
    assert all(m > 0 for m in moved), moved

"""The specialised instantiations of the in-place step kernel against its generic one (csrc/mcpc_ws2_lean.h: Ws2Mode).

Every case runs the same call on two engines -- the default, whose launches take a specialised instantiation where
`ws2_select_mode` (csrc/mcpc_run.hip) finds that every workgroup would decide alike, and `tuning="spec=0"`, which keeps every
launch on the generic kernel -- from the same state and seed, and demands

* bitwise equal final states, recorded states and read-out records, and flat gradient bucket (`torch.equal`): a mode removes
  branches and dead paths, not one floating-point operation;
* energies equal to 2e-6 relative, the bound `bench.py`'s self_check uses.  Observed on an MI355X: bitwise equal in every case
  (printed per case: run with -s);
* from `last_step_kernel()`, that the two engines really ran different instantiations -- or, for the nets no specialised mode
  serves, that both stayed on the generic one and the name says so by carrying no tag.

Shapes are the smallest that still take every path: cfg-M's net for the four-chunk read-out and the hand-off, a ragged net whose last
unit and last tiles are partly padding, one 16-chain unit more than the chip has CUs for the round schedule (whose default cycle is
longer than a call of 12 steps: the case runs once as planned and once with a cycle short enough to be taken)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
RELU, TANH = 1, 2
CFG_M = ([30, 256, 256], 784)
RAGGED = ([20, 40, 24], 50)
N_IN = 10
SPEC = "mcpc_steps_ws2_spec_kernel"
GENERIC = "mcpc::mcpc_steps_ws2_kernel<1, "


def _problem(sizes, n_out, B, seed):
    g = torch.Generator().manual_seed(seed)
    dims = [N_IN] + sizes + [n_out]
    W = [(torch.randn(dims[j + 1], dims[j], generator=g) / dims[j] ** 0.5).to(DEV) for j in range(len(dims) - 1)]
    b = [(0.1 * torch.randn(dims[j + 1], generator=g)).to(DEV) for j in range(len(dims) - 1)]
    y01 = (torch.rand(B, n_out, generator=g) < 0.3).float().to(DEV)
    yreal = torch.randn(B, n_out, generator=g).to(DEV)
    inputs = torch.randn(B, N_IN, generator=g).to(DEV)
    x0 = [torch.randn(B, n, generator=g).to(DEV) for n in sizes]
    return W, b, y01, yreal, inputs, x0


def _run(net, act, B, tuning, T, acc, gaussian=False, adam=False, settle=False):
    from montecarlopredictivecoding_amd import _lib as L
    from montecarlopredictivecoding_amd.engine import Engine
    sizes, n_out = net
    W, b, y01, yreal, inputs, x0 = _problem(sizes, n_out, B, seed=B + sum(sizes))
    eng = Engine(sizes, [act] * len(sizes), N_IN, n_out, B, device=DEV, tuning=tuning)
    try:
        eng.bind_params(W, b)
        eng.bind_inputs(inputs)
        eng.bind_target(yreal if gaussian else y01)
        eng.load_state(x0)
        if settle:
            torch.cuda.synchronize()
        n_rec = min(T, 5)
        how = dict(xopt=L.XOPT_ADAM, lr=0.1, noise_mode=L.NOISE_NONE) if adam else dict(lr=0.03, noise_mode=L.NOISE_PHILOX)
        res = eng.run(T, loss_kind=L.LOSS_GAUSSIAN if gaussian else L.LOSS_BERNOULLI, **how,
                      noise_var=2.0, seed=11, step_base=0, acc_begin=acc[0], acc_end=acc[1], energy_mode=L.ENERGY_ALL,
                      rec_begin=T - n_rec, rec_stride=1, rec_count=n_rec, rec_x=True, rec_out=True)
        xs = [torch.empty_like(x) for x in x0]
        eng.store_state(xs)
        flat = eng.read_param_grads_flat()
        eng.sync_check()
        return dict(x=xs, rec=res.rec_x + [res.rec_out], flat=flat, energies=res.energies, step=eng.last_step_kernel(),
                    pref=eng.query()["step_kernel"])
    finally:
        eng.close()


def _join(*keys):
    return ",".join(k for k in keys if k)


def _compare(case, net, act, B, T, acc, tuning="", gaussian=False, adam=False, spec_wait="spec_wait=0", settle=False):
    # spec_wait=0 (the default, spelt out): the run waits for the host copy of the target's flags however short it is
    a = _run(net, act, B, _join(tuning, spec_wait) or None, T, acc, gaussian, adam, settle)
    g = _run(net, act, B, _join(tuning, "spec=0"), T, acc, gaussian, adam, settle)
    for u, v in zip(a["x"] + a["rec"], g["x"] + g["rec"]):
        assert torch.isfinite(u).all() and torch.equal(u, v), case
    assert torch.equal(a["flat"], g["flat"]), case
    if acc[1] > acc[0]:
        assert bool(a["flat"].any()), case
    ea, eg = a["energies"], g["energies"]
    rel = ((ea - eg).abs() / eg.abs().clamp_min(1e-300)).max().item()
    print(f"[spec modes] {case}: default ran {a['step']!r}, spec=0 ran {g['step']!r}; energies bitwise equal: "
          f"{torch.equal(ea, eg)} (largest relative difference {rel:.2e})")
    assert bool(eg.any()) and rel <= 2e-6, (case, rel)
    # spec=0: the generic kernel alone, named as it always was
    assert GENERIC in g["step"] and SPEC not in g["step"], g["step"]
    return a["step"], g["step"]


def test_full_readout_width_with_a_wrapping_spill_ring():
    # four read-out chunks, hand-off, spill and flush; 32 accumulating steps through a ring of 12 slots in three parts (a spill this
    # small stays in the L2: those launches keep the generic kernel, the mixing steps in front of them take the hot mode)
    step, _ = _compare("cfg-M net, batch 32", CFG_M, RELU, 32, 40, (8, 40), tuning="slot_cap=12", spec_wait="")
    assert GENERIC in step and f"[{SPEC}: generic, hot]" in step, step


def test_inference_only_call_takes_the_mode_without_spill():
    step, _ = _compare("cfg-M net, inference only", CFG_M, RELU, 32, 12, (0, 0))
    assert step == f"{GENERIC}false> [{SPEC}: hot]", step


def test_short_call_takes_the_mode_once_the_flags_have_landed():
    # a threshold above the call's 12 steps: the run only polls the copy; with the stream drained in front of it the copy has landed
    step, _ = _compare("cfg-M net, inference only, short call", CFG_M, RELU, 32, 12, (0, 0), spec_wait="spec_wait=100", settle=True)
    assert step == f"{GENERIC}false> [{SPEC}: hot]", step


def test_map_warm_up_takes_the_adam_mode_and_an_accumulating_adam_call_none():
    step, _ = _compare("cfg-M net, Adam on x", CFG_M, RELU, 32, 12, (0, 0), adam=True)
    assert step == f"{GENERIC}false> [{SPEC}: map]", step
    step, step0 = _compare("cfg-M net, Adam on x, accumulating", CFG_M, RELU, 32, 12, (4, 12), adam=True)
    assert step == f"{GENERIC}false> [{SPEC}: generic, map]" and step0 == f"{GENERIC}false>", (step, step0)


def test_ragged_net_with_a_partly_padded_last_unit():
    # widths that are no multiple of 16 or 32; batch 40: the third 16-chain unit holds 8 chains and 8 rows of padding
    step, _ = _compare("ragged net, batch 40", RAGGED, RELU, 40, 12, (4, 12), tuning="ws=2")
    assert f"[{SPEC}: generic, hot]" in step, step


@pytest.mark.parametrize("what", ["tanh", "gaussian"])
def test_nets_without_a_specialised_mode_stay_generic_and_say_so(what):
    step, step0 = _compare(f"ragged net, {what}", RAGGED, TANH if what == "tanh" else RELU, 40, 12, (4, 12), tuning="ws=2",
                           gaussian=what == "gaussian")
    assert step == step0 == f"{GENERIC}false>", (step, step0)


@pytest.mark.parametrize("dealt", ["short cycle", "default plan"])
def test_round_schedule_with_accumulation(dealt):
    # One 16-chain unit more than the chip has CUs: the smallest shard that is dealt into rounds.  The default plan deals it into a
    # cycle longer than this call (on 256 CUs: 12 launches, every unit in 11 of them), so that its 4 + 8 steps run as plain launches
    # of 257 workgroups.  With half the CUs set aside (cu_slack) the cycle is two launches with every unit in one of them, and both
    # stretches of the call run on the round schedule's form of the kernel: MIX with the spill off and on.
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    B = 16 * (cus + 1)
    tuning = f"cu_slack={cus - (cus + 2) // 2}" if dealt == "short cycle" else ""
    step, step0 = _compare(f"round schedule ({dealt}), {B} chains", CFG_M, RELU, B, 12, (4, 12), tuning=tuning)
    if dealt == "short cycle":
        assert "round schedule: k=2 " in step and "round schedule: k=2 " in step0, (step, step0)
        assert step.startswith(f"{GENERIC}true>") and step.endswith(f"[{SPEC}: hot, hot+spill]") and " + " not in step, step
    else:
        assert step == f"{GENERIC}false> [{SPEC}: hot, hot+spill]", step


def test_wrapping_spill_ring_under_the_spilling_mode():
    # A shard large enough for its spill to go out at system scope (the mode with the spill on), its ring capped at 6 slots in three
    # parts: 16 accumulating steps go round it more than twice, every segment flushed beside the next.
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    step, _ = _compare("cfg-M net, large shard, wrapping ring", CFG_M, RELU, 16 * (cus + 1), 20, (4, 20), tuning="slot_cap=6")
    assert step == f"{GENERIC}false> [{SPEC}: hot, hot+spill]", step


def test_mixing_and_sampling_steps_of_one_call_take_both_modes():
    # 4 mixing + 8 sampling steps: one launch without and one with the spill inside the same call
    step, _ = _compare("cfg-M net, 4 + 8 steps", CFG_M, RELU, 32, 12, (4, 12))
    assert f"[{SPEC}: generic, hot]" in step, step

"""A run does what its plan says (csrc/mcpc_plan.h: plan_run; csrc/mcpc_run.hip: mcpc_run executes the plan's items in order).

With profiling on, mcpc_run brackets every launch of the step kernel with HIP events and counts the steps the launches cover
(mcpc_last_step_kernel_ms); mcpc_last_step_kernel_name names the forms it launched.  Both must be what mcpc_debug_run_plan plans for
the device's own CU count, and mcpc_last_flush_plan must be the text planned for the run's last flushing item:
  * one bracket per plain item -- also on the layer-wise kernels, where the bracket is around the whole pair-per-step sequence of
    the item (launch_lw_steps), not around each of its 2 n launches -- and rr_k per cycle of the round schedule;
  * the steps of all items, which tile the run: n_steps;
  * the plain kernel's name exactly when the plan holds a plain item, the round schedule's exactly when it holds a cycle.
The shapes are the smallest at which each branch of the executor runs: 20 units of a 16-16 -> 16 net, T = 40 with the window [7, 33)
and a ring of 3 parts of 2 slots (13 segments: the ring wraps four times), flushes overlapped and serial, `rr=0`, the barrier kernel,
the layer-wise kernels.  `cu_slack` leaves 16 CUs to the round schedule, but a shard is only dealt into rounds when it has more units
than the device has CUs (plan_engine), so at 20 units every item of these cases is a plain launch; the cycles -- inside and outside
the window, and the plain remainder behind them -- run in the two cases of one and a half units per CU (k = 3, m = 2).
Schedules of the same kernel agree as tests/test_gpu_rounds.py states: states and records bitwise, energies up to the regrouping of
fp32 partial sums, Hebbian sums bitwise where both schedules cut the window into the same segments."""
import functools

import numpy as np
import pytest
import torch

from tests.plan_util import plan, run_plan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES, N_OUT = [16, 16], 16
T, WINDOW = 40, (7, 33)
PLAIN = {"layer-wise": "mcpc::mcpc_lw_fwd_kernel + mcpc::mcpc_lw_bwd_kernel", "barrier": "mcpc::mcpc_steps_kernel<1, 4>"}


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _case(name):
    """(batch, tuning) of a case; `small`: 20 units with 16 CUs left by cu_slack, `more`: three units per two CUs."""
    cus = _cus()
    small = "cu_slack=%d,slot_cap=6" % max(cus - 16, 0)
    return {"small": (320, small), "small,no_overlap=1": (320, small + ",no_overlap=1"), "small,rr=0": (320, small + ",rr=0"),
            "small,ws=0": (320, small + ",ws=0"), "small,ws=4": (64, small + ",ws=4"),
            "more": (24 * cus, "slot_cap=6"), "more,rr=0": (24 * cus, "slot_cap=6,rr=0"),
            "more,ws=2": (24 * cus, "slot_cap=6,ws=2"), "more,ws=2,rr=0": (24 * cus, "slot_cap=6,ws=2,rr=0")}[name]


@functools.lru_cache(maxsize=None)
def _ran(name):
    """One learning call of the case with profiling on: its plans, what the library reports, and its results (computed once)."""
    from montecarlopredictivecoding_amd import _lib as L
    from montecarlopredictivecoding_amd.engine import Engine
    batch, tuning = _case(name)
    g = torch.Generator().manual_seed(5)
    dims = [SIZES[0]] + SIZES + [N_OUT]
    W = [((torch.rand(dims[j + 1], dims[j], generator=g) * 2 - 1) / dims[j] ** 0.5).to(DEV) for j in range(3)]
    b = [((torch.rand(dims[j + 1], generator=g) * 2 - 1) / dims[j] ** 0.5).to(DEV) for j in range(3)]
    y = (torch.rand(batch, N_OUT, generator=g) < 0.3).float().to(DEV)
    xs = [((torch.rand(batch, n, generator=g) * 2 - 1) * 0.5).to(DEV) for n in SIZES]
    eng = Engine(SIZES, [L.ACT_RELU] * 2, SIZES[0], N_OUT, batch, device=DEV, tuning=tuning)
    eng.bind_params(W, b); eng.bind_inputs(None); eng.bind_target(y)
    eng.load_state(xs)
    eng.set_profiling(True)
    res = eng.run(T, loss_kind=L.LOSS_BERNOULLI, lr=0.03, noise_mode=L.NOISE_PHILOX, seed=3, step_base=11, acc_begin=WINDOW[0],
                  acc_end=WINDOW[1], energy_mode=L.ENERGY_ALL, rec_begin=0, rec_stride=9, rec_count=5, rec_x=True)
    _, launches, steps = eng.last_step_kernel_ms()
    name_ran = eng.last_step_kernel()
    flush_text = [eng.last_flush_plan(j) for j in (1, 2)]
    eng.set_profiling(False)
    out = [torch.empty_like(x) for x in xs]
    eng.store_state(out)
    grads = eng.read_param_grads_flat()
    eng.sync_check()
    eng.close()
    net = dict(sizes=SIZES, n_out=N_OUT, batch=batch, tuning=tuning, n_cu=_cus(), total_mem=torch.cuda.get_device_properties(0).total_memory,
               n_in=SIZES[0])
    run = dict(T=T, t_begin=0, n_steps=T, acc_begin=WINDOW[0], acc_end=WINDOW[1], update_x=1, xopt_kind=L.XOPT_SGD,
               noise_mode=L.NOISE_PHILOX, loss_kind=L.LOSS_BERNOULLI)
    rp = run_plan(run=run, **net)
    return dict(plan=plan(**net), items=[dict(zip(rp["fields"], it)) for it in rp["items"]], unified=rp["unified"], launches=launches,
                steps=steps, name=name_ran, flush_text=flush_text, planned_text=rp["flushes"][-1]["text"], states=[t.cpu().numpy() for t in out + list(res.rec_x)], energies=res.energies.cpu().numpy(),
                grads=grads.cpu().numpy())


@pytest.mark.parametrize("name", ["small", "small,no_overlap=1", "small,rr=0", "small,ws=0", "small,ws=4", "more", "more,ws=2"])
def test_a_run_launches_what_its_plan_holds(name):
    c = _ran(name)
    p, items = c["plan"], c["items"]
    rr_k = p["rounds"]["k"]
    assert c["launches"] == sum(rr_k if k["q"] else 1 for k in items), (c["launches"], items)
    assert c["steps"] == T == sum(k["n"] for k in items)
    assert c["flush_text"] == c["planned_text"]          # the last flush ran the launches planned for the last flushing item
    has_plain, has_cycle = any(not k["q"] for k in items), any(k["q"] for k in items)
    plain = PLAIN.get(p["form"], "mcpc::mcpc_steps_u_kernel<false>" if c["unified"] else "mcpc::mcpc_steps_ws2_kernel<1, false>")
    cycle = "mcpc::mcpc_steps_u_kernel<true>" if c["unified"] else "mcpc::mcpc_steps_ws2_kernel<1, true>"
    assert (plain in c["name"]) == has_plain and ((cycle + " (round schedule: k=%d " % rr_k) in c["name"]) == has_cycle, (c["name"], items)
    # the branches the case is there for
    acc = [k for k in items if k["acc"]]
    assert [k["n"] for k in acc] == ([6, 6, 6, 6, 2] if "no_overlap" in name else [2] * 13)      # serial: the whole ring is one part
    assert np.all(np.isfinite(c["energies"])) and np.abs(c["grads"]).max() > 0
    if name.startswith("more") and "rr=0" not in name:
        assert p["rounds"]["on"] and (rr_k, p["rounds"]["m"]) == (3, 2) and p["workgroups"] == 24 * _cus() // 16
        # [0, 7) and [33, 40): a cycle of 2 x 3 steps and one plain step; the window: 13 cycles of 2 x 1
        assert [(k["n"], k["q"]) for k in items if not k["acc"]] == [(6, 3), (1, 0)] * 2 and all(k["q"] == 1 for k in acc)
    else:
        assert not has_cycle
    assert [k["part"] for k in acc] == ([0] * 5 if "no_overlap" in name else [i % 3 for i in range(13)])
    assert p["form"] == {"small,ws=0": "barrier", "small,ws=4": "layer-wise"}.get(name, "in-place")


@pytest.mark.parametrize("rounds,hw", [("small", "small,rr=0"), ("more", "more,rr=0"), ("more,ws=2", "more,ws=2,rr=0")])
def test_the_round_schedule_agrees_with_hardware_rounds_at_the_same_ring(rounds, hw):
    a, c = _ran(rounds), _ran(hw)
    for x, z in zip(a["states"], c["states"]):
        assert np.array_equal(x, z)
    np.testing.assert_allclose(a["energies"], c["energies"], rtol=2e-6)
    segments = lambda r: [(k["t0"], k["n"]) for k in r["items"] if k["acc"]]
    if segments(a) == segments(c):       # the flushes add the same partial sums in the same order
        assert np.array_equal(a["grads"], c["grads"])
    else:
        np.testing.assert_allclose(a["grads"], c["grads"], rtol=0, atol=2e-6 * np.abs(c["grads"]).max())

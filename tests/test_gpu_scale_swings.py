"""The step GEMMs' row scales when a row's magnitude jumps in time: the cases of tests/scale_swing_cases.py (read its docstring first) on
every step kernel form.  `mcpc_last_step_kernel_name` proves which kernel ran.

WHICH RUNS KEEP ROW WORDS.  Only the LEAN epilogues of the in-place kernel and the unified-wave kernel keep them (rowexp_track): a fused SGD
update with or without the Philox kick, or Adam without noise (csrc/mcpc_steps_ws2_body.inc: `lean`, `rowexp`).  Injected noise, a
gradients-only step and tuning no_lean=1 run the in-place kernel's generic epilogues, whose GEMM waves scan every row themselves, as the
barrier kernel does.  So Part A and the gradients-only step of Part C hold the SCANS (and the chunk sums' rescaling) to rows that jump, on
every form, and Part B and the update steps of Part C hold the WORDS to the scans.

PART A (injected kicks; forms default, ws=2, ws=2,no_lean=1, ws=0, ws=4 and the round schedule).  From the GPU run's OWN records the teeth are
asserted first (in every 16-chain tile, at every step, for every layer a row that rose by 2^20 beside one that fell by 2^20; under ReLU the
zero transitions), then
  1. bitwise against the barrier kernel (ws=0): states, records and recorded outputs of every other form equal its where the project
     states bitwise agreement -- the LDS-resident forms under a bounded Bernoulli read-out, every form with the read-out removed.
     An exponent that belongs to the row's previous content costs headroom bits on a FALLING row and no accuracy an fp64 bound could
     see; this sees it.
  2. the read-out's forward GEMM against fp64, sharply: a recorded output row against f(x_t) W^T + b of the recorded fp32 state, every element
     within C_OP + c_acc(K) + 2^-24 of its own sum |terms| (tests/test_gpu_accuracy.py).
  3. every step against fp64, GROSSLY: x_{t+1} against one fp64 step from the recorded x_t, within 1e-6 of the element's sum |terms|, all
     finite.  NOT a precision test: with a Linear gain of 2^-24 the terms are dominated by the kick and by x itself, lost bits of a GEMM
     are invisible.  It sees what a stale exponent on a RISING row gives: an fp16 overflow, Inf, then NaN in the chain.
  4. chains stay independent: with the schedule of one chain replaced by a constant-scale one every other chain keeps its bits.
PART B (growth, decay, Adam; forms default and ws=3 -- the unified-wave kernel --, ws=2 -- a specialised instantiation on the all-ReLU
regimes --, ws=0): the teeth from the records, assertions 1 and 3 (sharp on growth, where the GEMM terms are x_{t+1}), and the same call cut
in two mcpc_runs mid-way, bitwise the single run: a launch starts its words at generation 0 from a state far from the previous launch's.
PART C (chunks of a Gaussian read-out error 2^20 apart): one gradients-only step returns the back-projection, one update step from x = 0 its
negative through the lean epilogues and the ring slots' words; per entry the bound of its chunk (scale_swing_cases.c_reference), everything
finite.  Two steps whose error rows have the chunks in opposite orders, or every chunk 2^11 lower, against fp64 as in assertion 3.  And
wherever the lean epilogues serve, ws=2 (words) bitwise against ws=2,no_lean=1 (scans of the same kernel with the same chunks: the
agreement tests/test_gpu_rounds.py: test_epilogue_operands_in_lds_match_global_memory states, Gaussian loss included).

NEGATIVE CHECK (scratch builds, never committed): rowexp_track passed generation 0 at ONE call site of csrc/mcpc_ws2_lean.h, so that a
word only ever grows.  The FX-row site fails the bitwise and the fp64 test of growth_relu and decay on default, ws=3 and ws=2, decay's cut
call and the falling two-step case; the E-row site the same three tests of decay; the ring-slot site the falling two-step case alone.
No case of Part A can fail: its runs keep no words.

The achieved error / bound of every comparison goes to the parity log."""
import functools

import numpy as np
import pytest
import torch

from tests import parity_log
from tests import scale_swing_cases as sc
from tests.test_gpu_flush import STEP_WANT
from tests.test_gpu_wide import _t, final_states, loss_kw, make_engine

pytestmark = pytest.mark.gpu

U_KERNEL, WS2_KERNEL, BARRIER_KERNEL = STEP_WANT["ws=3"], STEP_WANT["ws=2"], STEP_WANT["ws=0"]
WS2_ANY = WS2_KERNEL.split("<")[0]                 # (the round schedule runs another instantiation of the same kernel)
SPEC = "mcpc_steps_ws2_spec_kernel"
ROUND = "round"                                    # Part A's round-schedule case: default tuning on the batch the plan deals into rounds
A_FORMS = [None, "ws=2", "ws=2,no_lean=1", "ws=0", "ws=4"]
A_LDS_FORMS = [None, "ws=2", "ws=2,no_lean=1"]         # (beside ws=0)
B_FORMS = [None, "ws=3", "ws=2", "ws=0"]
C_FORMS = ["ws=2", "ws=2,no_lean=1", "ws=0", "ws=3", "ws=4"]
NET = [(a, r) for a in sc.A_ACTS for r in (True, False)]
NET_IDS = [f"{a}-{'readout' if r else 'no_readout'}" for a, r in NET]


def _id(form):
    return form or "default"


def _lw(step):
    return "mcpc_lw_fwd_kernel" in step and "mcpc_lw_bwd_kernel" in step


def _hold(group, quantity, worst, bound=1.0, who=""):
    """worst <= bound, the achieved fraction of the bound in the parity log."""
    print(f"[{group}] {quantity} {who}: {worst:.3e} (bound {bound:.3e})")
    assert np.isfinite(worst), (group, quantity, who)
    parity_log.close(group, quantity, np.array([worst / bound]), np.array([0.0]), rtol=0.0, atol=1.0, err_msg=who)


def _finite(arrays, who):
    for i, a in enumerate(arrays):
        assert np.isfinite(a).all(), f"{who}: non-finite values in array {i}"


@functools.lru_cache(maxsize=None)
def _cus():
    return torch.cuda.get_device_properties(torch.device("cuda", 0)).multi_processor_count


# ================================================================================================================================
# PART A
def _a_batch(form):
    return sc.round_batch(_cus()) if form == ROUND else sc.B


def _a_call(eng, case, X0, kicks):
    from montecarlopredictivecoding_amd import _lib as L
    eng.load_state([_t(x) for x in X0])
    res = eng.run(sc.A_T, xopt=L.XOPT_SGD, lr=1.0, noise_mode=L.NOISE_EXTERNAL, noise_var=1.0, ext_noise=[_t(k) for k in kicks],
                  rec_begin=0, rec_stride=1, rec_count=sc.A_T, rec_x=True, rec_out=True, **loss_kw(case))
    eng.sync_check()
    states = sc.states_of([r.cpu().numpy() for r in res.rec_x], final_states(eng, case))
    return states, None if res.rec_out is None else res.rec_out.cpu().numpy(), eng.last_step_kernel()


@functools.lru_cache(maxsize=None)
def _a_run(act, readout, form):
    """One engine per (net, form): the call, and the call again with the schedule of chain A_FLAT replaced by a constant-scale one."""
    batch = _a_batch(form)
    case = sc.a_case(act, readout, batch)
    W, b, X0, inputs, target = sc.a_data(act, readout, batch)
    eng = make_engine(case, "" if form in (None, ROUND) else form, W=W, b=b, inputs=inputs, target=target)
    try:
        states, outs, step = _a_call(eng, case, X0, sc.a_kicks(batch))
        flat_states, flat_outs, flat_step = _a_call(eng, case, X0, sc.a_kicks(batch, flat=sc.A_FLAT))
    finally:
        eng.close()
    assert step == flat_step, (step, flat_step)
    return dict(states=states, outs=outs, step=step, flat_states=flat_states, flat_outs=flat_outs)


def _a_cases(forms, nets=NET, ids=NET_IDS):
    """(act, readout, form) of every net on every form, and the round-schedule case on its one net."""
    out = [pytest.param(a, r, f, id=f"{i}-{_id(f)}") for (a, r), i in zip(nets, ids) for f in forms]
    return out + [pytest.param("relu", True, ROUND, id="relu-readout-round")]


@pytest.mark.parametrize("act,readout,form", _a_cases(A_FORMS))
def test_the_kicked_rows_have_their_teeth_in_the_gpu_records(act, readout, form):
    got = _a_run(act, readout, form)
    _finite(got["states"] + ([got["outs"]] if readout else []), f"{act} {readout} {_id(form)}")
    lo, hi, rise, fall = sc.a_teeth(got["states"], act)
    print(f"[scale swings A] {act}, read-out {readout}, {_id(form)} ({got['step']}): row maxima 2^{np.log2(lo):.1f} .. 2^{np.log2(hi):.1f}, "
          f"per tile, step and layer a rise of 2^{np.log2(rise):.1f} and a fall of 2^{np.log2(fall):.1f} at least")


def test_every_form_of_part_a_ran_its_own_kernel():
    ran = {_id(f): _a_run("relu", True, f)["step"] for f in A_FORMS + [ROUND]}
    print(f"[scale swings A: step kernels] {ran}")
    # injected noise keeps the default tuning on the in-place kernel (use_unified)
    for f in ("default", "ws=2", "ws=2,no_lean=1"):
        assert ran[f].startswith(WS2_KERNEL) and "round schedule" not in ran[f], (f, ran[f])
    assert ran["ws=0"] == BARRIER_KERNEL, ran["ws=0"]
    assert _lw(ran["ws=4"]), ran["ws=4"]
    assert ran[ROUND].startswith(WS2_ANY) and "round schedule" in ran[ROUND], ran[ROUND]
    for (a, r) in NET:
        for f in A_FORMS:
            assert _a_run(a, r, f)["step"].split(" [")[0] == ran[_id(f)].split(" [")[0], (a, r, f)


def _a_bitwise_cases():
    out = []
    for (a, r), i in zip(NET, NET_IDS):
        for f in A_LDS_FORMS + ([] if r else ["ws=4"]):
            out.append(pytest.param(a, r, f, id=f"{i}-{_id(f)}"))
    return out + [pytest.param("relu", True, ROUND, id="relu-readout-round")]


@pytest.mark.parametrize("act,readout,form", _a_bitwise_cases())
def test_every_form_equals_the_barrier_kernel_when_rows_jump(act, readout, form):
    """1. bitwise against the barrier kernel (the round-schedule case: against the barrier kernel on the same batch)."""
    got = _a_run(act, readout, form)
    want = _a_round_barrier() if form == ROUND else _a_run(act, readout, "ws=0")
    for key in ("states", "flat_states"):
        for l, (g, w) in enumerate(zip(got[key], want[key])):
            assert np.array_equal(g, w), f"{act} {readout} {_id(form)}: {key} of layer {l + 1} differ from the row scan's in {np.count_nonzero(g != w)} elements, first at step {int(np.argwhere(g != w)[0][0])}"
    if readout:
        assert np.array_equal(got["outs"], want["outs"]) and np.array_equal(got["flat_outs"], want["flat_outs"]), f"{act} {_id(form)}: recorded outputs differ"


@functools.lru_cache(maxsize=None)
def _a_round_barrier():
    """The barrier kernel on the round-schedule case's batch."""
    batch = _a_batch(ROUND)
    case = sc.a_case("relu", True, batch)
    W, b, X0, inputs, target = sc.a_data("relu", True, batch)
    eng = make_engine(case, "ws=0", W=W, b=b, inputs=inputs, target=target)
    try:
        states, outs, step = _a_call(eng, case, X0, sc.a_kicks(batch))
        flat_states, flat_outs, _ = _a_call(eng, case, X0, sc.a_kicks(batch, flat=sc.A_FLAT))
    finally:
        eng.close()
    assert step == BARRIER_KERNEL, step
    return dict(states=states, outs=outs, step=step, flat_states=flat_states, flat_outs=flat_outs)


@pytest.mark.parametrize("act,readout,form", _a_cases(A_FORMS, [n for n in NET if n[1]], [i for n, i in zip(NET, NET_IDS) if n[1]]))
def test_recorded_outputs_of_jumping_rows_against_fp64(act, readout, form):
    """2. the read-out's forward GEMM, sharply."""
    got = _a_run(act, readout, form)
    W, b, _, _, _ = sc.a_data(act, readout, _a_batch(form))
    worst = sc.outputs_vs_fp64(W, b, act, got["states"][-1][:-1], got["outs"])
    _hold(f"scale swings A: outputs vs fp64 ({_id(form)})", f"{act}: o[t] / sum|terms|", worst, sc.out_bound(sc.SIZES[-1]))
    assert worst > 0


@pytest.mark.parametrize("act,readout,form", _a_cases(A_FORMS))
def test_every_step_of_jumping_rows_against_fp64(act, readout, form):
    """3. every step, grossly: no precision test (see the module docstring); it sees Inf, NaN and a scale off by a power of two."""
    got = _a_run(act, readout, form)
    batch = _a_batch(form)
    W, b, _, inputs, target = sc.a_data(act, readout, batch)
    case = sc.a_case(act, readout, batch)
    for key, flat in (("states", None), ("flat_states", sc.A_FLAT)):
        _finite(got[key], f"{act} {readout} {_id(form)} {key}")
        kicks = sc.a_kicks(batch, flat=flat)
        worst = sc.steps_vs_fp64(case, W, b, inputs, target, got[key], lambda t: [k[t] for k in kicks])
        _hold(f"scale swings A: steps vs fp64 ({_id(form)})", f"{act}{'' if readout else ', no read-out'}: x[t+1] / sum|terms|", worst, sc.STEP_RTOL, key)


@pytest.mark.parametrize("act,readout,form", _a_cases(A_FORMS))
def test_a_constant_scale_chain_changes_no_other_chain(act, readout, form):
    """4. every other chain keeps its bits."""
    got = _a_run(act, readout, form)
    others = np.arange(_a_batch(form)) != sc.A_FLAT
    for l, (a, f) in enumerate(zip(got["states"], got["flat_states"])):
        assert np.array_equal(a[:, others], f[:, others]), f"{act} {readout} {_id(form)}: layer {l + 1} of another chain changed"
        assert not np.array_equal(a[:, sc.A_FLAT], f[:, sc.A_FLAT])
    if readout:
        assert np.array_equal(got["outs"][:, others], got["flat_outs"][:, others]), f"{act} {_id(form)}: a recorded output of another chain changed"


# ================================================================================================================================
# PART B
def _b_call(eng, regime, case, X0, slices):
    from montecarlopredictivecoding_amd import _lib as L
    dev = torch.device("cuda", 0)
    T = sc.B_T
    eng.load_state([_t(x) for x in X0])
    rec = [torch.full((T, sc.B, n), float("nan"), device=dev) for n in sc.SIZES]
    rec_o = torch.full((T, sc.B, sc.N_OUT), float("nan"), device=dev)
    steps, t = [], 0
    for n_steps in slices:
        if regime == "adam":
            how = dict(xopt=L.XOPT_ADAM, lr=sc.ADAM_LR, adam_step0=t, noise_mode=L.NOISE_NONE)
        else:
            how = dict(xopt=L.XOPT_SGD, lr=1.0, noise_mode=L.NOISE_PHILOX, noise_var=sc.B_NOISE_VAR, seed=sc.B_SEED, step_base=0, chain_base=0)
        eng.run(T, t_begin=t, n_steps=n_steps, rec_begin=0, rec_stride=1, rec_count=T, rec_x=True, rec_x_bufs=rec, rec_out=True, rec_out_buf=rec_o,
                **how, **loss_kw(case))
        eng.sync_check()
        steps.append(eng.last_step_kernel())
        t += n_steps
    assert t == T
    return sc.states_of([r.cpu().numpy() for r in rec], final_states(eng, case)), rec_o.cpu().numpy(), steps


@functools.lru_cache(maxsize=None)
def _b_run(regime, form):
    case = sc.b_case(regime)
    W, b, X0, _, target = sc.b_data(regime)
    eng = make_engine(case, form or "", W=W, b=b, inputs=None, target=target)
    try:
        states, outs, steps = _b_call(eng, regime, case, X0, (sc.B_T,))
        cut_states, cut_outs, cut_steps = _b_call(eng, regime, case, X0, (sc.B_T // 2, sc.B_T - sc.B_T // 2))
    finally:
        eng.close()
    return dict(states=states, outs=outs, step=steps[0], cut_states=cut_states, cut_outs=cut_outs, cut_steps=cut_steps)


B_CASES = [pytest.param(r, f, id=f"{r}-{_id(f)}") for r in sc.B_REGIMES for f in B_FORMS]


@pytest.mark.parametrize("regime,form", B_CASES)
def test_the_growing_and_decaying_rows_have_their_teeth_in_the_gpu_records(regime, form):
    got = _b_run(regime, form)
    _finite(got["states"] + [got["outs"]], f"{regime} {_id(form)}")
    lo, hi, move = sc.b_teeth(got["states"], regime)
    print(f"[scale swings B] {regime}, {_id(form)} ({got['step']}): row maxima 2^{np.log2(lo):.1f} .. 2^{np.log2(hi):.1f}, smallest move asserted 2^{np.log2(move):.2f}")


def test_every_form_of_part_b_ran_its_own_kernel():
    ran = {(r, _id(f)): _b_run(r, f) for r in sc.B_REGIMES for f in B_FORMS}
    print(f"[scale swings B: step kernels] { {k: v['step'] for k, v in ran.items()} }")
    for r in sc.B_REGIMES:
        for f in ("default", "ws=3"):
            assert ran[(r, f)]["step"].startswith(U_KERNEL), (r, f, ran[(r, f)]["step"])
        assert ran[(r, "ws=0")]["step"] == BARRIER_KERNEL
        step = ran[(r, "ws=2")]["step"]
        assert step.startswith(WS2_KERNEL), (r, step)
        # the all-ReLU regimes take a specialised instantiation of the in-place kernel, and nothing else; the identity net has none
        want = {"growth": None, "growth_relu": "hot", "decay": "hot", "adam": "map"}[r]
        if want is None:
            assert SPEC not in step, (r, step)
        else:
            assert step.endswith(f"[{SPEC}: {want}]"), (r, step)
        for f in B_FORMS:
            assert set(ran[(r, _id(f))]["cut_steps"]) == {ran[(r, _id(f))]["step"]}, (r, f, ran[(r, _id(f))]["cut_steps"])


@pytest.mark.parametrize("regime,form", [p for p in B_CASES if p.values[1] != "ws=0"])
def test_row_words_equal_row_scans_when_rows_grow_or_decay(regime, form):
    """1. bitwise against the barrier kernel: on decay the only assertion with teeth."""
    got, want = _b_run(regime, form), _b_run(regime, "ws=0")
    for l, (g, w) in enumerate(zip(got["states"], want["states"])):
        assert np.array_equal(g, w), f"{regime} {_id(form)}: layer {l + 1} differs from the row scan's in {np.count_nonzero(g != w)} elements, first at step {int(np.argwhere(g != w)[0][0])}"
    assert np.array_equal(got["outs"], want["outs"]), f"{regime} {_id(form)}: recorded outputs differ"


@pytest.mark.parametrize("regime,form", B_CASES)
def test_every_step_of_growing_and_decaying_rows_against_fp64(regime, form):
    """3. every step against fp64: sharp on growth, where the GEMM terms ARE x_{t+1} (a word one step stale puts values 2^4 above fp16's
    range); gross on decay and under Adam."""
    got = _b_run(regime, form)
    W, b, _, _, target = sc.b_data(regime)
    case = sc.b_case(regime)
    _finite(got["states"], f"{regime} {_id(form)}")
    if regime == "adam":
        _hold(f"scale swings B: steps vs fp64 ({_id(form)})", "adam: x[t+1] error / bound", sc.adam_steps_vs_fp64(case, W, b, target, got["states"]))
    else:
        worst = sc.steps_vs_fp64(case, W, b, None, target, got["states"], sc.b_kicks_of(regime))
        _hold(f"scale swings B: steps vs fp64 ({_id(form)})", f"{regime}: x[t+1] / sum|terms|", worst, sc.STEP_RTOL)
        assert worst > 0


@pytest.mark.parametrize("regime,form", B_CASES)
def test_a_call_cut_mid_way_is_bitwise_the_single_run(regime, form):
    got = _b_run(regime, form)
    for l, (g, w) in enumerate(zip(got["cut_states"], got["states"])):
        assert np.array_equal(g, w), f"{regime} {_id(form)}: layer {l + 1} of the cut call differs in {np.count_nonzero(g != w)} elements, first at step {int(np.argwhere(g != w)[0][0])}"
    assert np.array_equal(got["cut_outs"], got["outs"]), f"{regime} {_id(form)}: recorded outputs of the cut call differ"


# ================================================================================================================================
# PART C
def _c_ran_the_form(step, form, updates_x):
    if form == "ws=4":
        return _lw(step)
    if form == "ws=0":
        return step == BARRIER_KERNEL
    if form == "ws=3" and updates_x:
        return step.startswith(U_KERNEL)
    return step.startswith(WS2_KERNEL)            # (a gradients-only run is never served by the unified-wave kernel: use_unified)


@functools.lru_cache(maxsize=None)
def _c_engine_runs(form):
    """One engine per form (the parameters that differ between the cases are bound again): the one-step case in three orders, the two-step
    case in two."""
    from montecarlopredictivecoding_amd import _lib as L
    case = sc.c_case()
    out = {}
    W, b, X0, _, target = sc.c_data(sc.C_ORDERS[0])[:5]
    eng = make_engine(case, form, W=W, b=b, inputs=None, target=target)
    try:
        for order in sc.C_ORDERS:
            W, b, X0, _, target = sc.c_data(order)[:5]
            eng.bind_params([_t(w) for w in W], [_t(v) for v in b])
            eng.bind_target(_t(target))
            eng.load_state([_t(x) for x in X0])
            res = eng.run(1, update_x=False, xopt=L.XOPT_SGD, lr=1.0, **loss_kw(case))
            eng.sync_check()
            out[("one", order)] = dict(xgrad=[g.cpu().numpy() for g in res.xgrad], step=eng.last_step_kernel())
            # the same back-projection through an UPDATE step (lr = 1 from x = 0 with zero biases: x_1 = -back), which the lean
            # epilogues serve: the chunks' exponents then come from the ring slots' words, and ws=3 runs the unified-wave kernel
            eng.load_state([_t(x) for x in X0])
            eng.run(1, xopt=L.XOPT_SGD, lr=1.0, noise_mode=L.NOISE_NONE, **loss_kw(case))
            eng.sync_check()
            out[("update", order)] = dict(xgrad=[-x for x in final_states(eng, case)], step=eng.last_step_kernel())
        for order in sc.C2_ORDERS:
            W, b, X0, _, target = sc.c2_data(order)
            eng.bind_params([_t(w) for w in W], [_t(v) for v in b])
            eng.bind_target(_t(target))
            eng.load_state([_t(x) for x in X0])
            res = eng.run(sc.C2_T, xopt=L.XOPT_SGD, lr=1.0, noise_mode=L.NOISE_NONE, rec_begin=0, rec_stride=1, rec_count=sc.C2_T, rec_x=True,
                          rec_out=True, **loss_kw(case))
            eng.sync_check()
            out[("two", order)] = dict(states=sc.states_of([r.cpu().numpy() for r in res.rec_x], final_states(eng, case)),
                                       outs=res.rec_out.cpu().numpy(), step=eng.last_step_kernel())
    finally:
        eng.close()
    return out


@pytest.mark.parametrize("form", C_FORMS)
@pytest.mark.parametrize("order", sc.C_ORDERS)
@pytest.mark.parametrize("how", ["one", "update"], ids=["gradients_only", "update_step"])
def test_chunks_of_a_gaussian_readout_error_at_very_different_scales(how, order, form):
    """A gradients-only step keeps the generic epilogues, whose GEMM waves scan every chunk's rows; the update step is served by the lean
    epilogues and their ring-slot words (csrc/mcpc_steps_ws2_body.inc: `lean`, `rowexp`).  The same bound either way."""
    got = _c_engine_runs(form)[(how, order)]
    assert _c_ran_the_form(got["step"], form, how == "update"), (form, got["step"])
    _finite(got["xgrad"], f"{order} {form}")
    assert not got["xgrad"][0].any() and not got["xgrad"][1].any()          # (zero parameters below the read-out)
    want, terms, bound = sc.c_reference(order)
    frac = np.abs(got["xgrad"][-1].astype(np.float64) - want) / terms / bound
    sharp = bound < 1e-5                                                      # the chunk that holds the row's maximum
    group = f"scale swings C: back-projection vs fp64 ({form})"
    _hold(group, f"{order}, {how}: chunk of the maximum, error / bound", float(frac[sharp].max()))
    _hold(group, f"{order}, {how}: every chunk, error / bound", float(frac.max()))
    assert frac[sharp].max() > 0


@pytest.mark.parametrize("form", C_FORMS)
@pytest.mark.parametrize("order", sc.C2_ORDERS)
def test_two_steps_with_the_chunks_in_opposite_orders(order, form):
    """The ring slots' generations across a step boundary: the slot that held the largest chunk of step 0 takes a larger one at step 1, or
    (falling) one 2^11 smaller.  Against fp64 as in assertion 3 of Part A (gross: it sees an overflow, not lost bits), the chunks' moves
    asserted from the recorded outputs."""
    got = _c_engine_runs(form)[("two", order)]
    assert _c_ran_the_form(got["step"], form, True), (form, got["step"])
    _finite(got["states"] + [got["outs"]], f"{order} {form}")
    s = sc.c2_teeth(got["outs"], order)
    print(f"[scale swings C] two steps, {order}, {form} ({got['step']}): chunk scales of e_o 2^{np.round(s[0], 1).tolist()} then 2^{np.round(s[1], 1).tolist()}")
    W, b, _, _, target = sc.c2_data(order)
    worst = sc.steps_vs_fp64(sc.c_case(), W, b, None, target, got["states"], lambda t: None)
    _hold(f"scale swings C: two steps vs fp64 ({form})", f"{order}: x[t+1] / sum|terms|", worst, sc.STEP_RTOL)
    assert worst > 0


@pytest.mark.parametrize("case", [("update", o) for o in sc.C_ORDERS] + [("two", o) for o in sc.C2_ORDERS], ids=lambda c: f"{c[0]}-{c[1]}".replace(" ", "_"))
def test_ring_slot_words_equal_row_scans_of_the_same_chunks(case):
    """ws=2 takes a chunk's exponent from its ring slot's word, ws=2,no_lean=1 scans the chunk: the same kernel, the same cut of the
    read-out, the same exponents -- the same bits.  On the falling case this is the assertion with teeth: a word left over from the step
    before is too large there, which costs 11 of 22 bits and nothing that the gross fp64 bound sees."""
    lean, scans = _c_engine_runs("ws=2")[case], _c_engine_runs("ws=2,no_lean=1")[case]
    assert lean["step"] == scans["step"] and lean["step"].startswith(WS2_KERNEL), (lean["step"], scans["step"])
    keys = ["xgrad"] if case[0] == "update" else ["states"]
    for key in keys:
        for l, (g, w) in enumerate(zip(lean[key], scans[key])):
            assert np.array_equal(g, w), f"{case}: layer {l + 1} differs between words and scans in {np.count_nonzero(g != w)} elements"
    if case[0] == "two":
        assert np.array_equal(lean["outs"], scans["outs"]), f"{case}: recorded outputs differ between words and scans"

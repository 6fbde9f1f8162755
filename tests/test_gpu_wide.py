"""The layer-wise step kernels (csrc/mcpc_steps_lw.h: mcpc_lw_fwd_kernel + mcpc_lw_bwd_kernel) on networks the LDS plans reject, and
against the LDS-resident kernels where both run.

Tolerances are the contract the engine tests state (tests/test_gpu_engine.py): energies rtol 1e-6, states and
records 1e-5 absolute, gradient bucket rtol 2e-4 + 2e-5 max|want|.  Every case of tests/wide_cases.py is a parity case: the oracle's own
fp32 rounding stays a decade inside these bounds (tests/test_wide_cases.py)."""
import numpy as np
import pytest
import torch

from oracle import mcpc_oracle as mo
from oracle.cases import make_case_inputs
from tests import parity_log
from tests import wide_cases as wc

pytestmark = pytest.mark.gpu

LW = "mcpc_lw_fwd_kernel"
MCPC_EINVAL, MCPC_ENOMEM = -1, -3          # include/mcpc.h
E_RTOL, X_ATOL = 1e-6, 1e-5


def _dev():
    return torch.device("cuda", 0)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def make_engine(case, tuning, batch=None, W=None, b=None, inputs=None, target=None):
    from montecarlopredictivecoding_amd.engine import Engine
    batch = case["B"] if batch is None else batch
    eng = Engine(case["sizes"], [wc.ACT[a] for a in case["acts"]], case["n_in"], case["n_out"], batch, device=_dev(), ecoef=case["ecoef"],
                 tuning=tuning)
    eng.bind_params([_t(w) for w in W], [None if x is None else _t(x) for x in b])
    eng.bind_inputs(None if inputs is None or not np.any(inputs) else _t(inputs))
    if target is not None:
        eng.bind_target(_t(target))
    return eng


def loss_kw(case, mask_start=0):
    from montecarlopredictivecoding_amd import _lib as L
    kind = {"none": L.LOSS_NONE, "gaussian": L.LOSS_GAUSSIAN, "bernoulli": L.LOSS_BERNOULLI}[case["loss"]]
    return dict(loss_kind=kind, loss_var=case["var"], mask_start=mask_start)


def flat_grads(eng):
    return eng.read_param_grads_flat().cpu().numpy()


def final_states(eng, case, batch=None):
    batch = case["B"] if batch is None else batch
    xs = [torch.empty(batch, n, device=_dev()) for n in case["sizes"]]
    eng.store_state(xs)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in xs]


def check_energies(group, en, ref, L_):
    parity_log.close(group, "overall[t]", en[:, -1], ref.overall, rtol=E_RTOL, atol=1e-6)
    parity_log.close(group, "loss[t]", en[:, 0], ref.loss, rtol=E_RTOL, atol=1e-6)
    parity_log.close(group, "layer energies[t]", en[:, 1:1 + L_], ref.layer_energy, rtol=E_RTOL, atol=1e-6)


def check_bucket(group, got, ref):
    want = wc.bucket(ref)
    parity_log.close(group, "gradient bucket", got, want, rtol=2e-4, atol=2e-5 * float(np.abs(want).max()))


def sgd_kick_call(eng, case, T=None, acc=(0, 0), seed=None, chain_base=0, t_begin=0, n_steps=None, energies_out=None, acc_reset=True,
                  energy=True, **kw):
    from montecarlopredictivecoding_amd import _lib as L
    T = case["T"] if T is None else T
    return eng.run(T, t_begin=t_begin, n_steps=n_steps, xopt=L.XOPT_SGD, lr=wc.LR, noise_mode=L.NOISE_PHILOX, noise_var=wc.NOISE_VAR,
                   seed=case["seed"] if seed is None else seed, step_base=0, chain_base=chain_base, acc_begin=acc[0], acc_end=acc[1],
                   acc_reset=acc_reset, energy_mode=L.ENERGY_ALL if energy else L.ENERGY_NONE, energies_out=energies_out,
                   **dict(loss_kw(case), **kw))


# ---- 1. wide shapes against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(wc.CASES))
def test_wide_shapes_match_the_oracle(name):
    case = wc.CASES[name]
    data = make_case_inputs(case)
    W, b, X0, inputs, target = data
    T, L_ = case["T"], len(case["sizes"])
    rec = [2, T - 1]
    ref = wc.oracle_run(case, acc=range(3, T), record_at=rec, inputs_data=data)
    eng = make_engine(case, "wide=1", W=W, b=b, inputs=inputs, target=target)
    assert LW in eng.query()["step_kernel"] and "mcpc_lw_bwd_kernel" in eng.query()["step_kernel"]
    eng.load_state([_t(x) for x in X0])
    res = sgd_kick_call(eng, case, acc=(3, T), rec_begin=2, rec_stride=T - 3, rec_count=2, rec_x=True, rec_out=True)
    xs = final_states(eng, case)
    assert LW in eng.last_step_kernel() and "mcpc_lw_bwd_kernel" in eng.last_step_kernel()
    group = "layer-wise kernels vs oracle: " + name
    check_energies(group, res.energies.cpu().numpy(), ref, L_)
    for l in range(L_):
        parity_log.close(group, "x final", xs[l], ref.xs[l], rtol=0, atol=X_ATOL)
        for k, t in enumerate(rec):
            parity_log.close(group, "x[t] (records)", res.rec_x[l][k].cpu().numpy(), ref.rec_xs[t][l], rtol=0, atol=X_ATOL)
    if case["n_out"]:
        for k, t in enumerate(rec):
            parity_log.close(group, "outputs[t]", res.rec_out[k].cpu().numpy(), ref.rec_out[t], rtol=0, atol=3 * X_ATOL)
    check_bucket(group, flat_grads(eng), ref)
    eng.close()


# ---- 2. every mode on one wide shape -----------------------------------------------------------------------------------------------------
def _r384(**kw):
    return dict(wc.CASES["r384"], **kw)


def test_adam_on_x_and_its_moments():
    """Adam on x without noise, the MAP warm-up.  The oracle does not return its moments: they are replayed here from its recorded states
    with its own forward / x_grads and the recurrences of mcpc_oracle.run, in fp32.  Bound of the moments: they are convex combinations of
    gradients (m) and of squared gradients (v) whose inputs agree to the state contract, so the same 1e-5 absolute holds for m, and
    2 |g| 1e-5 <= 1e-4 relative + 1e-5 for v."""
    from montecarlopredictivecoding_amd import _lib as L
    case = _r384()
    data = make_case_inputs(case)
    W, b, X0, inputs, target = data
    T, L_ = case["T"], 2
    net, ls = wc.net_spec(case, W, b), wc.loss_spec(case, target)
    xo = mo.XOpt(mo.OPT_ADAM, 0.02)
    ref = mo.run(net, inputs, X0, ls, xo, T, accumulate_p_at=list(range(T)), record_at=range(T))
    m = [np.zeros_like(x) for x in X0]
    v = [np.zeros_like(x) for x in X0]
    f32 = np.float32
    for t in range(T):
        xs = ref.rec_xs[t]
        gs = mo.x_grads(net, xs, mo.forward(net, inputs, xs, ls))
        for l in range(L_):
            m[l] = m[l] + (gs[l] - m[l]) * f32(1.0 - xo.beta1)
            v[l] = v[l] * f32(xo.beta2) + (f32(1.0 - xo.beta2) * gs[l]) * gs[l]
    eng = make_engine(case, "wide=1", W=W, b=b, inputs=inputs, target=target)
    eng.load_state([_t(x) for x in X0])
    res = eng.run(T, xopt=L.XOPT_ADAM, lr=0.02, acc_begin=0, acc_end=T, energy_mode=L.ENERGY_ALL, **loss_kw(case))
    xs = final_states(eng, case)
    ms = [torch.empty(case["B"], n, device=_dev()) for n in case["sizes"]]
    vs = [torch.empty(case["B"], n, device=_dev()) for n in case["sizes"]]
    eng.store_adam_state(ms, vs)
    torch.cuda.synchronize()
    group = "layer-wise kernels vs oracle: Adam on x"
    check_energies(group, res.energies.cpu().numpy(), ref, L_)
    for l in range(L_):
        parity_log.close(group, "x final", xs[l], ref.xs[l], rtol=0, atol=X_ATOL)
        parity_log.close(group, "exp_avg", ms[l].cpu().numpy(), m[l], rtol=0, atol=1e-5)
        parity_log.close(group, "exp_avg_sq", vs[l].cpu().numpy(), v[l], rtol=1e-4, atol=1e-5)
    check_bucket(group, flat_grads(eng), ref)
    eng.close()


@pytest.mark.parametrize("variant", ["external_noise", "gaussian_mask", "bernoulli_mask", "bernoulli_wild_targets", "no_bias", "ecoef"])
def test_modes_on_one_wide_shape(variant):
    from montecarlopredictivecoding_amd import _lib as L
    case = _r384()
    mask = 0
    if variant in ("bernoulli_mask", "bernoulli_wild_targets"):
        case["loss"] = "bernoulli"
    if variant == "no_bias":
        case["no_bias"] = [1]
    if variant == "ecoef":
        case["ecoef"] = [0.5, 2.0]
    if variant.endswith("_mask"):
        mask = mo.mask_start_from_perc(case["n_out"], 0.4)
    data = make_case_inputs(case)
    W, b, X0, inputs, target = data
    if variant == "bernoulli_wild_targets":
        # BCEWithLogits takes any target: -1.5 / 2.5, outside [0, 1] and outside [-1, 2].  (Not wilder: with -2.5 / 4.5 the loss of this
        # net falls through zero inside the 20 steps, and a relative bound on a sum that cancels is no parity statement -- there the
        # oracle's own fp32 run misses it too.  Here the loss stays above 1400 and the oracle's fp32 run is within 4e-8 of its fp64 run.)
        target = (target * 4.0 - 1.5).astype(np.float32)
    T, L_ = case["T"], 2
    net, ls = wc.net_spec(case, W, b), wc.loss_spec(case, target, mask)
    noise = wc.philox_noise(case, seed=77)
    ref = mo.run(net, inputs, X0, ls, mo.XOpt(mo.OPT_SGD, wc.LR), T, noise=noise, noise_var=wc.NOISE_VAR, accumulate_p_at=list(range(2, T)))
    eng = make_engine(case, "wide=1", W=W, b=b, inputs=inputs, target=target)
    eng.load_state([_t(x) for x in X0])
    if variant == "external_noise":
        ext = [_t(np.stack([noise(t, l) for t in range(T)])) for l in range(L_)]
        res = eng.run(T, xopt=L.XOPT_SGD, lr=wc.LR, noise_mode=L.NOISE_EXTERNAL, noise_var=wc.NOISE_VAR, ext_noise=ext, acc_begin=2, acc_end=T,
                      energy_mode=L.ENERGY_ALL, **loss_kw(case, mask))
    else:
        res = sgd_kick_call(eng, case, acc=(2, T), seed=77, mask_start=mask)
    xs = final_states(eng, case)
    group = "layer-wise kernels vs oracle: " + variant
    check_energies(group, res.energies.cpu().numpy(), ref, L_)
    for l in range(L_):
        parity_log.close(group, "x final", xs[l], ref.xs[l], rtol=0, atol=X_ATOL)
    check_bucket(group, flat_grads(eng), ref)
    eng.close()


def test_gradients_only_and_last_energy():
    from montecarlopredictivecoding_amd import _lib as L
    case = _r384()
    data = make_case_inputs(case)
    W, b, X0, inputs, target = data
    net, ls = wc.net_spec(case, W, b), wc.loss_spec(case, target)
    fw = mo.forward(net, inputs, X0, ls)
    gs = mo.x_grads(net, X0, fw)
    eng = make_engine(case, "wide=1", W=W, b=b, inputs=inputs, target=target)
    eng.load_state([_t(x) for x in X0])
    res = eng.run(1, update_x=False, xopt=L.XOPT_SGD, lr=wc.LR, energy_mode=L.ENERGY_ALL, **loss_kw(case))
    xs = final_states(eng, case)
    group = "layer-wise kernels vs oracle: update_x=0"
    for l in range(2):
        assert np.array_equal(xs[l], X0[l])
        parity_log.close(group, "xgrad", res.xgrad[l].cpu().numpy(), gs[l], rtol=0, atol=X_ATOL)
    en = res.energies.cpu().numpy()
    parity_log.close(group, "overall", en[0, -1], sum(fw["energies"]) + fw["loss"], rtol=E_RTOL)
    # energy_mode LAST: one row, the last step's
    T = case["T"]
    ref = wc.oracle_run(case, inputs_data=data)
    eng.load_state([_t(x) for x in X0])
    res = eng.run(T, xopt=L.XOPT_SGD, lr=wc.LR, noise_mode=L.NOISE_PHILOX, noise_var=wc.NOISE_VAR, seed=case["seed"], step_base=0,
                  energy_mode=L.ENERGY_LAST, **loss_kw(case))
    en = res.energies.cpu().numpy()
    assert en.shape[0] == 1
    parity_log.close("layer-wise kernels vs oracle: energy LAST", "overall", en[0, -1], ref.overall[-1], rtol=E_RTOL)
    parity_log.close("layer-wise kernels vs oracle: energy LAST", "loss", en[0, 0], ref.loss[-1], rtol=E_RTOL)
    eng.close()


def test_one_chain_one_step():
    case = _r384(B=1, T=1)
    data = make_case_inputs(case)
    W, b, X0, inputs, target = data
    ref = wc.oracle_run(case, inputs_data=data)
    eng = make_engine(case, "wide=1", W=W, b=b, inputs=inputs, target=target)
    eng.load_state([_t(x) for x in X0])
    res = sgd_kick_call(eng, case, acc=(0, 1))
    xs = final_states(eng, case)
    group = "layer-wise kernels vs oracle: one chain, T = 1"
    check_energies(group, res.energies.cpu().numpy(), ref, 2)
    for l in range(2):
        parity_log.close(group, "x final", xs[l], ref.xs[l], rtol=0, atol=X_ATOL)
    check_bucket(group, flat_grads(eng), ref)
    eng.close()


def test_many_chain_tiles_with_a_ragged_last_one():
    """3000 chains of 30-512-512 -> 784 for T = 6: 47 chain tiles of 64, the last one holds 56 chains."""
    case = dict(wc.CASES["b512"], B=3000, T=6)
    data = make_case_inputs(case)
    W, b, X0, inputs, target = data
    ref = wc.oracle_run(case, acc=range(1, 6), inputs_data=data)
    eng = make_engine(case, "wide=1", W=W, b=b, inputs=inputs, target=target)
    eng.load_state([_t(x) for x in X0])
    res = sgd_kick_call(eng, case, acc=(1, 6))
    xs = final_states(eng, case)
    group = "layer-wise kernels vs oracle: 3000 chains"
    check_energies(group, res.energies.cpu().numpy(), ref, 3)
    for l in range(3):
        parity_log.close(group, "x final", xs[l], ref.xs[l], rtol=0, atol=X_ATOL)
    check_bucket(group, flat_grads(eng), ref)
    eng.close()


# ---- 3. the same results as the forms that exist -------------------------------------------------------------------------------------------
BOTH = {
    "cfgM": dict(n_in=10, sizes=[30, 256, 256, 256], n_out=784, act="relu", loss="bernoulli", B=640, seed=201),
    "mcpc_ml": dict(n_in=10, sizes=[20, 128, 128], n_out=784, act="tanh", loss="gaussian", B=256, seed=202),
    "no_readout": dict(n_in=10, sizes=[16, 500], n_out=0, act="tanh", loss="none", B=96, seed=203),
}


@pytest.mark.parametrize("xopt", ["sgd_kick", "adam"])
@pytest.mark.parametrize("net", sorted(BOTH))
def test_layerwise_agrees_with_the_lds_resident_kernels(net, xopt):
    """60 steps on nets that fit both, ws=4 against the default tuning and against ws=0: states and records within the state contract of
    each other, energies rtol 2e-6 (two paths, each within 1e-6 of the truth), bucket at the bucket tolerance.  Bitwise: the forward GEMMs
    and the latent back-projections use the same fragments, row exponents and k order as the LDS kernels, so on the net WITHOUT a read-out
    states and records are asserted array_equal.  With a read-out its back-projection is ONE contraction over the whole read-out under the
    row's own exponent here, where the LDS kernels add chunks (rescaled sums under a Gaussian loss, a constant exponent under a bounded
    Bernoulli target): equal as long as no piece of an operand leaves fp16's normal range -- observed equal on both nets of this test on an
    MI355X, asserted at the contract only.  Energies and Hebbian sums are added in another order: tolerances."""
    from montecarlopredictivecoding_amd import _lib as L
    s = BOTH[net]
    case = wc._case(net, s["n_in"], s["sizes"], s["n_out"], s["act"], s["loss"], 60, s["seed"], B=s["B"])
    W, b, X0, inputs, target = make_case_inputs(case)
    T, L_ = 60, len(case["sizes"])
    out = {}
    for tuning in ("ws=4", "", "ws=0"):
        eng = make_engine(case, tuning, W=W, b=b, inputs=inputs, target=target)
        assert (LW in eng.query()["step_kernel"]) == (tuning == "ws=4")
        eng.load_state([_t(x) for x in X0])
        if xopt == "adam":
            res = eng.run(T, xopt=L.XOPT_ADAM, lr=0.02, acc_begin=10, acc_end=T, energy_mode=L.ENERGY_ALL, rec_begin=30, rec_stride=1, rec_count=1,
                          rec_x=True, rec_out=True, **loss_kw(case))
        else:
            res = sgd_kick_call(eng, case, acc=(10, T), rec_begin=30, rec_stride=1, rec_count=1, rec_x=True, rec_out=True)
        out[tuning] = (final_states(eng, case), res.energies.cpu().numpy(), flat_grads(eng), [r[0].cpu().numpy() for r in res.rec_x])
        eng.close()
    for other in ("", "ws=0"):
        group = "layer-wise kernels vs %s: %s, %s" % ("default tuning" if other == "" else "barrier kernel", net, xopt)
        a, o = out["ws=4"], out[other]
        for l in range(L_):
            parity_log.close(group, "x final", a[0][l], o[0][l], rtol=0, atol=X_ATOL)
            parity_log.close(group, "x[30] (record)", a[3][l], o[3][l], rtol=0, atol=X_ATOL)
            if net == "no_readout":
                assert np.array_equal(a[0][l], o[0][l]) and np.array_equal(a[3][l], o[3][l]), (group, l)
        parity_log.close(group, "energies", a[1], o[1], rtol=2e-6, atol=1e-6)
        parity_log.close(group, "gradient bucket", a[2], o[2], rtol=2e-4, atol=2e-5 * float(np.abs(o[2]).max()))


# ---- 4. chain independence, bitwise -------------------------------------------------------------------------------------------------------
def test_chains_are_independent_bitwise():
    case = dict(wc.CASES["k200"], B=70)
    W, b, X0, inputs, target = make_case_inputs(case)
    T = case["T"]

    def part(lo, hi):
        eng = make_engine(case, "ws=4", batch=hi - lo, W=W, b=b, inputs=inputs[lo:hi], target=target[lo:hi])
        eng.load_state([_t(x[lo:hi]) for x in X0])
        res = sgd_kick_call(eng, case, chain_base=lo)
        xs = final_states(eng, case, batch=hi - lo)
        en = res.energies.cpu().numpy()
        eng.close()
        return xs, en

    whole, en = part(0, 70)
    first, _ = part(0, 16)
    a, ea = part(0, 40)
    c, ec = part(40, 70)
    for l in range(len(case["sizes"])):
        assert np.array_equal(whole[l][:16], first[l]), "chains 0..15 alone differ from the same chains among 70"
        assert np.array_equal(whole[l][:40], a[l]) and np.array_equal(whole[l][40:], c[l]), "two shards with chain_base differ from one engine"
    parity_log.close("layer-wise kernels: shards vs whole", "energies", ea + ec, en, rtol=2e-6, atol=1e-6)


# ---- 5. slicing is invisible --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xopt", ["sgd_kick", "adam"])
def test_random_slicing_of_a_call_is_invisible(xopt):
    from montecarlopredictivecoding_amd import _lib as L
    case = dict(wc.CASES["k200"], T=30)
    W, b, X0, inputs, target = make_case_inputs(case)
    T = 30
    rng = np.random.RandomState(5)
    cuts = [0] + sorted(rng.choice(np.arange(1, T), size=4, replace=False).tolist()) + [T]
    out = []
    for pieces in ([0, T], cuts):
        eng = make_engine(case, "ws=4", W=W, b=b, inputs=inputs, target=target)
        eng.load_state([_t(x) for x in X0])
        en = torch.zeros(T, L.ENERGY_COLS, dtype=torch.float64, device=_dev())
        for i, (t0, t1) in enumerate(zip(pieces[:-1], pieces[1:])):
            if xopt == "adam":
                eng.run(T, t_begin=t0, n_steps=t1 - t0, xopt=L.XOPT_ADAM, lr=0.02, adam_step0=t0, acc_begin=7, acc_end=23, acc_reset=(i == 0),
                        energy_mode=L.ENERGY_ALL, energies_out=en, **loss_kw(case))
            else:
                sgd_kick_call(eng, case, T=T, acc=(7, 23), t_begin=t0, n_steps=t1 - t0, energies_out=en, acc_reset=(i == 0))
        out.append((final_states(eng, case), en.cpu().numpy(), flat_grads(eng)))
        eng.close()
    (xa, ea, ga), (xb, eb, gb) = out
    for l in range(len(case["sizes"])):
        assert np.array_equal(xa[l], xb[l]), "states differ between one run and slices %r" % (cuts,)
    assert np.array_equal(ea, eb), "energies differ between one run and slices %r" % (cuts,)
    parity_log.close("layer-wise kernels: slices vs one run", "gradient bucket", gb, ga, rtol=2e-4, atol=2e-5 * float(np.abs(ga).max()))


# ---- 6. repeatability ---------------------------------------------------------------------------------------------------------------------
def test_a_learning_call_is_bitwise_repeatable():
    case = wc.CASES["ragged"]
    W, b, X0, inputs, target = make_case_inputs(case)
    T = case["T"]
    out = []
    for _ in range(2):
        eng = make_engine(case, "wide=1", W=W, b=b, inputs=inputs, target=target)
        eng.load_state([_t(x) for x in X0])
        res = sgd_kick_call(eng, case, acc=(2, T))
        out.append((final_states(eng, case), res.energies.cpu().numpy(), flat_grads(eng)))
        eng.close()
    for l in range(len(case["sizes"])):
        assert np.array_equal(out[0][0][l], out[1][0][l])
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])


# ---- 7. LDS content does not matter -------------------------------------------------------------------------------------------------------
def test_lds_content_does_not_matter():
    """Widths 33 and 200: k ranges of 48 and 208, both with a ragged last k-block."""
    from montecarlopredictivecoding_amd.engine import debug_poison_lds
    case = wc.CASES["k200"]
    data = make_case_inputs(case)
    W, b, X0, inputs, target = data
    T = case["T"]
    ref = wc.oracle_run(case, acc=range(2, T), inputs_data=data)
    out = []
    for word in (0x7fa00000, 0):
        eng = make_engine(case, "wide=1", W=W, b=b, inputs=inputs, target=target)
        eng.load_state([_t(x) for x in X0])
        torch.cuda.synchronize()
        debug_poison_lds(_dev(), word)
        res = sgd_kick_call(eng, case, acc=(2, T))
        out.append((final_states(eng, case), res.energies.cpu().numpy(), flat_grads(eng)))
        eng.close()
    for l in range(len(case["sizes"])):
        assert np.array_equal(out[0][0][l], out[1][0][l])
        parity_log.close("layer-wise kernels, poisoned LDS vs oracle", "x final", out[0][0][l], ref.xs[l], rtol=0, atol=X_ATOL)
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    check_energies("layer-wise kernels, poisoned LDS vs oracle", out[0][1], ref, len(case["sizes"]))
    check_bucket("layer-wise kernels, poisoned LDS vs oracle", out[0][2], ref)


# ---- 8. nothing changed for those who did not ask -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", wc.REJECTED)
def test_wide_shapes_are_still_rejected_without_a_key(name):
    from montecarlopredictivecoding_amd import _lib as L
    from montecarlopredictivecoding_amd.engine import Engine
    case = wc.CASES[name]
    with pytest.raises(L.MCPCError) as exc:
        Engine(case["sizes"], [wc.ACT[a] for a in case["acts"]], case["n_in"], case["n_out"], case["B"], device=_dev(), tuning="")
    assert exc.value.code == MCPC_ENOMEM, exc.value


def test_incompatible_knobs_are_an_error_of_their_own():
    from montecarlopredictivecoding_amd import _lib as L
    from montecarlopredictivecoding_amd.engine import Engine
    for tuning in ("ws=4,no_xl=1", "ws=4,no_lean=1", "ws=4,overlay16=1", "ws=4,rr=0", "ws=4,u_row=100"):
        with pytest.raises(L.MCPCError) as exc:
            Engine([32, 384], [2, 2], 10, 100, 8, device=_dev(), tuning=tuning)
        assert exc.value.code == MCPC_EINVAL, (tuning, exc.value)
    # wide=1 composes: a forced kernel whose plan does not fit falls to the layer-wise kernels, one that fits keeps its kernel
    for tuning in ("ws=0,wide=1", "ws=2,wide=1", "ws=3,wide=1", "no_xl=1,wide=1"):
        eng = Engine([32, 384], [2, 2], 10, 100, 8, device=_dev(), tuning=tuning)
        assert LW in eng.query()["step_kernel"], tuning
        eng.close()
    eng = Engine([30, 64, 64], [1, 1, 1], 30, 100, 48, device=_dev(), tuning="wide=1")
    assert LW not in eng.query()["step_kernel"]
    eng.close()

"""A chain's special values stay in that chain, on every step kernel form (Part 1), and the per-element functions of
csrc/mcpc_device.h at their edges (Part 2).

PART 1.  The cases of tests/special_value_cases.py: 40 chains of which ONE starts from a dead (all f(x) = 0), huge (x 2^40), denormal
(x 1e-40), +Inf, -Inf or NaN row in every latent layer, on the six kernel forms (default, ws=3 unified, ws=2 in-place lean, ws=2 generic,
ws=0 barrier, ws=4 layer-wise; `mcpc_last_step_kernel_name` proves which one ran).  Per (net, form, kind, chain position) four calls:
(a) SGD + Philox kick with accumulation, every state and output recorded, the energy table; (b) Adam on x and its moments; (c) one
gradients-only step; (d) mcpc_chain_energies on the records of (a).
  1. Confinement: every OTHER chain's final state, records, outputs, x-gradients, Adam moments and per-chain energies are BITWISE those
     of the same call without the special chain.  No tolerance.
  2. A finite special chain against the fp64 oracle: states and records within 1e-6 max(10, max |x| of the chain) -- the state contract
     of BASELINE.md section 3 at the chain's own scale; its per-chain energies within the bound of chain_energy_cases.oracle_rows; the
     energy table rtol 1e-6; the gradient bucket rtol 2e-4 + 2e-5 max |want|.  (tests/test_special_value_cases.py: the oracle's own
     fp32 run uses at most a fifth of each.)
  3. A non-finite special chain: its own per-chain energies are non-finite, everyone else's finite (and equal to the baseline, 1).
  4. The forms against each other ON the special chain, NaN positions included, where the project states bitwise agreement: the four
     LDS-resident forms under a bounded Bernoulli read-out (csrc/mcpc_gemm_f16.h), all six on the nets with their read-out removed
     (tests/test_gpu_wide.py).  This holds rowexp_track (a ds_max_u32 on the exponent field) to gemm_row_exp (a scan) at the clamped
     exponents: field 0 and field 255."""
import functools

import numpy as np
import pytest
import torch

from tests import parity_log
from tests import special_value_cases as sv
from tests import wide_cases as wc
from tests.chain_energy_cases import columns
from tests.test_gpu_flush import STEP_CASES, STEP_WANT
from tests.test_gpu_wide import _t, final_states, loss_kw, make_engine, sgd_kick_call

pytestmark = pytest.mark.gpu

# the forms of tests/test_gpu_flush.py (None: default tuning), and the layer-wise kernels
FORMS = [t for n, t in STEP_CASES if n == "small"] + ["ws=4"]
U_KERNEL, WS2_KERNEL, BARRIER_KERNEL = STEP_WANT["ws=3"], STEP_WANT["ws=2"], STEP_WANT["ws=0"]
LDS_FORMS = [f for f in FORMS if f != "ws=4"]
NET_COMBOS = [(n, c) for n in sorted(sv.NETS) for c in sorted(sv.COMBOS)]


def _ran_the_form(step, form, updates_x):
    """Whether `step` (mcpc_last_step_kernel_name) is the kernel the form stands for.  A run on a specialised instantiation of the in-place
    kernel names it BEHIND the generic kernel's name; a gradients-only run is never served by the unified-wave kernel (use_unified)."""
    if form == "ws=4":
        return "mcpc_lw_fwd_kernel" in step and "mcpc_lw_bwd_kernel" in step
    if form is None:
        return any(step.startswith(k) for k in (U_KERNEL, WS2_KERNEL, BARRIER_KERNEL))
    want = WS2_KERNEL if form == "ws=3" and not updates_x else STEP_WANT[form]
    return step.startswith(want)


def _np(ts):
    return [t.cpu().numpy() for t in ts]


def _four_calls(eng, case, X0, inputs):
    """Calls (a)-(d) from the state X0; everything a test compares, as NumPy arrays."""
    from montecarlopredictivecoding_amd import _lib as L
    T, Ln, B = sv.T, len(case["sizes"]), case["B"]
    out = {}
    dev = inputs.device
    # (a) SGD with the Philox kick
    eng.load_state([_t(x) for x in X0])
    res = sgd_kick_call(eng, case, acc=(1, T), rec_begin=0, rec_stride=1, rec_count=T, rec_x=True, rec_out=True)
    eng.sync_check()
    out["kernel_a"] = eng.last_step_kernel()
    out["x"] = final_states(eng, case)
    out["rec"] = _np(res.rec_x)
    out["rec_out"] = None if res.rec_out is None else res.rec_out.cpu().numpy()
    out["energies"] = res.energies.cpu().numpy()
    out["bucket"] = eng.read_param_grads_flat().cpu().numpy()
    # (d) per-chain energies of the records of (a)
    rows = eng.chain_energies(inputs, res.rec_x, **loss_kw(case))
    eng.sync_check()
    out["rows"] = columns(rows.cpu().numpy(), Ln)
    # (b) Adam on x, no noise
    eng.load_state([_t(x) for x in X0])
    eng.run(T, xopt=L.XOPT_ADAM, lr=sv.ADAM_LR, **loss_kw(case))
    eng.sync_check()
    out["kernel_b"] = eng.last_step_kernel()
    out["adam_x"] = final_states(eng, case)
    ms = [torch.empty(B, n, device=dev) for n in case["sizes"]]
    vs = [torch.empty(B, n, device=dev) for n in case["sizes"]]
    eng.store_adam_state(ms, vs)
    eng.sync_check()
    out["exp_avg"], out["exp_avg_sq"] = _np(ms), _np(vs)
    # (c) one gradients-only step
    eng.load_state([_t(x) for x in X0])
    res = eng.run(1, update_x=False, xopt=L.XOPT_SGD, lr=wc.LR, **loss_kw(case))
    eng.sync_check()
    out["kernel_c"] = eng.last_step_kernel()
    out["xgrad"] = _np(res.xgrad)
    return out


def _chain_of(out, chain):
    """What assertion 4 compares of the special chain: states and records of (a), states of (b)."""
    return [x[chain] for x in out["x"]] + [r[:, chain] for r in out["rec"]] + [x[chain] for x in out["adam_x"]]


@functools.lru_cache(maxsize=None)
def _form_case(net, combo, form, readout=True):
    """Every (kind, chain position) of one (net, activation x loss, form) on ONE engine, the baseline computed once; assertions 1-3 are
    made here, the special chain's own numbers are returned for assertion 4.  Finite kinds run before the non-finite ones."""
    case = sv.case(net, combo, readout)
    W, b, X0, inputs, target = sv.data(net, combo, readout)
    eng = make_engine(case, form or "", W=W, b=b, inputs=inputs, target=target)
    inputs_t = _t(inputs)
    tag = f"{case['name']} {form or 'default'}"
    kernels, chains = set(), {}
    try:
        base = _four_calls(eng, case, X0, inputs_t)
        for key, upd in (("kernel_a", True), ("kernel_b", True), ("kernel_c", False)):
            assert _ran_the_form(base[key], form, upd), (tag, key, base[key])
        assert np.isfinite(base["rows"]).all() and np.isfinite(base["energies"]).all()
        for kind in sv.kinds(combo):
            for chain in sv.CHAINS:
                who = f"{tag}, {kind} chain {chain}"
                out = _four_calls(eng, case, sv.special_x0(X0, kind, chain), inputs_t)
                for key in ("kernel_a", "kernel_b", "kernel_c"):
                    assert out[key] == base[key], (who, out[key], base[key])
                kernels.add(out["kernel_a"])
                others = np.arange(sv.B) != chain
                # 1. confinement, bitwise
                for q in ("x", "adam_x", "exp_avg", "exp_avg_sq", "xgrad"):
                    for l, (got, want) in enumerate(zip(out[q], base[q])):
                        assert np.array_equal(got[others], want[others]), f"{who}: {q} of layer {l + 1} of another chain changed"
                for l, (got, want) in enumerate(zip(out["rec"], base["rec"])):
                    assert np.array_equal(got[:, others], want[:, others]), f"{who}: a record of layer {l + 1} of another chain changed"
                if readout:
                    assert np.array_equal(out["rec_out"][:, others], base["rec_out"][:, others]), f"{who}: a recorded output of another chain changed"
                assert np.array_equal(out["rows"][:, others], base["rows"][:, others]), f"{who}: per-chain energies of another chain changed"
                if kind == "dead":
                    assert max(float(r[:, chain].max()) for r in out["rec"]) < 0, f"{who}: the dead chain came alive"
                if kind in sv.FINITE and readout:
                    _check_finite_chain(who, form, net, combo, kind, chain, out)
                if kind in sv.NONFINITE:
                    # 3. (every other row is finite: it equals the finite baseline)
                    assert not np.isfinite(out["rows"][:, chain, -1]).any(), f"{who}: a finite overall energy of the special chain"
                chains[(kind, chain)] = _chain_of(out, chain)
    finally:
        eng.close()
    return dict(kernels=kernels, kernel_c=base["kernel_c"], chains=chains)


def _check_finite_chain(who, form, net, combo, kind, chain, out):
    """2. the special chain against the fp64 oracle.  (The parity log keeps one group per form and one quantity per kind.)"""
    ref = sv.oracle(net, combo, kind, chain)
    group = f"special chain vs fp64 oracle ({form or 'default'})"
    atol = sv.state_bound(net, combo, kind, chain)
    Ln = len(out["x"])
    for l in range(Ln):
        parity_log.close(group, f"{kind}: x final", out["x"][l][chain], ref.xs[l][chain], rtol=0, atol=atol, err_msg=who)
        want = np.stack([ref.rec_xs[t][l][chain] for t in range(sv.T)])
        parity_log.close(group, f"{kind}: x[t] records", out["rec"][l][:, chain], want, rtol=0, atol=atol, err_msg=who)
    en = out["energies"]
    assert np.isfinite(en).all(), who
    parity_log.close(group, f"{kind}: overall[t]", en[:, -1], ref.overall, rtol=1e-6, err_msg=who)
    parity_log.close(group, f"{kind}: loss[t]", en[:, 0], ref.loss, rtol=1e-6, err_msg=who)
    parity_log.close(group, f"{kind}: E_l[t]", en[:, 1:1 + Ln], ref.layer_energy, rtol=1e-6, err_msg=who)
    bucket = wc.bucket(ref)
    parity_log.close(group, f"{kind}: bucket", out["bucket"], bucket, rtol=2e-4, atol=2e-5 * float(np.abs(bucket).max()), err_msg=who)
    want, bound = sv.chain_rows(net, combo, chain, [r[:, chain:chain + 1] for r in out["rec"]])
    got = out["rows"][:, chain:chain + 1]
    for i, q in enumerate(["loss"] + [f"E_{l + 1}" for l in range(Ln)] + ["overall"]):
        bnd = np.maximum(bound[..., i], 1e-300)
        parity_log.close(group, f"{kind}: chain {q}/bound", got[..., i] / bnd, want[..., i] / bnd, rtol=0.0, atol=1.0, err_msg=who)


@pytest.mark.parametrize("form", FORMS, ids=[f or "default" for f in FORMS])
@pytest.mark.parametrize("net,combo", NET_COMBOS)
def test_a_special_chain_stays_in_its_chain(net, combo, form):
    got = _form_case(net, combo, form)
    assert len(got["chains"]) == len(sv.kinds(combo)) * len(sv.CHAINS)


@pytest.mark.parametrize("form", FORMS, ids=[f or "default" for f in FORMS])
@pytest.mark.parametrize("net,combo", NET_COMBOS)
def test_a_special_chain_stays_in_its_chain_without_a_readout(net, combo, form):
    got = _form_case(net, combo, form, readout=False)
    assert len(got["chains"]) == len(sv.kinds(combo)) * len(sv.CHAINS)


def _assert_forms_agree(net, combo, forms, readout):
    first = _form_case(net, combo, forms[0], readout)["chains"]
    for form in forms[1:]:
        other = _form_case(net, combo, form, readout)["chains"]
        for key in first:
            for i, (a, c) in enumerate(zip(first[key], other[key])):
                assert np.array_equal(a, c, equal_nan=True), \
                    f"{net} {combo} readout={readout}: the {key[0]} chain {key[1]} differs between {forms[0] or 'default'} and {form} (array {i})"


@pytest.mark.parametrize("net", sorted(sv.NETS))
def test_the_lds_forms_agree_bitwise_on_the_special_chain(net):
    """A bounded Bernoulli read-out: its error rows take a fixed exponent and the forms are stated to agree bitwise."""
    _assert_forms_agree(net, "relu_bernoulli", LDS_FORMS, True)


@pytest.mark.parametrize("net,combo", NET_COMBOS)
def test_all_forms_agree_bitwise_on_the_special_chain_without_a_readout(net, combo):
    _assert_forms_agree(net, combo, FORMS, False)


def test_every_form_ran_its_own_kernel():
    ran = {}
    for form in FORMS:
        got = _form_case("short", "relu_bernoulli", form)
        assert len(got["kernels"]) == 1, (form, got["kernels"])
        ran[form or "default"] = (next(iter(got["kernels"])), got["kernel_c"])
    print(f"[special values: step kernels] {ran}")
    assert ran["ws=3"][0].startswith(U_KERNEL) and ran["ws=3"][1].startswith(WS2_KERNEL)
    assert ran["ws=2"][0].startswith(WS2_KERNEL) and ran["ws=2,no_lean=1"][0].startswith(WS2_KERNEL)
    assert ran["ws=0"] == (BARRIER_KERNEL, BARRIER_KERNEL)
    assert "mcpc_lw_fwd_kernel" in ran["ws=4"][0] and "mcpc_lw_fwd_kernel" in ran["ws=4"][1]
    assert "mcpc_lw" not in ran["default"][0] and "mcpc_lw" not in ran["default"][1]


# ================================================================================================================================
# PART 2.  The per-element functions of csrc/mcpc_device.h at their edges, one element per chain.
#
# On a network of width 1 a row of mcpc_chain_energies (fp64 of ONE fp32 value) and an element of a gradients-only step's xgrad are single
# values of mcpc_step_math.h.  4096 chains, one sample point each; the inputs have their two lowest mantissa bits cleared (22 significant
# bits), so the two-piece fp16 split carries them EXACTLY through a K = 1 product with a weight of 1.0 (csrc/mcpc_gemm_f16.h) -- between
# the exponent clamps: a value below 2^-63 is rounded to a multiple of 2^-84 (the row is scaled by at most 2^60 and the pieces are fp16),
# a value of 2^74 or more overflows the pieces (documented there; such a chain's own energy overflows fp32 anyway) -- the two sample
# points +-1e30 of the read-out sweep are therefore run (their neighbours are held to their bounds) and printed, but not bounded.
#
#   net E   sizes (1,), identity, W0 = b0 = 0, W_out = 1, b_out = 0:  o = x_1,  loss[chain] = bce(o, y) or 0.5 inv_var (o - y)^2,
#           E_1 = 0.5 c x^2,  xgrad = x + (sigmoid(x) - y)
#   net T   sizes (1, 1), tanh, W1 = 1, b1 = 0, x_2 = 0:  E_2 = 0.5 tanh_f(x_1)^2,  xgrad_1 = x_1 + t (1 - t^2)
#   net R   net T with ReLU and x_2 = 1 (with x_2 = 0 the back-projected error of a denormal x_1 is itself zero and hides f'):
#           xgrad_1 = x_1 - f'(x_1) (1 - f(x_1)),  f' = 1 only for x > 0
#
# BOUNDS.  u = 2^-24, the unit roundoff of fp32: one correctly rounded operation is off by at most u |result|.  The transcendental
# instructions v_exp_f32 (2^x), v_log_f32 (log2) and v_rcp_f32 are taken at the 1 ulp <= 2 u |result| the instruction set reference
# states and csrc/mcpc_device.h has always assumed ("v_sqrt_f32 / v_rcp_f32 (1 ulp each)").  First order in u, with 1 % on top for the
# higher orders; 2^-126 / 2^-149 stand for a flushed or denormal result.  Every bound is evaluated in fp64 at each sample point.
#   e = exp(-|o|) as v_exp_f32(fl(-|o| c)), c = fl(log2 e):  the argument is off by 2 u |a| (the constant and the product), which moves e
#       by e ln2 2 u |a| = 2 u |o| e:      de <= e (2 u + 2 u |o|) + 2^-126
#   s = fl(1 + e):                          ds <= de + u s                    (1 + e rounds to 1 from |o| ~ 17 on: inside u s)
#   r = v_rcp_f32(s):                       dr <= r (ds / s + 2 u) = r (de / s + 3 u)
#   sigmoid_f, o >= 0:  sigma = r           dsigma <= sigma (de / s + 3 u)                                  <= 4.3 u = 2.6e-7
#              o <  0:  sigma = fl(e r)     dsigma <= de / s + sigma (de / s + 4 u)
#   bce = max(o, 0) - o y + fl(ln2) v_log_f32(s):  the logarithm term lg is off by lg 4 u (1 ulp, the constant, the product) + ds / s;
#       the three other operations (o y; max - o y; the sum; fewer when contracted into fma) by u (|o y| + |max - o y| + |bce|):
#                                           dbce <= lg 4 u + ds / s + u (|o y| + |max(o, 0) - o y| + |bce|) + 2^-149
#       At |o| >= 17 and y = 1 the true value e is below u and the computed one is 0: the bound there is absolute (ds / s ~ u), as the
#       loss's own contract is.
#   Gaussian loss 0.5 inv_var d^2, d = fl(o - y), inv_var = 2:  d carries u, its square 2 u, two products 2 u:   4 u |loss| + 2^-149
#   E_1 = 0.5 c fl(x^2), c a power of two:  u |E_1| + 2^-149; where 0.5 c x^2 exceeds fp32's range the result must be +Inf
#   xgrad of net E = fl(x + back), back the K = 1 back-projection of e_o = fl(sigma - y), a full 24-bit value: the split keeps 22 bits
#       (2^-22 |e_o|); a bounded 0/1 target fixes the row's exponent at 13, where a second piece below fp16's normal range is cut at 2^-37:
#                                           dsigma + u |e_o| + 2^-22 |e_o| + 2^-37 + u |xgrad|
#   tanh_f = 1 - 2 v_rcp_f32(fl(E + 1)), E = v_exp_f32(fl(x c2)), c2 = fl(2 log2 e):  the argument 2.885 x is off by 2 u |2.885 x|, which
#       moves E by 4 u |x| E; with E / (1 + E) = (1 + t) / 2 and 2 r = 1 - t:
#                                           dt <= (1 - t) ((1 + t) / 2 (2 u + 4 u |x|) + 3 u) + u |t| + 2^-126
#       = 4 u = 2.4e-7 at 0, 7 u = 4.2e-7 towards -1 (there 2 r ~ 2 carries the reciprocal's whole ulp), u towards +1.  ABSOLUTE: near 0 the
#       relative error of tanh_f is unbounded by design, and the trajectory contract is absolute too.
#   E_2 = 0.5 fl(mu^2), mu = t through the forward GEMM (2^-22 |t|):  D = dt + 2^-22 |t|;   |t| D + D^2 / 2 + u E_2 + 2^-149
#   xgrad_1 = fl(x + a t'), a = fl(1 - fl(t t)), t' = t through both GEMMs:  da <= 2 |t| dt + dt^2 + u,  D2 = dt + 2^-21 |t|;
#                                           da (|t| + D2) + (1 - t^2) D2 + u |(1 - t^2) t| + u |xgrad_1|
#   tanh_f(+-Inf) must be exactly +-1 and 1 - t^2 exactly 0: E_2 == 0.5 and xgrad_1 == x_1 there.
U = 2.0 ** -24
N2 = 4096
HIGHER = 1.01
F32_MAX = float(np.finfo(np.float32).max)
Y_VALUES = (0.0, 1.0, 0.3, -1.5, 2.5)
PART2 = "per-element functions vs fp64 (error / derived bound)"


def _clear2(v):
    """fp32 with the two lowest mantissa bits cleared."""
    a = np.array(v, dtype=np.float32)
    a.view(np.uint32)[...] &= np.uint32(0xFFFFFFFC)
    return a


def _signed(mags):
    m = _clear2(mags)
    return np.concatenate([m, -m])


def _pad(a, fill=0.0):
    out = np.full(N2, fill, np.float32)
    assert a.size <= N2
    out[:a.size] = a
    return out


# +-{0, 1e-42, 1e-30, 1e-8, a log-spaced grid to 16, 16 .. 18 in steps of 1/16, 30, 87, 88, 89, 103, 104, 1e4, 1e30}
O_SWEEP = _signed(np.concatenate([[0.0, 1e-42, 1e-30, 1e-8], np.geomspace(1e-6, 16.0, 360), 16.0 + np.arange(33) / 16.0,
                                  [30.0, 87.0, 88.0, 89.0, 103.0, 104.0, 1e4, 1e30]]))
# +-{0, 1e-42, 1e-8, 1e-4, a grid to 9, 9 .. 10, 44, 44.5, 88, 1e30, Inf}
X_SWEEP = _signed(np.concatenate([[0.0, 1e-42, 1e-8, 1e-4], np.geomspace(1e-3, 9.0, 1900), 9.0 + np.arange(65) / 64.0,
                                  [44.0, 44.5, 88.0, 1e30, np.inf]]))


def _readout_points(bounded):
    """(o, y) [N2]: every o of the sweep with every target value; bounded: targets 0 / 1 only."""
    o = np.tile(O_SWEEP, len(Y_VALUES))
    y = np.repeat(np.asarray(Y_VALUES, np.float32), O_SWEEP.size)
    if bounded:
        y = (np.arange(y.size) // O_SWEEP.size % 2).astype(np.float32)
    return _pad(o), _pad(y)


def _engine2(sizes, act, n_out, W, b, ecoef=None, tuning=None, target=None):
    from montecarlopredictivecoding_amd.engine import Engine
    dev = torch.device("cuda", 0)
    eng = Engine(list(sizes), [act] * len(sizes), 1, n_out, N2, device=dev, ecoef=ecoef, tuning=tuning)
    eng.bind_params([torch.tensor(w, dtype=torch.float32, device=dev).reshape(1, 1) for w in W],
                    [torch.tensor(v, dtype=torch.float32, device=dev).reshape(1) for v in b])
    eng.bind_inputs(None)
    if target is not None:
        eng.bind_target(_t(target.reshape(N2, 1)))
    return eng


def _col(x):
    return _t(np.asarray(x, np.float32).reshape(N2, 1))


def _hold(quantity, got, want, bound, mask=None):
    """|got - want| <= bound per sample point; the achieved fraction of the bound goes to the parity log, the largest error is printed."""
    got, want, bound = (np.asarray(a, np.float64).reshape(-1) for a in (got, want, bound))
    if mask is not None:
        got, want, bound = got[mask], want[mask], bound[mask]
    assert np.isfinite(want).all() and (bound > 0).all()
    err = np.abs(got - want)
    frac = err / bound
    i = int(np.nanargmax(np.where(np.isfinite(frac), frac, np.inf)))
    print(f"[{PART2}] {quantity}: max |error| {np.nanmax(err):.3e}; max error / bound {frac[i]:.3f} at want = {want[i]:.9g}, got = {got[i]:.9g}")
    parity_log.close(PART2, quantity, got / bound, want / bound, rtol=0.0, atol=1.0)


def _exp_parts(o):
    o = np.asarray(o, np.float64)
    e = np.exp(-np.abs(o))
    de = e * (2 * U + 2 * U * np.abs(o)) + 2.0 ** -126
    return o, e, 1.0 + e, de


def sigmoid_ref_and_bound(o):
    o, e, s, de = _exp_parts(o)
    sig = np.where(o >= 0, 1.0 / s, e / s)
    bound = np.where(o >= 0, sig * (de / s + 3 * U), de / s + sig * (de / s + 4 * U))
    return sig, HIGHER * bound


def bce_ref_and_bound(o, y):
    o, e, s, de = _exp_parts(o)
    y = np.asarray(y, np.float64)
    lg = np.logaddexp(0.0, -np.abs(o))
    ref = np.maximum(o, 0.0) - o * y + lg
    ds = de + U * s
    bound = lg * 4 * U + ds / s + U * (np.abs(o * y) + np.abs(np.maximum(o, 0.0) - o * y) + np.abs(ref)) + 2.0 ** -149
    return ref, HIGHER * bound


def tanh_ref_and_bound(x):
    x = np.asarray(x, np.float64)
    t = np.tanh(x)
    ax = np.where(np.isfinite(x), np.abs(x), 0.0)                    # (at +-Inf 1 - t or 1 + t is an exact zero)
    dt = (1 - t) * ((1 + t) / 2 * (2 * U + 4 * U * ax) + 3 * U) + U * np.abs(t) + 2.0 ** -126
    return t, dt


INSIDE = lambda v: np.abs(np.asarray(v, np.float64)) < 2.0 ** 74         # below the GEMM core's exponent clamp


@pytest.mark.parametrize("bounded", [False, True], ids=["any_target", "binary_target"])
def test_bce_with_logits_at_its_edges(bounded):
    from montecarlopredictivecoding_amd import _lib as L
    o, y = _readout_points(bounded)
    eng = _engine2((1,), L.ACT_IDENTITY, 1, W=[0.0, 1.0], b=[0.0, 0.0], target=y)
    rows = eng.chain_energies(None, [_col(o)], loss_kind=L.LOSS_BERNOULLI).cpu().numpy()[0]
    eng.sync_check()
    eng.close()
    want, bound = bce_ref_and_bound(o, y)
    _hold(f"bce_logits ({'0/1' if bounded else 'any'} target)", rows[:, 0], want, bound, INSIDE(o))
    print(f"[{PART2}] bce at |o| = 1e30 (above the exponent clamp, not bounded): {sorted(set(rows[~INSIDE(o), 0].tolist()), key=str)}")
    assert np.array_equal(rows[:, 0] + rows[:, 1], rows[:, -1], equal_nan=True)


def test_gaussian_loss_and_layer_energy_at_their_edges():
    from montecarlopredictivecoding_amd import _lib as L
    o, y = _readout_points(False)
    o64, y64 = o.astype(np.float64), y.astype(np.float64)
    for c in (0.5, 2.0):
        eng = _engine2((1,), L.ACT_IDENTITY, 1, W=[0.0, 1.0], b=[0.0, 0.0], ecoef=[c], target=y)
        rows = eng.chain_energies(None, [_col(o)], loss_kind=L.LOSS_GAUSSIAN, loss_var=0.5).cpu().numpy()[0]
        eng.sync_check()
        eng.close()
        want = (o64 - y64) ** 2                                        # 0.5 inv_var = 1
        _hold(f"gaussian loss (c = {c})", rows[:, 0], want, HIGHER * 4 * U * want + 2.0 ** -149, INSIDE(o))
        want = 0.5 * c * o64 * o64
        fits = want <= F32_MAX
        _hold(f"E_1 = 0.5 c x^2 (c = {c})", rows[:, 1], want, HIGHER * U * want + 2.0 ** -149, fits)
        assert np.isposinf(rows[~fits, 1]).all() and (~fits).sum() == 2 * len(Y_VALUES)


@pytest.mark.parametrize("tuning", [None, "ws=0", "ws=4"], ids=["default", "ws=0", "ws=4"])
@pytest.mark.parametrize("bounded", [False, True], ids=["any_target", "binary_target"])
def test_sigmoid_in_the_x_gradient_at_its_edges(bounded, tuning):
    from montecarlopredictivecoding_amd import _lib as L
    o, y = _readout_points(bounded)
    eng = _engine2((1,), L.ACT_IDENTITY, 1, W=[0.0, 1.0], b=[0.0, 0.0], tuning=tuning, target=y)
    eng.load_state([_col(o)])
    res = eng.run(1, update_x=False, xopt=L.XOPT_SGD, loss_kind=L.LOSS_BERNOULLI)
    eng.sync_check()
    got = res.xgrad[0].cpu().numpy().reshape(-1)
    eng.close()
    o64, y64 = o.astype(np.float64), y.astype(np.float64)
    sig, dsig = sigmoid_ref_and_bound(o)
    eo = sig - y64
    want = o64 + eo
    bound = dsig + HIGHER * (U * np.abs(eo) + 2.0 ** -22 * np.abs(eo) + 2.0 ** -37 + U * np.abs(want))
    _hold(f"x + sigmoid(x) - y ({'0/1' if bounded else 'any'} y, {tuning or 'default'})"[:60], got, want, bound, INSIDE(o))


@pytest.mark.parametrize("tuning", [None, "ws=0", "ws=4"], ids=["default", "ws=0", "ws=4"])
def test_tanh_at_its_edges(tuning):
    from montecarlopredictivecoding_amd import _lib as L
    x = _pad(X_SWEEP)
    zeros = np.zeros(N2, np.float32)
    eng = _engine2((1, 1), L.ACT_TANH, 0, W=[0.0, 1.0], b=[0.0, 0.0], tuning=tuning)
    rows = eng.chain_energies(None, [_col(x), _col(zeros)]).cpu().numpy()[0]
    eng.sync_check()
    eng.load_state([_col(x), _col(zeros)])
    res = eng.run(1, update_x=False, xopt=L.XOPT_SGD)
    eng.sync_check()
    g = res.xgrad[0].cpu().numpy().reshape(-1)
    eng.close()
    x64 = x.astype(np.float64)
    t, dt = tanh_ref_and_bound(x)
    finite = np.isfinite(x64)
    D = dt + 2.0 ** -22 * np.abs(t)
    e2 = 0.5 * t * t
    _hold(f"E_2 = 0.5 tanh_f(x)^2 ({tuning or 'default'})", rows[:, 2], e2, HIGHER * (np.abs(t) * D + D * D / 2 + U * e2) + 2.0 ** -149)
    da = 2 * np.abs(t) * dt + dt * dt + U
    D2 = dt + 2.0 ** -21 * np.abs(t)
    want = np.where(finite, x64, 0.0) + t * (1 - t * t)
    bound = HIGHER * (da * (np.abs(t) + D2) + (1 - t * t) * D2 + U * np.abs((1 - t * t) * t) + U * np.abs(want)) + 2.0 ** -149
    _hold(f"x + t (1 - t^2) ({tuning or 'default'})", g, want, bound, finite)
    # tanh_f(+-Inf) = +-1 exactly, its derivative exactly 0
    assert (~finite).sum() == 2 and np.array_equal(rows[~finite, 2], [0.5, 0.5]), rows[~finite, 2]
    assert np.array_equal(g[~finite], x[~finite]), g[~finite]


@pytest.mark.parametrize("tuning", [None, "ws=0", "ws=4"], ids=["default", "ws=0", "ws=4"])
def test_relu_derivative_at_zero_and_denormals(tuning):
    """f'(x) = 1 only for x > 0: -0, +0 and negative denormals give 0, the smallest positive denormal gives 1."""
    from montecarlopredictivecoding_amd import _lib as L
    mags = np.array([0.0, 1.4e-45, 1e-42, 1e-40, 1.1754942e-38, 1.17549435e-38, 1e-30, 1e-8, 0.5, 1.0, 3.0], np.float32)
    x = _pad(np.concatenate([mags, -mags]))
    assert np.signbit(x[mags.size]) and x[mags.size] == 0 and x[1] > 0
    eng = _engine2((1, 1), L.ACT_RELU, 0, W=[0.0, 1.0], b=[0.0, 0.0], tuning=tuning)
    eng.load_state([_col(x), _col(np.ones(N2, np.float32))])
    res = eng.run(1, update_x=False, xopt=L.XOPT_SGD)
    eng.sync_check()
    g = res.xgrad[0].cpu().numpy().reshape(-1).astype(np.float64)
    eng.close()
    x64 = x.astype(np.float64)
    f = np.maximum(x64, 0.0)
    want = x64 - (x64 > 0) * (1.0 - f)
    # the error 1 - f passes two K = 1 GEMMs (2^-21 of it); a denormal f or x may be flushed (2^-126)
    bound = HIGHER * (2.0 ** -21 * np.abs(1.0 - f) * (x64 > 0) + U * np.abs(want)) + 2.0 ** -125
    _hold(f"x - relu'(x) (1 - relu(x)) ({tuning or 'default'})", g, want, bound)

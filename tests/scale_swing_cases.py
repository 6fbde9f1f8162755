"""Shared by tests/test_scale_swing_cases.py (CPU) and tests/test_gpu_scale_swings.py: chain rows whose magnitude JUMPS from one step, and
one read-out chunk, to the next.  Cases, schedules, fp64 references and bounds; no device is needed here.

Every contraction of a step scales each chain row of its LDS operand by a power of two (csrc/mcpc_gemm_f16.h) that comes from a row
scan (gemm_row_exp: the barrier kernel, and the in-place kernel's generic epilogues), from the word the row's producers keep as
(generation << 8) | exponent field (rowexp_track: the in-place kernel's lean epilogues and the unified-wave kernel) or, for the chunks of
an unbounded read-out error, from the chunk's own maximum with the accumulators rescaled in between (GemmScale::run).  An exponent that
is one generation late, a ring slot's word that survives the slot's reuse, or a rescale the wrong way is wrong by exactly what the row
moved since: every case here makes that a factor of 2^4 .. 2^49, while every row maximum that enters a GEMM stays between the limits
asserted by a_teeth / b_teeth, far from the limits of the arithmetic (2^-63 / 2^74).

PART A -- rows driven by injected kicks (NOISE_EXTERNAL).  Net 5 -> 24 | 72 | 40 -> 784 (widths that are no multiple of 32; the in-place
plan cuts the read-out into four chunks), 40 chains (two full 16-chain tiles, one with 8 live chains), T = 14 steps of SGD with lr = 1 and
noise_var = 1: x_{t+1} = mu + f'(x_t) back + xi_t, the kick is added as it is.  Every Linear has row abs-sums of about 2^-24, so the kick
decides the row's scale.  A chain's state cycles through CYCLE (six states: the four scales 2^12, 2^-12, "the size of the GEMM terms",
"no kick", and 2^12 twice more, once with every unit negative, so that under ReLU an f(x) row is exactly zero between two rows that are
alive at 2^12); chain c is (c mod 6) states ahead of chain 0, so a 16-chain tile holds every state at every step.  What the fp64 oracle
gives for this recipe (test_scale_swing_cases.py prints and asserts it): row maxima of x between 2^-38 and 2^12, per tile, step and
layer a row that rises by 2^35.7 or more beside one that falls by 2^23.2 or more.  The floor of a row without a kick is its bias (2^-38),
in the first layer the prediction from the inputs (2^-24.6) and in the last one the read-out's back-projection (2^-24).

PART B -- rows that grow or decay geometrically by the dynamics alone (the unified-wave kernel and the specialised instantiations of the
in-place kernel take no injected noise).  The same widths, a Bernoulli read-out with a 0/1 target, 40 chains whose x_0 has a scale
2^-12 .. 2^12 of its own (every tile holds the whole range), T = 8, SGD with lr = 1 and the Philox kick at noise_var = 2^-120 (a kick of
2^-60 z, far below every value; the reference includes it), or Adam.  One step is x' = mu + f'(x) (W_next^T e_next), e = x - mu.
  growth        identity.  For a gain above 1 the step is dominated by -W_next^T W_next x: a negative definite map, so NO state can keep its
                signs while it grows, and under ReLU the units that carry a row die the step after (measured: rows of a random ReLU net
                move by 2^-2 .. 2^8 per step at gains of 2^2.5 and 2^3).  A linear net has no such trouble: x_0 lies along the eigenvector of the
                largest |eigenvalue| (_common_mode), each chain up to a fifth off it in its own way, and EVERY row of every layer rises
                by 2^4.3 .. 2^5.3 per step.  The chain that began at 2^12 ends at 2^50 -- a rise of 2^4 per step over 8 steps from 2^12
                cannot end below 2^44 whatever the net.
  growth_relu   all ReLU, random weights of gain 2^2.5, for the specialised instantiation: rows rise by 2^5 on average and unevenly.
                Asserted: per 16-chain tile, step and layer a row that rose by 2^2 at least (2^3 on the oracle) -- a row's maximum is
                scaled into [2^14, 2^15) and fp16 ends at 2^16, so under an exponent one step old such a row is Inf.
  decay         all ReLU.  Positive weights (row sums 2^-5.3) and positive states: every unit stays alive, the step is a positive linear
                map and x_0 lies along its Perron vector (+- a fifth): every row falls by 2^4.3 .. 2^4.7 per step.  Nothing may hold a
                row up: no inputs, zero biases, and a read-out saturated by its bias (b_out = +-110 where y = 1 / 0: the fp32 sigmoid is
                exactly y, the error row exactly zero).  The chain that began at 2^-12 ends at 2^-49: its last rows have passed the clamp
                of the scale exponent (2^60: maxima below 2^-46), which every mechanism applies alike, not the 2^-63 of the arithmetic.
  adam          all ReLU, lr = 2^12 from x_0 ~ 2^-12 with ordinary weights (+-1/sqrt(fan_in)): the first step moves every element by lr,
                every row by 2^24.

PART C -- the chunks of an unbounded (Gaussian) read-out error at very different scales.  24 | 72 | 40 -> 784, identity, all parameters but
the read-out's weights zero, x = 0: o = 0, e_o = -y, and a gradients-only step returns the back-projection W_out^T e_o as xgrad of the last
layer (an update step with lr = 1 its negative as the new state).  The target is scaled per chunk of 16 x `chunk` read-out units (the
in-place plan's chunks: mcpc_debug_plan), consecutive scales 2^20 apart, in three orders; unit j of the last layer connects to chunk
j mod n_chunks only, so every entry holds the terms of ONE chunk.  Two-step variants: c2_data.

BOUNDS (tests/test_gpu_accuracy.py, imported, never restated): a GEMM result is within C_OP + c_acc(K) of its own sum |terms|, one fp32
rounding on top where the result is stored as fp32 after a bias (2^-24); terms 2^rho below the row's maximum -- here: a chunk's, under
the largest chunk's exponent or any cut of the read-out -- max(C_OP, 2^-22 + 2^(rho - 39)) + c_acc(K): the RANGE paragraph there.  A whole
step is held to the 1e-6 of sum |terms| of test_gemm_core_accuracy_against_fp64, the terms of x_{t+1} = x - (x - mu) + f' back + kick
including x and -x."""
import functools

import numpy as np

from oracle import mcpc_oracle as mo
from oracle import philox

SIZES = [24, 72, 40]
N_IN, N_OUT, B = 5, 784, 40
ACT = {"identity": mo.ACT_IDENTITY, "relu": mo.ACT_RELU}
STEP_RTOL = 1e-6                          # test_gemm_core_accuracy_against_fp64


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, (list, tuple)):
            _frozen(*a)
        elif a is not None:
            a.setflags(write=False)


def _mags(rng, shape):
    """Magnitudes in [0.5, 1)."""
    return 0.5 + 0.5 * rng.random_sample(shape)


def _signed(rng, shape):
    return _mags(rng, shape) * np.where(rng.random_sample(shape) < 0.5, -1.0, 1.0)


def _linears(rng, dims, gains):
    """Uniform weights whose row abs-sums are about gains[j]."""
    return [((rng.random_sample((dims[j + 1], dims[j])) * 2 - 1) * (gains[j] / (0.5 * dims[j]))).astype(np.float32) for j in range(len(dims) - 1)]


def engine_case(name, act, n_out, loss, batch=B, n_in=N_IN):
    """The dict tests/test_gpu_wide.py: make_engine and loss_kw take."""
    return dict(name=name, n_in=n_in, sizes=list(SIZES), acts=[act] * len(SIZES), ecoef=[1.0] * len(SIZES), n_out=n_out, loss=loss, var=1.0,
                B=batch)


def net_spec(case, W, b):
    return mo.NetSpec(sizes=case["sizes"], acts=[ACT[a] for a in case["acts"]], W=W, b=b, has_head=case["n_out"] > 0)


def loss_spec(case, target):
    kind = {"none": mo.LOSS_NONE, "gaussian": mo.LOSS_GAUSSIAN, "bernoulli": mo.LOSS_BERNOULLI}[case["loss"]]
    return mo.LossSpec(kind, target, var=case["var"])


def as64(arrays):
    return [None if a is None else np.asarray(a, np.float64) for a in arrays]


def states_of(rec, final):
    """x_0 .. x_T per layer, [T + 1, B, n_l]: the T records of a run and its final state."""
    return [np.concatenate([np.asarray(r), np.asarray(x)[None]]) for r, x in zip(rec, final)]


def row_maxima(states):
    """Per layer [T + 1, B]: max |x| of every chain row."""
    return [np.abs(np.asarray(s, np.float64)).max(axis=-1) for s in states]


# ---- one step in fp64, with the sum of |terms| of every element ----------------------------------------------------------------------------
def sgd_step64(case, W, b, inputs, target, xs, kicks):
    """x_{t+1} = x - g + kick (lr = 1) in fp64 from the fp32 state `xs`, by the oracle's forward and x_grads; with it, per element, the sum
    of the absolute values of the terms that make it up (x, -x, the terms of mu, |f'| times the terms of the back-projected error, the
    kick), and the read-out's outputs with theirs.  The read-out error's own terms: (|o terms| + |y|) / var under a Gaussian loss;
    |sigmoid(o)| + |y| + |o terms| / 4 under a Bernoulli one (sigmoid' <= 1 / 4)."""
    net = net_spec(case, as64(W), as64(b))
    ls = loss_spec(case, None if target is None else np.asarray(target, np.float64))
    x64 = as64(xs)
    inp = np.zeros((x64[0].shape[0], case["n_in"])) if inputs is None else np.asarray(inputs, np.float64)
    with np.errstate(over="ignore"):
        fw = mo.forward(net, inp, x64, ls)
    gs = mo.x_grads(net, x64, fw)
    L = net.L
    aW, ab = [np.abs(w) for w in net.W], [0.0 if v is None else np.abs(v) for v in net.b]
    pre = [np.abs(inp)] + [np.abs(mo._act(net.acts[l], x64[l])) for l in range(L)]
    amu = [pre[j] @ aW[j].T + ab[j] for j in range(len(aW))]
    ae = [np.abs(x64[l]) + amu[l] for l in range(L)]
    out = out_terms = None
    if net.has_head:
        out, out_terms = fw["out"], amu[L]
        if ls.kind == mo.LOSS_GAUSSIAN:
            ae.append((amu[L] + np.abs(ls.target)) / ls.var)
        elif ls.kind == mo.LOSS_BERNOULLI:
            ae.append(np.abs(fw["e_out"] + ls.target) + np.abs(ls.target) + 0.25 * amu[L])
        else:
            ae.append(np.zeros_like(amu[L]))
    nxt, terms = [], []
    for l in range(L):
        k = 0.0 if kicks is None else np.asarray(kicks[l], np.float64)
        nxt.append(x64[l] - gs[l] + k)
        t = 2.0 * np.abs(x64[l]) + amu[l] + np.abs(k)
        if l + 1 < len(ae):
            t = t + np.abs(mo._dact(net.acts[l], x64[l])) * (ae[l + 1] @ aW[l + 1])
        terms.append(t)
    return dict(x=nxt, terms=terms, out=out, out_terms=out_terms, grads=gs)


def steps_vs_fp64(case, W, b, inputs, target, states, kick_of):
    """Assertion 3 over a recorded trajectory: max over steps, layers and elements of |x_{t+1} - fp64 step from x_t| / sum |terms|."""
    worst = 0.0
    T = states[0].shape[0] - 1
    for t in range(T):
        ref = sgd_step64(case, W, b, inputs, target, [s[t] for s in states], kick_of(t))
        for l, s in enumerate(states):
            err = np.abs(np.asarray(s[t + 1], np.float64) - ref["x"][l])
            worst = max(worst, float((err / np.maximum(ref["terms"][l], 1e-300)).max()))
    return worst


def out_bound(K):
    """Assertion 2: a read-out row against fp64, relative to its own sum |terms|."""
    from tests.test_gpu_accuracy import C_OP, c_acc
    return C_OP + c_acc(K) + 2.0 ** -24


def outputs_vs_fp64(W, b, act, x_last, outs):
    """max |o - (f(x) W^T + b)| / sum |terms| over recorded outputs `outs` [T, B, n_out] of the recorded last-layer states `x_last`."""
    f = mo._act(ACT[act], np.asarray(x_last, np.float64))
    W64, b64 = np.asarray(W[-1], np.float64), np.asarray(b[-1], np.float64)
    want = f @ W64.T + b64
    terms = np.abs(f) @ np.abs(W64).T + np.abs(b64)
    return float((np.abs(np.asarray(outs, np.float64) - want) / terms).max())


def outputs_fp32(W, b, act, x_last):
    """The oracle's own fp32 evaluation of the same rows."""
    return mo._linear(mo._act(ACT[act], np.asarray(x_last, np.float32)), W[-1], b[-1])


# ================================================================================================================================
# PART A
A_T = 14
A_GAIN = 2.0 ** -24
A_ACTS = ("identity", "relu")
HI, HINEG, LO, GEMM, NONE = "hi", "hi, all negative", "lo", "gemm", "none"
CYCLE = (HI, HINEG, HI, LO, GEMM, NONE)
A_SCALE = {HI: 2.0 ** 12, HINEG: 2.0 ** 12, LO: 2.0 ** -12, GEMM: 2.0 ** -36, NONE: 0.0}
A_FLAT = 21                               # the chain whose schedule assertion 4 replaces by a constant-scale one
A_LIMITS = (2.0 ** -40, 2.0 ** 40)
TEETH = 2.0 ** 20


def a_case(act, readout=True, batch=B):
    return engine_case(f"swing-A-{act}{'' if readout else '-no_readout'}", act, N_OUT if readout else 0, "bernoulli" if readout else "none", batch)


@functools.lru_cache(maxsize=None)
def a_data(act, readout=True, batch=B):
    """(W, b, X0, inputs, target), read-only.  x_0 is in the state the schedule gives step 0."""
    rng = np.random.RandomState(1201 + 10 * A_ACTS.index(act) + (0 if readout else 5))
    dims = [N_IN] + SIZES + ([N_OUT] if readout else [])
    W = _linears(rng, dims, [A_GAIN] * (len(dims) - 1))
    b = [(_signed(rng, dims[j + 1]) * 2.0 ** -38).astype(np.float32) for j in range(len(dims) - 1)]
    inputs = _signed(rng, (batch, N_IN)).astype(np.float32)
    target = (rng.random_sample((batch, N_OUT)) < 0.5).astype(np.float32) if readout else None
    X0 = [_a_rows(rng, -1, batch, n, None) + (_signed(rng, (batch, n)) * 2.0 ** -36 * (_a_amp(-1, batch) == 0)[:, None]).astype(np.float32)
          for n in SIZES]
    _frozen(W, b, X0, inputs, target)
    return W, b, X0, inputs, target


def a_state(t, chain):
    """The state of x_t of a chain: chain c is c mod 6 states ahead of chain 0."""
    return CYCLE[(t + chain) % len(CYCLE)]


def _a_amp(t, batch):
    return np.array([A_SCALE[a_state(t + 1, c)] for c in range(batch)])


def _a_rows(rng, t, batch, n, flat):
    """The kick of step t (it makes x_{t+1}) for one layer."""
    u = _signed(rng, (batch, n))
    neg = np.array([a_state(t + 1, c) == HINEG for c in range(batch)])
    u[neg] = -np.abs(u[neg])
    amp = _a_amp(t, batch)
    if flat is not None:
        amp[flat] = 1.0
    return (u * amp[:, None]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def a_kicks(batch=B, flat=None):
    """Per layer [A_T, batch, n_l] fp32, read-only.  `flat`: that chain gets kicks of constant scale 1 (with the same signs)."""
    rng = np.random.RandomState(1301)
    out = [np.stack(ks) for ks in zip(*[[_a_rows(rng, t, batch, n, flat) for n in SIZES] for t in range(A_T)])]
    _frozen(out)
    return out


@functools.lru_cache(maxsize=None)
def a_oracle(act, readout=True, batch=B, dtype="float64"):
    """The whole call on the oracle, every state and output recorded."""
    case = a_case(act, readout, batch)
    W, b, X0, inputs, target = a_data(act, readout, batch)
    kicks = a_kicks(batch)
    # (oracle.mcpc_oracle.run's SGD step and kick with lr = 1, without its parameter gradients: 4112 chains in the round-schedule case)
    dt = np.dtype(dtype)
    net, ls = net_spec(case, W, b), loss_spec(case, target)
    xs = [np.array(x, dtype=dt) for x in X0]
    rec, outs = [], []
    for t in range(A_T):
        with np.errstate(over="ignore"):
            fw = mo.forward(net, np.asarray(inputs, dt), xs, ls)
        rec.append(xs)
        outs.append(fw["out"])
        gs = mo.x_grads(net, xs, fw)
        xs = [(x - dt.type(1.0) * g) + dt.type(1.0) * np.asarray(k[t], dt) for x, g, k in zip(xs, gs, kicks)]
    states = states_of([np.stack([r[l] for r in rec]) for l in range(len(SIZES))], xs)
    return states, np.stack(outs) if readout else None


def a_teeth(states, act, limits=A_LIMITS):
    """The conditions of Part A on recorded states x_0 .. x_T: every row maximum inside `limits`; in every 16-chain tile, at every step
    after the first, for every layer, a row whose maximum rose by at least 2^20 over the previous step and another whose fell by as much;
    under ReLU, per layer, an f(x) row that is exactly zero at step t and alive at 2^11 or more at t + 1, and the reverse.  Returns the
    extremes for a report: (smallest, largest row maximum, smallest per-tile largest rise, smallest per-tile largest fall)."""
    lo, hi, rise, fall = np.inf, 0.0, np.inf, np.inf
    for l, (s, m) in enumerate(zip(states, row_maxima(states))):
        assert np.isfinite(m).all(), f"layer {l}: a non-finite row"
        assert m.min() >= limits[0] and m.max() <= limits[1], (l, m.min(), m.max())
        lo, hi = min(lo, float(m.min())), max(hi, float(m.max()))
        ratio = m[1:] / m[:-1]
        for c0 in range(0, m.shape[1], 16):
            r = ratio[:, c0:c0 + 16]
            up, down = r.max(axis=1), r.min(axis=1)
            assert (up >= TEETH).all(), f"layer {l}, tile {c0 // 16}: no row rises by 2^20 at step {int(np.argmin(up)) + 1} (2^{np.log2(up.min()):.1f})"
            assert (down <= 1 / TEETH).all(), f"layer {l}, tile {c0 // 16}: no row falls by 2^20 at step {int(np.argmax(down)) + 1} (2^{np.log2(down.max()):.1f})"
            rise, fall = min(rise, float(up.min())), min(fall, float(1 / down.max()))
        if act == "relu":
            dead = (np.asarray(s) <= 0).all(axis=-1)
            alive = np.asarray(s).max(axis=-1) >= 2.0 ** 11
            assert (dead[:-1] & alive[1:]).any(), f"layer {l}: no f(x) row goes from exactly zero to alive at 2^12"
            assert (alive[:-1] & dead[1:]).any(), f"layer {l}: no f(x) row goes from alive at 2^12 to exactly zero"
    return lo, hi, rise, fall


def round_batch(n_cu=256):
    """The smallest whole number of 16-chain tiles whose plan is dealt into the round schedule on `n_cu` CUs, read from the plan."""
    from tests import plan_util
    for batch in range(16 * max(n_cu - 2, 1), 16 * (n_cu + 3), 16):
        if plan_util.plan(SIZES, N_OUT, batch, None, n_cu=n_cu, n_in=N_IN)["rounds"]["on"]:
            return batch
    raise AssertionError(f"no batch near {16 * n_cu} chains is dealt into rounds on {n_cu} CUs")


# ================================================================================================================================
# PART B
B_T = 8
B_SEED = 1409
B_NOISE_VAR = 2.0 ** -120
B_MOVE = 2.0 ** 4
B_MOVE_RELU = 2.0 ** 2                    # growth_relu: see the module docstring
B_REGIMES = ("growth", "growth_relu", "decay", "adam")
B_ACT = {"growth": "identity", "growth_relu": "relu", "decay": "relu", "adam": "relu"}
B_GAIN = {"growth": 2.0 ** 0.95, "growth_relu": 2.0 ** 2.5, "decay": 2.0 ** -5.3}
B_WARMUP = {"growth": 60, "decay": 200}
B_SPREAD = 0.2                            # every chain leaves the common mode by up to a fifth, its own way
B_LIMITS = {"growth": (2.0 ** -20, 2.0 ** 52), "growth_relu": (2.0 ** -18, 2.0 ** 56), "decay": (2.0 ** -52, 2.0 ** 13), "adam": (2.0 ** -14, 2.0 ** 16)}
ADAM_LR, ADAM_JUMP = 2.0 ** 12, 2.0 ** 20


def b_case(regime):
    return engine_case(f"swing-B-{regime}", B_ACT[regime], N_OUT, "bernoulli")


def b_chain_exponents(batch=B):
    """-12 .. 12 in steps of 1.6, dealt so that every 16-chain tile holds the whole range and neighbours differ by 2^11 or so."""
    return -12.0 + 24.0 * ((np.arange(batch) * 7) % 16) / 15.0


def _chain_max(xs):
    return np.max([np.abs(x).max(axis=1) for x in xs], axis=0)[:, None]


@functools.lru_cache(maxsize=None)
def b_data(regime):
    """(W, b, X0, inputs, target), read-only; inputs is None (zeros)."""
    rng = np.random.RandomState(1401 + B_REGIMES.index(regime))
    dims = [N_IN] + SIZES + [N_OUT]
    target = (rng.random_sample((B, N_OUT)) < 0.5).astype(np.float32)
    b = [np.zeros(n, np.float32) for n in dims[1:]]
    scale = 2.0 ** b_chain_exponents()[:, None]
    if regime == "adam":
        W = [((rng.random_sample((dims[j + 1], dims[j])) * 2 - 1) / np.sqrt(dims[j])).astype(np.float32) for j in range(4)]
        b = [(0.1 * _signed(rng, dims[j + 1])).astype(np.float32) for j in range(4)]
        X0 = [(_signed(rng, (B, n)) * 2.0 ** -12).astype(np.float32) for n in SIZES]
    else:
        g = B_GAIN[regime]
        if regime == "decay":
            # positive weights with row sums g, positive states: every ReLU unit stays alive and the step is a positive linear map
            W = [((0.25 + 0.75 * rng.random_sample((dims[j + 1], dims[j]))) * g / (0.625 * dims[j])).astype(np.float32) for j in range(3)]
            # one and the same target row for every chain: the bias saturates the read-out at it
            target = np.repeat(target[:1], B, axis=0)
            b[3] = (110.0 * (2.0 * target[0] - 1.0)).astype(np.float32)
        else:
            # outputs of standard deviation g per unit of input rms
            W = [((rng.random_sample((dims[j + 1], dims[j])) * 2 - 1) * g * np.sqrt(3.0 / dims[j])).astype(np.float32) for j in range(3)]
        W.append(_linears(rng, dims[3:], [2.0 ** -24])[0])
        if regime == "growth_relu":
            b[0] = (_mags(rng, SIZES[0]) * 2.0 ** -30).astype(np.float32)
            X0 = [_signed(rng, (B, n)) for n in SIZES]
        else:
            X0 = _common_mode(regime, W, b, target, rng)
        X0 = [(x * scale / _chain_max(X0)).astype(np.float32) for x in X0]
    _frozen(W, b, X0, target)
    return W, b, X0, None, target


def _common_mode(regime, W, b, target, rng):
    """A state on which one step acts as a multiplication by ONE number, the same for every layer, found by iterating the fp64 step on
    states normalised per chain (the step is homogeneous in x but for the read-out's bounded error, 2^-25 at this scale).  growth: the
    eigenvector of the largest |eigenvalue| of the linear step.  decay: the Perron vector of the positive map; it has a twin of opposite
    sign (layers exchange with their neighbours: the map is bipartite), which averaging a step with its input removes.  Every chain then
    leaves it by up to B_SPREAD, its own way."""
    case = b_case(regime)
    decay = regime == "decay"
    xs = [rng.random_sample((B, n)) + 0.1 if decay else _signed(rng, (B, n)) for n in SIZES]
    for _ in range(B_WARMUP[regime]):
        nxt = sgd_step64(case, W, b, None, target, xs, None)["x"]
        if decay:
            lam = _chain_max(nxt) / _chain_max(xs)
            nxt = [a / lam + x for a, x in zip(nxt, xs)]
        m = _chain_max(nxt)
        xs = [x / m for x in nxt]
    if decay:
        return [x * (1.0 + B_SPREAD * (rng.random_sample(x.shape) * 2 - 1)) for x in xs]
    return [x + B_SPREAD * np.abs(x).max(axis=1, keepdims=True) * _signed(rng, x.shape) for x in xs]


@functools.lru_cache(maxsize=None)
def b_kick(t, l):
    return np.sqrt(B_NOISE_VAR) * philox.layer_normals(B_SEED, t, l, 0, B, SIZES[l]).astype(np.float64)


def b_kicks_of(regime):
    return (lambda t: None) if regime == "adam" else (lambda t: [b_kick(t, l) for l in range(len(SIZES))])


@functools.lru_cache(maxsize=None)
def b_oracle(regime, dtype="float64"):
    case = b_case(regime)
    W, b, X0, _, target = b_data(regime)
    inputs = np.zeros((B, N_IN), np.float32)
    adam = regime == "adam"
    xopt = mo.XOpt(mo.OPT_ADAM, ADAM_LR) if adam else mo.XOpt(mo.OPT_SGD, 1.0)
    with np.errstate(over="ignore"):
        res = mo.run(net_spec(case, W, b), inputs, X0, loss_spec(case, target), xopt, B_T,
                     noise=None if adam else (lambda t, l: philox.layer_normals(B_SEED, t, l, 0, B, SIZES[l])), noise_var=B_NOISE_VAR,
                     record_at=range(B_T), dtype=np.dtype(dtype).type)
    return states_of([np.stack([res.rec_xs[t][l] for t in range(B_T)]) for l in range(len(SIZES))], res.xs)


def b_teeth(states, regime):
    """Every row maximum inside B_LIMITS, and
      growth, decay   every row of every layer moved by at least 2^4 at every step, the way the regime says;
      growth_relu     in every 16-chain tile, at every step, for every layer, a row rose by at least 2^2 (see the module docstring);
      adam            every row jumped by at least 2^20 at the first step.
    Returns (smallest, largest row maximum, the smallest of the moves asserted)."""
    lo, hi, move = np.inf, 0.0, np.inf
    for l, m in enumerate(row_maxima(states)):
        assert np.isfinite(m).all() and m.min() > 0, f"layer {l}: a non-finite or all-zero row"
        assert m.min() >= B_LIMITS[regime][0] and m.max() <= B_LIMITS[regime][1], (regime, l, np.log2(m.min()), np.log2(m.max()))
        lo, hi = min(lo, float(m.min())), max(hi, float(m.max()))
        ratio = m[1:] / m[:-1]
        if regime == "decay":
            ratio = 1.0 / ratio
        if regime == "adam":
            ratio = ratio[:1]
        if regime == "growth_relu":
            ratio = np.stack([ratio[:, c0:c0 + 16].max(axis=1) for c0 in range(0, ratio.shape[1], 16)], axis=1)
        want = ADAM_JUMP if regime == "adam" else B_MOVE_RELU if regime == "growth_relu" else B_MOVE
        assert ratio.min() >= want, f"{regime}, layer {l}: a move of only 2^{np.log2(ratio.min()):.2f} at step {int(np.argmin(ratio.min(axis=1))) + 1}"
        move = min(move, float(ratio.min()))
    return lo, hi, move


def adam_steps_vs_fp64(case, W, b, target, states):
    """Assertion 3 under Adam: every x_{t+1} against ONE fp64 Adam step from the recorded x_t, the moments replayed in fp64 from the
    records (the recurrences of oracle.mcpc_oracle.run).  The gradient g_s of every step so far is good to STEP_RTOL of its own sum |terms|
    (dg_s); through m = sum (1 - b1) b1^(t - s) g_s, v = sum (1 - b2) b2^(t - s) g_s^2 and x' = x - a m / (sqrt(v) / c + eps):
        |dx'| <= STEP_RTOL |x| + (a / den) dm + (a |m| / den^2) dv / (2 c sqrt(v)),   dm = sum (1 - b1) b1^(t - s) dg_s,
                                                                                      dv = sum (1 - b2) b2^(t - s) 2 |g_s| dg_s.
    Gross by construction (an element whose gradient cancels may move by lr either way: the bound says so), it sees Inf, NaN and a
    scale that is off by a power of two.  Returns the largest error / bound."""
    xo = mo.XOpt(mo.OPT_ADAM, ADAM_LR)
    T = states[0].shape[0] - 1
    L = len(states)
    m = [np.zeros(s.shape[1:]) for s in states]
    v, dm, dv = [a.copy() for a in m], [a.copy() for a in m], [a.copy() for a in m]
    worst = 0.0
    for t in range(T):
        ref = sgd_step64(case, W, b, None, target, [s[t] for s in states], None)
        c = np.sqrt(1.0 - xo.beta2 ** (t + 1))
        a = xo.lr / (1.0 - xo.beta1 ** (t + 1))
        for l in range(L):
            g = ref["grads"][l]
            dg = STEP_RTOL * (ref["terms"][l] - np.abs(states[l][t]).astype(np.float64))      # (the terms of g: one x, not two)
            m[l] = xo.beta1 * m[l] + (1 - xo.beta1) * g
            v[l] = xo.beta2 * v[l] + (1 - xo.beta2) * g * g
            dm[l] = xo.beta1 * dm[l] + (1 - xo.beta1) * dg
            dv[l] = xo.beta2 * dv[l] + (1 - xo.beta2) * 2 * np.abs(g) * dg
            den = np.sqrt(v[l]) / c + xo.eps
            x = np.asarray(states[l][t], np.float64)
            want = x - a * m[l] / den
            bound = STEP_RTOL * (np.abs(x) + np.abs(want)) + a / den * dm[l] + a * np.abs(m[l]) / den ** 2 * dv[l] / np.maximum(2 * c * np.sqrt(v[l]), 1e-300)
            err = np.abs(np.asarray(states[l][t + 1], np.float64) - want)
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    return worst


# ================================================================================================================================
# PART C
C_ORDERS = ("ascending", "descending", "peak in the middle")
C_STEP = 20                               # consecutive chunk scales are 2^20 apart
C_GAIN = 2.0 ** -3


def c_case():
    return engine_case("swing-C", "identity", N_OUT, "gaussian")


@functools.lru_cache(maxsize=None)
def c_chunks():
    """(units per chunk, number of chunks, ring slots) of the in-place plan's cut of the read-out."""
    from tests import plan_util
    p = plan_util.plan(SIZES, N_OUT, B, "ws=2", n_in=N_IN)
    chunk, ring, tiles = p["main"]["chunk"], p["main"]["ring"], p["out_pad"] // 16
    return 16 * chunk, -(-tiles // chunk), ring


def c_exponents(order, n):
    """The chunks' target scales as exponents of two, 2^20 apart and centred on 0."""
    asc = [C_STEP * i - C_STEP * (n - 1) // 2 for i in range(n)]
    if order == "ascending":
        return asc
    if order == "descending":
        return asc[::-1]
    mid = n // 2                              # the largest in the middle, the others falling away to both sides
    rank = sorted(range(n), key=lambda i: (abs(i - mid), i))
    out = [0] * n
    for r, i in enumerate(rank):
        out[i] = asc[n - 1 - r]
    return out


@functools.lru_cache(maxsize=None)
def c_data(order):
    """(W, b, X0, inputs, target, chunk_of_unit [n_out], chunk_of_latent [n_last], exponents), read-only."""
    units, n, _ = c_chunks()
    rng = np.random.RandomState(1501)
    dims = [N_IN] + SIZES + [N_OUT]
    W = [np.zeros((dims[j + 1], dims[j]), np.float32) for j in range(4)]
    b = [np.zeros(k, np.float32) for k in dims[1:]]
    unit_chunk = np.arange(N_OUT) // units
    latent_chunk = np.arange(SIZES[-1]) % n
    W[3] = (_signed(rng, (N_OUT, SIZES[-1])) * C_GAIN * (unit_chunk[:, None] == latent_chunk[None, :])).astype(np.float32)
    ex = c_exponents(order, n)
    target = (_signed(rng, (B, N_OUT)) * 2.0 ** np.asarray(ex, np.float64)[unit_chunk][None, :]).astype(np.float32)
    X0 = [np.zeros((B, k), np.float32) for k in SIZES]
    _frozen(W, b, X0, target, unit_chunk, latent_chunk)
    return W, b, X0, None, target, unit_chunk, latent_chunk, ex


def c_reference(order):
    """(want, terms, bound) [B, n_last]: the back-projection W_out^T e_o with e_o = -y in fp64, every entry's sum |terms|, and its bound
    relative to that sum: C_OP + c_acc(K) in the chunk that holds the row's maximum, max(C_OP, 2^-22 + 2^(rho - 39)) + c_acc(K) in a chunk
    2^rho below it."""
    from tests.test_gpu_accuracy import C_OP, c_acc
    W, _, _, _, target, _, latent_chunk, ex = c_data(order)
    W3, y = np.asarray(W[3], np.float64), np.asarray(target, np.float64)
    want = (-y) @ W3
    terms = np.abs(y) @ np.abs(W3)
    rho = (max(ex) - np.asarray(ex))[latent_chunk]
    bound = np.maximum(C_OP, 2.0 ** -22 + 2.0 ** (rho - 39.0)) + c_acc(N_OUT)
    return want, terms, np.broadcast_to(bound, want.shape)


# ---- the two-step variants: the chunks' scales change between the two steps' error rows ------------------------------------------------
C2_ORDERS = ("ascending", "descending", "falling")
C2_T = 2
C2_FALL_GAIN = 2.0 ** -9
C2_FALL_X0 = (26, 30, 34, 38)             # the last layer's x_0 per block of units, as exponents of two (cycled if there are more chunks):
                                          # one ROW of the read-out's forward GEMM, so inside the 2^16 below its maximum that keep 22 bits


def c2_exponents(order, n):
    """(step 0, step 1): the chunk scales of e_o = o - y as exponents of two, ascending / descending.  Step 0 is -y (x = 0): `order`, 2^20
    apart.  Step 1 adds o_1 = W_out (b_L + W_out^T y): a chunk's error can only GROW by it -- to cancel y to one part in 2^20 is beyond
    fp32 -- so the reversed order stands ON the largest chunk of step 0: that chunk keeps its scale, the others rise above it, 2^3 and
    then 2^2 apart, the smallest of step 0 highest.  (All that a ring slot's word has to get wrong is the order: the slot that held the
    2^30 chunk at step 0 takes the 2^37 one at step 1.)"""
    s0 = c_exponents(order, n)
    top = max(s0)
    by_size = sorted(range(n), key=lambda c: -s0[c])             # the largest chunk of step 0 first
    s1 = [0] * n
    for r, c in enumerate(by_size):
        s1[c] = top if r == 0 else top + 3 + 2 * (r - 1)
    return s0, s1


@functools.lru_cache(maxsize=None)
def c2_data(order):
    """(W, b, X0, inputs, target), read-only.
    ascending, descending: c_data's read-out weights and target, and a bias of the last latent layer that carries the scales of step 1
    (every other parameter zero; lr = 1: x_1 = b_L + W_out^T y).
    falling: what rising chunks cannot show -- a chunk that joins a sum takes the SMALLER of its own and the sum's exponent
    (GemmScale::run), so inside a step a word that is too large changes nothing, and across steps only a row that FELL can be hurt by
    the word of the step before.  No target, no bias, read-out weights of gain 2^-9 and an x_0 of the last layer scaled per block, 2^4
    apart: e_o = W_out x, x' = -W_out^T e_o, every chunk falls by about 2^11 per step and keeps its place."""
    _, n, _ = c_chunks()
    if order == "falling":
        W, b, X0, _, target, _, latent_chunk, _ = c_data("ascending")
        rng = np.random.RandomState(1503)
        W = list(W[:3]) + [(W[3] * np.float32(C2_FALL_GAIN / C_GAIN))]
        ex = np.asarray([C2_FALL_X0[c % len(C2_FALL_X0)] for c in range(n)], np.float64)
        X0 = list(X0[:2]) + [(_signed(rng, X0[2].shape) * 2.0 ** ex[latent_chunk][None, :]).astype(np.float32)]
        target = np.zeros_like(target)
        _frozen(W, X0, target)
        return W, b, X0, None, target
    W, b, X0, _, target, _, latent_chunk, _ = c_data(order)
    rng = np.random.RandomState(1502)
    _, s1 = c2_exponents(order, n)
    b = [v.copy() for v in b]
    # o_1 of a chunk ~ C_GAIN sqrt(latents of its block) b_L: b_L = 2^s1 / (2 C_GAIN) puts it at 2^s1 or so
    b[2] = (_signed(rng, SIZES[-1]) * 2.0 ** np.asarray(s1, np.float64)[latent_chunk] / (2.0 * C_GAIN)).astype(np.float32)
    _frozen(b)
    return W, b, X0, None, target


def c2_chunk_scales(outs, order):
    """[T, n_chunks]: the largest |e_o| = |o - y| of every chunk over all chains, from recorded outputs [T, B, n_out]."""
    unit_chunk = c_data("ascending")[5]
    e = np.abs(np.asarray(outs, np.float64) - np.asarray(c2_data(order)[4], np.float64)[None])
    return np.stack([e[:, :, unit_chunk == c].max(axis=(1, 2)) for c in range(int(unit_chunk.max()) + 1)], axis=1)


def c2_teeth(outs, order):
    """From recorded outputs.  ascending / descending: the chunks' error scales are strictly ordered one way at step 0 and strictly the
    other way at step 1, the chunk that was smallest now 2^4 or more above the one that was largest.  falling: every chunk fell by 2^8 at
    least, all inside 2^-40 .. 2^40.  Returns the scales as exponents of two."""
    s = np.log2(c2_chunk_scales(outs, order))
    d0, d1 = np.diff(s[0]), np.diff(s[1])
    if order == "falling":
        assert (s[0] - s[1] >= 8).all() and s.min() >= -40 and s.max() <= 40, s
        return s
    up = order == "ascending"
    assert ((d0 > 0) if up else (d0 < 0)).all() and ((d1 < 0) if up else (d1 > 0)).all(), s
    assert abs(s[1, 0] - s[1, -1]) >= 4 and np.abs(d0).min() >= C_STEP - 2, s
    return s


@functools.lru_cache(maxsize=None)
def c2_oracle(order, dtype="float64"):
    case = c_case()
    W, b, X0, _, target = c2_data(order)
    res = mo.run(net_spec(case, W, b), np.zeros((B, N_IN), np.float32), X0, loss_spec(case, target), mo.XOpt(mo.OPT_SGD, 1.0), C2_T,
                 record_at=range(C2_T), dtype=np.dtype(dtype).type)
    states = states_of([np.stack([res.rec_xs[t][l] for t in range(C2_T)]) for l in range(len(SIZES))], res.xs)
    return states, np.stack([res.rec_out[t] for t in range(C2_T)])

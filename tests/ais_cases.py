"""The yardsticks of annealed importance sampling: fp64 NumPy restatements of the log-weight increment (include/mcpc.h:
mcpc_ais_increment) and of the whole estimator (montecarlopredictivecoding_amd/ais.py), the bounds a device result is held to, and the
known-answer case.  Shared by tests/test_ais_host.py, tests/test_gpu_ais_increment.py and tests/test_gpu_ais.py; no device, no torch.

1. THE INCREMENT'S BOUND.  Both sides are fp64, so the bound is a roundoff bound.  With u = 2^-53 the unit roundoff,
     o_u = bias_u + sum_k f(x_rk) W_uk        is a sum of width + 1 terms whose products are exact (ReLU, identity) or rounded once
                                               (tanh, itself a few ulp): |err o_u| <= (width + c) u S_u, S_u = |bias_u| + sum_k |f(x_rk) W_uk|;
     term_u(a) = softplus(a o_u) - y a o_u     carries that error times |d term / d o_u| = |a dl/do_u| (dl/do_u = sigmoid(a o) - y, or
                 (0.5 / var) (a o_u - y)^2      (a o - y) / var), plus a few ulp of its own value for exp / log1p and the last operations;
     logw_r = sum_u c0 term0_u - c1 term1_u    is a sum of at most 2 n_out terms in one order: (2 n_out) u times the sum of their moduli.
   Hence |got - want| <= K u M_r with
     M_r = sum_u [ c0 |term0_u| + c1 |term1_u| + (|c0 a0 dl0/do_u| + |c1 a1 dl1/do_u|) S_u ]
   and K <= (width + 2 n_out + c): at most 784 + 272 terms in the project's nets, 2^10 to be safe, times 2^3 for the device's few-ulp
   exp / log1p / tanh and the reference's own roundings.  K u = 2^13 2^-53 = 2^-40: the bound is 2^-40 M_r.  It is computed from the
   inputs, not tuned.  (The old logw of accumulate = 1 adds one rounding of the result: covered by counting |logw_old| into M_r.)

2. THE ESTIMATOR.  `estimator` walks the ladder exactly as ais.run does, driven by oracle.philox.layer_normals with the same
   (seed, step, layer, chain) words the device uses -- the prior draw at step_base, transition t of rung k at
   step_base + 1 + (k - 1) * steps_per_stage + t -- and oracle.mcpc_oracle.run for the Langevin steps.  dtype=float32 rounds the state
   and the step arithmetic where the oracle rounds (what the device does); dtype=float64 does not.  The increments are fp64 in both.

   The tolerance of the device against the fp32 restatement is 10 x the largest |logw(fp32) - logw(fp64)| over the case's chains:
   the fp32 trajectory's own distance from the real-number one is the scale on which two fp32 orders of evaluation may differ.
   Measured here on the CPU (python -m tests.ais_cases tolerances):
       gauss_tanh   6-16-16 -> 24, tanh, Gaussian var 0.7, 8 rungs x 4 steps, 5 x 16 chains:  max |logw32 - logw64| = 2.21135e-06
       bern_relu    5-33-17 -> 40, ReLU, Bernoulli, mask_start 21, 8 rungs x 4 steps, 5 x 16 chains: max |logw32 - logw64| = 1.09294e-06
   (log_p moves by 4.1e-07 and 1.3e-07).  FP32_VS_FP64 holds the two numbers; tests/test_ais_host.py recomputes them.

3. THE KNOWN-ANSWER CASE (KAT).  Identity net, 2 latent units, 32 Bernoulli outputs, read-out 1.5 randn / sqrt(2), no bias; 4 data
   drawn from the model; 256 replicas, 32 rungs with power 2, 10 steps per rung, lr 0.05, noise variance 2.  The exact log p(y) is a
   2-D quadrature in fp64 (`kat_exact`: the trapezoid rule on [-9, 9]^2 with 1801^2 nodes; the integrand is a Gaussian times a smooth
   bounded factor, so the rule converges geometrically -- halving the step moves the value by less than 1e-12).
   The restatement's own absolute error max_i |log p_hat_i - exact_i| over seeds 0..7 (python -m tests.ais_cases kat), fp32 state:
       0.321474  0.296329  0.287014  0.282394  0.302501  0.304179  0.357953  0.217942      KAT_TOL = 2 x 0.357953 = 0.715906
   Every error is negative (mean -0.19): the discretisation bias of unadjusted Langevin at lr = 0.05, not noise.  Over those seeds the
   ESS of the 256 weights is 59 .. 136 per datum with AIS against 18 .. 41 for the same replicas as plain prior samples (one rung):
   the condition "AIS beats prior sampling on every datum" holds at 2 latent units (a 4-unit net gave 82 .. 135 against 9 .. 22), so
   the exact value stays a quadrature and no golden file is needed.
"""
import functools
import math
import sys

import numpy as np

from oracle import mcpc_oracle as mo
from oracle import philox

ACT = {"identity": mo.ACT_IDENTITY, "relu": mo.ACT_RELU, "tanh": mo.ACT_TANH}
LOSS = {"gaussian": mo.LOSS_GAUSSIAN, "bernoulli": mo.LOSS_BERNOULLI}
BOUND = 2.0 ** -40


# ---- 1. the increment -------------------------------------------------------------------------------------------------------------
def _f(act, x):
    x = np.asarray(x, dtype=np.float64)
    if act == "relu":
        return np.where(x < 0, 0.0, x)              # a NaN stays a NaN
    if act == "tanh":
        return np.tanh(x)
    return x


def softplus(z):
    return np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))


def _terms(a, o, y, loss, var):
    """(term, |a dl/do|) per element at scale a."""
    z = a * o
    if loss == "bernoulli":
        return softplus(z) - y * z, np.abs(a * (1.0 / (1.0 + np.exp(-z)) - y))
    return (0.5 / var) * (z - y) ** 2, np.abs(a * (z - y) / var)


def increment(x, W, bias, y, act, loss, var, mask_start, a0, c0, a1, c1, logw=None):
    """(want, M): fp64 ``[rows]`` each -- the value mcpc_ais_increment leaves in logw (``logw`` None: accumulate = 0) and the M_r of
    the bound (module docstring).  A side whose c is exactly 0 is not evaluated."""
    x, W, y = (np.asarray(t, dtype=np.float64) for t in (x, W, y))
    fx = _f(act, x)
    with np.errstate(all="ignore"):
        o = fx @ W.T
        S = np.abs(fx) @ np.abs(W).T
        if bias is not None:
            b = np.asarray(bias, dtype=np.float64)
            o, S = o + b, S + np.abs(b)
        o, S, yy = o[:, mask_start:], S[:, mask_start:], y[:, mask_start:]
        want = np.zeros(x.shape[0])
        M = np.zeros(x.shape[0])
        for a, c, sign in ((a0, c0, 1.0), (a1, c1, -1.0)):
            if c == 0.0:
                continue
            t, d = _terms(a, o, yy, loss, var)
            want = want + sign * c * t.sum(1)
            M = M + (abs(c) * np.abs(t) + abs(c) * d * S).sum(1)
        if logw is not None:
            old = np.asarray(logw, dtype=np.float64)
            want, M = old + want, M + np.abs(old)
    return want, M


INCREMENT_CASES = {
    # name: rows, width, n_out, act, loss, var, mask_start, target
    "relu_bern_masked": dict(rows=70, width=17, n_out=40, act="relu", loss="bernoulli", var=None, mask_start=21, target="uniform"),
    "relu_bern_784": dict(rows=16, width=144, n_out=784, act="relu", loss="bernoulli", var=None, mask_start=0, target="binary"),
    "tanh_gauss": dict(rows=70, width=16, n_out=24, act="tanh", loss="gaussian", var=0.7, mask_start=0, target="normal"),
    "ident_bern_small": dict(rows=5, width=2, n_out=32, act="identity", loss="bernoulli", var=None, mask_start=0, target="binary"),
    "relu_gauss_one": dict(rows=130, width=33, n_out=1, act="relu", loss="gaussian", var=1.3, mask_start=0, target="normal"),
}
# the scalars of a first rung (a0 = 0 for the scaled read-out, c0 = 0 for the geometric ladder), a middle rung and the last one
RUNGS = {
    "bernoulli": {"first": (0.0, 1.0, 1.0 / 64, 1.0), "middle": (0.25, 1.0, 0.31640625, 1.0), "last": (0.87890625, 1.0, 1.0, 1.0)},
    "gaussian": {"first": (1.0, 0.0, 1.0, 1.0 / 64), "middle": (1.0, 0.25, 1.0, 0.31640625), "last": (1.0, 0.87890625, 1.0, 1.0)},
}


@functools.lru_cache(maxsize=None)
def increment_inputs(name):
    """Seeded fp32 (x, W, bias, y, logw_old fp64) of a case; never modified."""
    c = INCREMENT_CASES[name]
    rng = np.random.default_rng([17, sorted(INCREMENT_CASES).index(name)])
    x = (1.5 * rng.standard_normal((c["rows"], c["width"]))).astype(np.float32)
    W = (1.5 * rng.standard_normal((c["n_out"], c["width"])) / np.sqrt(c["width"])).astype(np.float32)
    bias = (0.5 * rng.standard_normal(c["n_out"])).astype(np.float32)
    if c["target"] == "uniform":
        y = rng.uniform(-0.5, 1.5, (c["rows"], c["n_out"])).astype(np.float32)
    elif c["target"] == "binary":
        y = (rng.random((c["rows"], c["n_out"])) < 0.4).astype(np.float32)
    else:
        y = rng.standard_normal((c["rows"], c["n_out"])).astype(np.float32)
    old = 3.0 * rng.standard_normal(c["rows"])
    for a in (x, W, bias, y, old):
        a.setflags(write=False)
    return x, W, bias, y, old


# ---- 2. the estimator ---------------------------------------------------------------------------------------------------------------
def schedule(stages, power=2.0):
    b = [(k / stages) ** power for k in range(stages + 1)]
    b[0], b[-1] = 0.0, 1.0
    return b


def log_norm(loss, n_active, var):
    return n_active * math.log(2.0) if loss == "bernoulli" else 0.5 * n_active * math.log(2.0 * math.pi * var)


def state_from_logw(logw, replicas, const):
    """[n, 4] fp64 (m, s1, s2, cnt) per datum by a direct log-mean-exp over its finite replicas."""
    nll = -(np.asarray(logw, dtype=np.float64).reshape(-1, replicas) - const)
    ok = np.isfinite(nll)
    m = np.where(ok, nll, np.inf).min(1)
    base = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(all="ignore"):
        e = np.where(ok, np.exp(-(np.where(ok, nll, 0.0) - base[:, None])), 0.0)
    return np.stack([m, e.sum(1), (e * e).sum(1), ok.sum(1).astype(np.float64)], axis=1)


def log_p(state):
    with np.errstate(all="ignore"):
        return np.where(state[:, 3] > 0, np.log(state[:, 1] / state[:, 3]) - state[:, 0], np.nan)


def ess(state):
    with np.errstate(all="ignore"):
        return np.where(state[:, 3] > 0, state[:, 1] ** 2 / state[:, 2], np.nan)


def estimator(W, b, sizes, acts, n_in, data, loss, var, mask_start, *, replicas, betas, steps_per_stage, lr, noise_var=2.0, seed=0,
              step_base=0, chain_base=0, dtype=np.float32):
    """(logw fp64 [N * replicas], state [N, 4]) of ais.run on a network given as lists of fp32 weights (torch layout) and biases, the
    last pair the read-out.  One chunk: the device's result does not depend on the chunking."""
    dt = np.dtype(dtype)
    L = len(sizes)
    data = np.asarray(data, dtype=np.float32)
    B = data.shape[0] * replicas
    y = np.repeat(data, replicas, axis=0)
    a_prev = np.zeros((B, n_in), dtype=dt)
    xs = []
    for j in range(L):                                                   # the ancestral draw (include/mcpc.h: mcpc_sample_prior, ecoef 1)
        mu = mo._linear(a_prev, W[j].astype(dt), None if b[j] is None else b[j].astype(dt))
        z = philox.layer_normals(seed, step_base, j, chain_base, B, sizes[j]).astype(dt)
        xs.append((mu + z).astype(dt))
        a_prev = mo._act(ACT[acts[j]], xs[j])
    inputs = np.zeros((B, n_in), dtype=np.float32)
    logw = np.zeros(B)
    K = len(betas) - 1
    for k in range(1, K + 1):
        sc = (betas[k - 1], 1.0, betas[k], 1.0) if loss == "bernoulli" else (1.0, betas[k - 1], 1.0, betas[k])
        logw, _ = increment(xs[-1], W[L], b[L], y, acts[-1], loss, var, mask_start, *sc, logw=logw)
        if k == K:
            break
        if loss == "bernoulli":                                          # the scaled read-out: an fp32 scratch copy, as the device's
            Wk = list(W[:L]) + [(W[L] * np.float32(betas[k])).astype(np.float32)]
            bk = list(b[:L]) + [None if b[L] is None else (b[L] * np.float32(betas[k])).astype(np.float32)]
            run_var = 1.0
        else:
            Wk, bk, run_var = W, b, var / betas[k]
        net = mo.NetSpec(sizes=list(sizes), acts=[ACT[a] for a in acts], W=list(Wk), b=list(bk))
        sb = step_base + 1 + (k - 1) * steps_per_stage
        res = mo.run(net, inputs, xs, mo.LossSpec(LOSS[loss], y, run_var, mask_start), mo.XOpt(mo.OPT_SGD, lr), steps_per_stage,
                     noise=lambda t, l, sb=sb: philox.layer_normals(seed, sb + t, l, chain_base, B, sizes[l]), noise_var=noise_var,
                     dtype=dt)
        xs = res.xs
    n_active = data.shape[1] - mask_start
    return logw, state_from_logw(logw, replicas, log_norm(loss, n_active, var))


ESTIMATOR_CASES = {
    "gauss_tanh": dict(n_in=6, sizes=(16, 16), n_out=24, act="tanh", loss="gaussian", var=0.7, perc=None, mask_start=0),
    "bern_relu": dict(n_in=5, sizes=(33, 17), n_out=40, act="relu", loss="bernoulli", var=None, perc=19 / 40, mask_start=21),
}
ESTIMATOR_RUN = dict(replicas=16, stages=8, steps_per_stage=4, lr=0.03, noise_var=2.0, seed=4321, step_base=100)
N_DATA = 5
# max |logw(fp32 restatement) - logw(fp64 restatement)| over the 80 chains of each case (python -m tests.ais_cases tolerances);
# the device is held to 10 x this against the fp32 restatement
FP32_VS_FP64 = {"gauss_tanh": 2.21135e-06, "bern_relu": 1.09294e-06}


@functools.lru_cache(maxsize=None)
def estimator_params(name):
    """Seeded fp32 weights, biases and data of a case; never modified."""
    c = ESTIMATOR_CASES[name]
    rng = np.random.default_rng([23, sorted(ESTIMATOR_CASES).index(name)])
    dims = [c["n_in"], *c["sizes"], c["n_out"]]
    W = [(rng.standard_normal((o, i)) / np.sqrt(i)).astype(np.float32) for i, o in zip(dims[:-1], dims[1:])]
    b = [(0.3 * rng.standard_normal(o)).astype(np.float32) for o in dims[1:]]
    if c["loss"] == "bernoulli":
        data = (rng.random((N_DATA, c["n_out"])) < 0.4).astype(np.float32)
    else:
        data = rng.standard_normal((N_DATA, c["n_out"])).astype(np.float32)
    for a in (*W, *b, data):
        a.setflags(write=False)
    return W, b, data


@functools.lru_cache(maxsize=None)
def estimator_reference(name, dtype="float32", chain_base=0, replicas=None):
    c = ESTIMATOR_CASES[name]
    W, b, data = estimator_params(name)
    r = dict(ESTIMATOR_RUN)
    if replicas is not None:
        r["replicas"] = replicas
    stages = r.pop("stages")
    return estimator(W, b, c["sizes"], [c["act"]] * len(c["sizes"]), c["n_in"], data, c["loss"], c["var"], c["mask_start"],
                     betas=schedule(stages), chain_base=chain_base, dtype=np.dtype(dtype), **r)


def estimator_tolerance(name):
    t = FP32_VS_FP64[name]
    assert t is not None, "FP32_VS_FP64 is not filled in"
    return 10.0 * t


# ---- 3. the known-answer case -----------------------------------------------------------------------------------------------------
KAT = dict(n_latent=2, n_out=32, n_data=4, replicas=256, stages=32, power=2.0, steps_per_stage=10, lr=0.05, noise_var=2.0)
# max_i |log p_hat_i - exact_i| of the fp32 restatement for seeds 0..7 (python -m tests.ais_cases kat)
KAT_ERRORS = (0.321474, 0.296329, 0.287014, 0.282394, 0.302501, 0.304179, 0.357953, 0.217942)
KAT_TOL = 2.0 * max(KAT_ERRORS)


@functools.lru_cache(maxsize=None)
def kat_params():
    """(W [Linear 0: zeros, read-out], b [zeros, None], data [4, 32]): x ~ N(0, I_2), y ~ Bernoulli(sigmoid(W x)); never modified."""
    rng = np.random.default_rng(2001)
    n, n_out = KAT["n_latent"], KAT["n_out"]
    W_L = (1.5 * rng.standard_normal((n_out, n)) / np.sqrt(n)).astype(np.float32)
    x_true = rng.standard_normal((KAT["n_data"], n))
    p = 1.0 / (1.0 + np.exp(-(x_true @ W_L.astype(np.float64).T)))
    data = (rng.random(p.shape) < p).astype(np.float32)
    W = [np.zeros((n, 1), dtype=np.float32), W_L]
    b = [np.zeros(n, dtype=np.float32), None]
    for a in (*W, b[0], data):
        a.setflags(write=False)
    return W, b, data


@functools.lru_cache(maxsize=None)
def kat_exact(nodes=1801, half_width=9.0):
    """fp64 [4]: log p(y_i) = log int N(x; 0, I) prod_u Bernoulli(y_iu | sigmoid(W_u x)) dx by the trapezoid rule."""
    W, _, data = kat_params()
    g = np.linspace(-half_width, half_width, nodes)
    h = g[1] - g[0]
    w1 = np.full(nodes, h)
    w1[0] = w1[-1] = 0.5 * h
    yT = data.astype(np.float64).T
    parts = []
    for i0 in range(0, nodes, 64):                                        # rows of the grid, 64 at a time
        gi, wi = g[i0:i0 + 64], w1[i0:i0 + 64]
        X = np.stack(np.meshgrid(gi, g, indexing="ij"), axis=-1).reshape(-1, 2)
        o = X @ W[1].astype(np.float64).T                                 # [nodes in the block, n_out]
        t = (-0.5 * (X * X).sum(1) - math.log(2.0 * math.pi) - softplus(o).sum(1) + np.log(np.outer(wi, w1).reshape(-1)))[:, None] + o @ yT
        parts.append(t)
    t = np.concatenate(parts, axis=0)                                     # [nodes^2, n_data]
    m = t.max(0)
    return m + np.log(np.exp(t - m).sum(0))


@functools.lru_cache(maxsize=None)
def kat_run(seed=0, stages=None, dtype="float32"):
    """(logw, state) of the restatement on the KAT; ``stages=1``: the same replicas as plain prior samples (one rung)."""
    W, b, data = kat_params()
    betas = schedule(KAT["stages"] if stages is None else stages, KAT["power"])
    return estimator(W, b, (KAT["n_latent"],), ["identity"], 1, data, "bernoulli", None, 0, replicas=KAT["replicas"], betas=betas,
                     steps_per_stage=KAT["steps_per_stage"], lr=KAT["lr"], noise_var=KAT["noise_var"], seed=seed, dtype=np.dtype(dtype))


def _main(what):
    if what == "tolerances":
        for name in sorted(ESTIMATOR_CASES):
            l32, s32 = estimator_reference(name, "float32")
            l64, s64 = estimator_reference(name, "float64")
            print(name, "max |logw32 - logw64| = %.6g" % np.abs(l32 - l64).max(), " max |log_p32 - log_p64| = %.6g" % np.abs(log_p(s32) - log_p(s64)).max(),
                  " ess", np.round(ess(s32), 1))
    elif what == "kat":
        exact = kat_exact()
        print("exact", exact, " (901 nodes: moves by %.3g)" % np.abs(kat_exact(901) - exact).max())
        for seed in range(8):
            _, st = kat_run(seed)
            _, st1 = kat_run(seed, stages=1)
            print("seed %d  max |err| = %.6f   err %s   ESS ais %s   ESS prior %s" % (
                seed, np.abs(log_p(st) - exact).max(), np.round(log_p(st) - exact, 4), np.round(ess(st), 1), np.round(ess(st1), 1)))


if __name__ == "__main__":
    _main(sys.argv[1] if len(sys.argv) > 1 else "kat")

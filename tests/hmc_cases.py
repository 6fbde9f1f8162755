"""The yardsticks of the Hamiltonian transition of L leapfrog steps (include/mcpc.h: mcpc_hmc_begin, mcpc_hmc_leap, mcpc_hmc_accept;
csrc/mcpc_hmc.h) and of annealed importance sampling with it (montecarlopredictivecoding_amd/ais.py, adjust="mala", leapfrog=L): NumPy
restatements, the seeded kernel cases, the bounds a device result is held to, and the figures measured on the CPU.  Shared by
tests/test_hmc_host.py, tests/test_gpu_hmc_kernels.py and tests/test_gpu_hmc_ais.py; no device, no torch.  Modelled on
tests/mala_cases.py, whose nets, cases and conventions it takes over, and on tests/smc_cases.py for the closed-form case.

1. THE ELEMENTS.  With eps = sqrt(2 lr) and h = eps / 2, in fp32 with eps rounded once from the double and every operation rounded on
   its own (NumPy has no fma): exactly what csrc/mcpc_hmc.h states, so the device is held to them BITWISE.
     `begin(x, g, z, lr)`          p = z,  q = fl(p - fl(h g)),  x_1 = fl(x + fl(eps q))                 -> (q, x_1)
     `leap(xt, q, gt, lr)`         q = fl(q - fl(eps g_t)),  x_{t+1} = fl(x_t + fl(eps q))               -> (q, x_{t+1})
     `end_momentum(q, gt, lr)`     p' = fl(q - fl(h g_t))
   One leapfrog step ends at x + eps z - (eps^2 / 2) g = x - lr g + sqrt(2 lr) z, the MALA proposal at noise_var = 2.

2. THE DECISION.  `kinetic(ps)` = 0.5 sum_u p_u^2 in fp64; `log_alpha(E, Et, K0, ps)` = ((E - E_t) + (K0 - K1), M) with K1 =
   kinetic(p'); `uniform(seed, step, chain0, B)` is word 0 of the Philox block of layer 0xFD, group 0, through u32_to_unit_open0.
   accept = log(u) < log_alpha (mala_cases.decide).

   THE BOUND of K0 and log_alpha.  Both sides (the kernel, this restatement) start from the SAME fp32 values p_u: BEGIN's p is the
   normal itself, ACCEPT's p' is the bitwise restated fp32 value.  eps = 2^-53.
     - (double)p (double)p is exact: 24 + 24 <= 53 significant bits.
     - A sum of N non-negative fp64 terms in ANY order (the kernel: N / 64 per lane, then six butterfly levels; NumPy: pairwise) is
       within (N - 1) eps (1 + O(N eps)) of sum_u p_u^2; the product by 0.5 is exact.  So |err K| <= (N - 1) eps K for either side.
     - E - E_t, K0 - K1 and their sum are three roundings of quantities bounded by M_r = |E| + |E_t| + K0 + K1: 3 eps M_r.
       K0 itself is an INPUT of ACCEPT (the same bits on both sides), so only K1 carries a summation error there.
   Hence |got - exact| <= (N - 1) eps K1 + 3 eps M_r <= (N + 2) eps M_r for either side and 2 (N + 2) eps M_r between the two; for K0
   of BEGIN, 2 (N - 1) eps K0.  MALA's count was N + 10; with N + 10 <= 2^11, i.e. N <= 2038, the bound 2 * 2^11 * 2^-53 M_r = 2^-41 M_r
   holds here with 8 eps M_r to spare for the second-order terms.  `BOUND = 2^-41`, MAX_UNITS = 2038 as in mala_cases: derived, and
   it does carry over.  Computed from the inputs, not tuned.

   A DECISION is safe when |log u - log_alpha| exceeds that bound plus the error of the device's fp64 log, 4 ulp of |log u|
   (`margin_needed`).  tests/test_hmc_host.py asserts that every chain of every kernel case is that far away and that between a
   quarter and three quarters of the chains accept; then the device's decisions must equal the restatement's, all of them.

3. THE KERNEL CASES (`KERNEL_CASES` = mala_cases' shapes, `kernel_inputs`).  (x, g, E) is a state; (q, x_t) is BEGIN from it with NumPy
   normals p0, K0 = kinetic(p0); g_t is unrelated to g; E_t is set so that log_alpha = -delta with delta ~ N(0, 2^2), -3 (accepts
   whatever u is) or +40 (rejects whatever u is).  step = 2^32 + 7, chain_base = 1000.   python -m tests.hmc_cases kernels
       three_layers     accepted 12 of 19   min margin 0.609   needed at most 5.96e-11
       one_row_accepts  accepted 1 of 1     min margin 3.25    needed at most 4.95e-11
       one_row_rejects  accepted 0 of 1     min margin 39.7    needed at most 7.54e-11
       one_unit         accepted 13 of 19   min margin 0.124   needed at most 3.3e-11
       six_layers       accepted 13 of 19   min margin 0.134   needed at most 1.83e-10

4. THE ESTIMATOR.  `estimator(..., leapfrog)`: leapfrog=1 IS mala_cases.estimator(adjust="mala").  Otherwise `leapfrog_ladder`: the same
   ladder, prior draw and increments; per rung g and E at the current state, then per transition BEGIN with the normals of its Philox step, L - 1 times
   (oracle gradient at x_t, LEAP), the oracle's gradient and mala_cases.chain_energy at the end, the decision with the uniform of that
   step.  Returns (logw, state, accepted [K - 1][B] counts, the smallest |log u - log_alpha| met).
   ais_cases' two estimator nets at lr = 0.1, leapfrog = 3 (`ESTIMATOR_RUN`), python -m tests.hmc_cases tolerances:
       bern_relu    accepted 74.8 %   chains whose fp32 / fp64 decisions differ: 0 of 80   max |logw32 - logw64| = 2.22574e-07   min margin 8.7e-05
       gauss_tanh   accepted 83.0 %   chains whose fp32 / fp64 decisions differ: 0 of 80   max |logw32 - logw64| = 4.58575e-07   min margin 2.3e-05
   The device is held to 10 x that on the chains whose accepted counts per rung equal the fp32 restatement's; at most 4 of 80 may
   differ and are left out.  With one leapfrog step and MALA's uniform (`leapfrog_ladder(leapfrog=1, uniform_of=mala_cases.uniform)`)
   the fp64 ladder takes the MALA restatement's decisions on both nets and their log-weights agree within 1.5e-14: the scheme is a
   strict generalisation (tests/test_hmc_host.py asserts it at 1e-12).  The decisions of a trajectory take their uniform from layer
   0xFD, not MALA's 0xFF, so every figure recorded here is that of another stream of uniforms than a figure measured with
   mala_cases.uniform would be (the closed-form case below then gives rms 0.650450, largest error 1.5996).

5. THE KAT (ais_cases.KAT) at lr = 0.15, leapfrog = 5, steps_per_stage = 2: ten gradient evaluations per rung, as the existing KAT.
   max_i |log p_hat_i - exact_i| of the fp32 restatement for seeds 0..7 (python -m tests.hmc_cases kat):
       0.172747 0.422875 0.239095 0.286764 0.223637 0.255579 0.321306 0.169418    mean signed error -0.031   acceptance 0.922
   KAT_TOL = 2 x the largest = 0.845750 (the KAT's existing rule); it is below the smallest unadjusted error 0.874240 (mala_cases.
   KAT_UNADJUSTED_ERRORS): a device that does not adjust cannot pass.  MALA's own errors there are smaller (0.04 .. 0.11): on this 2-D
   case MALA already mixes and the long trajectory buys nothing.  The case tests exactness, not gain.

6. THE CLOSED-FORM CASE (smc_cases.CF: 16 latent units, 24 Gaussian outputs, 4 data x 64 replicas, 16 rungs, lr 0.02, no resampling),
   five gradient evaluations per rung both ways, fp32 restatement, seeds 0..7 (python -m tests.hmc_cases cf):
       5 MALA steps per rung                  pooled rms error 2.551402   largest 4.4896   final ESS of 64: 1.0 .. 5.8    acceptance 0.973
       1 trajectory of 5 leapfrog steps       pooled rms error 0.687456   largest 1.4973   final ESS of 64: 1.5 .. 10.4   acceptance 0.969
   The device with leapfrog=5, steps_per_stage=1 must stay within cf_tol() = 2 x max(CF_ERRORS) per datum and its pooled rms below
   cf_rms_bound() = 1.3244, the geometric mean of the two rms figures (smc_cases' rule): a device that quietly runs one leapfrog step, or
   plain MALA, cannot pass.
"""
import functools
import math
import sys

import numpy as np

from oracle import mcpc_oracle as mo
from oracle import philox
from tests import ais_cases as A
from tests import mala_cases as M
from tests import smc_cases as S

MAX_LATENT = M.MAX_LATENT
UNIFORM_LAYER = 0xFD
BOUND = 2.0 ** -41
MAX_UNITS = 2038
LOG_ULPS = M.LOG_ULPS


# ---- 1. the elements --------------------------------------------------------------------------------------------------------------
def step_sizes(lr, dtype=np.float32):
    """(eps, h) in ``dtype``: eps = sqrt(2 lr) formed in double and rounded once, h = eps / 2 (exact)."""
    dt = np.dtype(dtype)
    eps = dt.type(np.sqrt(2.0 * float(lr)))
    return eps, dt.type(dt.type(0.5) * eps)


def begin(x, g, z, lr, dtype=np.float32):
    """(q, x_1) of one layer: p = z, q = p - h g, x_1 = x + eps q; every operation rounded in ``dtype``."""
    dt = np.dtype(dtype)
    eps, h = step_sizes(lr, dt)
    x, g, p = (np.asarray(t, dtype=dt) for t in (x, g, z))
    t = (h * g).astype(dt)
    q = (p - t).astype(dt)
    d = (eps * q).astype(dt)
    return q, (x + d).astype(dt)


def leap(xt, q, gt, lr, dtype=np.float32):
    """(q, x_{t+1}) of one layer: q = q - eps g_t, x_{t+1} = x_t + eps q."""
    dt = np.dtype(dtype)
    eps, _ = step_sizes(lr, dt)
    xt, q, gt = (np.asarray(t, dtype=dt) for t in (xt, q, gt))
    t = (eps * gt).astype(dt)
    q = (q - t).astype(dt)
    d = (eps * q).astype(dt)
    return q, (xt + d).astype(dt)


def end_momentum(q, gt, lr, dtype=np.float32):
    """p' of one layer: q - h g_t."""
    dt = np.dtype(dtype)
    _, h = step_sizes(lr, dt)
    q, gt = (np.asarray(t, dtype=dt) for t in (q, gt))
    t = (h * gt).astype(dt)
    return (q - t).astype(dt)


# ---- 2. the decision --------------------------------------------------------------------------------------------------------------
def kinetic(ps):
    """fp64 ``[rows]``: 0.5 sum_u p_u^2 over the layers of ``ps`` (a list of ``[rows, n_l]`` arrays)."""
    s = np.zeros(ps[0].shape[0])
    with np.errstate(all="ignore"):
        for p in ps:
            p = np.asarray(p, dtype=np.float64)
            s = s + (p * p).sum(1)
        return 0.5 * s


def log_alpha(E, Et, K0, ps):
    """(log_alpha, M): fp64 ``[rows]`` each; ``ps`` is the momentum at the trajectory's end (``end_momentum`` per layer)."""
    E, Et, K0 = (np.asarray(t, dtype=np.float64) for t in (E, Et, K0))
    K1 = kinetic(ps)
    with np.errstate(all="ignore"):
        la = (E - Et) + (K0 - K1)
        Mr = np.abs(E) + np.abs(Et) + K0 + K1
    return la, Mr


def uniform(seed, step, chain0, n_chains):
    """fp64 ``[n_chains]``: the decision's uniforms in (0, 1], exact fp32 values."""
    w = philox.layer_u32(seed, step, UNIFORM_LAYER, chain0, n_chains, 1)[:, 0]
    return philox.u32_to_unit_open0(w).astype(np.float64)


decide = M.decide


def margin_needed(Mr, u):
    """What |log u - log_alpha| must exceed for a decision to be safe from roundoff."""
    return BOUND * Mr + LOG_ULPS * 2.0 ** -52 * np.abs(np.log(u))


# ---- 3. the kernel cases ----------------------------------------------------------------------------------------------------------
KERNEL_RUN = dict(lr=0.1, seed=0xC0FFEE12345, step=(1 << 32) + 7, chain_base=1000)
KERNEL_CASES = {name: dict(c) for name, c in M.KERNEL_CASES.items()}
SHARE_CASES = M.SHARE_CASES


@functools.lru_cache(maxsize=None)
def kernel_inputs(name):
    """Seeded (xs, gs, E, xts, gts, Et, qs, K0) of a case: fp32 lists and fp64 ``[rows]``; never modified."""
    c = KERNEL_CASES[name]
    rng = np.random.default_rng([31, sorted(KERNEL_CASES).index(name)])
    rows, lr = c["rows"], KERNEL_RUN["lr"]
    xs = [(1.5 * rng.standard_normal((rows, n))).astype(np.float32) for n in c["widths"]]
    gs = [rng.standard_normal((rows, n)).astype(np.float32) for n in c["widths"]]
    p0 = [rng.standard_normal((rows, n)).astype(np.float32) for n in c["widths"]]
    pairs = [begin(x, g, p, lr) for x, g, p in zip(xs, gs, p0)]
    qs, xts = [p[0] for p in pairs], [p[1] for p in pairs]
    gts = [rng.standard_normal((rows, n)).astype(np.float32) for n in c["widths"]]
    K0 = kinetic(p0)
    E = 30.0 + 3.0 * rng.standard_normal(rows)
    delta = 2.0 * rng.standard_normal(rows) if c["delta"] is None else np.full(rows, c["delta"])
    dk, _ = log_alpha(np.zeros(rows), np.zeros(rows), K0, [end_momentum(q, gt, lr) for q, gt in zip(qs, gts)])      # K0 - K1
    Et = E + dk + delta                                                               # log_alpha = E - Et + dk = -delta (but for roundoff)
    for a in (*xs, *gs, *xts, *gts, *qs, E, Et, K0):
        a.setflags(write=False)
    return xs, gs, E, xts, gts, Et, qs, K0


def kernel_reference(name):
    """(log_alpha, M, u, accepted) of a case."""
    c = KERNEL_CASES[name]
    _, _, E, _, gts, Et, qs, K0 = kernel_inputs(name)
    la, Mr = log_alpha(E, Et, K0, [end_momentum(q, gt, KERNEL_RUN["lr"]) for q, gt in zip(qs, gts)])
    u = uniform(KERNEL_RUN["seed"], KERNEL_RUN["step"], KERNEL_RUN["chain_base"], c["rows"])
    return la, Mr, u, decide(la, u)


# ---- 4. the estimator -------------------------------------------------------------------------------------------------------------
def estimator(W, b, sizes, acts, n_in, data, loss, var, mask_start, *, replicas, betas, steps_per_stage, lr, leapfrog=1, noise_var=2.0,
              seed=0, step_base=0, chain_base=0, dtype=np.float32):
    """mala_cases.estimator(adjust="mala") with ``leapfrog``: 1 is that function itself; L >= 2 is ``leapfrog_ladder``.  (logw, state,
    accepted ``[K - 1][B]`` int64 counts, smallest |log u - log_alpha|)."""
    kw = dict(replicas=replicas, betas=betas, steps_per_stage=steps_per_stage, lr=lr, noise_var=noise_var, seed=seed, step_base=step_base,
              chain_base=chain_base, dtype=dtype)
    if leapfrog == 1:
        return M.estimator(W, b, sizes, acts, n_in, data, loss, var, mask_start, adjust="mala", **kw)
    return leapfrog_ladder(W, b, sizes, acts, n_in, data, loss, var, mask_start, leapfrog=leapfrog, **kw)


def leapfrog_ladder(W, b, sizes, acts, n_in, data, loss, var, mask_start, *, replicas, betas, steps_per_stage, lr, leapfrog, noise_var=2.0,
                    seed=0, step_base=0, chain_base=0, dtype=np.float32, uniform_of=None):
    """The ladder with every transition a trajectory of ``leapfrog`` >= 1 leapfrog steps.  ``uniform_of``: the decisions' uniforms,
    ``uniform`` (layer 0xFD) unless given -- with mala_cases.uniform and leapfrog = 1 the fp64 ladder decides as MALA's does."""
    if isinstance(leapfrog, bool) or not isinstance(leapfrog, int) or leapfrog < 1 or noise_var != 2.0:
        raise ValueError((leapfrog, noise_var))
    uniform_of = uniform if uniform_of is None else uniform_of
    dt = np.dtype(dtype)
    L = len(sizes)
    data = np.asarray(data, dtype=np.float32)
    B = data.shape[0] * replicas
    y = np.repeat(data, replicas, axis=0)
    a_prev = np.zeros((B, n_in), dtype=dt)
    xs = []
    for j in range(L):                                                      # the ancestral draw, as ais_cases.estimator makes it
        mu = mo._linear(a_prev, W[j].astype(dt), None if b[j] is None else b[j].astype(dt))
        z = philox.layer_normals(seed, step_base, j, chain_base, B, sizes[j]).astype(dt)
        xs.append((mu + z).astype(dt))
        a_prev = mo._act(A.ACT[acts[j]], xs[j])
    inputs = np.zeros((B, n_in), dtype=dt)
    logw = np.zeros(B)
    K = len(betas) - 1
    accepted = np.zeros((K - 1, B), dtype=np.int64)
    margin = np.inf
    for k in range(1, K + 1):
        sc = (betas[k - 1], 1.0, betas[k], 1.0) if loss == "bernoulli" else (1.0, betas[k - 1], 1.0, betas[k])
        logw, _ = A.increment(xs[-1], W[L], b[L], y, acts[-1], loss, var, mask_start, *sc, logw=logw)
        if k == K:
            break
        if loss == "bernoulli":
            Wk = list(W[:L]) + [(W[L] * np.float32(betas[k])).astype(np.float32)]
            bk = list(b[:L]) + [None if b[L] is None else (b[L] * np.float32(betas[k])).astype(np.float32)]
            run_var = 1.0
        else:
            Wk, bk, run_var = W, b, var / betas[k]
        net = mo.NetSpec(sizes=list(sizes), acts=[A.ACT[a] for a in acts], W=list(Wk), b=list(bk))
        spec = mo.LossSpec(A.LOSS[loss], y, run_var, mask_start)
        E, fw = M.chain_energy(net, inputs, xs, spec)
        g = mo.x_grads(net, xs, fw)
        for t in range(steps_per_stage):
            step = step_base + 1 + (k - 1) * steps_per_stage + t
            p0 = [philox.layer_normals(seed, step, l, chain_base, B, sizes[l]).astype(dt) for l in range(L)]
            K0 = kinetic(p0)
            pairs = [begin(xs[l], g[l], p0[l], lr, dt) for l in range(L)]
            q, xt = [p[0] for p in pairs], [p[1] for p in pairs]
            for _ in range(leapfrog - 1):                                   # interior points: the gradient alone
                gt = mo.x_grads(net, xt, mo.forward(net, inputs, xt, spec))
                pairs = [leap(xt[l], q[l], gt[l], lr, dt) for l in range(L)]
                q, xt = [p[0] for p in pairs], [p[1] for p in pairs]
            Et, fwt = M.chain_energy(net, inputs, xt, spec)
            gt = mo.x_grads(net, xt, fwt)
            la, _ = log_alpha(E, Et, K0, [end_momentum(q[l], gt[l], lr, dt) for l in range(L)])
            u = uniform_of(seed, step, chain_base, B)
            acc = decide(la, u)
            with np.errstate(all="ignore"):
                margin = min(margin, float(np.nanmin(np.abs(np.log(u) - la))))
            xs = [np.where(acc[:, None], p, x) for p, x in zip(xt, xs)]
            g = [np.where(acc[:, None], p, x) for p, x in zip(gt, g)]
            E = np.where(acc, Et, E)
            accepted[k - 1] += acc
    n_active = data.shape[1] - mask_start
    return logw, A.state_from_logw(logw, replicas, A.log_norm(loss, n_active, var)), accepted, margin


ESTIMATOR_RUN = dict(M.ESTIMATOR_RUN, leapfrog=3)
# max |logw(fp32) - logw(fp64)| of the leapfrog restatement over the 80 chains of each case, none of which decides differently in the
# two, and the share of accepted trajectories (python -m tests.hmc_cases tolerances); the device is held to 10 x the former on the
# chains that decide as the fp32 restatement does
FP32_VS_FP64 = {"gauss_tanh": 4.58575e-07, "bern_relu": 2.22574e-07}
FP32_VS_FP64_FLIPS = {"gauss_tanh": 0, "bern_relu": 0}
ACCEPTANCE = {"gauss_tanh": 0.830, "bern_relu": 0.748}
MAX_FLIPPED = M.MAX_FLIPPED


@functools.lru_cache(maxsize=None)
def estimator_reference(name, dtype="float32", chain_base=0, replicas=None, lr=None, leapfrog=None):
    c = A.ESTIMATOR_CASES[name]
    W, b, data = A.estimator_params(name)
    r = dict(ESTIMATOR_RUN)
    for key, v in (("replicas", replicas), ("lr", lr), ("leapfrog", leapfrog)):
        if v is not None:
            r[key] = v
    stages = r.pop("stages")
    return estimator(W, b, c["sizes"], [c["act"]] * len(c["sizes"]), c["n_in"], data, c["loss"], c["var"], c["mask_start"],
                     betas=A.schedule(stages), chain_base=chain_base, dtype=np.dtype(dtype), **r)


def estimator_tolerance(name):
    return 10.0 * FP32_VS_FP64[name]


# ---- 5. the known-answer case -------------------------------------------------------------------------------------------------------
KAT_RUN = dict(lr=0.15, leapfrog=5, steps_per_stage=2)
# max_i |log p_hat_i - exact_i| of the fp32 restatement for seeds 0..7 (python -m tests.hmc_cases kat)
KAT_ERRORS = (0.172747, 0.422875, 0.239095, 0.286764, 0.223637, 0.255579, 0.321306, 0.169418)
KAT_TOL = 2.0 * max(KAT_ERRORS)


@functools.lru_cache(maxsize=None)
def kat_run(seed=0, dtype="float32"):
    """The restatement on ais_cases' KAT with KAT_RUN: what ``estimator`` returns."""
    W, b, data = A.kat_params()
    K = A.KAT
    return estimator(W, b, (K["n_latent"],), ["identity"], 1, data, "bernoulli", None, 0, replicas=K["replicas"],
                     betas=A.schedule(K["stages"], K["power"]), noise_var=K["noise_var"], seed=seed, dtype=np.dtype(dtype), **KAT_RUN)


def kat_errors(seeds=range(8)):
    """(per-seed max |error|, mean signed error, mean acceptance)."""
    exact = A.kat_exact()
    errs, signed, acc = [], [], []
    for seed in seeds:
        res = kat_run(seed)
        e = A.log_p(res[1]) - exact
        errs.append(float(np.abs(e).max()))
        signed.append(float(e.mean()))
        acc.append(res[2].mean() / KAT_RUN["steps_per_stage"])
    return errs, float(np.mean(signed)), float(np.mean(acc))


# ---- 6. the closed-form case ----------------------------------------------------------------------------------------------------------
CF = S.CF
CF_SEEDS = S.CF_SEEDS
CF_RUNS = {"hmc": dict(leapfrog=5, steps_per_stage=1), "mala": dict(leapfrog=1, steps_per_stage=5)}
# rms error pooled over seeds x data of the fp32 restatement, and the per-seed max_i |log p_hat_i - exact_i| of the "hmc" run
# (python -m tests.hmc_cases cf)
CF_RMS = {"hmc": 0.687456, "mala": 2.551402}
CF_ERRORS = (1.380674, 1.497337, 1.029077, 0.523407, 1.182757, 0.876123, 1.323301, 1.286670)


def cf_tol():
    return 2.0 * max(CF_ERRORS)


def cf_rms_bound():
    return math.sqrt(CF_RMS["hmc"] * CF_RMS["mala"])


@functools.lru_cache(maxsize=None)
def cf_run(seed=0, which="hmc", dtype="float32"):
    """(logw, state, accepted, margin) of the restatement on smc_cases' closed-form case, without resampling."""
    W, b, data = S.cf_params()
    return estimator(W, b, (CF["n_latent"],), ["identity"], 1, data, "gaussian", CF["var"], 0, replicas=CF["replicas"],
                     betas=A.schedule(CF["stages"], CF["power"]), lr=CF["lr"], noise_var=CF["noise_var"], seed=seed,
                     dtype=np.dtype(dtype), **CF_RUNS[which])


def cf_errors(which, seeds=CF_SEEDS):
    """(errors [seeds, data], final ESS [seeds, data], mean acceptance) of the fp32 restatement."""
    exact = S.cf_exact()
    runs = [cf_run(seed, which) for seed in seeds]
    acc = np.mean([r[2].mean() / CF_RUNS[which]["steps_per_stage"] for r in runs])
    return np.stack([A.log_p(r[1]) - exact for r in runs]), np.stack([A.ess(r[1]) for r in runs]), float(acc)


def _main(what):
    if what == "tolerances":
        for name in sorted(A.ESTIMATOR_CASES):
            l32, _, a32, m32 = estimator_reference(name, "float32")
            l64, _, a64, m64 = estimator_reference(name, "float64")
            flipped = (a32 != a64).any(0)
            print(name, "accepted %.1f %%" % (100.0 * a32.mean() / ESTIMATOR_RUN["steps_per_stage"]), " chains that decide differently:",
                  int(flipped.sum()), " max |logw32 - logw64| = %.6g" % np.abs(l32 - l64)[~flipped].max(), " min margin %.2g / %.2g" % (m32, m64))
    elif what == "kat":
        e, s, a = kat_errors()
        print("KAT_ERRORS = (" + ", ".join("%.6f" % v for v in e) + ")", "  mean signed %.3f  acceptance %.3f" % (s, a))
    elif what == "kernels":
        for name in KERNEL_CASES:
            la, Mr, u, acc = kernel_reference(name)
            print(name, "accepted %d of %d" % (acc.sum(), acc.size), " min margin %.3g  needed at most %.3g" % (
                np.abs(np.log(u) - la).min(), margin_needed(Mr, u).max()))
    elif what == "cf":
        for which in ("mala", "hmc"):
            e, s, a = cf_errors(which)
            print("%-5s rms %.6f  max %.4f  mean %.4f  final ESS %.1f .. %.1f  acceptance %.3f" % (
                which, np.sqrt((e ** 2).mean()), np.abs(e).max(), e.mean(), s.min(), s.max(), a))
            if which == "hmc":
                print("CF_ERRORS = (" + ", ".join("%.6f" % v for v in np.abs(e).max(1)) + ")")


if __name__ == "__main__":
    _main(sys.argv[1] if len(sys.argv) > 1 else "kat")

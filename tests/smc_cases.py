"""The yardsticks of resampling in annealed importance sampling (include/mcpc.h: mcpc_smc_ancestors, mcpc_smc_gather;
csrc/mcpc_smc.h; montecarlopredictivecoding_amd/ais.py, resample="systematic"): the NumPy restatement of the arithmetic, the estimator
with resampling in fp32 and fp64 built on tests/ais_cases.py and tests/mala_cases.py, the closed-form linear-Gaussian case with its
exact value, and every figure measured on the CPU.  Shared by tests/test_smc_host.py, tests/test_gpu_smc_kernels.py and
tests/test_gpu_smc_ais.py; no device, no torch.

1. THE ARITHMETIC (`resample`).  Datum i owns rows i R .. i R + R - 1, fp64 throughout, NumPy has no fma:
     ok_j = isfinite(logw_j), cnt = #ok (cnt = 0: untouched, ess = NaN), m = max_ok logw_j, e_j = ok_j ? exp(logw_j - m) : 0
     c = np.cumsum(e), q = np.cumsum(e * e) (sequential, in replica order), S = c[-1], ess = (S * S) / q[-1]
     resample iff ess < threshold * float(R)
     u = (w >> 8) * 2^-24 + 2^-25, w = word 0 of the Philox block of (chain_base + i R, layer 0xFE, group 0, step; seed)
     p_s = ((float(s) + u) / float(R)) * S, a_s = np.searchsorted(c, p_s, "right") clamped to the last j with e_j > 0
     ancestors[i R + s] = i R + a_s and all R log-weights become m + log(S / cnt); otherwise identity ancestors, logw untouched.
   The device's exp may differ from NumPy's by ulps, so a device result is compared where the restatement is far from a tie:
   a SLOT where min_j |c_j - p_s| / S > 2^-40, a DECISION where |ess - threshold R| / R > 2^-40 (`SLOT_MARGIN`, `ESS_MARGIN`).
   The new log-weight is held to 2^-53 (R + 16) (1 + |want|): m is exact, S is R terms of a few ulp each, then one log.

2. THE KERNEL CASES (`KERNEL_CASES`, `kernel_logw`): seeded log-weights 3 N(0, 1) for R in {1, 3, 16, 65, 256} and n_data in
   {1, 5}, for which the restatement leaves no slot and no decision out at thresholds 0.5 and 1.0
   (python -m tests.smc_cases kernels prints the margins; tests/test_smc_host.py asserts them).

3. THE ESTIMATOR (`estimator`): ais_cases.estimator (adjust=None) or mala_cases.estimator (adjust="mala") with `resample` between
   the increment of rung k < K and its transitions, the uniform of Philox step step_base + 1 + (k - 1) steps_per_stage.  Returns
   (logw, state, trace) with trace.ess / .resampled [K - 1, N], .ancestors [K - 1, B], .accepted ([K - 1, B] or None) and the
   smallest margins met (.ess_margin in units of R, .slot_margin in units of S).
   ais_cases' two nets at ais_cases.ESTIMATOR_RUN (lr 0.03), python -m tests.smc_cases tolerances -- `ESTIMATOR_FIGURES` holds, per
   (net, threshold, adjust): the resampled (rung, datum) pairs of 35, max |logw32 - logw64| over the data on which fp32 and fp64
   take the same decisions, the number of data on which they do not, and the two margins of the fp32 restatement.
   The device is held to 10 x that maximum (ais_cases' convention) on the data whose decisions, ancestors and (adjusted) accepted
   counts all equal the fp32 restatement's; at most 1 of the 5 data may be left out.

4. THE CLOSED-FORM CASE (`CF`).  Identity net, 16 latent units, 24 Gaussian outputs, var 0.5, read-out 1.5 randn / sqrt(16), no
   bias, 4 data drawn from the model; 64 replicas, 16 rungs (power 2) x 5 unadjusted steps, lr 0.02.  log p(y) = log N(y; 0, W W^T +
   var I) exactly (`cf_exact`, fp64 Cholesky).  Over seeds 0..7 x 4 data, fp32 restatement (python -m tests.smc_cases cf):
   `CF_ERRORS` per-seed max |error| with resampling at ess_threshold 0.5, `CF_RMS` the pooled rms error plain and resampled.
   The device must stay within CF_TOL = 2 x max(CF_ERRORS) per datum and its pooled rms below the geometric mean of the two rms
   values (`CF_RMS_BOUND`), which the plain estimator misses: without resampling the test cannot pass.
"""
import functools
import math
import sys
from types import SimpleNamespace

import numpy as np

from oracle import mcpc_oracle as mo
from oracle import philox
from tests import ais_cases as A
from tests import mala_cases as M

UNIFORM_LAYER = 0xFE
MAX_REPLICAS = 4096
SLOT_MARGIN = 2.0 ** -40
ESS_MARGIN = 2.0 ** -40


# ---- 1. the arithmetic ----------------------------------------------------------------------------------------------------------------
def uniform(seed, step, chain):
    """The resampling uniform of the datum whose first chain has the global id ``chain``: exact in fp64, inside (0, 1)."""
    w = philox.layer_u32(seed, step, UNIFORM_LAYER, chain, 1, 1)[0, 0]
    return float(int(w) >> 8) * 2.0 ** -24 + 2.0 ** -25


def resample(logw, replicas, threshold, seed, step, chain_base=0):
    """What mcpc_smc_ancestors leaves: SimpleNamespace(ancestors int64 [n R] (rows of the call), logw fp64 [n R], diag fp64 [n, 4] =
    (ess, resampled, u, m + log(S / cnt)), ess_margin [n] = |ess - threshold R| / R (inf for cnt = 0), slot_margin [n, R] =
    min_j |c_j - p_s| / S (inf for a datum that does not resample), e [n, R] and S [n])."""
    R = int(replicas)
    old = np.asarray(logw, dtype=np.float64).reshape(-1, R)
    n = old.shape[0]
    new = old.copy()
    anc = np.arange(n * R, dtype=np.int64).reshape(n, R)
    diag = np.full((n, 4), np.nan)
    ess_margin = np.full(n, np.inf)
    slot_margin = np.full((n, R), np.inf)
    es = np.zeros((n, R))
    Ss = np.zeros(n)
    for i in range(n):
        u = uniform(seed, step, chain_base + i * R)
        ok = np.isfinite(old[i])
        cnt = int(ok.sum())
        diag[i] = (np.nan, 0.0, u, np.nan)
        if cnt == 0:
            continue
        m = old[i][ok].max()
        with np.errstate(all="ignore"):
            e = np.where(ok, np.exp(np.where(ok, old[i], m) - m), 0.0)
        c = np.cumsum(e)
        q = np.cumsum(e * e)
        S = c[-1]
        ess = (S * S) / q[-1]
        bar = threshold * float(R)
        neww = m + np.log(S / float(cnt))
        take = bool(ess < bar)
        diag[i] = (ess, 1.0 if take else 0.0, u, neww)
        ess_margin[i] = abs(ess - bar) / R
        es[i], Ss[i] = e, S
        if take:
            p = ((np.arange(R, dtype=np.float64) + u) / float(R)) * S
            a = np.searchsorted(c, p, "right")
            a = np.minimum(a, np.nonzero(e > 0.0)[0][-1])
            anc[i] = i * R + a
            new[i] = neww
            slot_margin[i] = np.abs(c[None, :] - p[:, None]).min(1) / S
    return SimpleNamespace(ancestors=anc.reshape(-1), logw=new.reshape(-1), diag=diag, ess_margin=ess_margin, slot_margin=slot_margin,
                           e=es, S=Ss)


def offspring_bounds(e, S, ancestors_of_datum):
    """(counts, low, high): the offspring of every replica of ONE datum and floor / ceil of R e_j / S, widened by one where R e_j / S
    is within 1e-9 of an integer (the quotient is rounded)."""
    R = e.shape[0]
    counts = np.bincount(np.asarray(ancestors_of_datum, dtype=np.int64), minlength=R)
    t = R * e / S
    return counts, np.floor(t - 1e-9), np.ceil(t + 1e-9)


def logw_tolerance(want, replicas):
    return 2.0 ** -53 * (replicas + 16) * (1.0 + np.abs(want))


# ---- 2. the kernel cases ----------------------------------------------------------------------------------------------------------------
KERNEL_RUN = dict(seed=0x5EED5EED123, step=(1 << 32) + 11, chain_base=3000)
KERNEL_REPLICAS = (1, 3, 16, 65, 256)
KERNEL_DATA = (1, 5)
KERNEL_THRESHOLDS = (0.5, 1.0)
GATHER_WIDTHS = (1, 2, 17, 33, 257)
KERNEL_SPREADS = (3.0, 0.2, 1.0, 0.05, 2.0)


@functools.lru_cache(maxsize=None)
def kernel_logw(replicas, n_data):
    """Seeded fp64 log-weights ``[n_data * replicas]``: -40 + s_i N(0, 1) with the spread s_i of datum i from `KERNEL_SPREADS`, so that
    at threshold 0.5 some data resample (s = 3, 1, 2) and others do not (s = 0.2, 0.05)."""
    rng = np.random.default_rng([31, replicas, n_data])
    s = np.repeat(np.asarray(KERNEL_SPREADS[:n_data]), replicas)
    w = -40.0 + s * rng.standard_normal(n_data * replicas)
    w.setflags(write=False)
    return w


def kernel_reference(replicas, n_data, threshold):
    return resample(kernel_logw(replicas, n_data), replicas, threshold, **KERNEL_RUN)


# ---- 3. the estimator -------------------------------------------------------------------------------------------------------------------
def estimator(W, b, sizes, acts, n_in, data, loss, var, mask_start, *, replicas, betas, steps_per_stage, lr, noise_var=2.0, seed=0,
              step_base=0, chain_base=0, dtype=np.float32, adjust=None, threshold=None):
    """ais_cases.estimator / mala_cases.estimator with resampling at ``threshold`` (None: none, and the trace is empty)."""
    dt = np.dtype(dtype)
    L = len(sizes)
    data = np.asarray(data, dtype=np.float32)
    N = data.shape[0]
    B = N * replicas
    y = np.repeat(data, replicas, axis=0)
    a_prev = np.zeros((B, n_in), dtype=dt)
    xs = []
    for j in range(L):                                                      # the ancestral draw, as ais_cases.estimator makes it
        mu = mo._linear(a_prev, W[j].astype(dt), None if b[j] is None else b[j].astype(dt))
        z = philox.layer_normals(seed, step_base, j, chain_base, B, sizes[j]).astype(dt)
        xs.append((mu + z).astype(dt))
        a_prev = mo._act(A.ACT[acts[j]], xs[j])
    inputs = np.zeros((B, n_in), dtype=np.float32 if adjust is None else dt)
    logw = np.zeros(B)
    K = len(betas) - 1
    tr = SimpleNamespace(ess=np.full((K - 1, N), np.nan), resampled=np.zeros((K - 1, N), dtype=bool),
                         ancestors=np.tile(np.arange(B, dtype=np.int64), (K - 1, 1)), ess_margin=np.inf, slot_margin=np.inf,
                         accepted=None if adjust is None else np.zeros((K - 1, B), dtype=np.int64))
    for k in range(1, K + 1):
        sc = (betas[k - 1], 1.0, betas[k], 1.0) if loss == "bernoulli" else (1.0, betas[k - 1], 1.0, betas[k])
        logw, _ = A.increment(xs[-1], W[L], b[L], y, acts[-1], loss, var, mask_start, *sc, logw=logw)
        if k == K:
            break
        first = step_base + 1 + (k - 1) * steps_per_stage
        if threshold is not None:
            r = resample(logw, replicas, threshold, seed, first, chain_base)
            tr.ess[k - 1], tr.resampled[k - 1], tr.ancestors[k - 1] = r.diag[:, 0], r.diag[:, 1] != 0.0, r.ancestors
            tr.ess_margin = min(tr.ess_margin, float(r.ess_margin.min()))
            tr.slot_margin = min(tr.slot_margin, float(r.slot_margin.min()))
            logw = r.logw
            xs = [np.ascontiguousarray(x[r.ancestors]) for x in xs]
        if loss == "bernoulli":                                             # the scaled read-out: an fp32 scratch copy, as the device's
            Wk = list(W[:L]) + [(W[L] * np.float32(betas[k])).astype(np.float32)]
            bk = list(b[:L]) + [None if b[L] is None else (b[L] * np.float32(betas[k])).astype(np.float32)]
            run_var = 1.0
        else:
            Wk, bk, run_var = W, b, var / betas[k]
        net = mo.NetSpec(sizes=list(sizes), acts=[A.ACT[a] for a in acts], W=list(Wk), b=list(bk))
        spec = mo.LossSpec(A.LOSS[loss], y, run_var, mask_start)
        if adjust is None:
            res = mo.run(net, inputs, xs, spec, mo.XOpt(mo.OPT_SGD, lr), steps_per_stage,
                         noise=lambda t, l, sb=first: philox.layer_normals(seed, sb + t, l, chain_base, B, sizes[l]), noise_var=noise_var,
                         dtype=dt)
            xs = res.xs
            continue
        E, fw = M.chain_energy(net, inputs, xs, spec)
        g = mo.x_grads(net, xs, fw)
        for t in range(steps_per_stage):
            step = first + t
            xp = [M.propose(xs[l], g[l], philox.layer_normals(seed, step, l, chain_base, B, sizes[l]), lr, noise_var, dt) for l in range(L)]
            Ep, fwp = M.chain_energy(net, inputs, xp, spec)
            gp = mo.x_grads(net, xp, fwp)
            la, _ = M.log_alpha(xs, g, E, xp, gp, Ep, lr, noise_var)
            acc = M.decide(la, M.uniform(seed, step, chain_base, B))
            xs = [np.where(acc[:, None], p, x) for p, x in zip(xp, xs)]
            g = [np.where(acc[:, None], p, x) for p, x in zip(gp, g)]
            E = np.where(acc, Ep, E)
            tr.accepted[k - 1] += acc
    n_active = data.shape[1] - mask_start
    return logw, A.state_from_logw(logw, replicas, A.log_norm(loss, n_active, var)), tr


ESTIMATOR_RUN = dict(A.ESTIMATOR_RUN)
THRESHOLDS = (0.5, 1.0)
ADJUSTS = (None, "mala")
MAX_DATA_LEFT_OUT = 1
# (net, threshold, adjust): (resampled pairs of 35, max |logw32 - logw64| over the data that decide alike, data that do not,
#                            ess margin / R, slot margin / S)            python -m tests.smc_cases tolerances
ESTIMATOR_FIGURES = {
    ("bern_relu", 0.5, None): (1, 1.09294e-06, 0, 0.0384, 0.00104),        # final ESS 9.0 5.4 8.6 14.8 8.3
    ("bern_relu", 0.5, "mala"): (1, 1.10385e-06, 0, 0.0372, 0.000736),     # final ESS 8.4 5.3 8.9 14.8 8.4
    ("bern_relu", 1.0, None): (35, 2.81626e-07, 0, 0.000328, 0.000143),    # final ESS 15.1 13.3 15.1 14.7 14.6
    ("bern_relu", 1.0, "mala"): (35, 2.38424e-07, 0, 0.000328, 4.66e-05),  # final ESS 15.4 14.0 14.8 14.5 14.3
    ("gauss_tanh", 0.5, None): (9, 7.73077e-07, 0, 0.022, 2.63e-05),       # final ESS 12.1 13.1 7.5 6.5 9.6 (plain: 1.9 .. 3.3)
    ("gauss_tanh", 0.5, "mala"): (9, 6.01511e-07, 0, 0.0131, 1.69e-05),    # final ESS 13.0 13.2 11.9 7.4 9.7
    ("gauss_tanh", 1.0, None): (35, 3.94982e-07, 0, 0.0032, 3.15e-05),     # final ESS 10.5 14.0 11.8 13.5 13.5
    ("gauss_tanh", 1.0, "mala"): (35, 5.95297e-07, 0, 0.0032, 7.19e-07),   # final ESS 11.5 13.7 10.2 13.4 14.0
}


@functools.lru_cache(maxsize=None)
def estimator_reference(name, threshold, adjust=None, dtype="float32"):
    c = A.ESTIMATOR_CASES[name]
    W, b, data = A.estimator_params(name)
    r = dict(ESTIMATOR_RUN)
    stages = r.pop("stages")
    return estimator(W, b, c["sizes"], [c["act"]] * len(c["sizes"]), c["n_in"], data, c["loss"], c["var"], c["mask_start"],
                     betas=A.schedule(stages), dtype=np.dtype(dtype), adjust=adjust, threshold=threshold, **r)


def data_that_agree(tr_a, tr_b, replicas):
    """bool [N]: the data on which two traces take the same decisions, ancestors and (adjusted) accepted counts."""
    N = tr_a.resampled.shape[1]
    same = (tr_a.resampled == tr_b.resampled).all(0)
    same &= (tr_a.ancestors == tr_b.ancestors).reshape(-1, N, replicas).all((0, 2))
    if tr_a.accepted is not None:
        same &= (tr_a.accepted == tr_b.accepted).reshape(-1, N, replicas).all((0, 2))
    return same


def estimator_figures(name, threshold, adjust):
    l32, _, t32 = estimator_reference(name, threshold, adjust, "float32")
    l64, _, t64 = estimator_reference(name, threshold, adjust, "float64")
    R = ESTIMATOR_RUN["replicas"]
    same = data_that_agree(t32, t64, R)
    d = np.abs(l32 - l64).reshape(-1, R)[same]
    return int(t32.resampled.sum()), float(d.max()) if d.size else float("nan"), int((~same).sum()), t32.ess_margin, t32.slot_margin


def estimator_tolerance(name, threshold, adjust):
    return 10.0 * ESTIMATOR_FIGURES[(name, threshold, adjust)][1]


# ---- 4. the closed-form case ------------------------------------------------------------------------------------------------------------
CF = dict(n_latent=16, n_out=24, var=0.5, n_data=4, replicas=64, stages=16, power=2.0, steps_per_stage=5, lr=0.02, noise_var=2.0,
          threshold=0.5)
CF_SEEDS = tuple(range(8))
# per-seed max_i |log p_hat_i - exact_i| of the fp32 restatement WITH resampling, and the rms error pooled over seeds x data of the
# restatement without and with it (python -m tests.smc_cases cf)
CF_ERRORS = (1.442541, 1.960544, 1.924692, 1.599439, 0.928797, 2.377614, 1.813725, 1.448438)
CF_RMS = {"plain": 2.911399, "resampled": 1.083925}          # (resampling at every rung: 1.104409)
# final ESS of 64: 1.0 .. 6.9 plain, 23.3 .. 58.8 resampled; mean error -2.24 and -0.79 (the step-size bias of unadjusted Langevin)


def cf_tol():
    return 2.0 * max(CF_ERRORS)


def cf_rms_bound():
    return math.sqrt(CF_RMS["plain"] * CF_RMS["resampled"])


@functools.lru_cache(maxsize=None)
def cf_params():
    """(W [Linear 0: zeros, read-out], b [zeros, None], data [4, 24]): x ~ N(0, I_16), y ~ N(W x, var I); never modified."""
    rng = np.random.default_rng(2006)
    n, n_out = CF["n_latent"], CF["n_out"]
    W_L = (1.5 * rng.standard_normal((n_out, n)) / np.sqrt(n)).astype(np.float32)
    x_true = rng.standard_normal((CF["n_data"], n))
    data = (x_true @ W_L.astype(np.float64).T + math.sqrt(CF["var"]) * rng.standard_normal((CF["n_data"], n_out))).astype(np.float32)
    W = [np.zeros((n, 1), dtype=np.float32), W_L]
    b = [np.zeros(n, dtype=np.float32), None]
    for a in (*W, b[0], data):
        a.setflags(write=False)
    return W, b, data


@functools.lru_cache(maxsize=None)
def cf_exact():
    """fp64 [4]: log N(y_i; 0, W W^T + var I) by a Cholesky factor."""
    W, _, data = cf_params()
    Wd, yd = W[1].astype(np.float64), data.astype(np.float64)
    C = Wd @ Wd.T + CF["var"] * np.eye(CF["n_out"])
    Lc = np.linalg.cholesky(C)
    z = np.linalg.solve(Lc, yd.T)
    return -0.5 * (z * z).sum(0) - np.log(np.diag(Lc)).sum() - 0.5 * CF["n_out"] * math.log(2.0 * math.pi)


@functools.lru_cache(maxsize=None)
def cf_run(seed=0, threshold=CF["threshold"], adjust=None, dtype="float32"):
    """(logw, state, trace) of the restatement on the closed-form case; ``threshold=None``: plain AIS."""
    W, b, data = cf_params()
    return estimator(W, b, (CF["n_latent"],), ["identity"], 1, data, "gaussian", CF["var"], 0, replicas=CF["replicas"],
                     betas=A.schedule(CF["stages"], CF["power"]), steps_per_stage=CF["steps_per_stage"], lr=CF["lr"],
                     noise_var=CF["noise_var"], seed=seed, dtype=np.dtype(dtype), adjust=adjust, threshold=threshold)


def cf_errors(threshold, seeds=CF_SEEDS):
    """(errors [seeds, data], final ESS [seeds, data]) of the fp32 restatement."""
    exact = cf_exact()
    runs = [cf_run(seed, threshold) for seed in seeds]
    return np.stack([A.log_p(st) - exact for _, st, _ in runs]), np.stack([A.ess(st) for _, st, _ in runs])


def _main(what):
    if what == "kernels":
        for R in KERNEL_REPLICAS:
            for n in KERNEL_DATA:
                for thr in KERNEL_THRESHOLDS:
                    r = kernel_reference(R, n, thr)
                    print("R %3d  n %d  threshold %.1f  resampled %d of %d  ess margin %.3g  slot margin %.3g" % (
                        R, n, thr, int(r.diag[:, 1].sum()), n, r.ess_margin.min(), r.slot_margin.min()))
    elif what == "tolerances":
        for name in sorted(A.ESTIMATOR_CASES):
            for thr in THRESHOLDS:
                for adjust in ADJUSTS:
                    f = estimator_figures(name, thr, adjust)
                    _, st, tr = estimator_reference(name, thr, adjust)
                    print('    ("%s", %.1f, %r): (%d, %.6g, %d, %.3g, %.3g),' % (name, thr, adjust, *f), "  # final ESS",
                          np.round(A.ess(st), 1))
    elif what == "cf":
        print("exact", cf_exact())
        e0, s0 = cf_errors(None)
        e1, s1 = cf_errors(CF["threshold"])
        e2, _ = cf_errors(1.0)
        print("plain      rms %.6f  max %.4f  mean %.4f  final ESS %.1f .. %.1f" % (np.sqrt((e0 ** 2).mean()), np.abs(e0).max(), e0.mean(),
                                                                                 s0.min(), s0.max()))
        print("resampled  rms %.6f  max %.4f  mean %.4f  final ESS %.1f .. %.1f" % (np.sqrt((e1 ** 2).mean()), np.abs(e1).max(), e1.mean(),
                                                                                 s1.min(), s1.max()))
        print("every rung rms %.6f" % np.sqrt((e2 ** 2).mean()))
        print("CF_ERRORS = (" + ", ".join("%.6f" % v for v in np.abs(e1).max(1)) + ")")


if __name__ == "__main__":
    _main(sys.argv[1] if len(sys.argv) > 1 else "cf")

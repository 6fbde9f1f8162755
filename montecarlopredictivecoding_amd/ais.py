"""Annealed importance sampling (Neal 2001) of the log marginal likelihood PER DATUM: the estimator behind ``PCTrainer.mcpc_ais``.

Importance sampling from the prior (``likelihood.log_likelihood``) is degenerate: its effective sample size is about 1 on a 784-pixel
read-out.  AIS walks every chain from an exact prior sample to the posterior over a ladder of distributions ``f_0 .. f_K`` with a few
Langevin steps per rung, and the product of the ratios ``f_k(x_{k-1}) / f_{k-1}(x_{k-1})`` met on the way is an importance weight whose
mean estimates ``Z_K / Z_0``.  Everything it needs is what the engine is fast at: ``Engine.sample_prior`` draws the start,
``Engine.run`` makes the transitions, ``engine.ais_increment`` (csrc/mcpc_ais.h) adds the log-ratio per chain in fp64.

The transitions are unadjusted Langevin steps (``adjust=None``: unbiased only as ``lr -> 0``) or Metropolis-adjusted ones
(``adjust="mala"``): a proposal ``engine.mala_propose``, the engine's gradient (``Engine.run(1, update_x=False)``) and energy
(``Engine.chain_energies``) at it, and the accept / reject decision ``engine.mala_accept`` (csrc/mcpc_mala.h).  Each adjusted
transition leaves its rung's distribution exactly invariant, so ``exp(log p_hat)`` is unbiased at any step size.  With ``leapfrog=L >=
2`` an adjusted transition is a Hamiltonian trajectory of L leapfrog steps of size ``sqrt(2 lr)`` with one decision at its end
(``engine.hmc_begin``, ``engine.hmc_leap``, ``engine.hmc_accept``, csrc/mcpc_hmc.h): the same L gradient evaluations spent on one
directed move instead of L random-walk steps, and ONE energy evaluation instead of L.  ``leapfrog=1`` is the MALA step itself.
``gradients="evaluator"`` evaluates a proposal with ONE ``Engine.state_gradients`` call on the proposal's own tensors
(csrc/mcpc_state_grad.h: gradient and, where the decision needs it, energy) instead of passing it through the engine's state.

The replicas of a datum may be RESAMPLED between rungs (``resample="systematic"``): when the effective sample size of a datum's
weights falls below ``ess_threshold * replicas``, ``engine.smc_ancestors`` draws the ancestors and resets the log-weights to the log
of their mean, and ``engine.smc_gather`` moves the state (csrc/mcpc_smc.h).  That is the sequential Monte Carlo sampler of Del
Moral, Doucet & Jasra (2006) on the same ladder, with either kind of transition.

The two ladders, both walked with what ``mcpc_run`` already takes:
  Bernoulli  ``f_k(x) = p(x) exp(-BCE(beta_k o(x), y))``: rung k runs the ordinary Bernoulli loss on a read-out scaled by ``beta_k``
             (a scratch copy, re-bound per rung).  At ``beta = 0`` the likelihood factor is the constant ``2^-n_active``.
  Gaussian   ``f_k(x) = p(x) exp(-beta_k (0.5 / var) |o(x) - y|^2)``: the geometric ladder, rung k runs ``loss_var = var / beta_k``.
             ``f_0`` is the prior; the likelihood's normaliser ``(2 pi var)^(-n_active / 2)`` is added at the end.

This module holds the host logic (schedule, scalars per rung, chunking, the fold of log-weights into a ``LogLikelihood`` state) as
functions that need no device, ``run``, the call, and ``_ladder``, the one loop over the rungs of a chunk that both kinds of
transition share.  No device code.
"""
import math
from types import SimpleNamespace
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib as L
from . import engine as E
from .likelihood import LogLikelihood, empty_state


def schedule(stages: int = 64, power: float = 2.0, betas: Optional[Sequence[float]] = None) -> List[float]:
    """The ladder ``beta_0 = 0 < beta_1 < ... < beta_K = 1``: ``(k / stages)^power`` for k = 0..stages, or ``betas`` as given, which
    must be strictly increasing from exactly 0 to exactly 1.  Anything else is a ValueError."""
    if betas is None:
        if isinstance(stages, bool) or not isinstance(stages, int) or stages < 1:
            raise ValueError(f"stages={stages!r}, must be an int of at least 1")
        power = float(power)
        if not (power > 0.0 and math.isfinite(power)):
            raise ValueError(f"power={power!r}, must be positive and finite")
        out = [(k / stages) ** power for k in range(stages + 1)]
        out[0], out[-1] = 0.0, 1.0
    else:
        try:
            out = [float(b) for b in betas]
        except (TypeError, ValueError):
            raise ValueError(f"betas must be a sequence of numbers, got {betas!r}") from None
        if len(out) < 2:
            raise ValueError(f"betas holds {len(out)} values, at least two (0 and 1) are needed")
        if out[0] != 0.0 or out[-1] != 1.0:
            raise ValueError(f"betas must start at 0 and end at 1, got {out[0]!r} .. {out[-1]!r}")
    if any(not math.isfinite(b) for b in out) or any(not a < b for a, b in zip(out, out[1:])):
        raise ValueError("betas must be finite and strictly increasing" + ("" if betas is not None else
                                                                          f" (stages={stages}, power={power}: two rungs coincide)"))
    return out


def rung_scalars(loss_kind: int, beta_prev: float, beta_k: float) -> Tuple[float, float, float, float]:
    """``(a0, c0, a1, c1)`` of ``ais_increment`` for the step from rung k-1 to rung k: ``c0 l(a0) - c1 l(a1) = log f_k - log f_{k-1}``."""
    if loss_kind == L.LOSS_BERNOULLI:
        return (float(beta_prev), 1.0, float(beta_k), 1.0)
    if loss_kind == L.LOSS_GAUSSIAN:
        return (1.0, float(beta_prev), 1.0, float(beta_k))
    raise ValueError(f"loss_kind={loss_kind}: the ladder is defined for the Bernoulli and the Gaussian read-out")


def rung_run(loss_kind: int, var: float, beta_k: float) -> Tuple[float, float]:
    """``(read-out scale, loss_var)`` of the Langevin steps that target ``f_k``."""
    if loss_kind == L.LOSS_BERNOULLI:
        return float(beta_k), 1.0
    return 1.0, float(var) / float(beta_k)


def log_norm(loss_kind: int, n_active: int, var: float = 1.0) -> float:
    """What is subtracted from a chain's log-weight: ``-log`` of the constant the ladder leaves out.  Bernoulli: ``f_0`` carries
    ``exp(-BCE(0, y)) = 2^-n_active``, so ``Z_0 = 2^-n_active`` and ``log p = log mean w + log Z_0``; Gaussian: the density's
    normaliser ``(2 pi var)^(-n_active / 2)``."""
    if loss_kind == L.LOSS_BERNOULLI:
        return n_active * math.log(2.0)
    return 0.5 * n_active * math.log(2.0 * math.pi * float(var))


def chunks(n_data: int, replicas: int, max_chains: int, chain_base: int = 0) -> List[Tuple[int, int, int]]:
    """``[(first datum, data, global id of the first chain)]``: the call as chunks of at most ``max_chains // replicas`` data.  Chain
    ``c`` of a chunk serves datum ``first + c // replicas``; its global id counts the chains of the whole call from ``chain_base``."""
    for name, v in (("replicas", replicas), ("max_chains", max_chains)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"{name}={v!r}, must be an int of at least 1")
    if isinstance(chain_base, bool) or not isinstance(chain_base, int) or chain_base < 0:
        raise ValueError(f"chain_base={chain_base!r}, must be a non-negative int")
    per = max_chains // replicas
    if per < 1:
        raise ValueError(f"max_chains={max_chains} holds not one datum's {replicas} replicas")
    if chain_base + n_data * replicas > 1 << 32:
        raise ValueError(f"chain_base={chain_base} with {n_data * replicas} chains: chain ids are 32 bits")
    return [(d0, min(per, n_data - d0), chain_base + d0 * replicas) for d0 in range(0, n_data, per)]


def engine_calls(n_data, replicas, max_chains, n_rungs, steps_per_stage, step_base=0, chain_base=0):
    """Every engine call of ``run`` that consumes normals, in order: ``(what, sample_base or chain_base, step_base, chains)`` with
    ``what`` "prior" (``Engine.sample_prior``) or "run" (``Engine.run`` of ``steps_per_stage`` steps).  The prior uses step
    ``step_base``; the transitions after increment k use steps ``step_base + 1 + (k - 1) * steps_per_stage`` onwards: no normal twice.
    It accounts for Philox steps, not launches: a transition takes ONE step whatever ``leapfrog`` is (its normals are the trajectory's
    momentum), so ``leapfrog`` does not enter."""
    out = []
    for _, n, g0 in chunks(n_data, replicas, max_chains, chain_base):
        out.append(("prior", g0, step_base, n * replicas))
        for k in range(1, n_rungs):
            out.append(("run", g0, step_base + 1 + (k - 1) * steps_per_stage, n * replicas))
    return out


def fold(logw: torch.Tensor, replicas: int, const: float) -> torch.Tensor:
    """``[n, 4]`` fp64 ``LogLikelihood`` states of n data from the log-weights ``logw`` ``[n * replicas]`` of their chains (datum i:
    chains ``i * replicas ..``): ``nll_r = -(logw_r - const)``, then ``m = min nll``, ``s1 = sum e^-(nll - m)``, ``s2 = sum e^-2(nll -
    m)``, ``cnt``, over the finite ones -- a replica whose log-weight is not finite is neither taken nor counted.  On the device of
    ``logw``.  Element-wise operations and a halving tree of additions only: a datum's state does not depend on the other data."""
    nll = -(logw.to(torch.float64).reshape(-1, int(replicas)) - float(const))
    ok = torch.isfinite(nll)
    n = nll.shape[0]
    m = torch.where(ok, nll, torch.full_like(nll, math.inf)).min(dim=1).values if nll.shape[1] else torch.full((n,), math.inf)
    live = m < math.inf
    base = torch.where(live, m, torch.zeros_like(m)).unsqueeze(1)
    e = torch.where(ok, torch.exp(-(torch.where(ok, nll, base) - base)), torch.zeros_like(nll))
    width = 1
    while width < nll.shape[1]:
        width *= 2
    pad = torch.zeros(n, width - nll.shape[1], dtype=torch.float64, device=nll.device)
    s1, s2, cnt = (torch.cat([t, pad], dim=1) for t in (e, e * e, ok.to(torch.float64)))
    while width > 1:
        width //= 2
        s1, s2, cnt = (t[:, :width] + t[:, width:2 * width] for t in (s1, s2, cnt))
    st = torch.stack([m, s1[:, 0], s2[:, 0], cnt[:, 0]], dim=1)
    return torch.where(live.unsqueeze(1), st, empty_state(n, nll.device))


def check_adjust(adjust):
    """``adjust`` as ``run`` takes it: None (unadjusted Langevin transitions) or "mala"; anything else is a ValueError."""
    if adjust is not None and not (isinstance(adjust, str) and adjust == "mala"):
        raise ValueError(f"adjust={adjust!r}, expected None or 'mala'")
    return adjust


def check_gradients(gradients, adjust=None):
    """``gradients`` as ``run`` takes it: "run" (a proposal passes through the engine's state: ``load_state``, ``Engine.run(1,
    update_x=False)``, ``Engine.chain_energies``) or "evaluator" (one ``Engine.state_gradients`` call on the proposal itself, which
    only an adjusted call makes: ``adjust="mala"``); anything else is a ValueError."""
    if not (isinstance(gradients, str) and gradients in ("run", "evaluator")):
        raise ValueError(f"gradients={gradients!r}, expected 'run' or 'evaluator'")
    if gradients == "evaluator" and adjust is None:
        raise ValueError("gradients='evaluator' with adjust=None: unadjusted transitions evaluate nothing, pass adjust='mala'")
    return gradients


def check_leapfrog(leapfrog, adjust=None, noise_var=2.0):
    """``leapfrog`` as ``run`` takes it: an int of at least 1.  More than one leapfrog step needs the decision at the trajectory's end
    (``adjust="mala"``) and ``noise_var == 2.0`` (a unit-mass Hamiltonian has no other noise scale: its one-step trajectory is the
    Langevin proposal at ``noise_var = 2``); anything else is a ValueError."""
    if isinstance(leapfrog, bool) or not isinstance(leapfrog, int) or leapfrog < 1:
        raise ValueError(f"leapfrog={leapfrog!r}, must be an int of at least 1")
    if leapfrog > 1 and adjust is None:
        raise ValueError(f"leapfrog={leapfrog} with adjust=None: a trajectory is accepted or rejected at its end, pass adjust='mala'")
    if leapfrog > 1 and not (isinstance(noise_var, (int, float)) and not isinstance(noise_var, bool) and float(noise_var) == 2.0):
        raise ValueError(f"leapfrog={leapfrog} with noise_var={noise_var!r}: a unit-mass Hamiltonian has noise_var = 2 alone")
    return leapfrog


def check_resample(resample, ess_threshold, replicas):
    """``(resample, ess_threshold as a float)`` as ``run`` takes them: ``resample`` None or "systematic", ``ess_threshold`` a number
    in [0, 1], and at most ``SMC_MAX_REPLICAS`` replicas when resampling (one workgroup walks a datum's weights); anything else is a
    ValueError."""
    if resample is not None and not (isinstance(resample, str) and resample == "systematic"):
        raise ValueError(f"resample={resample!r}, expected None or 'systematic'")
    if isinstance(ess_threshold, bool) or not isinstance(ess_threshold, (int, float)) or not 0.0 <= float(ess_threshold) <= 1.0:
        raise ValueError(f"ess_threshold={ess_threshold!r}, must be a number in [0, 1]")
    if resample is not None and isinstance(replicas, int) and replicas > L.SMC_MAX_REPLICAS:
        raise ValueError(f"replicas={replicas} with resample={resample!r}: at most {L.SMC_MAX_REPLICAS} replicas of a datum are resampled")
    return resample, float(ess_threshold)


def check_counts(replicas, steps_per_stage, noise_var, seed, step_base):
    for name, v, low in (("replicas", replicas, 1), ("steps_per_stage", steps_per_stage, 1), ("seed", seed, None), ("step_base", step_base, 0)):
        if isinstance(v, bool) or not isinstance(v, int) or (low is not None and v < low):
            raise ValueError(f"{name}={v!r}, must be an int" + ("" if low is None else f" of at least {low}"))
    if not (float(noise_var) > 0.0 and math.isfinite(float(noise_var))):
        raise ValueError(f"noise_var={noise_var!r}, must be positive and finite")


def resolve_lr(lr, xopt, why=""):
    """The Langevin step size: ``lr``, or the trainer's x optimiser's when that is plain SGD."""
    if lr is None:
        if xopt is None or xopt.kind != L.XOPT_SGD:
            raise ValueError("lr: the trainer's x optimiser is not plain SGD ({}); its lr is no Langevin step size -- pass lr=".format(
                why or "Adam"))
        return float(xopt.lr)
    lr = float(lr)
    if not (lr > 0.0 and math.isfinite(lr)):
        raise ValueError(f"lr={lr!r}, must be positive and finite")
    return lr


def _ladder(call, c):
    """Walk one chunk up the ladder: ``c.logw`` receives the log-weights.  ``call`` holds what every chunk of a call shares: ``adjust``,
    ``ladder``, ``steps_per_stage``, ``lr``, ``noise_var``, ``seed``, ``step_base`` as ``run`` takes them, the read-out's activation
    ``act`` and its ``loss``.  ``c`` holds what the chunk owns: its engine ``eng``, the chains' state ``xs`` (the prior draw on entry),
    their targets ``y``, ``logw``, the global id ``g0`` of the first chain, the model's own read-out ``W_L``, ``b_L`` and, on the
    Bernoulli ladder, the scratch read-out ``scaled = (W_s, b_s)`` the engine is bound to (else None).  ``call.leapfrog`` (1 when
    absent) is the number of leapfrog steps of an adjusted transition.

    Rung k adds its increment at the state the transitions of rung k - 1 left, re-packs the scaled read-out, and makes
    ``steps_per_stage`` transitions that target ``f_k``; step t of them takes its normals (and its uniform) from Philox step
    ``step_base + 1 + (k - 1) * steps_per_stage + t``.  Unadjusted, the state lives in the engine, ``c.xs`` is read back before each
    increment, and a rung is one ``Engine.run``.  Adjusted, the state lives in ``c.xs`` with its gradient ``g`` and energy ``En``, the
    engine only evaluates (once per step, at the proposal), and the return value is the number of accepted proposals per rung and
    chain, int32 ``[K - 1, B]`` (None when unadjusted).  With ``leapfrog = L >= 2`` a transition is ``hmc_begin``, L - 1 times a
    gradient at the trajectory's point (no energy there) and ``hmc_leap``, then gradient and energy at its end and ``hmc_accept``: the
    trajectory's position, momentum and initial kinetic energy live in three buffers allocated once per chunk.

    With ``call.resample``, rung k < K resamples between its increment and its transitions: ``engine.smc_ancestors`` decides per datum
    from ``c.logw`` (the uniform is that of the rung's first Philox step, under a layer index of its own) and ``engine.smc_gather``
    moves all latent layers.  Unadjusted, the gathered state is loaded back into the engine; adjusted, ``c.xs`` is replaced -- the
    gradient and the energy are re-evaluated at the start of every rung, so nothing stale survives.  ``c.smc_diag`` fp64
    ``[K - 1, n, 4]`` and ``c.ancestors`` int32 ``[K - 1, B]`` (rows of the chunk) receive the trace."""
    eng, xs, loss, K, mala = c.eng, c.xs, call.loss, len(call.ladder) - 1, call.adjust == "mala"
    run_kw = dict(loss_kind=loss.kind, mask_start=loss.mask_start, xopt=L.XOPT_SGD, lr=call.lr)
    accepted = None
    resample = getattr(call, "resample", None) is not None
    if resample:
        gathered = [torch.empty_like(x) for x in xs]
    if mala:
        accepted = torch.zeros(K - 1, xs[0].shape[0], dtype=torch.int32, device=xs[0].device)
        spare = [[torch.empty_like(x) for x in xs] for _ in range(2)]     # two proposal buffers: accept reads one and fills the other
    leapfrog = getattr(call, "leapfrog", 1)
    if leapfrog > 1:
        xt, q = spare                                                     # the trajectory's position and half-step momentum
        K0 = torch.empty(xs[0].shape[0], dtype=torch.float64, device=xs[0].device)

    evaluator = getattr(call, "gradients", "run") == "evaluator"
    eval_kw = dict(loss_kind=loss.kind, mask_start=loss.mask_start)

    def gradient(state, run_var):
        """Gradient of ``state`` under the rung's distribution (``update_x=False`` moves nothing; the evaluator reads ``state`` itself)."""
        if evaluator:
            return [g[0] for g in eng.state_gradients(None, state, loss_var=run_var, **eval_kw)[0]]
        eng.load_state(state)
        return eng.run(1, loss_var=run_var, update_x=False, step_base=0, **run_kw).xgrad

    def evaluate(state, run_var):
        """Gradient and energy of ``state`` under the rung's distribution: one launch each, or one evaluator call for both."""
        if evaluator:
            gs, en = eng.state_gradients(None, state, loss_var=run_var, energies=True, **eval_kw)
            return [g[0] for g in gs], en[0, :, -1].contiguous()
        g = gradient(state, run_var)
        en = eng.chain_energies(None, state, loss_var=run_var, **eval_kw)
        return g, en[0, :, -1].contiguous()

    def langevin(k, first, run_var):
        eng.run(call.steps_per_stage, loss_var=run_var, noise_mode=L.NOISE_PHILOX, noise_var=call.noise_var, seed=call.seed,
                step_base=first, chain_base=c.g0, **run_kw)

    def metropolis(k, first, run_var):
        g, En = evaluate(xs, run_var)
        xp = E.mala_propose(xs, g, call.lr, call.noise_var, call.seed, first, c.g0, out=spare[0])
        for t in range(call.steps_per_stage):
            gp, Ep = evaluate(xp, run_var)
            nxt = spare[(t + 1) % 2] if t + 1 < call.steps_per_stage else None
            E.mala_accept(xs, g, En, xp, gp, Ep, call.lr, call.noise_var, call.seed, first + t, c.g0, n_accepted=accepted[k - 1],
                          x_next=nxt)
            xp = nxt

    def hamiltonian(k, first, run_var):
        g, En = evaluate(xs, run_var)
        for t in range(call.steps_per_stage):
            E.hmc_begin(xs, g, call.lr, call.seed, first + t, c.g0, q_out=q, x_out=xt, K0=K0)
            for _ in range(leapfrog - 1):                                  # interior points: the gradient alone
                E.hmc_leap(xt, q, gradient(xt, run_var), call.lr)
            gt, Et = evaluate(xt, run_var)
            E.hmc_accept(xs, g, En, xt, gt, Et, q, K0, call.lr, call.seed, first + t, c.g0, n_accepted=accepted[k - 1])

    transitions = (hamiltonian if leapfrog > 1 else metropolis) if mala else langevin
    for k in range(1, K + 1):
        if not mala:
            eng.store_state(xs)
        a0, c0, a1, c1 = rung_scalars(loss.kind, call.ladder[k - 1], call.ladder[k])
        E.ais_increment(xs[-1], c.W_L, c.b_L, c.y, call.act, loss.kind, loss.var, loss.mask_start, a0, c0, a1, c1, c.logw, accumulate=True)
        if k == K:
            break
        if resample:
            E.smc_ancestors(c.logw, call.replicas, call.ess_threshold, call.seed, call.step_base + 1 + (k - 1) * call.steps_per_stage,
                            c.g0, ancestors=c.ancestors[k - 1], diag=c.smc_diag[k - 1])
            E.smc_gather(xs, c.ancestors[k - 1], out=gathered)
            if mala:
                xs, gathered = gathered, xs                                # (the closures above read this binding)
                c.xs = xs
            else:
                eng.load_state(gathered)
        scale, run_var = rung_run(loss.kind, loss.var, call.ladder[k])
        if c.scaled is not None:
            torch.mul(c.W_L, scale, out=c.scaled[0])
            if c.scaled[1] is not None:
                torch.mul(c.b_L, scale, out=c.scaled[1])
            eng.params_changed()
        transitions(k, call.step_base + 1 + (k - 1) * call.steps_per_stage, run_var)
    return accepted


def run(trainer, data, loss_fn, loss_fn_kwargs=None, *, replicas=64, stages=64, power=2.0, betas=None, steps_per_stage=5, lr=None,
        noise_var=2.0, seed=0, step_base=0, chain_base=0, max_chains=6000, adjust=None, resample=None, ess_threshold=0.5,
        leapfrog=1, gradients="run", return_logw=False, return_accepted=False, return_ancestors=False):
    """``PCTrainer.mcpc_ais`` (its docstring is the contract).  ``return_logw``: also the raw log-weights, fp64 ``[N * replicas]``.
    ``return_accepted``: also the accepted proposals (trajectories when ``leapfrog > 1``) per rung and chain, int32 ``[K - 1, N *
    replicas]`` (None when unadjusted).
    ``return_ancestors``: also the ancestor of every chain at every rung, int32 ``[K - 1, N * replicas]``, as indices into the chains
    of the call (None without resampling; the identity where a datum did not resample)."""
    from .predictive_coding import recognise
    loss_fn_kwargs = dict(loss_fn_kwargs or {})
    if "_target" in loss_fn_kwargs:
        raise ValueError("mcpc_ais: loss_fn_kwargs holds a _target; `data` is the target")
    ladder = schedule(stages, power, betas)
    check_adjust(adjust)
    trainer.mcpc_last_ais_resampling = None          # a call that raises leaves no trace behind
    resample, ess_threshold = check_resample(resample, ess_threshold, replicas)
    check_counts(replicas, steps_per_stage, noise_var, seed, step_base)
    check_leapfrog(leapfrog, adjust, noise_var)
    check_gradients(gradients, adjust)
    net, why = recognise.describe_model(trainer._model)
    if net is None:
        raise NotImplementedError("mcpc_ais: outside what the HIP engine expresses ({})".format(why))
    if net.n_out == 0:
        raise NotImplementedError("mcpc_ais: the model ends in a PCLayer; the evidence is that of a read-out's data")
    if loss_fn is None:
        raise NotImplementedError("mcpc_ais: a read-out distribution is needed (bernoulli_fn, fe_fn or their masked forms)")
    model_device = net.linears[0].weight.device
    if not isinstance(data, torch.Tensor):
        data = torch.tensor(data)                # a copy: the array may be read-only
    if data.dim() != 2 or data.shape[1] != net.n_out:
        raise ValueError(f"data: expected [N, {net.n_out}], got {tuple(data.shape)}")
    n_data = int(data.shape[0])
    # everything the call can refuse is refused here, before a device is asked for
    kw = dict(loss_fn_kwargs, _target=torch.zeros(1, net.n_out, device=model_device))       # (the loss is recognised by its kind alone)
    loss, why = recognise.describe_loss(loss_fn, kw, net.n_out, 1, model_device)
    if loss is None:
        raise NotImplementedError("mcpc_ais: outside what the HIP engine expresses ({})".format(why))
    if loss.kind not in (L.LOSS_BERNOULLI, L.LOSS_GAUSSIAN):
        raise NotImplementedError("mcpc_ais: the read-out is Bernoulli (bernoulli_fn) or Gaussian (fe_fn), masked or not")
    if lr is None:
        xopt, why = (None, "manual_optimizer_x_fn is set") if trainer._manual_optimizer_x_fn is not None else \
            recognise.describe_x_optimizer(trainer._optimizer_x_fn, trainer._optimizer_x_kwargs)
        lr = resolve_lr(None, xopt, why or "optimizer_x_fn is {}".format(getattr(trainer._optimizer_x_fn, "__name__", trainer._optimizer_x_fn)))
    else:
        lr = resolve_lr(lr, None)
    parts = chunks(n_data, replicas, max_chains, chain_base)
    plan = trainer._plan_or_raise("mcpc_ais", loss_fn, kw, model_alone=True)
    net, loss = plan["net"], plan["loss"]
    device = plan["device"]
    n_active = net.n_out - loss.mask_start
    const = log_norm(loss.kind, n_active, loss.var)
    y_all = data.to(device=device, dtype=torch.float32).contiguous()
    K = len(ladder) - 1
    call = SimpleNamespace(adjust=adjust, ladder=ladder, steps_per_stage=steps_per_stage, lr=lr, noise_var=float(noise_var), seed=seed,
                           step_base=step_base, act=net.acts[-1], loss=loss, resample=resample, ess_threshold=ess_threshold,
                           replicas=replicas, leapfrog=leapfrog, gradients=gradients)
    states, logws, accepts, diags, ancestors = [], [], [], [], []
    engines = []
    try:
        with torch.cuda.device(device):
            for d0, n, g0 in parts:
                B = n * replicas
                eng = trainer._engine_for(dict(plan, B=B))
                if all(eng is not e for e in engines):
                    engines.append(eng)
                trainer._sync_params(eng, net, plan=plan)
                weights, biases = eng.bound_params()
                W_L, b_L = weights[-1], biases[-1]
                y = y_all[d0:d0 + n].repeat_interleave(replicas, dim=0).contiguous()
                eng.bind_inputs(None)
                eng.bind_target(y)
                scaled = None
                if loss.kind == L.LOSS_BERNOULLI:
                    # the scaled read-out of the rung, a scratch copy the engine is bound to for the length of the chunk
                    scaled = (W_L.clone(), None if b_L is None else b_L.clone())
                    eng.bind_params(weights[:-1] + [scaled[0]], biases[:-1] + [scaled[1]])      # (re-packed per rung by the ladder)
                _, xs = eng.sample_prior(B, seed, step=step_base, sample_base=g0, latents=True, readout=None)
                if gradients != "evaluator":             # (the evaluator reads the chains' own tensors: the engine's state stays)
                    eng.load_state(xs)
                logw = torch.zeros(B, dtype=torch.float64, device=device)
                chunk = SimpleNamespace(eng=eng, xs=xs, y=y, logw=logw, g0=g0, W_L=W_L, b_L=b_L, scaled=scaled)
                if resample is not None:
                    chunk.smc_diag = torch.zeros(K - 1, n, 4, dtype=torch.float64, device=device)
                    chunk.ancestors = torch.empty(K - 1, B, dtype=torch.int32, device=device)
                accepts.append(_ladder(call, chunk))
                eng.sync_check()
                states.append(fold(logw, replicas, const))
                if return_logw:
                    logws.append(logw)
                if resample is not None:
                    diags.append(chunk.smc_diag)
                    ancestors.append(chunk.ancestors + d0 * replicas)       # rows of the chunk -> chains of the call
    finally:
        # the engines are cached (and shared with train_on_batch): each one holds the model's own read-out again
        for eng in engines:
            trainer._rebind_own_params(eng, plan)
    state = torch.cat(states, dim=0) if states else empty_state(0, device)
    res = LogLikelihood(state=state.to(plan["model_device"]))
    accepted = None
    if adjust == "mala":
        accepted = torch.cat(accepts, dim=1) if accepts else torch.zeros(K - 1, 0, dtype=torch.int32, device=device)
        # the share of accepted proposals per rung over all chains of the call
        trainer.mcpc_last_ais_acceptance = (accepted.sum(dim=1).to(torch.float64) / max(1, accepted.shape[1] * steps_per_stage)).to(
            plan["model_device"])
    else:
        trainer.mcpc_last_ais_acceptance = None
    anc = None
    if resample is not None:
        diag = torch.cat(diags, dim=1) if diags else torch.zeros(K - 1, 0, 4, dtype=torch.float64, device=device)
        anc = torch.cat(ancestors, dim=1) if ancestors else torch.zeros(K - 1, 0, dtype=torch.int32, device=device)
        resampled = diag[:, :, 1] != 0.0
        to = plan["model_device"]
        # the ESS of every datum BEFORE its rung's resampling, what was resampled, and the share of the data resampled per rung
        trainer.mcpc_last_ais_resampling = SimpleNamespace(
            ess=diag[:, :, 0].contiguous().to(to), resampled=resampled.to(to),
            share=(resampled.sum(dim=1).to(torch.float64) / max(1, resampled.shape[1])).to(to))
    out = (res,)
    if return_logw:
        out += (torch.cat(logws) if logws else torch.zeros(0, dtype=torch.float64, device=device),)
    if return_accepted:
        out += (accepted,)
    if return_ancestors:
        out += (anc,)
    return out if len(out) > 1 else res

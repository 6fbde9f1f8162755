"""Trainer factories: the three trainer shapes the scripts use.

Counterpart of /root/reference/utils/training_evaluation.py:16-70 (same config keys).
"""
import torch.optim as optim

from .. import predictive_coding as pc
# (the reference's module carries these names too -- figure_4.py:13 imports fe_fn from utils.training_evaluation)
from .model import bernoulli_fn, bernoulli_fn_mask, fe_fn, fe_fn_mask        # noqa: F401


def __getattr__(name):
    """Names of the reference's utils/training_evaluation.py that are not on the hot path (train, test, MNIST_LinearClassifier, KLdivergence,
    kl_divergence_discrete, get_paired_stat, get_fid): when a script runs under the launcher they come from the script's own module of that
    name (montecarlopredictivecoding_amd/run.py: script_own_attr); otherwise they do not exist here."""
    if name.startswith("__"):
        raise AttributeError(name)
    from ..run import script_own_attr
    return script_own_attr("utils.training_evaluation", name)


def get_pc_trainer(gen_pc, config, is_mcpc=False, training=True):
    """MAP / PC inference: T_pc steps, user optimizer on x, no noise (reference :16-39)."""
    common = dict(T=config["T_pc"], update_x_at="all", optimizer_x_fn=config["optimizer_x_fn_pc"],
                  optimizer_x_kwargs=config["optimizer_x_kwargs_pc"], early_stop_condition="False",
                  plot_progress_at=[])
    if is_mcpc:
        return pc.PCTrainer(gen_pc, update_p_at="never", **common)
    return pc.PCTrainer(gen_pc, update_p_at="last" if training else "never",
                        optimizer_p_fn=config["optimizer_p_fn"], optimizer_p_kwargs=config["optimizer_p_kwargs"],
                        **common)


def get_mcpc_trainer(gen_pc, config, training=True):
    """MCPC: mixing + sampling Langevin steps, gradients accumulated over the sampling steps (reference :43-56)."""
    mixing, sampling = config["mixing"], config["sampling"]
    return pc.PCTrainer(
        gen_pc, T=mixing + sampling, update_x_at="all", optimizer_x_fn=optim.SGD,
        optimizer_x_kwargs=config["optimizer_x_kwargs_mcpc"],
        update_p_at="last" if training else "never",
        accumulate_p_at=[mixing + i for i in range(sampling)],
        optimizer_p_fn=config["optimizer_p_fn_mcpc"] if training else optim.SGD,
        optimizer_p_kwargs=config["optimizer_p_kwargs_mcpc"] if training else {"lr": 0.0},
        plot_progress_at=[])


def get_mcpc_trainer_one_sample(gen_pc, config, training=True):
    """MCPC with a single Monte Carlo sample: K steps, update from the last one only (reference :58-70)."""
    return pc.PCTrainer(
        gen_pc, T=config["K"], update_x_at="all", optimizer_x_fn=optim.SGD,
        optimizer_x_kwargs=config["optimizer_x_kwargs_mcpc"],
        update_p_at="last" if training else "never",
        optimizer_p_fn=config["optimizer_p_fn_mcpc"] if training else optim.SGD,
        optimizer_p_kwargs=config["optimizer_p_kwargs_mcpc"] if training else {"lr": 0.0},
        plot_progress_at=[])


# ---- ancestral sampler and evaluators (reference utils/training_evaluation.py:72-100,140-206) -------------
def _cpu_normal_like(temp):
    """Standard normals of temp's shape drawn from torch's CPU generator and moved to temp's device -- the stream the
    reference consumes (training_evaluation.py:73-79 draws `torch.randn((N, n, 1))` on the CPU and `.cuda()`s it), so that a
    `torch.manual_seed` pins the ancestral sample on the GPU exactly as it does in the reference."""
    import torch
    return torch.randn(tuple(temp.shape)).to(temp.device)


def sample_pc(num_samples, model, config, use_cuda=False, is_return_hidden=False):
    """Ancestral sample of the generative model: unit-variance Gaussian noise is added at every PCLayer
    (the prior of a PC layer with the default energy), the read-out is sampled from the sensory
    distribution (Gaussian with ``input_var`` / Bernoulli of the logits) unless ``is_return_hidden``."""
    import torch
    from ..utils.model import bernoulli_fn, fe_fn
    device = next(model.parameters()).device
    temp = torch.zeros(num_samples, config["input_size"], device=device)
    with torch.no_grad():
        for module in model:
            if isinstance(module, pc.PCLayer):
                temp = temp + _cpu_normal_like(temp)
            else:
                temp = module(temp)
        if is_return_hidden:
            return temp.detach()
        if config["loss_fn"] is fe_fn:
            temp = temp + (config["input_var"] ** 0.5) * _cpu_normal_like(temp)
        elif config["loss_fn"] is bernoulli_fn:
            temp = (torch.rand_like(temp) <= temp.sigmoid()).double()
    return temp.detach()


def sample_pc_device(num_samples, model, config, use_cuda=False, is_return_hidden=False, seed=0, step=0, sample_base=0,
                     return_latents=False):
    """``sample_pc`` on the device (``PCTrainer.mcpc_sample_prior``; include/mcpc.h: mcpc_sample_prior): the same ancestral pass with
    the normals of the step kernels' Philox stream instead of torch's CPU generator and every Linear on the engine's packed weights.
    Sample ``i`` is a function of ``(seed, step, sample_base + i)`` and the parameters alone, so chunks drawn with an advancing
    ``sample_base`` are the bits of one draw; ``torch.manual_seed`` does not reach it.  ``config["loss_fn"]`` / ``config["input_var"]``
    choose the read-out draw as in ``sample_pc``; ``is_return_hidden`` returns the read-out as it is.  A PCLayer's noise has the variance
    ``1 / c`` of its energy coefficient ``c`` (``sample_pc`` adds unit noise whatever ``c``; with the default ``c = 1`` the two agree).
    Returns fp32 ``[num_samples, n_out]`` on the model's device -- Bernoulli draws are fp32 0/1 where the reference returns doubles --
    or, with ``return_latents``, ``(that, [x_l])``.  A model the engine does not express raises NotImplementedError; without a HIP
    device, MCPCLibraryError."""
    from ..engine import check_sample_prior
    from ..predictive_coding import recognise
    from ..utils.model import bernoulli_fn, fe_fn
    net, why = recognise.describe_model(model)
    if net is None:
        raise NotImplementedError("sample_pc_device: outside what the HIP engine expresses ({})".format(why))
    if net.n_in != config["input_size"]:
        raise ValueError("sample_pc_device: config['input_size']={} but the model takes {} inputs".format(config["input_size"], net.n_in))
    if net.n_out == 0:
        raise NotImplementedError("sample_pc_device: the model ends in a PCLayer, there is no read-out to sample "
                                  "(PCTrainer.mcpc_sample_prior(latents=True) returns its layers)")
    loss_fn = None if is_return_hidden or config["loss_fn"] not in (fe_fn, bernoulli_fn) else config["loss_fn"]
    kw = {"_var": config["input_var"]} if loss_fn is fe_fn else {}
    readout = "hidden" if loss_fn is None else "draw"
    check_sample_prior(len(net.sizes), net.n_out, num_samples, sample_base, {None: None, fe_fn: "gaussian", bernoulli_fn: "bernoulli"}[loss_fn],
                       kw.get("_var"), readout, bool(return_latents))
    trainer = pc.PCTrainer(model, update_p_at="never", plot_progress_at=[])
    out, xs = trainer.mcpc_sample_prior(num_samples, seed=seed, step=step, sample_base=sample_base, loss_fn=loss_fn, loss_fn_kwargs=kw,
                                        readout=readout, latents=bool(return_latents))
    return (out, xs) if return_latents else out


def get_mse_rec(gen_pc, config, dataloader, use_cuda):
    """Masked-reconstruction error: infer (MAP) from the bottom half of each image, score the top half."""
    import torch
    from ..utils.model import bernoulli_fn, bernoulli_fn_mask, fe_fn, fe_fn_mask
    loss_fn = {fe_fn: fe_fn_mask, bernoulli_fn: bernoulli_fn_mask}[config["loss_fn"]]
    gen_pc.train()
    device = next(gen_pc.parameters()).device
    pc_trainer = get_pc_trainer(gen_pc, config, training=False, is_mcpc=True)
    mse, n_data = 0.0, 0
    for data, _ in dataloader:
        data = data.to(device)
        pseudo_input = torch.zeros(data.shape[0], config["input_size"], device=device)
        pc_trainer.train_on_batch(inputs=pseudo_input, loss_fn=loss_fn,
                                  loss_fn_kwargs={"_target": data, "_var": config["input_var"]},
                                  is_log_progress=False, is_return_results_every_t=False,
                                  is_checking_after_callback_after_t=False)
        with torch.no_grad():
            img = gen_pc[-1](gen_pc[-2](gen_pc[-3].get_x().detach()))
            if config["loss_fn"] is bernoulli_fn:
                img = (img > 0).type_as(img)          # logits: threshold at 0
            half = round(data.shape[1] / 2)
            mse += float(((img[:, :-half] - data[:, :-half]) ** 2).mean(1).sum())
        n_data += data.shape[0]
    return mse / n_data


def get_mse_rec_posterior(gen_pc, config, dataloader, use_cuda):
    """Masked-reconstruction error of the posterior-predictive mean: ``get_mse_rec``'s protocol (infer from the bottom half of each
    image under the masked loss, score the top half), with the reconstruction E[output | bottom half] over the ``sampling`` steps that
    follow ``mixing`` steps of an MCPC call started from the MAP state.  The mean is accumulated on the device by the call itself
    (``PCTrainer.mcpc_moments``): the Bernoulli mean sigmoid(logits), thresholded at 0.5, for ``bernoulli_fn``; the read-out itself
    for ``fe_fn``."""
    import torch
    from ..utils.model import bernoulli_fn, bernoulli_fn_mask, fe_fn, fe_fn_mask, random_step
    loss_fn = {fe_fn: fe_fn_mask, bernoulli_fn: bernoulli_fn_mask}[config["loss_fn"]]
    is_bernoulli = config["loss_fn"] is bernoulli_fn
    gen_pc.train()
    device = next(gen_pc.parameters()).device
    pc_trainer = get_pc_trainer(gen_pc, config, training=False, is_mcpc=True)
    mcpc_trainer = get_mcpc_trainer(gen_pc, config, training=False)
    mcpc_trainer.mcpc_moments = dict(begin=config["mixing"], stride=1, layers=(), outputs="sigmoid" if is_bernoulli else "identity",
                                     variance=False)
    mse, n_data = 0.0, 0
    for data, _ in dataloader:
        data = data.to(device)
        pseudo_input = torch.zeros(data.shape[0], config["input_size"], device=device)
        kw = dict(inputs=pseudo_input, loss_fn=loss_fn, loss_fn_kwargs={"_target": data, "_var": config["input_var"]},
                  is_log_progress=False, is_return_results_every_t=False, is_checking_after_callback_after_t=False)
        pc_trainer.train_on_batch(**kw)
        mcpc_trainer.train_on_batch(callback_after_t=random_step, callback_after_t_kwargs={"_pc_trainer": mcpc_trainer},
                                    is_sample_x_at_batch_start=False, **kw)
        img = mcpc_trainer.mcpc_last_moments.out_mean
        if is_bernoulli:
            img = (img > 0.5).type_as(img)
        half = round(data.shape[1] / 2)
        mse += float(((img[:, :-half] - data[:, :-half]) ** 2).mean(1).sum())
        n_data += data.shape[0]
    return mse / n_data


def get_map_free_energy(gen_pc, config, dataloader, use_cuda):
    """Free energy of every datum at its MAP state: ``get_mse_rec``'s protocol (one MAP call per batch from a zero pseudo-input) under
    the UNMASKED loss of the config, then ``overall`` per chain -- read-out loss plus layer energies of the state the call left --
    evaluated on the device (``PCTrainer.mcpc_state_energies``).  Returns one fp64 ``[N]`` tensor on the model's device, in the
    loader's order."""
    import torch
    gen_pc.train()
    device = next(gen_pc.parameters()).device
    pc_trainer = get_pc_trainer(gen_pc, config, training=False, is_mcpc=True)
    out = []
    for data, _ in dataloader:
        data = data.to(device)
        pseudo_input = torch.zeros(data.shape[0], config["input_size"], device=device)
        kw = dict(inputs=pseudo_input, loss_fn=config["loss_fn"], loss_fn_kwargs={"_target": data, "_var": config["input_var"]})
        pc_trainer.train_on_batch(is_log_progress=False, is_return_results_every_t=False, is_checking_after_callback_after_t=False, **kw)
        out.append(pc_trainer.mcpc_state_energies(**kw).overall[0])
    return torch.cat(out)


def marginal_likelihood_from_logits(logits, dataloader):
    """log (1/S) sum_s p(y | o_s), averaged over the data, for read-out logits o_s [S, n0] (clamped to +-20 as the reference
    does, training_evaluation.py:177) -- the likelihood core of get_marginal_likelihood as a function of the prior samples.
    BCE(o, y) summed over pixels = sum softplus(o) - y.o, so the [B, S, n0] tensor the reference materialises per batch
    (:190-193) becomes one [B, n0] x [n0, S] product."""
    import torch
    logits = logits.clamp(-20, 20)
    sp = torch.nn.functional.softplus(logits).sum(1)                                                       # sum_j log(1+e^o)
    total, count = 0.0, 0
    with torch.no_grad():
        for data, _ in dataloader:
            data = data.to(logits.device).to(logits.dtype)
            nll = sp.unsqueeze(0) - data @ logits.t()                                                       # [B, S]
            m = nll.min(1).values
            p = torch.exp(-(nll - m.unsqueeze(1))).mean(1)
            total += float((torch.log(p) - m).sum())
            count += data.shape[0]
    return total / count


def get_marginal_likelihood(gen_pc, config, dataloader, use_cuda, n_samples=5000):
    """Importance-sampled log marginal likelihood per datum (Bernoulli read-out), samples from the prior."""
    from ..utils.model import bernoulli_fn
    if config["loss_fn"] is not bernoulli_fn:
        raise NotImplementedError("the reference implements the Bernoulli read-out only (training_evaluation.py:196)")
    logits = sample_pc(n_samples, gen_pc, config, use_cuda=use_cuda, is_return_hidden=True)                 # [S, n0]
    return marginal_likelihood_from_logits(logits, dataloader)


def get_marginal_likelihood_per_datum(gen_pc, config, dataloader, use_cuda, n_samples=5000, sample_chunk=None, clamp=20.0, sampler="torch",
                                      seed=0):
    """``get_marginal_likelihood`` per datum, in fp64 on the device, for both read-outs: a ``likelihood.LogLikelihood`` over the loader's
    data, in the loader's order -- ``.log_p`` per datum, ``.ess`` (the effective sample size of its importance weights),
    ``.n_samples``; ``.mean()`` is the reference's scalar.  The data are gathered onto the model's device once.  The prior samples are
    drawn with ``sample_pc(..., is_return_hidden=True)``: ``sample_chunk=None`` draws all ``n_samples`` at once and consumes the torch
    generator exactly as ``get_marginal_likelihood`` does (the same seed gives the same samples); otherwise they are drawn
    ``sample_chunk`` at a time and the state is accumulated over the chunks, so ``n_samples`` is not bounded by memory.
    ``bernoulli_fn`` reads the samples' read-outs as logits, ``fe_fn`` as means of a Gaussian of variance ``config["input_var"]``;
    both are clamped to ``+-clamp`` as the reference clamps (``math.inf``: not at all).
    ``sampler="device"`` draws every chunk with ``sample_pc_device(..., is_return_hidden=True, seed=seed, sample_base=s0)`` instead: the
    samples are then the same bits whatever ``sample_chunk`` is (only the accumulation's documented rounding bound remains), no normal
    is drawn on the CPU, and the torch generator is not consumed by the draws."""
    import torch
    from ..likelihood import log_likelihood
    from ..utils.model import bernoulli_fn, fe_fn
    if config["loss_fn"] is bernoulli_fn:
        loss, var = "bernoulli", None
    elif config["loss_fn"] is fe_fn:
        loss, var = "gaussian", float(config["input_var"])
    else:
        raise NotImplementedError("get_marginal_likelihood_per_datum: the read-out is bernoulli_fn or fe_fn")
    n_samples = int(n_samples)
    chunk = n_samples if sample_chunk is None else int(sample_chunk)
    if n_samples < 1 or chunk < 1:
        raise ValueError(f"n_samples={n_samples} and sample_chunk={sample_chunk!r} must be at least 1")
    if sampler not in ("torch", "device"):
        raise ValueError(f"sampler={sampler!r}, expected 'torch' or 'device'")
    device = next(gen_pc.parameters()).device
    data, state = None, None
    for s0 in range(0, n_samples, chunk):
        if sampler == "device":
            outputs = sample_pc_device(min(chunk, n_samples - s0), gen_pc, config, use_cuda=use_cuda, is_return_hidden=True, seed=seed,
                                       sample_base=s0)
        else:
            outputs = sample_pc(min(chunk, n_samples - s0), gen_pc, config, use_cuda=use_cuda, is_return_hidden=True)
        if data is None:
            # after the first draw, as get_marginal_likelihood walks its loader: a DataLoader's iterator takes a seed from the torch generator
            data = torch.cat([d.to(device).to(torch.float32).reshape(d.shape[0], -1) for d, _ in dataloader])
        state = log_likelihood(data, outputs, loss=loss, var=var, clamp=clamp, state=state)
    return state


def get_marginal_likelihood_ais(gen_pc, config, dataloader, use_cuda, replicas=64, stages=64, steps_per_stage=5, seed=0, **kw):
    """The log marginal likelihood per datum by annealed importance sampling on the device (``PCTrainer.mcpc_ais``): a
    ``likelihood.LogLikelihood`` over the loader's data, in the loader's order.  Where ``get_marginal_likelihood_per_datum`` weighs
    prior samples -- an effective sample size of about 1 on an image -- every datum here gets ``replicas`` chains that are annealed from
    the prior to its posterior over ``stages`` rungs of ``steps_per_stage`` Langevin steps.  The trainer is the MCPC trainer of
    ``config`` (``get_mcpc_trainer``: SGD on x with ``config["optimizer_x_kwargs_mcpc"]``, whose ``lr`` is the Langevin step size);
    ``config["loss_fn"]`` / ``config["input_var"]`` name the read-out.  Batch ``b`` of the loader uses the chain ids that follow those
    of the batches before it, so the result does not depend on the batch size.  ``kw``: further keywords of ``mcpc_ais`` (``power``,
    ``betas``, ``lr``, ``noise_var``, ``step_base``, ``chain_base``, ``max_chains``, ``adjust``, ``resample``, ``ess_threshold``, ``leapfrog``, ``gradients`` -- with ``adjust="mala", leapfrog=L`` each of a rung's
    ``steps_per_stage`` transitions is a Hamiltonian trajectory of L leapfrog steps; ``gradients="evaluator"`` evaluates an adjusted transition's
    proposals with one ``Engine.state_gradients`` call each)."""
    from ..likelihood import LogLikelihood
    from ..utils.model import bernoulli_fn, fe_fn
    if config["loss_fn"] not in (bernoulli_fn, fe_fn):
        raise NotImplementedError("get_marginal_likelihood_ais: the read-out is bernoulli_fn or fe_fn")
    loss_kw = {"_var": config["input_var"]} if config["loss_fn"] is fe_fn else {}
    gen_pc.train()
    device = next(gen_pc.parameters()).device
    trainer = get_mcpc_trainer(gen_pc, config, training=False)
    chain_base = int(kw.pop("chain_base", 0))
    parts = []
    for data, _ in dataloader:
        data = data.to(device).reshape(data.shape[0], -1)
        parts.append(trainer.mcpc_ais(data, config["loss_fn"], loss_kw, replicas=replicas, stages=stages, steps_per_stage=steps_per_stage,
                                      seed=seed, chain_base=chain_base, **kw))
        chain_base += data.shape[0] * replicas
    return LogLikelihood.cat(parts)


def knn_kl_divergence(x, y):
    """The nearest-neighbour (Perez-Cruz) estimate of D(P || Q) between samples ``x`` of P and ``y`` of Q on the device: what the
    reference's ``KLdivergence(x, y)`` (:240-284) estimates, by exact brute force instead of two KD-trees queried with ``eps=.01``, so
    that figure 5's clouds need no thinning (``cloud.kl_divergence``; ``x``, ``y``: ``cloud.Cloud``, tensors or arrays ``[rows, d]``).
    A 0-d fp64 tensor."""
    from ..cloud import kl_divergence
    return kl_divergence(x, y)

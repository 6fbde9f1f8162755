"""Loss functions, x initialisers, the Langevin callback and the MLP factory.

Counterpart of /root/reference/utils/model.py:8-69 (same names, arguments and numerical meaning).
Every callable that the HIP engine can fuse carries a ``_mcpc`` tag; the torch bodies below are what
the tags *mean* (they are executed only by the opt-in generic path and by the loss recogniser's
self-check), the fused path maps the tag to a kernel epilogue:

    fe_fn / fe_fn_mask            -> MCPC_LOSS_GAUSSIAN  (+ mask_start)
    bernoulli_fn / *_mask         -> MCPC_LOSS_BERNOULLI (+ mask_start)
    zero_fn                       -> MCPC_LOSS_NONE
    random_step                   -> MCPC_NOISE_PHILOX inside the x update
"""
import numpy as np
import torch
import torch.nn as nn

from ..predictive_coding.pc_layer import PCLayer


def __getattr__(name):
    """A name of the script's own utils/model.py that this module does not define (the reference's has none: every name of its
    utils/model.py:8-163 is here) comes from the script's own module when it runs under the launcher (run.py: script_own_attr)."""
    if name.startswith("__"):
        raise AttributeError(name)
    from ..run import script_own_attr
    return script_own_attr("utils.model", name)


# ---- x initialisers (reference utils/model.py:8-15) --------------------------------------------------
def sample_x_fn(inputs):
    return inputs["mu"].detach().clone().uniform_(-10.0, 10.0)


def sample_x_fn_normal(inputs):
    return torch.randn_like(inputs["mu"])


def sample_x_fn_cte(inputs):
    return 3 * torch.ones_like(inputs["mu"])


# ---- losses (reference utils/model.py:17-33) --------------------------------------------------------
def _last_columns(n_out, perc):
    return round(n_out * perc)


def fe_fn(output, _target, _var):
    return (1 / _var) * 0.5 * (output - _target).pow(2).sum()


def bernoulli_fn(output, _target, _var=None, _reduction="sum"):
    return nn.functional.binary_cross_entropy_with_logits(output, _target, reduction=_reduction)


def fe_fn_mask(output, _target, _var, perc=0.5):
    k = _last_columns(output.shape[1], perc)
    return (1 / _var) * 0.5 * (output[:, -k:] - _target[:, -k:]).pow(2).sum()


def bernoulli_fn_mask(output, _target, _var=None, perc=0.5):
    k = _last_columns(output.shape[1], perc)
    return nn.functional.binary_cross_entropy_with_logits(output[:, -k:], _target[:, -k:], reduction="sum")


def zero_fn(output):
    return torch.tensor(0.0)


fe_fn._mcpc = dict(loss="gaussian", masked=False)
fe_fn_mask._mcpc = dict(loss="gaussian", masked=True)
bernoulli_fn._mcpc = dict(loss="bernoulli", masked=False)
bernoulli_fn_mask._mcpc = dict(loss="bernoulli", masked=True)
zero_fn._mcpc = dict(loss="none", masked=False)


# ---- the Langevin kick (reference utils/model.py:35-44) -------------------------------------------------
def random_step(t, _pc_trainer, var=2.0):
    """x <- x + sqrt(var*lr)*xi.  ``var`` must be 2 for a correct posterior sampler.

    Passed as ``callback_after_t`` it is recognised by its tag and fused into the HIP x-update
    (counter-based Philox noise, no callback is actually invoked per step).  When it IS invoked
    (step-wise path, i.e. next to other user callbacks) it does what the reference does: overwrite
    every x.grad with N(0, sqrt(var/lr)) and step the x optimizer once more.
    """
    xs = _pc_trainer.get_model_xs()
    optimizer = _pc_trainer.get_optimizer_x()
    std = np.sqrt(var / optimizer.defaults["lr"])
    for x in xs:
        if x.grad is None:
            x.grad = torch.zeros_like(x)
        x.grad.normal_(0.0, std)
    optimizer.step()


random_step._mcpc = dict(langevin=True)


# ---- model factory (reference utils/model.py:47-69) -----------------------------------------------------
def get_model(config, use_cuda, sample_x_fn=sample_x_fn):
    act = {"relu": nn.ReLU, "tanh": nn.Tanh}[config["activation_fn"]]
    n1, n2, n3, n0 = config["input_size"], config["hidden_size"], config["hidden2_size"], config["output_size"]
    gen_pc = nn.Sequential(
        nn.Linear(n1, n1), PCLayer(sample_x_fn=sample_x_fn), act(),
        nn.Linear(n1, n2), PCLayer(sample_x_fn=sample_x_fn), act(),
        nn.Linear(n2, n3), PCLayer(sample_x_fn=sample_x_fn), act(),
        nn.Linear(n3, n0),
    )
    gen_pc.train()
    if use_cuda:
        gen_pc.cuda()
    return gen_pc


# ---- representations for down-stream probes (reference utils/model.py:71-163) ----------------------------
def get_representations(gen_pc, config, trainers, loader, rep_type="MAP", use_cuda=False, n=None):
    """Top-latent-layer representations of every batch of ``loader`` as a ``TensorDataset``.

    rep_type "MAP"          x_1 after PC (MAP) inference with ``trainers[0]``;
             "expectation"  mean of x_1 over ALL recorded Langevin steps of ``trainers[1]`` (started from the MAP state);
             "full"         every ``sampling/n``-th sample after the mixing phase, labels repeated ``n`` times.
    The Langevin trajectories come back from the engine's device-side record buffer in one copy.
    """
    from torch.utils.data import TensorDataset
    device = next(gen_pc.parameters()).device
    input_size = len(gen_pc[0].bias)
    reps, labels = [], []
    if rep_type != "MAP":
        if len(trainers) != 2:
            raise NotImplementedError
        assert rep_type in ("full", "expectation")
    pc_trainer = trainers[0]
    stride = 1
    if rep_type == "full":
        if n is not None:
            stride = int(config["sampling"] / n)
        else:
            n = config["sampling"]
    for data, label in loader:
        pseudo_input = torch.zeros(data.shape[0], input_size, device=device)
        data, label = data.to(device), label.to(device)
        kw = dict(inputs=pseudo_input, loss_fn=config["loss_fn"],
                  loss_fn_kwargs={"_target": data, "_var": config["input_var"]},
                  is_return_results_every_t=False, is_checking_after_callback_after_t=False)
        pc_trainer.train_on_batch(is_log_progress=(rep_type == "MAP"), **kw)
        if rep_type == "MAP":
            reps.append(gen_pc[1].get_x().detach().clone())
            labels.append(label)
            continue
        mcpc_trainer = trainers[1]
        kw["is_return_results_every_t"] = True
        results = mcpc_trainer.train_on_batch(
            callback_after_t=random_step, callback_after_t_kwargs={"_pc_trainer": mcpc_trainer},
            is_log_progress=False, is_sample_x_at_batch_start=False, is_return_representations=True, **kw)
        traj = torch.stack(results["representations"]).to(device)          # [T, B, n_1]
        if rep_type == "expectation":
            reps.append(traj.mean(0))
            labels.append(label)
        else:
            kept = traj[config["mixing"]::stride]
            reps.append(kept.reshape(-1, traj.shape[2]))
            labels.append(label.repeat(n))
    return TensorDataset(torch.cat(reps, dim=0), torch.cat(labels, dim=0))


def get_posterior_expectation(gen_pc, config, trainers, loader, use_cuda=False, with_variance=False):
    """The ``TensorDataset`` of ``get_representations(..., rep_type="expectation")`` -- MAP call with ``trainers[0]``, then an MCPC call
    with ``trainers[1]`` started from the MAP state, mean of x_1 over all T steps -- with the mean accumulated on the device by the
    call itself (``PCTrainer.mcpc_moments``, fp64 sums): no trajectory is recorded to the host or kept.  ``with_variance`` adds a third
    tensor, the per-unit posterior variance (unbiased, over the same T steps)."""
    from torch.utils.data import TensorDataset
    if len(trainers) != 2:
        raise NotImplementedError
    device = next(gen_pc.parameters()).device
    input_size = len(gen_pc[0].bias)
    pc_trainer, mcpc_trainer = trainers
    means, variances, labels = [], [], []
    saved = mcpc_trainer.mcpc_moments
    mcpc_trainer.mcpc_moments = dict(begin=0, stride=1, layers=(0,), outputs=None, variance=bool(with_variance))
    try:
        for data, label in loader:
            pseudo_input = torch.zeros(data.shape[0], input_size, device=device)
            data, label = data.to(device), label.to(device)
            kw = dict(inputs=pseudo_input, loss_fn=config["loss_fn"],
                      loss_fn_kwargs={"_target": data, "_var": config["input_var"]},
                      is_log_progress=False, is_return_results_every_t=False, is_checking_after_callback_after_t=False)
            pc_trainer.train_on_batch(**kw)
            mcpc_trainer.train_on_batch(callback_after_t=random_step, callback_after_t_kwargs={"_pc_trainer": mcpc_trainer},
                                        is_sample_x_at_batch_start=False, **kw)
            m = mcpc_trainer.mcpc_last_moments
            means.append(m.x_mean[0])
            if with_variance:
                variances.append(m.x_var[0])
            labels.append(label)
    finally:
        mcpc_trainer.mcpc_moments = saved
    tensors = [torch.cat(means, dim=0), torch.cat(labels, dim=0)]
    if with_variance:
        tensors.append(torch.cat(variances, dim=0))
    return TensorDataset(*tensors)


def get_posterior_covariance(gen_pc, config, trainers, loader, layers=(0,), pool=None):
    """Posterior means and covariances of the latent units, per batch of ``loader``: MAP call with ``trainers[0]``, then an MCPC call
    with ``trainers[1]`` started from the MAP state (the protocol of ``get_posterior_expectation``), over the steps from
    ``config["mixing"]`` on, accumulated on the device by the call itself (``PCTrainer.mcpc_covariance``, fp64 sums on the fp64 MFMA):
    no trajectory is recorded.  ``layers``: the PC layers whose units are the columns; ``pool``: None for one matrix per datum, "chains"
    for one per batch.  Returns ``(means, covariances, labels)``: per datum ``[N, D]`` / ``[N, D, D]`` fp64 and ``[N]``; pooled, one
    ``[D]`` / ``[D, D]`` per batch stacked into ``[batches, D]`` / ``[batches, D, D]``, and the labels of all data."""
    if len(trainers) != 2:
        raise NotImplementedError
    device = next(gen_pc.parameters()).device
    input_size = len(gen_pc[0].bias)
    pc_trainer, mcpc_trainer = trainers
    means, covs, labels = [], [], []
    saved = mcpc_trainer.mcpc_covariance
    mcpc_trainer.mcpc_covariance = dict(begin=int(config["mixing"]), stride=1, layers=tuple(layers), outputs=None, pool=pool)
    try:
        for data, label in loader:
            pseudo_input = torch.zeros(data.shape[0], input_size, device=device)
            data, label = data.to(device), label.to(device)
            kw = dict(inputs=pseudo_input, loss_fn=config["loss_fn"],
                      loss_fn_kwargs={"_target": data, "_var": config["input_var"]},
                      is_log_progress=False, is_return_results_every_t=False, is_checking_after_callback_after_t=False)
            pc_trainer.train_on_batch(**kw)
            mcpc_trainer.train_on_batch(callback_after_t=random_step, callback_after_t_kwargs={"_pc_trainer": mcpc_trainer},
                                        is_sample_x_at_batch_start=False, **kw)
            c = mcpc_trainer.mcpc_last_covariance
            if pool is None:
                means.append(c.mean)
                covs.append(c.cov(ddof=1))
            else:
                means.append(c.mean.unsqueeze(0))
                covs.append(c.cov(ddof=1).unsqueeze(0))
            labels.append(label)
    finally:
        mcpc_trainer.mcpc_covariance = saved
    return torch.cat(means, dim=0), torch.cat(covs, dim=0), torch.cat(labels, dim=0)


def get_posterior_error_statistics(gen_pc, config, trainers, loader, layers=(0,), quantity="error", outputs=None):
    """Posterior means, variances and rms of the error units ``eps_l = x_l - mu_l`` (``quantity="error"``) or of the predictions
    ``mu_l`` (``"prediction"``), per batch of ``loader``: MAP call with ``trainers[0]``, then an MCPC call with ``trainers[1]`` started
    from the MAP state (the protocol of ``get_posterior_covariance``), over the steps from ``config["mixing"]`` on, evaluated and
    accumulated on the device by the call itself (``PCTrainer.mcpc_errors``): no trajectory is recorded and no forward pass is
    replayed.  ``layers``: the PC layers asked for; ``outputs``: None, "error" or "prediction" for the read-out.  Returns ``(means,
    variances, rms, labels)``: three dicts by block name ("e0".. / "mu0".., "eout" / "out") of fp64 ``[N, n_l]`` over all data in the
    loader's order, and the labels ``[N]``."""
    if len(trainers) != 2:
        raise NotImplementedError
    device = next(gen_pc.parameters()).device
    input_size = len(gen_pc[0].bias)
    pc_trainer, mcpc_trainer = trainers
    means, variances, rms, labels = {}, {}, {}, []
    saved = mcpc_trainer.mcpc_errors
    mcpc_trainer.mcpc_errors = dict(begin=int(config["mixing"]), stride=1, layers=tuple(layers), quantity=quantity, outputs=outputs)
    try:
        for data, label in loader:
            pseudo_input = torch.zeros(data.shape[0], input_size, device=device)
            data, label = data.to(device), label.to(device)
            kw = dict(inputs=pseudo_input, loss_fn=config["loss_fn"],
                      loss_fn_kwargs={"_target": data, "_var": config["input_var"]},
                      is_log_progress=False, is_return_results_every_t=False, is_checking_after_callback_after_t=False)
            pc_trainer.train_on_batch(**kw)
            mcpc_trainer.train_on_batch(callback_after_t=random_step, callback_after_t_kwargs={"_pc_trainer": mcpc_trainer},
                                        is_sample_x_at_batch_start=False, **kw)
            e = mcpc_trainer.mcpc_last_errors
            for name in e.names:
                means.setdefault(name, []).append(e.mean(name))
                variances.setdefault(name, []).append(e.var(name, ddof=1))
                rms.setdefault(name, []).append(e.rms(name))
            labels.append(label)
    finally:
        mcpc_trainer.mcpc_errors = saved

    def cat(d):
        return {k: torch.cat(v, dim=0) for k, v in d.items()}
    return cat(means), cat(variances), cat(rms), torch.cat(labels, dim=0)


def get_posterior_histogram(gen_pc, config, trainers, loader, layers=(0,), bins=50, range=None, pool=None):
    """Posterior histograms of the latent units, per batch of ``loader``: MAP call with ``trainers[0]``, then an MCPC call with
    ``trainers[1]`` started from the MAP state (the protocol of ``get_posterior_covariance``), over the steps from ``config["mixing"]``
    on, counted on the device by the call itself (``PCTrainer.mcpc_histogram``, integer counters in LDS): no trajectory is recorded.
    ``layers``: the PC layers whose units are binned; ``bins`` / ``range``: as in ``mcpc_histogram`` (an int with ``range=(lo, hi)``, or
    edges; the range is never taken from the data); ``pool``: None for one histogram per datum, "chains" for one per unit.  Returns
    ``(histogram, labels)``: a ``histogram.Histogram`` whose chains are all data in the loader's order (``B`` = their number), or, pooled,
    the merge of the batches' histograms (``n`` = the samples of all batches; the batches must be of one size, ``Histogram.merge``); and
    the labels of all data."""
    from ..histogram import Histogram
    if len(trainers) != 2:
        raise NotImplementedError
    device = next(gen_pc.parameters()).device
    input_size = len(gen_pc[0].bias)
    pc_trainer, mcpc_trainer = trainers
    parts, labels = [], []
    saved = mcpc_trainer.mcpc_histogram
    mcpc_trainer.mcpc_histogram = dict(begin=int(config["mixing"]), stride=1, layers=tuple(layers), outputs=None, bins=bins, range=range,
                                       pool=pool)
    try:
        for data, label in loader:
            pseudo_input = torch.zeros(data.shape[0], input_size, device=device)
            data, label = data.to(device), label.to(device)
            kw = dict(inputs=pseudo_input, loss_fn=config["loss_fn"],
                      loss_fn_kwargs={"_target": data, "_var": config["input_var"]},
                      is_log_progress=False, is_return_results_every_t=False, is_checking_after_callback_after_t=False)
            pc_trainer.train_on_batch(**kw)
            mcpc_trainer.train_on_batch(callback_after_t=random_step, callback_after_t_kwargs={"_pc_trainer": mcpc_trainer},
                                        is_sample_x_at_batch_start=False, **kw)
            parts.append(mcpc_trainer.mcpc_last_histogram)
            labels.append(label)
    finally:
        mcpc_trainer.mcpc_histogram = saved
    first = parts[0]
    if pool is not None:
        for h in parts[1:]:
            first = first.merge(h)
        return first, torch.cat(labels, dim=0)

    def cat(field):
        return {k: torch.cat([getattr(h, field)[k] for h in parts], dim=0) for k in first.names}
    whole = Histogram(n=first.n, B=sum(h.B for h in parts), pooled=False, names=list(first.names), edges=dict(first.edges),
                      counts=cat("counts"), under=cat("under"), over=cat("over"), nan=cat("nan"))
    return whole, torch.cat(labels, dim=0)


def get_posterior_ess(gen_pc, config, trainers, loader, layers=(0,), max_lag=32):
    """How far the posterior samples of the latent units can be trusted, per batch of ``loader``: MAP call with ``trainers[0]``, then an
    MCPC call with ``trainers[1]`` started from the MAP state (the protocol of ``get_posterior_histogram``), over the steps from
    ``config["mixing"]`` on; the call itself adds the lagged products of every (datum, unit) on the device
    (``PCTrainer.mcpc_autocovariance``): no trajectory is recorded.  ``layers``: the PC layers looked at; ``max_lag``: the largest lag
    kept (0..64).  Returns ``(autocovariance, labels)``: an ``autocovariance.Autocovariance`` whose chains are all data in the loader's
    order (``B`` = their number; ``.acf``, ``.tau``, ``.ess``, ``.mcse``, ``.truncated`` per datum and unit), and the labels of all
    data."""
    from ..autocovariance import Autocovariance
    if len(trainers) != 2:
        raise NotImplementedError
    device = next(gen_pc.parameters()).device
    input_size = len(gen_pc[0].bias)
    pc_trainer, mcpc_trainer = trainers
    parts, labels = [], []
    saved = mcpc_trainer.mcpc_autocovariance
    mcpc_trainer.mcpc_autocovariance = dict(begin=int(config["mixing"]), stride=1, layers=tuple(layers), outputs=None, max_lag=max_lag)
    try:
        for data, label in loader:
            pseudo_input = torch.zeros(data.shape[0], input_size, device=device)
            data, label = data.to(device), label.to(device)
            kw = dict(inputs=pseudo_input, loss_fn=config["loss_fn"],
                      loss_fn_kwargs={"_target": data, "_var": config["input_var"]},
                      is_log_progress=False, is_return_results_every_t=False, is_checking_after_callback_after_t=False)
            pc_trainer.train_on_batch(**kw)
            mcpc_trainer.train_on_batch(callback_after_t=random_step, callback_after_t_kwargs={"_pc_trainer": mcpc_trainer},
                                        is_sample_x_at_batch_start=False, **kw)
            parts.append(mcpc_trainer.mcpc_last_autocovariance)
            labels.append(label)
    finally:
        mcpc_trainer.mcpc_autocovariance = saved
    return Autocovariance.cat(parts), torch.cat(labels, dim=0)


def get_posterior_class_probabilities(gen_pc, config, trainers, loader, classifier, layer=0, link="softmax"):
    """The posterior class probabilities a linear classifier on a latent layer assigns, per batch of ``loader``: MAP call with
    ``trainers[0]``, then an MCPC call with ``trainers[1]`` started from the MAP state (the protocol of ``get_posterior_ess``), over
    the steps from ``config["mixing"]`` on; the call itself applies the classifier to every sample of the layer on the device and adds
    the class probabilities, their squares, the argmax votes and the entropies (``PCTrainer.mcpc_probe``): no trajectory is recorded
    (the reference loops over the recorded representations on the host, figure_2.py ``comparison_ideal_observer``).  ``classifier``: an
    ``nn.Linear`` on the layer, or a module that holds exactly one (``MNIST_LinearClassifier``).  Returns ``(probe, labels)``: a
    ``probe.Probe`` whose chains are all data in the loader's order (``Probe.cat`` of the batches; ``.mean``, ``.var``,
    ``.vote_share``, ``.predict``, ``.entropy``, ``.expected_entropy``, ``.mutual_information`` per datum), and the labels of all
    data."""
    from ..probe import Probe
    if len(trainers) != 2:
        raise NotImplementedError
    linears = [m for m in classifier.modules() if isinstance(m, torch.nn.Linear)]
    if len(linears) != 1:
        raise ValueError("get_posterior_class_probabilities: the classifier must be an nn.Linear or hold exactly one, it holds {}".format(
            len(linears)))
    device = next(gen_pc.parameters()).device
    input_size = len(gen_pc[0].bias)
    pc_trainer, mcpc_trainer = trainers
    parts, labels = [], []
    saved = mcpc_trainer.mcpc_probe
    mcpc_trainer.mcpc_probe = dict(begin=int(config["mixing"]), stride=1, layer=layer, linear=linears[0], link=link)
    try:
        for data, label in loader:
            pseudo_input = torch.zeros(data.shape[0], input_size, device=device)
            data, label = data.to(device), label.to(device)
            kw = dict(inputs=pseudo_input, loss_fn=config["loss_fn"],
                      loss_fn_kwargs={"_target": data, "_var": config["input_var"]},
                      is_log_progress=False, is_return_results_every_t=False, is_checking_after_callback_after_t=False)
            pc_trainer.train_on_batch(**kw)
            mcpc_trainer.train_on_batch(callback_after_t=random_step, callback_after_t_kwargs={"_pc_trainer": mcpc_trainer},
                                        is_sample_x_at_batch_start=False, **kw)
            parts.append(mcpc_trainer.mcpc_last_probe)
            labels.append(label)
    finally:
        mcpc_trainer.mcpc_probe = saved
    return Probe.cat(parts), torch.cat(labels, dim=0)


def get_posterior_class_density(gen_pc, config, trainers, loader, classifier, layer=0, link="softmax", bins=40, range=(-1, 1), project=None,
                                pool=None):
    """The joint density of a linear classifier's class probabilities on a latent layer, projected onto a plane, per batch of
    ``loader`` (the reference's figure_2.py, ``posterior_non_linear_model``: panels 2c and 2d): MAP call with ``trainers[0]``, then an
    MCPC call with ``trainers[1]`` started from the MAP state (the protocol of ``get_posterior_class_probabilities``), over the steps
    from ``config["mixing"]`` on; the call itself applies the classifier to every sample of the layer, projects the link values with
    ``project`` (fp32 ``[2, C]``; None = the regular C-gon of ``proba_to_coordinate``) and bins the two coordinates jointly on the device
    (``PCTrainer.mcpc_histogram2d``): no trajectory is recorded.  ``bins`` / ``range`` as the request takes them.  ``classifier``: an
    ``nn.Linear`` on the layer, or a module that holds exactly one.  Returns one ``histogram2d.Histogram2D`` over all data in the
    loader's order, one grid per datum (``Histogram2D.cat`` of the batches; with ``pool="chains"`` the batches' pooled grids merged).
    The loader's labels are not consulted."""
    from ..histogram2d import Histogram2D
    if len(trainers) != 2:
        raise NotImplementedError
    linears = [m for m in classifier.modules() if isinstance(m, torch.nn.Linear)]
    if len(linears) != 1:
        raise ValueError("get_posterior_class_density: the classifier must be an nn.Linear or hold exactly one, it holds {}".format(
            len(linears)))
    device = next(gen_pc.parameters()).device
    input_size = len(gen_pc[0].bias)
    pc_trainer, mcpc_trainer = trainers
    parts = []
    saved = mcpc_trainer.mcpc_histogram2d
    mcpc_trainer.mcpc_histogram2d = dict(begin=int(config["mixing"]), stride=1, probe=dict(layer=layer, linear=linears[0], link=link),
                                         project=project, bins=bins, range=range, pool=pool)
    try:
        for data, _ in loader:
            pseudo_input = torch.zeros(data.shape[0], input_size, device=device)
            data = data.to(device)
            kw = dict(inputs=pseudo_input, loss_fn=config["loss_fn"],
                      loss_fn_kwargs={"_target": data, "_var": config["input_var"]},
                      is_log_progress=False, is_return_results_every_t=False, is_checking_after_callback_after_t=False)
            pc_trainer.train_on_batch(**kw)
            mcpc_trainer.train_on_batch(callback_after_t=random_step, callback_after_t_kwargs={"_pc_trainer": mcpc_trainer},
                                        is_sample_x_at_batch_start=False, **kw)
            parts.append(mcpc_trainer.mcpc_last_histogram2d)
    finally:
        mcpc_trainer.mcpc_histogram2d = saved
    if pool is None:
        density = Histogram2D.cat(parts)
    else:
        density = parts[0]
        for part in parts[1:]:
            density = density.merge(part)
    return density


def get_posterior_cloud(gen_pc, config, trainers, loader, layer=2, units=None, loss_fn=None):
    """The posterior samples themselves of a few units of one latent layer, per batch of ``loader``: MAP call with ``trainers[0]``,
    then an MCPC call with ``trainers[1]`` started from the MAP state (the protocol of ``get_posterior_ess``), over the steps from
    ``config["mixing"]`` on; the call itself gathers the units' samples out of its record ring into a device tensor
    (``PCTrainer.mcpc_cloud``): no trajectory goes to the host (the reference records every layer with ``is_return_xs`` and keeps 5
    units of one, figure_5.py).  ``units``: 1..32 unit indices of the layer (None = all of a layer at most 32 wide).  ``loss_fn``: the
    loss of both calls, ``config["loss_fn"]`` by default; ``zero_fn`` gives figure 5's spontaneous activity (the data are then not
    looked at).  Returns a ``cloud.Cloud`` on the engine's device whose chains are all data in the loader's order (``Cloud.cat`` of
    the batches): the input of ``cloud.kl_divergence``."""
    from ..cloud import Cloud
    if len(trainers) != 2:
        raise NotImplementedError
    device = next(gen_pc.parameters()).device
    input_size = len(gen_pc[0].bias)
    pc_trainer, mcpc_trainer = trainers
    loss_fn = config["loss_fn"] if loss_fn is None else loss_fn
    parts = []
    saved = mcpc_trainer.mcpc_cloud
    mcpc_trainer.mcpc_cloud = dict(begin=int(config["mixing"]), stride=1, layer=layer, units=None if units is None else tuple(units))
    try:
        for batch in loader:
            data = batch[0] if isinstance(batch, (tuple, list)) else batch
            pseudo_input = torch.zeros(data.shape[0], input_size, device=device)
            data = data.to(device)
            kw = dict(inputs=pseudo_input, loss_fn=loss_fn,
                      loss_fn_kwargs={} if loss_fn is zero_fn else {"_target": data, "_var": config["input_var"]},
                      is_log_progress=False, is_return_results_every_t=False, is_checking_after_callback_after_t=False)
            pc_trainer.train_on_batch(**kw)
            mcpc_trainer.train_on_batch(callback_after_t=random_step, callback_after_t_kwargs={"_pc_trainer": mcpc_trainer},
                                        is_sample_x_at_batch_start=False, **kw)
            parts.append(mcpc_trainer.mcpc_last_cloud)
    finally:
        mcpc_trainer.mcpc_cloud = saved
    return Cloud.cat(parts)


def get_variability_time_course(gen_pc, config, trainers, data, window=1000, every=1, layers=None):
    """How the variability of the latent units changes when a stimulus sets in (the reference's figure_5.py,
    ``variability_stimulus_onset_nonlinear``), on one batch ``data``: a MAP call with ``trainers[0]`` and an MCPC call with
    ``trainers[1]`` from its state, both without a loss; then an MCPC call under ``zero_fn`` (no input) that starts a stream of samples,
    and an MCPC call under ``config["loss_fn"]`` on ``data`` that carries the stream on.  The two calls themselves reduce, on the
    device, the standard deviation of the last ``window`` samples of every (datum, unit) and its mean and spread across them, per
    ``every``-th step (``PCTrainer.mcpc_rolling`` with ``carry=``): no trajectory is recorded (the reference records every step of
    every layer and takes pandas' ``rolling(window).std()`` of them), and the windows of the second call's first ``window - 1`` rows
    reach back into the first.  ``layers``: the PC layers looked at (None = all).  Returns the ``rolling.Rolling`` of both calls joined
    in time; ``.all()`` pools the layers, ``.mean_std`` / ``.sem`` of it are the figure's line and band, and the stimulus sets in at
    step ``T`` of ``.steps``.  The plain mean and standard deviation across all series are given, not the reference's average of
    per-chunk standard deviations; the mean is the same quantity."""
    from ..rolling import Rolling
    if len(trainers) != 2:
        raise NotImplementedError
    device = next(gen_pc.parameters()).device
    input_size = len(gen_pc[0].bias)
    pc_trainer, mcpc_trainer = trainers
    if layers is None:
        layers = range(sum(isinstance(m, PCLayer) for m in gen_pc.modules()))
    pseudo_input = torch.zeros(data.shape[0], input_size, device=device)
    data = data.to(device)
    quiet = dict(is_log_progress=False, is_return_results_every_t=False, is_checking_after_callback_after_t=False)
    mc = dict(callback_after_t=random_step, callback_after_t_kwargs={"_pc_trainer": mcpc_trainer}, is_sample_x_at_batch_start=False)
    request = dict(begin=0, stride=1, layers=tuple(layers), outputs=None, window=int(window), every=int(every), pool="all")
    saved = mcpc_trainer.mcpc_rolling
    try:
        mcpc_trainer.mcpc_rolling = None
        pc_trainer.train_on_batch(inputs=pseudo_input, **quiet)
        mcpc_trainer.train_on_batch(inputs=pseudo_input, **mc, **quiet)
        mcpc_trainer.mcpc_rolling = dict(request)
        mcpc_trainer.train_on_batch(inputs=pseudo_input, loss_fn=zero_fn, loss_fn_kwargs={}, **mc, **quiet)
        before = mcpc_trainer.mcpc_last_rolling
        mcpc_trainer.mcpc_rolling = dict(request, carry=before)
        mcpc_trainer.train_on_batch(inputs=pseudo_input, loss_fn=config["loss_fn"],
                                    loss_fn_kwargs={"_target": data, "_var": config["input_var"]}, **mc, **quiet)
        after = mcpc_trainer.mcpc_last_rolling
    finally:
        mcpc_trainer.mcpc_rolling = saved
    return Rolling.cat([before, after], dim="time")

"""The posterior of a linear probe on a latent layer of a Langevin call: the request (``PCTrainer.mcpc_probe``) and the result
(``PCTrainer.mcpc_last_probe``).

The reference's classification result is not a statistic of the units: ``figure_2.py`` (``comparison_ideal_observer``) trains a linear
classifier on the top latent layer, records 10 000 steps of an MCPC call and adds ``softmax(classifier(representation))`` over the
recorded steps on the host.  Here the fused call applies the read-out to every sample of the layer out of its record ring on the device
(csrc/mcpc_probe.h: one lane per chain and class, fp64 logits that are bitwise a sequential loop, however the call is sliced) and keeps
four sums per chain: the class probabilities, their squares, the argmax votes and the entropy of each sample's softmax.  The predictive
distribution, its Monte Carlo spread and the split of its uncertainty (H[mean p] against mean H[p]) follow without a trajectory.  This
module holds no device code: validation of the request, which steps are samples, and the fp64 arithmetic on the sums.
"""
from dataclasses import dataclass
from typing import Optional

import torch

from .sampling import SampleWindow, parse_keys, parse_layer, parse_window, sample_steps  # noqa: F401

_KEYS = ("begin", "stride", "layer", "weight", "bias", "linear", "link")
LINKS = ("identity", "sigmoid", "softmax")
MAX_CLASSES = 64                                 # include/mcpc.h: MCPC_PROBE_MAX_CLASSES


@dataclass(frozen=True, eq=False)
class ProbeSpec(SampleWindow):
    """A validated ``mcpc_probe`` request for a call of ``T`` steps.  ``weight`` / ``bias`` are the caller's tensors, detached."""
    layer: int
    weight: torch.Tensor
    bias: Optional[torch.Tensor]
    link: str
    C: int

    def on(self, device):
        """(W, bias or None) as contiguous fp32 on ``device``: what the kernel reads."""
        w = self.weight.to(device=device, dtype=torch.float32).contiguous()
        b = None if self.bias is None else self.bias.to(device=device, dtype=torch.float32).contiguous()
        return w, b


def validate_spec(spec, T: int, n_layers: int, sizes, B: int) -> ProbeSpec:
    """``PCTrainer.mcpc_probe`` -> ProbeSpec, or ValueError: not a dict, unknown keys, ``begin`` outside [0, T), ``stride`` < 1, no
    ``layer`` or one out of range, both or neither of ``linear`` and ``weight``, a weight that is not ``[C, sizes[layer]]`` with C in
    1..64, a bias that is not ``[C]``, an unknown link.  Defaults: begin=0, stride=1, bias=None, link="softmax"."""
    parse_keys("mcpc_probe", spec, _KEYS)
    begin, stride = parse_window("mcpc_probe", spec, T)
    layer = parse_layer("mcpc_probe", spec, n_layers, "the probe reads")
    linear, weight, bias = spec.get("linear"), spec.get("weight"), spec.get("bias")
    if linear is not None and (weight is not None or bias is not None):
        raise ValueError("mcpc_probe: both linear and weight / bias are given; pass one of them")
    if linear is None and weight is None:
        raise ValueError("mcpc_probe: neither linear nor weight is given: the probe needs its read-out")
    if linear is not None:
        if not isinstance(linear, torch.nn.Linear):
            raise ValueError(f"mcpc_probe: linear must be a torch.nn.Linear, got {type(linear).__name__}")
        weight, bias = linear.weight, linear.bias
    if not isinstance(weight, torch.Tensor) or weight.dim() != 2:
        raise ValueError("mcpc_probe: weight must be a 2-D tensor [classes, width], got {}".format(
            tuple(weight.shape) if isinstance(weight, torch.Tensor) else type(weight).__name__))
    width = int(sizes[layer])
    C = int(weight.shape[0])
    if int(weight.shape[1]) != width:
        raise ValueError(f"mcpc_probe: weight is {tuple(weight.shape)}, layer {layer} is {width} wide: expected [classes, {width}]")
    if not 1 <= C <= MAX_CLASSES:
        raise ValueError(f"mcpc_probe: weight has {C} classes, outside 1..{MAX_CLASSES}")
    if bias is not None and (not isinstance(bias, torch.Tensor) or tuple(bias.shape) != (C,)):
        raise ValueError("mcpc_probe: bias must be a tensor of shape ({},), got {}".format(
            C, tuple(bias.shape) if isinstance(bias, torch.Tensor) else type(bias).__name__))
    link = spec.get("link", "softmax")
    if link not in LINKS:
        raise ValueError(f"mcpc_probe: link={link!r}, expected 'softmax', 'sigmoid' or 'identity'")
    return ProbeSpec(begin=begin, stride=stride, layer=layer, weight=weight.detach(), bias=None if bias is None else bias.detach(),
                     link=link, T=T, C=C)


@dataclass
class Probe:
    """The sums of one fused call, on the model's device: ``n`` samples per chain of ``B`` chains, ``C`` classes, with p the link values
    of a sample's logits: ``psum`` fp64 ``[B, C]`` the sums of p, ``psumsq`` fp64 ``[B, C]`` of p^2, ``votes`` int64 ``[B, C + 1]`` the
    samples whose largest logit is the class (column C: samples with a NaN logit, which cast no vote), ``entsum`` fp64 ``[B]`` the summed
    entropies of the samples' softmax (softmax only, else None).  Everything derived is fp64 torch, per chain."""
    n: int
    B: int
    C: int
    link: str
    psum: torch.Tensor
    psumsq: torch.Tensor
    votes: torch.Tensor
    entsum: Optional[torch.Tensor] = None

    def mean(self) -> torch.Tensor:
        """The mean link value over the window, ``[B, C]``: with softmax the posterior class probabilities."""
        return self.psum / self.n

    def var(self, ddof: int = 0) -> torch.Tensor:
        """The variance of the link values over the window, ``[B, C]``, clamped at 0."""
        m = self.mean()
        return torch.clamp(self.psumsq / self.n - m * m, min=0.0) * (self.n / (self.n - ddof))

    def vote_share(self) -> torch.Tensor:
        """The share of the samples whose largest logit is the class, ``[B, C]`` (samples with a NaN logit count in none)."""
        return self.votes[:, :self.C].to(torch.float64) / self.n

    def predict(self) -> torch.Tensor:
        """The class of the largest mean, int64 ``[B]``."""
        return torch.argmax(self.mean(), dim=1)

    def _softmax_only(self, what):
        if self.link != "softmax":
            raise ValueError(f"Probe.{what}: the entropies are those of class probabilities; this probe's link is {self.link!r}")

    def entropy(self) -> torch.Tensor:
        """H[mean p], the entropy of the predictive distribution, ``[B]`` (nats; 0 log 0 = 0)."""
        self._softmax_only("entropy")
        m = self.mean()
        return -torch.where(m > 0, m * torch.log(torch.where(m > 0, m, torch.ones_like(m))), torch.zeros_like(m)).sum(dim=1)

    def expected_entropy(self) -> torch.Tensor:
        """mean H[p], the mean entropy of the samples' own distributions, ``[B]``."""
        self._softmax_only("expected_entropy")
        return self.entsum / self.n

    def mutual_information(self) -> torch.Tensor:
        """H[mean p] - mean H[p], ``[B]``: the part of the predictive uncertainty that comes from the spread of the samples."""
        self._softmax_only("mutual_information")
        return self.entropy() - self.expected_entropy()

    @staticmethod
    def cat(parts) -> "Probe":
        """The results of different batches (same request, same n) joined along the chains."""
        parts = list(parts)
        first = parts[0]
        if any((p.n, p.C, p.link) != (first.n, first.C, first.link) for p in parts):
            raise ValueError("Probe.cat: the results are of different requests")

        def join(f):
            return torch.cat([getattr(p, f) for p in parts], dim=0)
        return Probe(n=first.n, B=sum(p.B for p in parts), C=first.C, link=first.link, psum=join("psum"), psumsq=join("psumsq"),
                     votes=join("votes"), entsum=join("entsum") if first.link == "softmax" else None)

    def merge(self, other: "Probe") -> "Probe":
        """The same chains with the samples of ``other`` added: the sums add."""
        if (other.B, other.C, other.link) != (self.B, self.C, self.link):
            raise ValueError("Probe.merge: the results are of different chains or requests")
        return Probe(n=self.n + other.n, B=self.B, C=self.C, link=self.link, psum=self.psum + other.psum,
                     psumsq=self.psumsq + other.psumsq, votes=self.votes + other.votes,
                     entsum=self.entsum + other.entsum if self.link == "softmax" else None)


def new_state(B: int, C: int, link: str, device):
    """Zeroed accumulators of a probe on ``device``: dict(psum, psumsq, votes, entsum)."""
    return dict(psum=torch.zeros(B, C, dtype=torch.float64, device=device), psumsq=torch.zeros(B, C, dtype=torch.float64, device=device),
                votes=torch.zeros(B, C + 1, dtype=torch.int64, device=device),
                entsum=torch.zeros(B, dtype=torch.float64, device=device) if link == "softmax" else None)


def from_state(n: int, B: int, C: int, link: str, state, device) -> Probe:
    """The kernel's accumulators (``new_state``) -> Probe on ``device``."""
    return Probe(n=n, B=B, C=C, link=link, psum=state["psum"].to(device), psumsq=state["psumsq"].to(device),
                 votes=state["votes"].to(device), entsum=None if state["entsum"] is None else state["entsum"].to(device))

"""Posterior moments of a Langevin call: the request (``PCTrainer.mcpc_moments``) and the result (``PCTrainer.mcpc_last_moments``).

The reference consumes an MCPC call as statistics over its sampling window (``get_representations(rep_type="expectation")``,
utils/model.py:150-156; the means and histograms of figure_2.py / figure_3.py) and computes them in torch from the recorded steps.
Here the fused call reduces its records on the device (csrc/mcpc_moments.h) and the trajectory is never materialised.  This module
holds no device code: validation of the request, which steps are samples, and the fp64 arithmetic from sums to mean and variance.
"""
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import torch

from .sampling import SampleWindow, parse_keys, parse_layers, parse_outputs, parse_window, sample_steps  # noqa: F401

_KEYS = ("begin", "stride", "layers", "outputs", "variance")
_OUTPUTS = (None, "identity", "sigmoid")


@dataclass(frozen=True)
class MomentsSpec(SampleWindow):
    """A validated ``mcpc_moments`` request for a call of ``T`` steps."""
    layers: Tuple[int, ...]
    outputs: Optional[str]
    variance: bool


def validate_spec(spec, T: int, n_layers: int, n_out: int) -> MomentsSpec:
    """``PCTrainer.mcpc_moments`` -> MomentsSpec, or ValueError: unknown keys, ``begin`` outside [0, T), ``stride`` < 1, a layer
    index out of range, ``outputs`` on a model without a read-out.  Defaults: begin=0, stride=1, layers=(), outputs=None,
    variance=True."""
    parse_keys("mcpc_moments", spec, _KEYS)
    begin, stride = parse_window("mcpc_moments", spec, T)
    layers = parse_layers("mcpc_moments", spec, n_layers)          # layers=None is not a sequence here
    outputs = parse_outputs("mcpc_moments", spec, n_out, _OUTPUTS)
    return MomentsSpec(begin=begin, stride=stride, layers=layers, outputs=outputs,
                       variance=bool(spec.get("variance", True)), T=T)


def mean_from_sums(s: Optional[torch.Tensor], n: int) -> Optional[torch.Tensor]:
    """sum / n in fp64, then cast to fp32."""
    return None if s is None else (s / n).to(torch.float32)


def var_from_sums(s: Optional[torch.Tensor], q: Optional[torch.Tensor], n: int) -> Optional[torch.Tensor]:
    """max(0, (sumsq - sum^2 / n) / (n - 1)) in fp64, then cast to fp32; NaN for n = 1 (as torch.var of one sample)."""
    if s is None or q is None:
        return None
    if n < 2:
        return torch.full(s.shape, float("nan"), dtype=torch.float32, device=s.device)
    return ((q - s * s / n) / (n - 1)).clamp_(min=0.0).to(torch.float32)


@dataclass
class Moments:
    """Moments of one fused call, on the model's device.  ``x_*[l]`` is None for a layer not asked for, ``*_sumsq`` / ``*_var``
    are None with ``variance=False``.  The sums are raw fp64: the statistics of several calls merge by adding sums and ``n``
    (``merge``)."""
    n: int
    x_sum: List[Optional[torch.Tensor]] = field(default_factory=list)
    x_sumsq: List[Optional[torch.Tensor]] = field(default_factory=list)
    out_sum: Optional[torch.Tensor] = None
    out_sumsq: Optional[torch.Tensor] = None

    @property
    def x_mean(self):
        return [mean_from_sums(s, self.n) for s in self.x_sum]

    @property
    def x_var(self):
        return [var_from_sums(s, q, self.n) for s, q in zip(self.x_sum, self.x_sumsq)]

    @property
    def out_mean(self):
        return mean_from_sums(self.out_sum, self.n)

    @property
    def out_var(self):
        return var_from_sums(self.out_sum, self.out_sumsq, self.n)

    def merge(self, other: "Moments") -> "Moments":
        """The moments of both calls' samples together (same chains, same request)."""
        def add(a, b):
            return None if a is None or b is None else a + b
        return Moments(n=self.n + other.n, x_sum=[add(a, b) for a, b in zip(self.x_sum, other.x_sum)],
                       x_sumsq=[add(a, b) for a, b in zip(self.x_sumsq, other.x_sumsq)],
                       out_sum=add(self.out_sum, other.out_sum), out_sumsq=add(self.out_sumsq, other.out_sumsq))

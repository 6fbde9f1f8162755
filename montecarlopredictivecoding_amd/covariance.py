"""Posterior covariances of a Langevin call: the request (``PCTrainer.mcpc_covariance``) and the result
(``PCTrainer.mcpc_last_covariance``).

The covariance between units, within a layer and across layers, is what separates a sampler from a MAP estimator.  From a recorded
trajectory it is ``x.T @ x`` in fp64 over every step; here the fused call reduces its record ring on the device (csrc/mcpc_cov.h: fp64
sums of outer products on the fp64 MFMA; csrc/mcpc_moments.h: the first-order sums) and the trajectory is never materialised.  This module
holds no device code: validation of the request, which steps are samples, and the fp64 arithmetic from sums to mean, covariance and
correlation.
"""
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import torch

from .sampling import (SampleWindow, column_list, human_bytes, parse_keys, parse_layers, parse_outputs, parse_window,  # noqa: F401
                       require_columns, sample_steps)

_KEYS = ("begin", "stride", "layers", "outputs", "pool")
_OUTPUTS = (None, "identity", "sigmoid")
_POOLS = (None, "chains")


@dataclass(frozen=True)
class CovarianceSpec(SampleWindow):
    """A validated ``mcpc_covariance`` request for a call of ``T`` steps."""
    layers: Tuple[int, ...]
    outputs: Optional[str]
    pooled: bool
    columns: Tuple[Tuple[str, int, int], ...]       # (name, start, width) of every column group, in order

    @property
    def D(self) -> int:
        return sum(w for _, _, w in self.columns)


def result_bytes(D: int, B: int, pooled: bool) -> int:
    """Bytes of the result of a request, the fp64 outer products and first-order sums: what ``mcpc_covariance_max_bytes`` bounds.  (While
    the call runs the pooled form also holds the per-chain first-order sums, 8 B per chain and column, and the kernel's workspace,
    ``engine.cov_workspace_bytes``: bounded by the batch and the widths, not by the request.)"""
    return 8 * (D * D + D) * (1 if pooled else B)


def validate_spec(spec, T: int, n_layers: int, n_out: int, sizes, B: int, max_bytes: int) -> CovarianceSpec:
    """``PCTrainer.mcpc_covariance`` -> CovarianceSpec, or ValueError: not a dict, unknown keys, ``begin`` outside [0, T), ``stride``
    < 1, a layer index out of range, no column at all, ``outputs`` on a model without a read-out, an unknown ``pool``, a result larger
    than ``max_bytes``.  Defaults: begin=0, stride=1, layers=all latent layers, outputs=None, pool=None (one matrix per chain)."""
    parse_keys("mcpc_covariance", spec, _KEYS)
    begin, stride = parse_window("mcpc_covariance", spec, T)
    layers = parse_layers("mcpc_covariance", spec, n_layers, none_means="all")
    outputs = parse_outputs("mcpc_covariance", spec, n_out, _OUTPUTS)
    pool = spec.get("pool", None)
    if pool not in _POOLS:
        raise ValueError(f"mcpc_covariance: pool={pool!r}, expected None (one matrix per chain) or 'chains'")
    require_columns("mcpc_covariance", layers, outputs)
    columns = column_list(layers, sizes, None if outputs is None else "out", n_out, starts=True)
    start = sum(w for _, _, w in columns)
    pooled = pool == "chains"
    need = result_bytes(start, B, pooled)
    if need > max_bytes:
        what = f"one {start} x {start} fp64 matrix" if pooled else f"{B} chains x {start} x {start} fp64"
        raise ValueError(f"mcpc_covariance: the result ({what}) takes {human_bytes(need)}, more than mcpc_covariance_max_bytes = "
                         f"{human_bytes(max_bytes)}: ask for fewer layers" + ("" if pooled else " or pool='chains'"))
    return CovarianceSpec(begin=begin, stride=stride, layers=layers, outputs=outputs, pooled=pooled, T=T, columns=columns)


@dataclass
class Covariance:
    """Second moments of one fused call, on the model's device.  ``n`` samples per chain of ``B`` chains; ``columns`` names the column
    groups, ``(name, start, width)`` with names "x0", "x1", ... and "out".  ``sum`` / ``outer`` are the raw fp64 sums: ``[B, D]`` /
    ``[B, D, D]`` per chain, ``[D]`` / ``[D, D]`` pooled over the chains.  The statistics of several calls merge by adding sums and
    ``n`` (``merge``)."""
    n: int
    B: int
    pooled: bool
    columns: List[Tuple[str, int, int]] = field(default_factory=list)
    sum: Optional[torch.Tensor] = None
    outer: Optional[torch.Tensor] = None

    @property
    def N(self) -> int:
        """Samples behind one matrix."""
        return self.n * self.B if self.pooled else self.n

    @property
    def mean(self) -> torch.Tensor:
        """sum / N, fp64."""
        return self.sum / self.N

    def cov(self, ddof: int = 1) -> torch.Tensor:
        """(outer - sum sum^T / N) / (N - ddof) in fp64; NaN for N - ddof < 1."""
        N = self.N
        if N - ddof < 1:
            return torch.full_like(self.outer, float("nan"))
        s = self.sum
        return (self.outer - s.unsqueeze(-1) * s.unsqueeze(-2) / N) / (N - ddof)

    def corr(self) -> torch.Tensor:
        """cov / (sd sd^T), fp64 (NaN where a unit does not vary)."""
        c = self.cov(ddof=1)
        sd = torch.diagonal(c, dim1=-2, dim2=-1).sqrt()
        return c / (sd.unsqueeze(-1) * sd.unsqueeze(-2))

    def _span(self, name):
        for nm, start, width in self.columns:
            if nm == name:
                return slice(start, start + width)
        raise KeyError(f"no column group {name!r}; this result has {[c[0] for c in self.columns]}")

    def block(self, a: str, b: str, ddof: int = 1) -> torch.Tensor:
        """The covariance between the units of two named column groups: ``cov(ddof)[..., a, b]``."""
        return self.cov(ddof)[..., self._span(a), self._span(b)]

    def merge(self, other: "Covariance") -> "Covariance":
        """The sums of both calls' samples together (same chains, same request)."""
        if (self.B, self.pooled, list(self.columns)) != (other.B, other.pooled, list(other.columns)):
            raise ValueError("Covariance.merge: the two results are of different requests")
        return Covariance(n=self.n + other.n, B=self.B, pooled=self.pooled, columns=list(self.columns),
                          sum=self.sum + other.sum, outer=self.outer + other.outer)

"""Posterior statistics of the error units and predictions of a Langevin call: the request (``PCTrainer.mcpc_errors``) and the result
(``PCTrainer.mcpc_last_errors``).

The latent states ``x_l`` are half of a predictive-coding network's population; the other half are the error units ``eps_l = x_l -
mu_l`` and the predictions ``mu_l = f(x_{l-1}) W_l^T + b_l``.  From a recorded trajectory they need a forward pass replayed in torch
per step; here the fused call evaluates them out of its record ring on the device (csrc/mcpc_pred_err.h: the step kernels' own GEMM,
written per unit as DERIVED RECORDS in the layout of a record) and reduces the derived records with the reducers the states go
through (csrc/mcpc_moments.h, csrc/mcpc_cov.h).  This module holds no device code: validation of the request, which steps are samples,
the byte bound, and the fp64 arithmetic from sums to mean, variance and rms.
"""
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch

from .covariance import Covariance, result_bytes as cov_result_bytes
from .sampling import (SampleWindow, column_list, human_bytes, parse_keys, parse_layers, parse_outputs, parse_window,  # noqa: F401
                       require_columns, sample_steps)

_KEYS = ("begin", "stride", "layers", "quantity", "outputs", "variance", "covariance")
_QUANTITIES = ("error", "prediction")
_OUTPUTS = (None, "error", "prediction")
_COVARIANCES = (None, "chain", "chains")


def block_name(quantity: str, layer: Optional[int]) -> str:
    """"e0".. / "mu0".. for a latent layer, "eout" / "out" for the read-out (layer None)."""
    if layer is None:
        return "eout" if quantity == "error" else "out"
    return ("e" if quantity == "error" else "mu") + str(layer)


def layers_read(layers, with_output: bool, n_layers: int) -> Tuple[int, ...]:
    """The latent layers whose recorded states the evaluation reads: a requested layer itself and the layer below it (its
    prediction's input); the last layer for the read-out."""
    need = set()
    for l in layers:
        need.add(l)
        if l > 0:
            need.add(l - 1)
    if with_output:
        need.add(n_layers - 1)
    return tuple(sorted(need))


@dataclass(frozen=True)
class ErrorsSpec(SampleWindow):
    """A validated ``mcpc_errors`` request for a call of ``T`` steps."""
    layers: Tuple[int, ...]
    quantity: str
    outputs: Optional[str]
    variance: bool
    covariance: Optional[str]                       # None, "chain" (one matrix per chain) or "chains" (pooled over the chains)
    columns: Tuple[Tuple[str, int, int], ...]       # (name, start, width) of every block, in order
    reads: Tuple[int, ...]                          # latent layers that go through the record ring

    @property
    def D(self) -> int:
        return sum(w for _, _, w in self.columns)

    @property
    def pooled(self) -> bool:
        return self.covariance == "chains"

    def max_samples(self, n_steps: int) -> int:
        """The most samples a slice of n_steps steps can hold (a derived buffer has that many records)."""
        return min(self.n, -(-n_steps // self.stride))

    def bytes(self, B: int, rows: int) -> int:
        """What ``mcpc_errors_max_bytes`` bounds, for derived buffers of ``rows`` records."""
        return request_bytes(self.D, B, rows, self.variance, self.covariance)


def request_bytes(D: int, B: int, rows: int, variance: bool, covariance: Optional[str]) -> int:
    """Bytes a request of D columns on B chains holds on the device: the fp32 derived buffers of one ring half (``rows`` records), the
    fp64 sums (and sums of squares), and with ``covariance`` the result of that request (covariance.result_bytes)."""
    derived = 4 * rows * B * D
    sums = 8 * B * D * (2 if variance else 1)
    cov = 0 if covariance is None else cov_result_bytes(D, B, covariance == "chains")
    return derived + sums + cov


def check_bytes(spec: ErrorsSpec, B: int, rows: int, max_bytes: int):
    need = spec.bytes(B, rows)
    if need > max_bytes:
        raise ValueError(f"mcpc_errors: the request ({spec.D} columns x {B} chains: derived records of {rows} sample{'' if rows == 1 else 's'}, sums"
                         + ("" if spec.covariance is None else ", covariance") + f") takes {human_bytes(need)}, more than "
                         f"mcpc_errors_max_bytes = {human_bytes(max_bytes)}: ask for fewer layers"
                         + (" or covariance='chains'" if spec.covariance == "chain" else ""))


def validate_spec(spec, T: int, n_layers: int, n_out: int, sizes, B: int, has_loss: bool, max_bytes: int) -> ErrorsSpec:
    """``PCTrainer.mcpc_errors`` -> ErrorsSpec, or ValueError: not a dict, unknown keys, ``begin`` outside [0, T), ``stride`` < 1, a
    layer index out of range, an unknown ``quantity`` / ``outputs`` / ``covariance``, no column at all, ``outputs`` on a model without
    a read-out, ``outputs="error"`` on a call without a loss, a request that takes more than ``max_bytes`` even with derived buffers
    of one sample (the trainer checks again with the samples one slice holds, before anything runs).  Defaults: begin=0, stride=1,
    layers=(), quantity="error", outputs=None, variance=True, covariance=None."""
    parse_keys("mcpc_errors", spec, _KEYS)
    begin, stride = parse_window("mcpc_errors", spec, T)
    layers = parse_layers("mcpc_errors", spec, n_layers)            # layers=None is not a sequence here
    quantity = spec.get("quantity", "error")
    if quantity not in _QUANTITIES:
        raise ValueError(f"mcpc_errors: quantity={quantity!r}, expected 'error' or 'prediction'")
    outputs = parse_outputs("mcpc_errors", spec, n_out, _OUTPUTS)
    if outputs == "error" and not has_loss:
        raise ValueError("mcpc_errors: outputs='error' asked of a call without a loss (the read-out has no error then)")
    covariance = spec.get("covariance", None)
    if covariance not in _COVARIANCES:
        raise ValueError(f"mcpc_errors: covariance={covariance!r}, expected None, 'chain' (one matrix per chain) or 'chains' (pooled)")
    require_columns("mcpc_errors", layers, outputs)
    columns = column_list(layers, sizes, None if outputs is None else block_name(outputs, None), n_out,
                          layer_name=lambda l: block_name(quantity, l), starts=True)
    out = ErrorsSpec(begin=begin, stride=stride, layers=layers, quantity=quantity, outputs=outputs, variance=bool(spec.get("variance", True)),
                     covariance=covariance, T=T, columns=columns, reads=layers_read(layers, outputs is not None, n_layers))
    check_bytes(out, B, 1, max_bytes)
    return out


@dataclass
class Errors:
    """First and second moments of the error units / predictions of one fused call, on the model's device.  Per block name ("e0".. or
    "mu0".., "eout" or "out"): raw fp64 ``sum`` and ``sumsq`` of shape ``[B, n_l]`` (``sumsq`` is None with ``variance=False``) over
    ``n`` samples per chain.  ``covariance``: a covariance.Covariance over the same blocks when the request asked for it.  The
    statistics of several calls merge by adding sums and ``n`` (``merge``)."""
    n: int
    sum: Dict[str, torch.Tensor] = field(default_factory=dict)
    sumsq: Dict[str, Optional[torch.Tensor]] = field(default_factory=dict)
    covariance: Optional[Covariance] = None

    @property
    def names(self) -> List[str]:
        return list(self.sum)

    def _get(self, table, name):
        if name not in self.sum:
            raise KeyError(f"no block {name!r}; this result has {self.names}")
        return table[name]

    def mean(self, name: str) -> torch.Tensor:
        """sum / n, fp64."""
        return self._get(self.sum, name) / self.n

    def var(self, name: str, ddof: int = 1) -> torch.Tensor:
        """max(0, (sumsq - sum^2 / n) / (n - ddof)) in fp64; NaN for n - ddof < 1."""
        s, q = self._get(self.sum, name), self._get(self.sumsq, name)
        if q is None:
            raise ValueError("the request had variance=False: no sums of squares were kept")
        if self.n - ddof < 1:
            return torch.full_like(s, float("nan"))
        return ((q - s * s / self.n) / (self.n - ddof)).clamp_(min=0.0)

    def rms(self, name: str) -> torch.Tensor:
        """sqrt(sumsq / n), fp64: the size of an error unit whatever its mean."""
        q = self._get(self.sumsq, name)
        if q is None:
            raise ValueError("the request had variance=False: no sums of squares were kept")
        return (q / self.n).sqrt()

    def merge(self, other: "Errors") -> "Errors":
        """The sums of both calls' samples together (same chains, same request)."""
        if self.names != other.names or (self.covariance is None) != (other.covariance is None):
            raise ValueError("Errors.merge: the two results are of different requests")

        def add(a, b):
            return None if a is None or b is None else a + b
        return Errors(n=self.n + other.n, sum={k: self.sum[k] + other.sum[k] for k in self.sum},
                      sumsq={k: add(self.sumsq[k], other.sumsq[k]) for k in self.sum},
                      covariance=None if self.covariance is None else self.covariance.merge(other.covariance))

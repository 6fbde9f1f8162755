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

from .covariance import Covariance, human_bytes, result_bytes as cov_result_bytes

_KEYS = ("begin", "stride", "layers", "quantity", "outputs", "variance", "covariance")
_QUANTITIES = ("error", "prediction")
_OUTPUTS = (None, "error", "prediction")
_COVARIANCES = (None, "chain", "chains")


def sample_steps(begin: int, T: int, stride: int) -> range:
    """The steps of a call of T steps whose records are samples."""
    return range(begin, T, stride)


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
class ErrorsSpec:
    """A validated ``mcpc_errors`` request for a call of ``T`` steps."""
    begin: int
    stride: int
    layers: Tuple[int, ...]
    quantity: str
    outputs: Optional[str]
    variance: bool
    covariance: Optional[str]                       # None, "chain" (one matrix per chain) or "chains" (pooled over the chains)
    T: int
    columns: Tuple[Tuple[str, int, int], ...]       # (name, start, width) of every block, in order
    reads: Tuple[int, ...]                          # latent layers that go through the record ring

    @property
    def n(self) -> int:
        return len(sample_steps(self.begin, self.T, self.stride))

    @property
    def D(self) -> int:
        return sum(w for _, _, w in self.columns)

    @property
    def pooled(self) -> bool:
        return self.covariance == "chains"

    def chunk(self, t0: int, n_steps: int):
        """(first, count): the samples among steps t0 .. t0 + n_steps - 1 are rows first, first + stride, ... of a chunk that holds
        one record per step from t0 on."""
        f = self.begin if t0 <= self.begin else self.begin + -(-(t0 - self.begin) // self.stride) * self.stride
        return f - t0, len(range(f, min(t0 + n_steps, self.T), self.stride))

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
    if not isinstance(spec, dict):
        raise ValueError(f"mcpc_errors: expected a dict or None, got {type(spec).__name__}")
    unknown = sorted(k for k in spec if k not in _KEYS)
    if unknown:
        raise ValueError(f"mcpc_errors: unknown keys {unknown}; known: {list(_KEYS)}")
    begin, stride = spec.get("begin", 0), spec.get("stride", 1)
    for name, v in (("begin", begin), ("stride", stride)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"mcpc_errors: {name} must be an int, got {v!r}")
    if not 0 <= begin < T:
        raise ValueError(f"mcpc_errors: begin={begin} outside [0, T={T})")
    if stride < 1:
        raise ValueError(f"mcpc_errors: stride={stride}, must be at least 1")
    layers = spec.get("layers", ())
    if isinstance(layers, int) and not isinstance(layers, bool):
        layers = (layers,)
    try:
        layers = tuple(layers)
    except TypeError:
        raise ValueError(f"mcpc_errors: layers must be a sequence of layer indices, got {layers!r}") from None
    for l in layers:
        if isinstance(l, bool) or not isinstance(l, int) or not 0 <= l < n_layers:
            raise ValueError(f"mcpc_errors: layer index {l!r} out of range, the model has {n_layers} PC layers (0..{n_layers - 1})")
    layers = tuple(sorted(set(layers)))
    quantity = spec.get("quantity", "error")
    if quantity not in _QUANTITIES:
        raise ValueError(f"mcpc_errors: quantity={quantity!r}, expected 'error' or 'prediction'")
    outputs = spec.get("outputs", None)
    if outputs not in _OUTPUTS:
        raise ValueError(f"mcpc_errors: outputs={outputs!r}, expected None, 'error' or 'prediction'")
    if outputs is not None and n_out < 1:
        raise ValueError("mcpc_errors: outputs asked of a model without a read-out (it ends with a PCLayer)")
    if outputs == "error" and not has_loss:
        raise ValueError("mcpc_errors: outputs='error' asked of a call without a loss (the read-out has no error then)")
    covariance = spec.get("covariance", None)
    if covariance not in _COVARIANCES:
        raise ValueError(f"mcpc_errors: covariance={covariance!r}, expected None, 'chain' (one matrix per chain) or 'chains' (pooled)")
    if not layers and outputs is None:
        raise ValueError("mcpc_errors: no columns: layers is empty and outputs is None")
    columns, start = [], 0
    for l in layers:
        columns.append((block_name(quantity, l), start, int(sizes[l])))
        start += int(sizes[l])
    if outputs is not None:
        columns.append((block_name(outputs, None), start, int(n_out)))
        start += int(n_out)
    out = ErrorsSpec(begin=begin, stride=stride, layers=layers, quantity=quantity, outputs=outputs, variance=bool(spec.get("variance", True)),
                     covariance=covariance, T=T, columns=tuple(columns), reads=layers_read(layers, outputs is not None, n_layers))
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

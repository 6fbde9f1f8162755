"""Lagged autocovariances of a Langevin call: the request (``PCTrainer.mcpc_autocovariance``) and the result
(``PCTrainer.mcpc_last_autocovariance``).

The samples of one chain are strongly autocorrelated: SGD on x with injected noise moves a unit a little per step.  Every mean, variance
and histogram of a call therefore carries a Monte Carlo error that its n samples alone do not tell, and ``mixing``, ``T`` and ``lr`` are
chosen blind without it.  What an MCMC user reads next to the moments is the autocorrelation function, the integrated autocorrelation
time tau and the effective sample size n / tau.  Here the fused call adds, per (chain, unit) and lag k = 0..max_lag, the raw products
sum_j g_j g_{j-k} out of its record ring on the device (csrc/mcpc_acov.h: one thread per element, fp64, bitwise a sequential loop
however the call is sliced) and keeps the first and the last ``max_lag`` samples; the trajectory is never materialised.  This module
holds no device code: validation of the request, which steps are samples, and the fp64 arithmetic from the raw sums to the centred
estimator, Geyer's tau, ESS and the Monte Carlo standard error.

Cancellation.  The estimator is centred AFTERWARDS, from raw fp64 sums: c_k = (lagged_k - m ((sum - tail_k) + (sum - head_k)) +
(n - k) m^2) / n.  Each of the three terms is about n (c_0 + m^2) and is held to 2^-53 relative, so c_k loses about n 2^-53 (1 + m^2 / c_0)
relative to c_0.  A check on the host with n = 300 gave 2e-14 of c_0 at |m| = 3 sigma and 2e-9 at |m| = 1000 sigma: a unit whose mean is
many thousand standard deviations away from 0 wants its records shifted before they are reduced, which this module does not do.
"""
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch

from .sampling import (SampleWindow, column_list, human_bytes, parse_keys, parse_layers, parse_outputs, parse_window,  # noqa: F401
                       require_columns, sample_steps)

_KEYS = ("begin", "stride", "layers", "outputs", "max_lag")
_OUTPUTS = (None, "identity", "sigmoid")
MAX_LAG = 64                                     # include/mcpc.h: MCPC_ACOV_MAX_LAG


@dataclass(frozen=True, eq=False)
class AutocovarianceSpec(SampleWindow):
    """A validated ``mcpc_autocovariance`` request for a call of ``T`` steps."""
    layers: Tuple[int, ...]
    outputs: Optional[str]
    max_lag: int
    columns: Tuple[Tuple[str, int], ...]            # (name, width) of every block, in order: "x0", "x1", ..., "out"


def state_bytes(columns, B: int, max_lag: int) -> int:
    """Bytes of the state of a request (fp64 lagged and sum, fp32 window and head): what ``mcpc_autocovariance_max_bytes`` bounds."""
    return B * sum(w for _, w in columns) * (8 * (max_lag + 1) + 8 + 4 * max_lag + 4 * max_lag)


def validate_spec(spec, T: int, n_layers: int, n_out: int, sizes, B: int, max_bytes: int) -> AutocovarianceSpec:
    """``PCTrainer.mcpc_autocovariance`` -> AutocovarianceSpec, or ValueError: not a dict, unknown keys, ``begin`` outside [0, T),
    ``stride`` < 1, a layer index out of range, no column at all, ``outputs`` on a model without a read-out, no ``max_lag`` or one
    outside 0..64, a state larger than ``max_bytes``.  Defaults: begin=0, stride=1, layers=(), outputs=None."""
    parse_keys("mcpc_autocovariance", spec, _KEYS)
    begin, stride = parse_window("mcpc_autocovariance", spec, T)
    layers = parse_layers("mcpc_autocovariance", spec, n_layers, none_means="empty")
    outputs = parse_outputs("mcpc_autocovariance", spec, n_out, _OUTPUTS)
    require_columns("mcpc_autocovariance", layers, outputs)
    if "max_lag" not in spec or spec["max_lag"] is None:
        raise ValueError(f"mcpc_autocovariance: max_lag is required: the largest lag kept, an int in 0..{MAX_LAG}")
    max_lag = spec["max_lag"]
    if isinstance(max_lag, bool) or not isinstance(max_lag, int):
        raise ValueError(f"mcpc_autocovariance: max_lag must be an int, got {max_lag!r}")
    if not 0 <= max_lag <= MAX_LAG:
        raise ValueError(f"mcpc_autocovariance: max_lag={max_lag} outside 0..{MAX_LAG}")
    columns = column_list(layers, sizes, None if outputs is None else "out", n_out)
    need = state_bytes(columns, B, max_lag)
    if need > max_bytes:
        raise ValueError(f"mcpc_autocovariance: the state ({B} chains x {sum(w for _, w in columns)} units x {max_lag + 1} lags in fp64, "
                         f"and the first and last {max_lag} samples) takes {human_bytes(need)}, more than "
                         f"mcpc_autocovariance_max_bytes = {human_bytes(max_bytes)}: ask for fewer layers or fewer lags")
    return AutocovarianceSpec(begin=begin, stride=stride, layers=layers, outputs=outputs, max_lag=max_lag, T=T, columns=columns)


def geyer(rho: torch.Tensor, n: int):
    """Geyer's initial monotone positive sequence on autocorrelations ``rho`` ``[..., K + 1]`` of ``n`` samples -> ``(tau, truncated)``.
    P_m = rho_2m + rho_2m+1 for m < M = (K + 1) // 2; the sum stops at the first P_m <= 0; P'_m = min(P'_m-1, P_m);
    tau = -1 + 2 sum P'_m, floored at 1 / log10(n) (the cap ESS <= n log10 n).  ``truncated``: no P_m <= 0 appeared among the M pairs
    (none at all with K = 0): tau is then a lower bound.  NaN in ``rho`` counts as P_m <= 0; the caller decides what tau is there."""
    K1 = rho.shape[-1]
    M = K1 // 2
    if M == 0:
        return torch.full(rho.shape[:-1], float("nan"), dtype=torch.float64, device=rho.device), \
            torch.ones(rho.shape[:-1], dtype=torch.bool, device=rho.device)
    P = rho[..., 0:2 * M:2] + rho[..., 1:2 * M:2]                                    # [..., M]
    alive = torch.cumprod((P > 0).to(torch.int8), dim=-1).to(torch.bool)             # before the first P_m <= 0
    mono = torch.cummin(torch.where(alive, P, torch.zeros_like(P)), dim=-1).values
    tau = -1.0 + 2.0 * torch.where(alive, mono, torch.zeros_like(P)).sum(-1)
    if n > 1:
        tau = torch.clamp(tau, min=1.0 / math.log10(n))
    return tau, alive[..., -1]


@dataclass
class Autocovariance:
    """Lagged products of one fused call, on the model's device: ``n`` samples per chain of ``B`` chains, lags 0..``max_lag`` = K.  Per
    block name ("x0", "x1", ..., "out"; ``names`` keeps their order), with g the block's transform and s_0 .. s_n-1 its samples:
    ``lagged[name]`` fp64 ``[B, w, K + 1]``, the RAW sums of g(s_j) g(s_j-k) over j >= k; ``sum[name]`` fp64 ``[B, w]``;
    ``head[name]`` fp32 ``[K, B, w]``, the samples 0..K-1; ``tail[name]`` fp32 ``[K, B, w]``, ``tail[k]`` the sample k + 1 places from
    the end (both valid for k < min(K, n)).  Everything derived is fp64 torch, per (chain, unit)."""
    n: int
    B: int
    max_lag: int
    names: List[str] = field(default_factory=list)
    lagged: Dict[str, torch.Tensor] = field(default_factory=dict)
    sum: Dict[str, torch.Tensor] = field(default_factory=dict)
    head: Dict[str, torch.Tensor] = field(default_factory=dict)
    tail: Dict[str, torch.Tensor] = field(default_factory=dict)

    def _get(self, name):
        if name not in self.lagged:
            raise KeyError(f"no block {name!r}; this result has {list(self.names)}")
        return self.lagged[name]

    def mean(self, name: str) -> torch.Tensor:
        """The mean over the window, ``[B, w]``."""
        self._get(name)
        return self.sum[name] / self.n

    def _edge_sums(self, t):
        """fp32 ``[K, B, w]`` -> fp64 ``[B, w, K + 1]``: the sums of the first k rows, k = 0..K."""
        c = torch.cumsum(t.to(torch.float64), dim=0)
        return torch.cat([c.new_zeros((1,) + tuple(t.shape[1:])), c], dim=0).permute(1, 2, 0)

    def acov(self, name: str) -> torch.Tensor:
        """The biased autocovariance estimator centred on the window mean m, ``[B, w, K + 1]``:
        c_k = (1 / n) sum_{j < n - k} (g_j - m)(g_j+k - m), and 0 for k >= n."""
        lag = self._get(name)
        n, K = self.n, self.max_lag
        s = self.sum[name].unsqueeze(-1)
        m = s / n
        k = torch.arange(K + 1, dtype=torch.float64, device=lag.device)
        c = (lag - m * ((s - self._edge_sums(self.tail[name])) + (s - self._edge_sums(self.head[name]))) + (n - k) * (m * m)) / n
        return torch.where(k < n, c, torch.zeros_like(c))

    def acf(self, name: str) -> torch.Tensor:
        """The autocorrelation function c_k / c_0, ``[B, w, K + 1]``; NaN where c_0 == 0."""
        c = self.acov(name)
        c0 = c[..., :1]
        return torch.where(c0 == 0, torch.full_like(c, float("nan")), c / c0)

    def _geyer(self, name):
        rho = self.acf(name)
        tau, trunc = geyer(rho, self.n)
        bad = torch.isnan(rho[..., 0])
        if self.n < 4:
            bad = torch.ones_like(bad)
        return torch.where(bad, torch.full_like(tau, float("nan")), tau), trunc & ~bad

    def tau(self, name: str) -> torch.Tensor:
        """The integrated autocorrelation time by Geyer's initial monotone positive sequence (``geyer``), ``[B, w]``; NaN for n < 4 or
        c_0 == 0.  Where ``truncated`` it is a lower bound."""
        return self._geyer(name)[0]

    def truncated(self, name: str) -> torch.Tensor:
        """bool ``[B, w]``: no pair P_m <= 0 appeared within ``max_lag``, so tau is a lower bound: ask for more lags."""
        return self._geyer(name)[1]

    def ess(self, name: str) -> torch.Tensor:
        """The effective sample size n / tau, ``[B, w]`` (at most n log10 n)."""
        return self.n / self.tau(name)

    def mcse(self, name: str) -> torch.Tensor:
        """The Monte Carlo standard error of the mean, sqrt(c_0 tau / n), ``[B, w]``."""
        return torch.sqrt(self.acov(name)[..., 0] * self.tau(name) / self.n)

    @staticmethod
    def cat(parts) -> "Autocovariance":
        """The results of different batches (same request, same n) joined along the chains."""
        parts = list(parts)
        first = parts[0]
        if any((p.n, p.max_lag, list(p.names)) != (first.n, first.max_lag, list(first.names)) for p in parts):
            raise ValueError("Autocovariance.cat: the results are of different requests")

        def join(f, dim):
            return {k: torch.cat([getattr(p, f)[k] for p in parts], dim=dim) for k in first.names}
        return Autocovariance(n=first.n, B=sum(p.B for p in parts), max_lag=first.max_lag, names=list(first.names),
                              lagged=join("lagged", 0), sum=join("sum", 0), head=join("head", 1), tail=join("tail", 1))


def from_state(spec: AutocovarianceSpec, B: int, state, device) -> Autocovariance:
    """The kernel's state per block (dicts with lagged, sum, window, head) -> Autocovariance on ``device``."""
    a = Autocovariance(n=spec.n, B=B, max_lag=spec.max_lag, names=[nm for nm, _ in spec.columns])
    for (nm, _), st in zip(spec.columns, state):
        a.lagged[nm], a.sum[nm] = st["lagged"].to(device), st["sum"].to(device)
        a.head[nm], a.tail[nm] = st["head"].to(device), st["window"].to(device)
    return a

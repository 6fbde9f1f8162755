"""Posterior histograms of a Langevin call: the request (``PCTrainer.mcpc_histogram``) and the result
(``PCTrainer.mcpc_last_histogram``).

The reference looks at an MCPC call through the marginal distribution of a unit over the sampling window: ``plt.hist(...,
bins=np.linspace(lo, hi, k), density=True)`` on recorded trajectories (figure_2.py, figure_3.py, figure_4.py, figure_6.py).  Two moments
do not describe a posterior behind a ReLU or a Bernoulli read-out; counts do, and quantiles, credible intervals and densities follow from
them.  Here the fused call bins its record ring on the device (csrc/mcpc_hist.h: integer counters in LDS, a bin decided by fp32
comparison against the edges alone) and the trajectory is never materialised.  This module holds no device code: validation of the
request, which steps are samples, the edges, and the fp64 arithmetic from counts to density, cdf and quantiles.

The range is never taken from the data: a streaming pass cannot know the extremes.  Values outside the edges are counted in ``under`` and
``over``, NaNs in ``nan``, so that per (chain, unit) bins + under + over + nan = n (n x B when pooled).
"""
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .sampling import (SampleWindow, column_list, human_bytes, parse_keys, parse_layers, parse_outputs, parse_window,  # noqa: F401
                       require_columns, sample_steps)

_KEYS = ("begin", "stride", "layers", "outputs", "bins", "range", "pool")
_OUTPUTS = (None, "identity", "sigmoid")
_POOLS = (None, "chains")
MAX_BINS = 256                                   # include/mcpc.h: MCPC_HIST_MAX_BINS


@dataclass(frozen=True, eq=False)
class HistogramSpec(SampleWindow):
    """A validated ``mcpc_histogram`` request for a call of ``T`` steps."""
    layers: Tuple[int, ...]
    outputs: Optional[str]
    pooled: bool
    columns: Tuple[Tuple[str, int], ...]            # (name, width) of every block, in order: "x0", "x1", ..., "out"
    edges: Tuple[np.ndarray, ...]                   # per block: the fp32 edges, [n_bins + 1]


def result_bytes(columns, edges, B: int, pooled: bool) -> int:
    """Bytes of the int64 counts of a request (bins, under, over, nan): what ``mcpc_histogram_max_bytes`` bounds."""
    return 8 * sum(w * (len(e) + 2) for (_, w), e in zip(columns, edges)) * (1 if pooled else B)


def _edges(name, bins, rng, who="mcpc_histogram", max_bins=MAX_BINS):
    """The fp32 edges of block ``name``: ``bins`` an int with ``rng = (lo, hi)``, or a sequence of edges.  ``who`` opens the messages and
    ``max_bins`` bounds the bins (``mcpc_histogram2d`` parses each axis here too)."""
    if isinstance(bins, bool):
        raise ValueError(f"{who}: bins of {name!r} must be an int or a sequence of edges, got {bins!r}")
    if isinstance(bins, (int, np.integer)):
        if not 1 <= bins <= max_bins:
            raise ValueError(f"{who}: bins={bins} of {name!r}, must be 1..{max_bins}")
        if rng is None:
            raise ValueError(f"{who}: bins={bins} of {name!r} needs range=(lo, hi): the range is never taken from the data (a "
                             "streaming pass cannot know the extremes)")
        try:
            lo, hi = (float(v) for v in rng)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: range of {name!r} must be (lo, hi), got {rng!r}") from None
        if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
            raise ValueError(f"{who}: range of {name!r} must be finite with lo < hi, got {(lo, hi)!r}")
        e64 = np.linspace(lo, hi, int(bins) + 1)
    else:
        try:
            e64 = np.asarray(bins, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: bins of {name!r} must be an int or a sequence of edges, got {bins!r}") from None
        if e64.ndim != 1 or not 2 <= e64.size <= max_bins + 1:
            raise ValueError(f"{who}: edges of {name!r}: expected a 1-D sequence of 2..{max_bins + 1} values, got shape "
                             f"{e64.shape}")
    with np.errstate(over="ignore"):
        e32 = e64.astype(np.float32)
    if not np.isfinite(e32).all():
        raise ValueError(f"{who}: edges of {name!r} are not finite in fp32")
    if not (np.diff(e32) > 0).all():
        raise ValueError(f"{who}: edges of {name!r} are not strictly ascending in fp32 (they are rounded to fp32: the fp32 "
                         "edges are the edges)")
    return e32


def validate_spec(spec, T: int, n_layers: int, n_out: int, sizes, B: int, max_bytes: int) -> HistogramSpec:
    """``PCTrainer.mcpc_histogram`` -> HistogramSpec, or ValueError: not a dict, unknown keys, ``begin`` outside [0, T), ``stride`` < 1,
    a layer index out of range, no column at all, ``outputs`` on a model without a read-out, an unknown ``pool``, no ``bins``, an int
    ``bins`` without ``range``, edges that are not finite and strictly ascending in fp32, a result larger than ``max_bytes``.
    Defaults: begin=0, stride=1, layers=(), outputs=None, pool=None (one histogram per chain and unit).  ``bins`` and ``range`` may be
    dicts keyed by block name ("x0", ..., "out")."""
    parse_keys("mcpc_histogram", spec, _KEYS)
    begin, stride = parse_window("mcpc_histogram", spec, T)
    layers = parse_layers("mcpc_histogram", spec, n_layers, none_means="empty")
    outputs = parse_outputs("mcpc_histogram", spec, n_out, _OUTPUTS)
    pool = spec.get("pool", None)
    if pool not in _POOLS:
        raise ValueError(f"mcpc_histogram: pool={pool!r}, expected None (one histogram per chain) or 'chains'")
    require_columns("mcpc_histogram", layers, outputs)
    columns = column_list(layers, sizes, None if outputs is None else "out", n_out)
    if "bins" not in spec or spec["bins"] is None:
        raise ValueError("mcpc_histogram: bins is required: an int with range=(lo, hi), or a sequence of edges (either may be a dict "
                         "keyed by block name)")
    bins, rng = spec["bins"], spec.get("range", None)
    names = [nm for nm, _ in columns]
    for what, v in (("bins", bins), ("range", rng)):
        if isinstance(v, dict):
            stray = sorted(k for k in v if k not in names)
            if stray:
                raise ValueError(f"mcpc_histogram: {what} names blocks {stray} that the request does not have; it has {names}")
    edges = []
    for nm in names:
        b = bins
        if isinstance(bins, dict):
            if nm not in bins:
                raise ValueError(f"mcpc_histogram: bins has no entry for block {nm!r}; the request has {names}")
            b = bins[nm]
        r = rng.get(nm) if isinstance(rng, dict) else rng
        edges.append(_edges(nm, b, r))
    pooled = pool == "chains"
    need = result_bytes(columns, edges, B, pooled)
    if need > max_bytes:
        cols = sum(w for _, w in columns)
        what = f"{cols} units" if pooled else f"{B} chains x {cols} units"
        raise ValueError(f"mcpc_histogram: the result ({what} x up to {max(len(e) for e in edges) + 2} int64 counters) takes "
                         f"{human_bytes(need)}, more than mcpc_histogram_max_bytes = {human_bytes(max_bytes)}: ask for fewer layers"
                         " or fewer bins" + ("" if pooled else " or pool='chains'"))
    return HistogramSpec(begin=begin, stride=stride, layers=layers, outputs=outputs, pooled=pooled, T=T, columns=columns,
                         edges=tuple(edges))


@dataclass
class Histogram:
    """Histograms of one fused call, on the model's device.  ``n`` samples per chain of ``B`` chains.  Per block name ("x0", "x1", ...,
    "out"; ``names`` keeps their order): ``edges[name]`` fp32 ``[nb + 1]``, ``counts[name]`` int64 ``[B, w, nb]`` (``[w, nb]`` pooled
    over the chains), ``under[name]`` / ``over[name]`` / ``nan[name]`` int64 ``[B, w]`` (``[w]``).  Bins are half-open, the last one
    closed, as ``np.histogram`` with explicit edges.  Per (chain, unit): bins + under + over + nan = n (n x B pooled).  The results of
    several calls merge by adding counts and ``n`` (``merge``)."""
    n: int
    B: int
    pooled: bool
    names: List[str] = field(default_factory=list)
    edges: Dict[str, torch.Tensor] = field(default_factory=dict)
    counts: Dict[str, torch.Tensor] = field(default_factory=dict)
    under: Dict[str, torch.Tensor] = field(default_factory=dict)
    over: Dict[str, torch.Tensor] = field(default_factory=dict)
    nan: Dict[str, torch.Tensor] = field(default_factory=dict)

    @property
    def N(self) -> int:
        """Samples behind one histogram."""
        return self.n * self.B if self.pooled else self.n

    def _get(self, name):
        if name not in self.counts:
            raise KeyError(f"no block {name!r}; this result has {list(self.names)}")
        return self.counts[name], self.edges[name].to(torch.float64)

    def density(self, name: str) -> torch.Tensor:
        """counts / bin width / in-range total in fp64: numpy's ``density=True`` (NaN where nothing is in range)."""
        c, e = self._get(name)
        c = c.to(torch.float64)
        return c / (e[1:] - e[:-1]) / c.sum(-1, keepdim=True)

    def cdf(self, name: str) -> torch.Tensor:
        """The share of the in-range mass at or below the right edge of every bin, fp64 ``[..., nb]`` (NaN where nothing is in range)."""
        c, _ = self._get(name)
        return torch.cumsum(c, -1).to(torch.float64) / c.sum(-1, keepdim=True).to(torch.float64)

    def quantile(self, name: str, q) -> torch.Tensor:
        """The value below which the share ``q`` of the in-range mass lies, linear inside the bin that crosses it; fp64, ``[...]`` for a
        scalar ``q`` and ``[..., len(q)]`` for a sequence.  NaN where nothing is in range."""
        c, e = self._get(name)
        scalar = not isinstance(q, (list, tuple, np.ndarray, torch.Tensor))
        qs = torch.as_tensor([q] if scalar else q, dtype=torch.float64, device=c.device).reshape(-1)
        if bool(((qs < 0) | (qs > 1)).any()):
            raise ValueError(f"quantile: q must lie in [0, 1], got {q!r}")
        cum = torch.cumsum(c, -1).to(torch.float64)                                  # [..., nb]
        total = cum[..., -1:]
        out = []
        for qv in qs:
            target = qv * total                                                      # [..., 1]
            hit = (cum >= target) & (c > 0)
            idx = torch.argmax(hit.to(torch.int8), dim=-1, keepdim=True)             # the first bin that crosses it
            cnt = torch.gather(c, -1, idx).to(torch.float64)
            below = torch.gather(cum, -1, idx) - cnt
            lo, hi = e[:-1][idx], e[1:][idx]
            v = lo + (target - below) / cnt * (hi - lo)
            out.append(torch.where(total > 0, v, torch.full_like(v, float("nan"))).squeeze(-1))
        return out[0] if scalar else torch.stack(out, dim=-1)

    def pool(self) -> "Histogram":
        """The histograms summed over the chains: what ``pool="chains"`` gives."""
        if self.pooled:
            return self

        def s(d):
            return {k: v.sum(dim=0) for k, v in d.items()}
        return Histogram(n=self.n, B=self.B, pooled=True, names=list(self.names), edges=dict(self.edges), counts=s(self.counts),
                         under=s(self.under), over=s(self.over), nan=s(self.nan))

    def merge(self, other: "Histogram") -> "Histogram":
        """The counts of both calls' samples together (same chains, same request)."""
        same = (self.B, self.pooled, list(self.names)) == (other.B, other.pooled, list(other.names)) and all(
            self.counts[k].shape == other.counts[k].shape and torch.equal(self.edges[k], other.edges[k].to(self.edges[k].device))
            for k in self.names)
        if not same:
            raise ValueError("Histogram.merge: the two results are of different requests")

        def add(a, b):
            return {k: a[k] + b[k] for k in self.names}
        return Histogram(n=self.n + other.n, B=self.B, pooled=self.pooled, names=list(self.names), edges=dict(self.edges),
                         counts=add(self.counts, other.counts), under=add(self.under, other.under), over=add(self.over, other.over),
                         nan=add(self.nan, other.nan))

    def total(self, name: str) -> torch.Tensor:
        """bins + under + over + nan per (chain, unit): ``N`` everywhere."""
        return self.counts[name].sum(-1) + self.under[name] + self.over[name] + self.nan[name]


def from_counts(spec: HistogramSpec, B: int, raw, device) -> Histogram:
    """The kernel's tables (per block int64 ``[..., nb + 3]``: bins, under, over, nan) -> Histogram on ``device``."""
    h = Histogram(n=spec.n, B=B, pooled=spec.pooled, names=[nm for nm, _ in spec.columns])
    for (nm, _), e, t in zip(spec.columns, spec.edges, raw):
        t = t.to(device)
        nb = len(e) - 1
        h.edges[nm] = torch.from_numpy(e.copy()).to(device)
        h.counts[nm] = t[..., :nb].contiguous()
        h.under[nm], h.over[nm], h.nan[nm] = t[..., nb].contiguous(), t[..., nb + 1].contiguous(), t[..., nb + 2].contiguous()
    return h

"""Joint histograms of a Langevin call: the request (``PCTrainer.mcpc_histogram2d``) and the result (``PCTrainer.mcpc_last_histogram2d``).

The flagship panels of the reference's ``figure_2.py`` (2c and 2d, ``posterior_non_linear_model``) show the density of the softmax of a
linear classifier on ``x_0``, projected onto the plane of the class polygon (``proba_to_coordinate``) and binned in 2-D: whether the
posterior of a masked digit has two modes is a property of a joint density, which neither a sum nor a marginal shows.  The same holds
for any two latent units, within a layer or across layers.  Here the fused call counts the pairs on the device out of its record ring
(csrc/mcpc_hist2d.h: integer counters in LDS, each axis decided by fp32 comparison against its edges alone, as ``mcpc_histogram``
decides it) and the trajectory is never materialised.  A request takes one of two forms: pairs of latent units, or the plane of a
probe, whose coordinates are two derived records (``engine.probe_records`` twice: the class probabilities, then their projection).
This module holds no device code: validation of the request, which steps are samples, the edges, and the arithmetic on the counts.
"""
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import probe as _probe
from .histogram import _edges
from .sampling import SampleWindow, check_layer_index, human_bytes, parse_keys, parse_window, sample_steps  # noqa: F401

_KEYS = ("begin", "stride", "x", "y", "probe", "project", "bins", "range", "pool")
_PROBE_KEYS = ("layer", "weight", "bias", "linear", "link")
_POOLS = (None, "chains")
MAX_BINS = 128                                   # include/mcpc.h: MCPC_HIST2D_MAX_BINS, per axis
MAX_CELLS = 12288                                # include/mcpc.h: MCPC_HIST2D_MAX_CELLS, (nx + 3) * (ny + 3)
_NAME = "mcpc_histogram2d"


def polygon(C: int) -> np.ndarray:
    """The regular C-gon of the reference's ``proba_to_coordinate``: ``P[0][i] = cos(2 pi i / C)``, ``P[1][i] = sin(2 pi i / C)``,
    formed in fp64 and rounded to fp32, ``[2, C]``."""
    a = 2.0 * np.pi * np.arange(C, dtype=np.float64) / C
    return np.stack([np.cos(a), np.sin(a)]).astype(np.float32)


@dataclass(frozen=True, eq=False)
class Histogram2DSpec(SampleWindow):
    """A validated ``mcpc_histogram2d`` request for a call of ``T`` steps.  Units form: ``probe`` is None, pair k is unit ``pairs[k][0]``
    of layer ``x_layer`` against unit ``pairs[k][1]`` of layer ``y_layer``.  Probe form: ``probe`` is the validated read-out,
    ``project`` the fp32 ``[2, C]`` plane, and the one pair is the plane's two coordinates."""
    layers: Tuple[int, ...]                          # the layers the request reads
    x_layer: Optional[int]
    y_layer: Optional[int]
    pairs: Tuple[Tuple[int, int], ...]
    probe: Optional[_probe.ProbeSpec]
    project: Optional[np.ndarray]
    pooled: bool
    edges_x: np.ndarray
    edges_y: np.ndarray

    def max_samples(self, n_steps: int) -> int:
        """The most samples a slice of n_steps steps can hold (a derived record buffer of the probe form has that many rows)."""
        return min(self.n, -(-n_steps // self.stride))


def result_bytes(n_pairs: int, nx: int, ny: int, B: int, pooled: bool) -> int:
    """Bytes of the int64 counts of a request: what ``mcpc_histogram2d_max_bytes`` bounds."""
    return 8 * n_pairs * (nx + 3) * (ny + 3) * (1 if pooled else B)


def _units(axis, v, n_layers, sizes):
    try:
        layer, units = v
        units = (units,) if isinstance(units, int) and not isinstance(units, bool) else tuple(units)
    except (TypeError, ValueError):
        raise ValueError(f"{_NAME}: {axis} must be (layer, (unit, ...)), got {v!r}") from None
    check_layer_index(_NAME, layer, n_layers)
    for u in units:
        if isinstance(u, bool) or not isinstance(u, (int, np.integer)) or not 0 <= u < sizes[layer]:
            raise ValueError(f"{_NAME}: unit {u!r} of {axis} out of range, layer {layer} has {int(sizes[layer])} units")
    return layer, tuple(int(u) for u in units)


def _per_axis(what, v):
    """``bins`` or ``range`` -> (of x, of y)."""
    if what == "bins":
        if isinstance(v, (int, np.integer)) and not isinstance(v, bool):
            return v, v
        try:
            a, b = v
        except (TypeError, ValueError):
            raise ValueError(f"{_NAME}: bins must be an int, (nx, ny) or (edges_x, edges_y), got {v!r}") from None
        return a, b
    if v is None:
        return None, None
    try:
        a, b = v
    except (TypeError, ValueError):
        raise ValueError(f"{_NAME}: range must be (lo, hi) or ((lo, hi), (lo, hi)), got {v!r}") from None
    if isinstance(a, (int, float, np.integer, np.floating)):
        return (a, b), (a, b)
    return a, b


def validate_spec(spec, T: int, n_layers: int, n_out: int, sizes, B: int, max_bytes: int) -> Histogram2DSpec:
    """``PCTrainer.mcpc_histogram2d`` -> Histogram2DSpec, or ValueError: not a dict, unknown keys, ``begin`` outside [0, T), ``stride``
    < 1, both or neither of the two forms (``x=`` with ``y=``, or ``probe=``), unit lists of unequal length, a unit or layer out of
    range, a probe ``mcpc_probe`` would refuse, ``project`` that is not a finite ``[2, C]``, no ``bins``, an int ``bins`` without
    ``range``, edges that are not finite and strictly ascending in fp32, more than 128 bins on an axis or ``(nx + 3) * (ny + 3)`` over
    12288 cells, an unknown ``pool``, a result larger than ``max_bytes``.  Defaults: begin=0, stride=1, project=None (the class
    polygon), pool=None (one grid per chain and pair)."""
    parse_keys(_NAME, spec, _KEYS)
    begin, stride = parse_window(_NAME, spec, T)
    x, y, pr = spec.get("x"), spec.get("y"), spec.get("probe")
    if pr is not None and (x is not None or y is not None):
        raise ValueError(f"{_NAME}: both forms are given (x= / y= and probe=); pass exactly one of them")
    if pr is None and (x is None or y is None):
        raise ValueError(f"{_NAME}: neither form is complete: pass x= and y= (pairs of latent units), or probe= (the plane of a probe)")
    project = spec.get("project")
    probe_spec, x_layer, y_layer = None, None, None
    if pr is None:
        if project is not None:
            raise ValueError(f"{_NAME}: project belongs to the probe form, and x= / y= are given")
        x_layer, ux = _units("x", x, n_layers, sizes)
        y_layer, uy = _units("y", y, n_layers, sizes)
        if len(ux) != len(uy) or not ux:
            raise ValueError(f"{_NAME}: x names {len(ux)} units and y {len(uy)}: the lists pair up, so they are of equal length, at "
                             "least 1")
        pairs = tuple(zip(ux, uy))
        layers = tuple(sorted({x_layer, y_layer}))
    else:
        parse_keys(f"{_NAME}: probe", pr, _PROBE_KEYS)
        try:
            probe_spec = _probe.validate_spec(dict(pr, begin=begin, stride=stride), T, n_layers, sizes, B)
        except ValueError as exc:                    # mcpc_probe's own checks, told as this request's
            raise ValueError(f"{_NAME}: probe: " + str(exc).partition(": ")[2]) from None
        C = probe_spec.C
        if project is None:
            project = polygon(C)
        else:
            try:
                project = np.array(project.detach().cpu() if isinstance(project, torch.Tensor) else project, dtype=np.float32)
            except (TypeError, ValueError):
                raise ValueError(f"{_NAME}: project must be a [2, {C}] array, got {type(project).__name__}") from None
            if project.shape != (2, C):
                raise ValueError(f"{_NAME}: project has shape {project.shape}, expected (2, {C}): two coordinates per class")
            if not np.isfinite(project).all():
                raise ValueError(f"{_NAME}: project is not finite in fp32")
        pairs = ((0, 1),)
        layers = (probe_spec.layer,)
    pool = spec.get("pool", None)
    if pool not in _POOLS:
        raise ValueError(f"{_NAME}: pool={pool!r}, expected None (one grid per chain) or 'chains'")
    if "bins" not in spec or spec["bins"] is None:
        raise ValueError(f"{_NAME}: bins is required: an int or (nx, ny) with range=, or (edges_x, edges_y)")
    bx, by = _per_axis("bins", spec["bins"])
    rx, ry = _per_axis("range", spec.get("range", None))
    edges_x = _edges("x", bx, rx, who=_NAME, max_bins=MAX_BINS)
    edges_y = _edges("y", by, ry, who=_NAME, max_bins=MAX_BINS)
    nx, ny = len(edges_x) - 1, len(edges_y) - 1
    if (nx + 3) * (ny + 3) > MAX_CELLS:
        raise ValueError(f"{_NAME}: {nx} x {ny} bins are ({nx} + 3) * ({ny} + 3) = {(nx + 3) * (ny + 3)} cells with the side rows and "
                         f"columns, more than {MAX_CELLS}: ask for fewer bins")
    pooled = pool == "chains"
    need = result_bytes(len(pairs), nx, ny, B, pooled)
    if need > max_bytes:
        what = f"{len(pairs)} pairs" if pooled else f"{B} chains x {len(pairs)} pairs"
        raise ValueError(f"{_NAME}: the result ({what} x {nx + 3} x {ny + 3} int64 counters) takes {human_bytes(need)}, more than "
                         f"mcpc_histogram2d_max_bytes = {human_bytes(max_bytes)}: ask for fewer pairs or fewer bins"
                         + ("" if pooled else " or pool='chains'"))
    return Histogram2DSpec(begin=begin, stride=stride, T=T, layers=layers, x_layer=x_layer, y_layer=y_layer, pairs=pairs,
                           probe=probe_spec, project=project, pooled=pooled, edges_x=edges_x, edges_y=edges_y)


@dataclass
class Histogram2D:
    """Joint histograms of one fused call, on the model's device: ``n`` samples per chain of ``B`` chains, ``pairs`` the pairs counted
    (units form: (unit of x, unit of y); probe form: ``[(0, 1)]``, the plane's coordinates).  ``full`` is int64
    ``[B, pairs, nx + 3, ny + 3]`` (``[pairs, nx + 3, ny + 3]`` pooled over the chains): the row index the class of x, the column index
    that of y, the bins then under, over, nan.  Bins are half-open, the last one closed.  Every grid sums to ``N``."""
    n: int
    B: int
    pooled: bool
    pairs: List[Tuple[int, int]]
    edges_x: torch.Tensor
    edges_y: torch.Tensor
    full: torch.Tensor

    @property
    def N(self) -> int:
        """Samples behind one grid."""
        return self.n * self.B if self.pooled else self.n

    @property
    def nx(self) -> int:
        return int(self.edges_x.numel()) - 1

    @property
    def ny(self) -> int:
        return int(self.edges_y.numel()) - 1

    @property
    def counts(self) -> torch.Tensor:
        """The bins alone, int64 ``[..., pairs, nx, ny]``."""
        return self.full[..., :self.nx, :self.ny]

    @property
    def nan(self) -> torch.Tensor:
        """Per grid the samples with a NaN on either axis, int64 ``[..., pairs]``."""
        f, nx, ny = self.full, self.nx, self.ny
        return f[..., nx + 2, :].sum(-1) + f[..., :, ny + 2].sum(-1) - f[..., nx + 2, ny + 2]

    @property
    def outside(self) -> torch.Tensor:
        """Per grid the samples without a NaN that lie under or over the edges on either axis, int64 ``[..., pairs]``."""
        return self.full.sum((-2, -1)) - self.counts.sum((-2, -1)) - self.nan

    def total(self) -> torch.Tensor:
        """Every cell of a grid added up: ``N`` everywhere."""
        return self.full.sum((-2, -1))

    def density(self) -> torch.Tensor:
        """counts / bin area / in-range total in fp64: ``np.histogram2d(density=True)`` over the in-range samples (NaN where nothing is
        in range)."""
        c = self.counts.to(torch.float64)
        ex, ey = self.edges_x.to(torch.float64), self.edges_y.to(torch.float64)
        area = (ex[1:] - ex[:-1])[:, None] * (ey[1:] - ey[:-1])[None, :]
        return c / area / c.sum((-2, -1), keepdim=True)

    def marginal(self, axis: str, sides: bool = False) -> torch.Tensor:
        """The counts of one axis, whatever the other holds: int64 ``[..., pairs, nx]`` for "x" (``ny`` for "y"); with ``sides`` the
        columns under, over, nan follow, and the table is what ``mcpc_histogram`` counts for that unit with the same edges."""
        if axis not in ("x", "y"):
            raise ValueError(f"marginal: axis must be 'x' or 'y', got {axis!r}")
        m = self.full.sum(-1) if axis == "x" else self.full.sum(-2)
        return m if sides else m[..., :(self.nx if axis == "x" else self.ny)]

    def pool(self) -> "Histogram2D":
        """The grids summed over the chains: what ``pool="chains"`` gives."""
        if self.pooled:
            return self
        return Histogram2D(n=self.n, B=self.B, pooled=True, pairs=list(self.pairs), edges_x=self.edges_x, edges_y=self.edges_y,
                           full=self.full.sum(dim=0))

    def _same_request(self, other, what):
        dev = self.edges_x.device
        if not (self.pooled == other.pooled and list(self.pairs) == list(other.pairs)
                and torch.equal(self.edges_x, other.edges_x.to(dev)) and torch.equal(self.edges_y, other.edges_y.to(dev))):
            raise ValueError(f"Histogram2D.{what}: the results are of different requests")

    def merge(self, other: "Histogram2D") -> "Histogram2D":
        """The counts of both calls' samples together (same chains, same edges and pairs)."""
        self._same_request(other, "merge")
        if self.B != other.B:
            raise ValueError("Histogram2D.merge: the results are of different chains")
        return Histogram2D(n=self.n + other.n, B=self.B, pooled=self.pooled, pairs=list(self.pairs), edges_x=self.edges_x,
                           edges_y=self.edges_y, full=self.full + other.full.to(self.full.device))

    @staticmethod
    def cat(parts) -> "Histogram2D":
        """The per-chain results of different batches (same request, same n) joined along the chains."""
        parts = list(parts)
        first = parts[0]
        for p in parts[1:]:
            first._same_request(p, "cat")
        if first.pooled or any(p.n != first.n for p in parts):
            raise ValueError("Histogram2D.cat: per-chain results of equally many samples join along the chains; pooled ones merge")
        return Histogram2D(n=first.n, B=sum(p.B for p in parts), pooled=False, pairs=list(first.pairs), edges_x=first.edges_x,
                           edges_y=first.edges_y, full=torch.cat([p.full for p in parts], dim=0))

    def cpu(self) -> "Histogram2D":
        return Histogram2D(n=self.n, B=self.B, pooled=self.pooled, pairs=list(self.pairs), edges_x=self.edges_x.cpu(),
                           edges_y=self.edges_y.cpu(), full=self.full.cpu())


def from_counts(spec: Histogram2DSpec, B: int, full: torch.Tensor, device) -> Histogram2D:
    """The kernel's table -> Histogram2D on ``device``."""
    return Histogram2D(n=spec.n, B=B, pooled=spec.pooled, pairs=list(spec.pairs), edges_x=torch.from_numpy(spec.edges_x.copy()).to(device),
                       edges_y=torch.from_numpy(spec.edges_y.copy()).to(device), full=full.to(device))

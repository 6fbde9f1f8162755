"""Sample clouds of a Langevin call and the nearest-neighbour KL divergence between two of them: the request (``PCTrainer.mcpc_cloud``),
the result (``PCTrainer.mcpc_last_cloud``) and the estimator.

The six reducers answer "what is the distribution of one call"; the reference's ``figure_5.py`` asks how far apart the distributions of
two calls are: it records 10 000 steps of every latent layer on the host, keeps 5 units of one layer, thins the rows by 20 "to prevent
memory overload" and estimates D(prior || posterior) with ``KLdivergence`` (``utils/training_evaluation.py``), the Perez-Cruz estimator
on two scipy KD-trees.  Here the fused call gathers the chosen units of the layer out of its record ring into one device tensor (a
cloud of 9 500 x 256 rows x 5 floats is 48.6 MB), and the estimator's hot path -- for every row of x the k smallest distances into y
-- is brute force on the device (csrc/mcpc_knn.h), exact, unthinned if the caller so wishes.  This module holds no device code:
validation of the request, which steps are samples, the row order of a cloud, streaming the reference set, and the fp64 arithmetic
from distances to the estimate.
"""
from dataclasses import dataclass
from typing import Optional, Tuple

import math

import torch

from . import _lib as L
from .sampling import SampleWindow, human_bytes, parse_keys, parse_layer, parse_window, sample_steps  # noqa: F401

_KEYS = ("begin", "stride", "layer", "units")
MAX_UNITS = 32                                   # include/mcpc.h: MCPC_KNN_MAX_DIM
KNN_CHUNK_BYTES = 256 << 20                      # reference rows handed to one knn_accumulate call by knn_sqdist


@dataclass(frozen=True)
class CloudSpec(SampleWindow):
    """A validated ``mcpc_cloud`` request for a call of ``T`` steps."""
    layer: int
    units: Tuple[int, ...]

    @property
    def d(self) -> int:
        return len(self.units)


def validate_spec(spec, T: int, n_layers: int, sizes, B: int, max_bytes: int) -> CloudSpec:
    """``PCTrainer.mcpc_cloud`` -> CloudSpec, or ValueError: not a dict, unknown keys, ``begin`` outside [0, T), ``stride`` < 1, no
    ``layer`` or one out of range, ``units`` that are not 1..32 distinct ints inside the layer (None = every unit, an error on a layer
    wider than 32), a cloud of more than ``max_bytes``.  Defaults: begin=0, stride=1, units=None."""
    parse_keys("mcpc_cloud", spec, _KEYS)
    begin, stride = parse_window("mcpc_cloud", spec, T)
    layer = parse_layer("mcpc_cloud", spec, n_layers, "the cloud is taken from")
    width = int(sizes[layer])
    units = spec.get("units", None)
    if units is None:
        if width > MAX_UNITS:
            raise ValueError(f"mcpc_cloud: units=None asks for every unit of layer {layer}, which is {width} wide; a cloud holds at most "
                             f"{MAX_UNITS} units: name them")
        units = tuple(range(width))
    if isinstance(units, int) and not isinstance(units, bool):
        units = (units,)
    try:
        units = tuple(units)
    except TypeError:
        raise ValueError(f"mcpc_cloud: units must be a sequence of unit indices, got {units!r}") from None
    if not 1 <= len(units) <= MAX_UNITS:
        raise ValueError(f"mcpc_cloud: {len(units)} units, expected 1..{MAX_UNITS}")
    for u in units:
        if isinstance(u, bool) or not isinstance(u, int) or not 0 <= u < width:
            raise ValueError(f"mcpc_cloud: unit index {u!r} out of range, layer {layer} has {width} units (0..{width - 1})")
    if len(set(units)) != len(units):
        raise ValueError(f"mcpc_cloud: units {list(units)} are not distinct")
    out = CloudSpec(begin=begin, stride=stride, layer=layer, units=units, T=T)
    need = 4 * out.n * B * out.d
    if need > max_bytes:
        raise ValueError(f"mcpc_cloud: the cloud ({out.n} samples x {B} chains x {out.d} units fp32) takes {human_bytes(need)}, more than "
                         f"mcpc_cloud_max_bytes = {human_bytes(max_bytes)}: ask for a larger stride, a later begin or fewer units")
    return out


@dataclass
class Cloud:
    """The samples of chosen units of one layer over one fused call.  ``points``: fp32 ``[n, B, d]`` (sample, chain, unit), kept ON THE
    ENGINE'S DEVICE even when the model was built on the CPU (a staged model): its consumers are device kernels (``knn_sqdist``,
    ``kl_divergence``), and a copy to the host and back is what this module exists to avoid; ``.cpu()`` gives a host copy.  ``units``:
    the unit indices of the columns, ``layer``: the PC layer."""
    points: torch.Tensor
    units: Tuple[int, ...]
    layer: int

    @property
    def n(self) -> int:
        return int(self.points.shape[0])

    @property
    def B(self) -> int:
        return int(self.points.shape[1])

    @property
    def d(self) -> int:
        return int(self.points.shape[2])

    def flat(self) -> torch.Tensor:
        """``[n * B, d]``, step-major then chain: the row order of the reference's ``torch.concatenate([r[layer] for r in xs[mixing:]])``
        (a view)."""
        return self.points.reshape(self.n * self.B, self.d)

    def thin(self, indent: int) -> torch.Tensor:
        """``flat()[::indent]``: the reference's thinning of the rows."""
        return self.flat()[::int(indent)]

    def cpu(self) -> "Cloud":
        return Cloud(points=self.points.cpu(), units=self.units, layer=self.layer)

    @staticmethod
    def cat(parts) -> "Cloud":
        """The clouds of different batches (same request, same n) joined along the chains, in the order given."""
        parts = list(parts)
        first = parts[0]
        if any((p.n, tuple(p.units), p.layer) != (first.n, tuple(first.units), first.layer) for p in parts):
            raise ValueError("Cloud.cat: the clouds are of different requests")
        return Cloud(points=torch.cat([p.points for p in parts], dim=1), units=first.units, layer=first.layer)


def _on_device(a, name):
    """``a`` (Cloud, tensor or array, [rows, d]) as a contiguous fp32 tensor on a HIP device: its own if it lives on one, else the current one."""
    if isinstance(a, Cloud):
        a = a.flat()
    if not isinstance(a, torch.Tensor):
        a = torch.as_tensor(a)
    if a.dim() == 1:
        a = a.unsqueeze(0)                       # np.atleast_2d, as the reference
    if a.dim() != 2:
        raise ValueError(f"{name}: expected [rows, d], got shape {tuple(a.shape)}")
    if a.device.type != "cuda":
        if not torch.cuda.is_available():
            raise L.MCPCLibraryError("no HIP device is visible (%s lives on %s): the nearest-neighbour search runs on an MI355X only; "
                                     "there is no CPU path" % (name, a.device))
        a = a.to(torch.device("cuda", torch.cuda.current_device()))
    return a.to(torch.float32).contiguous()


def knn_sqdist(x, y, k: int, chunk_bytes: Optional[int] = None) -> torch.Tensor:
    """The ``k`` smallest SQUARED distances from every row of ``x`` into the rows of ``y``: fp32 ``[n, k]`` on the device, ascending
    (``engine.knn_accumulate``; +inf where ``y`` has fewer than ``k`` rows).  ``x``, ``y``: ``Cloud``, device tensors, CPU tensors or
    numpy arrays ``[rows, d]``; host data are copied to the current HIP device.  ``y`` is streamed in chunks of at most ``chunk_bytes``
    (default ``KNN_CHUNK_BYTES``) with ``accumulate=True``: the result does not depend on the chunking, bit for bit."""
    from .engine import knn_accumulate, knn_workspace_bytes
    x, y = _on_device(x, "x"), _on_device(y, "y")
    if y.device != x.device:
        y = y.to(x.device)
    if x.shape[1] != y.shape[1]:
        raise ValueError(f"x has {x.shape[1]} coordinates, y has {y.shape[1]}")
    n, d = int(x.shape[0]), int(x.shape[1])
    rows = max(1, int(KNN_CHUNK_BYTES if chunk_bytes is None else chunk_bytes) // (4 * d))
    best = torch.empty(n, int(k), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        starts = range(0, max(int(y.shape[0]), 1), rows)
        sizes = {min(rows, int(y.shape[0]) - r0) for r0 in (starts[0], starts[-1])}           # a full chunk and the last one
        ws = torch.empty(max(4, *(knn_workspace_bytes(n, m, d, k) for m in sizes)), dtype=torch.uint8, device=x.device)
        first = True
        for r0 in starts:
            knn_accumulate(x, y[r0:r0 + rows], k, best, accumulate=not first, workspace=ws)
            first = False
    return best


def kl_from_sqdist(r2: torch.Tensor, s2: torch.Tensor, n: int, m: int, d: int) -> torch.Tensor:
    """The Perez-Cruz estimate of D(P || Q) from squared nearest-neighbour distances: ``r2[i]`` from x_i to its nearest OTHER row of x
    (the second smallest of x into itself), ``s2[i]`` from x_i to its nearest row of y; ``n`` rows of x, ``m`` of y, ``d`` coordinates:
    ``-(d / n) sum_i (log r2_i - log s2_i) / 2 + log(m / (n - 1))`` -- the reference's ``-log(r / s).sum() * d / n + log(m / (n - 1.))``
    with r = sqrt(r2).  fp64 torch on the device of the inputs, a 0-d tensor.  Duplicates (r2 = 0) give what the arithmetic gives."""
    r2, s2 = r2.to(torch.float64), s2.to(torch.float64)
    return -(d / n) * (0.5 * (torch.log(r2) - torch.log(s2))).sum() + math.log(m / (n - 1.0))


def kl_divergence(x, y) -> torch.Tensor:
    """The nearest-neighbour estimate of D(P || Q) between samples ``x`` of P and ``y`` of Q (``Cloud``, tensors or arrays ``[rows, d]``;
    the reference's ``KLdivergence(x, y)``, exact instead of ``eps=.01``): the second smallest distance of x into itself and the
    smallest of x into y on the device, the sum of logarithms in fp64.  A 0-d fp64 tensor on the device.  Non-finite samples raise
    ValueError."""
    x, y = _on_device(x, "x"), _on_device(y, "y")
    for name, a in (("x", x), ("y", y)):
        if not bool(torch.isfinite(a).all()):
            raise ValueError(f"kl_divergence: {name} holds non-finite samples")
    n, d = int(x.shape[0]), int(x.shape[1])
    r2 = knn_sqdist(x, x, 2)[:, 1]
    s2 = knn_sqdist(x, y, 1)[:, 0]
    return kl_from_sqdist(r2, s2, n, int(y.shape[0]), d)

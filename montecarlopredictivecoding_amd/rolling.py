"""Rolling-window variability of a Langevin call: the request (``PCTrainer.mcpc_rolling``) and the result
(``PCTrainer.mcpc_last_rolling``).

The other reducers of the record ring pool over time: one number per element for the whole sampling window.  How the variability of a
chain CHANGES -- along a call, and across the boundary of two calls, which is what a stimulus onset is -- is a rolling statistic: the
standard deviation of the last ``window`` samples of every (chain, unit), and its mean and spread across them, per time step (the
reference takes pandas' ``rolling(window).std()`` of recorded trajectories: figure_5.py, ``variability_stimulus_onset_nonlinear``).  Here
the fused call leaves, per ``every``-th full window, the variance of each element and the sums of sd, sd^2 and the variance over the
elements, reduced out of its record ring on the device (csrc/mcpc_roll.h: one thread per element, fp64 sums of the entering and the
leaving sample, bitwise a sequential loop however the call is sliced); no trajectory is recorded.  ``carry=`` continues the stream of an
earlier call, so that a window runs across the boundary.  This module holds no device code: validation of the request, which steps are
samples and which samples emit a row, and the fp64 arithmetic from the raw sums to the mean and spread.

Cancellation.  The window's sums are updated, not recomputed: each sample adds at most 4 roundings to sums bounded by W D^2, D = max |g|
of the element, so |error of v| <= 16 j 2^-53 D^2 after j samples of the stream: about 3e-9 at j = 16000 and D = 10, against variances
of order 1.  A unit whose mean is thousands of standard deviations away from 0 wants its records shifted before they are reduced, which
this module does not do.
"""
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch

from .sampling import (SampleWindow, column_list, human_bytes, parse_keys, parse_layers, parse_outputs, parse_window,  # noqa: F401
                       require_columns, sample_steps)

_KEYS = ("begin", "stride", "layers", "outputs", "window", "every", "pool", "carry")
_OUTPUTS = (None, "identity", "sigmoid")
_POOLS = (None, "all")
_GROUP = 256                                    # csrc/mcpc_roll.h: kRollBlock, elements per workgroup of the scalar form


def emitted_rows(n_seen: int, n: int, window: int, every: int = 1) -> int:
    """Rows that samples ``n_seen .. n_seen + n - 1`` of a stream emit: one per sample j >= window - 1 with
    (j - (window - 1)) % every == 0."""
    j = max(n_seen, window - 1)
    j += -(j - (window - 1)) % every
    return (n_seen + n - 1 - j) // every + 1 if j < n_seen + n else 0


@dataclass(frozen=True, eq=False)
class RollingSpec(SampleWindow):
    """A validated ``mcpc_rolling`` request for a call of ``T`` steps."""
    layers: Tuple[int, ...]
    outputs: Optional[str]
    window: int
    every: int
    pool: Optional[str]
    carry: Optional["Rolling"]
    columns: Tuple[Tuple[str, int], ...]            # (name, width) of every block, in order: "x0", "x1", ..., "out"

    @property
    def n_seen(self) -> int:
        """Samples of the stream before this call."""
        return 0 if self.carry is None else self.carry.n_seen

    @property
    def rows(self) -> int:
        return emitted_rows(self.n_seen, self.n, self.window, self.every)

    def chunk_rows(self, n_seen: int, count: int) -> int:
        """Rows a chunk of ``count`` samples emits when the stream held ``n_seen`` samples before it."""
        return emitted_rows(n_seen, count, self.window, self.every)

    @property
    def steps(self) -> List[int]:
        """The call step of the newest sample of every row this call emits."""
        W, ev, seen = self.window, self.every, self.n_seen
        j = max(seen, W - 1)
        j += -(j - (W - 1)) % ev
        return [self.begin + (k - seen) * self.stride for k in range(j, seen + self.n, ev)]


def request_bytes(columns, B: int, window: int, n: int, rows: int, pool) -> int:
    """Bytes a request holds on the device: the state (s1, s2 in fp64 and the last ``window`` samples in fp32), the kernel's workspace
    for a slice as long as the call, and the result: what ``mcpc_rolling_max_bytes`` bounds."""
    E = [B * w for _, w in columns]
    state = sum(e * (16 + 4 * window) for e in E)
    workspace = max(-(-e // _GROUP) for e in E) * n * 32
    result = len(E) * rows * 32 + (sum(E) * rows * 8 if pool is None else 0)
    return state + workspace + result


def validate_spec(spec, T: int, n_layers: int, n_out: int, sizes, B: int, max_bytes: int) -> RollingSpec:
    """``PCTrainer.mcpc_rolling`` -> RollingSpec, or ValueError: not a dict, unknown keys, ``begin`` outside [0, T), ``stride`` < 1, a
    layer index out of range, no column at all, ``outputs`` on a model without a read-out, no ``window`` or one below 2, ``every`` < 1,
    ``pool`` not None or "all", a ``carry`` that is no Rolling of the same request, state + workspace + result larger than
    ``max_bytes``.  Defaults: begin=0, stride=1, layers=(), outputs=None, every=1, pool="all", carry=None."""
    parse_keys("mcpc_rolling", spec, _KEYS)
    begin, stride, every = parse_window("mcpc_rolling", spec, T, more_ints=(("every", 1),))
    if every < 1:
        raise ValueError(f"mcpc_rolling: every={every}, must be at least 1")
    layers = parse_layers("mcpc_rolling", spec, n_layers, none_means="empty")
    outputs = parse_outputs("mcpc_rolling", spec, n_out, _OUTPUTS)
    require_columns("mcpc_rolling", layers, outputs)
    if "window" not in spec or spec["window"] is None:
        raise ValueError("mcpc_rolling: window is required: the samples a rolling variance covers, an int of at least 2")
    window = spec["window"]
    if isinstance(window, bool) or not isinstance(window, int):
        raise ValueError(f"mcpc_rolling: window must be an int, got {window!r}")
    if window < 2:
        raise ValueError(f"mcpc_rolling: window={window}, must be at least 2")
    pool = spec.get("pool", "all")
    if pool not in _POOLS:
        raise ValueError(f"mcpc_rolling: pool={pool!r}, expected None or 'all'")
    columns = column_list(layers, sizes, None if outputs is None else "out", n_out)
    carry = spec.get("carry", None)
    if carry is not None:
        if not isinstance(carry, Rolling) or carry.state is None:
            raise ValueError("mcpc_rolling: carry must be the Rolling an earlier call left in mcpc_last_rolling (with its state)")
        mine = dict(B=B, layers=layers, window=window, stride=stride, every=every, outputs=outputs)
        theirs = dict(B=carry.B, layers=tuple(carry.layers), window=carry.window, stride=carry.stride, every=carry.every,
                      outputs=carry.outputs)
        diff = [k for k in mine if mine[k] != theirs[k]]
        if diff or tuple(carry.columns) != columns:
            raise ValueError("mcpc_rolling: carry is the result of a different request: " + (", ".join(
                f"{k}={theirs[k]!r} there, {mine[k]!r} here" for k in diff) or f"blocks {list(carry.columns)} there, {list(columns)} here"))
    out = RollingSpec(begin=begin, stride=stride, layers=layers, outputs=outputs, window=window, every=every, pool=pool, carry=carry,
                      T=T, columns=columns)
    need = request_bytes(columns, B, window, out.n, out.rows, pool)
    if need > max_bytes:
        raise ValueError(f"mcpc_rolling: the state ({B} chains x {sum(w for _, w in columns)} units x a window of {window} samples in "
                         f"fp32, and two fp64 sums), the workspace and the result ({out.rows} rows"
                         f"{'' if pool is not None else ' of every element in fp64'}) take {human_bytes(need)}, more than "
                         f"mcpc_rolling_max_bytes = {human_bytes(max_bytes)}: ask for a shorter window, fewer layers or a larger every")
    return out


@dataclass
class Rolling:
    """Rolling-window variability of one fused call (or of several, joined), per block name ("x0", "x1", ..., "out"; ``names`` keeps
    their order).  ``rows`` windows, each of ``window`` samples; ``steps[r]`` is the call step of row r's newest sample.
    ``sums[name]`` fp64 ``[rows, 4]``: over the (chain, unit) elements of the block whose variance is finite, the sum of sd, of sd^2, of
    the variance, and their count.  ``var[name]`` fp64 ``[rows, B, w]``, the variance (ddof 1) of every element's window, with
    ``pool=None`` only.  Everything derived is fp64 torch ``[rows]``.  ``state``: per block the kernel's s1, s2, hist on the engine's
    device, and ``n_seen`` the samples of the stream so far: what ``carry=`` continues."""
    B: int
    window: int
    every: int
    stride: int
    layers: Tuple[int, ...]
    outputs: Optional[str]
    columns: Tuple[Tuple[str, int], ...]
    T: int                                           # steps of the call(s) this result covers
    n_seen: int
    steps: torch.Tensor                              # int64 [rows], on the CPU
    names: List[str] = field(default_factory=list)
    sums: Dict[str, torch.Tensor] = field(default_factory=dict)
    var: Dict[str, torch.Tensor] = field(default_factory=dict)
    state: Optional[list] = None

    @property
    def rows(self) -> int:
        return int(self.steps.numel())

    def _get(self, name):
        if name not in self.sums:
            raise KeyError(f"no block {name!r}; this result has {list(self.names)}")
        return self.sums[name]

    def count(self, name: str) -> torch.Tensor:
        """The elements whose variance is finite, ``[rows]`` (fp64, whole numbers)."""
        return self._get(name)[:, 3]

    def mean_std(self, name: str) -> torch.Tensor:
        """The mean over the elements of the rolling standard deviation, ``[rows]``."""
        s = self._get(name)
        return s[:, 0] / s[:, 3]

    def mean_var(self, name: str) -> torch.Tensor:
        """The mean over the elements of the rolling variance, ``[rows]``."""
        s = self._get(name)
        return s[:, 2] / s[:, 3]

    def std_std(self, name: str) -> torch.Tensor:
        """The standard deviation (ddof 1) across the elements of the rolling standard deviation, ``[rows]``."""
        s = self._get(name)
        c = s[:, 3]
        return torch.sqrt(torch.clamp((s[:, 1] - s[:, 0] * (s[:, 0] / c)) / (c - 1), min=0.0))

    def sem(self, name: str) -> torch.Tensor:
        """``std_std`` over the square root of the count, ``[rows]``."""
        return self.std_std(name) / torch.sqrt(self.count(name))

    def all(self) -> "Rolling":
        """The blocks pooled into one, "all": every (chain, unit) of every block a series, which is what the figure plots."""
        total = self.sums[self.names[0]].clone()
        for k in self.names[1:]:
            total = total + self.sums[k]
        return Rolling(B=self.B, window=self.window, every=self.every, stride=self.stride, layers=self.layers, outputs=self.outputs,
                       columns=(("all", sum(w for _, w in self.columns)),), T=self.T, n_seen=self.n_seen, steps=self.steps,
                       names=["all"], sums={"all": total})

    @staticmethod
    def cat(parts, dim: str = "time") -> "Rolling":
        """``dim="time"``: the results of successive calls of one stream (the later ones with ``carry=``) joined along the rows; the
        steps of a later call count on from the steps of the earlier ones, and the state is the last call's.  ``dim="chains"``: the
        results of different batches (same request, same rows) joined along the chains; their sums add."""
        parts = list(parts)
        first = parts[0]

        def key(p):
            return (p.window, p.every, p.stride, tuple(p.layers), p.outputs, list(p.names), sorted(p.var))
        if any(key(p) != key(first) for p in parts):
            raise ValueError("Rolling.cat: the results are of different requests")
        if dim == "time":
            if any(p.B != first.B for p in parts):
                raise ValueError("Rolling.cat: the results are of different requests")
            steps, t0 = [], 0
            for p in parts:
                steps.append(p.steps + t0)
                t0 += p.T
            return Rolling(B=first.B, window=first.window, every=first.every, stride=first.stride, layers=first.layers,
                           outputs=first.outputs, columns=first.columns, T=t0, n_seen=parts[-1].n_seen, steps=torch.cat(steps),
                           names=list(first.names), sums={k: torch.cat([p.sums[k] for p in parts], dim=0) for k in first.names},
                           var={k: torch.cat([p.var[k] for p in parts], dim=0) for k in first.var}, state=parts[-1].state)
        if dim != "chains":
            raise ValueError(f"Rolling.cat: dim={dim!r}, expected 'time' or 'chains'")
        if any(not torch.equal(p.steps, first.steps) or p.T != first.T for p in parts):
            raise ValueError("Rolling.cat: the results are of different requests")
        sums = {}
        for k in first.names:
            sums[k] = first.sums[k].clone()
            for p in parts[1:]:
                sums[k] = sums[k] + p.sums[k]
        return Rolling(B=sum(p.B for p in parts), window=first.window, every=first.every, stride=first.stride, layers=first.layers,
                       outputs=first.outputs, columns=first.columns, T=first.T, n_seen=first.n_seen, steps=first.steps,
                       names=list(first.names), sums=sums, var={k: torch.cat([p.var[k] for p in parts], dim=1) for k in first.var})


def new_state(spec: RollingSpec, B: int, device):
    """The kernel's state per block for a call: fresh, or a copy of the carried one (the earlier result keeps its own)."""
    if spec.carry is not None:
        return [dict(s1=st["s1"].to(device, copy=True), s2=st["s2"].to(device, copy=True), hist=st["hist"].to(device, copy=True),
                     n_seen=st["n_seen"]) for st in spec.carry.state]
    return [dict(s1=torch.zeros(B, w, dtype=torch.float64, device=device), s2=torch.zeros(B, w, dtype=torch.float64, device=device),
                 hist=torch.zeros(spec.window, B, w, dtype=torch.float32, device=device), n_seen=0) for _, w in spec.columns]


def from_state(spec: RollingSpec, B: int, state, pooled, elem, device) -> Rolling:
    """The kernel's outputs per block (``pooled`` [rows, 4]; ``elem`` [rows, B, w] or None) -> Rolling with the results on ``device``."""
    r = Rolling(B=B, window=spec.window, every=spec.every, stride=spec.stride, layers=spec.layers, outputs=spec.outputs,
                columns=spec.columns, T=spec.T, n_seen=spec.n_seen + spec.n, steps=torch.tensor(spec.steps, dtype=torch.int64),
                names=[nm for nm, _ in spec.columns], state=state)
    for (nm, _), p, e in zip(spec.columns, pooled, elem):
        r.sums[nm] = p.to(device)
        if e is not None:
            r.var[nm] = e.to(device)
    return r

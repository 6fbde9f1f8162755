"""The statistics a fused call reduces out of its record ring: one reducer per request, and the table that names the requests.

``PCTrainer._run_fused_sliced`` runs a call as slices; the records of a slice fill one half of a two-buffer device ring.  A reducer
turns the filled half into its statistic on the device, so that the trajectory is never materialised.  The driver knows reducers only
through this interface:

``layers``            the latent layers it reads from the ring,
``reads_out``         whether it reads the read-out's records,
``step_bytes(B)``     further device bytes per step of a slice, beside the ring (the derived records of the prediction errors),
``side_stream``       whether its reduction may run on the drain's side stream while the next slice fills the other half,
``attr``              the trainer attribute its result is left in,
``start(B, dev, S)``  allocate accumulators and workspace, for slices of at most ``S`` steps; the last point at which a request is
                      refused (ValueError), before anything runs,
``reduce(t0, n, view)`` add the samples among steps t0 .. t0 + n - 1; ``view.x[l]`` is the ring half's block of latent layer l (row k is
                      step t0 + k) and ``view.out`` the read-out rows of this slice,
``result()``          the statistic, on the model's device.

Reducers run after every slice in the order of ``REQUESTS``, on the current stream.  A request is named in ``REQUESTS`` alone:
``train_on_batch`` validates the requests of a call from it and ``_run_fused`` builds the reducers from it.
"""
from dataclasses import dataclass
from typing import Any, Callable, Optional

import torch

from .. import _lib as L
from .. import autocovariance, chain_energies, cloud, covariance, errors, histogram, histogram2d, moments, probe, rolling
from ..engine import (acov_accumulate, cov_accumulate, cov_workspace_bytes, hist2d_accumulate, hist_accumulate, moments_accumulate,
                      probe_accumulate, probe_records, roll_accumulate, roll_workspace_bytes)


@dataclass
class Call:
    """What a reducer may know of the call it serves."""
    trainer: Any                                 # the PCTrainer: its mcpc_* settings
    eng: Any                                     # the Engine
    net: Any                                     # recognise.Net
    model_device: torch.device                   # where results go
    inputs: Optional[torch.Tensor]               # the call's inputs on the engine's device (None: all zero)
    loss_kw: dict                                # loss_kind, loss_var, mask_start of the call


@dataclass
class RingView:
    """One filled half of the ring."""
    x: list                                      # per latent layer the [n, B, n_l] rows of this slice, None for a layer not in the ring
    out: Optional[torch.Tensor]                  # the read-out's rows of this slice, from row 0


class Reducer:
    attr = None
    side_stream = False

    def __init__(self, spec, call: Call):
        self.spec, self.call = spec, call
        self.layers = tuple(getattr(spec, "layers", ()))
        self.reads_out = getattr(spec, "outputs", None) is not None

    def step_bytes(self, B):
        return 0

    def start(self, B, dev, S):
        self.B, self.dev = B, dev

    def reduce(self, t0, n, view):
        first, cnt = self.spec.chunk(t0, n)
        if cnt:
            self.add(first, cnt, t0, view)

    def blocks(self, view):
        """The blocks of the request's columns, in their order."""
        return [view.x[l] for l in self.layers] + ([view.out] if self.reads_out else [])

    def transforms(self):
        return ["identity"] * len(self.layers) + ([self.spec.outputs] if self.reads_out else [])

    def zeros(self, *shape, dtype=torch.float64):
        return torch.zeros(*shape, dtype=dtype, device=self.dev)


class MomentsReducer(Reducer):
    """``mcpc_moments``: fp64 sums and sums of squares per (chain, unit), by ``moments_accumulate``.  The one reducer that may run on
    the side stream (``mcpc_moments_side_stream``)."""
    attr = "mcpc_last_moments"

    def __init__(self, spec, call):
        super().__init__(spec, call)
        self.side_stream = bool(call.trainer.mcpc_moments_side_stream)

    def start(self, B, dev, S):
        super().start(B, dev, S)
        net, spec = self.call.net, self.spec
        self.x_sum = [self.zeros(B, n) if l in spec.layers else None for l, n in enumerate(net.sizes)]
        self.x_sumsq = [self.zeros(B, n) if l in spec.layers and spec.variance else None for l, n in enumerate(net.sizes)]
        self.out_sum = self.zeros(B, net.n_out) if self.reads_out else None
        self.out_sumsq = self.zeros(B, net.n_out) if self.reads_out and spec.variance else None

    def add(self, first, cnt, t0, view):
        for l in self.layers:
            moments_accumulate(view.x[l], first, self.spec.stride, cnt, self.x_sum[l], self.x_sumsq[l], accumulate=True)
        if self.reads_out:
            moments_accumulate(view.out, first, self.spec.stride, cnt, self.out_sum, self.out_sumsq, transform=self.spec.outputs,
                               accumulate=True)

    def result(self):
        md = self.call.model_device

        def back(t):
            return None if t is None else t.to(md)
        return moments.Moments(n=self.spec.n, x_sum=[back(t) for t in self.x_sum], x_sumsq=[back(t) for t in self.x_sumsq],
                               out_sum=back(self.out_sum), out_sumsq=back(self.out_sumsq))


class ChainEnergiesReducer(Reducer):
    """``mcpc_chain_energies``: every latent layer goes through the ring and ``Engine.chain_energies`` evaluates the steps asked for out
    of its rows into one ``[n, B, L + 2]`` table."""
    attr = "mcpc_last_chain_energies"

    def __init__(self, spec, call):
        super().__init__(spec, call)
        self.layers = tuple(range(len(call.net.sizes)))

    def start(self, B, dev, S):
        super().start(B, dev, S)
        self.table = torch.empty(self.spec.n, B, L.ENERGY_COLS, dtype=torch.float64, device=dev)
        self.kw = dict(self.call.loss_kw, max_rows=self.call.trainer.mcpc_chain_energies_max_rows)

    def add(self, first, cnt, t0, view):
        spec, eng, inputs = self.spec, self.call.eng, self.call.inputs
        k0 = (t0 + first - spec.begin) // spec.stride            # index of the slice's first evaluated step among all of them
        if spec.stride == 1:
            eng.chain_energies(inputs, [r_[first:first + cnt] for r_ in view.x], out=self.table[k0:k0 + cnt], **self.kw)
        else:
            for k in range(cnt):
                row = first + k * spec.stride
                eng.chain_energies(inputs, [r_[row:row + 1] for r_ in view.x], out=self.table[k0 + k:k0 + k + 1], **self.kw)

    def result(self):
        return chain_energies.from_table(self.table, len(self.call.net.sizes), self.call.trainer._energy_coefficient, self.spec.steps,
                                         self.call.model_device)


class CovarianceReducer(Reducer):
    """``mcpc_covariance``: fp64 outer products by ``cov_accumulate`` and the first-order sums of each block by ``moments_accumulate``.
    The outer products depend on where the slices fall (within the bound of DESIGN.md section 4)."""
    attr = "mcpc_last_covariance"

    def start(self, B, dev, S):
        super().start(B, dev, S)
        spec, D = self.spec, self.spec.D
        widths = [w for _, _, w in spec.columns]
        self.xf = self.transforms()
        self.outer = self.zeros(*((D, D) if spec.pooled else (B, D, D)))
        # the first-order sums of a block, contiguous for moments_accumulate; gathered into `sum` at the end
        self.part = [self.zeros(B, w) for w in widths]
        self.ws = torch.empty(max(cov_workspace_bytes(B, widths), 8), dtype=torch.uint8, device=dev) if spec.pooled else None

    def add(self, first, cnt, t0, view):
        spec, blocks = self.spec, self.blocks(view)
        for blk, part, xf in zip(blocks, self.part, self.xf):
            moments_accumulate(blk, first, spec.stride, cnt, part, None, transform=xf, accumulate=True)
        cov_accumulate(blocks, first, spec.stride, cnt, self.outer, transforms=self.xf, pool=spec.pooled, accumulate=True,
                       workspace=self.ws)

    def result(self):
        spec, md = self.spec, self.call.model_device
        s = torch.cat(self.part, dim=1)
        if spec.pooled:
            s = s.sum(dim=0)
        return covariance.Covariance(n=spec.n, B=self.B, pooled=spec.pooled, columns=list(spec.columns), sum=s.to(md),
                                     outer=self.outer.to(md))


class HistogramReducer(Reducer):
    """``mcpc_histogram``: int64 counts per block by ``hist_accumulate``."""
    attr = "mcpc_last_histogram"

    def start(self, B, dev, S):
        super().start(B, dev, S)
        spec = self.spec
        self.xf = self.transforms()
        self.counts = [self.zeros(*((w, len(e) + 2) if spec.pooled else (B, w, len(e) + 2)), dtype=torch.int64)
                       for (_, w), e in zip(spec.columns, spec.edges)]

    def add(self, first, cnt, t0, view):
        spec = self.spec
        for blk, e, counts, xf in zip(self.blocks(view), spec.edges, self.counts, self.xf):
            hist_accumulate(blk, first, spec.stride, cnt, e, counts, transform=xf, pool=spec.pooled, accumulate=True)

    def result(self):
        return histogram.from_counts(self.spec, self.B, self.counts, self.call.model_device)


class AutocovarianceReducer(Reducer):
    """``mcpc_autocovariance``: lagged products per block by ``acov_accumulate``, in step order; the samples seen so far are counted per
    block and the kernel's own window carries the lags across slices."""
    attr = "mcpc_last_autocovariance"

    def start(self, B, dev, S):
        super().start(B, dev, S)
        K = self.spec.max_lag
        self.xf = self.transforms()
        self.state = [dict(lagged=self.zeros(B, w, K + 1), sum=self.zeros(B, w), window=self.zeros(K, B, w, dtype=torch.float32),
                           head=self.zeros(K, B, w, dtype=torch.float32), n_seen=0) for _, w in self.spec.columns]

    def add(self, first, cnt, t0, view):
        spec = self.spec
        for blk, st, xf in zip(self.blocks(view), self.state, self.xf):
            acov_accumulate(blk, first, spec.stride, cnt, spec.max_lag, st["n_seen"], st["lagged"], st["sum"], st["window"], st["head"],
                            transform=xf)
            st["n_seen"] += cnt

    def result(self):
        return autocovariance.from_state(self.spec, self.B, self.state, self.call.model_device)


class ProbeReducer(Reducer):
    """``mcpc_probe``: one ``probe_accumulate`` per slice adds the link values, votes and entropies of the slice's samples of the
    probe's layer (overwriting in the first slice that holds one)."""
    attr = "mcpc_last_probe"

    def __init__(self, spec, call):
        super().__init__(spec, call)
        self.layers = (spec.layer,)

    def start(self, B, dev, S):
        super().start(B, dev, S)
        self.w, self.b = self.spec.on(dev)
        self.state = probe.new_state(B, self.spec.C, self.spec.link, dev)
        self.seen = False

    def add(self, first, cnt, t0, view):
        spec, st = self.spec, self.state
        probe_accumulate(view.x[spec.layer], first, spec.stride, cnt, self.w, self.b, spec.link, st["psum"], st["psumsq"], st["votes"],
                         st["entsum"], accumulate=self.seen)
        self.seen = True

    def result(self):
        spec = self.spec
        return probe.from_state(spec.n, self.B, spec.C, spec.link, self.state, self.call.model_device)


class CloudReducer(Reducer):
    """``mcpc_cloud``: the slice's samples of the chosen units are gathered (``index_select``) into one preallocated tensor, which
    stays on the engine's device."""
    attr = "mcpc_last_cloud"

    def __init__(self, spec, call):
        super().__init__(spec, call)
        self.layers = (spec.layer,)

    def start(self, B, dev, S):
        super().start(B, dev, S)
        self.points = torch.empty(self.spec.n, B, self.spec.d, dtype=torch.float32, device=dev)
        self.units = torch.tensor(self.spec.units, dtype=torch.int64, device=dev)

    def add(self, first, cnt, t0, view):
        spec = self.spec
        k0 = (t0 + first - spec.begin) // spec.stride            # index of the slice's first sample among all of them
        rows = view.x[spec.layer][first:first + (cnt - 1) * spec.stride + 1:spec.stride]
        torch.index_select(rows, 2, self.units, out=self.points[k0:k0 + cnt])

    def result(self):
        return cloud.Cloud(points=self.points, units=self.spec.units, layer=self.spec.layer)


class RollingReducer(Reducer):
    """``mcpc_rolling``: ``roll_accumulate`` feeds each block's samples to its rolling variance, in step order; the samples seen and
    the rows emitted so far are counted per block, and the kernel's own history carries a window across slices (and, with ``carry=``,
    across calls)."""
    attr = "mcpc_last_rolling"

    def start(self, B, dev, S):
        super().start(B, dev, S)
        spec = self.spec
        self.xf = self.transforms()
        self.state = rolling.new_state(spec, B, dev)
        self.row = [0] * len(self.state)                         # rows this call has emitted for the block
        self.pooled = [self.zeros(spec.rows, 4) for _ in spec.columns]
        self.elem = [self.zeros(spec.rows, B, w) if spec.pool is None else None for _, w in spec.columns]
        self.ws = torch.empty(max(max(roll_workspace_bytes(B, w, min(S, spec.n)) for _, w in spec.columns), 8), dtype=torch.uint8,
                              device=dev)

    def add(self, first, cnt, t0, view):
        spec = self.spec
        for j, (blk, st, xf, pooled, elem) in enumerate(zip(self.blocks(view), self.state, self.xf, self.pooled, self.elem)):
            r0 = self.row[j]
            self.row[j] += roll_accumulate(blk, first, spec.stride, cnt, spec.window, spec.every, st["n_seen"], st["s1"], st["s2"],
                                           st["hist"], out_elem=None if elem is None else elem[r0:], out_pool=pooled[r0:],
                                           workspace=self.ws, transform=xf)
            st["n_seen"] += cnt

    def result(self):
        return rolling.from_state(self.spec, self.B, self.state, self.pooled, self.elem, self.call.model_device)


class ErrorsReducer(Reducer):
    """``mcpc_errors``: the requested layers and the layers their predictions read go through the ring; the slice's samples (gathered
    first when the stride skips steps) are evaluated by ``Engine.prediction_errors`` into one set of derived buffers, which
    ``moments_accumulate`` / ``cov_accumulate`` reduce.  The derived buffers are as long as the longest slice's samples, so the byte
    bound is checked again in ``start``."""
    attr = "mcpc_last_errors"

    def __init__(self, spec, call):
        super().__init__(spec, call)
        self.layers, self.reads_out = spec.reads, False          # the read-out's prediction is evaluated from the last layer's records

    def step_bytes(self, B):
        return -(-4 * B * self.spec.D // self.spec.stride)       # the derived records of a step's share of the samples

    def start(self, B, dev, S):
        super().start(B, dev, S)
        spec, tr = self.spec, self.call.trainer
        rows = spec.max_samples(S)
        errors.check_bytes(spec, B, rows, tr.mcpc_errors_max_bytes)
        self.bufs = {name: torch.empty(rows, B, w, dtype=torch.float32, device=dev) for name, _, w in spec.columns}
        self.sum = {name: self.zeros(B, w) for name, _, w in spec.columns}
        self.sumsq = {name: self.zeros(B, w) if spec.variance else None for name, _, w in spec.columns}
        self.outer = self.ws = None
        if spec.covariance is not None:
            D = spec.D
            self.outer = self.zeros(*((D, D) if spec.pooled else (B, D, D)))
            if spec.pooled:
                self.ws = torch.empty(max(cov_workspace_bytes(B, [w for _, _, w in spec.columns]), 8), dtype=torch.uint8, device=dev)
        self.kw = dict(self.call.loss_kw, layers=spec.layers, quantity=spec.quantity, outputs=spec.outputs,
                       max_rows=tr.mcpc_chain_energies_max_rows)

    def add(self, first, cnt, t0, view):
        spec = self.spec
        # the slice's samples alone (a copy when the stride skips steps): the derived buffers hold samples only
        stop = first + (cnt - 1) * spec.stride + 1
        recs = [x[first:stop:spec.stride].contiguous() if l in spec.reads else None for l, x in enumerate(view.x)]
        self.call.eng.prediction_errors(self.call.inputs, recs, out={name: buf[:cnt] for name, buf in self.bufs.items()}, **self.kw)
        for name, buf in self.bufs.items():
            moments_accumulate(buf, 0, 1, cnt, self.sum[name], self.sumsq[name], accumulate=True)
        if self.outer is not None:
            cov_accumulate(list(self.bufs.values()), 0, 1, cnt, self.outer, pool=spec.pooled, accumulate=True, workspace=self.ws)

    def result(self):
        spec, md = self.spec, self.call.model_device
        pcov = None
        if self.outer is not None:
            s = torch.cat([self.sum[name] for name, _, _ in spec.columns], dim=1)
            if spec.pooled:
                s = s.sum(dim=0)
            pcov = covariance.Covariance(n=spec.n, B=self.B, pooled=spec.pooled, columns=list(spec.columns), sum=s.to(md),
                                         outer=self.outer.to(md))
        return errors.Errors(n=spec.n, sum={k: v.to(md) for k, v in self.sum.items()},
                             sumsq={k: None if v is None else v.to(md) for k, v in self.sumsq.items()}, covariance=pcov)


class Histogram2DReducer(Reducer):
    """``mcpc_histogram2d``: int64 joint counts by ``hist2d_accumulate``.  Units form: straight out of the ring rows of the one or two
    layers.  Probe form: the slice's samples go through ``probe_records`` twice -- the link values of the probe, then their projection
    onto the plane, two derived records as long as the longest slice's samples -- and the plane's two coordinates are the one pair."""
    attr = "mcpc_last_histogram2d"

    def __init__(self, spec, call):
        super().__init__(spec, call)
        self.layers, self.reads_out = spec.layers, False

    def step_bytes(self, B):
        if self.spec.probe is None:
            return 0
        return -(-4 * B * (self.spec.probe.C + 2) // self.spec.stride)   # the derived records of a step's share of the samples

    def start(self, B, dev, S):
        super().start(B, dev, S)
        spec = self.spec
        grid = (len(spec.pairs), len(spec.edges_x) + 2, len(spec.edges_y) + 2)
        self.counts = self.zeros(*(grid if spec.pooled else (B,) + grid), dtype=torch.int64)
        if spec.probe is not None:
            rows = spec.max_samples(S)
            self.w, self.b = spec.probe.on(dev)
            self.plane = torch.from_numpy(spec.project.copy()).to(dev)
            self.p = torch.empty(rows, B, spec.probe.C, dtype=torch.float32, device=dev)
            self.xy = torch.empty(rows, B, 2, dtype=torch.float32, device=dev)

    def add(self, first, cnt, t0, view):
        spec = self.spec
        kw = dict(pool=spec.pooled, accumulate=True)
        if spec.probe is None:
            hist2d_accumulate(view.x[spec.x_layer], view.x[spec.y_layer], first, spec.stride, cnt, spec.pairs, spec.edges_x,
                              spec.edges_y, self.counts, **kw)
            return
        probe_records(view.x[spec.probe.layer], first, spec.stride, cnt, self.w, self.b, spec.probe.link, out=self.p[:cnt])
        probe_records(self.p, 0, 1, cnt, self.plane, None, "identity", out=self.xy[:cnt])
        hist2d_accumulate(self.xy, self.xy, 0, 1, cnt, spec.pairs, spec.edges_x, spec.edges_y, self.counts, **kw)

    def result(self):
        return histogram2d.from_counts(self.spec, self.B, self.counts, self.call.model_device)


@dataclass(frozen=True)
class Request:
    """One row of ``REQUESTS``."""
    attr: str                                    # the trainer attribute that holds the request (None = off)
    key: str                                     # where the validated request goes in the call's plan
    module: Any                                  # the request module: its validate_spec(request, T, *args)
    only: str                                    # the end of the sentence that refuses a call the fused loop does not run
    args: Callable                               # (trainer, net, plan) -> validate_spec's arguments after T
    reducer: type


def _columns(max_bytes):
    return lambda tr, net, plan: (len(net.sizes), net.n_out, net.sizes, plan["B"], getattr(tr, max_bytes))


# in the order the reducers run after a slice
REQUESTS = (
    Request("mcpc_moments", "moments", moments, "posterior moments are accumulated by the fused HIP loop only",
            lambda tr, net, plan: (len(net.sizes), net.n_out), MomentsReducer),
    Request("mcpc_chain_energies", "chain_energies", chain_energies,
            "per-chain energies are evaluated out of the fused HIP loop's record ring only", lambda tr, net, plan: (),
            ChainEnergiesReducer),
    Request("mcpc_covariance", "covariance", covariance, "posterior covariances are accumulated by the fused HIP loop only",
            _columns("mcpc_covariance_max_bytes"), CovarianceReducer),
    Request("mcpc_histogram", "histogram", histogram, "posterior histograms are counted by the fused HIP loop only",
            _columns("mcpc_histogram_max_bytes"), HistogramReducer),
    Request("mcpc_autocovariance", "autocovariance", autocovariance, "lagged autocovariances are accumulated by the fused HIP loop only",
            _columns("mcpc_autocovariance_max_bytes"), AutocovarianceReducer),
    Request("mcpc_probe", "probe", probe, "the posterior of a probe is accumulated by the fused HIP loop only",
            lambda tr, net, plan: (len(net.sizes), net.sizes, plan["B"]), ProbeReducer),
    Request("mcpc_cloud", "cloud", cloud, "the sample cloud is gathered by the fused HIP loop only",
            lambda tr, net, plan: (len(net.sizes), net.sizes, plan["B"], tr.mcpc_cloud_max_bytes), CloudReducer),
    Request("mcpc_rolling", "rolling", rolling, "the rolling variability is accumulated by the fused HIP loop only",
            _columns("mcpc_rolling_max_bytes"), RollingReducer),
    Request("mcpc_errors", "errors", errors, "prediction errors are evaluated out of the fused HIP loop's record ring only",
            lambda tr, net, plan: (len(net.sizes), net.n_out, net.sizes, plan["B"], plan["loss"].kind != L.LOSS_NONE,
                                   tr.mcpc_errors_max_bytes), ErrorsReducer),
    Request("mcpc_histogram2d", "histogram2d", histogram2d, "joint histograms are counted by the fused HIP loop only",
            _columns("mcpc_histogram2d_max_bytes"), Histogram2DReducer),
)


def validate(trainer, plan, T, runs_on=None):
    """Validate every request set on the trainer into ``plan`` (ValueError), or refuse the call: ``runs_on`` says where a call runs that
    the fused loop does not ("on the generic torch loop (why)", "step by step (why)") and no reducer can serve."""
    for row in REQUESTS:
        if getattr(trainer, row.attr) is None:
            continue
        if runs_on is not None:
            raise NotImplementedError(f"{row.attr} is set, and this call runs {runs_on}: {row.only}")
        net = plan["net"]
        plan[row.key] = row.module.validate_spec(getattr(trainer, row.attr), T, *row.args(trainer, net, plan))


def reducers(plan, call: Call):
    """The reducers of the requests validated into ``plan``, in the order they run."""
    return [row.reducer(plan[row.key], call) for row in REQUESTS if row.key in plan]

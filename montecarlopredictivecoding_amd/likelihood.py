"""The importance-sampled log marginal likelihood PER DATUM: the result (``LogLikelihood``) and the front that streams the samples
(``log_likelihood``).

The reference's ``get_marginal_likelihood`` (``utils/training_evaluation.py``) draws S samples from the prior, forms the fp32 matrix of
negative log-likelihoods ``[batch, S]`` per batch and keeps one number, the mean over the data of ``log mean_s p(y | sample s)``.
Importance sampling from the prior is degenerate for most data -- a handful of samples carry the whole weight -- and the mean hides
that.  Here every datum keeps the state of its own estimate, ``(m, s1, s2, cnt)``: the smallest nll, the sums of ``exp(-(nll - m))``
and of its square and the number of samples taken, accumulated in fp64 on the device (csrc/mcpc_loglik.h).  From it come the estimate
``log(s1 / cnt) - m``, the effective sample size of its weights ``s1^2 / s2``, and a rule to merge the states of disjoint sets of
samples, so that S is bounded by patience and not by memory.  This module holds no device code.
"""
import math
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib as L

LOGLIK_CHUNK_BYTES = 256 << 20                   # read-outs handed to one loglik_accumulate call by log_likelihood
_TARGET_JOBS = 8192                              # csrc/mcpc_loglik.h: kLoglikTargetJobs


def plan(n_data: int, n_samp: int, width: int) -> dict:
    """The launch shape of one ``loglik_accumulate`` call, the twin of csrc/mcpc_loglik.h's ``loglik_plan``: 16-datum tiles, 16-sample
    tiles, sample tiles per group, groups, and the workspace bytes they need (tests hold it against ``loglik_workspace_bytes``)."""
    n_dtiles, n_stiles = (int(n_data) + 15) // 16, (int(n_samp) + 15) // 16
    if n_dtiles == 0 or n_stiles == 0:
        return dict(n_dtiles=0, n_stiles=0, tiles_per_group=0, groups=0, workspace_bytes=0)
    want = min(-(-_TARGET_JOBS // n_dtiles), n_stiles)
    per = -(-n_stiles // want)
    groups = -(-n_stiles // per)
    return dict(n_dtiles=n_dtiles, n_stiles=n_stiles, tiles_per_group=per, groups=groups,
                workspace_bytes=8 * (groups * n_dtiles * 16 * 4 + int(n_data) + int(n_samp)))


def empty_state(n: int, device=None) -> torch.Tensor:
    """``[n, 4]`` fp64 states without samples: ``(+inf, 0, 0, 0)``."""
    st = torch.zeros(int(n), 4, dtype=torch.float64, device=device)
    st[:, 0] = math.inf
    return st


def merge_states(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """The merge rule of include/mcpc.h (mcpc_loglik_accumulate) in torch fp64: the states of the same data over two disjoint sets of
    samples.  An empty side has the factor 0; inf - inf is never formed."""
    a, b = a.to(torch.float64), b.to(torch.float64)
    if a.shape != b.shape or a.dim() != 2 or a.shape[1] != 4:
        raise ValueError(f"expected two [N, 4] states, got {tuple(a.shape)} and {tuple(b.shape)}")
    m = torch.minimum(a[:, 0], b[:, 0])
    live = m < math.inf                           # a taken nll is finite: m is finite or +inf
    base = torch.where(live, m, torch.zeros_like(m))
    zero = torch.zeros_like(m)
    fa = torch.where(a[:, 0] < math.inf, torch.exp(base - torch.where(a[:, 0] < math.inf, a[:, 0], base)), zero)
    fb = torch.where(b[:, 0] < math.inf, torch.exp(base - torch.where(b[:, 0] < math.inf, b[:, 0], base)), zero)
    out = torch.stack([m, a[:, 1] * fa + b[:, 1] * fb, a[:, 2] * fa * fa + b[:, 2] * fb * fb, a[:, 3] + b[:, 3]], dim=1)
    return torch.where(live.unsqueeze(1), out, empty_state(m.shape[0], m.device))


@dataclass
class LogLikelihood:
    """The importance-sampling state of N data: ``state`` fp64 ``[N, 4]``, per datum ``(m, s1, s2, cnt)`` (include/mcpc.h:
    mcpc_loglik_accumulate), on the device that accumulated it."""
    state: torch.Tensor

    def __len__(self) -> int:
        return int(self.state.shape[0])

    @property
    def n_samples(self) -> torch.Tensor:
        """``[N]``: the samples taken per datum (those with a finite nll)."""
        return self.state[:, 3]

    @property
    def log_p(self) -> torch.Tensor:
        """``[N]``: ``log(s1 / cnt) - m``, the estimate of log p(datum); NaN where no sample was taken."""
        m, s1, cnt = self.state[:, 0], self.state[:, 1], self.state[:, 3]
        taken = cnt > 0
        one = torch.ones_like(s1)
        val = torch.log(torch.where(taken, s1, one) / torch.where(taken, cnt, one)) - torch.where(taken, m, torch.zeros_like(m))
        return torch.where(taken, val, torch.full_like(val, math.nan))

    @property
    def ess(self) -> torch.Tensor:
        """``[N]``: the effective sample size of the importance weights, ``s1^2 / s2``, in [1, cnt]; NaN where no sample was taken."""
        s1, s2 = self.state[:, 1], self.state[:, 2]
        taken = self.state[:, 3] > 0
        val = s1 * s1 / torch.where(taken, s2, torch.ones_like(s2))
        return torch.where(taken, val, torch.full_like(val, math.nan))

    def mean(self) -> float:
        """The reference's scalar: the mean of ``log_p`` over the data."""
        return float(self.log_p.mean())

    def merge(self, other: "LogLikelihood") -> "LogLikelihood":
        """The same data, more samples."""
        if len(other) != len(self):
            raise ValueError(f"LogLikelihood.merge: {len(self)} data against {len(other)}")
        return LogLikelihood(state=merge_states(self.state, other.state.to(self.state.device)))

    @staticmethod
    def cat(parts) -> "LogLikelihood":
        """More data: the states of different data joined in the order given."""
        parts = list(parts)
        return LogLikelihood(state=torch.cat([p.state for p in parts], dim=0))

    def cpu(self) -> "LogLikelihood":
        return LogLikelihood(state=self.state.cpu())


def _on_device(a, name):
    """``a`` (tensor or array, [rows, width]) as a contiguous fp32 tensor on a HIP device: its own if it lives on one, else the current one."""
    if not isinstance(a, torch.Tensor):
        a = torch.tensor(a)                      # a copy: the array may be read-only
    if a.dim() == 1:
        a = a.unsqueeze(0)
    if a.dim() != 2:
        raise ValueError(f"{name}: expected [rows, width], got shape {tuple(a.shape)}")
    if a.device.type != "cuda":
        if not torch.cuda.is_available():
            raise L.MCPCLibraryError("no HIP device is visible (%s lives on %s): the marginal likelihood runs on an MI355X only; "
                                     "there is no CPU path" % (name, a.device))
        a = a.to(torch.device("cuda", torch.cuda.current_device()))
    return a.to(torch.float32).contiguous()


def log_likelihood(data, outputs, loss="bernoulli", var=None, clamp=20.0, state: Optional[LogLikelihood] = None,
                   chunk_bytes: Optional[int] = None) -> LogLikelihood:
    """The per-datum importance-sampling state of ``data`` ``[N, width]`` over the read-outs ``outputs`` ``[S, width]`` of prior samples
    (logits for ``loss="bernoulli"``, means for ``loss="gaussian"`` with the variance ``var``), clamped to ``+-clamp`` as the reference
    clamps to 20 (``math.inf``: not at all).  ``data``, ``outputs``: device tensors, CPU tensors or arrays; host data are copied to the
    current HIP device.  ``outputs`` is streamed in chunks of at most ``chunk_bytes`` (default ``LOGLIK_CHUNK_BYTES``) with
    ``accumulate=True``; ``state``: a ``LogLikelihood`` of the same data over EARLIER samples, which is continued (not modified).  The
    chunking moves the result within the rounding bound of include/mcpc.h, not bitwise."""
    from .engine import loglik_accumulate, loglik_workspace_bytes
    y, o = _on_device(data, "data"), _on_device(outputs, "outputs")
    if o.device != y.device:
        o = o.to(y.device)
    if y.shape[1] != o.shape[1]:
        raise ValueError(f"data has {y.shape[1]} columns, outputs has {o.shape[1]}")
    n, width, S = int(y.shape[0]), int(y.shape[1]), int(o.shape[0])
    rows = max(1, int(LOGLIK_CHUNK_BYTES if chunk_bytes is None else chunk_bytes) // (4 * width))
    if state is not None:
        if len(state) != n:
            raise ValueError(f"state holds {len(state)} data, data has {n}")
        st = state.state.to(device=y.device, dtype=torch.float64).clone().contiguous()
    else:
        st = torch.empty(n, 4, dtype=torch.float64, device=y.device)
    with torch.cuda.device(y.device):
        starts = range(0, max(S, 1), rows)
        sizes = {min(rows, S - r0) for r0 in (starts[0], starts[-1])}                          # a full chunk and the last one
        ws = torch.empty(max(8, *(loglik_workspace_bytes(n, m, width) for m in sizes)), dtype=torch.uint8, device=y.device)
        first = state is None
        for r0 in starts:
            loglik_accumulate(y, o[r0:r0 + rows], loss, var, clamp, st, accumulate=not first, workspace=ws)
            first = False
    return LogLikelihood(state=st)

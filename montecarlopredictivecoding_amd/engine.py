"""Thin object wrapper over the libmcpc C ABI.

PyTorch appears here only as the owner of device memory and of the HIP stream: every tensor is
handed to the library as ``data_ptr()`` + sizes.  The computation is the hand-written HIP code in
``csrc/`` -- this module contains no arithmetic and no fallback.
"""
import ctypes as C
import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import torch

from . import _lib as L


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _check_tensor(t: torch.Tensor, shape, device, name, dtype=torch.float32):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t)}")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    if t.device != device:
        raise ValueError(f"{name}: expected device {device}, got {t.device}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: tensor must be contiguous")


def _record_window(rec, first, stride, n, rank=3, what="[records, B, width]", holds="rec holds"):
    """What a stateless reducer checks before it looks at its own arguments.  ``rec`` is a record buffer as an engine run fills it: a
    contiguous fp32 tensor of ``rank`` dimensions (None: one at least) on a HIP device.  The records ``first + k * stride``, k < n, lie
    inside it (the library refuses negative ones itself).  Returns (device, shape, first, stride, n), the three as ints."""
    if not isinstance(rec, torch.Tensor) or (rec.dim() < 1 if rank is None else rec.dim() != rank):
        raise TypeError(f"rec: expected a torch.Tensor {what}")
    device = rec.device
    if device.type != "cuda":
        raise ValueError(f"rec: expected a tensor on a HIP device, got {device}")
    _check_tensor(rec, rec.shape, device, "rec")
    first, stride, n = int(first), int(stride), int(n)
    if n > 0 and first >= 0 and stride >= 1 and first + (n - 1) * stride >= rec.shape[0]:
        raise ValueError(f"{holds} {rec.shape[0]} records, the last one asked for is {first + (n - 1) * stride}")
    return device, tuple(int(d) for d in rec.shape), first, stride, n


def _workspace_bytes(fn, *args) -> int:
    """The figure of one of the library's ``mcpc_*_workspace_bytes``; a negative one is its error code."""
    need = fn(*args)
    if need < 0:
        L.check(need)
    return need


def _check_workspace(workspace, device, need, align, asks):
    """A caller's workspace (None: one is allocated): a contiguous tensor on ``device``, ``align``-byte aligned, of at least ``need``
    bytes, the figure the function named ``asks`` gave.  Returns (workspace, its bytes)."""
    if workspace is None:
        workspace = torch.empty(max(need, align), dtype=torch.uint8, device=device)
    if not isinstance(workspace, torch.Tensor):
        raise TypeError(f"workspace: expected a torch.Tensor, got {type(workspace)}")
    if workspace.device != device:
        raise ValueError(f"workspace: expected device {device}, got {workspace.device}")
    if not workspace.is_contiguous():
        raise ValueError("workspace: tensor must be contiguous")
    if workspace.data_ptr() % align:
        raise ValueError(f"workspace: must be {align}-byte aligned")
    ws_bytes = workspace.numel() * workspace.element_size()
    if ws_bytes < need:
        raise ValueError(f"workspace: {ws_bytes} bytes, {asks} asks for {need}")
    return workspace, ws_bytes


def _current_stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


@dataclass
class RunResult:
    energies: Optional[torch.Tensor] = None      # float64 [rows, ENERGY_COLS]: loss, E_1..E_L, overall
    rec_x: List[torch.Tensor] = field(default_factory=list)
    rec_out: Optional[torch.Tensor] = None
    xgrad: List[torch.Tensor] = field(default_factory=list)


class Engine:
    """One MCPC engine = one network shape + one shard of chains on one GPU."""

    def __init__(self, sizes: Sequence[int], acts: Sequence[int], n_in: int, n_out: int, batch: int,
                 device=None, ecoef: Optional[Sequence[float]] = None, spill_budget_bytes: int = 0,
                 tuning: Optional[str] = None):
        self._h = C.c_void_p()
        self._lib = L.load()
        if not torch.cuda.is_available():
            raise L.MCPCLibraryError("no HIP device visible: the MCPC engine has no CPU path")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.sizes = [int(s) for s in sizes]
        self.acts = [int(a) for a in acts]
        self.ecoef = [1.0] * len(self.sizes) if ecoef is None else [float(c) for c in ecoef]
        self.n_in, self.n_out, self.batch = int(n_in), int(n_out), int(batch)
        self.L = len(self.sizes)
        if not (1 <= self.L <= L.MAX_LATENT):
            raise ValueError(f"1..{L.MAX_LATENT} latent layers supported, got {self.L}")
        d = L.NetDesc()
        d.abi_version = L.ABI_VERSION
        d.n_latent, d.n_in, d.n_out, d.batch = self.L, self.n_in, self.n_out, self.batch
        d.device = self.device.index
        d.spill_budget_bytes = int(spill_budget_bytes)
        # developer overrides of the schedule heuristics ("ws=0,no_overlap=1", see include/mcpc.h).  The library reads no
        # environment; this harness-side variable lets the test-suite pin every kernel variant through the facade too.
        self.tuning = tuning if tuning is not None else os.environ.get("MCPC_TUNING")
        d.tuning = self.tuning.encode() if self.tuning else None
        for i in range(self.L):
            d.sizes[i], d.acts[i], d.ecoef[i] = self.sizes[i], self.acts[i], self.ecoef[i]
        L.check(self._lib.mcpc_create(C.byref(d), C.byref(self._h)))
        self._keep = {}          # borrowed tensors the library holds pointers to
        self.n_lin = self.L + (1 if self.n_out > 0 else 0)
        self.step_counter = 0    # Philox step offset, advances across runs
        # what a facade that caches engines (PCTrainer) notes on them: a signature of the parameters it bound, which every
        # bind_params forgets (None: whoever comes next binds afresh), and why the engine runs on the layer-wise kernels, if it does
        self.bound_sig = None
        self.wide_reason = None

    # ---- lifetime ------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.mcpc_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return _current_stream(self.device)

    def lin_shape(self, j):
        n_in = self.n_in if j == 0 else self.sizes[j - 1]
        n_out = self.sizes[j] if j < self.L else self.n_out
        return n_out, n_in

    # ---- binding -------------------------------------------------------------------------------
    def bind_params(self, weights: Sequence[torch.Tensor], biases: Sequence[Optional[torch.Tensor]]):
        if len(weights) != self.n_lin or len(biases) != self.n_lin:
            raise ValueError(f"expected {self.n_lin} Linear layers, got {len(weights)}")
        for j, (W, b) in enumerate(zip(weights, biases)):
            n_out, n_in = self.lin_shape(j)
            _check_tensor(W, (n_out, n_in), self.device, f"weight[{j}]")
            if b is not None:
                _check_tensor(b, (n_out,), self.device, f"bias[{j}]")
            L.check(self._lib.mcpc_bind_params(self._h, j, _ptr(W), _ptr(b)))
        self._keep["W"], self._keep["b"] = list(weights), list(biases)
        self.bound_sig = None
        self.params_changed()

    def bound_params(self):
        """``(weights, biases)`` as the last ``bind_params`` took them: lists of the bound tensors, a bias None where there is none."""
        return list(self._keep["W"]), list(self._keep["b"])

    def params_changed(self):
        L.check(self._lib.mcpc_params_changed(self._h, self._stream()))

    def bind_inputs(self, inputs: Optional[torch.Tensor]):
        if inputs is not None:
            _check_tensor(inputs, (self.batch, self.n_in), self.device, "inputs")
        self._keep["inputs"] = inputs
        L.check(self._lib.mcpc_bind_inputs(self._h, _ptr(inputs), self._stream()))

    def bind_target(self, target: torch.Tensor):
        _check_tensor(target, (self.batch, self.n_out), self.device, "target")
        L.check(self._lib.mcpc_bind_target(self._h, _ptr(target), self._stream()))

    def _ptr_array(self, tensors, names):
        arr = (C.c_void_p * self.L)()
        for l, t in enumerate(tensors):
            _check_tensor(t, (self.batch, self.sizes[l]), self.device, f"{names}[{l}]")
            arr[l] = t.data_ptr()
        return arr

    def load_state(self, xs: Sequence[torch.Tensor]):
        L.check(self._lib.mcpc_load_state(self._h, self._ptr_array(xs, "x"), self._stream()))

    def store_state(self, xs: Sequence[torch.Tensor]):
        L.check(self._lib.mcpc_store_state(self._h, self._ptr_array(xs, "x"), self._stream()))

    def store_adam_state(self, ms: Sequence[torch.Tensor], vs: Sequence[torch.Tensor]):
        L.check(self._lib.mcpc_store_adam_state(self._h, self._ptr_array(ms, "exp_avg"), self._ptr_array(vs, "exp_avg_sq"),
                                                self._stream()))

    # ---- the hot loop ----------------------------------------------------------------------------
    def run(self, T: int, t_begin: int = 0, n_steps: Optional[int] = None, *,
            loss_kind=L.LOSS_NONE, loss_var=1.0, mask_start=0,
            xopt=L.XOPT_SGD, lr=0.1, betas=(0.9, 0.999), eps=1e-8, adam_step0=0,
            update_x=True, noise_mode=L.NOISE_NONE, noise_var=2.0, seed=0, step_base=None, chain_base=0,
            ext_noise: Optional[Sequence[torch.Tensor]] = None,
            acc_begin=0, acc_end=0, acc_reset=True,
            energy_mode=L.ENERGY_NONE, energies_out: Optional[torch.Tensor] = None,
            rec_begin=0, rec_stride=1, rec_count=0, rec_x=False, rec_out=False,
            rec_x_bufs: Optional[Sequence[Optional[torch.Tensor]]] = None,
            rec_out_buf: Optional[torch.Tensor] = None) -> RunResult:
        """``rec_x``: bool, or one bool per latent layer (record only those layers).  ``rec_x_bufs`` / ``rec_out_buf``:
        caller-owned record buffers ``[>= rec_count][batch][n]`` to write into (a ring that is drained to host memory while
        the next slice of the call runs) instead of fresh allocations."""
        n_steps = T - t_begin if n_steps is None else n_steps
        r = L.RunDesc()
        r.T, r.t_begin, r.n_steps = T, t_begin, n_steps
        r.loss_kind, r.loss_var, r.mask_start = loss_kind, loss_var, mask_start
        r.xopt_kind, r.lr = xopt, lr
        r.beta1, r.beta2, r.eps, r.adam_step0 = betas[0], betas[1], eps, adam_step0
        r.update_x = 1 if update_x else 0
        r.noise_mode, r.noise_var = noise_mode, noise_var
        r.seed = seed & 0xFFFFFFFFFFFFFFFF
        r.step_base = self.step_counter if step_base is None else step_base
        r.chain_base = chain_base
        res = RunResult()
        keep = []
        if noise_mode == L.NOISE_EXTERNAL:
            if ext_noise is None or len(ext_noise) != self.L:
                raise ValueError("NOISE_EXTERNAL needs one tensor per latent layer")
            for l, t in enumerate(ext_noise):
                _check_tensor(t, (n_steps, self.batch, self.sizes[l]), self.device, f"ext_noise[{l}]")
                r.ext_noise[l] = t.data_ptr()
                keep.append(t)
        r.acc_begin, r.acc_end, r.acc_reset = acc_begin, acc_end, 1 if acc_reset else 0
        r.energy_mode = energy_mode
        if energy_mode != L.ENERGY_NONE:
            rows = T if energy_mode == L.ENERGY_ALL else 1
            if energies_out is None:
                res.energies = torch.zeros(rows, L.ENERGY_COLS, dtype=torch.float64, device=self.device)
            else:
                _check_tensor(energies_out, (rows, L.ENERGY_COLS), self.device, "energies_out", torch.float64)
                res.energies = energies_out
            r.energies_out = res.energies.data_ptr()
        r.rec_begin, r.rec_stride, r.rec_count = rec_begin, rec_stride, rec_count
        if rec_count > 0:
            want = [bool(rec_x)] * self.L if isinstance(rec_x, bool) else [bool(v) for v in rec_x]
            for l in range(self.L):
                if want[l]:
                    if rec_x_bufs is not None and rec_x_bufs[l] is not None:
                        t = rec_x_bufs[l][:rec_count]
                        _check_tensor(t, (rec_count, self.batch, self.sizes[l]), self.device, f"rec_x_bufs[{l}]")
                    else:
                        t = torch.empty(rec_count, self.batch, self.sizes[l], dtype=torch.float32, device=self.device)
                    res.rec_x.append(t)
                    r.rec_x[l] = t.data_ptr()
                else:
                    res.rec_x.append(None)
            if rec_out and self.n_out > 0:
                if rec_out_buf is not None:
                    res.rec_out = rec_out_buf[:rec_count]
                    _check_tensor(res.rec_out, (rec_count, self.batch, self.n_out), self.device, "rec_out_buf")
                else:
                    res.rec_out = torch.empty(rec_count, self.batch, self.n_out, dtype=torch.float32, device=self.device)
                r.rec_out = res.rec_out.data_ptr()
        if not update_x:
            for l in range(self.L):
                t = torch.empty(self.batch, self.sizes[l], dtype=torch.float32, device=self.device)
                res.xgrad.append(t)
                r.xgrad[l] = t.data_ptr()
        L.check(self._lib.mcpc_run(self._h, C.byref(r), self._stream()))
        if step_base is None and update_x:
            self.step_counter += n_steps
        self._keep["run"] = keep
        return res

    # ---- per-chain energies ------------------------------------------------------------------------
    def chain_energies(self, inputs: Optional[torch.Tensor], x_rec: Sequence[torch.Tensor], *, loss_kind=L.LOSS_NONE, loss_var=1.0,
                       mask_start=0, out: Optional[torch.Tensor] = None, max_rows: int = 0) -> torch.Tensor:
        """Loss, layer energies and overall of every chain at every recorded step (include/mcpc.h: mcpc_chain_energies).

        ``x_rec[l]``: contiguous fp32 ``[n_rec, batch, n_l]`` as a run records it, or ``[batch, n_l]`` for one state.  ``inputs``:
        ``[batch, n_in]`` or None (zeros).  The target is the one bound with ``bind_target``.  Returns (or fills ``out``) fp64
        ``[n_rec, batch, ENERGY_COLS]``: column 0 the loss, 1..L the layer energies, the last one overall.  ``max_rows``: rows per
        scratch chunk (0 = the library's default); the result does not depend on it.  On the current torch stream."""
        if len(x_rec) != self.L:
            raise ValueError(f"x_rec: expected one tensor per latent layer ({self.L}), got {len(x_rec)}")
        if inputs is not None:
            _check_tensor(inputs, (self.batch, self.n_in), self.device, "inputs")
        n_rec = 1 if x_rec[0].dim() == 2 else int(x_rec[0].shape[0])
        arr = (C.c_void_p * self.L)()
        for l, t in enumerate(x_rec):
            shape = (self.batch, self.sizes[l]) if t.dim() == 2 else (n_rec, self.batch, self.sizes[l])
            _check_tensor(t, shape, self.device, f"x_rec[{l}]")
            arr[l] = t.data_ptr()
        if out is None:
            out = torch.empty(n_rec, self.batch, L.ENERGY_COLS, dtype=torch.float64, device=self.device)
        else:
            _check_tensor(out, (n_rec, self.batch, L.ENERGY_COLS), self.device, "out", torch.float64)
        L.check(self._lib.mcpc_chain_energies(self._h, _ptr(inputs), arr, n_rec, loss_kind, loss_var, mask_start, _ptr(out),
                                              int(max_rows), self._stream()))
        return out

    def prediction_errors(self, inputs: Optional[torch.Tensor], x_rec: Sequence[Optional[torch.Tensor]], *, layers=None, quantity="error",
                          outputs=None, loss_kind=L.LOSS_NONE, loss_var=1.0, mask_start=0, out: Optional[dict] = None,
                          max_rows: int = 0) -> dict:
        """Prediction errors ``x_l - mu_l`` and/or predictions ``mu_l`` of recorded states, per unit, as derived records (include/mcpc.h:
        mcpc_prediction_errors).

        ``x_rec`` / ``inputs`` / ``max_rows`` as in ``chain_energies``; an entry of ``x_rec`` may be None for a layer the evaluation
        does not read (it reads a requested layer and the one below it; the last layer for the read-out).  ``layers``: latent layer
        indices (None = all); ``quantity``: "error", "prediction" or "both"; ``outputs``: None, "error" (the read-out error the step
        kernels propagate, under ``loss_kind`` / ``loss_var`` / ``mask_start`` and the bound target), "prediction" (the logits) or
        "both".  Returns (or fills the tensors of ``out``, a dict by the same names) contiguous fp32 ``[n_rec, batch, n_l]`` tensors by
        name: "e<l>" / "mu<l>", "eout" / "out" -- the layout of a record, so ``moments_accumulate``, ``cov_accumulate``,
        ``hist_accumulate``, ``acov_accumulate`` and ``roll_accumulate`` take them as they take one.  On the current torch stream."""
        if len(x_rec) != self.L:
            raise ValueError(f"x_rec: expected one entry per latent layer ({self.L}), got {len(x_rec)}")
        if quantity not in ("error", "prediction", "both"):
            raise ValueError(f"quantity={quantity!r}, expected 'error', 'prediction' or 'both'")
        if outputs not in (None, "error", "prediction", "both"):
            raise ValueError(f"outputs={outputs!r}, expected None, 'error', 'prediction' or 'both'")
        layers = tuple(range(self.L)) if layers is None else tuple(sorted(set(int(l) for l in layers)))
        for l in layers:
            if not 0 <= l < self.L:
                raise ValueError(f"layer index {l} out of range 0..{self.L - 1}")
        if inputs is not None:
            _check_tensor(inputs, (self.batch, self.n_in), self.device, "inputs")
        given = [t for t in x_rec if t is not None]
        if not given:
            raise ValueError("x_rec: every entry is None")
        n_rec = 1 if given[0].dim() == 2 else int(given[0].shape[0])
        arr = (C.c_void_p * self.L)()
        for l, t in enumerate(x_rec):
            if t is None:
                continue
            shape = (self.batch, self.sizes[l]) if t.dim() == 2 else (n_rec, self.batch, self.sizes[l])
            _check_tensor(t, shape, self.device, f"x_rec[{l}]")
            arr[l] = t.data_ptr()
        res = {}

        def dest(name, n):
            if out is not None and name in out:
                _check_tensor(out[name], (n_rec, self.batch, n), self.device, f"out[{name!r}]")
                res[name] = out[name]
            else:
                res[name] = torch.empty(n_rec, self.batch, n, dtype=torch.float32, device=self.device)
            return res[name].data_ptr()
        err = (C.c_void_p * self.L)()
        pred = (C.c_void_p * self.L)()
        for l in layers:
            if quantity in ("error", "both"):
                err[l] = dest(f"e{l}", self.sizes[l])
            if quantity in ("prediction", "both"):
                pred[l] = dest(f"mu{l}", self.sizes[l])
        err_out = dest("eout", self.n_out) if outputs in ("error", "both") else None
        pred_out = dest("out", self.n_out) if outputs in ("prediction", "both") else None
        L.check(self._lib.mcpc_prediction_errors(self._h, _ptr(inputs), arr, n_rec, loss_kind, loss_var, mask_start, err, pred, err_out,
                                                 pred_out, int(max_rows), self._stream()))
        return res

    # ---- gradients of handed-over states --------------------------------------------------------------
    def state_gradients(self, inputs: Optional[torch.Tensor], x: Sequence[torch.Tensor], *, loss_kind=L.LOSS_NONE, loss_var=1.0,
                        mask_start=0, energies: bool = False, out: Optional[Sequence[torch.Tensor]] = None,
                        energies_out: Optional[torch.Tensor] = None, max_rows: int = 0):
        """``dF/dx_l`` of handed-over states and, when asked, their energies, in one evaluator call (include/mcpc.h:
        mcpc_state_gradients).  The engine's own state, moments, Philox position and records are not touched.

        ``x[l]``: contiguous fp32 ``[n_rec, batch, n_l]``, or ``[batch, n_l]`` for one state; ``inputs``, the target, the loss arguments
        and ``max_rows`` as in ``chain_energies``.  Returns ``(grads, table)``: ``grads[l]`` fp32 ``[n_rec, batch, n_l]`` (the tensors of
        ``out`` where given), bitwise what ``run(1, update_x=False).xgrad`` gives on the layer-wise kernels after ``load_state``; ``table``
        fp64 ``[n_rec, batch, ENERGY_COLS]`` bitwise ``chain_energies`` of the same rows (``energies_out`` where given), or None
        unless ``energies`` (an ``energies_out`` asks for them too).  On the current torch stream."""
        if len(x) != self.L:
            raise ValueError(f"x: expected one tensor per latent layer ({self.L}), got {len(x)}")
        if inputs is not None:
            _check_tensor(inputs, (self.batch, self.n_in), self.device, "inputs")
        n_rec = 1 if x[0].dim() == 2 else int(x[0].shape[0])
        xs = (C.c_void_p * self.L)()
        for l, t in enumerate(x):
            shape = (self.batch, self.sizes[l]) if t.dim() == 2 else (n_rec, self.batch, self.sizes[l])
            _check_tensor(t, shape, self.device, f"x[{l}]")
            xs[l] = t.data_ptr()
        if out is not None and len(out) != self.L:
            raise ValueError(f"out: expected one tensor per latent layer ({self.L}), got {len(out)}")
        gs = (C.c_void_p * self.L)()
        grads = []
        for l in range(self.L):
            if out is None:
                g = torch.empty(n_rec, self.batch, self.sizes[l], dtype=torch.float32, device=self.device)
            else:
                g = out[l]
                _check_tensor(g, (n_rec, self.batch, self.sizes[l]), self.device, f"out[{l}]")
            grads.append(g)
            gs[l] = g.data_ptr()
        table = None
        if energies_out is not None:
            _check_tensor(energies_out, (n_rec, self.batch, L.ENERGY_COLS), self.device, "energies_out", torch.float64)
            table = energies_out
        elif energies:
            table = torch.empty(n_rec, self.batch, L.ENERGY_COLS, dtype=torch.float64, device=self.device)
        d = L.GradientDesc()
        d.inputs = None if inputs is None else inputs.data_ptr()
        d.x, d.grad = xs, gs
        d.n_rec, d.loss_kind, d.loss_var, d.mask_start = n_rec, loss_kind, loss_var, mask_start
        d.energies = None if table is None else table.data_ptr()
        d.max_rows = int(max_rows)
        d.stream = self._stream()
        L.check(self._lib.mcpc_state_gradients(self._h, C.byref(d)))
        return grads, table

    # ---- ancestral samples ---------------------------------------------------------------------------
    def sample_prior(self, n: int, seed: int, step: int = 0, sample_base: int = 0, inputs: Optional[torch.Tensor] = None, loss=None,
                     var=None, readout="hidden", latents=False, out: Optional[torch.Tensor] = None, max_rows: int = 0):
        """``n`` ancestral samples of the generative model: ``x_1 ~ N(mu_1, 1/c_1)``, ``x_2 ~ N(mu_2(x_1), 1/c_2)``, ..., the read-out
        (include/mcpc.h: mcpc_sample_prior).  Sample ``i`` has the global id ``sample_base + i``; its values depend on ``(seed, step,
        id)``, the bound weights and its row of ``inputs`` (``[n, n_in]``, None = zeros) alone -- not on ``n``, ``max_rows`` or the
        engine's batch.  ``readout``: "hidden" (logits / means), "mean" (sigmoid for ``loss="bernoulli"``), "draw" (0/1 for
        "bernoulli"; mean + sqrt(``var``) * normal for "gaussian"), or None (no read-out).  ``latents``: False, True (every layer) or the
        layer indices to return.  Returns ``(out or None, [x_l or None])``, contiguous fp32 ``[n, width]`` on the engine's device -- the
        layout of a record with ``B = n``.  ``out``: a tensor to fill with the read-out.  The normals are ``philox_normals(seed, step,
        layer, sample_base, n, n_l, device)``.  On the current torch stream."""
        n, loss_kind, loss_var, code, layers, want_out = check_sample_prior(self.L, self.n_out, n, sample_base, loss, var, readout, latents,
                                                                            max_rows)
        if inputs is not None:
            _check_tensor(inputs, (n, self.n_in), self.device, "inputs")
        if not want_out:
            if out is not None:
                raise ValueError("out: given with readout=None")
        elif out is None:
            out = torch.empty(n, self.n_out, dtype=torch.float32, device=self.device)
        else:
            _check_tensor(out, (n, self.n_out), self.device, "out")
        xs = [None] * self.L
        arr = (C.c_void_p * self.L)()
        for l in layers:
            xs[l] = torch.empty(n, self.sizes[l], dtype=torch.float32, device=self.device)
            arr[l] = xs[l].data_ptr()
        L.check(self._lib.mcpc_sample_prior(self._h, _ptr(inputs), n, int(seed), int(step), int(sample_base), loss_kind, loss_var, code, arr,
                                            _ptr(out), int(max_rows), self._stream()))
        return out, xs

    # ---- parameter gradients ---------------------------------------------------------------------
    def read_param_grads(self, j: int, dW: torch.Tensor, db: Optional[torch.Tensor], scale=1.0, accumulate=False):
        n_out, n_in = self.lin_shape(j)
        _check_tensor(dW, (n_out, n_in), self.device, "dW")
        if db is not None:
            _check_tensor(db, (n_out,), self.device, "db")
        L.check(self._lib.mcpc_read_param_grads(self._h, j, _ptr(dW), _ptr(db), scale, 1 if accumulate else 0, self._stream()))

    def param_count(self) -> int:
        return int(self._lib.mcpc_param_count(self._h))

    def read_param_grads_flat(self, scale=1.0, tail=0) -> torch.Tensor:
        """The flat gradient bucket (W0, b0, W1, b1, ...) scaled by `scale`; `tail` extra floats behind it (uninitialised: the caller's
        own words that travel with the bucket through its one all-reduce)."""
        n = self.param_count()
        flat = torch.empty(n + tail, dtype=torch.float32, device=self.device)
        L.check(self._lib.mcpc_read_param_grads_flat(self._h, _ptr(flat), n, scale, self._stream()))
        return flat

    # ---- the library's own collective (hosts that are not on torch.distributed; include/mcpc.h "multi-GPU") ------
    @staticmethod
    def comm_unique_id() -> bytes:
        """Rank 0: the RCCL unique id (128 bytes) every rank passes to comm_init."""
        buf = C.create_string_buffer(L.COMM_ID_BYTES)
        L.check(L.load().mcpc_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, n_ranks: int, rank: int, unique_id: bytes):
        if len(unique_id) != L.COMM_ID_BYTES:
            raise ValueError(f"unique id of {len(unique_id)} bytes, expected {L.COMM_ID_BYTES}")
        L.check(self._lib.mcpc_comm_init(self._h, n_ranks, rank, C.create_string_buffer(unique_id, L.COMM_ID_BYTES)))

    def allreduce_grads(self, flat: torch.Tensor):
        """In-place sum of the gradient bucket over the shards (ncclAllReduce on the caller's stream)."""
        if flat.dtype != torch.float32 or not flat.is_contiguous() or flat.device != self.device:
            raise ValueError("the bucket must be a contiguous float32 tensor on the engine's device")
        L.check(self._lib.mcpc_allreduce_grads(self._h, _ptr(flat), flat.numel(), self._stream()))
        return flat

    def comm_destroy(self):
        L.check(self._lib.mcpc_comm_destroy(self._h))

    def sync_check(self):
        """Synchronise the stream and raise MCPCError if a kernel reported a device-side fault."""
        L.check(self._lib.mcpc_sync_check(self._h, self._stream()))

    # ---- introspection -----------------------------------------------------------------------------
    def query(self):
        a, b, c, d = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        L.check(self._lib.mcpc_query(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        name = self._lib.mcpc_step_kernel_name(self._h).decode()
        return dict(lds_bytes=a.value, chains_per_wg=b.value, n_workgroups=c.value, spill_slots=d.value, step_kernel=name)

    def last_step_kernel(self) -> str:
        """The step kernel the last run launched (include/mcpc.h: mcpc_last_step_kernel_name; query()["step_kernel"] is the preference)."""
        return self._lib.mcpc_last_step_kernel_name(self._h).decode()

    def last_flush_plan(self, j: int) -> str:
        """What the last Hebbian flush of Linear j >= 1 launched, e.g. 'heb7<17,2>x1+heb7<16,2>x2 ksplit=12 rps=1536 tm' (mcpc_last_flush_plan)."""
        return self._lib.mcpc_last_flush_plan(self._h, j).decode()

    def set_profiling(self, enable: bool):
        L.check(self._lib.mcpc_set_profiling(self._h, 1 if enable else 0))

    def last_step_kernel_ms(self):
        ms, n, s = C.c_float(), C.c_int32(), C.c_int64()
        L.check(self._lib.mcpc_last_step_kernel_ms(self._h, C.byref(ms), C.byref(n), C.byref(s)))
        return ms.value, n.value, s.value

    def last_shader_clock_ghz(self):
        g = C.c_float()
        L.check(self._lib.mcpc_last_shader_clock_ghz(self._h, C.byref(g)))
        return g.value


def check_sample_prior(n_latent, n_out, n, sample_base=0, loss=None, var=None, readout="hidden", latents=False, max_rows=0):
    """The argument checks of ``Engine.sample_prior`` for a network of ``n_latent`` layers and ``n_out`` outputs; no device is needed.
    Returns (n, loss_kind, loss_var, readout code, the latent layers wanted, whether the read-out is)."""
    n, sample_base = int(n), int(sample_base)
    if n < 0:
        raise ValueError(f"n={n}, must not be negative")
    if sample_base < 0 or sample_base + n > 1 << 32:
        raise ValueError(f"sample_base={sample_base} with n={n}: sample ids are 32 bits (sample_base + n <= 2^32)")
    if int(max_rows) < 0:
        raise ValueError(f"max_rows={max_rows}, must not be negative (0 = default)")
    if readout not in _SAMPLE_READOUTS:
        raise ValueError(f"readout={readout!r}, expected 'hidden', 'mean', 'draw' or None")
    if loss not in (None, "bernoulli", "gaussian"):
        raise ValueError(f"loss: expected None, 'bernoulli' or 'gaussian', got {loss!r}")
    if latents is True:
        layers = tuple(range(n_latent))
    elif latents is False or latents is None:
        layers = ()
    else:
        layers = tuple(sorted(set(int(l) for l in latents)))
    for l in layers:
        if not 0 <= l < n_latent:
            raise ValueError(f"layer index {l} out of range 0..{n_latent - 1}")
    want_out = readout is not None and n_out > 0           # (a network that ends in a PCLayer has no read-out to return)
    if not want_out and not layers:
        raise ValueError("nothing is asked for: no read-out and no latent layer")
    if want_out and readout != "hidden" and loss is None:
        raise ValueError(f"readout={readout!r} needs a loss ('bernoulli' or 'gaussian')")
    if loss == "gaussian" and want_out and readout == "draw":
        if var is None or not float(var) > 0.0:
            raise ValueError(f"var: a draw of the Gaussian read-out needs a positive variance, got {var!r}")
    loss_var = float(var) if var is not None else 1.0
    return n, _LOGLIK_LOSSES.get(loss, L.LOSS_NONE), loss_var, _SAMPLE_READOUTS[readout], layers, want_out


def debug_poison_lds(device, word=0x7FA00000):
    """Diagnostic (tests only): fill the LDS of every compute unit of `device` with a 32-bit pattern (default: a signalling NaN)."""
    lib = L.load()
    device = torch.device(device)
    stream = _current_stream(device)
    L.check(lib.mcpc_debug_poison_lds(device.index or 0, word, stream))


def philox_normals(seed, step, layer, chain_base, batch, n_units, device, raw=False) -> torch.Tensor:
    """The device generator's normals (or raw u32 bit patterns viewed as int32) for one layer/step."""
    lib = L.load()
    device = torch.device(device)
    out = torch.empty(batch, n_units, dtype=torch.float32, device=device)
    stream = _current_stream(device)
    L.check(lib.mcpc_philox_normals(device.index or 0, seed, step, layer, chain_base, batch, n_units,
                                    _ptr(out), 1 if raw else 0, stream))
    return out.view(torch.int32) if raw else out


def box_muller(a, b):
    """``(z0, z1)``: the step kernels' Box-Muller transform of the bit pairs ``(a[i], b[i])`` (include/mcpc.h: mcpc_box_muller), the
    transform on bits the caller chooses instead of Philox outputs.  ``a``, ``b``: contiguous int32 or uint32 device tensors of one
    dimension and equal length (int32 is read as the same 32 bits: what ``philox_normals(raw=True)`` returns).  The radius comes from
    ``a >> 8``, the angle from ``b >> 8``.  On the current torch stream."""
    lib = L.load()
    for t, name in ((a, "a"), (b, "b")):
        if not isinstance(t, torch.Tensor) or t.dim() != 1:
            raise TypeError(f"{name}: expected a torch.Tensor [n]")
        if t.dtype not in (torch.int32, torch.uint32):
            raise TypeError(f"{name}: expected torch.int32 or torch.uint32, got {t.dtype}")
    device = a.device
    if device.type != "cuda":
        raise ValueError(f"a: expected a tensor on a HIP device, got {device}")
    n = int(a.shape[0])
    _check_tensor(a, (n,), device, "a", dtype=a.dtype)
    _check_tensor(b, (n,), device, "b", dtype=b.dtype)
    z0 = torch.empty(n, dtype=torch.float32, device=device)
    z1 = torch.empty(n, dtype=torch.float32, device=device)
    if n == 0:                                     # an empty tensor has no address to hand over
        return z0, z1
    stream = _current_stream(device)
    L.check(lib.mcpc_box_muller(device.index or 0, _ptr(a), _ptr(b), n, _ptr(z0), _ptr(z1), stream))
    return z0, z1


_MOM_TRANSFORMS = {None: L.MOM_IDENTITY, "identity": L.MOM_IDENTITY, "sigmoid": L.MOM_SIGMOID,
                   L.MOM_IDENTITY: L.MOM_IDENTITY, L.MOM_SIGMOID: L.MOM_SIGMOID}


def _transform(t, what="transform", pair=False):
    """The library's code of the transform ``t`` of a reducer; ``pair``: ``t`` holds the two of hist2d_accumulate's axes, and both
    codes are returned.  Any other name is the reducers' ValueError."""
    names = tuple(t) if pair else (t,)
    if (pair and len(names) != 2) or any(x not in _MOM_TRANSFORMS for x in names):
        raise ValueError(f"{what}: expected {'two of ' if pair else ''}'identity' or 'sigmoid', got {names if pair else t!r}")
    codes = [_MOM_TRANSFORMS[x] for x in names]
    return codes if pair else codes[0]


def moments_accumulate(rec, first, stride, n, sum, sumsq=None, transform="identity", accumulate=True):
    """Add records ``rec[first + k * stride]``, k < n, and their squares to the fp64 accumulators ``sum`` / ``sumsq`` on the device
    (include/mcpc.h: mcpc_moments_accumulate), in ascending order of k, one thread per element: the sums are bitwise those of a
    sequential fp64 loop, however the records are chunked over calls.  ``rec``: contiguous fp32 ``[records, ...]`` as an engine run
    records it; ``sum`` / ``sumsq``: contiguous fp64 of ``rec[0].numel()`` elements (``sumsq`` may be None).  ``transform``:
    "identity", or "sigmoid" for the read-out's Bernoulli mean.  ``accumulate=False`` overwrites.  On the current torch stream."""
    lib = L.load()
    xf = _transform(transform)
    device, shape, first, stride, n = _record_window(rec, first, stride, n, rank=None, what="[records, ...]")
    row = 1
    for d in shape[1:]:
        row *= d
    for t, name in ((sum, "sum"), (sumsq, "sumsq")):
        if t is None and name == "sumsq":
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: expected a torch.Tensor, got {type(t)}")
        if t.numel() != row:
            raise ValueError(f"{name}: expected {row} elements (one per element of a record), got {t.numel()}")
        _check_tensor(t, t.shape, device, name, torch.float64)
    stream = _current_stream(device)
    L.check(lib.mcpc_moments_accumulate(device.index or 0, _ptr(rec), row, first, stride, n, xf,
                                        _ptr(sum), _ptr(sumsq), 1 if accumulate else 0, stream))


def cov_workspace_bytes(B, widths, pool=True) -> int:
    """Bytes of device workspace ``cov_accumulate`` needs for ``B`` chains and blocks of these widths (0 unless pooled)."""
    w = (C.c_int32 * len(widths))(*[int(x) for x in widths])
    return _workspace_bytes(L.load().mcpc_cov_workspace_bytes, int(B), w, len(widths), 1 if pool else 0)


def cov_accumulate(recs, first, stride, n, outer, transforms=None, pool=False, accumulate=True, workspace=None):
    """Add the outer products ``v v^T`` of records ``first + k * stride``, k < n, to the fp64 accumulator ``outer`` on the device
    (include/mcpc.h: mcpc_cov_accumulate; the fp64 MFMA).  ``recs``: a sequence of contiguous fp32 ``[records, B, w_j]`` buffers as an
    engine run records them; ``v`` is the concatenation of a chain's rows in that order, ``D = sum w_j``.  ``outer``: contiguous fp64
    ``[B, D, D]``, or ``[D, D]`` with ``pool=True`` (summed over the chains too).  ``transforms``: per block "identity" or "sigmoid"
    (None = all identity).  ``accumulate=False`` overwrites.  ``workspace`` (pooled only): a contiguous device tensor of at least
    ``cov_workspace_bytes(B, widths)`` bytes, 8-B aligned; None allocates one for this call.  Both triangles are written and bitwise
    equal; two runs give the same bits; chunking the records over calls differently does not (within the bound of DESIGN.md section
    4).  On the current torch stream."""
    lib = L.load()
    if isinstance(recs, torch.Tensor) or not len(recs):
        raise TypeError("recs: expected a non-empty sequence of torch.Tensor [records, B, width]")
    recs = list(recs)
    if len(recs) > L.MAX_LATENT + 1:
        raise ValueError(f"recs: {len(recs)} blocks, at most {L.MAX_LATENT + 1}")
    transforms = [None] * len(recs) if transforms is None else list(transforms)
    if len(transforms) != len(recs):
        raise ValueError(f"transforms: expected one per block ({len(recs)}), got {len(transforms)}")
    xf = (C.c_int32 * len(recs))(*[_transform(t, "transforms") for t in transforms])
    for j, r in enumerate(recs):
        if not isinstance(r, torch.Tensor) or r.dim() != 3:
            raise TypeError(f"recs[{j}]: expected a torch.Tensor [records, B, width]")
    device = recs[0].device
    if device.type != "cuda":
        raise ValueError(f"recs[0]: expected a tensor on a HIP device, got {device}")
    R, B = int(recs[0].shape[0]), int(recs[0].shape[1])
    for j, r in enumerate(recs):
        _check_tensor(r, (R, B, r.shape[2]), device, f"recs[{j}]")
    widths = [int(r.shape[2]) for r in recs]
    D = sum(widths)
    _, _, first, stride, n = _record_window(recs[0], first, stride, n, holds="recs hold")
    if not isinstance(outer, torch.Tensor):
        raise TypeError(f"outer: expected a torch.Tensor, got {type(outer)}")
    _check_tensor(outer, (D, D) if pool else (B, D, D), device, "outer", torch.float64)
    w = (C.c_int32 * len(recs))(*widths)
    need = _workspace_bytes(lib.mcpc_cov_workspace_bytes, B, w, len(recs), 1 if pool else 0)
    ws_bytes = 0
    if pool:
        workspace, ws_bytes = _check_workspace(workspace, device, need, 8, "cov_workspace_bytes")
    ptrs = (C.c_void_p * len(recs))(*[r.data_ptr() for r in recs])
    stream = _current_stream(device)
    L.check(lib.mcpc_cov_accumulate(device.index or 0, ptrs, w, xf, len(recs), B, first, stride, n, 1 if pool else 0, _ptr(outer),
                                    1 if accumulate else 0, _ptr(workspace) if pool else None, ws_bytes, stream))


def hist_accumulate(rec, first, stride, n, edges, counts, transform="identity", pool=False, accumulate=True):
    """Count records ``rec[first + k * stride]``, k < n, into the int64 histogram ``counts`` on the device (include/mcpc.h:
    mcpc_hist_accumulate).  ``rec``: contiguous fp32 ``[records, B, width]`` as an engine run records it.  ``edges``: 1-D fp32 CPU
    tensor or array of ``n_bins + 1`` finite, strictly ascending values (at most ``L.HIST_MAX_BINS`` bins).  ``counts``: contiguous int64
    ``[B, width, n_bins + 3]``, or ``[width, n_bins + 3]`` with ``pool=True`` (summed over the chains): the bins, then under, over, nan.
    A bin is decided by fp32 comparison against the edges alone (half-open, the last one closed), as ``np.histogram`` with explicit
    edges does.  ``transform``: "identity", or "sigmoid" for the read-out's Bernoulli mean.  ``accumulate=False`` overwrites.  Counts are
    integers: exact, however the records are chunked over calls.  On the current torch stream."""
    lib = L.load()
    xf = _transform(transform)
    device, (R, B, width), first, stride, n = _record_window(rec, first, stride, n)
    e = torch.as_tensor(edges)
    if e.device.type != "cpu" or e.dtype != torch.float32 or e.dim() != 1:
        raise TypeError("edges: expected a 1-D fp32 CPU tensor or array")
    e = e.contiguous()
    n_bins = e.numel() - 1
    if not 1 <= n_bins <= L.HIST_MAX_BINS:
        raise ValueError(f"edges: {e.numel()} values, expected 2..{L.HIST_MAX_BINS + 1} (1..{L.HIST_MAX_BINS} bins)")
    if not isinstance(counts, torch.Tensor):
        raise TypeError(f"counts: expected a torch.Tensor, got {type(counts)}")
    _check_tensor(counts, (width, n_bins + 3) if pool else (B, width, n_bins + 3), device, "counts", torch.int64)
    stream = _current_stream(device)
    L.check(lib.mcpc_hist_accumulate(device.index or 0, _ptr(rec), B, width, first, stride, n, xf,
                                     C.cast(e.data_ptr(), C.POINTER(C.c_float)), n_bins, 1 if pool else 0, _ptr(counts),
                                     1 if accumulate else 0, stream))


def acov_accumulate(rec, first, stride, n, max_lag, n_seen, lagged, sum, window, head, transform="identity"):
    """Add records ``rec[first + j * stride]``, j < n, as samples ``n_seen .. n_seen + n - 1`` of a stream to its lagged products on the
    device (include/mcpc.h: mcpc_acov_accumulate).  ``rec``: contiguous fp32 ``[records, B, width]`` as an engine run records it.  The
    caller owns the state, on the device of ``rec``: ``lagged`` fp64 ``[B, width, max_lag + 1]`` (per element and lag k the sum of
    g(s_j) g(s_{j-k})), ``sum`` fp64 ``[B, width]``, ``window`` and ``head`` fp32 ``[max_lag, B, width]`` (the last and the first
    ``max_lag`` samples; ``window`` carries the lags across calls).  ``max_lag``: 0..``L.ACOV_MAX_LAG``.  ``n_seen``: the samples the
    stream held before this call; 0 starts one (``lagged`` and ``sum`` are overwritten).  ``transform``: "identity", or "sigmoid" for the
    read-out's Bernoulli mean.  Every accumulator is bitwise a sequential fp64 loop over the stream, however it is chunked over calls.
    On the current torch stream."""
    lib = L.load()
    xf = _transform(transform)
    device, (R, B, width), first, stride, n = _record_window(rec, first, stride, n)
    max_lag, n_seen = int(max_lag), int(n_seen)
    if not 0 <= max_lag <= L.ACOV_MAX_LAG:
        raise ValueError(f"max_lag={max_lag}, expected 0..{L.ACOV_MAX_LAG}")
    _check_tensor(lagged, (B, width, max_lag + 1), device, "lagged", torch.float64)
    _check_tensor(sum, (B, width), device, "sum", torch.float64)
    _check_tensor(window, (max_lag, B, width), device, "window")
    _check_tensor(head, (max_lag, B, width), device, "head")
    stream = _current_stream(device)
    L.check(lib.mcpc_acov_accumulate(device.index or 0, _ptr(rec), B, width, first, stride, n, xf, max_lag,
                                     n_seen, _ptr(lagged), _ptr(sum), _ptr(window), _ptr(head), stream))


def roll_workspace_bytes(B, width, n) -> int:
    """Bytes of device workspace ``roll_accumulate`` needs for the pooled rows of a chunk of ``n`` samples of ``B`` chains x ``width``
    units (include/mcpc.h: mcpc_roll_workspace_bytes)."""
    return _workspace_bytes(L.load().mcpc_roll_workspace_bytes, int(B), int(width), int(n))


def roll_rows(n_seen, n, window, every=1) -> int:
    """Rows a chunk of ``n`` samples emits after ``n_seen`` samples of the stream: one per sample j >= window - 1 with
    (j - (window - 1)) % every == 0."""
    n_seen, n, window, every = int(n_seen), int(n), int(window), int(every)
    j = max(n_seen, window - 1)
    j += -(j - (window - 1)) % every
    return (n_seen + n - 1 - j) // every + 1 if j < n_seen + n else 0


def roll_accumulate(rec, first, stride, n, window, every, n_seen, s1, s2, hist, out_elem=None, out_pool=None, workspace=None,
                    transform="identity"):
    """Feed records ``rec[first + j * stride]``, j < n, as samples ``n_seen .. n_seen + n - 1`` of a stream to its rolling-window variance
    on the device (include/mcpc.h: mcpc_roll_accumulate).  ``rec``: contiguous fp32 ``[records, B, width]`` as an engine run records it.
    The caller owns the state, on the device of ``rec``: ``s1`` and ``s2`` fp64 ``[B, width]`` (the sums of g and g^2 over the current
    window), ``hist`` fp32 ``[window, B, width]`` (a circular buffer, sample j in row j mod window).  ``n_seen``: the samples the stream
    held before this call; 0 starts one.  Every sample j >= window - 1 with (j - (window - 1)) % every == 0 emits a row; the call's
    ``roll_rows(n_seen, n, window, every)`` rows are numbered from 0 in its outputs: ``out_elem`` fp64 ``[rows, B, width]``, the
    variance (ddof 1) of the window that ends at the row's sample, bitwise a sequential fp64 loop over the stream however it is
    chunked; ``out_pool`` fp64 ``[rows, 4]``, over the elements whose variance is finite the sums of its square root, of that squared,
    of the variance, and their count.  Either may be None, not both; both may hold more rows than the call emits.  ``workspace`` (with
    ``out_pool``): a contiguous device tensor of at least ``roll_workspace_bytes(B, width, n)`` bytes, 8-B aligned; None allocates one
    for this call.  ``transform``: "identity", or "sigmoid" for the read-out's Bernoulli mean.  Returns the rows emitted.  On the
    current torch stream."""
    lib = L.load()
    xf = _transform(transform)
    device, (R, B, width), first, stride, n = _record_window(rec, first, stride, n)
    window, every, n_seen = int(window), int(every), int(n_seen)
    if window < 2:
        raise ValueError(f"window={window}, expected at least 2")
    if every < 1:
        raise ValueError(f"every={every}, expected at least 1")
    _check_tensor(s1, (B, width), device, "s1", torch.float64)
    _check_tensor(s2, (B, width), device, "s2", torch.float64)
    _check_tensor(hist, (window, B, width), device, "hist")
    if out_elem is None and out_pool is None:
        raise ValueError("out_elem and out_pool are both None")
    rows = roll_rows(n_seen, n, window, every) if n >= 0 and n_seen >= 0 else 0
    if out_elem is not None:
        if not isinstance(out_elem, torch.Tensor) or out_elem.dim() != 3 or out_elem.shape[0] < rows:
            raise ValueError(f"out_elem: expected a torch.Tensor of at least {rows} rows [rows, {B}, {width}]")
        _check_tensor(out_elem, (out_elem.shape[0], B, width), device, "out_elem", torch.float64)
    if out_pool is not None:
        if not isinstance(out_pool, torch.Tensor) or out_pool.dim() != 2 or out_pool.shape[0] < rows:
            raise ValueError(f"out_pool: expected a torch.Tensor of at least {rows} rows [rows, 4]")
        _check_tensor(out_pool, (out_pool.shape[0], 4), device, "out_pool", torch.float64)
        need = roll_workspace_bytes(B, width, max(n, 0))
        workspace, _ = _check_workspace(workspace, device, need, 8, "roll_workspace_bytes")

    def out_ptr(t):
        # a tensor without rows has no address, and the library tells the outputs asked for by their pointers: s1's stands in (a call
        # that emits no row writes no output)
        return None if t is None else C.c_void_p(t.data_ptr() or s1.data_ptr())
    stream = _current_stream(device)
    L.check(lib.mcpc_roll_accumulate(device.index or 0, _ptr(rec), B, width, first, stride, n, xf, window, every,
                                     n_seen, _ptr(s1), _ptr(s2), _ptr(hist), out_ptr(out_elem), out_ptr(out_pool),
                                     _ptr(workspace) if out_pool is not None else None, stream))
    return rows


_PROBE_LINKS = {"identity": L.PROBE_IDENTITY, "sigmoid": L.PROBE_SIGMOID, "softmax": L.PROBE_SOFTMAX}


def probe_accumulate(rec, first, stride, n, W, bias, link, psum, psumsq, votes, entsum, accumulate=True):
    """Add the linear probe ``link(W r + bias)`` of records ``rec[first + j * stride]``, j < n, to per-chain sums on the device
    (include/mcpc.h: mcpc_probe_accumulate).  ``rec``: contiguous fp32 ``[records, B, width]`` as an engine run records it.  ``W``:
    contiguous fp32 ``[C, width]`` (the layout of ``nn.Linear.weight``), C in 1..``L.PROBE_MAX_CLASSES``; ``bias``: fp32 ``[C]`` or None
    for zeros; ``link``: "identity", "sigmoid" or "softmax".  ``psum`` and ``psumsq`` (may be None): fp64 ``[B, C]``, the sums of the
    link values and of their squares; ``votes``: int64 ``[B, C + 1]``, argmax counts of the logits (the lowest index on a tie) and, in
    column C, the samples with a NaN logit; ``entsum``: fp64 ``[B]``, the summed entropies of the samples' softmax (softmax only, else
    None).  Everything on the device of ``rec``.  ``accumulate=False`` overwrites.  One lane owns a (chain, class) and walks the samples
    in order: the result does not depend on how the records are chunked over calls.  On the current torch stream."""
    lib = L.load()
    if link not in _PROBE_LINKS:
        raise ValueError(f"link: expected 'identity', 'sigmoid' or 'softmax', got {link!r}")
    device, (R, B, width), first, stride, n = _record_window(rec, first, stride, n)
    if not isinstance(W, torch.Tensor) or W.dim() != 2:
        raise TypeError("W: expected a torch.Tensor [C, width]")
    n_classes = int(W.shape[0])
    if not 1 <= n_classes <= L.PROBE_MAX_CLASSES:
        raise ValueError(f"W: {n_classes} classes, expected 1..{L.PROBE_MAX_CLASSES}")
    _check_tensor(W, (n_classes, width), device, "W")
    if bias is not None:
        _check_tensor(bias, (n_classes,), device, "bias")
    _check_tensor(psum, (B, n_classes), device, "psum", torch.float64)
    if psumsq is not None:
        _check_tensor(psumsq, (B, n_classes), device, "psumsq", torch.float64)
    _check_tensor(votes, (B, n_classes + 1), device, "votes", torch.int64)
    if link == "softmax":
        _check_tensor(entsum, (B,), device, "entsum", torch.float64)
    elif entsum is not None:
        raise ValueError(f"entsum: the entropy is that of a softmax; expected None with link={link!r}")
    stream = _current_stream(device)
    L.check(lib.mcpc_probe_accumulate(device.index or 0, _ptr(rec), B, width, first, stride, n, _ptr(W), _ptr(bias), n_classes,
                                      _PROBE_LINKS[link], _ptr(psum), _ptr(psumsq), _ptr(votes), _ptr(entsum), 1 if accumulate else 0,
                                      stream))


def probe_records(rec, first, stride, n, W, bias, link, out=None):
    """The linear probe ``link(W r + bias)`` of records ``rec[first + j * stride]``, j < n, as a derived record (include/mcpc.h:
    mcpc_probe_records): fp32 ``[n, B, C]`` on the device of ``rec``, row j the link values of record ``first + j * stride``, bitwise
    what ``probe_accumulate`` adds for that sample.  ``rec``, ``W``, ``bias``, ``link`` as ``probe_accumulate`` takes them.  ``out``:
    a contiguous fp32 ``[n, B, C]`` tensor to fill, or None to allocate one.  The result has the layout of a record buffer: every
    stateless reducer takes it as ``rec``, and an identity-link probe on it projects the class probabilities.  On the current torch
    stream."""
    lib = L.load()
    if link not in _PROBE_LINKS:
        raise ValueError(f"link: expected 'identity', 'sigmoid' or 'softmax', got {link!r}")
    device, (R, B, width), first, stride, n = _record_window(rec, first, stride, n)
    if not isinstance(W, torch.Tensor) or W.dim() != 2:
        raise TypeError("W: expected a torch.Tensor [C, width]")
    n_classes = int(W.shape[0])
    if not 1 <= n_classes <= L.PROBE_MAX_CLASSES:
        raise ValueError(f"W: {n_classes} classes, expected 1..{L.PROBE_MAX_CLASSES}")
    _check_tensor(W, (n_classes, width), device, "W")
    if bias is not None:
        _check_tensor(bias, (n_classes,), device, "bias")
    if out is None:
        out = torch.empty(max(n, 0), B, n_classes, dtype=torch.float32, device=device)
    _check_tensor(out, (max(n, 0), B, n_classes), device, "out")
    if n == 0:                                     # an empty tensor has no address to hand over
        return out
    stream = _current_stream(device)
    L.check(lib.mcpc_probe_records(device.index or 0, _ptr(rec), B, width, first, stride, n, _ptr(W), _ptr(bias), n_classes,
                                   _PROBE_LINKS[link], _ptr(out), stream))
    return out


def _hist2d_edges(edges, name):
    e = torch.as_tensor(edges)
    if e.device.type != "cpu" or e.dtype != torch.float32 or e.dim() != 1:
        raise TypeError(f"{name}: expected a 1-D fp32 CPU tensor or array")
    e = e.contiguous()
    if not 1 <= e.numel() - 1 <= L.HIST2D_MAX_BINS:
        raise ValueError(f"{name}: {e.numel()} values, expected 2..{L.HIST2D_MAX_BINS + 1} (1..{L.HIST2D_MAX_BINS} bins)")
    return e


def hist2d_accumulate(rec_x, rec_y, first, stride, n, pairs, edges_x, edges_y, counts, transforms=("identity", "identity"), pool=False,
                      accumulate=True):
    """Count the pairs ``(rec_x[k][c][px], rec_y[k][c][py])`` of records ``k = first + j * stride``, j < n, into the int64 joint
    histograms ``counts`` on the device (include/mcpc.h: mcpc_hist2d_accumulate).  ``rec_x`` / ``rec_y``: contiguous fp32
    ``[records, B, width_x]`` / ``[records, B, width_y]`` of equally many records and chains; they may be the same tensor.  ``pairs``: a
    sequence of ``(px, py)`` column indices, any number (more than ``L.HIST2D_MAX_PAIRS`` are split over several library calls).
    ``edges_x`` / ``edges_y``: 1-D fp32 CPU tensors or arrays of ``nx + 1`` / ``ny + 1`` finite, strictly ascending values, at most
    ``L.HIST2D_MAX_BINS`` bins each and ``(nx + 3) * (ny + 3) <= L.HIST2D_MAX_CELLS``.  ``counts``: contiguous int64
    ``[B, pairs, nx + 3, ny + 3]``, or ``[pairs, nx + 3, ny + 3]`` with ``pool=True``: per axis the bins, then under, over, nan, each
    decided as ``hist_accumulate`` decides it.  ``transforms``: per axis "identity" or "sigmoid".  ``accumulate=False`` overwrites.
    Counts are integers: exact, however the records are chunked over calls and the pairs are ordered.  On the current torch stream."""
    lib = L.load()
    xf = _transform(transforms, "transforms", pair=True)
    device, (R, B, wx), first, stride, n = _record_window(rec_x, first, stride, n)
    if not isinstance(rec_y, torch.Tensor) or rec_y.dim() != 3:
        raise TypeError("rec_y: expected a torch.Tensor [records, B, width]")
    _check_tensor(rec_y, (R, B, rec_y.shape[2]), device, "rec_y")
    wy = int(rec_y.shape[2])
    pairs = [(int(a), int(b)) for a, b in pairs]
    if not pairs:
        raise ValueError("pairs: expected at least one (x column, y column)")
    for k, (a, b) in enumerate(pairs):
        if not (0 <= a < wx and 0 <= b < wy):
            raise ValueError(f"pairs[{k}] = {(a, b)}: outside the records' columns (0..{wx - 1}, 0..{wy - 1})")
    ex, ey = _hist2d_edges(edges_x, "edges_x"), _hist2d_edges(edges_y, "edges_y")
    nx, ny = ex.numel() - 1, ey.numel() - 1
    if (nx + 3) * (ny + 3) > L.HIST2D_MAX_CELLS:
        raise ValueError(f"edges: (nx + 3) * (ny + 3) = {(nx + 3) * (ny + 3)} cells, more than {L.HIST2D_MAX_CELLS}")
    if not isinstance(counts, torch.Tensor):
        raise TypeError(f"counts: expected a torch.Tensor, got {type(counts)}")
    grid = (len(pairs), nx + 3, ny + 3)
    _check_tensor(counts, grid if pool else (B,) + grid, device, "counts", torch.int64)
    stream = _current_stream(device)
    fptr = C.POINTER(C.c_float)

    def call(some, into):
        flat = (C.c_int32 * (2 * len(some)))(*[v for p in some for v in p])
        L.check(lib.mcpc_hist2d_accumulate(device.index or 0, _ptr(rec_x), wx, _ptr(rec_y), wy, B, first, stride, n, xf[0], xf[1], flat,
                                           len(some), C.cast(ex.data_ptr(), fptr), nx, C.cast(ey.data_ptr(), fptr), ny,
                                           1 if pool else 0, _ptr(into), 1 if accumulate else 0, stream))
    if len(pairs) <= L.HIST2D_MAX_PAIRS:
        call(pairs, counts)
        return
    # more pairs than a launch carries: a call per group of them; pooled, a group's grids are contiguous in counts, per chain they are
    # not, and the group counts into a buffer of its own that is added (or copied) into its columns
    for p0 in range(0, len(pairs), L.HIST2D_MAX_PAIRS):
        some = pairs[p0:p0 + L.HIST2D_MAX_PAIRS]
        if pool:
            call(some, counts[p0:p0 + len(some)])
        else:
            part = counts[:, p0:p0 + len(some)].contiguous()
            call(some, part)
            counts[:, p0:p0 + len(some)] = part


def knn_workspace_bytes(nq, nr, d, k) -> int:
    """Bytes of device workspace ``knn_accumulate`` needs for ``nq`` queries into ``nr`` reference rows of ``d`` coordinates, ``k`` kept."""
    return _workspace_bytes(L.load().mcpc_knn_workspace_bytes, int(nq), int(nr), int(d), int(k))


def knn_accumulate(q, ref, k, best, accumulate=False, workspace=None):
    """The ``k`` smallest squared distances from every row of ``q`` into the rows of ``ref``, on the device (include/mcpc.h:
    mcpc_knn_accumulate).  ``q``: contiguous fp32 ``[nq, d]``, ``ref``: contiguous fp32 ``[nr, d]``, d in 1..``L.KNN_MAX_DIM``, k in
    1..``L.KNN_MAX_K``; ``best``: contiguous fp32 ``[nq, k]``, ascending per row.  Differences in fp32, summed by ``fmaf`` in column
    order; the selection is min / max alone, so a NaN distance is never selected, slots without a neighbour hold +inf, and ``best`` is
    bitwise independent of the order of the reference rows and of how ``ref`` is chunked over calls with ``accumulate=True`` (the k best
    of the old ``best`` and this call's distances).  ``accumulate=False`` overwrites.  ``workspace``: a contiguous device tensor of at
    least ``knn_workspace_bytes(nq, nr, d, k)`` bytes, 4-B aligned; None allocates one for this call.  Everything on the device of
    ``q``.  On the current torch stream."""
    lib = L.load()
    if not isinstance(q, torch.Tensor) or q.dim() != 2:
        raise TypeError("q: expected a torch.Tensor [nq, d]")
    if not isinstance(ref, torch.Tensor) or ref.dim() != 2:
        raise TypeError("ref: expected a torch.Tensor [nr, d]")
    device = q.device
    if device.type != "cuda":
        raise ValueError(f"q: expected a tensor on a HIP device, got {device}")
    nq, d = (int(s) for s in q.shape)
    nr = int(ref.shape[0])
    k = int(k)
    if not 1 <= d <= L.KNN_MAX_DIM:
        raise ValueError(f"q: {d} coordinates, expected 1..{L.KNN_MAX_DIM}")
    if not 1 <= k <= L.KNN_MAX_K:
        raise ValueError(f"k: {k}, expected 1..{L.KNN_MAX_K}")
    _check_tensor(q, (nq, d), device, "q")
    _check_tensor(ref, (nr, d), device, "ref")
    _check_tensor(best, (nq, k), device, "best")
    need = _workspace_bytes(lib.mcpc_knn_workspace_bytes, nq, nr, d, k)
    workspace, ws_bytes = _check_workspace(workspace, device, need, 4, "knn_workspace_bytes")
    stream = _current_stream(device)
    L.check(lib.mcpc_knn_accumulate(device.index or 0, _ptr(q), nq, _ptr(ref), nr, d, k, _ptr(best), 1 if accumulate else 0,
                                    _ptr(workspace), ws_bytes, stream))


_LOGLIK_LOSSES = {"bernoulli": L.LOSS_BERNOULLI, "gaussian": L.LOSS_GAUSSIAN}
_SAMPLE_READOUTS = {None: L.SAMPLE_HIDDEN, "hidden": L.SAMPLE_HIDDEN, "mean": L.SAMPLE_MEAN, "draw": L.SAMPLE_DRAW}


def loglik_workspace_bytes(n_data, n_samp, width) -> int:
    """Bytes of device workspace ``loglik_accumulate`` needs for ``n_data`` data against ``n_samp`` samples of ``width`` columns."""
    return _workspace_bytes(L.load().mcpc_loglik_workspace_bytes, int(n_data), int(n_samp), int(width))


def loglik_accumulate(y, out, loss, var, clamp, state, accumulate=False, workspace=None):
    """The importance-sampling state of every datum's log marginal likelihood over the read-outs of prior samples, on the device
    (include/mcpc.h: mcpc_loglik_accumulate).  ``y``: contiguous fp32 ``[n_data, width]``, the data; ``out``: contiguous fp32
    ``[n_samp, width]``, logits (``loss="bernoulli"``) or means (``loss="gaussian"``, with the variance ``var``; None otherwise),
    clamped to ``+-clamp`` (``math.inf``: not at all); ``state``: contiguous fp64 ``[n_data, 4]``, per datum ``(m, s1, s2, cnt)`` --
    the smallest nll, the sums of ``exp(-(nll - m))`` and of its square, the samples taken.  fp64 throughout, the dot products on the
    fp64 MFMA.  ``accumulate=False`` overwrites; ``accumulate=True`` merges the old state with this call's, so the samples can be
    streamed -- equal to the one-shot call within a rounding bound, not bitwise; two runs of the same call are bitwise equal.  A
    (datum, sample) pair with a non-finite nll is neither taken nor counted.  ``workspace``: a contiguous device tensor of at least
    ``loglik_workspace_bytes(n_data, n_samp, width)`` bytes, 8-B aligned; None allocates one for this call.  Everything on the device
    of ``y``.  On the current torch stream."""
    lib = L.load()
    if not isinstance(y, torch.Tensor) or y.dim() != 2:
        raise TypeError("y: expected a torch.Tensor [n_data, width]")
    if not isinstance(out, torch.Tensor) or out.dim() != 2:
        raise TypeError("out: expected a torch.Tensor [n_samp, width]")
    device = y.device
    if device.type != "cuda":
        raise ValueError(f"y: expected a tensor on a HIP device, got {device}")
    if loss not in _LOGLIK_LOSSES:
        raise ValueError(f"loss: expected 'bernoulli' or 'gaussian', got {loss!r}")
    if loss == "gaussian":
        if var is None or not float(var) > 0.0:
            raise ValueError(f"var: the Gaussian read-out needs a positive variance, got {var!r}")
    elif var is not None:
        raise ValueError(f"var: expected None with loss={loss!r}")
    clamp = float(clamp)
    if not clamp > 0.0:
        raise ValueError(f"clamp: expected a positive bound (math.inf: none), got {clamp!r}")
    n_data, width = (int(s) for s in y.shape)
    n_samp = int(out.shape[0])
    if width < 1:
        raise ValueError("y: expected at least one column")
    _check_tensor(y, (n_data, width), device, "y")
    _check_tensor(out, (n_samp, width), device, "out")
    _check_tensor(state, (n_data, 4), device, "state", torch.float64)
    need = _workspace_bytes(lib.mcpc_loglik_workspace_bytes, n_data, n_samp, width)
    workspace, ws_bytes = _check_workspace(workspace, device, need, 8, "loglik_workspace_bytes")
    stream = _current_stream(device)
    L.check(lib.mcpc_loglik_accumulate(device.index or 0, _ptr(y), n_data, _ptr(out), n_samp, width, _LOGLIK_LOSSES[loss],
                                       float(var) if loss == "gaussian" else 1.0, clamp, _ptr(state), 1 if accumulate else 0,
                                       _ptr(workspace), ws_bytes, stream))


_AIS_ACTS = {"identity": L.ACT_IDENTITY, "relu": L.ACT_RELU, "tanh": L.ACT_TANH,
             L.ACT_IDENTITY: L.ACT_IDENTITY, L.ACT_RELU: L.ACT_RELU, L.ACT_TANH: L.ACT_TANH}
_AIS_LOSSES = {**_LOGLIK_LOSSES, L.LOSS_BERNOULLI: L.LOSS_BERNOULLI, L.LOSS_GAUSSIAN: L.LOSS_GAUSSIAN}


def ais_increment(x, W, bias, y, act, loss, var, mask_start, a0, c0, a1, c1, logw, accumulate=True):
    """Add the log-weight increment of one rung of annealed importance sampling to ``logw`` on the device (include/mcpc.h:
    mcpc_ais_increment).  ``x``: contiguous fp32 ``[rows, width]``, the last latent layer of ``rows`` chains; ``W``: contiguous fp32
    ``[n_out, width]`` (the layout of ``nn.Linear.weight``), the UNSCALED read-out; ``bias``: fp32 ``[n_out]`` or None for zeros;
    ``y``: contiguous fp32 ``[rows, n_out]``, the target row of each chain; ``act``: "identity", "relu", "tanh" or an ``L.ACT_*``;
    ``loss``: "bernoulli", "gaussian" or an ``L.LOSS_*`` (Gaussian: with the variance ``var``); ``logw``: contiguous fp64 ``[rows]``.
    With ``o = f(x) W^T + bias`` and ``l(a)`` the loss of ``a o`` against ``y`` summed over the columns from ``mask_start`` on,
    ``logw += c0 l(a0) - c1 l(a1)`` per row (``accumulate=False`` overwrites); a side whose ``c`` is exactly 0 is not evaluated.  fp64
    throughout, the contraction on the fp64 MFMA.  A row's result depends on that row, ``W``, ``bias`` and the scalars alone, and two
    runs of the same call are bitwise equal.  Everything on the device of ``x``.  On the current torch stream."""
    lib = L.load()
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise TypeError("x: expected a torch.Tensor [rows, width]")
    if not isinstance(W, torch.Tensor) or W.dim() != 2:
        raise TypeError("W: expected a torch.Tensor [n_out, width]")
    device = x.device
    if device.type != "cuda":
        raise ValueError(f"x: expected a tensor on a HIP device, got {device}")
    if act not in _AIS_ACTS:
        raise ValueError(f"act: expected 'identity', 'relu' or 'tanh', got {act!r}")
    if loss not in _AIS_LOSSES:
        raise ValueError(f"loss: expected 'bernoulli' or 'gaussian', got {loss!r}")
    loss_kind = _AIS_LOSSES[loss]
    if loss_kind == L.LOSS_GAUSSIAN and (var is None or not float(var) > 0.0):
        raise ValueError(f"var: the Gaussian read-out needs a positive variance, got {var!r}")
    rows, width = (int(s) for s in x.shape)
    n_out = int(W.shape[0])
    if width < 1 or n_out < 1:
        raise ValueError(f"x has {width} columns and W {n_out} rows: expected at least one of each")
    mask_start = int(mask_start)
    if not 0 <= mask_start < n_out:
        raise ValueError(f"mask_start={mask_start} outside 0..{n_out - 1}")
    scalars = [float(v) for v in (a0, c0, a1, c1)]
    if any(v != v for v in scalars):
        raise ValueError(f"(a0, c0, a1, c1) = {tuple(scalars)}: a NaN")
    _check_tensor(x, (rows, width), device, "x")
    _check_tensor(W, (n_out, width), device, "W")
    if bias is not None:
        _check_tensor(bias, (n_out,), device, "bias")
    _check_tensor(y, (rows, n_out), device, "y")
    _check_tensor(logw, (rows,), device, "logw", torch.float64)
    if rows == 0:                                  # an empty tensor has no address to hand over
        return
    stream = _current_stream(device)
    L.check(lib.mcpc_ais_increment(device.index or 0, _ptr(x), rows, width, _AIS_ACTS[act], _ptr(W), _ptr(bias), n_out, _ptr(y), loss_kind,
                                   float(var) if loss_kind == L.LOSS_GAUSSIAN else 1.0, mask_start, *scalars, _ptr(logw),
                                   1 if accumulate else 0, stream))


def _mala_shape(xs):
    """(rows, widths, device) of a state as the MALA entries take it: a list of 1..MAX_LATENT fp32 ``[rows, n_l]`` tensors on one HIP
    device."""
    if not isinstance(xs, (list, tuple)) or not 1 <= len(xs) <= L.MAX_LATENT:
        raise ValueError(f"xs: expected a list of 1..{L.MAX_LATENT} tensors, one per layer")
    for l, t in enumerate(xs):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise TypeError(f"xs[{l}]: expected a torch.Tensor [rows, width]")
        if t.shape[1] < 1:
            raise ValueError(f"xs[{l}]: a layer of width 0")
    device = xs[0].device
    if device.type != "cuda":
        raise ValueError(f"xs[0]: expected a tensor on a HIP device, got {device}")
    return int(xs[0].shape[0]), [int(t.shape[1]) for t in xs], device


def _mala_ptrs(tensors, name, rows, widths, device):
    """The host array of device pointers of a state of that shape."""
    if not isinstance(tensors, (list, tuple)) or len(tensors) != len(widths):
        raise ValueError(f"{name}: expected a list of {len(widths)} tensors, one per layer")
    arr = (C.c_void_p * len(widths))()
    for l, t in enumerate(tensors):
        _check_tensor(t, (rows, widths[l]), device, f"{name}[{l}]")
        arr[l] = t.data_ptr()
    return arr


def _mala_scalars(lr, noise_var, seed, step, chain_base):
    lr, noise_var = float(lr), float(noise_var)
    for name, v in (("lr", lr), ("noise_var", noise_var)):
        if not (v > 0.0 and v != float("inf")):
            raise ValueError(f"{name}={v!r}, must be positive and finite")
    return lr, noise_var, int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF, int(chain_base) & 0xFFFFFFFFFFFFFFFF


def mala_propose(xs, gs, lr, noise_var, seed, step, chain_base=0, out=None):
    """The Langevin proposal of a Metropolis-adjusted step on the device (include/mcpc.h: mcpc_mala_propose): per layer
    ``out_l = (x_l - lr g_l) + sqrt(noise_var lr) xi_l`` in fp32, four separate roundings, with ``xi_l`` the normals of ``(seed, step,
    layer l, chain_base + row)`` -- ``philox_normals`` of the same arguments, those a fused Langevin step at that ``(seed, step)``
    consumes.  ``xs``, ``gs``: one contiguous fp32 ``[rows, n_l]`` tensor per layer (1..MAX_LATENT of them): a state and its gradient
    (``Engine.run(1, update_x=False).xgrad``).  ``out``: tensors to fill (they must not overlap ``xs`` or ``gs``), or None for fresh
    ones.  Returns ``out``.  On the current torch stream."""
    lib = L.load()
    rows, widths, device = _mala_shape(xs)
    x_arr, g_arr = _mala_ptrs(xs, "xs", rows, widths, device), _mala_ptrs(gs, "gs", rows, widths, device)
    lr, noise_var, seed, step, chain_base = _mala_scalars(lr, noise_var, seed, step, chain_base)
    if out is None:
        out = [torch.empty_like(x) for x in xs]
    o_arr = _mala_ptrs(out, "out", rows, widths, device)
    if rows == 0:                                  # an empty tensor has no address to hand over
        return out
    w_arr = (C.c_int32 * len(widths))(*widths)
    L.check(lib.mcpc_mala_propose(device.index or 0, x_arr, g_arr, w_arr, len(widths), rows, lr, noise_var, seed, step, chain_base, o_arr,
                                  _current_stream(device)))
    return out


def mala_accept(xs, gs, E, xps, gps, Ep, lr, noise_var, seed, step, chain_base=0, diag=None, n_accepted=None, x_next=None):
    """The Metropolis-Hastings decision of a Metropolis-adjusted Langevin step on the device (include/mcpc.h: mcpc_mala_accept).
    ``(xs, gs, E)``: the current state, its gradient and its energy (fp64 ``[rows]``, the last column of ``Engine.chain_energies``);
    ``(xps, gps, Ep)``: the proposal ``mala_propose`` made at this ``(seed, step, chain_base)`` with this ``lr`` and ``noise_var``, and
    the gradient and energy the engine evaluated at it.  Per chain ``log_alpha = E - E' - (|x - x' + lr g'|^2 - |x' - x + lr g|^2) /
    (2 noise_var lr)`` in fp64 and ``accept = log(u) < log_alpha`` with ``u`` the chain's Philox uniform of ``(seed, step, layer
    0xFF)``.  An accepted chain's rows of ``xs``, ``gs`` and ``E`` are overwritten IN PLACE with the proposal's; a rejected one keeps
    its bits.  A row's result depends on that row alone and two runs are bitwise equal.  Optional: ``diag`` fp64 ``[rows, 3]`` receives
    (log_alpha, u, accepted); ``n_accepted`` int32 ``[rows]`` is incremented for an accepted chain; ``x_next``, a state, receives the
    proposal of ``step + 1`` from the selected ``(x, g)``, bitwise ``mala_propose``'s (it must not overlap another argument).  On the
    current torch stream."""
    lib = L.load()
    rows, widths, device = _mala_shape(xs)
    n = len(widths)
    x_arr, g_arr = _mala_ptrs(xs, "xs", rows, widths, device), _mala_ptrs(gs, "gs", rows, widths, device)
    xp_arr, gp_arr = _mala_ptrs(xps, "xps", rows, widths, device), _mala_ptrs(gps, "gps", rows, widths, device)
    xn_arr = None if x_next is None else _mala_ptrs(x_next, "x_next", rows, widths, device)
    _check_tensor(E, (rows,), device, "E", torch.float64)
    _check_tensor(Ep, (rows,), device, "Ep", torch.float64)
    if diag is not None:
        _check_tensor(diag, (rows, 3), device, "diag", torch.float64)
    if n_accepted is not None:
        _check_tensor(n_accepted, (rows,), device, "n_accepted", torch.int32)
    lr, noise_var, seed, step, chain_base = _mala_scalars(lr, noise_var, seed, step, chain_base)
    if rows == 0:
        return
    w_arr = (C.c_int32 * n)(*widths)
    L.check(lib.mcpc_mala_accept(device.index or 0, x_arr, g_arr, _ptr(E), xp_arr, gp_arr, _ptr(Ep), w_arr, n, rows, lr, noise_var, seed,
                                 step, chain_base, _ptr(diag), _ptr(n_accepted), xn_arr, _current_stream(device)))


def hmc_begin(xs, gs, lr, seed, step, chain_base=0, q_out=None, x_out=None, K0=None):
    """The first leapfrog step of a Hamiltonian trajectory on the device (include/mcpc.h: mcpc_hmc_begin): per layer, with ``eps =
    sqrt(2 lr)`` rounded to fp32 once and ``h = eps / 2``, ``p = xi_l``, ``q_l = p - h g_l``, ``x_out_l = x_l + eps q_l`` in fp32, every
    operation rounded separately, with ``xi_l`` the normals of ``(seed, step, layer l, chain_base + row)`` -- ``philox_normals`` of
    the same arguments, those ``mala_propose`` takes.  ``K0`` fp64 ``[rows]`` receives the kinetic energy ``0.5 |p|^2`` per chain.
    ``xs``, ``gs``: one contiguous fp32 ``[rows, n_l]`` tensor per layer (1..MAX_LATENT of them): a state and its gradient
    (``Engine.run(1, update_x=False).xgrad``).  ``q_out``, ``x_out``, ``K0``: tensors to fill (they must not overlap ``xs`` or ``gs``),
    or None for fresh ones.  Returns ``(q_out, x_out, K0)``.  On the current torch stream."""
    lib = L.load()
    rows, widths, device = _mala_shape(xs)
    x_arr, g_arr = _mala_ptrs(xs, "xs", rows, widths, device), _mala_ptrs(gs, "gs", rows, widths, device)
    lr, _, seed, step, chain_base = _mala_scalars(lr, 2.0, seed, step, chain_base)
    if q_out is None:
        q_out = [torch.empty_like(x) for x in xs]
    if x_out is None:
        x_out = [torch.empty_like(x) for x in xs]
    if K0 is None:
        K0 = torch.empty(rows, dtype=torch.float64, device=device)
    q_arr, o_arr = _mala_ptrs(q_out, "q_out", rows, widths, device), _mala_ptrs(x_out, "x_out", rows, widths, device)
    _check_tensor(K0, (rows,), device, "K0", torch.float64)
    if rows == 0:                                  # an empty tensor has no address to hand over
        return q_out, x_out, K0
    w_arr = (C.c_int32 * len(widths))(*widths)
    L.check(lib.mcpc_hmc_begin(device.index or 0, x_arr, g_arr, w_arr, len(widths), rows, lr, seed, step, chain_base, q_arr, o_arr,
                               _ptr(K0), _current_stream(device)))
    return q_out, x_out, K0


def hmc_leap(xts, qs, gts, lr):
    """An interior leapfrog step of a Hamiltonian trajectory on the device (include/mcpc.h: mcpc_hmc_leap), IN PLACE on the
    trajectory's position ``xts`` and half-step momentum ``qs``: ``q_l = q_l - eps g_t,l``, then ``x_t,l = x_t,l + eps q_l`` with
    ``eps = sqrt(2 lr)``, in fp32, every operation rounded separately.  ``gts``: the gradient at ``xts`` as it stands before the call.
    No random numbers.  On the current torch stream."""
    lib = L.load()
    rows, widths, device = _mala_shape(xts)
    x_arr, q_arr = _mala_ptrs(xts, "xts", rows, widths, device), _mala_ptrs(qs, "qs", rows, widths, device)
    g_arr = _mala_ptrs(gts, "gts", rows, widths, device)
    lr = _mala_scalars(lr, 2.0, 0, 0, 0)[0]
    if rows == 0:
        return
    w_arr = (C.c_int32 * len(widths))(*widths)
    L.check(lib.mcpc_hmc_leap(device.index or 0, x_arr, q_arr, g_arr, w_arr, len(widths), rows, lr, _current_stream(device)))


def hmc_accept(xs, gs, E, xts, gts, Et, qs, K0, lr, seed, step, chain_base=0, diag=None, n_accepted=None):
    """The Metropolis decision at the end of a Hamiltonian trajectory on the device (include/mcpc.h: mcpc_hmc_accept).  ``(xs, gs,
    E)``: the current state, its gradient and its energy (fp64 ``[rows]``, the last column of ``Engine.chain_energies``); ``(xts, gts,
    Et)``: the trajectory's end and the gradient and energy the engine evaluated at it; ``qs``, ``K0``: the half-step momentum and
    the initial kinetic energy that ``hmc_begin`` at this ``(seed, step, chain_base)`` and ``lr`` started and ``hmc_leap`` carried.
    Per chain ``p' = q - (eps / 2) g_t`` in fp32, ``log_alpha = (E - E_t) + (K0 - 0.5 |p'|^2)`` in fp64 and ``accept = log(u) <
    log_alpha`` with ``u`` the chain's Philox uniform of ``(seed, step, layer 0xFD)``.  An accepted chain's rows of ``xs``, ``gs`` and
    ``E`` are overwritten IN PLACE with the end point's; a rejected one keeps its bits.  ``xts``, ``gts``, ``qs`` and ``K0`` are never
    written.  A row's result depends on that row alone and two runs are bitwise equal.  Optional: ``diag`` fp64 ``[rows, 3]`` receives
    (log_alpha, u, accepted); ``n_accepted`` int32 ``[rows]`` is incremented for an accepted chain.  On the current torch stream."""
    lib = L.load()
    rows, widths, device = _mala_shape(xs)
    n = len(widths)
    x_arr, g_arr = _mala_ptrs(xs, "xs", rows, widths, device), _mala_ptrs(gs, "gs", rows, widths, device)
    xt_arr, gt_arr = _mala_ptrs(xts, "xts", rows, widths, device), _mala_ptrs(gts, "gts", rows, widths, device)
    q_arr = _mala_ptrs(qs, "qs", rows, widths, device)
    _check_tensor(E, (rows,), device, "E", torch.float64)
    _check_tensor(Et, (rows,), device, "Et", torch.float64)
    _check_tensor(K0, (rows,), device, "K0", torch.float64)
    if diag is not None:
        _check_tensor(diag, (rows, 3), device, "diag", torch.float64)
    if n_accepted is not None:
        _check_tensor(n_accepted, (rows,), device, "n_accepted", torch.int32)
    lr, _, seed, step, chain_base = _mala_scalars(lr, 2.0, seed, step, chain_base)
    if rows == 0:
        return
    w_arr = (C.c_int32 * n)(*widths)
    L.check(lib.mcpc_hmc_accept(device.index or 0, x_arr, g_arr, _ptr(E), xt_arr, gt_arr, _ptr(Et), q_arr, _ptr(K0), w_arr, n, rows, lr,
                                seed, step, chain_base, _ptr(diag), _ptr(n_accepted), _current_stream(device)))


def smc_ancestors(logw, replicas, threshold, seed, step, chain_base=0, ancestors=None, diag=None):
    """The resampling decision and the ancestors of every datum of a chunk on the device (include/mcpc.h: mcpc_smc_ancestors).
    ``logw``: fp64 ``[n_data * replicas]``, datum i owning rows ``i * replicas ..``.  Per datum, in fp64 and sequentially in replica
    order, ``ess = (sum e)^2 / sum e^2`` with ``e_j = exp(logw_j - max)`` over the finite log-weights; when ``ess < threshold *
    replicas`` the datum draws ``replicas`` ancestors by systematic resampling with the Philox uniform of ``(seed, step, layer 0xFE,
    chain_base + i * replicas)`` and ALL its log-weights are overwritten IN PLACE with the log of the mean weight; otherwise it gets
    identity ancestors and its log-weights are not written.  ``threshold`` in [0, 1], ``replicas`` in 1..SMC_MAX_REPLICAS.  A datum's
    result depends on its own log-weights and scalars alone and two runs are bitwise equal.  Optional: ``ancestors`` int32 ``[n_data
    * replicas]`` to fill (else a fresh one), ``diag`` fp64 ``[n_data, 4]`` receives (ess, resampled, u, log mean weight).  Returns
    ``ancestors`` (row indices into the chunk).  On the current torch stream."""
    lib = L.load()
    if not isinstance(logw, torch.Tensor) or logw.dim() != 1:
        raise TypeError("logw: expected a torch.Tensor [n_data * replicas]")
    device = logw.device
    if device.type != "cuda":
        raise ValueError(f"logw: expected a tensor on a HIP device, got {device}")
    if isinstance(replicas, bool) or not isinstance(replicas, int) or not 1 <= replicas <= L.SMC_MAX_REPLICAS:
        raise ValueError(f"replicas={replicas!r}, must be an int in 1..{L.SMC_MAX_REPLICAS}")
    threshold = float(threshold)
    if not 0.0 <= threshold <= 1.0:
        raise ValueError(f"threshold={threshold!r} outside [0, 1]")
    rows = int(logw.shape[0])
    if rows % replicas:
        raise ValueError(f"logw holds {rows} rows, no multiple of replicas={replicas}")
    _check_tensor(logw, (rows,), device, "logw", torch.float64)
    if ancestors is None:
        ancestors = torch.empty(rows, dtype=torch.int32, device=device)
    _check_tensor(ancestors, (rows,), device, "ancestors", torch.int32)
    if diag is not None:
        _check_tensor(diag, (rows // replicas, 4), device, "diag", torch.float64)
    if rows == 0:                                  # an empty tensor has no address to hand over
        return ancestors
    mask = 0xFFFFFFFFFFFFFFFF
    L.check(lib.mcpc_smc_ancestors(device.index or 0, _ptr(logw), rows // replicas, replicas, threshold, int(seed) & mask, int(step) & mask,
                                   int(chain_base) & mask, _ptr(ancestors), _ptr(diag), _current_stream(device)))
    return ancestors


def smc_gather(xs, ancestors, out=None, n_bad=None):
    """``out_l[r] = xs_l[ancestors[r]]`` for every layer of a state in one launch (include/mcpc.h: mcpc_smc_gather), bitwise and out of
    place.  ``xs``: one contiguous fp32 ``[rows, n_l]`` tensor per layer (1..MAX_LATENT of them); ``ancestors``: int32 ``[rows]``.  An
    index outside ``0..rows - 1`` is never dereferenced: that row copies itself and ``n_bad`` (int32 ``[1]``, optional) is incremented.
    ``out``: tensors to fill (they must not overlap ``xs``), or None for fresh ones.  Returns ``out``.  On the current torch stream."""
    lib = L.load()
    rows, widths, device = _mala_shape(xs)
    x_arr = _mala_ptrs(xs, "xs", rows, widths, device)
    _check_tensor(ancestors, (rows,), device, "ancestors", torch.int32)
    if out is None:
        out = [torch.empty_like(x) for x in xs]
    o_arr = _mala_ptrs(out, "out", rows, widths, device)
    if n_bad is not None:
        _check_tensor(n_bad, (1,), device, "n_bad", torch.int32)
    if rows == 0:
        return out
    w_arr = (C.c_int32 * len(widths))(*widths)
    L.check(lib.mcpc_smc_gather(device.index or 0, x_arr, w_arr, len(widths), rows, _ptr(ancestors), o_arr, _ptr(n_bad),
                                _current_stream(device)))
    return out

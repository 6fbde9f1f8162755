#!/usr/bin/env python3
"""SHA-256 of every Linear's dW / db after a learning call, for every case of tests/test_gpu_flush.py's tables (shapes x forms, the
heb171 re-split, the row axis, the scale history, the step-kernel axis) and for cfg-M's net with a ring that wraps three times,
overlapped and with no_overlap=1.  One line per (case, Linear): run it once per library (MCPC_LIB=scripts/bin/libmcpc_<commit>.so
from scripts/build_old_lib.sh for an earlier commit) and diff the outputs -- a change that leaves the flush's arithmetic alone
leaves every line alone.

    python3 scripts/flush_hashes.py > out/flush_hashes_head.txt
    MCPC_LIB=scripts/bin/libmcpc_<commit>.so python3 scripts/flush_hashes.py > out/flush_hashes_<commit>.txt
"""
import hashlib
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from montecarlopredictivecoding_amd import _lib as L  # noqa: E402
from montecarlopredictivecoding_amd.engine import Engine  # noqa: E402
from tests import test_gpu_flush as F  # noqa: E402

DEV = F.DEV


def _grads(tag, eng, dims):
    for j in range(len(dims) - 1):
        gW, gb = torch.empty(dims[j + 1], dims[j], device=DEV), torch.empty(dims[j + 1], device=DEV)
        eng.read_param_grads(j, gW, gb)
        eng.sync_check()
        sha = [hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:32] for t in (gW, gb)]
        print(f"{tag} | Linear {j} | dW {sha[0]} db {sha[1]} | {eng.last_flush_plan(j)}", flush=True)


def exact(tag, sizes, n_out, B, T, tuning, seed, seg_len=None, seg_exps=None):
    """The exact-image problem of test_gpu_flush._run_exact (zero weights, identity activations, injected states)."""
    dims = [F.N_IN] + list(sizes) + ([n_out] if n_out else [])
    W = [torch.zeros(dims[j + 1], dims[j], device=DEV) for j in range(len(dims) - 1)]
    b = [torch.zeros(dims[j + 1], device=DEV) for j in range(len(dims) - 1)]
    states = [x.to(DEV) for x in F._exact_states(sizes, B, T, seed, seg_len, seg_exps)]
    g = torch.Generator().manual_seed(seed + 1000)
    y = (torch.rand(B, n_out, generator=g) * 2 - 1).to(DEV) if n_out else None
    eng = Engine(sizes, [L.ACT_IDENTITY] * len(sizes), F.N_IN, n_out, B, device=DEV, tuning=tuning)
    try:
        eng.bind_params(W, b)
        eng.bind_inputs(None)
        if n_out:
            eng.bind_target(y)
        eng.load_state([x[0].contiguous() for x in states])
        ext = [torch.cat([x[1:], torch.zeros_like(x[:1])]).contiguous() for x in states]
        eng.run(T, loss_kind=L.LOSS_GAUSSIAN if n_out else L.LOSS_NONE, loss_var=1.0, lr=1.0, noise_mode=L.NOISE_EXTERNAL, noise_var=1.0,
                ext_noise=ext, acc_begin=0, acc_end=T)
        _grads(tag, eng, dims)
    finally:
        eng.close()


def realistic(tag, sizes, n_out, B, act, tuning, T, acc_begin):
    """The realistic problem of test_gpu_flush._step_case (random weights, Bernoulli read-out, Philox noise)."""
    g = torch.Generator().manual_seed(B + len(sizes))
    dims = [F.N_IN] + list(sizes) + [n_out]
    W = [(torch.randn(dims[j + 1], dims[j], generator=g) / math.sqrt(dims[j])).to(DEV) for j in range(len(dims) - 1)]
    b = [(0.1 * torch.randn(dims[j + 1], generator=g)).to(DEV) for j in range(len(dims) - 1)]
    y = (torch.rand(B, n_out, generator=g) < 0.3).float().to(DEV)
    x0 = [torch.randn(B, n, generator=g).to(DEV) for n in sizes]
    eng = Engine(sizes, [act] * len(sizes), F.N_IN, n_out, B, device=DEV, tuning=tuning)
    try:
        eng.bind_params(W, b)
        eng.bind_inputs(None)
        eng.bind_target(y)
        eng.load_state(x0)
        eng.run(T, loss_kind=L.LOSS_BERNOULLI, lr=0.03, noise_mode=L.NOISE_PHILOX, noise_var=2.0, seed=5, step_base=0, acc_begin=acc_begin,
                acc_end=T)
        _grads(tag, eng, dims)
    finally:
        eng.close()


def main():
    join = lambda *t: ",".join(x for x in t if x) or None
    for net, (sizes, n_out, _) in F.SHAPE_NETS.items():
        for form, knob in F.FORMS.items():
            exact(f"shape {net} {form}", sizes, n_out, F.SHAPE_B, F.SHAPE_T, knob, seed=len(net))
    sizes, n_out, _ = F.SHAPE_NETS["128-256-272"]
    exact("shape 128-256-272 f16 heb171", sizes, n_out, F.SHAPE_B, F.SHAPE_T, "heb171=1", seed=len("128-256-272"))
    for case, (B, T, extra) in F.ROW_CASES.items():
        for form, knob in F.FORMS.items():
            exact(f"rows {case} {form}", *F.ROW_NET, B, T, join(knob, extra), seed=T)
    for ring, extra in F.HIST_TUNINGS.items():
        for form, knob in F.FORMS.items():
            exact(f"scale history {ring} {form}", *F.HIST_NET, 48, F.SEG_LEN * len(F.SEG_EXPS), join(knob, extra), seed=7,
                  seg_len=F.SEG_LEN, seg_exps=F.SEG_EXPS)
    for net, tuning in F.STEP_CASES:
        cfg = F.STEP_NETS[net]
        act = {"tanh": L.ACT_TANH, "relu": L.ACT_RELU}[cfg["act"]]
        realistic(f"step kernel {net} {tuning or 'default'}", cfg["sizes"], cfg["n_out"], cfg["B"], act, tuning, F.STEP_T, F.STEP_T - F.STEP_ACC)
    # cfg-M's net, 256 chains: ring parts of 2 slots, 20 accumulating steps = 10 segments (the three parts are refilled three times);
    # serially the whole ring of 6 slots is one part: segments of 6, 6, 6, 2
    for tuning in ("slot_cap=6", "slot_cap=6,no_overlap=1"):
        realistic(f"cfg-M learning call {tuning}", [30, 256, 256], 784, 256, L.ACT_RELU, tuning, 24, 4)


if __name__ == "__main__":
    main()

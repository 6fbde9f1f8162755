#!/usr/bin/env python3
"""Posterior covariances accumulated on the device (csrc/mcpc_cov.h, PCTrainer.mcpc_covariance) against the two other ways to run the
same call (developer measurement for DESIGN.md section 7, profiles/cov_cost.txt).

    python scripts/cov_cost.py [--workloads g,a0,a3,m0,m3] [--repeats 3] [--T 1000] [--out FILE]
    python scripts/cov_cost.py --kernel-alone                  # only the first part: cov_accumulate by itself, HIP events

A run times cov_accumulate alone first and the workloads after it; --out FILE replaces FILE with what was printed.

Workloads, through the facade (PCTrainer.train_on_batch, host work included, wall clock around synchronised calls), one MCPC call of T
steps each, the covariance over the steps from T / 5 on:
  g   g13's shape: 6-16-16 -> 24 at 4096 chains, all layers (38 columns), pooled
  a0  the reference's net 20-128-128 -> 784 at 256 chains, layers=(0,), per chain
  a3  the same, all layers (276 columns), per chain
  m0  cfg-M's net 30 | 256-256-256 -> 784 at 6000 chains, layers=(0,), pooled
  m3  the same, all layers (768 columns), pooled
Variants:
  cov    the call with mcpc_covariance
  plain  the same call without it and without records: cov - plain is what the covariance costs
  torch  what a user does without it: record the trajectory (is_return_representations / is_return_xs), then sum and x.T @ x in torch
         fp64 on the same GPU, step chunk by step chunk
Every variant is warmed up once; then the variants alternate inside each of --repeats rounds; min (max) of the rounds is reported.
A run without a GPU fails: there is no fallback."""
import argparse
import os
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import montecarlopredictivecoding_amd.predictive_coding as pc  # noqa: E402
import montecarlopredictivecoding_amd.predictive_coding.pc_trainer as pt  # noqa: E402
import montecarlopredictivecoding_amd.utils.model as um  # noqa: E402

DEV = torch.device("cuda", 0)


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def replay():
    """Every run of a workload draws the same x0 and the same Langevin noise, so that the variants compute the same statistics."""
    torch.manual_seed(3)
    pt._PHILOX_STEPS[0] = 0


def torch_outer(steps, pooled, chunk=50):
    """(sum, outer) in torch fp64 on the GPU from recorded steps: steps[k] is a list of [B, n_l] host tensors."""
    s = o = None
    for k0 in range(0, len(steps), chunk):
        x = torch.stack([torch.cat(list(st), dim=1) for st in steps[k0:k0 + chunk]]).to(DEV, non_blocking=True).double()   # [c, B, D]
        if pooled:
            f = x.reshape(-1, x.shape[2])
            ds, do = f.sum(0), f.T @ f
        else:
            c = x.transpose(0, 1)
            ds, do = x.sum(0), c.transpose(1, 2) @ c
        s, o = (ds, do) if s is None else (s + ds, o + do)
    return s, o


class Workload:
    def __init__(self, name, dims, n_out, B, T, layers, pool, lr=0.01):
        mods = []
        for i in range(1, len(dims)):
            mods += [torch.nn.Linear(dims[i - 1], dims[i]), pc.PCLayer(sample_x_fn=um.sample_x_fn_normal), torch.nn.ReLU()]
        self.model = torch.nn.Sequential(*mods, torch.nn.Linear(dims[-1], n_out)).to(DEV)
        self.model.train()
        self.name, self.T, self.begin, self.B, self.layers, self.pool = name, T, T // 5, B, layers, pool
        self.all_layers = len(layers) == len(dims) - 1
        self.data = (torch.rand(B, n_out, device=DEV) < 0.3).float()
        self.inputs = torch.zeros(B, dims[0], device=DEV)
        self.tr = pc.PCTrainer(self.model, T=T, optimizer_x_fn=torch.optim.SGD, optimizer_x_kwargs={"lr": lr}, update_p_at="never",
                               plot_progress_at=[])
        self.n = T - self.begin
        self.D = sum(dims[1 + l] for l in layers)
        self.slices = 0

    def run(self, variant):
        replay()
        kw = dict(inputs=self.inputs, loss_fn=um.bernoulli_fn, loss_fn_kwargs={"_target": self.data, "_var": None},
                  callback_after_t=um.random_step, callback_after_t_kwargs={"_pc_trainer": self.tr}, is_log_progress=False,
                  is_checking_after_callback_after_t=False)
        self.tr.mcpc_covariance = dict(begin=self.begin, layers=self.layers, pool=self.pool) if variant == "cov" else None
        if variant == "torch":
            if self.all_layers:
                r = self.tr.train_on_batch(is_return_results_every_t=True, is_return_xs=True, **kw)
                steps = r["xs"][self.begin:]
            else:
                r = self.tr.train_on_batch(is_return_results_every_t=True, is_return_representations=True, **kw)
                steps = [[x] for x in r["representations"][self.begin:]]
            return torch_outer(steps, self.pool is not None)
        self.tr.train_on_batch(is_return_results_every_t=False, **kw)
        if variant == "cov":
            self.slices = self.tr.last_record_slices
            c = self.tr.mcpc_last_covariance
            return c.sum, c.outer
        return None


def workloads(args):
    T = args.T
    ref, cfg_m = [20, 20, 128, 128], [30, 256, 256, 256]
    return {
        "g": lambda: Workload("g: 6-16-16 -> 24, 4096 chains, all layers (38 columns), pooled", [6, 6, 16, 16], 24, 4096, T, (0, 1, 2), "chains"),
        "a0": lambda: Workload("a0: 20-128-128 -> 784, 256 chains, layers=(0,) (20 columns), per chain", ref, 784, 256, T, (0,), None),
        "a3": lambda: Workload("a3: 20-128-128 -> 784, 256 chains, all layers (276 columns), per chain", ref, 784, 256, T, (0, 1, 2), None),
        "m0": lambda: Workload("m0: 30 | 256-256-256 -> 784, 6000 chains, layers=(0,) (256 columns), pooled", cfg_m, 784, 6000, T, (0,), "chains"),
        "m3": lambda: Workload("m3: 30 | 256-256-256 -> 784, 6000 chains, all layers (768 columns), pooled", cfg_m, 784, 6000, T, (0, 1, 2), "chains"),
    }


def kernel_alone(say):
    """cov_accumulate by itself (HIP events) on 64 records of each workload's shape."""
    from montecarlopredictivecoding_amd.engine import cov_accumulate, cov_workspace_bytes
    say("# cov_accumulate alone, 64 records per call; HIP events, min of 3 after a warm-up; MFMAs = row groups x tile pairs")
    for name, widths, B, pool in (("g", (6, 16, 16), 4096, True), ("a0", (20,), 256, False), ("a3", (20, 128, 128), 256, False),
                                  ("m0", (256,), 6000, True), ("m3", (256, 256, 256), 6000, True)):
        n = 64
        recs = [torch.randn(n, B, w, device=DEV) for w in widths]
        D = sum(widths)
        out = torch.zeros(*((D, D) if pool else (B, D, D)), dtype=torch.float64, device=DEV)
        ws = torch.empty(max(cov_workspace_bytes(B, widths, pool=pool), 8), dtype=torch.uint8, device=DEV) if pool else None
        ts = []
        for _ in range(4):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            cov_accumulate(recs, 0, 1, n, out, pool=pool, accumulate=True, workspace=ws)
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        best = min(ts[1:])
        nt = sum((w + 15) // 16 for w in widths)
        mfma = n * B / 4 * nt * (nt + 1) / 2
        say("%-3s %4d columns %5d chains  %9.3f ms  %8.2f us per record  %7.2f G MFMA/s  %6.1f GB/s of records" % (
            name, D, B, best, best * 1e3 / n, mfma / best / 1e6, 4.0 * n * B * D / best / 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="g,a0,a3,m0,m3")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--kernel-alone", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "scripts/cov_cost.py needs a GPU"
    warnings.simplefilter("ignore")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    kernel_alone(say)
    if not args.kernel_alone:
        table = workloads(args)
        for w in args.workloads.split(","):
            wl = table[w]()
            variants = ["cov", "plain", "torch"]
            got = {}
            for v in variants:
                try:
                    got[v] = wl.run(v)                                           # warm-up
                except RuntimeError as exc:                                      # (out of memory: the recorded trajectory does not fit)
                    say("# %s: %s does not run: %s" % (w, v, str(exc).splitlines()[0]))
                    variants = [x for x in variants if x != v]
            if "cov" not in variants or "plain" not in variants:                 # nothing to compare: only the recording call may be missing
                say("# %s: skipped" % wl.name)
                del wl, got
                torch.cuda.empty_cache()
                continue
            times = {v: [] for v in variants}
            for _ in range(args.repeats):
                for v in variants:
                    times[v].append(wall_ms(lambda: wl.run(v))[0])
            say("# %s, T = %d, %d samples per chain" % (wl.name, wl.T, wl.n))
            say("#   %d slice(s) of the record ring; ms per call, min (max) of %d" % (wl.slices, args.repeats))
            for v in variants:
                say("%-6s %9.2f (%9.2f) ms" % (v, min(times[v]), max(times[v])))
            cov, plain = min(times["cov"]), min(times["plain"])
            say("cov - plain = %.2f ms = %.1f %% of the plain call, %.2f us per sample step" % (
                cov - plain, 100 * (cov - plain) / plain, (cov - plain) * 1e3 / wl.n))
            if "torch" in variants:
                say("torch / cov = %.2f" % (min(times["torch"]) / cov))
                (s1, o1), (s2, o2) = got["cov"], got["torch"]
                say("largest difference of outer between the two ways, relative to its largest entry: %.2e" % (
                    (o1 - o2).abs().max() / o2.abs().max()).item())
            del wl, got
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Posterior histograms counted on the device (csrc/mcpc_hist.h, PCTrainer.mcpc_histogram) against the moments kernel on the same
records and against the two other ways to run the same call (developer measurement for DESIGN.md section 7, profiles/hist_cost.txt).

    python scripts/hist_cost.py [--workloads g,a0,a3,m0] [--repeats 3] [--T 1000] [--bins 50] [--out FILE]
    python scripts/hist_cost.py --part kernel|g|a0|a3|m0       # one part, in this process

Without --part the script only drives: every part runs in a child process of its own under a time limit (--limit seconds), one after the
other, and the first part that fails or runs out of time ends the run; --out FILE replaces FILE with what the parts printed.

Part `kernel`: hist_accumulate alone, 64 records per call, in GB/s of records, beside moments_accumulate with sumsq ON THE SAME RECORDS
(it reads the same bytes: the yardstick); HIP events, min of 3 after a warm-up.  Shapes as in scripts/cov_cost.py:
  g   6-16-16 at 4096 chains, all layers, pooled           a0  20 units at 256 chains, per chain
  a3  20-128-128 at 256 chains, all layers, per chain      m0  256 units at 6000 chains, pooled
plus a3L, a3 with 512 records per call (the counters' read-modify-write amortised over a longer chunk), and f2, figure_2.py's shape: one
unit, 256 chains, 4096 records (the record axis is split over workgroups).
Parts g, a0, a3, m0: one MCPC call of T steps through the facade (PCTrainer.train_on_batch, host work included, wall clock around
synchronised calls), the histogram over the steps from T / 5 on, --bins uniform bins on [-4, 4]:
  hist   the call with mcpc_histogram
  plain  the same call without it and without records: hist - plain is what the histogram costs
  torch  what a user does without it: record the trajectory, then bucketize + scatter_add in torch on the same GPU, chunk by chunk
Every variant is warmed up once; then the variants alternate inside each of --repeats rounds; min (max) of the rounds is reported.
A run without a GPU fails: there is no fallback."""
import argparse
import os
import subprocess
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LO, HI = -4.0, 4.0


def wall_ms(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def event_ms(fn, repeats=3):
    """min of `repeats` after a warm-up, HIP events."""
    import torch
    ts = []
    for _ in range(repeats + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return min(ts[1:])


def kernel_alone(say, bins):
    import numpy as np
    import torch
    from montecarlopredictivecoding_amd.engine import hist_accumulate, moments_accumulate
    dev = torch.device("cuda", 0)
    say("# hist_accumulate alone beside moments_accumulate (sum and sumsq) on the same records; HIP events, min of 3 after a warm-up;")
    say("# %d uniform bins on [%g, %g], values N(0, 1); GB/s of records read" % (bins, LO, HI))
    edges = np.linspace(LO, HI, bins + 1).astype(np.float32)
    for name, widths, B, pool, n in (("g", (6, 16, 16), 4096, True, 64), ("a0", (20,), 256, False, 64), ("a3", (20, 128, 128), 256, False, 64),
                                     ("m0", (256,), 6000, True, 64), ("a3L", (20, 128, 128), 256, False, 512), ("f2", (1,), 256, True, 4096)):
        recs = [torch.randn(n, B, w, device=dev) for w in widths]
        counts = [torch.zeros(*((w, bins + 3) if pool else (B, w, bins + 3)), dtype=torch.int64, device=dev) for w in widths]
        sums = [(torch.zeros(B, w, dtype=torch.float64, device=dev), torch.zeros(B, w, dtype=torch.float64, device=dev)) for w in widths]

        def hist():
            for r, c in zip(recs, counts):
                hist_accumulate(r, 0, 1, n, edges, c, pool=pool, accumulate=True)

        def mom():
            for r, (s, q) in zip(recs, sums):
                moments_accumulate(r, 0, 1, n, s, q, accumulate=True)
        th, tm = event_ms(hist), event_ms(mom)
        gb = 4.0 * n * B * sum(widths) / 1e6
        say("%-3s %4d units %5d chains %5d records %-9s  hist %8.3f ms %7.1f GB/s   moments %8.3f ms %7.1f GB/s   hist / moments rate %.2f" % (
            name, sum(widths), B, n, "pooled" if pool else "per chain", th, gb / th, tm, gb / tm, tm / th))
        assert all(int(c.sum()) == 4 * n * B * w for c, w in zip(counts, widths))      # four timed calls, every value counted once


def torch_hist(steps, edges, pooled, dev, chunk=50):
    """Counts [.., nb + 2] (bins, then everything outside) in torch on the GPU from recorded steps: steps[k] is a list of [B, n_l] host
    tensors."""
    import torch
    nb = edges.numel() - 1
    out = None
    for k0 in range(0, len(steps), chunk):
        x = torch.stack([torch.cat(list(st), dim=1) for st in steps[k0:k0 + chunk]]).to(dev, non_blocking=True)       # [c, B, D]
        idx = torch.bucketize(x, edges, right=True) - 1
        idx = torch.where(x == edges[-1], torch.full_like(idx, nb - 1), idx)
        idx = torch.where((idx < 0) | (idx >= nb), torch.full_like(idx, nb), idx)
        c = torch.zeros(x.shape[1], x.shape[2], nb + 1, dtype=torch.int64, device=dev)
        c.scatter_add_(2, idx.permute(1, 2, 0), torch.ones_like(idx.permute(1, 2, 0)))
        out = c if out is None else out + c
    return out.sum(0) if pooled else out


def facade(say, which, T, bins, repeats):
    import torch
    import montecarlopredictivecoding_amd.predictive_coding as pc
    import montecarlopredictivecoding_amd.predictive_coding.pc_trainer as pt
    import montecarlopredictivecoding_amd.utils.model as um
    dev = torch.device("cuda", 0)
    ref, cfg_m = [20, 20, 128, 128], [30, 256, 256, 256]
    name, dims, n_out, B, layers, pool = {
        "g": ("g: 6-16-16 -> 24, 4096 chains, all layers (38 units), pooled", [6, 6, 16, 16], 24, 4096, (0, 1, 2), "chains"),
        "a0": ("a0: 20-128-128 -> 784, 256 chains, layers=(0,) (20 units), per chain", ref, 784, 256, (0,), None),
        "a3": ("a3: 20-128-128 -> 784, 256 chains, all layers (276 units), per chain", ref, 784, 256, (0, 1, 2), None),
        "m0": ("m0: 30 | 256-256-256 -> 784, 6000 chains, layers=(0,) (256 units), pooled", cfg_m, 784, 6000, (0,), "chains"),
    }[which]
    mods = []
    for i in range(1, len(dims)):
        mods += [torch.nn.Linear(dims[i - 1], dims[i]), pc.PCLayer(sample_x_fn=um.sample_x_fn_normal), torch.nn.ReLU()]
    model = torch.nn.Sequential(*mods, torch.nn.Linear(dims[-1], n_out)).to(dev)
    model.train()
    data = (torch.rand(B, n_out, device=dev) < 0.3).float()
    inputs = torch.zeros(B, dims[0], device=dev)
    tr = pc.PCTrainer(model, T=T, optimizer_x_fn=torch.optim.SGD, optimizer_x_kwargs={"lr": 0.01}, update_p_at="never", plot_progress_at=[])
    begin = T // 5
    all_layers = len(layers) == len(dims) - 1
    slices = [0]

    def run(variant):
        torch.manual_seed(3)                                 # every run draws the same x0 and the same Langevin noise
        pt._PHILOX_STEPS[0] = 0
        kw = dict(inputs=inputs, loss_fn=um.bernoulli_fn, loss_fn_kwargs={"_target": data, "_var": None},
                  callback_after_t=um.random_step, callback_after_t_kwargs={"_pc_trainer": tr}, is_log_progress=False,
                  is_checking_after_callback_after_t=False)
        tr.mcpc_histogram = dict(begin=begin, layers=layers, bins=bins, range=(LO, HI), pool=pool) if variant == "hist" else None
        if variant == "torch":
            if all_layers:
                r = tr.train_on_batch(is_return_results_every_t=True, is_return_xs=True, **kw)
                steps = r["xs"][begin:]
            else:
                r = tr.train_on_batch(is_return_results_every_t=True, is_return_representations=True, **kw)
                steps = [[x] for x in r["representations"][begin:]]
            edges = torch.linspace(LO, HI, bins + 1, dtype=torch.float64).to(torch.float32).to(dev)
            return torch_hist(steps, edges, pool is not None, dev)
        tr.train_on_batch(is_return_results_every_t=False, **kw)
        if variant == "hist":
            slices[0] = tr.last_record_slices
            h = tr.mcpc_last_histogram
            return torch.cat([torch.cat([h.counts[nm], (h.under[nm] + h.over[nm] + h.nan[nm]).unsqueeze(-1)], dim=-1) for nm in h.names],
                             dim=-2)
        return None

    variants = ["hist", "plain", "torch"]
    got = {}
    for v in list(variants):
        try:
            got[v] = run(v)                                                  # warm-up
        except RuntimeError as exc:                                          # (out of memory: the recorded trajectory does not fit)
            if v != "torch":
                raise
            say("# %s: %s does not run: %s" % (which, v, str(exc).splitlines()[0]))
            variants.remove(v)
    times = {v: [] for v in variants}
    for _ in range(repeats):
        for v in variants:
            times[v].append(wall_ms(lambda: run(v))[0])
    say("# %s, T = %d, %d samples per chain, %d bins" % (name, T, T - begin, bins))
    say("#   %d slice(s) of the record ring; ms per call, min (max) of %d" % (slices[0], repeats))
    for v in variants:
        say("%-6s %9.2f (%9.2f) ms" % (v, min(times[v]), max(times[v])))
    hist, plain = min(times["hist"]), min(times["plain"])
    say("hist - plain = %.2f ms = %.1f %% of the plain call, %.2f us per sample step" % (
        hist - plain, 100 * (hist - plain) / plain, (hist - plain) * 1e3 / (T - begin)))
    if "torch" in variants:
        say("torch / hist = %.2f" % (min(times["torch"]) / hist))
        say("counts that differ between the two ways: %d of %d" % (int((got["hist"] != got["torch"]).sum()), got["hist"].numel()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="g,a0,a3,m0")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--bins", type=int, default=50)
    ap.add_argument("--part", default=None)
    ap.add_argument("--limit", type=int, default=240, help="seconds a part may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.part is not None:
        import torch
        assert torch.cuda.is_available(), "scripts/hist_cost.py needs a GPU"
        warnings.simplefilter("ignore")

        def say(s):
            print(s, flush=True)
        if args.part == "kernel":
            kernel_alone(say, args.bins)
        else:
            facade(say, args.part, args.T, args.bins, args.repeats)
        return 0
    lines = []
    for part in ["kernel"] + [w for w in args.workloads.split(",") if w]:
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--T", str(args.T), "--bins", str(args.bins),
               "--repeats", str(args.repeats)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired as exc:
            print(exc.stdout or "", flush=True)
            print("# part %s ran out of its %d s: the run ends here" % (part, args.limit), flush=True)
            return 124
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:
            print("# part %s failed with status %d: the run ends here" % (part, r.returncode), flush=True)
            return r.returncode
        lines += r.stdout.splitlines()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""The rolling-window variability accumulated on the device (csrc/mcpc_roll.h, PCTrainer.mcpc_rolling): the kernel alone against its
traffic model, what the request adds to a call, and the call it replaces (developer measurement for DESIGN.md section 7,
profiles/roll_cost.txt).

    python scripts/roll_cost.py [--repeats 3] [--T 8000] [--window 1000] [--out FILE]
    python scripts/roll_cost.py --part kernel|call        # one part, in this process

Without --part the script only drives: every part runs in a child process of its own under a time limit (--limit seconds), one after the
other, and the first part that fails or runs out of time ends the run; --out FILE replaces FILE with what the parts printed.

Part `kernel`: roll_accumulate alone, mid-stream, on the figure's widest layer (256 chains x 128 units) and on all 276 units as one
block, T records per call, window W, every = 1, pooled rows only; HIP events, min of 3 after a warm-up; beside moments_accumulate with
sumsq on the same records.  The traffic model: 4 B of the entering and 4 B of the leaving record per element and sample, the history
read for the call's first W samples in place of the leaving record and written for its last W (4 B each), 32 B of state per element,
and 32 B per workgroup and row written to the workspace and read back.
Part `call`: one inference-only MCPC call of T steps on the figure's net (20 | 128-128 -> 784, ReLU, 256 chains) through the facade
(PCTrainer.train_on_batch, host work included, wall clock around synchronised calls):
  roll   the call with mcpc_rolling = dict(layers=(0, 1, 2), window=W)
  plain  the same call without it and without records: roll - plain is what the request costs
  xs     the same call with is_return_xs=True and every step's results: every step of every layer copied to pinned host memory, which is
         what the rolling statistic needed before (pandas on the host comes on top and is not timed)
All are warmed up once; then they alternate inside each of --repeats rounds; min (max) of the rounds is reported.
A run without a GPU fails: there is no fallback."""
import argparse
import os
import subprocess
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def model_bytes(E, n, W, rows, groups):
    return 8 * n * E + 4 * min(n, W) * E + 32 * E + 2 * 32 * groups * rows + 32 * rows


def kernel_alone(say, T, W):
    import torch
    from montecarlopredictivecoding_amd.engine import moments_accumulate, roll_accumulate, roll_rows, roll_workspace_bytes
    dev = torch.device("cuda", 0)
    say("# roll_accumulate alone, mid-stream (n_seen = %d), window %d, every 1, pooled rows only, beside moments_accumulate (sum and sumsq)" % (T, W))
    say("# on the same records; HIP events, min of 3 after a warm-up; values N(0, 1); GB/s against the traffic model of the docstring")
    for name, B, w in (("x1", 256, 128), ("all", 256, 276)):
        E = B * w
        rec = torch.randn(T, B, w, device=dev)
        s, q = torch.zeros(B, w, dtype=torch.float64, device=dev), torch.zeros(B, w, dtype=torch.float64, device=dev)
        tm = event_ms(lambda: moments_accumulate(rec, 0, 1, T, s, q, accumulate=True))
        s1, s2 = torch.zeros(B, w, dtype=torch.float64, device=dev), torch.zeros(B, w, dtype=torch.float64, device=dev)
        hist = torch.randn(W, B, w, device=dev)
        rows = roll_rows(T, T, W, 1)
        pool = torch.zeros(rows, 4, dtype=torch.float64, device=dev)
        ws = torch.empty(roll_workspace_bytes(B, w, T), dtype=torch.uint8, device=dev)
        tr = event_ms(lambda: roll_accumulate(rec, 0, 1, T, W, 1, T, s1, s2, hist, out_pool=pool, workspace=ws))
        groups = -(-(E // 4) // 256)
        gb = model_bytes(E, T, W, rows, groups) / 1e6
        say("%-3s %4d units %4d chains %5d records  moments %8.3f ms %7.1f GB/s of records   roll %8.3f ms %7.1f GB/s of the model (%.1f MB), "
            "%.3f us per sample, roll / moments time %.2f" % (name, w, B, T, tm, 4e-6 * T * E / tm, tr, gb / tr, gb, tr * 1e3 / T, tr / tm))
        del rec, hist, pool, ws


def facade(say, T, W, repeats):
    import torch
    import montecarlopredictivecoding_amd.predictive_coding as pc
    import montecarlopredictivecoding_amd.predictive_coding.pc_trainer as pt
    import montecarlopredictivecoding_amd.utils.model as um
    dev = torch.device("cuda", 0)
    dims, n_out, B = [20, 128, 128], 784, 256
    mods = []
    for i in range(len(dims)):
        mods += [torch.nn.Linear(dims[i - 1] if i else dims[0], dims[i]), pc.PCLayer(sample_x_fn=um.sample_x_fn_normal), torch.nn.ReLU()]
    model = torch.nn.Sequential(*mods, torch.nn.Linear(dims[-1], n_out)).to(dev)
    model.train()
    data = (torch.rand(B, n_out, device=dev) < 0.3).float()
    inputs = torch.zeros(B, dims[0], device=dev)
    tr = pc.PCTrainer(model, T=T, optimizer_x_fn=torch.optim.SGD, optimizer_x_kwargs={"lr": 0.05}, update_p_at="never", plot_progress_at=[])
    slices = [0]

    def run(variant):
        torch.manual_seed(3)                                 # every run draws the same x0 and the same Langevin noise
        pt._PHILOX_STEPS[0] = 0
        tr.mcpc_rolling = dict(layers=(0, 1, 2), window=W) if variant == "roll" else None
        res = tr.train_on_batch(inputs=inputs, loss_fn=um.bernoulli_fn, loss_fn_kwargs={"_target": data, "_var": 0.3},
                                callback_after_t=um.random_step, callback_after_t_kwargs={"_pc_trainer": tr}, is_log_progress=False,
                                is_checking_after_callback_after_t=False, is_return_results_every_t=variant == "xs",
                                is_return_xs=variant == "xs")
        if variant == "roll":
            slices[0] = tr.last_record_slices
            return tr.mcpc_last_rolling
        return len(res["xs"]) if variant == "xs" else None

    variants = ["roll", "plain", "xs"]
    got = {v: run(v) for v in variants}                                              # warm-up
    times = {v: [] for v in variants}
    for _ in range(repeats):
        for v in variants:
            times[v].append(wall_ms(lambda: run(v))[0])
    say("# figure 5: 20 | 20-128-128 -> 784, 256 chains, inference only, T = %d, layers=(0, 1, 2) (276 units), window = %d, every = 1" % (T, W))
    say("#   %d slice(s) of the record ring; ms per call, min (max) of %d; xs: %.2f GB to pinned host memory" % (
        slices[0], repeats, 4e-9 * T * B * sum(dims)))
    for v in variants:
        say("%-6s %9.2f (%9.2f) ms" % (v, min(times[v]), max(times[v])))
    roll, plain, xs = (min(times[v]) for v in variants)
    say("roll - plain = %.2f ms = %.1f %% of the plain call, %.2f us per sample step;  xs - plain = %.2f ms = %.1f %%" % (
        roll - plain, 100 * (roll - plain) / plain, (roll - plain) * 1e3 / T, xs - plain, 100 * (xs - plain) / plain))
    a = got["roll"].all()
    m = a.mean_std("all")
    say("%d rows; mean rolling sd over %d series: first row %.4f, last row %.4f, sem of the last %.2e" % (
        a.rows, int(a.count("all")[0]), float(m[0]), float(m[-1]), float(a.sem("all")[-1])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--T", type=int, default=8000)
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--part", default=None)
    ap.add_argument("--limit", type=int, default=240, help="seconds a part may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.part is not None:
        import torch
        assert torch.cuda.is_available(), "scripts/roll_cost.py needs a GPU"
        warnings.simplefilter("ignore")

        def say(s):
            print(s, flush=True)
        if args.part == "kernel":
            kernel_alone(say, args.T, args.window)
        else:
            facade(say, args.T, args.window, args.repeats)
        return 0
    lines = []
    for part in ("kernel", "call"):
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--T", str(args.T), "--window", str(args.window),
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

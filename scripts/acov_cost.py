#!/usr/bin/env python3
"""Lagged autocovariances accumulated on the device (csrc/mcpc_acov.h, PCTrainer.mcpc_autocovariance): the kernel alone beside the
moments kernel on the same records, and what the request adds to a call (developer measurement for DESIGN.md section 7,
profiles/acov_cost.txt).

    python scripts/acov_cost.py [--repeats 3] [--T 5000] [--begin 1000] [--max-lag 32] [--out FILE]
    python scripts/acov_cost.py --part kernel|m1        # one part, in this process

Without --part the script only drives: every part runs in a child process of its own under a time limit (--limit seconds), one after the
other, and the first part that fails or runs out of time ends the run; --out FILE replaces FILE with what the parts printed.

Part `kernel`: acov_accumulate alone on cfg-M's layer-1 shape (m1: 6000 chains x 256 units) and on a3 (256 chains x 276 units), 128 records
per call in the steady state of a stream, for max_lag 8 / 16 / 32 / 64 (one per capacity instantiated) and 24 / 48 (lags computed and not
stored), and m1L: m1 with 512 records per call at max_lag 32 (the state's read-modify-write amortised over a longer chunk); HIP events,
min of 3 after a warm-up.  Reported: GB/s of records read, fp64 FMA/s that the result needs (records x elements x (max_lag +
1)) and that the instantiation executes (capacity + 1), beside moments_accumulate with sumsq ON THE SAME RECORDS (it reads the same
bytes: the yardstick).
Part `m1`: one inference-only MCPC call of T steps on cfg-M's net (30 | 256-256-256 -> 784, 6000 chains) through the facade
(PCTrainer.train_on_batch, host work included, wall clock around synchronised calls):
  acov   the call with mcpc_autocovariance = dict(begin, layers=(1,), max_lag)
  plain  the same call without it and without records: acov - plain is what the request costs
Both are warmed up once; then they alternate inside each of --repeats rounds; min (max) of the rounds is reported.
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


def kernel_alone(say):
    import torch
    from montecarlopredictivecoding_amd.engine import acov_accumulate, moments_accumulate
    dev = torch.device("cuda", 0)
    say("# acov_accumulate alone, mid-stream (n_seen = 1000), beside moments_accumulate (sum and sumsq) on the same records; HIP events,")
    say("# min of 3 after a warm-up; values N(0, 1); GB/s of records read; GFMA/s fp64: needed = records x elements x (max_lag + 1),")
    say("# executed = records x elements x (capacity + 1)")
    for name, B, w, n, lags in (("m1", 6000, 256, 128, (8, 16, 24, 32, 48, 64)), ("a3", 256, 276, 128, (8, 16, 24, 32, 48, 64)),
                                ("m1L", 6000, 256, 512, (32,))):
        rec = torch.randn(n, B, w, device=dev)
        s, q = torch.zeros(B, w, dtype=torch.float64, device=dev), torch.zeros(B, w, dtype=torch.float64, device=dev)
        tm = event_ms(lambda: moments_accumulate(rec, 0, 1, n, s, q, accumulate=True))
        gb = 4.0 * n * B * w / 1e6
        say("%-3s %4d units %5d chains %4d records  moments %8.3f ms %7.1f GB/s" % (name, w, B, n, tm, gb / tm))
        for K in lags:
            cap = 8 if K <= 8 else 16 if K <= 16 else 32 if K <= 32 else 64
            lagged = torch.zeros(B, w, K + 1, dtype=torch.float64, device=dev)
            window, head = torch.randn(K, B, w, device=dev), torch.zeros(K, B, w, device=dev)
            ta = event_ms(lambda: acov_accumulate(rec, 0, 1, n, K, 1000, lagged, s, window, head))
            fma = 1e-6 * n * B * w
            say("%-3s max_lag %2d (capacity %2d)  acov %8.3f ms %7.1f GB/s  %8.1f GFMA/s needed %8.1f executed   acov / moments time %.2f" % (
                name, K, cap, ta, gb / ta, fma * (K + 1) / ta, fma * (cap + 1) / ta, ta / tm))
            del lagged, window, head


def facade(say, T, begin, max_lag, repeats):
    import torch
    import montecarlopredictivecoding_amd.predictive_coding as pc
    import montecarlopredictivecoding_amd.predictive_coding.pc_trainer as pt
    import montecarlopredictivecoding_amd.utils.model as um
    dev = torch.device("cuda", 0)
    dims, n_out, B = [30, 256, 256, 256], 784, 6000
    mods = []
    for i in range(1, len(dims)):
        mods += [torch.nn.Linear(dims[i - 1], dims[i]), pc.PCLayer(sample_x_fn=um.sample_x_fn_normal), torch.nn.ReLU()]
    model = torch.nn.Sequential(*mods, torch.nn.Linear(dims[-1], n_out)).to(dev)
    model.train()
    data = (torch.rand(B, n_out, device=dev) < 0.3).float()
    inputs = torch.zeros(B, dims[0], device=dev)
    tr = pc.PCTrainer(model, T=T, optimizer_x_fn=torch.optim.SGD, optimizer_x_kwargs={"lr": 0.01}, update_p_at="never", plot_progress_at=[])
    slices = [0]

    def run(variant):
        torch.manual_seed(3)                                 # every run draws the same x0 and the same Langevin noise
        pt._PHILOX_STEPS[0] = 0
        tr.mcpc_autocovariance = dict(begin=begin, layers=(1,), max_lag=max_lag) if variant == "acov" else None
        tr.train_on_batch(inputs=inputs, loss_fn=um.bernoulli_fn, loss_fn_kwargs={"_target": data, "_var": None},
                          callback_after_t=um.random_step, callback_after_t_kwargs={"_pc_trainer": tr}, is_log_progress=False,
                          is_checking_after_callback_after_t=False, is_return_results_every_t=False)
        if variant == "acov":
            slices[0] = tr.last_record_slices
            return tr.mcpc_last_autocovariance
        return None

    variants = ["acov", "plain"]
    got = {v: run(v) for v in variants}                                              # warm-up
    times = {v: [] for v in variants}
    for _ in range(repeats):
        for v in variants:
            times[v].append(wall_ms(lambda: run(v))[0])
    n = T - begin
    say("# m1: 30 | 256-256-256 -> 784, 6000 chains, inference only, T = %d, layers=(1,) (256 units), max_lag = %d, %d samples per chain"
        % (T, max_lag, n))
    say("#   %d slice(s) of the record ring; ms per call, min (max) of %d" % (slices[0], repeats))
    for v in variants:
        say("%-6s %9.2f (%9.2f) ms" % (v, min(times[v]), max(times[v])))
    acov, plain = min(times["acov"]), min(times["plain"])
    say("acov - plain = %.2f ms = %.1f %% of the plain call, %.2f us per sample step" % (
        acov - plain, 100 * (acov - plain) / plain, (acov - plain) * 1e3 / n))
    a = got["acov"]
    tau = a.tau("x1")
    ok = torch.isfinite(tau)
    say("tau of x1 over %d (chain, unit) pairs: median %.2f, 90 %% %.2f, truncated at max_lag: %.1f %%; ESS median %.0f of %d samples" % (
        int(ok.sum()), float(tau[ok].median()), float(tau[ok].quantile(0.9)), 100 * float(a.truncated("x1").double().mean()),
        float(a.ess("x1")[ok].median()), n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--T", type=int, default=5000)
    ap.add_argument("--begin", type=int, default=1000)
    ap.add_argument("--max-lag", type=int, default=32)
    ap.add_argument("--part", default=None)
    ap.add_argument("--limit", type=int, default=240, help="seconds a part may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.part is not None:
        import torch
        assert torch.cuda.is_available(), "scripts/acov_cost.py needs a GPU"
        warnings.simplefilter("ignore")

        def say(s):
            print(s, flush=True)
        if args.part == "kernel":
            kernel_alone(say)
        else:
            facade(say, args.T, args.begin, args.max_lag, args.repeats)
        return 0
    lines = []
    for part in ("kernel", "m1"):
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--T", str(args.T), "--begin", str(args.begin),
               "--max-lag", str(args.max_lag), "--repeats", str(args.repeats)]
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

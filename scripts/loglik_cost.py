#!/usr/bin/env python3
"""The per-datum log marginal likelihood on the device (csrc/mcpc_loglik.h, likelihood.py): what the kernel costs alone, what the
front costs end to end, what the eager fp32 evaluator costs on the same GPU, and how far the two results are apart (developer
measurement for DESIGN.md section 7, profiles/loglik_cost.txt).

    python scripts/loglik_cost.py [--repeats 3] [--out FILE]
    python scripts/loglik_cost.py --part kernel|front|eager      # one part, in this process

Without --part the script only drives: every part runs in a child process of its own under a time limit (--limit seconds), one after
the other, and the first that fails or runs out of time ends the run; --out FILE replaces FILE with what the parts printed.

The shape is table_1.py's: 10 000 data x 5 000 prior samples x 784 pixels, Bernoulli read-out, clamp 20.  The inputs are seeded:
binary data and the logits of a random 20-unit linear read-out (what matters to the cost is the shape; what matters to the fp32 gap
is that the nll are sums of 784 terms of the size a trained model's are).

  kernel  loglik_accumulate alone (HIP events; the workspace allocated outside the timed window), both read-outs: the three launches
          of one call, and the fp64 MFMA rate the contraction achieves beside the chip's 78.6e12 flop/s.
  front   likelihood.log_likelihood end to end on device tensors (wall clock around synchronised calls): state and workspace
          allocated, one call; and streamed in ten chunks of 500 samples.
  eager   utils.training_evaluation.marginal_likelihood_from_logits on the same tensors in batches of 120 data, the reference's
          100 * 6000 / n_samples (wall clock around synchronised calls), its scalar beside the device's, and the largest absolute
          difference per datum between the fp32 arithmetic of that function (its statements, keeping the vector it sums) and the
          fp64 state.
A run without a GPU fails: there is no fallback."""
import argparse
import os
import subprocess
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TABLE1 = dict(n_data=10000, n_samp=5000, width=784, batch=120)
FP64_MFMA_RATE = 78.6e12                         # flop/s, matrix fp64, MI355X


def wall_ms(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def inputs(dev):
    import torch
    g = torch.Generator(device="cpu").manual_seed(23)
    n, s, w = TABLE1["n_data"], TABLE1["n_samp"], TABLE1["width"]
    data = (torch.rand(n, w, generator=g) < 0.13).float()
    logits = torch.randn(s, 20, generator=g) @ (1.5 * torch.randn(20, w, generator=g)) - 2.0
    return data.to(dev), logits.to(dev)


def part_kernel(say, repeats):
    import torch
    from montecarlopredictivecoding_amd.engine import loglik_accumulate, loglik_workspace_bytes
    from montecarlopredictivecoding_amd.likelihood import plan
    dev = torch.device("cuda", 0)
    data, logits = inputs(dev)
    n, s, w = TABLE1["n_data"], TABLE1["n_samp"], TABLE1["width"]
    p = plan(n, s, w)
    say("# loglik_accumulate alone, %d data x %d samples x %d, HIP events, min (max) of %d; %d datum tiles x %d groups of %d sample "
        "tiles = %d waves; workspace %d bytes" % (n, s, w, repeats, p["n_dtiles"], p["groups"], p["tiles_per_group"],
                                                 p["n_dtiles"] * p["groups"], p["workspace_bytes"]))
    for loss, var in (("bernoulli", None), ("gaussian", 0.3)):
        state = torch.empty(n, 4, dtype=torch.float64, device=dev)
        ws = torch.empty(max(loglik_workspace_bytes(n, s, w), 8), dtype=torch.uint8, device=dev)
        loglik_accumulate(data, logits, loss, var, 20.0, state, workspace=ws)          # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            loglik_accumulate(data, logits, loss, var, 20.0, state, workspace=ws)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        flop = 2.0 * n * s * w
        say("%-9s %9.3f (%9.3f) ms  %.2fe12 flop/s in the contraction = %.0f %% of the fp64 MFMA rate %.1fe12"
            % (loss, min(ms), max(ms), flop / (min(ms) * 1e-3) / 1e12, 100 * flop / (min(ms) * 1e-3) / FP64_MFMA_RATE, FP64_MFMA_RATE / 1e12))


def part_front(say, repeats):
    import torch
    from montecarlopredictivecoding_amd.likelihood import log_likelihood
    dev = torch.device("cuda", 0)
    data, logits = inputs(dev)
    w = TABLE1["width"]
    say("# likelihood.log_likelihood end to end on device tensors, wall clock around synchronised calls, min (max) of %d" % repeats)
    for what, kw in (("one call", {}), ("ten chunks of 500 samples", dict(chunk_bytes=500 * w * 4))):
        log_likelihood(data, logits, **kw)                                             # warm-up
        t = [wall_ms(lambda: log_likelihood(data, logits, **kw)) for _ in range(repeats)]
        ll = t[0][1]
        say("%-26s %9.3f (%9.3f) ms  mean log p = %.9f  ESS %.2f .. %.2f (median %.2f) of %d"
            % (what, min(m for m, _ in t), max(m for m, _ in t), ll.mean(), float(ll.ess.min()), float(ll.ess.max()),
               float(ll.ess.median()), TABLE1["n_samp"]))


def eager_per_datum(logits, batches):
    """marginal_likelihood_from_logits, statement by statement, keeping the per-datum vector it sums."""
    import torch
    logits = logits.clamp(-20, 20)
    sp = torch.nn.functional.softplus(logits).sum(1)
    out = []
    with torch.no_grad():
        for data, _ in batches:
            data = data.to(logits.device).to(logits.dtype)
            nll = sp.unsqueeze(0) - data @ logits.t()
            m = nll.min(1).values
            p = torch.exp(-(nll - m.unsqueeze(1))).mean(1)
            out.append(torch.log(p) - m)
    return torch.cat(out)


def part_eager(say, repeats):
    import torch
    from montecarlopredictivecoding_amd.likelihood import log_likelihood
    from montecarlopredictivecoding_amd.utils.training_evaluation import marginal_likelihood_from_logits
    dev = torch.device("cuda", 0)
    data, logits = inputs(dev)
    batches = [(data[i:i + TABLE1["batch"]], None) for i in range(0, data.shape[0], TABLE1["batch"])]
    say("# utils.training_evaluation.marginal_likelihood_from_logits (eager torch, fp32) on the same tensors in %d batches of %d data, "
        "wall clock around synchronised calls, min (max) of %d" % (len(batches), TABLE1["batch"], repeats))
    marginal_likelihood_from_logits(logits, batches)                                   # warm-up
    t = [wall_ms(lambda: marginal_likelihood_from_logits(logits, batches)) for _ in range(repeats)]
    scalar = t[0][1]
    ll = log_likelihood(data, logits)
    say("eager fp32 %9.3f (%9.3f) ms  mean log p = %.9f;  the device's fp64: %.9f;  difference of the scalars %.3g"
        % (min(m for m, _ in t), max(m for m, _ in t), scalar, ll.mean(), abs(scalar - ll.mean())))
    per = eager_per_datum(logits, batches).double()
    gap = (per - ll.log_p).abs()
    say("per datum, fp32 statements against the fp64 state: largest |difference| %.3g nats, median %.3g (the mean of the fp32 vector "
        "is %.9f)" % (float(gap.max()), float(gap.median()), float(per.mean())))


PARTS = {"kernel": part_kernel, "front": part_front, "eager": part_eager}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--part", default=None, choices=sorted(PARTS))
    ap.add_argument("--limit", type=int, default=240, help="seconds a part may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.part is not None:
        import torch
        assert torch.cuda.is_available(), "scripts/loglik_cost.py needs a GPU"
        warnings.simplefilter("ignore")

        def say(s):
            print(s, flush=True)
        PARTS[args.part](say, args.repeats)
        return 0
    lines = []
    for part in ("kernel", "front", "eager"):
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--repeats", str(args.repeats)]
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

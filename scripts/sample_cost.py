#!/usr/bin/env python3
"""Ancestral samples on the device (csrc/mcpc_ancestral.h): what `sample_pc_device` costs beside the torch `sample_pc` it stands in for,
on the same GPU, and what that does to `get_marginal_likelihood_per_datum` end to end (developer measurement for DESIGN.md section 7,
profiles/sample_cost.txt).

    python scripts/sample_cost.py [--out FILE]
    python scripts/sample_cost.py --part sampler|kernel|likelihood      # one part, in this process

Without --part the script only drives: every part runs in a child process of its own under a time limit (--limit seconds), one after
the other, and the first that fails or runs out of time ends the run; --out FILE replaces FILE with what the parts printed.

Nets (n_in - latents - n_out, relu, torch's default initialisation, seeded): 20-128-128-784 and 30-256-256-784.  Every figure is the
median of timed calls after a warm-up call, wall clock around synchronised calls unless it says HIP events.

  sampler     sample_pc_device(is_return_hidden=True) and sample_pc(is_return_hidden=True) for n = 5 000, 100 000 and 1 000 000 samples,
              the last in ten chunks of 100 000 (the device chunks advance sample_base; each chunk's tensor is dropped before the next).
  kernel      Engine.sample_prior alone (HIP events, the output allocated outside the timed window), with the roofline beside it: the
              bytes the read-out writes, n x n_out x 4, against the 4.5 TB/s a streaming store reaches, and the fp32-equivalent GEMM
              work, 2 n sum_j n_{j-1} n_j, against the 98e12 flop/s the 64 x 128 tile reaches on three fp16 MFMAs per product
              (Kce).
  likelihood  get_marginal_likelihood_per_datum end to end, 10 000 data x 5 000 samples, with sampler="torch" and sampler="device".
A run without a GPU fails: there is no fallback."""
import argparse
import os
import statistics
import subprocess
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NETS = ((20, (128, 128), 784), (30, (256, 256), 784))
SIZES = ((5000, 1, 5), (100000, 1, 3), (1000000, 10, 3))          # samples, chunks, timed calls
STORE_RATE, TILE_RATE = 4.5e12, 98e12


def median_ms(fn, repeats):
    import torch
    fn()                                                           # warm-up
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ms)


def make_model(n_in, sizes, n_out, dev):
    import torch
    from montecarlopredictivecoding_amd import predictive_coding as pc
    from montecarlopredictivecoding_amd.utils.model import bernoulli_fn
    torch.manual_seed(1)
    mods, below = [], n_in
    for n in sizes:
        mods += [torch.nn.Linear(below, n), pc.PCLayer(), torch.nn.ReLU()]
        below = n
    mods.append(torch.nn.Linear(below, n_out))
    return torch.nn.Sequential(*mods).to(dev), dict(input_size=n_in, loss_fn=bernoulli_fn, input_var=0.3)


def name_of(net):
    return "%d-%s-%d" % (net[0], "-".join(map(str, net[1])), net[2])


def part_sampler(say):
    import torch
    from montecarlopredictivecoding_amd.utils.training_evaluation import sample_pc, sample_pc_device
    dev = torch.device("cuda", 0)
    say("# sample_pc_device(hidden) beside sample_pc(hidden), one MI355X, %d CPU threads for torch; median wall-clock ms" % torch.get_num_threads())
    say("# %-16s %9s %7s %12s %12s %8s" % ("net", "samples", "chunks", "device ms", "torch ms", "ratio"))
    for net in NETS:
        model, cfg = make_model(*net, dev)
        for n, chunks, repeats in SIZES:
            per = n // chunks

            def on_device():
                for k in range(chunks):
                    sample_pc_device(per, model, cfg, is_return_hidden=True, seed=9, sample_base=k * per)

            def on_torch():
                for _ in range(chunks):
                    sample_pc(per, model, cfg, use_cuda=True, is_return_hidden=True)
            d, t = median_ms(on_device, repeats), median_ms(on_torch, repeats)
            say("%-18s %9d %7d %12.3f %12.3f %8.1f" % (name_of(net), n, chunks, d, t, t / d))


def part_kernel(say):
    import torch
    from montecarlopredictivecoding_amd.engine import Engine
    dev = torch.device("cuda", 0)
    say("# Engine.sample_prior(hidden) alone, HIP events, median of 5; roofline: the read-out's stores at %.1f TB/s, the GEMMs at %.0fe12 "
        "flop/s" % (STORE_RATE / 1e12, TILE_RATE / 1e12))
    say("# %-16s %9s %10s %12s %12s" % ("net", "samples", "ms", "stores ms", "GEMM ms"))
    for net in NETS:
        n_in, sizes, n_out = net
        model, _ = make_model(*net, dev)
        lins = [m for m in model if isinstance(m, torch.nn.Linear)]
        eng = Engine(list(sizes), [1] * len(sizes), n_in, n_out, 64, device=dev)
        eng.bind_params([m.weight.data for m in lins], [m.bias.data for m in lins])
        dims = list(sizes) + [n_out]
        for n in (5000, 100000):
            out = torch.empty(n, n_out, device=dev)
            eng.sample_prior(n, 9, out=out)
            torch.cuda.synchronize()
            ms = []
            for _ in range(5):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                eng.sample_prior(n, 9, out=out)
                b.record()
                torch.cuda.synchronize()
                ms.append(a.elapsed_time(b))
            flop = 2.0 * n * sum(i * o for i, o in zip(dims[:-1], dims[1:]))
            say("%-18s %9d %10.3f %12.3f %12.3f" % (name_of(net), n, statistics.median(ms), n * n_out * 4 / STORE_RATE * 1e3, flop / TILE_RATE * 1e3))
        eng.close()


def part_likelihood(say):
    import torch
    from montecarlopredictivecoding_amd.utils.training_evaluation import get_marginal_likelihood_per_datum
    dev = torch.device("cuda", 0)
    model, cfg = make_model(*NETS[1], dev)
    g = torch.Generator(device="cpu").manual_seed(23)
    data = (torch.rand(10000, 784, generator=g) < 0.13).float()
    loader = [(data[i:i + 1000], None) for i in range(0, 10000, 1000)]
    say("# get_marginal_likelihood_per_datum end to end, %s, 10 000 data x 5 000 samples, median wall-clock ms of 3" % name_of(NETS[1]))
    for sampler in ("torch", "device"):
        ms = median_ms(lambda: get_marginal_likelihood_per_datum(model, cfg, loader, True, n_samples=5000, sampler=sampler, seed=9), 3)
        say("sampler=%-8s %10.3f ms" % (sampler, ms))


PARTS = {"sampler": part_sampler, "kernel": part_kernel, "likelihood": part_likelihood}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default=None, choices=sorted(PARTS))
    ap.add_argument("--limit", type=int, default=360, help="seconds a part may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.part is not None:
        import torch
        assert torch.cuda.is_available(), "scripts/sample_cost.py needs a GPU"
        warnings.simplefilter("ignore")

        def say(s):
            print(s, flush=True)
        PARTS[args.part](say)
        return 0
    lines = []
    for part in ("kernel", "sampler", "likelihood"):
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part]
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

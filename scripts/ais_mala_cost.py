#!/usr/bin/env python3
"""What Metropolis-adjusted transitions cost annealed importance sampling on the device (csrc/mcpc_mala.h, ais.py): developer
measurement for DESIGN.md section 7, profiles/ais_mala_cost.txt.

    python scripts/ais_mala_cost.py [--reps 7] [--data 93] [--out profiles/ais_mala_cost.txt]
    python scripts/ais_mala_cost.py --count STEPS          (one small adjusted call, for a kernel trace: see below)

The reference's table_1 net (20-128-128-784, ReLU, Bernoulli read-out, lr 0.1) with seeded weights and binary data, one process.
`utils.training_evaluation.get_marginal_likelihood_ais` at 64 replicas x 64 stages x 5 steps on --data data (93: one chunk of 5952
chains at the default max_chains), without and with adjust="mala", ALTERNATING, each call's wall time from its start to the end of a
torch.cuda.synchronize(); the median (min .. max) of --reps calls each after one warm-up call of each.  Then the acceptance per rung of
one adjusted PCTrainer.mcpc_ais call on the same data.  The unadjusted figure is also what a checkout WITHOUT the adjusted mode prints
(`adjust` is passed only when it is asked for), so the script measures the parent commit unchanged.

Launches per adjusted step: run the script twice under a kernel trace with `--count 4` and `--count 14` (stages = 2: one rung with
transitions, 16 chains) and divide the difference of the numbers of traced kernels by 10.  A run without a GPU fails."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NET = dict(n_in=20, hidden=128, n_out=784, lr=0.1)
RUN = dict(replicas=64, stages=64, steps_per_stage=5)


def build(dev):
    import torch
    import torch.nn as nn
    from montecarlopredictivecoding_amd import predictive_coding as pc
    from montecarlopredictivecoding_amd.utils import model as um
    torch.manual_seed(97)
    h = NET["hidden"]
    model = nn.Sequential(nn.Linear(NET["n_in"], h), pc.PCLayer(), nn.ReLU(), nn.Linear(h, h), pc.PCLayer(), nn.ReLU(),
                          nn.Linear(h, NET["n_out"])).to(dev)
    model.train()
    config = dict(loss_fn=um.bernoulli_fn, input_var=None, input_size=NET["n_in"], mixing=50, sampling=100,
                  optimizer_x_kwargs_mcpc={"lr": NET["lr"]})
    return model, config, um


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--data", type=int, default=93)
    ap.add_argument("--count", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "scripts/ais_mala_cost.py needs a GPU"
    from montecarlopredictivecoding_amd import predictive_coding as pc
    from montecarlopredictivecoding_amd.utils.training_evaluation import get_marginal_likelihood_ais
    dev = torch.device("cuda", 0)
    model, config, um = build(dev)
    g = torch.Generator().manual_seed(5)
    trainer = pc.PCTrainer(model, T=4, optimizer_x_fn=torch.optim.SGD, optimizer_x_kwargs={"lr": NET["lr"]}, update_p_at="never",
                           plot_progress_at=[])
    if args.count:
        data = (torch.rand(1, NET["n_out"], generator=g) < 0.13).float().to(dev)
        trainer.mcpc_ais(data, um.bernoulli_fn, {}, replicas=16, stages=2, steps_per_stage=args.count, adjust="mala")
        torch.cuda.synchronize()
        print("one adjusted call: 16 chains, 2 stages (one rung with transitions), %d steps" % args.count)
        return 0
    data = (torch.rand(args.data, NET["n_out"], generator=g) < 0.13).float()
    loader = [(data, None)]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    has_adjust = "adjust" in pc.PCTrainer.mcpc_ais.__code__.co_varnames
    modes = [None, "mala"] if has_adjust else [None]

    def call(adjust):
        kw = {} if adjust is None else {"adjust": adjust}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ll = get_marginal_likelihood_ais(model, config, loader, True, **RUN, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, ll

    times = {m: [] for m in modes}
    for m in modes:
        call(m)                                                          # warm-up: engines, scratch, the allocator's pools
    for _ in range(args.reps):
        for m in modes:                                                  # alternating
            times[m].append(call(m)[0])
    say("# %d-%d-%d-%d ReLU, Bernoulli, lr %.2f; %d data x %d replicas = %d chains, %d stages x %d steps; wall time of "
        "get_marginal_likelihood_ais incl. a final synchronize, median (min .. max) of %d alternating calls, ms" % (
            NET["n_in"], NET["hidden"], NET["hidden"], NET["n_out"], NET["lr"], args.data, RUN["replicas"], args.data * RUN["replicas"],
            RUN["stages"], RUN["steps_per_stage"], args.reps))
    for m in modes:
        t = times[m]
        say("adjust=%-6s  %9.1f (%9.1f .. %9.1f) ms" % (m, statistics.median(t), min(t), max(t)))
    if has_adjust:
        say("adjusted / unadjusted = %.2f" % (statistics.median(times["mala"]) / statistics.median(times[None])))
        plain = trainer.mcpc_ais(data.to(dev), um.bernoulli_fn, {}, **RUN)
        ll = trainer.mcpc_ais(data.to(dev), um.bernoulli_fn, {}, adjust="mala", **RUN)
        acc = trainer.mcpc_last_ais_acceptance.cpu().numpy()
        say("acceptance per rung: min %.3f  median %.3f  max %.3f" % (acc.min(), statistics.median(acc.tolist()), acc.max()))
        say("  rungs 1..%d: %s" % (len(acc), " ".join("%.3f" % a for a in acc)))
        say("mean log p: unadjusted %.3f  adjusted %.3f; mean ESS of %d: unadjusted %.1f  adjusted %.1f" % (
            plain.mean(), ll.mean(), RUN["replicas"], float(plain.ess.mean()), float(ll.ess.mean())))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

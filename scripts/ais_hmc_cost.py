#!/usr/bin/env python3
"""What one Hamiltonian trajectory of five leapfrog steps per rung costs annealed importance sampling on the device against five MALA
steps per rung (csrc/mcpc_hmc.h, csrc/mcpc_mala.h, ais.py): developer measurement for DESIGN.md section 7, profiles/ais_hmc_cost.txt.

    python scripts/ais_hmc_cost.py [--reps 7] [--data 93] [--out profiles/ais_hmc_cost.txt]

The reference's table_1 net (20-128-128-784, ReLU, Bernoulli read-out, lr 0.1) with seeded weights and binary data of MNIST's size,
one process.  `utils.training_evaluation.get_marginal_likelihood_ais` at 64 replicas x 64 stages on --data data (93: one chunk of
5952 chains at the default max_chains) with adjust="mala", steps_per_stage=5 and with adjust="mala", leapfrog=5, steps_per_stage=1:
five gradient evaluations per rung either way, five energy evaluations against one.  ALTERNATING, each call's wall time from its
start to the end of a torch.cuda.synchronize(); the median (min .. max) of --reps calls each after one warm-up call of each.  The
MALA figure is also what a checkout WITHOUT `leapfrog` prints (the keyword is passed only when asked for), so the script measures
the parent commit unchanged.  Then the mean acceptance, the mean log p and the final ESS of one call of each kind.  A run without a
GPU fails."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.ais_mala_cost import NET, RUN, build      # noqa: E402  (the same net, the same run)

MODES = {"mala x 5": dict(steps_per_stage=5), "leapfrog 5": dict(steps_per_stage=1, leapfrog=5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--data", type=int, default=93)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "scripts/ais_hmc_cost.py needs a GPU"
    from montecarlopredictivecoding_amd import predictive_coding as pc
    from montecarlopredictivecoding_amd.utils.training_evaluation import get_marginal_likelihood_ais
    dev = torch.device("cuda", 0)
    model, config, um = build(dev)
    g = torch.Generator().manual_seed(5)
    trainer = pc.PCTrainer(model, T=4, optimizer_x_fn=torch.optim.SGD, optimizer_x_kwargs={"lr": NET["lr"]}, update_p_at="never",
                           plot_progress_at=[])
    data = (torch.rand(args.data, NET["n_out"], generator=g) < 0.13).float()
    loader = [(data, None)]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    has = "leapfrog" in pc.PCTrainer.mcpc_ais.__code__.co_varnames
    modes = [m for m in MODES if has or "leapfrog" not in MODES[m]]
    run = dict(RUN)
    run.pop("steps_per_stage")

    def call(mode):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ll = get_marginal_likelihood_ais(model, config, loader, True, adjust="mala", **run, **MODES[mode])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, ll

    times = {m: [] for m in modes}
    for m in modes:
        call(m)                                                          # warm-up: engines, scratch, the allocator's pools
    for _ in range(args.reps):
        for m in modes:                                                  # alternating
            times[m].append(call(m)[0])
    say("# %d-%d-%d-%d ReLU, Bernoulli, lr %.2f; %d data x %d replicas = %d chains, %d stages, adjust=mala, five gradient evaluations "
        "per rung; wall time of get_marginal_likelihood_ais incl. a final synchronize, median (min .. max) of %d alternating calls, ms" % (
            NET["n_in"], NET["hidden"], NET["hidden"], NET["n_out"], NET["lr"], args.data, run["replicas"], args.data * run["replicas"],
            run["stages"], args.reps))
    base = statistics.median(times[modes[0]])
    for m in modes:
        t = times[m]
        say("%-11s %-36s %9.1f (%9.1f .. %9.1f) ms   x %.3f of %s" % (
            m, " ".join("%s=%d" % kv for kv in MODES[m].items()), statistics.median(t), min(t), max(t), statistics.median(t) / base, modes[0]))
    say("# one call each: the acceptance (mean over the rungs), the mean log p and the final ESS of %d" % run["replicas"])
    for m in modes:
        ll = trainer.mcpc_ais(data.to(dev), um.bernoulli_fn, {}, adjust="mala", **run, **MODES[m])
        acc = trainer.mcpc_last_ais_acceptance
        say("%-11s acceptance %.3f (%.3f .. %.3f)  mean log p %.3f  final ESS: median %.1f (%.1f .. %.1f)" % (
            m, float(acc.mean()), float(acc.min()), float(acc.max()), ll.mean(), float(ll.ess.median()), float(ll.ess.min()),
            float(ll.ess.max())))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

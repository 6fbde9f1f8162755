#!/usr/bin/env python3
"""What resampling costs annealed importance sampling on the device (csrc/mcpc_smc.h, ais.py): developer measurement for DESIGN.md
section 7, profiles/ais_smc_cost.txt.

    python scripts/ais_smc_cost.py [--reps 7] [--data 93] [--out profiles/ais_smc_cost.txt]

The reference's table_1 net (20-128-128-784, ReLU, Bernoulli read-out, lr 0.1) with seeded weights and binary data of MNIST's size,
one process.  `utils.training_evaluation.get_marginal_likelihood_ais` at 64 replicas x 64 stages x 5 steps on --data data (93: one
chunk of 5952 chains at the default max_chains) with resample=None and with resample="systematic" at ess_threshold 0.5 and 1.0, for
both kinds of transition, ALTERNATING, each call's wall time from its start to the end of a torch.cuda.synchronize(); the median
(min .. max) of --reps calls each after one warm-up call of each.  The resample=None figure is also what a checkout WITHOUT
resampling prints (the keywords are passed only when asked for), so the script measures the parent commit unchanged.
Then the mcpc_smc_ancestors launch alone (log-weights -40 + 3 N(0, 1), threshold 1: every datum resamples), at 64 and at 4096
replicas: events around 200 times (restore the log-weights, launch) and around 200 restoring copies alone, the launch being their
difference; and the ESS trace and the final ESS of one call of each kind.  A run without a GPU fails."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.ais_mala_cost import NET, RUN, build      # noqa: E402  (the same net, the same run)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--data", type=int, default=93)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "scripts/ais_smc_cost.py needs a GPU"
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

    has = "resample" in pc.PCTrainer.mcpc_ais.__code__.co_varnames
    modes = [(adj, thr) for adj in (None, "mala") for thr in ((None, 0.5, 1.0) if has else (None,))]

    def keywords(mode):
        adj, thr = mode
        kw = {} if adj is None else {"adjust": adj}
        if thr is not None:
            kw.update(resample="systematic", ess_threshold=thr)
        return kw

    def call(mode):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ll = get_marginal_likelihood_ais(model, config, loader, True, **RUN, **keywords(mode))
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
        t, base = times[m], statistics.median(times[(m[0], None)])
        say("adjust=%-6s ess_threshold=%-5s %9.1f (%9.1f .. %9.1f) ms   x %.3f of resample=None" % (
            m[0], m[1], statistics.median(t), min(t), max(t), statistics.median(t) / base))
    if has:
        from montecarlopredictivecoding_amd.engine import smc_ancestors
        say("# mcpc_smc_ancestors alone, threshold 1 (every datum resamples), events around 200 x (restore logw, launch), us per launch")
        for R, n in ((64, 1), (64, args.data), (4096, 1), (4096, args.data)):
            src = -40.0 + 3.0 * torch.randn(n * R, dtype=torch.float64, generator=g).to(dev)
            logw, anc = src.clone(), torch.empty(n * R, dtype=torch.int32, device=dev)
            for _ in range(5):
                smc_ancestors(logw.copy_(src), R, 1.0, 1, 2, 0, ancestors=anc)
            t = {True: [], False: []}
            for _ in range(5):
                for with_launch in (True, False):                        # a resampled datum's weights are equal afterwards: restore them
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)     # before every launch, and
                    a.record()                                           # time the restoring copies alone too
                    for _ in range(200):
                        logw.copy_(src)
                        if with_launch:
                            smc_ancestors(logw, R, 1.0, 1, 2, 0, ancestors=anc)
                    b.record()
                    torch.cuda.synchronize()
                    t[with_launch].append(a.elapsed_time(b) * 1e3 / 200)
            both, copy = statistics.median(t[True]), statistics.median(t[False])
            say("replicas %4d  data %3d  copy + launch %8.1f (%8.1f .. %8.1f) us  copy alone %6.1f us  launch %8.1f us" % (
                R, n, both, min(t[True]), max(t[True]), copy, both - copy))
        say("# the ESS trace (before resampling; median over the data) and the final ESS of one call each")
        for m in modes:
            ll = trainer.mcpc_ais(data.to(dev), um.bernoulli_fn, {}, **RUN, **keywords(m))
            tr = trainer.mcpc_last_ais_resampling
            say("adjust=%-6s ess_threshold=%-5s mean log p %.3f  final ESS of %d: median %.1f (%.1f .. %.1f)" % (
                m[0], m[1], ll.mean(), RUN["replicas"], float(ll.ess.median()), float(ll.ess.min()), float(ll.ess.max())))
            if tr is not None:
                ess = tr.ess.median(dim=1).values.cpu().numpy()
                say("  resampled (rung, datum) pairs: %d of %d; median ESS at rungs 1, 8, 16, .. : %s" % (
                    int(tr.resampled.sum()), tr.resampled.numel(), " ".join("%.1f" % ess[k] for k in range(0, len(ess), 8)[:9])))
                say("  share of the data resampled per rung, rungs 1..%d: %s" % (len(ess), " ".join("%.2f" % s for s in tr.share.cpu().numpy())))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

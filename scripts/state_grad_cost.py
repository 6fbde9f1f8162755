#!/usr/bin/env python3
"""What evaluating a proposal with ONE Engine.state_gradients call saves the adjusted transitions of annealed importance sampling
(csrc/mcpc_state_grad.h, ais.py: gradients="evaluator" against "run"): developer measurement for DESIGN.md section 7,
profiles/state_grad_cost.txt.

    python scripts/state_grad_cost.py [--reps 7] [--data 93] [--out profiles/state_grad_cost.txt]
    python scripts/state_grad_cost.py --kernels 20        # the evaluator alone, for a kernel trace

Part 1.  The reference's table_1 net (20-128-128-784, ReLU, Bernoulli read-out, lr 0.1) with seeded weights and binary data of MNIST's
size, one process: scripts/ais_mala_cost.py's net and run.  `utils.training_evaluation.get_marginal_likelihood_ais` at 64 replicas x
64 stages on --data data (93: one chunk of 5952 chains) with adjust="mala", steps_per_stage=5 and with adjust="mala", leapfrog=5,
steps_per_stage=1, each under gradients="run" and gradients="evaluator": the four ALTERNATING, each call's wall time from its start
to the end of a torch.cuda.synchronize(); the median (min .. max) of --reps calls each after one warm-up call of each.  Then the mean
acceptance and the mean log p of one call of each (the two forms of a mode must agree to rounding: the evaluator's gradient is the
layer-wise kernels').

Part 2.  Engine.state_gradients alone on cfg-M's net (30 | 256-256-256 -> 784, ReLU, Bernoulli) with 16 384 rows (4 states of 4096
chains: one chunk), between two HIP events, min of 5 after a warm-up: without and with the energies, beside Engine.chain_energies and
Engine.prediction_errors(quantity="error") of the same rows.  The events bracket a whole call (mu_1, the prep launch, the two tile
launches, the finish kernel); `--kernels N` runs N calls and nothing else, for `rocprofv3 --kernel-trace --stats`, which gives the
two tile launches by themselves.  A run without a GPU fails."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.ais_mala_cost import NET, RUN, build      # noqa: E402  (the same net, the same run)

MODES = {"mala x 5": dict(steps_per_stage=5), "leapfrog 5": dict(steps_per_stage=1, leapfrog=5)}
FORMS = ("run", "evaluator")
CFG_M = dict(sizes=[256, 256, 256], n_in=30, n_out=784, B=4096, n_rec=4)


def cfg_m_engine(torch, dev):
    from montecarlopredictivecoding_amd import _lib as L
    from montecarlopredictivecoding_amd.engine import Engine
    c = CFG_M
    torch.manual_seed(4)
    eng = Engine(c["sizes"], [L.ACT_RELU] * 3, c["n_in"], c["n_out"], c["B"], device=dev)
    dims = [c["n_in"]] + c["sizes"] + [c["n_out"]]
    eng.bind_params([torch.randn(dims[j + 1], dims[j], device=dev) / dims[j] ** 0.5 for j in range(4)],
                    [0.1 * torch.randn(dims[j + 1], device=dev) for j in range(4)])
    eng.bind_target((torch.rand(c["B"], c["n_out"], device=dev) < 0.3).float())
    xs = [torch.randn(c["n_rec"], c["B"], n, device=dev) for n in c["sizes"]]
    return eng, xs, L


def alone(torch, dev, say):
    eng, xs, L = cfg_m_engine(torch, dev)
    c = CFG_M
    rows = c["n_rec"] * c["B"]
    grads = [torch.empty_like(x) for x in xs]
    table = torch.empty(c["n_rec"], c["B"], L.ENERGY_COLS, dtype=torch.float64, device=dev)
    kw = dict(loss_kind=L.LOSS_BERNOULLI)
    calls = {
        "state_gradients": lambda: eng.state_gradients(None, xs, out=grads, **kw),
        "state_gradients, energies": lambda: eng.state_gradients(None, xs, out=grads, energies_out=table, **kw),
        "chain_energies": lambda: eng.chain_energies(None, xs, out=table, **kw),
        "prediction_errors": lambda: eng.prediction_errors(None, xs, quantity="error", **kw),
    }
    # the GEMMs of a call, fp32-equivalent: forward 256x256 twice and 256x784, backward the same three transposed
    fwd = 2 * (256 * 256 * 2 + 256 * 784)
    flop = {"state_gradients": 2 * fwd, "state_gradients, energies": 2 * fwd, "chain_energies": fwd, "prediction_errors": fwd}
    say("# Engine.state_gradients alone: cfg-M's net %d | %s -> %d, ReLU, Bernoulli loss, %d rows (%d states x %d chains, one chunk); a whole "
        "call between two HIP events, min of 5 after a warm-up" % (c["n_in"], "-".join(map(str, c["sizes"])), c["n_out"], rows, c["n_rec"], c["B"]))
    for name, fn in calls.items():
        ts = []
        for _ in range(6):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        best = min(ts[1:])
        say("%-28s %8.3f ms  %6.1f ns per row  %6.1f TFLOP/s of fp32-equivalent GEMM" % (name, best, best * 1e6 / rows, flop[name] * rows / best / 1e9))
    eng.sync_check()
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--data", type=int, default=93)
    ap.add_argument("--kernels", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "scripts/state_grad_cost.py needs a GPU"
    dev = torch.device("cuda", 0)
    if args.kernels:
        eng, xs, L = cfg_m_engine(torch, dev)
        table = torch.empty(CFG_M["n_rec"], CFG_M["B"], L.ENERGY_COLS, dtype=torch.float64, device=dev)
        for _ in range(args.kernels):
            eng.state_gradients(None, xs, energies_out=table, loss_kind=L.LOSS_BERNOULLI)
        torch.cuda.synchronize()
        eng.close()
        print("%d calls of Engine.state_gradients with energies, %d rows each" % (args.kernels, CFG_M["n_rec"] * CFG_M["B"]))
        return 0
    from montecarlopredictivecoding_amd import predictive_coding as pc
    from montecarlopredictivecoding_amd.utils.training_evaluation import get_marginal_likelihood_ais
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

    run = dict(RUN)
    run.pop("steps_per_stage")
    kinds = [(m, f) for m in MODES for f in FORMS]

    def call(kind):
        mode, form = kind
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ll = get_marginal_likelihood_ais(model, config, loader, True, adjust="mala", gradients=form, **run, **MODES[mode])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, ll

    times = {k: [] for k in kinds}
    for k in kinds:
        call(k)                                                          # warm-up: engines, scratch, the allocator's pools
    for _ in range(args.reps):
        for k in kinds:                                                  # alternating
            times[k].append(call(k)[0])
    say("# %d-%d-%d-%d ReLU, Bernoulli, lr %.2f; %d data x %d replicas = %d chains, %d stages, adjust=mala, five gradient evaluations "
        "per rung; wall time of get_marginal_likelihood_ais incl. a final synchronize, median (min .. max) of %d alternating calls, ms" % (
            NET["n_in"], NET["hidden"], NET["hidden"], NET["n_out"], NET["lr"], args.data, run["replicas"], args.data * run["replicas"],
            run["stages"], args.reps))
    for mode in MODES:
        base = statistics.median(times[(mode, "run")])
        for form in FORMS:
            t = times[(mode, form)]
            say("%-11s gradients=%-10s %9.1f (%9.1f .. %9.1f) ms   x %.3f of gradients=run" % (
                mode, form, statistics.median(t), min(t), max(t), statistics.median(t) / base))
    say("# one call each: the acceptance (mean over the rungs), the mean log p and the final ESS of %d" % run["replicas"])
    for mode, form in kinds:
        ll = trainer.mcpc_ais(data.to(dev), um.bernoulli_fn, {}, adjust="mala", gradients=form, **run, **MODES[mode])
        acc = trainer.mcpc_last_ais_acceptance
        say("%-11s gradients=%-10s acceptance %.3f (%.3f .. %.3f)  mean log p %.3f  final ESS: median %.1f" % (
            mode, form, float(acc.mean()), float(acc.min()), float(acc.max()), ll.mean(), float(ll.ess.median())))
    alone(torch, dev, say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

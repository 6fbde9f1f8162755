#!/usr/bin/env python3
"""Per-chain energies evaluated on the device (csrc/mcpc_chain_energy.h, PCTrainer.mcpc_chain_energies) against the two other ways to
run the same call (developer measurement for DESIGN.md section 7, profiles/chain_energies.txt).

    python scripts/chain_energies.py [--workloads a,b] [--repeats 3] [--T-b 1000] [--out FILE]
    python scripts/chain_energies.py --only b:spec              # one warm-up and one timed call, for a kernel trace
    python scripts/chain_energies.py --kernel-alone              # Engine.chain_energies by itself, HIP events

Workloads, through the facade (PCTrainer.train_on_batch, host work included, wall clock around synchronised calls):
  a  the reference's net 20-128-128 -> 784 at 256 chains: one MCPC call of 50 + 100 steps, the trace of all 150 steps
  b  cfg-M's net 30 | 256-256-256 -> 784 at 6000 chains, one MCPC call of T = 1000, the trace from step 200
Variants:
  spec   the call with mcpc_chain_energies
  plain  the same call without it and without records: spec - plain is what the trace costs
  torch  the only way without it: is_return_xs, then the energies of the same steps in eager torch on the same GPU
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
    """Every run of a workload draws the same x0 and the same Langevin noise, so that the variants compute the same trace."""
    torch.manual_seed(3)
    pt._PHILOX_STEPS[0] = 0


def torch_energies(model, inputs, data, xs_steps, chunk=25):
    """overall [n, B] of recorded states in eager torch on the GPU: xs_steps[k][l] is x_l at the k-th step (host tensors)."""
    lins = [m for m in model if isinstance(m, torch.nn.Linear)]
    out = []
    with torch.no_grad():
        for k0 in range(0, len(xs_steps), chunk):
            part = xs_steps[k0:k0 + chunk]
            xs = [torch.stack([s[l] for s in part]).to(DEV, non_blocking=True) for l in range(len(lins) - 1)]
            a = inputs.unsqueeze(0).expand(len(part), -1, -1)
            overall = torch.zeros(len(part), inputs.shape[0], dtype=torch.float64, device=DEV)
            for l, x in enumerate(xs):
                mu = torch.nn.functional.linear(a, lins[l].weight, lins[l].bias)
                overall += (0.5 * (x - mu) ** 2).sum(-1).double()
                a = torch.relu(x)
            o = torch.nn.functional.linear(a, lins[-1].weight, lins[-1].bias)
            overall += torch.nn.functional.binary_cross_entropy_with_logits(o, data.expand_as(o), reduction="none").sum(-1).double()
            out.append(overall)
    return torch.cat(out)


class Workload:
    def __init__(self, dims, n_out, B, T, begin, lr):
        mods = []
        for i in range(1, len(dims)):
            mods += [torch.nn.Linear(dims[i - 1], dims[i]), pc.PCLayer(sample_x_fn=um.sample_x_fn_normal), torch.nn.ReLU()]
        self.model = torch.nn.Sequential(*mods, torch.nn.Linear(dims[-1], n_out)).to(DEV)
        self.model.train()
        self.T, self.begin, self.B = T, begin, B
        self.data = (torch.rand(B, n_out, device=DEV) < 0.3).float()
        self.inputs = torch.zeros(B, dims[0], device=DEV)
        self.tr = pc.PCTrainer(self.model, T=T, optimizer_x_fn=torch.optim.SGD, optimizer_x_kwargs={"lr": lr}, update_p_at="never",
                               plot_progress_at=[])
        self.n = T - begin

    def run(self, variant):
        replay()
        kw = dict(inputs=self.inputs, loss_fn=um.bernoulli_fn, loss_fn_kwargs={"_target": self.data, "_var": None},
                  callback_after_t=um.random_step, callback_after_t_kwargs={"_pc_trainer": self.tr}, is_log_progress=False,
                  is_checking_after_callback_after_t=False)
        self.tr.mcpc_chain_energies = dict(begin=self.begin) if variant == "spec" else None
        if variant == "torch":
            r = self.tr.train_on_batch(is_return_results_every_t=True, is_return_xs=True, **kw)
            return torch_energies(self.model, self.inputs, self.data, r["xs"][self.begin:])
        self.tr.train_on_batch(is_return_results_every_t=False, **kw)
        if variant == "spec":
            self.slices = self.tr.last_record_slices
            return self.tr.mcpc_last_chain_energies.overall
        return None


class WorkloadA(Workload):
    name = "a: 20-128-128 -> 784, 256 chains, MCPC 50 + 100 steps, the trace of every step"

    def __init__(self, args):
        torch.manual_seed(1)
        super().__init__([20, 20, 128, 128], 784, 256, 150, 0, 0.01)


class WorkloadB(Workload):
    name = "b: 30 | 256-256-256 -> 784, 6000 chains, MCPC T = 1000, the trace from step 200"

    def __init__(self, args):
        torch.manual_seed(2)
        super().__init__([30, 256, 256, 256], 784, 6000, args.T_b, args.T_b // 5, 0.01)


def kernel_alone(say):
    """Engine.chain_energies by itself (HIP events): cfg-M's net, 6000 chains, n_rec records per call."""
    from montecarlopredictivecoding_amd import _lib as L
    from montecarlopredictivecoding_amd.engine import Engine
    sizes, n_in, n_out, B = [256, 256, 256], 30, 784, 6000
    torch.manual_seed(4)
    eng = Engine(sizes, [L.ACT_RELU] * 3, n_in, n_out, B, device=DEV)
    dims = [n_in] + sizes + [n_out]
    eng.bind_params([torch.randn(dims[j + 1], dims[j], device=DEV) / dims[j] ** 0.5 for j in range(4)],
                    [0.1 * torch.randn(dims[j + 1], device=DEV) for j in range(4)])
    eng.bind_target((torch.rand(B, n_out, device=DEV) < 0.3).float())
    say("# Engine.chain_energies alone: cfg-M's net, 6000 chains, Bernoulli loss; rows = n_rec x 6000; HIP events, min of 3 after a warm-up")
    flop = 2 * (256 * 256 * 2 + 256 * 784)
    for n_rec in (1, 4, 16, 64):
        xs = [torch.randn(n_rec, B, n, device=DEV) for n in sizes]
        out = torch.empty(n_rec, B, L.ENERGY_COLS, dtype=torch.float64, device=DEV)
        ts = []
        for _ in range(4):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            eng.chain_energies(None, xs, loss_kind=L.LOSS_BERNOULLI, out=out)
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        best = min(ts[1:])
        say("n_rec %3d  %8d rows  %8.3f ms  %7.2f us per record  %6.1f TFLOP/s of fp32-equivalent GEMM" % (
            n_rec, n_rec * B, best, best * 1e3 / n_rec, flop * n_rec * B / best / 1e9))
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="a,b")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--T-b", type=int, default=1000)
    ap.add_argument("--only", default=None, help="workload:variant, e.g. b:spec -- one warm-up and one timed call (for a kernel trace)")
    ap.add_argument("--kernel-alone", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "scripts/chain_energies.py needs a GPU"
    warnings.simplefilter("ignore")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    classes = {"a": WorkloadA, "b": WorkloadB}
    if args.only:
        w, variant = args.only.split(":")
        wl = classes[w](args)
        wl.run(variant)
        ms, _ = wall_ms(lambda: wl.run(variant))
        say("# %s  %s: %.2f ms" % (wl.name, variant, ms))
    elif not args.kernel_alone:
        for w in args.workloads.split(","):
            wl = classes[w](args)
            variants = ["spec", "plain", "torch"]
            got = {}
            for v in variants:
                got[v] = wl.run(v)                                               # warm-up
            times = {v: [] for v in variants}
            for _ in range(args.repeats):
                for v in variants:
                    times[v].append(wall_ms(lambda: wl.run(v))[0])
            say("# %s" % wl.name)
            say("#   %d slice(s) of the record ring; ms per call, min (max) of %d" % (wl.slices, args.repeats))
            for v in variants:
                say("%-6s %9.2f (%9.2f) ms" % (v, min(times[v]), max(times[v])))
            spec, plain = min(times["spec"]), min(times["plain"])
            say("spec - plain = %.2f ms = %.1f %% of the plain call, %.2f us per evaluated step" % (
                spec - plain, 100 * (spec - plain) / plain, (spec - plain) * 1e3 / wl.n))
            say("torch / spec = %.2f" % (min(times["torch"]) / spec))
            a, b = got["spec"], got["torch"]
            say("largest relative difference of overall between the two ways: %.2e" % ((a - b).abs() / b.abs()).max().item())
            del wl, got
            torch.cuda.empty_cache()
    if args.kernel_alone:
        kernel_alone(say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

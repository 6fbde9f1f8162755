#!/usr/bin/env python3
"""Posterior moments accumulated on the device (csrc/mcpc_moments.h, PCTrainer.mcpc_moments) against the two other ways to run the same
call (developer measurement for DESIGN.md section 7, profiles/posterior_moments.txt).

    python scripts/posterior_moments.py [--workloads a,b] [--chunk-mb 1024[,64,256]] [--side-stream] [--repeats 3] [--out FILE]
    python scripts/posterior_moments.py --only b:moments          # one warm-up and one timed call, for a kernel trace

Workloads, through the facade (PCTrainer.train_on_batch, host work included, wall clock around synchronised calls):
  a  the reference's net 20-128-128 -> 784 at 256 chains: MAP call (T_pc = 250) + MCPC call (50 + 100 steps), mean of x_1 over all steps
     -- get_representations(rep_type="expectation")
  b  cfg-M's net 30 | 256-256-256 -> 784 at 6000 chains, one MCPC call of T = 1000, mean and variance of sigmoid(read-out) from step 200
Variants:
  moments  the call with mcpc_moments
  plain    the same call without moments and without records: moments - plain is what the statistics cost
  records  the only way without mcpc_moments: record every step, reduce what the call returns in torch
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
from montecarlopredictivecoding_amd.engine import moments_accumulate  # noqa: E402
from montecarlopredictivecoding_amd.utils.training_evaluation import get_mcpc_trainer, get_pc_trainer  # noqa: E402

DEV = torch.device("cuda", 0)


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def replay():
    """Every run of a workload draws the same x0 and the same Langevin noise, so that the variants compute the same statistics."""
    torch.manual_seed(3)
    pt._PHILOX_STEPS[0] = 0


class WorkloadA:
    name = "a: 20-128-128 -> 784, 256 chains, MAP 250 + MCPC 150 steps, mean of x_1 (layers=(0,))"

    def __init__(self, args):
        torch.manual_seed(1)
        self.cfg = dict(input_size=20, hidden_size=128, hidden2_size=128, output_size=784, activation_fn="relu", loss_fn=um.bernoulli_fn,
                        input_var=None, T_pc=250, optimizer_x_fn_pc=torch.optim.Adam, optimizer_x_kwargs_pc={"lr": 0.1},
                        mixing=50, sampling=100, optimizer_x_kwargs_mcpc={"lr": 0.01},
                        optimizer_p_fn_mcpc=torch.optim.Adam, optimizer_p_kwargs_mcpc={"lr": 0.01})
        self.model = um.get_model(self.cfg, True, sample_x_fn=um.sample_x_fn_normal)
        self.data = (torch.rand(256, 784, device=DEV) < 0.3).float()
        self.inputs = torch.zeros(256, 20, device=DEV)
        self.pc_tr = get_pc_trainer(self.model, self.cfg, is_mcpc=True, training=False)
        self.mc_tr = get_mcpc_trainer(self.model, self.cfg, training=False)
        self.mc_tr.mcpc_moments_chunk_bytes = args.chunk_bytes
        self.mc_tr.mcpc_moments_side_stream = args.side_stream
        self.T, self.row = 150, 256 * 20
        self.n = 150

    def run(self, variant):
        replay()
        kw = dict(inputs=self.inputs, loss_fn=um.bernoulli_fn, loss_fn_kwargs={"_target": self.data, "_var": None},
                  is_log_progress=False, is_checking_after_callback_after_t=False)
        self.pc_tr.train_on_batch(is_return_results_every_t=False, **kw)
        mk = dict(callback_after_t=um.random_step, callback_after_t_kwargs={"_pc_trainer": self.mc_tr},
                  is_sample_x_at_batch_start=False, **kw)
        self.mc_tr.mcpc_moments = dict(begin=0, layers=(0,), variance=False) if variant == "moments" else None
        if variant == "records":
            r = self.mc_tr.train_on_batch(is_return_results_every_t=True, is_return_representations=True, **mk)
            return torch.stack(r["representations"]).to(DEV).mean(0)          # get_representations, rep_type="expectation"
        self.mc_tr.train_on_batch(is_return_results_every_t=False, **mk)
        return self.mc_tr.mcpc_last_moments.x_mean[0] if variant == "moments" else None


class WorkloadB:
    name = "b: 30 | 256-256-256 -> 784, 6000 chains, MCPC T = 1000, mean and variance of sigmoid(read-out) over steps 200.."

    def __init__(self, args):
        torch.manual_seed(2)
        dims = [30, 256, 256, 256]
        mods = []
        for i in range(1, len(dims)):
            mods += [torch.nn.Linear(dims[i - 1], dims[i]), pc.PCLayer(sample_x_fn=um.sample_x_fn_normal), torch.nn.ReLU()]
        self.model = torch.nn.Sequential(*mods, torch.nn.Linear(256, 784)).to(DEV)
        self.model.train()
        self.T, self.begin, self.B = args.T_b, args.T_b // 5, 6000
        self.data = (torch.rand(self.B, 784, device=DEV) < 0.3).float()
        self.inputs = torch.zeros(self.B, 30, device=DEV)
        self.tr = pc.PCTrainer(self.model, T=self.T, optimizer_x_fn=torch.optim.SGD, optimizer_x_kwargs={"lr": 0.01}, update_p_at="never",
                               plot_progress_at=[])
        self.tr.mcpc_moments_chunk_bytes = args.chunk_bytes
        self.tr.mcpc_moments_side_stream = args.side_stream
        self.row, self.n = self.B * 784, self.T - self.begin

    def run(self, variant):
        replay()
        kw = dict(inputs=self.inputs, loss_fn=um.bernoulli_fn, loss_fn_kwargs={"_target": self.data, "_var": None},
                  callback_after_t=um.random_step, callback_after_t_kwargs={"_pc_trainer": self.tr}, is_log_progress=False,
                  is_checking_after_callback_after_t=False)
        self.tr.mcpc_moments = dict(begin=self.begin, outputs="sigmoid", variance=True) if variant == "moments" else None
        if variant == "records":
            r = self.tr.train_on_batch(is_return_results_every_t=True, is_return_outputs=True, **kw)
            outs = r["outputs"][self.begin:]
            s = torch.zeros(self.B, 784, device=DEV)
            q = torch.zeros(self.B, 784, device=DEV)
            for k in range(0, len(outs), 50):                                  # (chunks of 50 steps: one 15 GB temporary less)
                g = torch.stack(outs[k:k + 50]).sigmoid_()
                s += g.sum(0)
                q += g.square_().sum(0)
            n = len(outs)
            return s / n, (q - s * s / n) / (n - 1)
        self.tr.train_on_batch(is_return_results_every_t=False, **kw)
        if variant == "moments":
            self.slices = self.tr.last_record_slices
        m = self.tr.mcpc_last_moments
        return (m.out_mean, m.out_var) if variant == "moments" else None


def reducer_alone(say):
    """The kernel by itself (HIP events): records of cfg-M's read-out at 6000 chains, chunks that fit the 256 MiB L3 and chunks that do not."""
    row = 6000 * 784
    say("# mcpc_moments_kernel alone: chunks of cfg-M's read-out records (6000 x 784 fp32 = 18.8 MB per step), sigmoid, sum + sumsq;")
    say("#   bytes = 4 B per element and record + 32 B per element and call (accumulators read and written); fresh = written just before")
    s = torch.zeros(row, dtype=torch.float64, device=DEV)
    q = torch.zeros(row, dtype=torch.float64, device=DEV)
    for steps in (3, 6, 13, 27, 54, 109, 218):
        rec = torch.randn(steps, row, device=DEV)
        best = {}
        for mode in ("cold", "fresh"):
            ts = []
            for _ in range(4):
                if mode == "fresh":
                    rec.mul_(1.0)                                              # the chunk was just written, as after a slice of steps
                else:
                    torch.empty(1 << 28, dtype=torch.float32, device=DEV).zero_()     # 1 GiB through the cache
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                moments_accumulate(rec, 0, 1, steps, s, q, transform="sigmoid", accumulate=True)
                b.record()
                b.synchronize()
                ts.append(a.elapsed_time(b))
            best[mode] = min(ts[1:])
        nbytes = row * (4 * steps + 32)
        say("chunk %4d steps %7.1f MiB   cold %8.3f ms %6.2f TB/s   fresh %8.3f ms %6.2f TB/s   %6.2f us per step (fresh)" % (
            steps, steps * row * 4 / 2 ** 20, best["cold"], nbytes / best["cold"] / 1e9, best["fresh"], nbytes / best["fresh"] / 1e9,
            best["fresh"] * 1e3 / steps))
        del rec
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="a,b")
    ap.add_argument("--chunk-mb", default="1024")
    ap.add_argument("--side-stream", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--T-b", type=int, default=1000)
    ap.add_argument("--only", default=None, help="workload:variant, e.g. b:moments -- one warm-up and one timed call (for a kernel trace)")
    ap.add_argument("--reducer-alone", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "scripts/posterior_moments.py needs a GPU"
    warnings.simplefilter("ignore")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    classes = {"a": WorkloadA, "b": WorkloadB}
    chunks = [int(float(c) * 2 ** 20) for c in args.chunk_mb.split(",")]
    if args.only:
        w, variant = args.only.split(":")
        args.chunk_bytes = chunks[0]
        wl = classes[w](args)
        wl.run(variant)
        ms, _ = wall_ms(lambda: wl.run(variant))
        say("# %s  %s: %.2f ms (chunk %d MiB, %s)" % (wl.name, variant, ms, chunks[0] >> 20, "side stream" if args.side_stream else "serial"))
    else:
        for w in args.workloads.split(","):
            for ci, chunk in enumerate(chunks):
                args.chunk_bytes = chunk
                wl = classes[w](args)
                variants = ["moments", "plain", "records"] if ci == 0 else ["moments", "plain"]
                got = {}
                for v in variants:
                    got[v] = wl.run(v)                                           # warm-up
                times = {v: [] for v in variants}
                for _ in range(args.repeats):
                    for v in variants:
                        times[v].append(wall_ms(lambda: wl.run(v))[0])
                say("# %s" % wl.name)
                say("#   ring halves of at most %d MiB (%s), reducer %s; ms per call, min (max) of %d" % (
                    chunk >> 20, "%d slices" % wl.slices if hasattr(wl, "slices") else "1 slice", "on a side stream" if args.side_stream else "on the call's stream",
                    args.repeats))
                for v in variants:
                    say("%-8s %9.2f (%9.2f) ms" % (v, min(times[v]), max(times[v])))
                mom, plain = min(times["moments"]), min(times["plain"])
                say("moments - plain = %.2f ms = %.1f %% of the plain call, %.2f us per sampled step" % (
                    mom - plain, 100 * (mom - plain) / plain, (mom - plain) * 1e3 / wl.n))
                if "records" in times:
                    say("records / moments = %.2f" % (min(times["records"]) / mom))
                    # the two ways agree (fp32 torch reduction against fp64 sums)
                    a, b = got["moments"], got["records"]
                    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
                    say("largest difference between the two ways: " + ", ".join("%.2e" % (x - y).abs().max().item() for x, y in zip(a, b)))
                del wl, got
                torch.cuda.empty_cache()
    if args.reducer_alone:
        reducer_alone(say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

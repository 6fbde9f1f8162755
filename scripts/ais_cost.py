#!/usr/bin/env python3
"""What a rung of annealed importance sampling costs on the device (csrc/mcpc_ais.h, ais.py): developer measurement for DESIGN.md
section 7, profiles/ais_cost.txt.

    python scripts/ais_cost.py [--reps 20] [--inner 10] [--out profiles/ais_cost.txt]

cfg-M's net (30-256-256-784, ReLU, Bernoulli read-out), 6000 chains, seeded weights and binary targets, one process.  Every figure
is the median of --reps repetitions after a warm-up of the same shape; a repetition is --inner back-to-back calls between two HIP
events on the stream (the clock is the device's event timer; the step kernel's own shader clock is printed beside (d)).

  (a) one engine.ais_increment (one kernel launch);
  (b) the same increment composed from what the library had before it: Engine.prediction_errors(outputs="prediction") on a second
      engine that holds the unscaled read-out, plus the torch fp64 expression of the two losses on its fp32 logits;
  (c) one re-bind of the scaled read-out: the fp32 scale of W and b into the scratch copy + Engine.params_changed (the re-pack);
  (d) one Langevin step of the same engine (Engine.run of 20 steps / 20).
Then the share of a whole rung, (a) + (c) + steps_per_stage x (d), that (a) + (c) take at steps_per_stage 1, 5 and 20, and the
largest |(a) - (b)| of the two results with the bound of tests/ais_cases.py beside it.  A run without a GPU fails: there is no fallback."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NET = dict(n_in=30, sizes=(256, 256), n_out=784, chains=6000)


def timed(fn, reps, inner):
    """median, min, max in microseconds per call of fn."""
    import torch
    fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / inner)
    return statistics.median(us), min(us), max(us)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "scripts/ais_cost.py needs a GPU"
    from montecarlopredictivecoding_amd import _lib as L
    from montecarlopredictivecoding_amd.engine import Engine, ais_increment
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator().manual_seed(31)
    dims = [NET["n_in"], *NET["sizes"], NET["n_out"]]
    W = [(torch.randn(o, i, generator=g) / i ** 0.5).to(dev) for i, o in zip(dims[:-1], dims[1:])]
    b = [(0.1 * torch.randn(o, generator=g)).to(dev) for o in dims[1:]]
    B = NET["chains"]
    y = (torch.rand(B, NET["n_out"], generator=g) < 0.13).float().to(dev)
    acts = [L.ACT_RELU] * len(NET["sizes"])
    eng = Engine(list(NET["sizes"]), acts, NET["n_in"], NET["n_out"], B, device=dev)
    plain = Engine(list(NET["sizes"]), acts, NET["n_in"], NET["n_out"], B, device=dev)
    W_s, b_s = torch.empty_like(W[-1]), torch.empty_like(b[-1])
    eng.bind_params(W[:-1] + [W_s], b[:-1] + [b_s])
    plain.bind_params(W, b)
    for e in (eng, plain):
        e.bind_inputs(None)
        e.bind_target(y)
    _, xs = plain.sample_prior(B, 7, step=0, latents=True, readout=None)
    eng.load_state(xs)
    beta0, beta1 = 0.25, 0.31640625
    logw = torch.zeros(B, dtype=torch.float64, device=dev)
    say("# cfg-M's net %d-%s-%d, ReLU, Bernoulli, %d chains; median (min .. max) of %d repetitions of %d calls between two HIP events, "
        "microseconds per call" % (NET["n_in"], "-".join(str(s) for s in NET["sizes"]), NET["n_out"], B, args.reps, args.inner))

    def a_call():
        ais_increment(xs[-1], W[-1], b[-1], y, "relu", "bernoulli", None, 0, beta0, 1.0, beta1, 1.0, logw, accumulate=False)

    out = {"out": torch.empty(1, B, NET["n_out"], device=dev)}
    composed = torch.zeros(B, dtype=torch.float64, device=dev)

    def b_call():
        o = plain.prediction_errors(None, [None, xs[-1]], layers=(), outputs="prediction", out=out)["out"][0].double()
        yd = y.double()
        z0, z1 = beta0 * o, beta1 * o
        t0 = torch.clamp(z0, min=0) + torch.log1p(torch.exp(-z0.abs())) - yd * z0
        t1 = torch.clamp(z1, min=0) + torch.log1p(torch.exp(-z1.abs())) - yd * z1
        torch.sum(t0 - t1, dim=1, out=composed)

    def c_call():
        torch.mul(W[-1], beta1, out=W_s)
        torch.mul(b[-1], beta1, out=b_s)
        eng.params_changed()

    def d_call():
        eng.run(20, loss_kind=L.LOSS_BERNOULLI, mask_start=0, xopt=L.XOPT_SGD, lr=0.03, noise_mode=L.NOISE_PHILOX, noise_var=2.0, seed=1,
                step_base=1, chain_base=0)

    ta = timed(a_call, args.reps, args.inner)
    tb = timed(b_call, args.reps, args.inner)
    tc = timed(c_call, args.reps, args.inner)
    td = tuple(v / 20 for v in timed(d_call, args.reps, max(1, args.inner // 5)))
    eng.set_profiling(True)
    d_call()
    eng.sync_check()
    ghz = eng.last_shader_clock_ghz()
    eng.set_profiling(False)
    say("(a) ais_increment                                   %9.1f (%9.1f .. %9.1f) us" % ta)
    say("(b) prediction_errors(prediction) + torch fp64      %9.1f (%9.1f .. %9.1f) us" % tb)
    say("(c) scale the read-out + params_changed             %9.1f (%9.1f .. %9.1f) us" % tc)
    say("(d) one Langevin step (run of 20 / 20), %s  %9.1f (%9.1f .. %9.1f) us; shader clock %.3f GHz" % ((eng.last_step_kernel(),) + td + (ghz,)))
    for sps in (1, 5, 20):
        rung = ta[0] + tc[0] + sps * td[0]
        say("steps_per_stage %2d: a rung takes %8.1f us, (a) + (c) are %4.1f %% of it" % (sps, rung, 100 * (ta[0] + tc[0]) / rung))
    say("(a) / (b) = %.2f: the kernel is %s than the composition" % (ta[0] / tb[0], "no slower" if ta[0] <= tb[0] else "SLOWER"))
    a_call()
    b_call()
    torch.cuda.synchronize()
    say("largest |(a) - (b)| over the chains %.3g on |logw| up to %.3g ((b) forms its logits on the step kernels' fp16-split GEMM in fp32, "
        "(a) in fp64)" % (float((logw - composed).abs().max()), float(logw.abs().max())))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

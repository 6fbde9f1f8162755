#!/usr/bin/env python3
"""Wide networks on the layer-wise kernels (csrc/mcpc_steps_lw.h): time per Langevin step against eager torch on the same GPU and
against the LDS-resident kernels where both run (developer measurement for DESIGN.md section 7, profiles/wide_nets.txt).

    python scripts/wide_nets.py [--rows eager|both|all] [--min-call 0.25] [--out FILE]

Eager torch = the op mix of oracle/torch_port.py (plain torch modules: the reference's forward, one autograd backward(), the optimizer
step on x, the kick) with model and state on the GPU: the reference's arithmetic on rocBLAS fp32.  Every row: warm-up call, T chosen from
a short probe so that a timed call lasts at least --min-call seconds, then two timed calls alternating between the two sides (HIP events
around whole calls); the smaller of the two times is reported per side and the larger is shown beside it as the spread.
A run without a GPU fails: there is no fallback."""
import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from montecarlopredictivecoding_amd import _lib as L  # noqa: E402
from montecarlopredictivecoding_amd.engine import Engine  # noqa: E402
from oracle import torch_port  # noqa: E402

DEV = torch.device("cuda", 0)
LR, NOISE_VAR = 0.05, 2.0
ACT = {"relu": 1, "tanh": 2}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    b.synchronize()
    return a.elapsed_time(b)


def params(n_in, sizes, n_out, gen):
    dims = [n_in] + list(sizes) + ([n_out] if n_out else [])
    W, b = [], []
    for j in range(len(dims) - 1):
        k = 1.0 / math.sqrt(dims[j])
        W.append(((torch.rand(dims[j + 1], dims[j], generator=gen) * 2 - 1) * k))
        b.append(((torch.rand(dims[j + 1], generator=gen) * 2 - 1) * k))
    return W, b


class EngineSide:
    def __init__(self, shape, B, tuning, W, b, X0, inputs, target):
        n_in, sizes, n_out, act, loss = shape
        self.eng = Engine(sizes, [ACT[act]] * len(sizes), n_in, n_out, B, device=DEV, tuning=tuning)
        self.keep = ([w.to(DEV) for w in W], [x.to(DEV) for x in b])
        self.eng.bind_params(*self.keep)
        self.eng.bind_inputs(inputs.to(DEV) if inputs is not None else None)
        self.loss = dict(loss_kind={"gaussian": L.LOSS_GAUSSIAN, "bernoulli": L.LOSS_BERNOULLI}[loss], loss_var=1.0)
        self.eng.bind_target(target.to(DEV))
        self.X0 = [x.to(DEV) for x in X0]
        self.kernel = self.eng.query()["step_kernel"]

    def call(self, T, learn):
        self.eng.load_state(self.X0)
        self.eng.run(T, xopt=L.XOPT_SGD, lr=LR, noise_mode=L.NOISE_PHILOX, noise_var=NOISE_VAR, seed=1, step_base=0,
                     acc_begin=0, acc_end=T if learn else 0, energy_mode=L.ENERGY_LAST, **self.loss)


class EagerSide:
    """oracle/torch_port.py's loop on the GPU.  An inference-only call still runs the one backward() of the reference's loop (it is how
    the reference gets dF/dx; the parameter gradients come with it), a learning call lets them accumulate from step 0."""
    kernel = "eager torch (rocBLAS fp32)"

    def __init__(self, shape, B, W, b, X0, inputs, target):
        n_in, sizes, n_out, act, loss = shape
        self.model, self.nodes, self.lins = torch_port.build(sizes, [act] * len(sizes), n_in, n_out, [w.numpy() for w in W], [x.numpy() for x in b])
        self.model.to(DEV)
        self.inputs = (inputs if inputs is not None else torch.zeros(B, n_in)).to(DEV)
        self.X0 = [x.to(DEV) for x in X0]
        self.loss_fn = torch_port.make_loss(loss, target.to(DEV), 1.0, 0)

    def call(self, T, learn):
        torch_port.run(self.model, self.nodes, self.lins, self.inputs, self.X0, self.loss_fn, T, LR, xopt="sgd", noise_var=NOISE_VAR,
                       acc_begin=0 if learn else None, record_energy=False)


def measure(sides, learn, min_call):
    """[(name, us per step, us per step of the slower repeat, T)] -- the sides alternate inside each repeat"""
    Ts = []
    for s in sides:
        s.call(4, learn); torch.cuda.synchronize()                     # warm-up: code objects, rocBLAS picks its kernels
        # T from a short probe, then raised until a call really lasts min_call (what a call costs once -- binding, the flush of Linear 0,
        # the read-back of the energies -- weighs on a short probe and would make T too small)
        T = 8
        for _ in range(4):
            ms = event_ms(lambda: s.call(T, learn))
            if ms >= min_call * 1e3 or T >= 20000:
                break
            T = int(min(20000, max(T + 1, math.ceil(1.15 * T * min_call * 1e3 / max(ms, 1e-3)))))
        Ts.append(T)
    times = [[] for _ in sides]
    for _ in range(2):
        for i, s in enumerate(sides):
            times[i].append(event_ms(lambda: s.call(Ts[i], learn)) * 1e3 / Ts[i])
    return [(s.kernel, min(t), max(t), T) for s, t, T in zip(sides, times, Ts)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="all", choices=["eager", "both", "all"])
    ap.add_argument("--min-call", type=float, default=0.25)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "scripts/wide_nets.py needs a GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    gen = torch.Generator().manual_seed(7)

    def data(shape, B):
        n_in, sizes, n_out, act, loss = shape
        W, b = params(n_in, sizes, n_out, gen)
        X0 = [torch.rand(B, n, generator=gen) * 2 - 1 for n in sizes]
        inputs = torch.rand(B, n_in, generator=gen) * 2 - 1 if n_in == 784 else None
        target = (torch.rand(B, n_out, generator=gen) < 0.3).float() if loss == "bernoulli" else torch.rand(B, n_out, generator=gen) * 2 - 0.5
        return W, b, X0, inputs, target

    if args.rows in ("eager", "all"):
        say("# layer-wise kernels (tuning wide=1) against eager torch on the same GPU: us per Langevin step (SGD + kick), min of two calls (max)")
        for shape in [(30, [512, 512], 784, "relu", "bernoulli"), (30, [1024, 1024], 784, "relu", "bernoulli"), (784, [512, 512], 10, "relu", "gaussian")]:
            for B in (6000, 256):
                d = data(shape, B)
                sides = [EngineSide(shape, B, "wide=1", *d), EagerSide(shape, B, *d)]
                assert "mcpc_lw_fwd_kernel" in sides[0].kernel, sides[0].kernel
                for learn in (False, True):
                    (_, lw, lw_hi, T0), (_, eg, eg_hi, T1) = measure(sides, learn, args.min_call)
                    say("%-4d | %-14s -> %-4d %6d chains  %-9s  layer-wise %9.1f (%9.1f) us/step T=%-5d  eager %9.1f (%9.1f) us/step T=%-5d  eager / layer-wise = %.2f" % (
                        shape[0], "-".join(map(str, shape[1])), shape[2], B, "learning" if learn else "inference", lw, lw_hi, T0, eg, eg_hi, T1, eg / lw))
                sides[0].eng.close()
                del sides
                torch.cuda.empty_cache()
    if args.rows in ("both", "all"):
        say("# layer-wise kernels (tuning ws=4) against the LDS-resident kernels (default tuning) where both run: us per step, min of two calls (max)")
        for shape, B in [((30, [256, 256, 256], 784, "relu", "bernoulli"), 6000), ((20, [128, 128], 784, "relu", "bernoulli"), 256)]:
            d = data(shape, B)
            sides = [EngineSide(shape, B, "ws=4", *d), EngineSide(shape, B, "", *d)]
            for learn in (False, True):
                (_, lw, lw_hi, T0), (name, ld, ld_hi, T1) = measure(sides, learn, args.min_call)
                say("%-4d | %-14s -> %-4d %6d chains  %-9s  layer-wise %9.1f (%9.1f) us/step  %s %9.1f (%9.1f) us/step  layer-wise / LDS-resident = %.2f" % (
                    shape[0], "-".join(map(str, shape[1])), shape[2], B, "learning" if learn else "inference", lw, lw_hi, name.split("(")[0].strip(), ld, ld_hi, lw / ld))
            for s in sides:
                s.eng.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

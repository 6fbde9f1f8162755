#!/usr/bin/env python3
"""The posterior of a linear probe accumulated on the device (csrc/mcpc_probe.h, PCTrainer.mcpc_probe): what the request adds to a
call, beside what the same result costs without it (developer measurement for DESIGN.md section 7, profiles/probe_cost.txt).

    python scripts/probe_cost.py [--repeats 3] [--out FILE]
    python scripts/probe_cost.py --part fig2|m          # one shape, in this process

Without --part the script only drives: every shape runs in a child process of its own under a time limit (--limit seconds), one after
the other, and the first that fails or runs out of time ends the run; --out FILE replaces FILE with what the parts printed.

Shapes: `fig2`, the reference's figure_2 (20-128-128 -> 784, 128 chains, T = 10 000, mixing 1 000) and `m`, cfg-M (30-256-256 -> 784,
6 000 chains, T = 5 000, mixing 1 000); a 10-class softmax probe on layer 0.  One inference-only MCPC call through the facade
(PCTrainer.train_on_batch, host work included, wall clock around synchronised calls), three ways:
  plain  (a) the call without a probe and without records
  probe  (b) the call with mcpc_probe = dict(begin=mixing, layer=0, linear=classifier)
  loop   (c) what the package offered before: the call with is_return_representations=True, then the loop of the reference
             (figure_2.py, comparison_ideal_observer) over the recorded steps from `mixing` on, on the GPU: the step's representation to
             the device, probability += softmax(classifier(representation))
All three are warmed up once; then they alternate inside each of --repeats rounds; min (max) of the rounds is reported, and (b) - (a)
beside (c) - (a).  The class probabilities of (b) and (c) are compared.  A run without a GPU fails: there is no fallback."""
import argparse
import os
import subprocess
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"fig2": dict(sizes=(20, 128, 128), n_out=784, B=128, T=10000, mixing=1000),
          "m": dict(sizes=(30, 256, 256), n_out=784, B=6000, T=5000, mixing=1000)}
CLASSES = 10


def wall_ms(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def facade(say, name, repeats):
    import torch
    import montecarlopredictivecoding_amd.predictive_coding as pc
    import montecarlopredictivecoding_amd.predictive_coding.pc_trainer as pt
    import montecarlopredictivecoding_amd.utils.model as um
    dev = torch.device("cuda", 0)
    shape = SHAPES[name]
    sizes, n_out, B, T, mixing = shape["sizes"], shape["n_out"], shape["B"], shape["T"], shape["mixing"]
    torch.manual_seed(1)
    model = um.get_model(dict(input_size=sizes[0], hidden_size=sizes[1], hidden2_size=sizes[2], output_size=n_out, activation_fn="relu"),
                         True, sample_x_fn=um.sample_x_fn_normal)
    clf = torch.nn.Linear(sizes[0], CLASSES).to(dev)
    data = (torch.rand(B, n_out, device=dev) < 0.3).float()
    inputs = torch.zeros(B, sizes[0], device=dev)
    tr = pc.PCTrainer(model, T=T, optimizer_x_fn=torch.optim.SGD, optimizer_x_kwargs={"lr": 0.01}, update_p_at="never", plot_progress_at=[])
    slices = {}

    def run(variant):
        torch.manual_seed(3)                                 # every run draws the same x0 and the same Langevin noise
        pt._PHILOX_STEPS[0] = 0
        tr.mcpc_probe = dict(begin=mixing, layer=0, linear=clf) if variant == "probe" else None
        loop = variant == "loop"
        res = tr.train_on_batch(inputs=inputs, loss_fn=um.bernoulli_fn, loss_fn_kwargs={"_target": data, "_var": None},
                                callback_after_t=um.random_step, callback_after_t_kwargs={"_pc_trainer": tr}, is_log_progress=False,
                                is_checking_after_callback_after_t=False, is_return_results_every_t=loop, is_return_representations=loop)
        slices[variant] = tr.last_record_slices
        if variant == "probe":
            return tr.mcpc_last_probe.mean()
        if loop:
            reps = res["representations"]
            prob = torch.zeros(B, CLASSES, device=dev)
            with torch.no_grad():
                for idx in range(T - mixing):
                    prob += torch.softmax(clf(reps[idx + mixing].to(dev)), 1)
            return prob / (T - mixing)
        return None

    variants = ["probe", "plain", "loop"]
    got = {v: run(v) for v in variants}                                              # warm-up
    times = {v: [] for v in variants}
    for _ in range(repeats):
        for v in variants:
            times[v].append(wall_ms(lambda: run(v))[0])
    n = T - mixing
    say("# %s: %s -> %d, %d chains, inference only, T = %d, a %d-class softmax probe on layer 0 (%d units) from step %d on: "
        "%d samples per chain" % (name, "-".join(str(s) for s in sizes), n_out, B, T, CLASSES, sizes[0], mixing, n))
    say("#   slices of the record ring: probe %d, loop %d; ms per call, min (max) of %d" % (slices["probe"], slices["loop"], repeats))
    for v, what in (("plain", "(a)"), ("probe", "(b)"), ("loop", "(c)")):
        say("%-5s %s %9.2f (%9.2f) ms" % (v, what, min(times[v]), max(times[v])))
    a, b, c = min(times["plain"]), min(times["probe"]), min(times["loop"])
    say("(b) - (a) = %.2f ms = %.1f %% of the plain call, %.2f us per sample step;  (c) - (a) = %.2f ms = %.1f %%;  "
        "((c) - (a)) / ((b) - (a)) = %.1f" % (b - a, 100 * (b - a) / a, (b - a) * 1e3 / n, c - a, 100 * (c - a) / a, (c - a) / (b - a)))
    say("max |mean p of (b) - mean p of (c)| = %.3g (fp64 sums of fp32 softmax against an fp32 running sum)"
        % float((got["probe"] - got["loop"].double()).abs().max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--part", default=None, choices=sorted(SHAPES))
    ap.add_argument("--limit", type=int, default=300, help="seconds a part may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.part is not None:
        import torch
        assert torch.cuda.is_available(), "scripts/probe_cost.py needs a GPU"
        warnings.simplefilter("ignore")

        def say(s):
            print(s, flush=True)
        facade(say, args.part, args.repeats)
        return 0
    lines = []
    for part in ("fig2", "m"):
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

#!/usr/bin/env python3
"""Prediction errors and predictions of recorded states on the device (csrc/mcpc_pred_err.h, PCTrainer.mcpc_errors): the kernel alone
against its traffic and GEMM model, what the request adds to a call, and the route it replaces (developer measurement for DESIGN.md
section 7, profiles/pred_err_cost.txt).

    python scripts/pred_err_cost.py [--repeats 3] [--T 5000] [--T-xs 200] [--out FILE]
    python scripts/pred_err_cost.py --part kernel|call|replay        # one part, in this process

Without --part the script only drives: every part runs in a child process of its own under a time limit (--limit seconds), one after the
other, and the first part that fails or runs out of time ends the run; --out FILE replaces FILE with what the parts printed.

Part `kernel`: Engine.prediction_errors alone on cfg-M's net (30 | 256-256-256 -> 784, ReLU, Bernoulli read-out), 16384 rows (4 records
of 4096 chains: one scratch chunk); every layer and the read-out, errors only / predictions only / both, and layer 2 alone; HIP events,
min of 3 after a warm-up; beside Engine.chain_energies on the same rows.  The model: 4 B read per row and recorded unit and 8 B written
and 4 + 4 B read back per padded unit by the prep kernel and the tile, 4 B written per row, unit and destination; 2 * K * N flop per row
and Linear.
Part `call`: one inference-only MCPC call of T steps on cfg-M's net at 6000 chains through the facade (PCTrainer.train_on_batch, host
work included, wall clock around synchronised calls):
  errors  the call with mcpc_errors = dict(begin=T // 5, layers=(0, 1, 2), outputs="error")
  plain   the same call without it and without records: errors - plain is what the request costs
Part `replay`, at T-xs steps (the trajectory of a 5000-step call does not fit a host: 4 B x 6000 x 768 x T):
  errors  as above, at T-xs steps
  plain   as above, at T-xs steps
  xs      the only route without the request: is_return_xs (every step of every layer copied to pinned host memory), then the forward
          pass of the sample steps replayed in eager torch on the same GPU, with fp64 sums of the errors and their squares
All are warmed up once; then they alternate inside each of --repeats rounds; min (max) of the rounds is reported.
A run without a GPU fails: there is no fallback."""
import argparse
import os
import subprocess
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES, N_IN, N_OUT = [256, 256, 256], 30, 784


def wall_ms(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def event_ms(fn, repeats=3):
    """min of `repeats` after a warm-up, HIP events."""
    import torch
    ts = []
    for _ in range(repeats + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return min(ts[1:])


def kernel_alone(say):
    import torch
    from montecarlopredictivecoding_amd import _lib as L
    from montecarlopredictivecoding_amd.engine import Engine
    dev = torch.device("cuda", 0)
    B, n_rec = 4096, 4
    rows = B * n_rec
    torch.manual_seed(4)
    eng = Engine(SIZES, [L.ACT_RELU] * 3, N_IN, N_OUT, B, device=dev)
    dims = [N_IN] + SIZES + [N_OUT]
    eng.bind_params([torch.randn(dims[j + 1], dims[j], device=dev) / dims[j] ** 0.5 for j in range(4)],
                    [0.1 * torch.randn(dims[j + 1], device=dev) for j in range(4)])
    eng.bind_target((torch.rand(B, N_OUT, device=dev) < 0.3).float())
    xs = [torch.randn(n_rec, B, n, device=dev) for n in SIZES]
    say("# Engine.prediction_errors alone: cfg-M's net, %d rows (%d records of %d chains, one chunk), Bernoulli read-out; HIP events," % (rows, n_rec, B))
    say("# min of 3 after a warm-up; GB/s against the traffic model of the docstring, TFLOP/s of fp32-equivalent GEMM")
    table = torch.empty(n_rec, B, L.ENERGY_COLS, dtype=torch.float64, device=dev)
    t_ce = event_ms(lambda: eng.chain_energies(None, xs, loss_kind=L.LOSS_BERNOULLI, out=table))
    say("%-34s %8.3f ms" % ("chain_energies (the same rows)", t_ce))
    cases = (("every layer + read-out, errors", dict(quantity="error", outputs="error")),
             ("every layer + read-out, predictions", dict(quantity="prediction", outputs="prediction")),
             ("every layer + read-out, both", dict(quantity="both", outputs="both")),
             ("layer 2 alone, errors", dict(layers=(2,), quantity="error")))
    for name, kw in cases:
        layers = kw.get("layers", (0, 1, 2))
        head = kw.get("outputs") is not None
        per = 2 if "both" in (kw["quantity"], kw.get("outputs")) else 1
        out = {}
        for l in layers:
            for q in (("e", "mu") if kw["quantity"] == "both" else (("e",) if kw["quantity"] == "error" else ("mu",))):
                out["%s%d" % (q, l)] = torch.empty(n_rec, B, SIZES[l], device=dev)
        if head:
            for q in (("eout", "out") if kw["outputs"] == "both" else (("eout",) if kw["outputs"] == "error" else ("out",))):
                out[q] = torch.empty(n_rec, B, N_OUT, device=dev)
        read = sorted(set(layers) | {l - 1 for l in layers if l > 0} | ({2} if head else set()))
        recs = [x if l in read else None for l, x in enumerate(xs)]
        t = event_ms(lambda: eng.prediction_errors(None, recs, loss_kind=L.LOSS_BERNOULLI, out=out, **kw))
        units_out = sum(SIZES[l] for l in layers) + (N_OUT if head else 0)
        nbytes = rows * (sum(SIZES[l] for l in read) * (4 + 8 + 8) + units_out * 4 * per)
        flop = 2 * rows * (sum(SIZES[l - 1] * SIZES[l] for l in layers if l > 0) + (SIZES[2] * N_OUT if head else 0))
        say("%-34s %8.3f ms  %6.1f MB modelled %7.1f GB/s  %6.1f TFLOP/s  %.3f us per record of %d chains" % (
            name, t, nbytes / 1e6, nbytes / t / 1e6, flop / t / 1e9, t * 1e3 / n_rec, B))
    eng.close()


def _workload(T, B=6000):
    import torch
    import montecarlopredictivecoding_amd.predictive_coding as pc
    import montecarlopredictivecoding_amd.utils.model as um
    dev = torch.device("cuda", 0)
    torch.manual_seed(2)
    dims = [N_IN] + SIZES
    mods = []
    for i in range(1, len(dims)):
        mods += [torch.nn.Linear(dims[i - 1], dims[i]), pc.PCLayer(sample_x_fn=um.sample_x_fn_normal), torch.nn.ReLU()]
    model = torch.nn.Sequential(*mods, torch.nn.Linear(dims[-1], N_OUT)).to(dev)
    model.train()
    data = (torch.rand(B, N_OUT, device=dev) < 0.3).float()
    inputs = torch.zeros(B, N_IN, device=dev)
    tr = pc.PCTrainer(model, T=T, optimizer_x_fn=torch.optim.SGD, optimizer_x_kwargs={"lr": 0.01}, update_p_at="never", plot_progress_at=[])
    return um, model, data, inputs, tr


def torch_replay(model, inputs, data, xs_steps, chunk=10):
    """fp64 sums of the errors and their squares of recorded states, the forward pass replayed in eager torch on the GPU."""
    import torch
    dev = inputs.device
    lins = [m for m in model if isinstance(m, torch.nn.Linear)]
    sums = None
    with torch.no_grad():
        for k0 in range(0, len(xs_steps), chunk):
            part = xs_steps[k0:k0 + chunk]
            xs = [torch.stack([s[l] for s in part]).to(dev, non_blocking=True) for l in range(len(lins) - 1)]
            a = inputs.unsqueeze(0).expand(len(part), -1, -1)
            errs = []
            for l, x in enumerate(xs):
                errs.append(x - torch.nn.functional.linear(a, lins[l].weight, lins[l].bias))
                a = torch.relu(x)
            o = torch.nn.functional.linear(a, lins[-1].weight, lins[-1].bias)
            errs.append(torch.sigmoid(o) - data)
            part_sums = [(e.double().sum(0), (e.double() ** 2).sum(0)) for e in errs]
            sums = part_sums if sums is None else [(s + ps, q + pq) for (s, q), (ps, pq) in zip(sums, part_sums)]
    return sums


def facade(say, T, repeats, with_xs):
    import torch
    import montecarlopredictivecoding_amd.predictive_coding.pc_trainer as pt
    um, model, data, inputs, tr = _workload(T)
    begin = T // 5
    slices = [0]

    def run(variant):
        torch.manual_seed(3)                                 # every run draws the same x0 and the same Langevin noise
        pt._PHILOX_STEPS[0] = 0
        tr.mcpc_errors = dict(begin=begin, layers=(0, 1, 2), outputs="error") if variant == "errors" else None
        res = tr.train_on_batch(inputs=inputs, loss_fn=um.bernoulli_fn, loss_fn_kwargs={"_target": data, "_var": None},
                                callback_after_t=um.random_step, callback_after_t_kwargs={"_pc_trainer": tr}, is_log_progress=False,
                                is_checking_after_callback_after_t=False, is_return_results_every_t=variant == "xs",
                                is_return_xs=variant == "xs")
        if variant == "errors":
            slices[0] = tr.last_record_slices
            return tr.mcpc_last_errors
        if variant == "xs":
            return torch_replay(model, inputs, data, res["xs"][begin:])
        return None

    variants = ["errors", "plain"] + (["xs"] if with_xs else [])
    got = {v: run(v) for v in variants}                                              # warm-up
    times = {v: [] for v in variants}
    for _ in range(repeats):
        for v in variants:
            times[v].append(wall_ms(lambda: run(v))[0])
    say("# cfg-M: 30 | 256-256-256 -> 784, 6000 chains, inference only, T = %d, mcpc_errors from step %d: layers (0, 1, 2) and the read-out" % (T, begin))
    say("#   error (1552 columns, %d samples); %d slice(s) of the record ring; ms per call, min (max) of %d" % (T - begin, slices[0], repeats))
    if with_xs:
        say("#   xs: %.2f GB to pinned host memory, then the forward pass of the sample steps in eager torch" % (4e-9 * T * 6000 * sum(SIZES)))
    for v in variants:
        say("%-6s %9.2f (%9.2f) ms" % (v, min(times[v]), max(times[v])))
    errors, plain = min(times["errors"]), min(times["plain"])
    say("errors - plain = %.2f ms = %.1f %% of the plain call, %.2f us per sample step" % (
        errors - plain, 100 * (errors - plain) / plain, (errors - plain) * 1e3 / (T - begin)))
    if with_xs:
        xs = min(times["xs"])
        say("xs - plain = %.2f ms = %.1f %% of the plain call;  xs / errors = %.2f" % (xs - plain, 100 * (xs - plain) / plain, xs / errors))
        e = got["errors"]
        worst = 0.0
        for name, (s, _) in zip(e.names, got["xs"]):
            worst = max(worst, float(((e.sum[name] - s).abs() / (1e-30 + s.abs().max())).max()))
        say("largest difference of a sum between the two routes, relative to the block's largest sum: %.2e" % worst)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--T", type=int, default=5000)
    ap.add_argument("--T-xs", type=int, default=200)
    ap.add_argument("--part", default=None)
    ap.add_argument("--limit", type=int, default=240, help="seconds a part may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.part is not None:
        import torch
        assert torch.cuda.is_available(), "scripts/pred_err_cost.py needs a GPU"
        warnings.simplefilter("ignore")

        def say(s):
            print(s, flush=True)
        if args.part == "kernel":
            kernel_alone(say)
        elif args.part == "call":
            facade(say, args.T, args.repeats, False)
        else:
            facade(say, args.T_xs, args.repeats, True)
        return 0
    lines = []
    for part in ("kernel", "call", "replay"):
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--T", str(args.T), "--T-xs", str(args.T_xs),
               "--repeats", str(args.repeats)]
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

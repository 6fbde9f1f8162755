#!/usr/bin/env python3
"""Joint histograms counted on the device (csrc/mcpc_hist2d.h, csrc/mcpc_probe.h: mcpc_probe_records; PCTrainer.mcpc_histogram2d): what
the kernels cost, beside the same tensors through eager torch, and what the request adds to a call (developer measurement for
DESIGN.md section 7, profiles/hist2d_cost.txt).

    python scripts/hist2d_cost.py [--out FILE]
    python scripts/hist2d_cost.py --part fig2|units        # one shape, in this process

Without --part the script only drives: every shape runs in a child process of its own under a time limit (--limit seconds), one after
the other, and the first that fails or runs out of time ends the run; --out FILE replaces FILE with what the parts printed.

Shapes: `fig2`, the class-plane panel of the reference's figure_2 (B = 128 chains, layer 0 of 20 units, a 10-class softmax probe,
n = 9 000 samples, 40 x 40 bins), and `units`, pairs of latent units (B = 1 024, a layer of 128 units, 64 pairs, n = 9 000, 50 x 50).
Per shape:
  1. each kernel alone on a record tensor in device memory: HIP events, min (max) of 3 after a warm-up;
  2. the same tensors through eager torch on the same GPU: `fig2` softmax(rec W^T + b) and its projection, then for both shapes
     index_select of the columns, bucketize per axis (with the side classes under / over / nan and the closed last bin, which the kernel
     counts too), one flat bincount; HIP events alike.  On `units` the counts are compared for equality;
  3. one inference-only MCPC call through the facade (PCTrainer.train_on_batch, T = 10 000, mixing 1 000, wall clock around
     synchronised calls, min (max) of 3) with and without the request.
A run without a GPU fails: there is no fallback."""
import argparse
import os
import subprocess
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"fig2": dict(B=128, width=20, C=10, n=9000, bins=40, sizes=(20, 128, 128), n_out=784, T=10000, mixing=1000),
          "units": dict(B=1024, width=128, pairs=64, n=9000, bins=50, sizes=(128, 128, 128), n_out=784, T=10000, mixing=1000)}
REPEATS = 3


def event_ms(fn):
    """min, max ms of REPEATS runs of fn between HIP events, after one warm-up; and fn's last result."""
    import torch
    out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return min(ms), max(ms), out


def eager_classes(v, e):
    """The class of every value as the kernel decides it: bins, then under, over, nan."""
    import torch
    nb = e.numel() - 1
    idx = torch.bucketize(v, e, right=True) - 1
    idx = torch.where(v == e[nb], nb - 1, idx)
    idx = torch.where(v < e[0], nb, idx)
    idx = torch.where(v > e[nb], nb + 1, idx)
    return torch.where(torch.isnan(v), nb + 2, idx)


def eager_counts(rx, ry, px, py, ex, ey):
    """[B, pairs, nx + 3, ny + 3] int64 through index_select, bucketize per axis and one flat bincount."""
    import torch
    n, B = rx.shape[0], rx.shape[1]
    ncx, ncy = ex.numel() + 2, ey.numel() + 2
    cx = eager_classes(torch.index_select(rx, 2, px), ex)
    cy = eager_classes(torch.index_select(ry, 2, py), ey)
    slot = torch.arange(B * px.numel(), device=rx.device).reshape(1, B, px.numel())
    flat = (slot * ncx + cx) * ncy + cy
    return torch.bincount(flat.reshape(-1), minlength=B * px.numel() * ncx * ncy).reshape(B, px.numel(), ncx, ncy)


def kernels(say, name):
    import numpy as np
    import torch
    from montecarlopredictivecoding_amd.engine import hist2d_accumulate, probe_records
    from montecarlopredictivecoding_amd.histogram2d import polygon
    dev = torch.device("cuda", 0)
    s = SHAPES[name]
    B, width, n, nb = s["B"], s["width"], s["n"], s["bins"]
    g = torch.Generator(device=dev).manual_seed(1)
    rec = torch.randn(n, B, width, device=dev, generator=g)
    if name == "fig2":
        C = s["C"]
        W, b = torch.randn(C, width, device=dev, generator=g), torch.randn(C, device=dev, generator=g)
        P = torch.from_numpy(polygon(C)).to(dev)
        e = np.linspace(-1.0, 1.0, nb + 1).astype(np.float32)
        ed = torch.from_numpy(e).to(dev)
        p = torch.empty(n, B, C, device=dev)
        xy = torch.empty(n, B, 2, device=dev)
        counts = torch.zeros(B, 1, nb + 3, nb + 3, dtype=torch.int64, device=dev)
        lo, hi, _ = event_ms(lambda: probe_records(rec, 0, 1, n, W, b, "softmax", out=p))
        say("kernel probe_records softmax %d -> %d      %8.3f (%8.3f) ms" % (width, C, lo, hi))
        lo2, hi2, _ = event_ms(lambda: probe_records(p, 0, 1, n, P, None, "identity", out=xy))
        say("kernel probe_records identity %d -> 2      %8.3f (%8.3f) ms" % (C, lo2, hi2))
        lo3, hi3, _ = event_ms(lambda: hist2d_accumulate(xy, xy, 0, 1, n, [(0, 1)], e, e, counts, accumulate=False))
        say("kernel hist2d 1 pair %d x %d               %8.3f (%8.3f) ms" % (nb, nb, lo3, hi3))
        say("kernels together                           %8.3f ms" % (lo + lo2 + lo3))
        i0, i1 = torch.tensor([0], device=dev), torch.tensor([1], device=dev)

        def eager():
            q = torch.softmax(rec @ W.T + b, dim=2) @ P.T
            return eager_counts(q, q, i0, i1, ed, ed)
        elo, ehi, ec = event_ms(eager)
        say("eager softmax, projection, bucketize, bincount %8.3f (%8.3f) ms" % (elo, ehi))
        say("eager / kernels = %.2f;  cells that differ: %d of %d (the eager softmax is another fp32 softmax: samples next to an edge may"
            " move)" % (elo / (lo + lo2 + lo3), int((ec != counts).sum()), counts.numel()))
        return
    pairs = s["pairs"]
    perm = torch.randperm(width, generator=torch.Generator().manual_seed(2))
    px, py = perm[:pairs].tolist(), perm[pairs:2 * pairs].tolist()
    e = np.linspace(-3.0, 3.0, nb + 1).astype(np.float32)
    ed = torch.from_numpy(e).to(dev)
    for pool in (False, True):
        counts = torch.zeros((pairs, nb + 3, nb + 3) if pool else (B, pairs, nb + 3, nb + 3), dtype=torch.int64, device=dev)
        lo, hi, _ = event_ms(lambda: hist2d_accumulate(rec, rec, 0, 1, n, list(zip(px, py)), e, e, counts, pool=pool, accumulate=False))
        say("kernel hist2d %d pairs %d x %d pool=%d       %8.3f (%8.3f) ms" % (pairs, nb, nb, pool, lo, hi))
        if not pool:
            per_chain, k_ms = counts.clone(), lo
    dx, dy = torch.tensor(px, device=dev), torch.tensor(py, device=dev)
    elo, ehi, ec = event_ms(lambda: eager_counts(rec, rec, dx, dy, ed, ed))
    say("eager index_select, bucketize, bincount    %8.3f (%8.3f) ms" % (elo, ehi))
    say("eager / kernel = %.2f;  counts equal: %s" % (elo / k_ms, bool(torch.equal(ec, per_chain))))


def facade(say, name):
    import torch
    import montecarlopredictivecoding_amd.predictive_coding as pc
    import montecarlopredictivecoding_amd.predictive_coding.pc_trainer as pt
    import montecarlopredictivecoding_amd.utils.model as um
    dev = torch.device("cuda", 0)
    s = SHAPES[name]
    sizes, n_out, B, T, mixing, nb = s["sizes"], s["n_out"], s["B"], s["T"], s["mixing"], s["bins"]
    torch.manual_seed(1)
    model = um.get_model(dict(input_size=sizes[0], hidden_size=sizes[1], hidden2_size=sizes[2], output_size=n_out, activation_fn="relu"),
                         True, sample_x_fn=um.sample_x_fn_normal)
    data = (torch.rand(B, n_out, device=dev) < 0.3).float()
    inputs = torch.zeros(B, sizes[0], device=dev)
    tr = pc.PCTrainer(model, T=T, optimizer_x_fn=torch.optim.SGD, optimizer_x_kwargs={"lr": 0.01}, update_p_at="never", plot_progress_at=[])
    if name == "fig2":
        request = dict(begin=mixing, probe=dict(layer=0, linear=torch.nn.Linear(sizes[0], s["C"]).to(dev)), bins=nb, range=(-1, 1))
    else:
        perm = torch.randperm(sizes[0], generator=torch.Generator().manual_seed(2)).tolist()
        request = dict(begin=mixing, x=(0, perm[:s["pairs"]]), y=(0, perm[s["pairs"]:2 * s["pairs"]]), bins=nb, range=(-3, 3))

    def run(with_request):
        torch.manual_seed(3)
        pt._PHILOX_STEPS[0] = 0
        tr.mcpc_histogram2d = request if with_request else None
        torch.cuda.synchronize()
        t = time.perf_counter()
        tr.train_on_batch(inputs=inputs, loss_fn=um.bernoulli_fn, loss_fn_kwargs={"_target": data, "_var": None},
                          callback_after_t=um.random_step, callback_after_t_kwargs={"_pc_trainer": tr}, is_log_progress=False,
                          is_checking_after_callback_after_t=False, is_return_results_every_t=False)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3
    times = {True: [], False: []}
    run(True), run(False)                                                            # warm-up
    for _ in range(REPEATS):
        for w in (True, False):
            times[w].append(run(w))
    h = None
    run(True)
    h = tr.mcpc_last_histogram2d
    a, b = min(times[False]), min(times[True])
    say("facade %s -> %d, %d chains, T = %d, %d samples: plain %9.2f (%9.2f) ms, with mcpc_histogram2d %9.2f (%9.2f) ms: + %.2f ms = "
        "%.1f %%, %d slices; every grid sums to n: %s"
        % ("-".join(str(v) for v in sizes), n_out, B, T, T - mixing, a, max(times[False]), b, max(times[True]), b - a, 100 * (b - a) / a,
           tr.last_record_slices, bool((h.total() == h.N).all())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default=None, choices=sorted(SHAPES))
    ap.add_argument("--limit", type=int, default=300, help="seconds a part may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.part is not None:
        import torch
        assert torch.cuda.is_available(), "scripts/hist2d_cost.py needs a GPU"
        warnings.simplefilter("ignore")

        def say(s):
            print(s, flush=True)
        s = SHAPES[args.part]
        say("# %s: B = %d, width %d, n = %d, %d x %d bins, ms, min (max) of %d" % (args.part, s["B"], s["width"], s["n"], s["bins"], s["bins"],
                                                                                REPEATS))
        kernels(say, args.part)
        facade(say, args.part)
        return 0
    lines = []
    for part in ("fig2", "units"):
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part]
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

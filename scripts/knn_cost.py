#!/usr/bin/env python3
"""The nearest-neighbour KL divergence between two sample clouds on the device (csrc/mcpc_knn.h, PCTrainer.mcpc_cloud, cloud.py): what
the search costs alone, what the request adds to a call, and the estimate three ways (developer measurement for DESIGN.md section 7,
profiles/knn_cost.txt).

    python scripts/knn_cost.py [--repeats 3] [--out FILE]
    python scripts/knn_cost.py --part kernel|call|kl      # one part, in this process

Without --part the script only drives: every part runs in a child process of its own under a time limit (--limit seconds), one after
the other, and the first that fails or runs out of time ends the run; --out FILE replaces FILE with what the parts printed.

  kernel  knn_accumulate alone (HIP events; the workspace allocated outside the timed window) on Gaussian clouds of d = 5 at figure 5's
          thinned size, 121 600 x 121 600 (9 500 steps x 256 chains / 20), and at its full size, 2 432 000 x 2 432 000, for k = 2 (x
          into itself) and k = 1 (x into y): achieved pair distances per second beside the VALU instruction-count bound of the header
          (5 packed subtract-FMA pairs for two pairs of rows + the selection, against 256 CUs x 64 lanes x 2.4 GHz).
  call    one inference-only MCPC call of figure 5's shape (20-128-128 -> 784, 256 chains, mixing 500, sampling 9 500) through the
          facade, wall clock around synchronised calls, three ways that alternate: plain, with mcpc_cloud = dict(begin=500, layer=2,
          units=<5>), and with is_return_results_every_t=True, is_return_xs=True (what figure_5.py does: every layer of every step
          to the host).
  kl      D(x || y) of two Gaussian clouds of figure 5's shape, d = 5: on the device (cloud.kl_divergence) thinned by 20 and
          unthinned; thinned through torch.cdist + topk in chunks on the same GPU; thinned through the reference's route, scipy's
          cKDTree (k = 2 and k = 1, eps=.01) on a host copy, the copy included -- if scipy imports.
A run without a GPU fails: there is no fallback."""
import argparse
import math
import os
import subprocess
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIG5 = dict(sizes=(20, 128, 128), n_out=784, B=256, mixing=500, sampling=9500, indent=20, units=(3, 17, 40, 77, 101))
LANE_RATE = 256 * 64 * 2.4e9                     # VALU lane-instructions per second: CUs x lanes x clock


def valu_per_pair(d, k):
    """Lane-instructions per pair distance as the kernel is written: d packed subtracts and d packed FMAs serve two pairs; the selection
    is one fminf and a compare-exchange (fminf, fmaxf) per further slot."""
    kt = 1 if k <= 1 else 2 if k <= 2 else 4
    return d + 1 + 2 * (kt - 1)


def wall_ms(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def clouds(n, d, dev):
    import torch
    g = torch.Generator(device="cpu").manual_seed(17)
    x = torch.randn(n, d, generator=g)
    y = 0.4 + 1.2 * torch.randn(n, d, generator=g)
    return x.to(dev), y.to(dev)


def part_kernel(say, repeats):
    import torch
    from montecarlopredictivecoding_amd.engine import knn_accumulate, knn_workspace_bytes
    dev = torch.device("cuda", 0)
    d = len(FIG5["units"])
    full = FIG5["sampling"] * FIG5["B"]
    say("# knn_accumulate alone, d = %d, Gaussian clouds, HIP events, min (max) of %d; bound: VALU lane-instructions per pair against "
        "%.1fe12 per second" % (d, repeats, LANE_RATE / 1e12))
    for n in (full // FIG5["indent"], full):
        x, y = clouds(n, d, dev)
        for k, ref, what in ((2, x, "x into x"), (1, y, "x into y")):
            best = torch.empty(n, k, device=dev)
            ws = torch.empty(max(knn_workspace_bytes(n, n, d, k), 4), dtype=torch.uint8, device=dev)
            knn_accumulate(x, ref, k, best, workspace=ws)                             # warm-up
            torch.cuda.synchronize()
            ms = []
            for _ in range(repeats):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                knn_accumulate(x, ref, k, best, workspace=ws)
                b.record()
                torch.cuda.synchronize()
                ms.append(a.elapsed_time(b))
            pairs = float(n) * n
            bound = LANE_RATE / valu_per_pair(d, k)
            say("%9d x %9d  k = %d (%s)  %10.2f (%10.2f) ms  %.3fe12 pairs/s  = %.0f %% of the bound %.2fe12 (%d lane-instructions per pair)"
                % (n, n, k, what, min(ms), max(ms), pairs / (min(ms) * 1e-3) / 1e12, 100 * pairs / (min(ms) * 1e-3) / bound,
                   bound / 1e12, valu_per_pair(d, k)))


def part_call(say, repeats):
    import torch
    import montecarlopredictivecoding_amd.predictive_coding as pc
    import montecarlopredictivecoding_amd.predictive_coding.pc_trainer as pt
    import montecarlopredictivecoding_amd.utils.model as um
    dev = torch.device("cuda", 0)
    sizes, n_out, B, mixing = FIG5["sizes"], FIG5["n_out"], FIG5["B"], FIG5["mixing"]
    T = mixing + FIG5["sampling"]
    torch.manual_seed(1)
    model = um.get_model(dict(input_size=sizes[0], hidden_size=sizes[1], hidden2_size=sizes[2], output_size=n_out, activation_fn="relu"),
                         True, sample_x_fn=um.sample_x_fn_normal)
    data = (torch.rand(B, n_out, device=dev) < 0.3).float()
    inputs = torch.zeros(B, sizes[0], device=dev)
    tr = pc.PCTrainer(model, T=T, optimizer_x_fn=torch.optim.SGD, optimizer_x_kwargs={"lr": 0.05}, update_p_at="never", plot_progress_at=[])
    slices = {}

    def run(variant):
        torch.manual_seed(3)                                 # every run draws the same x0 and the same Langevin noise
        pt._PHILOX_STEPS[0] = 0
        tr.mcpc_cloud = dict(begin=mixing, layer=2, units=FIG5["units"]) if variant == "cloud" else None
        rec = variant == "xs"
        res = tr.train_on_batch(inputs=inputs, loss_fn=um.bernoulli_fn, loss_fn_kwargs={"_target": data, "_var": None},
                                callback_after_t=um.random_step, callback_after_t_kwargs={"_pc_trainer": tr}, is_log_progress=False,
                                is_checking_after_callback_after_t=False, is_return_results_every_t=rec, is_return_xs=rec)
        slices[variant] = tr.last_record_slices
        if variant == "cloud":
            return tr.mcpc_last_cloud.flat()
        if rec:
            return torch.concatenate([r[2] for r in res["xs"][mixing:]])[:, list(FIG5["units"])]
        return None

    variants = ["cloud", "plain", "xs"]
    got = {v: run(v) for v in variants}                                              # warm-up
    same = bool(torch.equal(got["cloud"].cpu(), got["xs"].cpu()))
    times = {v: [] for v in variants}
    for _ in range(repeats):
        for v in variants:
            times[v].append(wall_ms(lambda: run(v))[0])
    say("# figure 5's call: %s -> %d, %d chains, inference only, T = %d, the cloud: 5 units of layer 2 from step %d on = %d rows (%.1f MB)"
        % ("-".join(str(s) for s in sizes), n_out, B, T, mixing, got["cloud"].shape[0], got["cloud"].numel() * 4 / 1e6))
    say("#   slices of the record ring: cloud %d, xs %d; ms per call, min (max) of %d; the cloud equals the recording's rows bitwise: %s"
        % (slices["cloud"], slices["xs"], repeats, same))
    for v, what in (("plain", "(a)"), ("cloud", "(b) mcpc_cloud"), ("xs", "(c) is_return_xs, every step to the host")):
        say("%-5s %9.2f (%9.2f) ms  %s" % (v, min(times[v]), max(times[v]), what))
    a, b, c = min(times["plain"]), min(times["cloud"]), min(times["xs"])
    say("(b) - (a) = %.2f ms = %.1f %% of the plain call;  (c) - (a) = %.2f ms = %.1f %%" % (b - a, 100 * (b - a) / a, c - a, 100 * (c - a) / a))


def part_kl(say, repeats):
    import torch
    from montecarlopredictivecoding_amd.cloud import kl_divergence, kl_from_sqdist
    dev = torch.device("cuda", 0)
    d, indent = len(FIG5["units"]), FIG5["indent"]
    full = FIG5["sampling"] * FIG5["B"]
    x, y = clouds(full, d, dev)
    xt, yt = x[::indent].contiguous(), y[::indent].contiguous()
    n = xt.shape[0]

    def cdist_topk():
        """The same estimate through torch on the same GPU: distances of a block of rows to every row, topk, in chunks of 4096 rows."""
        r2, s2 = [], []
        for i in range(0, n, 4096):
            blk = xt[i:i + 4096]
            r2.append(torch.topk(torch.cdist(blk, xt), 2, dim=1, largest=False).values[:, 1] ** 2)
            s2.append(torch.topk(torch.cdist(blk, yt), 1, dim=1, largest=False).values[:, 0] ** 2)
        return kl_from_sqdist(torch.cat(r2), torch.cat(s2), n, n, d)

    def best_of(fn, reps):
        fn()                                                                          # warm-up
        t = [wall_ms(fn) for _ in range(reps)]
        return min(m for m, _ in t), max(m for m, _ in t), t[0][1]

    say("# D(x || y), two Gaussian clouds of figure 5's shape (d = %d): thinned by %d = %d rows each, unthinned = %d rows each; wall "
        "clock around synchronised calls, min (max) of %d" % (d, indent, n, full, repeats))
    lo, hi, kl_dev = best_of(lambda: kl_divergence(xt, yt), repeats)
    say("device, thinned      %10.2f (%10.2f) ms  KL = %.9f" % (lo, hi, float(kl_dev)))
    lo, hi, kl_t = best_of(cdist_topk, repeats)
    say("cdist + topk, thinned %9.2f (%10.2f) ms  KL = %.9f  (differs from the device's by %.3g)" % (lo, hi, float(kl_t), abs(float(kl_t) - float(kl_dev))))
    try:
        from scipy.spatial import cKDTree
    except ImportError as exc:
        say("scipy cKDTree, thinned: not measured, scipy does not import here (%s)" % exc)
    else:
        import numpy as np

        def trees():
            xh, yh = xt.cpu().numpy(), yt.cpu().numpy()
            r = cKDTree(xh).query(xh, k=2, eps=.01, p=2)[0][:, 1]
            s = cKDTree(yh).query(xh, k=1, eps=.01, p=2)[0]
            return -np.log(r / s).sum() * d / n + np.log(n / (n - 1.0))
        ms, kl_h = wall_ms(trees)
        say("scipy cKDTree eps=.01 on a host copy, thinned (once) %10.2f ms  KL = %.9f  (differs from the device's by %.3g; "
            "d log 1.01 = %.3g)" % (ms, kl_h, abs(kl_h - float(kl_dev)), d * math.log(1.01)))
    lo, hi, kl_full = best_of(lambda: kl_divergence(x, y), max(1, repeats - 1))
    say("device, unthinned    %10.2f (%10.2f) ms  KL = %.9f" % (lo, hi, float(kl_full)))


PARTS = {"kernel": part_kernel, "call": part_call, "kl": part_kl}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--part", default=None, choices=sorted(PARTS))
    ap.add_argument("--limit", type=int, default=240, help="seconds a part may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.part is not None:
        import torch
        assert torch.cuda.is_available(), "scripts/knn_cost.py needs a GPU"
        warnings.simplefilter("ignore")

        def say(s):
            print(s, flush=True)
        PARTS[args.part](say, args.repeats)
        return 0
    lines = []
    for part in ("kernel", "call", "kl"):
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

"""The Hebbian flush against fp64 sums of the recorded states, on every plan `plan_flush` (csrc/mcpc_plan.h) can choose; `flush_spill`
(csrc/mcpc_flush.hip) executes the planned launches.

A learning call records x_t on every step of its accumulation window; the fp64 sums of the same window are then built from the records
(as tests/test_gpu_headline.py does):  dF/dW_j = -sum e_j^T f(x_{j-1}) for the latent Linears, +sum e_o^T f(x_L) for the
read-out, the bias sums alike (Linear 0's -sum e_1 through e0sum / mcpc_dw0_kernel).  Every entry is compared with a bound relative to
ITS OWN sum of |terms|, and `mcpc_last_flush_plan` proves which kernels, K-splits and layouts computed it: the text the planner
formatted for the flush that ran -- every runner holds it to the "text" mcpc_debug_run_plan gives, for the device's own CU count, for
the run's last flushing item.

EXACT-IMAGE PROBLEMS isolate the flush (the `_flush_problem` of test_gpu_accuracy.py): all-zero weights and biases, identity
activations, a Gaussian read-out with var = 1.  Every prediction is an exact 0, so e_l = x_l, f(x_l) = x_l and e_o = -y: the spilled images
ARE the recorded states, bit for bit.  The states are chosen by the test through NOISE_EXTERNAL: with lr = 1 and noise_var = 1 the SGD step
(csrc/mcpc_kernels.h) is  x_{t+1} = x_t - lr g + sqrt(noise_var lr) xi_t = x_t - x_t + xi_t = xi_t  (g = e_l exactly: the back-projection
of zero weights is 0), so the state of step t + 1 is the injected kick of step t.  The arithmetic being bounded is then the flush's alone:

  fp16-piece form (mcpc_heb7_kernel, csrc/mcpc_hebbian.h + mcpc_gemm_f16.h).  Both operand images are scaled by one power of two per
  image and segment (exact) and cut into two fp16 pieces; the three piece products e_h a_h, e_h a_m, e_m a_h enter a 16x16x32 fp16 MFMA
  exactly, e_m a_m is dropped: per term |error| <= C_OP |e a|, C_OP = 3 x 2^-22 (test_gpu_accuracy.py's derivation).  The MFMA chain of a
  split does one fp32 rounding of its running sum per MFMA, three MFMAs per 32-row stage: 3 ceil(rps / 32) x 2^-24 of sum |terms| (rps =
  rows per split).  The fixed-order slab reduction (mcpc_reduce_jobs_kernel) adds the ksplit partial sums and then the flush's total to G:
  ksplit roundings, and one more per flush of the window:
      W:  (C_OP + (3 ceil(rps / 32) + ksplit + n_flush) 2^-24) sum |terms|
  fp32-MFMA form (mcpc_heb_kernel, tuning heb_fp32=1): operands are the fp32 values, no C_OP; each term may be rounded once by the
  16x16x4 fp32 MFMA, whose chain rounds once per 4 rows:
      W:  ((1 + ceil(rps / 4) + ksplit + n_flush) 2^-24) sum |terms|
  streaming form (mcpc_dw_kernel): fp32 FMA chains, exact products; a split's sum is at most rps - 1 additions deep:
      W:  ((rps + ksplit + n_flush) 2^-24) sum |terms|
  bias sums (VALU column sums of the fp32 error image, every form; any order of at most rps - 1 additions per split):
      b:  ((rps + ksplit + n_flush) 2^-24) sum |e|
  Linear 0's bias: e0sum adds e_1 step by step (n_acc roundings), mcpc_dw0_kernel sums the chains in a tree of at most Bpad - 1 additions:
      b0: ((n_acc + Bpad) 2^-24) sum |e_1|
`rps`, `ksplit` are read from mcpc_last_flush_plan (the planner is not copied here).  The one-exponent-per-image scaling keeps a value
2^-rho below its image's maximum exact to 22 bits while rho <= 18 (test_gpu_accuracy.py: RANGE); the images here are Gaussian, whose
smallest values lose more but weigh nothing against an entry's sum |terms| (their absolute error is 2^-39 of the image's maximum).

REALISTIC PROBLEMS (random weights, tanh / ReLU, Bernoulli read-out, Philox noise) serve the step-kernel axis, whose spill writers
differ: the errors are computed by the step kernel (fp16-piece GEMMs, tanh by v_exp), so the bound is the 1e-5 sum |terms| the headline
window test uses.

SCALE HISTORY.  The fp16 form scales each spilled image by the largest |value| of ITS segment (KParams::spillmax, one word per ring part,
reset when the part is refilled).  Here consecutive segments differ by 2^+-16 and one segment is all zero; every segment writes a
different group of units of every layer, so that each entry of the gradient holds the terms of ONE segment and is held to that segment's
own bound -- a flush that read another part's maximum loses 16 bits (2^-6 of its terms) or overflows fp16 (inf / NaN), and entries that
pair two groups must come out exactly 0.

TEETH.  For every case the fp64 contribution of every 32-row stage of every flush (rows = step x padded chain, in flush order) is
computed, and the smallest of them still exceeds 20 x the tolerance of an entry it touches: a dropped or doubled stage -- the unit of
the Hebbian kernels' pipeline -- fails the test.  The same holds for the last unit tile of a ragged 17-tile group.
"""
import functools
import math
import re

import numpy as np
import pytest
import torch

from tests import parity_log

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
U24 = 2.0 ** -24
C_OP = 3.0 * 2.0 ** -22
N_IN = 8
TEETH = 20.0
GROUP = "Hebbian flush vs fp64 of the recorded states (error / bound)"

_LAUNCH = re.compile(r"^(heb7?)<(\d+),(\d+)(,T)?>x(\d+)(?:\*(\d+))?$")


def parse_plan(s):
    """'heb7<17,2>x1+heb7<16,2>x2 ksplit=12 rps=1536 tm' -> dict(kernel='heb7', launches=[(te, ra, swapped, n_mt, n_nt)...], ksplit, rps, layout);
    'dw tiles=6 ksplit=8 rps=64 rm' -> kernel 'dw', launches []."""
    m = re.match(r"^(.+) ksplit=(\d+) rps=(\d+) (tm|rm)$", s)
    assert m, f"unparsable flush plan {s!r}"
    body, ksplit, rps, layout = m.group(1), int(m.group(2)), int(m.group(3)), m.group(4)
    if body.startswith("dw tiles="):
        return dict(kernel="dw", launches=[], ksplit=ksplit, rps=rps, layout=layout, text=s)
    launches, kern = [], None
    for tok in body.split("+"):
        lm = _LAUNCH.match(tok)
        assert lm, f"unparsable launch {tok!r} in {s!r}"
        assert kern in (None, lm.group(1)), s
        kern = lm.group(1)
        launches.append((int(lm.group(2)), int(lm.group(3)), lm.group(4) is not None, int(lm.group(5)), int(lm.group(6) or 1)))
    return dict(kernel=kern, launches=launches, ksplit=ksplit, rps=rps, layout=layout, text=s)


def instantiations(p, heb171=False):
    """Kernel instantiations a parsed plan launched, as plan_flush names them: 'heb7<17,2>', 'heb<4,2,T>', 'heb7<17,1>/heb171', 'dw'."""
    if p["kernel"] == "dw":
        return {"dw"}
    out = set()
    for te, ra, sw, _, _ in p["launches"]:
        name = f"{p['kernel']}<{te},{ra}{',T' if sw else ''}>"
        out.add(name + "/heb171" if heb171 and p["kernel"] == "heb7" and (te, ra) == (17, 1) else name)
    return out


def w_coeff(p, n_flush):
    k = p["kernel"]
    if k == "heb7":
        return C_OP + (3 * math.ceil(p["rps"] / 32) + p["ksplit"] + n_flush) * U24
    if k == "heb":
        return (1 + math.ceil(p["rps"] / 4) + p["ksplit"] + n_flush) * U24
    return (p["rps"] + p["ksplit"] + n_flush) * U24


def b_coeff(p, n_flush):
    return (p["rps"] + p["ksplit"] + n_flush) * U24


def _bpad(B):
    return (B + 31) // 32 * 32


def _planned_text(sizes, n_out, B, tuning, run):
    """The flush texts, Linear 1 first, that mcpc_debug_run_plan plans on this device for the last flushing item of `run`."""
    from tests.plan_util import run_plan
    props = torch.cuda.get_device_properties(0)
    rp = run_plan(sizes=sizes, n_out=n_out, batch=B, tuning=tuning, n_cu=props.multi_processor_count, total_mem=props.total_memory,
                  n_in=N_IN, run=run)
    assert rp["flushes"], "the run accumulates: it flushes"
    return rp["flushes"][-1]["text"]


def _pad_rows(x, B):
    """[T, B, n] -> [T, Bpad, n] with zero rows for the padding chains (the spilled image's row order: step, then chain)."""
    if x.shape[1] == _bpad(B):
        return x
    return torch.cat([x, x.new_zeros(x.shape[0], _bpad(B) - B, x.shape[2])], 1)


def _stage_ratio(E, A, tolW, B):
    """Smallest over the 32-row stages of every flush of max over entries of |stage contribution| / tolerance (stages with a zero operand
    contribute nothing and are skipped).  E [T, B, ne], A [T, B, na] in fp64."""
    Ep, Ap = _pad_rows(E, B), _pad_rows(A, B)
    T, Bp = Ep.shape[0], Ep.shape[1]
    # a flush starts at a step and Bpad % 32 == 0: its stages are 32 chains of one step
    Es = Ep.reshape(T * Bp // 32, 32, -1)
    As = Ap.reshape(T * Bp // 32, 32, -1)
    inv = torch.where(tolW > 0, 1.0 / tolW.clamp_min(1e-300), torch.zeros_like(tolW))
    best = math.inf
    for s0 in range(0, Es.shape[0], 32):
        e, a = Es[s0:s0 + 32], As[s0:s0 + 32]
        live = (e.abs().amax((1, 2)) > 0) & (a.abs().amax((1, 2)) > 0)
        if not bool(live.any()):
            continue
        c = torch.bmm(e[live].transpose(1, 2), a[live])            # [stages, ne, na]
        r = (c.abs() * inv).amax((1, 2))
        best = min(best, float(r.min()))
    return best


def _check_linear(tag, j, got_W, got_b, want_W, want_b, mag_W, mag_b, cW, cb):
    """Assert |got - want| <= c sum|terms| per entry (exactly equal where sum|terms| = 0), log error / bound; return (worst W, worst b)."""
    worst = []
    for what, got, want, mag, c in (("dW", got_W, want_W, mag_W, cW), ("db", got_b, want_b, mag_b, cb)):
        tol = c * mag
        err = (got - want).abs()
        zero = tol == 0
        assert bool(torch.isfinite(got).all()), f"{tag} Linear {j} {what}: non-finite entries"
        assert not bool((err[zero] > 0).any()), f"{tag} Linear {j} {what}: entries without terms are not 0"
        ratio = torch.where(zero, torch.zeros_like(err), err / tol.clamp_min(1e-300))
        parity_log.close(GROUP, f"{tag}: Linear {j} {what}", ratio.cpu().numpy(), np.zeros(tuple(ratio.shape)), rtol=0, atol=1.0,
                         err_msg=f"(max error / bound; bound coefficient {c:.3e} of sum|terms|)")
        worst.append(float(ratio.max()))
    return worst


# ---- exact-image problems ------------------------------------------------------------------------------------------------------
def _exact_states(sizes, B, T, seed, seg_len=None, seg_exps=None):
    """States x_t [T][B][n_l] of the exact-image problem: Gaussian, or (scale history) segment k of `seg_len` steps non-zero only in unit
    group k of every layer and scaled by 2^seg_exps[k] (None: all zero)."""
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(T, B, n, generator=g, dtype=torch.float32) for n in sizes]
    if seg_exps is not None:
        ng = len(seg_exps)
        for x, n in zip(xs, sizes):
            gsz = n // ng
            assert gsz >= 1
            mask = torch.zeros(T, 1, n)
            for t in range(T):
                k = t // seg_len
                if seg_exps[k] is not None:
                    mask[t, 0, k * gsz:(k + 1) * gsz] = 2.0 ** seg_exps[k]
            x *= mask
    return xs


def _run_exact(sizes, n_out, B, T, tuning, seed=1, seg_len=None, seg_exps=None):
    """One learning call of the exact-image problem: accumulation and records over all T steps.  Returns the engine's gradients, the
    records, the target, the flush plans and the step kernel that ran."""
    from montecarlopredictivecoding_amd import _lib as L
    from montecarlopredictivecoding_amd.engine import Engine
    dims = [N_IN] + list(sizes) + ([n_out] if n_out else [])
    W = [torch.zeros(dims[j + 1], dims[j], device=DEV) for j in range(len(dims) - 1)]
    b = [torch.zeros(dims[j + 1], device=DEV) for j in range(len(dims) - 1)]
    states = [x.to(DEV) for x in _exact_states(sizes, B, T, seed, seg_len, seg_exps)]
    g = torch.Generator().manual_seed(seed + 1000)
    y = (torch.rand(B, n_out, generator=g) * 2 - 1).to(DEV) if n_out else None
    eng = Engine(sizes, [L.ACT_IDENTITY] * len(sizes), N_IN, n_out, B, device=DEV, tuning=tuning)
    try:
        eng.bind_params(W, b)
        eng.bind_inputs(None)
        if n_out:
            eng.bind_target(y)
        eng.load_state([x[0].contiguous() for x in states])
        # xi_t = x_{t+1}; the last kick is never seen
        ext = [torch.cat([x[1:], torch.zeros_like(x[:1])]).contiguous() for x in states]
        res = eng.run(T, loss_kind=L.LOSS_GAUSSIAN if n_out else L.LOSS_NONE, loss_var=1.0, lr=1.0, noise_mode=L.NOISE_EXTERNAL,
                      noise_var=1.0, ext_noise=ext, acc_begin=0, acc_end=T, rec_begin=0, rec_stride=1, rec_count=T, rec_x=True)
        grads = []
        for j in range(len(dims) - 1):
            gW, gb = torch.empty_like(W[j]), torch.empty_like(b[j])
            eng.read_param_grads(j, gW, gb)
            grads.append((gW, gb))
        eng.sync_check()
        plans = {j: eng.last_flush_plan(j) for j in range(1, len(dims) - 1)}
        assert eng.last_flush_plan(0) == "" and eng.last_flush_plan(len(dims) - 1) == ""
        assert [plans[j] for j in sorted(plans)] == _planned_text(sizes, n_out, B, tuning, dict(
            T=T, t_begin=0, n_steps=T, acc_begin=0, acc_end=T, update_x=1, xopt_kind=L.XOPT_SGD, noise_mode=L.NOISE_EXTERNAL,
            loss_kind=L.LOSS_GAUSSIAN if n_out else L.LOSS_NONE))
        q = eng.query()
        step = eng.last_step_kernel()
    finally:
        eng.close()
    for r, x in zip(res.rec_x, states):
        assert torch.equal(r, x), "the exact-image problem's states are not the injected ones (sign / scale convention of the kick)"
    return dict(grads=grads, rec=res.rec_x, y=y, plans=plans, spill_slots=q["spill_slots"], step=step)


def _ring_segment(tuning, spill_slots):
    """Steps per flush segment: the whole ring with no_overlap=1, else one of its ring_parts (default 3) parts."""
    t = dict(kv.split("=") for kv in (tuning or "").split(",") if kv)
    if t.get("no_overlap") == "1":
        return spill_slots
    parts = int(t.get("ring_parts", 3))
    return spill_slots // parts if spill_slots >= parts else spill_slots // 2


def _check_exact(tag, sizes, n_out, B, T, tuning, out, seg_len):
    """Hold every Linear of an exact-image run to its derived bound; teeth; return per-Linear parsed plans and the worst error / bound."""
    rec = [r.double() for r in out["rec"]]
    n_flush = math.ceil(T / seg_len)
    assert T <= seg_len or T % seg_len == 0, "equal segments: the last flush's plan is every flush's plan"
    heb171 = "heb171=1" in (tuning or "")
    parsed, worst, teeth = {}, 0.0, math.inf
    L_ = len(sizes)
    for j in range(L_ + (1 if n_out else 0)):
        gW, gb = (t.double() for t in out["grads"][j])
        if j == 0:
            # Linear 0 sees a zero pseudo-input: dW0 == 0, db0 = -sum e_1 = -sum x_1
            assert not bool(gW.any())
            e = rec[0]
            want, mag = -e.sum((0, 1)), e.abs().sum((0, 1))
            tol = (T + _bpad(B)) * U24 * mag
            err = (gb - want).abs()
            assert bool((err <= tol).all()), f"{tag} Linear 0 db: {float((err / tol.clamp_min(1e-300)).max()):.3e} of the bound"
            ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.zeros_like(err))
            parity_log.close(GROUP, f"{tag}: Linear 0 db", ratio.cpu().numpy(), np.zeros(tuple(ratio.shape)), rtol=0, atol=1.0)
            worst = max(worst, float(ratio.max()))
            continue
        p = parse_plan(out["plans"][j])
        parsed[j] = p
        A = rec[j - 1]
        if j < L_:
            E, sign = rec[j], -1.0
        else:
            E, sign = (-out["y"].double())[None].expand(T, B, n_out), 1.0
        want_W = sign * torch.einsum("tbu,tbi->ui", E, A)
        mag_W = torch.einsum("tbu,tbi->ui", E.abs(), A.abs())
        want_b, mag_b = sign * E.sum((0, 1)), E.abs().sum((0, 1))
        cW, cb = w_coeff(p, n_flush), b_coeff(p, n_flush)
        wW, wb = _check_linear(tag, j, gW, gb, want_W, want_b, mag_W, mag_b, cW, cb)
        worst = max(worst, wW, wb)
        tt = _stage_ratio(E, A, cW * mag_W, B)
        teeth = min(teeth, tt)
        print(f"[flush {tag}] Linear {j} {A.shape[2]}->{E.shape[2]}: {p['text']}  dW {wW:.3f}, db {wb:.3f} of the bound "
              f"(W: {cW:.2e} sum|terms|); smallest 32-row stage = {tt:.1f} x its entries' tolerance")
        assert wW <= 1.0 and wb <= 1.0
        assert tt > TEETH, f"{tag} Linear {j}: a 32-row stage is only {tt:.1f} x the tolerance"
        if p["kernel"] != "dw":
            et = (E.shape[2] + 15) // 16
            if any(te == 17 and n_mt * 17 > et for te, _, sw, n_mt, _ in p["launches"] if not sw):
                # ragged 17-tile group: the last unit tile of the output must be far above its tolerance
                last = slice(16 * (et - 1), E.shape[2])
                r = float((want_W[last].abs() / (cW * mag_W[last]).clamp_min(1e-300)).max())
                print(f"[flush {tag}] Linear {j}: ragged group ({et} tiles), last unit tile = {r:.0f} x its tolerance")
                assert r > TEETH
    return parsed, worst, teeth, heb171


# Each row: one Linear in -> out (unpadded), nets chaining them; {Linear j: the launches of its fp16-form plan}.  The fp32 form launches
# the same instantiations of mcpc_heb_kernel; mcpc_dw_kernel serves the shapes neither tiling takes.
SHAPE_NETS = {
    # 16->256 swapped <1,2,T>; 256->512 <16,2>x2; 512->256 two activation-tile groups; 256->240 <16,2> with 15 of 16 tiles
    "16-256-512-256-240": ([16, 256, 512, 256], 240, {1: "<1,2,T>x1", 2: "<16,2>x2", 3: "<16,2>x1*2", 4: "<16,2>x1"}),
    # 32->256 swapped <2,2,T>; 256->128 <8,2>; 128->128 <8,1>; 128->272 <17,1>
    "32-256-128-128-272": ([32, 256, 128, 128], 272, {1: "<2,2,T>x1", 2: "<8,2>x1", 3: "<8,1>x1", 4: "<17,1>x1"}),
    # 64->256 swapped <4,2,T>; 128->144 <16,1> with 9 of 16 tiles
    "64-256-128-144": ([64, 256, 128], 144, {1: "<4,2,T>x1", 2: "<8,2>x1", 3: "<16,1>x1"}),
    # 256->528 = 17 + 16 tiles
    "128-256-528": ([128, 256], 528, {1: "<16,1>x1", 2: "<17,2>x1+<16,2>x1"}),
    # 128->784 = 17 + 16 + 16 tiles on RA = 1
    "256-128-784": ([256, 128], 784, {1: "<8,2>x1", 2: "<17,1>x1+<16,1>x2"}),
    # ragged 17-tile groups: 19 and 20 output tiles in two groups of 17
    "128-256-304": ([128, 256], 304, {1: "<16,1>x1", 2: "<17,2>x2"}),
    "128-256-320": ([128, 256], 320, {2: "<17,2>x2"}),
    "128-256-272": ([128, 256], 272, {2: "<17,2>x1"}),
    # the streaming kernel, widths that are not multiples of 64 (48, 100 -> 112, 60 -> 64, 200 -> 208)
    "32-48-100-60": ([32, 48, 100], 60, {1: "dw", 2: "dw", 3: "dw"}),
    "64-200-784": ([64, 200], 784, {1: "dw", 2: "dw"}),
}
FORMS = {"f16": None, "fp32": "heb_fp32=1"}
SHAPE_B, SHAPE_T = 64, 8

HEB_INSTANTIATIONS = ["<1,2,T>", "<2,2,T>", "<4,2,T>", "<8,1>", "<8,2>", "<16,1>", "<16,2>", "<17,1>", "<17,2>"]


@functools.lru_cache(maxsize=None)
def _shape_case(net, form, heb171=False):
    sizes, n_out, _ = SHAPE_NETS[net]
    tuning = ",".join(t for t in (FORMS[form], "heb171=1" if heb171 else None) if t) or None
    out = _run_exact(sizes, n_out, SHAPE_B, SHAPE_T, tuning, seed=len(net))
    seg = _ring_segment(tuning, out["spill_slots"])
    assert seg >= SHAPE_T
    tag = f"shape {net} {form}{' heb171' if heb171 else ''}"
    parsed, worst, teeth, _ = _check_exact(tag, sizes, n_out, SHAPE_B, SHAPE_T, tuning, out, seg)
    names = set()
    for p in parsed.values():
        names |= instantiations(p, heb171)
    return {j: p["text"] for j, p in parsed.items()}, parsed, names


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("net", list(SHAPE_NETS))
def test_flush_plan_of_every_shape_matches_fp64(net, form):
    texts, parsed, _ = _shape_case(net, form)
    for j, want in SHAPE_NETS[net][2].items():
        p = parsed[j]
        if want == "dw":
            assert p["kernel"] == "dw" and p["layout"] == "rm", texts[j]
            continue
        kern = "heb7" if form == "f16" else "heb"
        assert p["text"].split(" ")[0] == "+".join(kern + w for w in want.split("+")), (j, texts[j], want)
        assert p["layout"] == ("tm" if form == "f16" else "rm"), texts[j]


def test_flush_heb171_resplit_matches_fp64():
    """tuning heb171=1: the <17,2> group of a 256 -> 272 Linear runs on <17,1> with twice the activation-tile groups."""
    texts, parsed, _ = _shape_case("128-256-272", "f16", heb171=True)
    assert parsed[2]["text"].split(" ")[0] == "heb7<17,1>x1*2", texts[2]


def test_flush_coverage_names_every_instantiation_on_both_forms():
    seen = set()
    for net in SHAPE_NETS:
        for form in FORMS:
            seen |= _shape_case(net, form)[2]
    seen |= _shape_case("128-256-272", "f16", heb171=True)[2]
    want = {k + i for k in ("heb7", "heb") for i in HEB_INSTANTIATIONS} | {"heb7<17,1>/heb171", "dw"}
    print(f"[flush coverage] {sorted(seen)}")
    assert want <= seen, f"never launched: {sorted(want - seen)}"


# ---- row axis --------------------------------------------------------------------------------------------------------------------
ROW_NET = ([32, 256, 128, 48], 100)         # <2,2,T>, <8,2>, dw, dw
ROW_CASES = {
    # one step of B = 17 (Bpad = 32): a flush of 32 rows, one stage, one split
    "32 rows": (17, 1, None),
    # B = 33 (Bpad = 64: the fourth 16-chain unit is all padding, zeroed once by ensure_spill), 41 steps = 2624 rows: ten K-splits of
    # 288 rows on the tiled kernels, the last one 32 rows
    "short last split, padding unit": (33, 41, None),
    # three ring segments of 8 steps (slot_cap 24, three parts)
    "three segments": (64, 24, "slot_cap=24"),
}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("case", list(ROW_CASES))
def test_flush_row_axis_matches_fp64(case, form):
    B, T, extra = ROW_CASES[case]
    tuning = ",".join(t for t in (FORMS[form], extra) if t) or None
    sizes, n_out = ROW_NET
    out = _run_exact(sizes, n_out, B, T, tuning, seed=T)
    seg = _ring_segment(tuning, out["spill_slots"])
    parsed, worst, teeth, _ = _check_exact(f"rows {case} {form}", sizes, n_out, B, T, tuning, out, seg)
    rows = min(T, seg) * _bpad(B)
    if case == "32 rows":
        assert rows == 32 and all(p["ksplit"] == 1 and p["rps"] == 32 for p in parsed.values()), [p["text"] for p in parsed.values()]
    elif case.startswith("short"):
        tiled = [p for p in parsed.values() if p["kernel"] != "dw"]
        assert tiled and all(p["ksplit"] > 1 and rows % p["rps"] != 0 for p in tiled), [p["text"] for p in tiled]
    else:
        assert seg == 8 and T // seg == 3


# ---- scale history ---------------------------------------------------------------------------------------------------------------
# segment k writes unit group k of every layer at 2^SEG_EXPS[k] (None: the segment is all zero): neighbours differ by 2^+-16
SEG_EXPS = [0, 16, 0, -16, None, 0, 16, -16]
SEG_LEN = 4
HIST_NET = ([128, 256, 256], 272)             # <16,1>, <16,2>, <17,2>
HIST_TUNINGS = {
    "serial": "no_overlap=1,slot_cap=4",
    "2 parts": "ring_parts=2,slot_cap=8",
    "3 parts": "ring_parts=3,slot_cap=12",
    "3 parts, one flush stream": "ring_parts=3,slot_cap=12,flush_streams=1",
    "4 parts": "ring_parts=4,slot_cap=16",
}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("ring", list(HIST_TUNINGS))
def test_flush_scale_history_each_segment_holds_its_own_bound(ring, form):
    tuning = ",".join(t for t in (FORMS[form], HIST_TUNINGS[ring]) if t)
    sizes, n_out = HIST_NET
    B, T = 48, SEG_LEN * len(SEG_EXPS)
    out = _run_exact(sizes, n_out, B, T, tuning, seed=7, seg_len=SEG_LEN, seg_exps=SEG_EXPS)
    seg = _ring_segment(tuning, out["spill_slots"])
    assert seg == SEG_LEN, (out["spill_slots"], seg)
    _check_exact(f"scale history {ring} {form}", sizes, n_out, B, T, tuning, out, seg)


# ---- step-kernel axis: realistic problems ----------------------------------------------------------------------------------------
STEP_NETS = {
    "small": dict(sizes=[30, 64, 64], n_out=100, act="tanh", B=48),
    "cfg-M width": dict(sizes=[30, 256, 256], n_out=784, act="relu", B=256),
    "round schedule": dict(sizes=[30, 256, 256], n_out=784, act="relu", B=6000),
}
STEP_CASES = [("small", None), ("small", "ws=3"), ("small", "ws=2"), ("small", "ws=2,no_lean=1"), ("small", "ws=0"),
              ("cfg-M width", None), ("cfg-M width", "ws=2,no_lean=1"), ("cfg-M width", "ws=0"), ("round schedule", None)]
STEP_WANT = {"ws=3": "mcpc::mcpc_steps_u_kernel<false>", "ws=2": "mcpc::mcpc_steps_ws2_kernel<1, false>",
             "ws=2,no_lean=1": "mcpc::mcpc_steps_ws2_kernel<1, false>", "ws=0": "mcpc::mcpc_steps_kernel<1, 4>"}
STEP_T, STEP_ACC = 12, 4


@functools.lru_cache(maxsize=None)
def _step_case(net, tuning):
    from montecarlopredictivecoding_amd import _lib as L
    from montecarlopredictivecoding_amd.engine import Engine
    cfg = STEP_NETS[net]
    sizes, n_out, B = cfg["sizes"], cfg["n_out"], cfg["B"]
    act = {"tanh": L.ACT_TANH, "relu": L.ACT_RELU}[cfg["act"]]
    g = torch.Generator().manual_seed(B + len(sizes))
    dims = [N_IN] + sizes + [n_out]
    W = [(torch.randn(dims[j + 1], dims[j], generator=g) / math.sqrt(dims[j])).to(DEV) for j in range(len(dims) - 1)]
    b = [(0.1 * torch.randn(dims[j + 1], generator=g)).to(DEV) for j in range(len(dims) - 1)]
    y = (torch.rand(B, n_out, generator=g) < 0.3).float().to(DEV)
    x0 = [torch.randn(B, n, generator=g).to(DEV) for n in sizes]
    eng = Engine(sizes, [act] * len(sizes), N_IN, n_out, B, device=DEV, tuning=tuning)
    try:
        eng.bind_params(W, b)
        eng.bind_inputs(None)
        eng.bind_target(y)
        eng.load_state(x0)
        res = eng.run(STEP_T, loss_kind=L.LOSS_BERNOULLI, lr=0.03, noise_mode=L.NOISE_PHILOX, noise_var=2.0, seed=5, step_base=0,
                      acc_begin=STEP_T - STEP_ACC, acc_end=STEP_T, rec_begin=STEP_T - STEP_ACC, rec_stride=1, rec_count=STEP_ACC, rec_x=True)
        grads = []
        for j in range(len(dims) - 1):
            gW, gb = torch.empty_like(W[j]), torch.empty_like(b[j])
            eng.read_param_grads(j, gW, gb)
            grads.append((gW.double(), gb.double()))
        eng.sync_check()
        step = eng.last_step_kernel()
        plans = [eng.last_flush_plan(j) for j in range(1, len(dims) - 1)]
        assert plans == _planned_text(sizes, n_out, B, tuning, dict(
            T=STEP_T, t_begin=0, n_steps=STEP_T, acc_begin=STEP_T - STEP_ACC, acc_end=STEP_T, update_x=1, xopt_kind=L.XOPT_SGD,
            noise_mode=L.NOISE_PHILOX, loss_kind=L.LOSS_BERNOULLI))
        pref = eng.query()["step_kernel"]
    finally:
        eng.close()
    f = (lambda x: torch.tanh(x)) if cfg["act"] == "tanh" else (lambda x: x.clamp_min(0))
    rec = [r.double() for r in res.rec_x]
    Wd, bd = [w.double() for w in W], [v.double() for v in b]
    fx = [f(x) for x in rec]
    errs = [rec[0] - bd[0]] + [rec[l] - (fx[l - 1] @ Wd[l].T + bd[l]) for l in range(1, len(sizes))]
    eo = torch.sigmoid(fx[-1] @ Wd[-1].T + bd[-1]) - y.double()
    tag = f"step kernel {net} {tuning or 'default'}"
    worst, teeth = 0.0, math.inf
    assert not bool(grads[0][0].any())
    for j in range(len(dims) - 1):
        if j == 0:
            E, A, sign = errs[0], None, -1.0
        elif j < len(sizes):
            E, A, sign = errs[j], fx[j - 1], -1.0
        else:
            E, A, sign = eo, fx[-1], 1.0
        want_b, mag_b = sign * E.sum((0, 1)), E.abs().sum((0, 1))
        if A is None:
            wb = _check_linear(tag, j, grads[j][0], grads[j][1], torch.zeros_like(grads[j][0]), want_b, torch.zeros_like(grads[j][0]),
                               mag_b, 1e-5, 1e-5)[1]
            worst = max(worst, wb)
            continue
        want_W = sign * torch.einsum("tbu,tbi->ui", E, A)
        mag_W = torch.einsum("tbu,tbi->ui", E.abs(), A.abs())
        wW, wb = _check_linear(tag, j, grads[j][0], grads[j][1], want_W, want_b, mag_W, mag_b, 1e-5, 1e-5)
        worst = max(worst, wW, wb)
        teeth = min(teeth, _stage_ratio(E, A, 1e-5 * mag_W, B))
    print(f"[flush {tag}] ran {step!r} (engine preference {pref!r}); plans {plans}; worst error {worst:.3f} of the bound, "
          f"smallest 32-row stage {teeth:.1f} x the tolerance")
    return step, worst, teeth


@pytest.mark.parametrize("net,tuning", STEP_CASES, ids=[f"{n}-{t or 'default'}" for n, t in STEP_CASES])
def test_flush_after_every_step_kernel_matches_fp64(net, tuning):
    step, worst, teeth = _step_case(net, tuning)
    assert worst <= 1.0
    assert teeth > TEETH, teeth
    if tuning in STEP_WANT:
        assert step == STEP_WANT[tuning], step
    if net == "round schedule":
        assert "round schedule" in step, step


def test_step_kernel_coverage_names_every_form_as_run():
    ran = {_step_case(n, t)[0] for n, t in STEP_CASES}
    print(f"[step kernel coverage] {sorted(ran)}")
    for want in ("mcpc::mcpc_steps_u_kernel<false>", "mcpc::mcpc_steps_ws2_kernel<1, false>", "mcpc::mcpc_steps_kernel<1, 4>"):
        assert want in ran, (want, ran)
    assert any("round schedule" in s for s in ran), ran

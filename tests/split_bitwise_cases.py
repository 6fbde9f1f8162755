"""The calls whose results are recorded from the PARENT commit's library and compared bitwise (tests/test_gpu_split_bitwise.py).

Every step-kernel form shares one operand split (csrc/mcpc_gemm_f16.h: split2_pair), so a test of one form against another cannot
see a change in it; these cases are therefore run once on a library built from the commit BEFORE such a change
(scripts/make_split_golden.sh) and their results kept under tests/golden/.  This module only defines the cases and runs them on
whatever library the process has loaded; it is shared by the recording script and the test.

  A   the small net of profiles/step_math_ab.txt: sizes [5, 40, 33], 7 inputs, read-out 21, batch 33 (three chain tiles, the last
      ragged), T = 12, accumulation 4..12 -- on the default form, ws=2 (in-place), ws=0 (barrier) and ws=4 (layer-wise), with ReLU and
      tanh, a Bernoulli read-out with a 0/1 target and a Gaussian one;
  B   cfg-M's widths 30-256-256 -> 784 at batch 48 (three chain tiles), T = 8, accumulation 4..8, 0/1 target: the specialised `hot`
      instantiation, the flush kernels heb7<17, 2>, <16, 2>, <2, 2, true>.  One chain per tile starts from a row whose entries span
      2^-10 .. 2^10 of the others' (more than 2^17 between them: second pieces that are fp16 subnormals).  `B special` also has a
      chain with +Inf and -Inf and a chain with NaN in its initial state (they poison the energies and the gradient, which sum
      over chains: `B` without them keeps those informative);
  C   the same net at batch 4112 (one 16-chain unit more than an MI355X has CUs: the round schedule), whose Hebbian spill goes out
      at system scope: the `hot` and `hot+spill` MIX instantiations.

Recorded per case: the final states, the states and the read-out recorded at one step, all energies, the flat gradient bucket and the
name of the step kernel that ran.  Arrays of at most RAW_BYTES are kept as they are, larger ones as the SHA-256 of their bytes with
every NaN replaced by one bit pattern ("NaNs by position"): equal digests are equal arrays."""
import hashlib

import numpy as np

RELU, TANH = 1, 2
RAW_BYTES = 6144
N_IN_A = 7


def cases():
    out = []
    for tuning in ("", "ws=2", "ws=0", "ws=4"):
        for act in ("relu", "tanh"):
            for loss in ("bernoulli", "gaussian"):
                out.append(dict(name=f"A {tuning or 'default'} {act} {loss}", sizes=[5, 40, 33], n_in=N_IN_A, n_out=21, B=33, T=12, acc=(4, 12),
                                rec_at=6, act=act, loss=loss, tuning=tuning, init="plain", seed=101))
    cfg_m = dict(sizes=[30, 256, 256], n_in=30, n_out=784, T=8, acc=(4, 8), rec_at=6, act="relu", loss="bernoulli", tuning="", seed=202)
    out.append(dict(cfg_m, name="B", B=48, init="wide"))
    out.append(dict(cfg_m, name="B special", B=48, init="special"))
    out.append(dict(cfg_m, name="C", B=4112, init="wide"))
    return out


def make_inputs(case):
    """NumPy inputs of a case: weights, biases, inputs, target, initial states (float32)"""
    rng = np.random.default_rng(case["seed"])
    dims = [case["n_in"]] + case["sizes"] + [case["n_out"]]
    f = np.float32
    W = [(rng.standard_normal((dims[j + 1], dims[j])) / np.sqrt(dims[j])).astype(f) for j in range(len(dims) - 1)]
    b = [(0.1 * rng.standard_normal(dims[j + 1])).astype(f) for j in range(len(dims) - 1)]
    B = case["B"]
    inputs = rng.standard_normal((B, case["n_in"])).astype(f)
    if case["loss"] == "bernoulli":
        target = (rng.random((B, case["n_out"])) < 0.3).astype(f)
    else:
        target = rng.standard_normal((B, case["n_out"])).astype(f)
    x0 = [rng.standard_normal((B, n)).astype(f) for n in case["sizes"]]
    if case["init"] in ("wide", "special"):
        for tile in range(min(3, B // 16)):
            c = 16 * tile + 3
            for x in x0:
                x[c] *= np.exp2(rng.integers(-10, 11, size=x.shape[1])).astype(f)
    if case["init"] == "special":
        x0[0][5, 2], x0[1][5, 100], x0[1][5, 7] = np.inf, -np.inf, np.inf
        x0[1][21, 33] = np.nan
    return W, b, inputs, target, x0


def run_case(case, device):
    """name -> NumPy array of everything a case records, plus the step kernel's name under "kernel" and the flush plans under "flush" """
    import torch
    from montecarlopredictivecoding_amd import _lib as L
    from montecarlopredictivecoding_amd.engine import Engine
    W, b, inputs, target, x0 = make_inputs(case)
    dev = lambda a: torch.from_numpy(a).to(device)
    act = RELU if case["act"] == "relu" else TANH
    eng = Engine(case["sizes"], [act] * len(case["sizes"]), case["n_in"], case["n_out"], case["B"], device=device, tuning=case["tuning"] or None)
    try:
        Wt, bt = [dev(w) for w in W], [dev(x) for x in b]
        eng.bind_params(Wt, bt)
        it, tt = dev(inputs), dev(target)
        eng.bind_inputs(it)
        eng.bind_target(tt)
        eng.load_state([dev(x) for x in x0])
        T = case["T"]
        res = eng.run(T, loss_kind=L.LOSS_BERNOULLI if case["loss"] == "bernoulli" else L.LOSS_GAUSSIAN, loss_var=0.7, lr=0.03,
                      noise_mode=L.NOISE_PHILOX, noise_var=2.0, seed=11, step_base=0, acc_begin=case["acc"][0], acc_end=case["acc"][1],
                      energy_mode=L.ENERGY_ALL, rec_begin=case["rec_at"], rec_stride=1, rec_count=1, rec_x=True, rec_out=True)
        xs = [torch.empty(case["B"], n, device=device) for n in case["sizes"]]
        eng.store_state(xs)
        flat = eng.read_param_grads_flat()
        eng.sync_check()
        out = {f"x{l}": x.cpu().numpy() for l, x in enumerate(xs)}
        out.update({f"rec_x{l}": x.cpu().numpy() for l, x in enumerate(res.rec_x)})
        out["rec_out"] = res.rec_out.cpu().numpy()
        out["energies"] = res.energies.cpu().numpy()
        out["flat"] = flat.cpu().numpy()
        out["kernel"] = eng.last_step_kernel()
        out["flush"] = " | ".join(eng.last_flush_plan(j) for j in range(1, len(case["sizes"]) + 1))       # what the last flush launched, per Linear
        return out
    finally:
        eng.close()


def digest(a):
    a = np.ascontiguousarray(a).copy()
    if a.dtype.kind == "f":
        a[np.isnan(a)] = np.nan          # one bit pattern for every NaN
    return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)


def keeps_raw(name, a):
    return a.nbytes <= RAW_BYTES and not name.startswith("rec_")

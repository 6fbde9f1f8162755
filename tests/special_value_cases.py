"""Shared by tests/test_special_value_cases.py (CPU) and tests/test_gpu_special_values.py: ONE special chain among ordinary ones.

Two small nets (the table below), 40 chains -- two full 16-chain workgroups and one with 8 live chains beside its padding chains; one
partly live 64-row tile of the layer-wise kernels -- and T = 4 steps of the recipe of tests/wide_cases.py (SGD on x with lr 0.05, the
Philox kick with noise_var 2, non-zero inputs).  In every latent layer the x0 of ONE chain is replaced by a special row:

    dead       x = -|x| - 5          f(x) of a ReLU layer is exactly zero: an all-zero row of every forward GEMM (ReLU nets only)
    huge       x 2^40                the row's exponent leaves its neighbours' by 40; below the exponent clamp (|v| < 2^74)
    denormal   x 1e-40               the row's maximum has exponent field 0: the clamped exponent of gemm_row_exp / rowexp_track
    +inf, -inf, nan                  unit 0 of the row: exponent field 255, or a NaN that v_max skips

The statements the GPU tests hold the kernels to: every OTHER chain is bitwise what it is without the special one (the oracle's own
other chains are: test_special_value_cases.py), and a finite special chain follows the fp64 oracle at ITS OWN scale."""
import functools

import numpy as np

from oracle import mcpc_oracle as mo
from oracle.cases import make_case_inputs
from tests import chain_energy_cases as cc
from tests import wide_cases as wc

B, T = 40, 4
ADAM_LR = 0.02
NETS = {
    # every contraction has at most 64 terms (the four-product form); k ranges of 48 and 32, widths that are no multiple of 16
    "short": dict(n_in=5, sizes=[33, 48, 17], n_out=40, seed=311),
    # K = 208 (ragged), 96 and 112: the three-product form
    "long": dict(n_in=5, sizes=[33, 200, 96], n_out=112, seed=312),
}
COMBOS = {"relu_bernoulli": ("relu", "bernoulli"), "tanh_gaussian": ("tanh", "gaussian")}
CHAINS = (21, 16, 39)                    # inside a tile, first of a tile, last live chain (next to the padding)
FINITE = ("dead", "huge", "denormal")
NONFINITE = ("+inf", "-inf", "nan")
_LOSS = {"none": mo.LOSS_NONE, "gaussian": mo.LOSS_GAUSSIAN, "bernoulli": mo.LOSS_BERNOULLI}


def kinds(combo):
    """Finite kinds first, then the non-finite ones; `dead` on ReLU nets only."""
    return tuple(k for k in FINITE + NONFINITE if k != "dead" or COMBOS[combo][0] == "relu")


def case(net, combo, readout=True):
    s = NETS[net]
    act, loss = COMBOS[combo]
    seed = s["seed"] + 10 * sorted(COMBOS).index(combo)
    if not readout:
        return wc._case(f"{net}-{act}-no_readout", s["n_in"], s["sizes"], 0, act, "none", T, seed, inputs_zero=False, B=B)
    return wc._case(f"{net}-{combo}", s["n_in"], s["sizes"], s["n_out"], act, loss, T, seed, inputs_zero=False, B=B)


@functools.lru_cache(maxsize=None)
def data(net, combo, readout=True):
    """(W, b, X0, inputs, target) of the case, read-only: the ordinary chains of every run."""
    out = make_case_inputs(case(net, combo, readout))
    for a in list(out[0]) + list(out[1]) + list(out[2]) + [out[3], out[4]]:
        if a is not None:
            a.setflags(write=False)
    return out


def special_x0(X0, kind, chain):
    """Copies of X0 with the row of `chain` made special in every latent layer (kind None: plain copies)."""
    out = [np.array(x, dtype=np.float32, copy=True) for x in X0]
    for x in out:
        if kind is None:
            continue
        if kind == "dead":
            x[chain] = -np.abs(x[chain]) - np.float32(5.0)
        elif kind == "huge":
            x[chain] = x[chain] * np.float32(2.0 ** 40)
        elif kind == "denormal":
            x[chain] = x[chain] * np.float32(1e-40)
        else:
            x[chain, 0] = {"+inf": np.inf, "-inf": -np.inf, "nan": np.nan}[kind]
    return out


@functools.lru_cache(maxsize=None)
def oracle(net, combo, kind, chain, dtype="float64", readout=True):
    """The learning call (a) on the oracle: accumulation over steps 1..T-1, every state recorded.  Never modified by a test."""
    c = case(net, combo, readout)
    W, b, X0, inputs, target = data(net, combo, readout)
    with np.errstate(all="ignore"):
        return wc.oracle_run(c, np.dtype(dtype).type, acc=range(1, T), record_at=range(T),
                             inputs_data=(W, b, special_x0(X0, kind, chain), inputs, target))


def chain_states(res, chain):
    """[T + 1][L] rows of one chain: the T records and the final state of an oracle run."""
    return [[x[chain] for x in res.rec_xs[t]] for t in range(T)] + [[x[chain] for x in res.xs]]


def chain_scale(net, combo, kind, chain):
    """max |x| of the chain over the fp64 oracle's records and final state."""
    return max(float(np.abs(r).max()) for rows in chain_states(oracle(net, combo, kind, chain), chain) for r in rows)


def state_bound(net, combo, kind, chain):
    """The state contract of BASELINE.md section 3 (1e-5 absolute, stated for x of order 10) at the chain's own scale."""
    return 1e-6 * max(10.0, chain_scale(net, combo, kind, chain))


def chain_rows(net, combo, chain, xs_chain, dtype=np.float64):
    """Per-chain energies of ONE chain for states xs_chain[l] = [n, 1, n_l]: (want, bound) of chain_energy_cases.oracle_rows in fp64;
    with dtype float32 the oracle's own fp32 forward of the same states (the bound is then the fp64 one, unchanged)."""
    c = case(net, combo)
    W, b, _, inputs, target = data(net, combo)
    cd = dict(sizes=tuple(c["sizes"]), act=wc.ACT[c["acts"][0]], loss=_LOSS[c["loss"]], n_out=c["n_out"], var=c["var"], mask_start=0)
    d = dict(W=W, b=b, inputs=inputs[chain:chain + 1], target=target[chain:chain + 1])
    with np.errstate(over="ignore"):                       # exp(-o) of the oracle's sigmoid at a huge chain's logits: 1 / inf = 0
        want, bound = cc.oracle_rows(cd, xs_chain, d=d)
        if np.dtype(dtype) == np.float64:
            return want, bound
        L = len(c["sizes"])
        got = np.zeros_like(want)
        net_ = wc.net_spec(c, W, b)
        for k in range(xs_chain[0].shape[0]):
            fw = mo.forward(net_, d["inputs"], [np.asarray(x[k], np.float32) for x in xs_chain],
                            mo.LossSpec(cd["loss"], d["target"], cd["var"], 0))
            got[k, 0, 0] = fw["loss"]
            got[k, 0, 1:1 + L] = fw["energies"]
            got[k, 0, -1] = got[k, 0, :-1].sum()
    return got, bound

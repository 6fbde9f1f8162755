"""Parity cases for networks too wide for the LDS plans (the layer-wise kernels, csrc/mcpc_steps_lw.h).

The table is shared by tests/test_wide_cases.py (CPU: every case is a parity case -- the oracle's own fp32 rounding stays far inside the
contract) and tests/test_gpu_wide.py / test_gpu_wide_facade.py (the engine against the oracle).  Recipe of every case: parameters uniform
in +-1/sqrt(fan_in) (oracle.cases.make_case_inputs), x0 uniform in +-1, 40 chains, SGD on x with lr 0.05, the Philox kick with noise_var 2."""
import numpy as np

from oracle import mcpc_oracle as mo
from oracle import philox
from oracle.cases import make_case_inputs

ACT = {"identity": 0, "relu": 1, "tanh": 2}
LR, NOISE_VAR, B = 0.05, 2.0, 40


def _case(name, n_in, sizes, n_out, act, loss, T, seed, inputs_zero=True, **kw):
    c = dict(name=name, n_in=n_in, sizes=list(sizes), acts=[act] * len(sizes), ecoef=[1.0] * len(sizes), n_out=n_out, loss=loss, var=1.0,
             B=B, seed=seed, x0_range=1.0, inputs_zero=inputs_zero, T=T)
    c.update(kw)
    return c


# the four shapes mcpc_create rejects without tuning wide=1 / ws=4 ...
REJECTED = ["w1024", "r384", "clf512", "b512"]
CASES = {c["name"]: c for c in [
    _case("w1024", 10, [64, 1024, 1024], 0, "tanh", "none", 20, 101),
    _case("r384", 10, [32, 384], 100, "tanh", "gaussian", 20, 102),
    _case("clf512", 784, [512, 512], 10, "relu", "gaussian", 20, 103, inputs_zero=False),
    _case("b512", 10, [30, 512, 512], 784, "tanh", "bernoulli", 20, 104),
    # ... ReLU at that width: T = 6 (a kink that flips between fp32 and fp64 is not a rounding error; tests/test_gpu_fuzz.py takes T = 5)
    _case("b512relu", 10, [30, 512, 512], 784, "relu", "bernoulli", 6, 105),
    # six latent layers (six of 320 still fit the barrier kernel's LDS plan: 384 do not)
    _case("six384", 10, [384] * 6, 0, "tanh", "none", 20, 106),
    # widths that are no multiples of 16 or 32
    _case("ragged", 10, [50, 700, 333], 1000, "tanh", "gaussian", 20, 107),
    _case("raggedrelu", 10, [50, 700, 333], 1000, "relu", "bernoulli", 6, 108),
    _case("k200", 10, [33, 200, 384], 100, "tanh", "gaussian", 20, 109),
]}


def loss_spec(case, target, mask_start=0):
    kind = {"none": mo.LOSS_NONE, "gaussian": mo.LOSS_GAUSSIAN, "bernoulli": mo.LOSS_BERNOULLI}[case["loss"]]
    return mo.LossSpec(kind, target, var=case["var"], mask_start=mask_start)


def net_spec(case, W, b):
    return mo.NetSpec(sizes=case["sizes"], acts=[ACT[a] for a in case["acts"]], W=W, b=b, ecoef=list(case["ecoef"]), has_head=case["n_out"] > 0)


def philox_noise(case, seed=None, chain_base=0, nb=None, step_base=0):
    seed = case["seed"] if seed is None else seed
    nb = case["B"] if nb is None else nb
    return lambda t, l: philox.layer_normals(seed, step_base + t, l, chain_base, nb, case["sizes"][l])


def oracle_run(case, dtype=np.float32, acc=None, record_at=(), inputs_data=None):
    """The case's learning call on the oracle: SGD + Philox kick, accumulation over `acc` (default: every step)."""
    W, b, X0, inputs, target = inputs_data if inputs_data is not None else make_case_inputs(case)
    T = case["T"]
    acc = list(range(T)) if acc is None else list(acc)
    return mo.run(net_spec(case, W, b), inputs, X0, loss_spec(case, target), mo.XOpt(mo.OPT_SGD, LR), T, noise=philox_noise(case),
                  noise_var=NOISE_VAR, accumulate_p_at=acc, record_at=record_at, dtype=dtype)


def bucket(res):
    """(W0, b0, W1, b1, ...) flat, as the engine's gradient bucket."""
    parts = []
    for g, gb in zip(res.gW, res.gb):
        parts.append(np.asarray(g, dtype=np.float64).reshape(-1))
        if gb is not None:
            parts.append(np.asarray(gb, dtype=np.float64).reshape(-1))
    return np.concatenate(parts)

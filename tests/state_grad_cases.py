"""Shared by the state-gradient tests: the nets, their data, the fp64 oracle of dF/dx one chain at a time and its error bound.

The four nets of tests/chain_energy_cases.py as they are, and three of this file's own.  The bound follows from the project's stated
GEMM bound (tests/test_gpu_accuracy.py: a product sum is off by at most 1e-6 * S, S the sum of the absolute products):
    g_l[u] = e_l[u] -+ f'(x_u) back_u,    e_l = c_l (x_l - mu_l),    back_u = sum_k e_{l+1,k} W_ku
  * mu_l[u] is off by 1e-6 S^mu_l[u], so e_l[u] by 1e-6 c_l S^mu_l[u];
  * back_u is off by 1e-6 sum_k |e_{l+1,k} W_ku| for its own GEMM, and by sum_k kappa 1e-6 S_{l+1}[k] |W_ku| for the error of the
    operand e_{l+1}: kappa = |d e / d mu| is c_{l+1} for a latent layer, 1 / var for a Gaussian read-out and at most 1/4 (the slope of
    the sigmoid) for a Bernoulli one;
  * the epilogue rounds four times (the difference, the scaling, the product, the sum): 4 * 2^-24 (|e_l[u]| + |f'(x_u) back_u|);
  * tanh: f' = 1 - f^2 moves by 2 |f| per unit of f, and tanh_f is off by at most TANH_ABS absolutely:
    2 |f(x_u)| |back_u| TANH_ABS.
Together
    |got - want|_u <= 1e-6 (c_l S^mu_l[u] + |f'(x_u)| (sum_k |e_{l+1,k} W_ku| + sum_k kappa S_{l+1}[k] |W_ku|))
                      + 4 * 2^-24 (|e_l[u]| + |f'(x_u) back_u|)  [+ 2 |f(x_u)| |back_u| TANH_ABS]
Everything on the right is computed here, in fp64."""
import functools

import numpy as np

from oracle import mcpc_oracle as mo
from tests import chain_energy_cases as cc

N_REC = cc.N_REC
U = 2.0 ** -24
# DESIGN.md section 2, the per-element functions: `tanh_f` is off by at most 7 u absolutely (4 u at 0, 7 u towards -1, u towards +1)
TANH_ABS = 7 * U

NETS = dict(cc.NETS)
NETS.update({
    # no read-out, identity: the last layer has no back-projection, the first has one; 40 = 8 mod 32
    "ident_nohead": dict(sizes=(40, 24), n_in=9, n_out=0, act=mo.ACT_IDENTITY, loss=mo.LOSS_NONE, var=1.0, mask_start=0, B=20,
                         inputs=True, target=None, seed=11),
    # the most layers the library takes, every energy coefficient in play
    "six_tanh": dict(sizes=(16, 48, 24, 40, 33, 17), n_in=6, n_out=12, act=mo.ACT_TANH, loss=mo.LOSS_GAUSSIAN, var=0.5, mask_start=0, B=24,
                     inputs=True, target="normal", seed=12, ecoef=(1.0, 0.5, 2.0, 1.0, 0.25, 1.5)),
    # the short back-projection (one k-block) into a wide layer: seven jobs of the backward launch
    "wide_under_small": dict(sizes=(12, 784), n_in=4, n_out=10, act=mo.ACT_TANH, loss=mo.LOSS_GAUSSIAN, var=1.3, mask_start=0, B=16,
                             inputs=False, target="normal", seed=13),
})
OWN = ("ident_nohead", "six_tanh", "wide_under_small")


def ecoef(name):
    c = NETS[name] if isinstance(name, str) else name
    return list(c.get("ecoef", [1.0] * len(c["sizes"])))


@functools.lru_cache(maxsize=None)
def data(name):
    """Weights, biases, inputs, target and N_REC states of order 1, fp32 NumPy; never modified by a test."""
    if name in cc.NETS:
        return cc.data(name)
    c = NETS[name]
    rs = np.random.RandomState(c["seed"])
    dims = [c["n_in"]] + list(c["sizes"]) + ([c["n_out"]] if c["n_out"] else [])
    W = [(rs.randn(dims[j + 1], dims[j]) / np.sqrt(dims[j])).astype(np.float32) for j in range(len(dims) - 1)]
    b = [(0.3 * rs.randn(dims[j + 1])).astype(np.float32) for j in range(len(dims) - 1)]
    B = c["B"]
    inputs = rs.randn(B, c["n_in"]).astype(np.float32) if c["inputs"] else np.zeros((B, c["n_in"]), np.float32)
    target = rs.randn(B, c["n_out"]).astype(np.float32) if c["target"] == "normal" else None
    xs = [rs.randn(N_REC, B, n).astype(np.float32) for n in c["sizes"]]
    for a in W + b + [inputs] + xs + ([target] if target is not None else []):
        a.setflags(write=False)
    return dict(W=W, b=b, inputs=inputs, target=target, xs=xs)


def oracle_rows(name, xs, d=None):
    """oracle.mcpc_oracle.forward + x_grads on float64 copies, ONE CHAIN AT A TIME, for states xs[l] = [n, B, n_l].
    Returns (want, bound): lists over the layers of [n, B, n_l].  ``name``: a net of NETS, or a case of the caller's own (a dict of the
    same keys; ``act``, ``loss`` as the oracle's constants) with its data in ``d``."""
    c = NETS[name] if isinstance(name, str) else name
    d = data(name) if d is None else d
    L = len(c["sizes"])
    ec = ecoef(name)
    f64 = lambda a: None if a is None else np.asarray(a, np.float64)
    W, b = [f64(w) for w in d["W"]], [f64(v) for v in d["b"]]
    has_head = c["n_out"] > 0
    net = mo.NetSpec(sizes=list(c["sizes"]), acts=[c["act"]] * L, W=W, b=b, ecoef=ec, has_head=has_head)
    inputs, target = f64(d["inputs"]), f64(d["target"])
    n, B = xs[0].shape[0], xs[0].shape[1]
    want = [np.zeros((n, B, w)) for w in c["sizes"]]
    bound = [np.zeros((n, B, w)) for w in c["sizes"]]
    absW = [np.abs(w) for w in W]
    kappa_out = {mo.LOSS_GAUSSIAN: 1.0 / c["var"], mo.LOSS_BERNOULLI: 0.25, mo.LOSS_NONE: 0.0}[c["loss"]]
    for k in range(n):
        for ch in range(B):
            loss = mo.LossSpec(c["loss"], None if target is None else target[ch:ch + 1], c["var"], c["mask_start"])
            x = [f64(t[k, ch:ch + 1]) for t in xs]
            fw = mo.forward(net, inputs[ch:ch + 1], x, loss)
            gs = mo.x_grads(net, x, fw)
            S = [np.abs(fw["acts_in"][j]) @ absW[j].T + np.abs(b[j]) for j in range(len(W))]             # [1, n_j] each
            for l in range(L):
                want[l][k, ch] = gs[l][0]
                fx, dfx = mo._act(c["act"], x[l]), mo._dact(c["act"], x[l])
                e = fw["errs"][l]
                if l + 1 < L:
                    e_up, kappa = fw["errs"][l + 1], ec[l + 1]
                elif has_head:
                    e_up, kappa = fw["e_out"], kappa_out
                else:
                    e_up = None
                if e_up is None:
                    back = gemm = operand = np.zeros_like(e)
                else:
                    back = e_up @ W[l + 1]
                    gemm = np.abs(e_up) @ absW[l + 1]
                    operand = (kappa * S[l + 1]) @ absW[l + 1]
                bnd = 1e-6 * (ec[l] * S[l] + np.abs(dfx) * (gemm + operand)) + 4 * U * (np.abs(e) + np.abs(dfx * back))
                if c["act"] == mo.ACT_TANH:
                    bnd = bnd + 2 * np.abs(fx) * np.abs(back) * TANH_ABS
                bound[l][k, ch] = bnd[0]
    return want, bound


@functools.lru_cache(maxsize=None)
def reference(name):
    """The oracle rows of the case's own states, computed once."""
    want, bound = oracle_rows(name, data(name)["xs"])
    for a in want + bound:
        a.setflags(write=False)
    return want, bound


def log_against_bound(parity_log, group, got, want, bound):
    """Per layer |got - want| <= bound, through chain_energy_cases.log_against_bound (the achieved fraction goes to the parity log)."""
    for l in range(len(want)):
        cc.log_against_bound(parity_log, group, np.asarray(got[l], np.float64)[..., None], want[l][..., None], bound[l][..., None],
                             [f"dF/dx_{l + 1}"])

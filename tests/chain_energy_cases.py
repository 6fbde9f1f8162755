"""Shared by the chain-energy tests: the nets, their data, and the per-chain fp64 oracle with its error bound.

The bound follows from the project's stated GEMM bound (tests/test_gpu_accuracy.py: test_gemm_core_accuracy_against_fp64): a
prediction mu_u = sum_k a_k W_uk + b_u is off by at most 1e-6 * S_u, S_u = sum_k |a_k W_uk| + |b_u|.  A layer energy
0.5 c sum_u d_u^2 moves by c |d_u| per unit of mu_u, its own fp32 arithmetic by less than 1e-6 of itself:
    |got - want| <= 1e-6 * (want + sum_u c |d_u| S_u)
and the loss likewise with |dloss / do_u| in place of c |d_u|.  S_u is computed here, in fp64."""
import functools

import numpy as np

from oracle import mcpc_oracle as mo

N_REC = 3

NETS = {
    # two chain tiles of a workgroup and a second, partly live workgroup; K <= 64 (the four-product form)
    "tanh_gauss": dict(sizes=(6, 16, 16), n_in=6, n_out=24, act=mo.ACT_TANH, loss=mo.LOSS_GAUSSIAN, var=0.7, mask_start=0, B=70,
                       inputs=False, target="normal", seed=1),
    # k ranges of 16 mod 32, a mask inside a tile, targets outside {0, 1}
    "relu_bern_mask": dict(sizes=(200, 33, 17), n_in=5, n_out=40, act=mo.ACT_RELU, loss=mo.LOSS_BERNOULLI, var=1.0, mask_start=21, B=70,
                           inputs=True, target="uniform", seed=2),
    # several jobs per layer, K > 64 (the three-product form)
    "relu_bern_wide": dict(sizes=(272, 144), n_in=20, n_out=784, act=mo.ACT_RELU, loss=mo.LOSS_BERNOULLI, var=1.0, mask_start=0, B=16,
                           inputs=True, target="binary", seed=3),
    # one latent layer, no read-out, non-zero inputs: mu_1 only, no GEMM
    "mu1_only": dict(sizes=(37,), n_in=7, n_out=0, act=mo.ACT_TANH, loss=mo.LOSS_NONE, var=1.0, mask_start=0, B=20,
                     inputs=True, target=None, seed=4),
}


@functools.lru_cache(maxsize=None)
def data(name):
    """Weights, biases, inputs, target and N_REC recorded states of order 1, fp32 NumPy; never modified by a test."""
    c = NETS[name]
    rs = np.random.RandomState(c["seed"])
    dims = [c["n_in"]] + list(c["sizes"]) + ([c["n_out"]] if c["n_out"] else [])
    W = [(rs.randn(dims[j + 1], dims[j]) / np.sqrt(dims[j])).astype(np.float32) for j in range(len(dims) - 1)]
    b = [(0.3 * rs.randn(dims[j + 1])).astype(np.float32) for j in range(len(dims) - 1)]
    B = c["B"]
    inputs = rs.randn(B, c["n_in"]).astype(np.float32) if c["inputs"] else np.zeros((B, c["n_in"]), np.float32)
    target = None
    if c["target"] == "normal":
        target = rs.randn(B, c["n_out"]).astype(np.float32)
    elif c["target"] == "uniform":
        target = rs.uniform(-0.5, 1.5, size=(B, c["n_out"])).astype(np.float32)
    elif c["target"] == "binary":
        target = (rs.rand(B, c["n_out"]) < 0.3).astype(np.float32)
    xs = [rs.randn(N_REC, B, n).astype(np.float32) for n in c["sizes"]]
    for a in W + b + [inputs] + xs + ([target] if target is not None else []):
        a.setflags(write=False)
    return dict(W=W, b=b, inputs=inputs, target=target, xs=xs)


def oracle_rows(name, xs, d=None, ecoef=None):
    """oracle.mcpc_oracle.forward on float64 copies, ONE CHAIN AT A TIME, for states xs[l] = [n, B, n_l].  Returns (want, bound), both
    [n, B, L + 2] in the library's column order (loss, E_1..E_L, overall), columns of absent layers left out: L = len(sizes)."""
    c = NETS[name] if isinstance(name, str) else name          # (or a case of the caller's own, with its data in d)
    d = data(name) if d is None else d
    L = len(c["sizes"])
    ecoef = [1.0] * L if ecoef is None else ecoef
    f64 = lambda a: None if a is None else np.asarray(a, np.float64)
    W, b = [f64(w) for w in d["W"]], [f64(v) for v in d["b"]]
    net = mo.NetSpec(sizes=list(c["sizes"]), acts=[c["act"]] * L, W=W, b=b, ecoef=list(ecoef), has_head=c["n_out"] > 0)
    inputs, target = f64(d["inputs"]), f64(d["target"])
    n, B = xs[0].shape[0], xs[0].shape[1]
    want = np.zeros((n, B, L + 2))
    bound = np.zeros((n, B, L + 2))
    absW = [np.abs(w) for w in W]
    for k in range(n):
        for ch in range(B):
            loss = mo.LossSpec(c["loss"], None if target is None else target[ch:ch + 1], c["var"], c["mask_start"])
            fw = mo.forward(net, inputs[ch:ch + 1], [f64(x[k, ch:ch + 1]) for x in xs], loss)
            for l in range(L):
                S = np.abs(fw["acts_in"][l]) @ absW[l].T + np.abs(b[l])                  # [1, n_l]
                want[k, ch, 1 + l] = fw["energies"][l]
                bound[k, ch, 1 + l] = 1e-6 * (fw["energies"][l] + float((np.abs(fw["errs"][l]) * S).sum()))
            if c["loss"] != mo.LOSS_NONE:
                S = np.abs(fw["acts_in"][L]) @ absW[L].T + np.abs(b[L])
                want[k, ch, 0] = fw["loss"]
                bound[k, ch, 0] = 1e-6 * (fw["loss"] + float((np.abs(fw["e_out"]) * S).sum()))
            want[k, ch, -1] = want[k, ch, :-1].sum()
            bound[k, ch, -1] = bound[k, ch, :-1].sum()
    return want, bound


@functools.lru_cache(maxsize=None)
def reference(name):
    """The oracle rows of the case's own recorded states, computed once."""
    want, bound = oracle_rows(name, data(name)["xs"])
    want.setflags(write=False)
    bound.setflags(write=False)
    return want, bound


def columns(table, L):
    """The library's [.., MAX_LATENT + 2] table -> [.., L + 2] (loss, E_1..E_L, overall); the unused columns must be zero."""
    table = np.asarray(table)
    assert (table[..., 1 + L:-1] == 0).all()
    return np.concatenate([table[..., :1 + L], table[..., -1:]], axis=-1)


def log_against_bound(parity_log, group, got, want, bound, names):
    """Assert |got - want| <= bound per column; the achieved fraction of the bound is the `excess` the parity log keeps."""
    for i, q in enumerate(names):
        bnd = np.maximum(bound[..., i], 1e-300)
        frac = float(np.max(np.abs(got[..., i] - want[..., i]) / bnd))
        print(f"{group}: {q}: achieved {frac:.3f} of the bound")
        parity_log.close(group, q + " / bound", got[..., i] / bnd, want[..., i] / bnd, rtol=0.0, atol=1.0)

"""The yardstick of the per-datum marginal likelihood (include/mcpc.h: mcpc_loglik_accumulate): an fp64 numpy reference and the
tolerance a result is held to.  Shared by tests/test_loglik_host.py and tests/test_gpu_loglik.py; no device, no torch.

The tolerance is computed from the inputs, not tuned.  With gamma = (width + 16) * 2^-53 -- a sum of `width` exact products in any
order, plus the roundings of forming the nll from it --
  Bernoulli  delta(i, s) = gamma * (sum_j |y_ij c_sj| + b_s)
  Gaussian   delta(i, s) = gamma * (0.5 / var) * (a_i + b_s + 2 sum_j |y_ij c_sj|)
bounds the error of one nll.  Log-mean-exp is 1-Lipschitz in the sup norm of the nll, so
  tol_logp(i) = 4 * max_s delta(i, s) + (n_samp + 64) * 2^-52:
the factor 4 covers the device's exp / log1p / log at 2 ulp or less and the roundings of the merges, the second term the summation
of n_samp positive terms.  The effective sample size s1^2 / s2 is held to the same figure, relative.
"""
import numpy as np

LOSSES = ("bernoulli", "gaussian")


def _clamped(o, clamp):
    o = np.asarray(o, dtype=np.float64)
    return o if np.isinf(clamp) else np.clip(o, -clamp, clamp)            # np.clip keeps a NaN


def softplus(c):
    return np.maximum(c, 0.0) + np.log1p(np.exp(-np.abs(c)))


def nll_matrix(y, o, loss, var=None, clamp=20.0):
    """fp64 ``[n_data, n_samp]``: the negative log-likelihood of every datum under every sample's read-out."""
    y = np.asarray(y, dtype=np.float64)
    c = _clamped(o, clamp)
    with np.errstate(all="ignore"):
        if loss == "bernoulli":
            return softplus(c).sum(1)[None, :] - y @ c.T
        if loss == "gaussian":
            a, b = (y * y).sum(1), (c * c).sum(1)
            return (0.5 / var) * (a[:, None] + b[None, :] - 2.0 * (y @ c.T)) + 0.5 * y.shape[1] * np.log(2.0 * np.pi * var)
    raise ValueError(loss)


def state_from_nll(nll):
    """``[n_data, 4]``: (m, s1, s2, cnt) over the finite entries of every row; a row without one is the empty state (+inf, 0, 0, 0)."""
    nll = np.asarray(nll, dtype=np.float64)
    ok = np.isfinite(nll)
    cnt = ok.sum(1).astype(np.float64)
    m = np.where(ok, nll, np.inf).min(1) if nll.shape[1] else np.full(nll.shape[0], np.inf)
    base = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(all="ignore"):
        e = np.where(ok, np.exp(-(np.where(ok, nll, 0.0) - base[:, None])), 0.0)
    return np.stack([m, e.sum(1), (e * e).sum(1), cnt], axis=1)


def ref_state(y, o, loss, var=None, clamp=20.0):
    return state_from_nll(nll_matrix(y, o, loss, var, clamp))


def log_p(state):
    state = np.asarray(state, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(state[:, 3] > 0, np.log(state[:, 1] / state[:, 3]) - state[:, 0], np.nan)


def ess(state):
    state = np.asarray(state, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(state[:, 3] > 0, state[:, 1] ** 2 / state[:, 2], np.nan)


def merge(a, b):
    """The merge rule of include/mcpc.h in numpy."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.empty_like(a)
    for i in range(a.shape[0]):
        m = min(a[i, 0], b[i, 0])
        if m == np.inf:
            out[i] = (np.inf, 0.0, 0.0, 0.0)
            continue
        fa = np.exp(m - a[i, 0]) if a[i, 0] < np.inf else 0.0
        fb = np.exp(m - b[i, 0]) if b[i, 0] < np.inf else 0.0
        out[i] = (m, a[i, 1] * fa + b[i, 1] * fb, a[i, 2] * fa * fa + b[i, 2] * fb * fb, a[i, 3] + b[i, 3])
    return out


def delta(y, o, loss, var=None, clamp=20.0):
    """``[n_data, n_samp]``: the bound on the error of one nll (module docstring); non-finite entries (pairs that are not taken) are 0."""
    y = np.asarray(y, dtype=np.float64)
    c = _clamped(o, clamp)
    gamma = (y.shape[1] + 16) * 2.0 ** -53
    with np.errstate(all="ignore"):
        dot = np.abs(y) @ np.abs(c).T
        if loss == "bernoulli":
            d = gamma * (dot + softplus(c).sum(1)[None, :])
        else:
            d = gamma * (0.5 / var) * ((y * y).sum(1)[:, None] + (c * c).sum(1)[None, :] + 2.0 * dot)
    return np.where(np.isfinite(d), d, 0.0)


def tol(y, o, loss, var=None, clamp=20.0):
    """``[n_data]``: the absolute tolerance of log_p and the relative tolerance of the ESS."""
    d = delta(y, o, loss, var, clamp)
    n_samp = d.shape[1]
    worst = d.max(1) if n_samp else np.zeros(d.shape[0])
    return 4.0 * worst + (n_samp + 64) * 2.0 ** -52


def assert_state_close(got, want, tolerance, what=""):
    """cnt exactly; log_p within ``tolerance``, the ESS within ``tolerance`` relative; NaN (cnt = 0) where the reference has it."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    np.testing.assert_array_equal(got[:, 3], want[:, 3], err_msg=f"{what}: cnt")
    lp_g, lp_w, es_g, es_w = log_p(got), log_p(want), ess(got), ess(want)
    none = want[:, 3] == 0
    assert np.isnan(lp_g[none]).all() and np.isnan(es_g[none]).all(), what
    assert (got[none, 0] == np.inf).all() and (got[none, 1:3] == 0).all(), f"{what}: a datum without samples is the empty state"
    some = ~none
    err_lp = np.abs(lp_g[some] - lp_w[some])
    err_es = np.abs(es_g[some] - es_w[some]) / es_w[some]
    t = np.broadcast_to(tolerance, none.shape)[some]
    if some.any():
        print("%s: max |log_p err| %.3g, max rel ESS err %.3g, smallest tolerance %.3g" % (what, err_lp.max(), err_es.max(), t.min()))
    assert (err_lp <= t).all(), (what, "log_p", float(err_lp.max()), float(t.min()))
    assert (err_es <= t).all(), (what, "ess", float(err_es.max()), float(t.min()))


def make_case(n_data, n_samp, width, loss, seed=0):
    """Seeded fp32 inputs of the kind the evaluator sees: binary data and logits of a few units for Bernoulli, real data and means for
    Gaussian.  Returns (y, o, var)."""
    rng = np.random.default_rng([seed, n_data, n_samp, width, LOSSES.index(loss)])
    if loss == "bernoulli":
        y = (rng.random((n_data, width)) < 0.3).astype(np.float32)
        o = (3.0 * rng.standard_normal((n_samp, width))).astype(np.float32)
        return y, o, None
    y = rng.standard_normal((n_data, width)).astype(np.float32)
    o = (y[rng.integers(0, n_data, n_samp)] + 0.7 * rng.standard_normal((n_samp, width))).astype(np.float32) if n_data else \
        rng.standard_normal((n_samp, width)).astype(np.float32)
    return y, o, 0.3

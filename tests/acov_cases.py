"""The definition the autocovariance tests compare against: the sequential fp64 host loop over fp32 samples, and the direct centred
estimator in numpy."""
import numpy as np


def ref_stream(g, K, stops=None):
    """g: fp32 ``[n, E]`` (already transformed), the samples of a stream in order.  The loop ``acc[k] += (double)g_j * (double)g_{j-k}``
    for every j and every k <= min(j, K), and ``sum += (double)g_j``.  Returns ``{m: (lagged [E, K + 1] fp64, sum [E] fp64, head
    [min(K, m), E] fp32, window [min(K, m), E] fp32)}`` for every m in ``stops`` (default: n alone): the state after m samples; row k of
    window is the sample k + 1 places back from sample m."""
    g = np.ascontiguousarray(g, dtype=np.float32)
    n, E = g.shape
    stops = {n} if stops is None else set(stops)
    gd = g.astype(np.float64)
    lag, s = np.zeros((E, K + 1)), np.zeros(E)
    out = {}

    def snap(m):
        v = min(K, m)
        out[m] = (lag.copy(), s.copy(), g[:v].copy(), g[m - v:m][::-1].copy())
    if 0 in stops:
        snap(0)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(n):
            s = s + gd[j]
            for k in range(min(j, K) + 1):
                lag[:, k] = lag[:, k] + gd[j] * gd[j - k]              # the product of two fp32 values is exact in fp64
            if j + 1 in stops:
                snap(j + 1)
    return out


def direct_acov(g, K):
    """The biased estimator centred on the mean, straight from the samples in fp64: ``[E, K + 1]``, 0 for k >= n."""
    x = np.asarray(g, dtype=np.float64)
    n = x.shape[0]
    d = x - x.mean(axis=0)
    c = np.zeros((x.shape[1], K + 1))
    for k in range(min(K, n - 1) + 1):
        c[:, k] = (d[k:] * d[:n - k]).sum(axis=0) / n
    return c


def ar1(phi, n, mean, seed, scale=1.0):
    """An AR(1) series in fp32: x_j = mean + z_j, z_j = phi z_{j-1} + e_j."""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal(n) * scale
    z = np.zeros(n)
    z[0] = e[0] / np.sqrt(max(1 - phi * phi, 1e-12))
    for j in range(1, n):
        z[j] = phi * z[j - 1] + e[j]
    return (mean + z).astype(np.float32)

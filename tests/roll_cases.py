"""The definition the rolling-variance tests compare against: the sequential fp64 host loop over fp32 samples (the bitwise reference), a
direct two-pass variance of every window, and series to feed them."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view


def ref_roll(g, W, every=1):
    """g: fp32 ``[n, E]`` (already transformed), the samples of a stream in order.  The loop of csrc/mcpc_roll.h, vectorised over the
    elements only: s1 += g_j, s2 += g_j^2, the sample j - W leaves, and every full window with (j - (W - 1)) % every == 0 emits
    m = s1 / W, v = (s2 - s1 * m) / (W - 1), negative -> 0 (NaN stays).  Returns ``(v [rows, E] fp64, s1 [E], s2 [E], samples)``:
    ``samples[r]`` is the stream index of row r's newest sample."""
    g = np.ascontiguousarray(g, dtype=np.float32)
    n, E = g.shape
    gd = g.astype(np.float64)
    s1, s2 = np.zeros(E), np.zeros(E)
    rows, samples = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(n):
            s1 = s1 + gd[j]
            s2 = s2 + gd[j] * gd[j]                                    # the product of two fp32 values is exact in fp64
            if j >= W:
                s1 = s1 - gd[j - W]
                s2 = s2 - gd[j - W] * gd[j - W]
            if j >= W - 1 and (j - (W - 1)) % every == 0:
                m = s1 / W
                v = (s2 - s1 * m) / (W - 1)
                rows.append(np.where(v < 0, 0.0, v))
                samples.append(j)
    return (np.stack(rows) if rows else np.zeros((0, E))), s1, s2, samples


def two_pass(g, W, every=1):
    """``var(ddof=1)`` of every window of W samples, straight from the samples in fp64: ``[rows, E]``."""
    x = np.asarray(g, dtype=np.float64)
    if x.shape[0] < W:
        return np.zeros((0, x.shape[1]))
    return sliding_window_view(x, W, axis=0).var(axis=-1, ddof=1)[::every]


def pooled(v):
    """v ``[rows, E]`` -> ``[rows, 4]``: over the finite elements of a row the fp64 sums of sqrt(v), of its square, of v, and their count."""
    ok = np.isfinite(v)
    with np.errstate(invalid="ignore"):
        sd = np.sqrt(np.where(ok, v, 0.0))
    return np.stack([np.where(ok, sd, 0.0).sum(1), np.where(ok, sd * sd, 0.0).sum(1), np.where(ok, v, 0.0).sum(1), ok.sum(1).astype(np.float64)],
                    axis=1)


def noise(n, E, seed, mean=0.7, scale=1.5):
    """White fp32 samples ``[n, E]``."""
    return (np.random.default_rng(seed).standard_normal((n, E)) * scale + mean).astype(np.float32)


def onset(n, E, seed, at, mean=0.5):
    """fp32 ``[n, E]`` whose spread drops at sample ``at`` (a stimulus onset quenches the variability) and whose mean jumps there."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, E))
    x[:at] *= 2.0
    x[at:] = x[at:] * 0.5 + 3.0
    return (x + mean).astype(np.float32)

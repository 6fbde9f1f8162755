"""The numpy definition of the posterior histograms (helper of the histogram tests, no test of its own)."""
import numpy as np


def ref_hist(values32, edges32):
    """values32: fp32 [n, ...]; edges32: fp32 [nb + 1], strictly ascending.  Returns (bins [..., nb], under [...], over [...], nan [...])
    in int64, counted over axis 0: bin i holds edges[i] <= v < edges[i + 1], the last bin is closed at edges[nb], under is v < edges[0]
    (-inf included), over is v > edges[nb] (+inf included).  Comparisons are exact (fp32 values in fp64)."""
    v = np.asarray(values32, dtype=np.float32).astype(np.float64)
    e = np.asarray(edges32, dtype=np.float32).astype(np.float64)
    nb = e.size - 1
    isnan = np.isnan(v)
    idx = np.searchsorted(e, v, side="right") - 1           # -1: under; nb: at or above the last edge; NaN sorts last (nb)
    idx = np.where(v == e[nb], nb - 1, idx)                  # the last bin is closed
    under = (~isnan) & (v < e[0])
    over = (~isnan) & (v > e[nb])
    inside = ~(isnan | under | over)
    bins = np.zeros(v.shape[1:] + (nb,), dtype=np.int64)
    for i in range(nb):
        bins[..., i] = (inside & (idx == i)).sum(axis=0)
    return bins, under.sum(axis=0).astype(np.int64), over.sum(axis=0).astype(np.int64), isnan.sum(axis=0).astype(np.int64)


def table(values32, edges32):
    """ref_hist as the kernel's table [..., nb + 3]: bins, under, over, nan."""
    b, u, o, n = ref_hist(values32, edges32)
    return np.concatenate([b, u[..., None], o[..., None], n[..., None]], axis=-1)

"""The numpy definition of the joint histograms (helper of the hist2d tests, no test of its own), and the inputs they share."""
import numpy as np


def classes(values32, edges32):
    """fp32 values -> the class of each against fp32 edges [nb + 1]: 0..nb-1 the bins (half-open, the last one closed), nb under
    (-inf included), nb + 1 over (+inf included), nb + 2 NaN.  Comparisons are exact (fp32 values in fp64), -0.0 == +0.0, denormals
    are compared as they are."""
    v = np.asarray(values32, dtype=np.float32).astype(np.float64)
    e = np.asarray(edges32, dtype=np.float32).astype(np.float64)
    nb = e.size - 1
    idx = np.searchsorted(e, v, side="right") - 1
    idx = np.where(v == e[nb], nb - 1, idx)
    idx = np.where(v < e[0], nb, idx)
    idx = np.where(v > e[nb], nb + 1, idx)
    return np.where(np.isnan(v), nb + 2, idx).astype(np.int64)


def ref_hist2d(x, y, edges_x, edges_y):
    """x, y: fp32 [n, ...] of one shape -> int64 [..., nx + 3, ny + 3], counted over axis 0: cell (class of x, class of y)."""
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    assert x.shape == y.shape
    ncx, ncy = len(edges_x) + 2, len(edges_y) + 2
    cells = ncx * ncy
    flat = (classes(x, edges_x) * ncy + classes(y, edges_y)).reshape(x.shape[0], -1)
    m = flat.shape[1]
    out = np.bincount((flat + np.arange(m, dtype=np.int64) * cells).ravel(), minlength=m * cells)
    return out.reshape(x.shape[1:] + (ncx, ncy)).astype(np.int64)


def ref_pairs(rx, ry, pairs, edges_x, edges_y, pool=False):
    """rx fp32 [n, B, wx], ry fp32 [n, B, wy], pairs [(px, py), ...] -> what the kernel's `counts` hold: [B, pairs, nx + 3, ny + 3],
    or summed over the chains with `pool`."""
    px, py = [p for p, _ in pairs], [q for _, q in pairs]
    out = ref_hist2d(rx[:, :, px], ry[:, :, py], edges_x, edges_y)
    return out.sum(0) if pool else out


def sigmoid32(v):
    """A host stand-in for the library's sigmoid that the tests use only AWAY from the edges (see where it is called)."""
    return (1.0 / (1.0 + np.exp(-v.astype(np.float64)))).astype(np.float32)


EDGES_SPECIAL = np.array([-2.0, -1.0, 0.0, 1e-40, 1.0, 2.0], dtype=np.float32)    # an edge at 0.0 and a denormal edge

# values on every edge, +-0.0, denormals on both sides of them, +-inf, NaN
SPECIAL = np.array([-2.0, -1.0, 0.0, -0.0, 1e-40, 1.0, 2.0, -1e-42, 1e-42, 2e-40, np.nextafter(np.float32(2.0), np.float32(3.0)),
                    np.nextafter(np.float32(-2.0), np.float32(-3.0)), np.inf, -np.inf, np.nan, 0.5, -1.5], dtype=np.float32)
# the class of each by hand against EDGES_SPECIAL (5 bins: under = 5, over = 6, nan = 7): -2 opens bin 0; -1 bin 1; +-0.0 bin 2 (the
# edge 0.0 opens it, and -0.0 == 0.0); 1e-40 opens bin 3; 1 opens bin 4; 2 closes the last bin; -1e-42 is below 0.0: bin 1; 1e-42 lies
# in [0, 1e-40): bin 2; 2e-40 in [1e-40, 1): bin 3; just above 2: over; just below -2: under; +inf over; -inf under; NaN nan; 0.5 bin 3;
# -1.5 bin 0
SPECIAL_CLASS = np.array([0, 1, 2, 2, 3, 4, 4, 1, 2, 3, 6, 5, 6, 5, 7, 3, 0], dtype=np.int64)


def special_pairs():
    """(x, y) fp32 [n]: every special value against every special value -- NaN in x only, in y only and in both are among them."""
    n = SPECIAL.size
    return np.repeat(SPECIAL, n), np.tile(SPECIAL, n)

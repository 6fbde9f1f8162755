"""The numpy reference of the nearest-neighbour search (include/mcpc.h: mcpc_knn_accumulate) and the error bound its tests hold the kernel to.

`kbest` is brute force in fp64 on the same fp32 rows: every squared distance D(i, j) = sum_c (q[i][c] - ref[j][c])^2 exactly as fp64 gives
it (the difference of two fp32 values is exact in fp64 unless their exponents are more than 29 apart, and then the error is below
2^-53 relative to the larger; the squares and the sum round in fp64, d * 2^-53), a NaN distance replaced by +inf, the k smallest per row
ascending, +inf where there are fewer than k.

The bound, with u = 2^-24 (half an fp32 ulp at 1), derived from the arithmetic the header defines, not from what the kernel gives.  The
kernel computes t_c = fl(q_c - r_c) = (q_c - r_c)(1 + e_c), |e_c| <= u, and a_c = fl(t_c^2 + a_(c-1)) by fmaf, one rounding each.  Every
term is non-negative, so no cancellation: t_c^2 = (q_c - r_c)^2 (1 + e_c)^2 is within (2 u + u^2) relative of its exact term, and each of
the d fmaf roundings multiplies the running sum by (1 + f_c), |f_c| <= u (the first one, onto a = 0, included).  A term passes at
most d such roundings, so D_fp32 = sum_c (q_c - r_c)^2 (1 + g_c) with |g_c| <= (1 + u)^(d + 2) - 1 <= (d + 3) u for d <= 32 (the
second-order part, at most (d + 2)^2 u^2 / 2 < 1e-12, is what the 3 in place of 2 pays for many times over).  Hence
|D_fp32 - D| <= (d + 3) u D: the issue's relative (d + 3) * 2^-24.  This holds while no t_c^2 or partial sum is subnormal; the tests scale
their data so that no squared distance is.  The k-th smallest of values each moved by at most a relative eps is itself moved by at
most eps (an order statistic is monotone in every argument: raise every value by the factor 1 + eps and the k-th smallest rises by
exactly that factor, lower them and it falls by it, and the perturbed values lie in between), so the bound carries over from D to
best[i][s] slot by slot, ties and all.  min and max round nothing: no further term.

For the estimator: KL = -(d / n) sum_i (log r2_i - log s2_i) / 2 + const, and a relative eps on r2_i and on s2_i moves each logarithm by
eps (1 + eps): the sum of n terms of two half-logarithms by n eps, the estimate by d eps = d (d + 3) u; the tests allow twice that,
d (d + 3) 2^-23, which also covers the fp64 evaluation.  The reference queries its trees with eps=.01: each of its distances lies in
[true, 1.01 true], so each log(r / s) is off by at most log 1.01 and its estimate by at most d log 1.01.
"""
import math

import numpy as np

U = 2.0 ** -24


def dist_bound(d):
    """Relative error of one fp32 squared distance in d coordinates, and of every entry of best."""
    return (d + 3) * U


def kl_tolerance(d):
    """|kl_divergence on the device - the reference's KLdivergence| on the same fp32 clouds."""
    return d * math.log(1.01) + (d + 3) * 2.0 ** -23 * d


def sqdist(q, ref):
    """fp64 [nq, nr] squared distances of fp32 rows; a NaN stays a NaN."""
    q, ref = np.asarray(q, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.zeros((q.shape[0], ref.shape[0]))
        for c in range(q.shape[1]):
            t = q[:, c][:, None] - ref[:, c][None, :]
            out += t * t
    return out


def kbest(q, ref, k, old=None):
    """fp64 [nq, k]: the k smallest squared distances of every row of q into ref (and the values of `old` [nq, k], if given), ascending;
    a NaN never counts, +inf fills up."""
    D = sqdist(q, ref)
    if old is not None:
        D = np.concatenate([D, np.asarray(old, dtype=np.float64)], axis=1)
    D = np.where(np.isnan(D), np.inf, D)
    D = np.concatenate([D, np.full((D.shape[0], k), np.inf)], axis=1)
    return np.sort(D, axis=1)[:, :k]


def kl_from_sqdist(r2, s2, n, m, d):
    """The Perez-Cruz estimate in numpy fp64 from squared distances, written as the reference writes it: with r = sqrt(r2), s = sqrt(s2)."""
    r, s = np.sqrt(np.asarray(r2, dtype=np.float64)), np.sqrt(np.asarray(s2, dtype=np.float64))
    return -np.log(r / s).sum() * d / n + np.log(m / (n - 1.0))


def kl_exact(x, y):
    """The estimate from exact fp64 brute-force distances of fp32 clouds x [n, d], y [m, d]."""
    r2 = kbest(x, x, 2)[:, 1]
    s2 = kbest(x, y, 1)[:, 0]
    return kl_from_sqdist(r2, s2, x.shape[0], y.shape[0], x.shape[1])

"""The Box-Muller transform of csrc/mcpc_device.h (`box_muller`) in float64, from the same integer fields, and the bounds the device's
fp32 form is held to (tests/test_gpu_box_muller.py, tests/test_box_muller_host.py).  Plain NumPy, no GPU.

The transform.  From two 32-bit words a, b, with the low 8 bits of each shifted out:

    u1 = ((a >> 8) + 1) 2^-24   in (0, 1]        r  = sqrt(-2 ln u1)
    u2 = (b >> 8) 2^-24         in [0, 1)        z0 = r cos(2 pi u2),  z1 = r sin(2 pi u2)

It is separable -- the radius depends on a alone, the angle on b alone -- and each factor has 2^24 arguments, so both can be swept
exhaustively and the moments of z over the full 2^24 x 2^24 grid are products of means over the two tables (`grid_moments`).

THE RADIUS BOUND.  The device computes r = v_sqrt_f32(c * v_log_f32(u1)) with c = fp32(-2 ln 2) = -1.3862943611198906f.  With
eps = 2^-24 (half an ulp, relative) and 2 eps = 2^-23 (one ulp, relative):
  * u1 is exact: (a >> 8) + 1 <= 2^24 converts to fp32 without rounding and the scaling by 2^-24 is exact.
  * v_log_f32 is within 1 ulp (the project's figure):       log2_dev = log2(u1) (1 + d1),   |d1| <= 2 eps
  * the constant is the nearest fp32 to -2 ln 2:                                 c = -2 ln 2 (1 + dc),           |dc| <= eps
    (its actual error, `C_REL_ERR`, is 1.2e-8 = 0.2 eps; the derivation keeps eps)
  * the product rounds once:                                                     p = c log2_dev (1 + d2),        |d2| <= eps
  * v_sqrt_f32 is within 1 ulp (the comment in box_muller):                      r_dev = sqrt(p) (1 + d3),       |d3| <= 2 eps
so r_dev = sqrt(-2 ln u1) sqrt((1 + d1)(1 + dc)(1 + d2)) (1 + d3).  The square root halves what comes before it:

    |r_dev / r - 1|  <=  (2 eps + eps + eps) / 2 + 2 eps + O(eps^2)  =  4 eps  =  2 x 2^-23  =  2^-22  =  2.4e-7

`RADIUS_RTOL` is that figure with the second-order terms (at most 8 eps^2 < 2^-44 in all) covered by a factor 1 + 2^-20.  No result
on the way is subnormal: the smallest non-zero |log2 u1| is 8.6e-8 (u1 = 1 - 2^-24).  At u1 = 1 the logarithm must be a zero, of
either sign (c * +0 = -0 and v_sqrt_f32(-0) = -0): a logarithm that is positive there by any amount gives a NaN radius.

The largest radius is at u1 = 2^-24: sqrt(48 ln 2) = 5.76811 (`R_MAX`); the tail of the device's normals ends there.

THE ANGLE FUNCTIONS.  v_cos_f32 and v_sin_f32 take the angle in turns (u2 itself, exact).  The project states no accuracy figure for them
and none is derived here: a normal is held to the project's existing tolerance of 2e-5 absolute against its twin (`Z_ATOL`,
tests/test_gpu_engine.py), exhaustively over the angles, and the worst errors of the two functions are measured and recorded
(profiles/box_muller_accuracy.txt).

THE MOMENT CAPS (`CAPS`).  Conditions on the exact moments of the device's distribution over the whole grid, far below what any sampled
statistic of the suite resolves (the golden sampling statistics resolve a variance to sqrt(2 / 6e6) = 6e-4):
    |E z| <= 1e-6,   |E z^2 - 1| <= 1e-5,   |E z0 z1| <= 1e-5,   |E z^4 - 3| <= 1e-4
The ideal transform on the same grids sits well inside them (`IDEAL`; the radius grid is a right-endpoint sum over a logarithmic
singularity: E r^2 = 2 - ln(2 pi 2^24) / 2^24 + ... by Stirling's formula), so a failure on the device is the device's.
"""
import numpy as np

N = 1 << 24                                        # radii, and angles
EPS = 2.0 ** -24
C_F32 = float(np.float32(-1.3862943611198906))     # the device's constant
C_REL_ERR = abs(C_F32 / (-2.0 * np.log(2.0)) - 1.0)
RADIUS_RTOL = ((2 * EPS + EPS + EPS) / 2 + 2 * EPS) * (1.0 + 2.0 ** -20)
R_MAX = float(np.sqrt(48.0 * np.log(2.0)))         # u1 = 2^-24
Z_ATOL = 2e-5
CAPS = {"mean": 1e-6, "var": 1e-5, "cross": 1e-5, "fourth": 1e-4}
# the ideal fp64 transform on the 2^24 x 2^24 grid (tests/test_box_muller_host.py pins them to 1e-8)
IDEAL = {"E r^2": 1.99999890, "E r^4": 7.99995924, "E cos^2": 0.5, "E cos^4": 0.375}


def u1_of(a):
    """(0, 1]: ((a >> 8) + 1) 2^-24 in float64 (exact)."""
    return ((np.asarray(a, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24


def u2_of(b):
    """[0, 1): (b >> 8) 2^-24 in float64 (exact), the fraction of a turn."""
    return (np.asarray(b, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def radius(a):
    """sqrt(-2 ln u1) in float64.  log1p of the exact difference u1 - 1 keeps full relative accuracy next to u1 = 1."""
    u1 = u1_of(a)
    return np.sqrt(-2.0 * np.where(u1 > 0.5, np.log1p(u1 - 1.0), np.log(u1)))


def angle(b):
    """(cos, sin) of 2 pi u2 in float64."""
    t = 2.0 * np.pi * u2_of(b)
    return np.cos(t), np.sin(t)


def box_muller(a, b):
    """(z0, z1) in float64."""
    r = radius(a)
    c, s = angle(b)
    return r * c, r * s


def all_fields():
    """k << 8 for every k in [0, 2^24): every radius when passed as a, every angle when passed as b."""
    return np.arange(N, dtype=np.uint32) << np.uint32(8)


def grid_moments(R, C, S):
    """The moments of z0 = R(i) C(j), z1 = R(i) S(j) over the full product grid of a radius table and an angle table (float64), as
    products of table means."""
    R, C, S = (np.asarray(x, dtype=np.float64) for x in (R, C, S))
    R2, C2, S2 = R * R, C * C, S * S
    ER, ER2, ER4 = R.mean(), R2.mean(), (R2 * R2).mean()
    return {"E z0": ER * C.mean(), "E z1": ER * S.mean(),
            "E z0^2": ER2 * C2.mean(), "E z1^2": ER2 * S2.mean(),
            "E z0 z1": ER2 * (C * S).mean(),
            "E z0^4": ER4 * (C2 * C2).mean(), "E z1^4": ER4 * (S2 * S2).mean(),
            "E r^2": ER2, "E r^4": ER4, "E cos": C.mean(), "E sin": S.mean(), "E cos sin": (C * S).mean(),
            "E cos^2": C2.mean(), "E sin^2": S2.mean(), "E cos^4": (C2 * C2).mean(), "E sin^4": (S2 * S2).mean()}


def cap_violations(m):
    """The moments of `grid_moments` that lie outside `CAPS`, as {name: (value, target, cap)}; empty when all hold."""
    checks = [("E z0", 0.0, "mean"), ("E z1", 0.0, "mean"), ("E z0^2", 1.0, "var"), ("E z1^2", 1.0, "var"), ("E z0 z1", 0.0, "cross"),
              ("E z0^4", 3.0, "fourth"), ("E z1^4", 3.0, "fourth")]
    return {k: (m[k], want, CAPS[cap]) for k, want, cap in checks if not abs(m[k] - want) <= CAPS[cap]}


_IDEAL = {}


def ideal_tables():
    """(R, C, S) of the ideal transform over all 2^24 fields, float64; computed once, shared, read-only."""
    if not _IDEAL:
        f = all_fields()
        R = radius(f)
        C, S = angle(f)
        for x in (R, C, S):
            x.setflags(write=False)
        _IDEAL["t"] = (R, C, S)
    return _IDEAL["t"]

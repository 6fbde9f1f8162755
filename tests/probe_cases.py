"""The numpy reference of the linear probe (include/mcpc.h: mcpc_probe_accumulate) and the error bounds its tests hold the kernel to.

Logits by the sequential fp64 loop over k (vectorised over everything else) rounded to fp32: what the kernel computes bitwise.  Votes by
np.argmax with the NaN column.  Identity sums by a sequential fp64 loop over the samples.  Softmax and entropy in fp64 from those fp32
logits: what the kernel's fp32 link is bounded against.

The bounds, with u = 2^-24 (half an fp32 ulp at 1), derived from the arithmetic the header defines, not from what the kernel gives:

softmax, per sample and class (the issue's derivation): d = v - m rounds with relative error u, which moves e = exp(d) by at most
u |d| e^-|d| <= u / e absolutely; expf is within 4 * 2^-23 = 8 u relative; the C - 1 additions of S (a tree is no worse than a chain)
and the division give C u + 2 u relative; p <= 1.  Hence |p - p_ref| <= (C + 16) u, |psum - ref| <= n (C + 16) u and, p + p_ref <= 2,
|psumsq - ref| <= 2 n (C + 16) u.

entropy, per sample: H = log S - sum_i p_i d_i, d_i = v_i - m <= 0, so H = log S + sum_i p_i |d_i|, and with 1 <= S <= C and H <= log C both
log S and sum_i p_i |d_i| are at most log C.  Per class p_i |d_i| <= |d_i| e^-|d_i| <= 1 / e and p_i d_i^2 <= 4 / e^2 < 0.55.
  S:      e_i is off by at most 8 u e_i + u / e, so their exact sum by (8 + C / e) u relative (S >= 1); the additions add (C - 1) u:
          eS <= (1.37 C + 7) u <= (1.5 C + 7) u relative.
  log S:  |log S_k - log S| <= eS, and logf adds one ulp of a value of at most log C: 2 u log C.
  terms:  p_i = e_i / S is off by (8 + |d_i|) u (its e) + eS (S) + u (the division) relative, d_i by u, the product rounds once more:
          |t_i - p_i d_i| <= p_i |d_i| ((11 + |d_i|) u + eS).  Summed over the classes: 11 u log C + 0.55 C u + eS log C.  (An e_i below
          the normal range, where expf's error is not relative, has p_i |d_i| < 2^-119: nothing.)
  sum:    the tree adds at most 6 levels, each u relative to sum |t_i| <= log C: 6 u log C; the final subtraction u log C.
Hence |H_k - H| <= ((1.5 C + 7)(1 + log C) + 20 log C + C) u, and n times that for entsum.
"""
import math

import numpy as np

U = 2.0 ** -24


def p_bound(C):
    return (C + 16) * U


def h_bound(C):
    return ((1.5 * C + 7) * (1 + math.log(C)) + 20 * math.log(C) + C) * U


def logits(r, W, bias=None):
    """r fp32 [..., width], W fp32 [C, width], bias fp32 [C] or None -> fp32 [..., C]: z = bias; z = z + W[i][k] * r[k] for k ascending
    in fp64 (a product of two fp32 values is exact there), rounded to fp32 at the end."""
    C, width = W.shape
    z = np.zeros(r.shape[:-1] + (C,), dtype=np.float64)
    if bias is not None:
        z = z + bias.astype(np.float64)
    W64, r64 = W.astype(np.float64), r.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(width):
            z = z + W64[:, k] * r64[..., k, None]
        return z.astype(np.float32)


def votes(v):
    """v fp32 [n, B, C] -> int64 [B, C + 1]: argmax counts (the lowest index on a tie), column C the samples with a NaN logit."""
    n, B, C = v.shape
    out = np.zeros((B, C + 1), dtype=np.int64)
    bad = np.isnan(v).any(axis=2)
    arg = np.where(bad, C, np.argmax(v, axis=2))
    for j in range(n):
        np.add.at(out, (np.arange(B), arg[j]), 1)
    return out


def sums(p):
    """p fp32 [n, B, C] -> (psum, psumsq) fp64 [B, C] by the sequential loop over the samples."""
    s = np.zeros(p.shape[1:], dtype=np.float64)
    q = np.zeros(p.shape[1:], dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(p.shape[0]):
            g = p[j].astype(np.float64)
            s = s + g
            q = q + g * g
    return s, q


def softmax64(v):
    """v fp32 [..., C] -> (p fp64 [..., C], H fp64 [...]): the softmax of the fp32 logits and its entropy log S - sum p (v - m), in fp64."""
    with np.errstate(invalid="ignore", over="ignore"):
        v64 = v.astype(np.float64)
        d = v64 - v64.max(axis=-1, keepdims=True)
        e = np.exp(d)
        S = e.sum(axis=-1, keepdims=True)
        p = e / S
        H = np.log(S[..., 0]) - (p * d).sum(axis=-1)
    return p, H


def device_sigmoid(v, device):
    """The library's own sigmoid of fp32 [n, B, C], per row from `moments_accumulate` with n = 1 (sum = 0 + g, exact): needs a GPU."""
    import torch
    from montecarlopredictivecoding_amd.engine import moments_accumulate
    n, B, C = v.shape
    buf = torch.from_numpy(np.ascontiguousarray(v)).to(device)
    one = torch.zeros(B, C, dtype=torch.float64, device=device)
    g = np.empty_like(v)
    for j in range(n):
        moments_accumulate(buf, j, 1, 1, one, None, transform="sigmoid", accumulate=False)
        g[j] = one.cpu().numpy().astype(np.float32)
    return g

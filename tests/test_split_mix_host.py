"""The second piece of the fp16 operand split, rounded once (csrc/mcpc_gemm_f16.h: split2_pair), against the two roundings it replaced.

`split2_pair` cuts x 2^e into two fp16 pieces: h = fp16(x s) and m = fp16(x s - h), s = 2^e.  Until this test came m was rounded twice --
r = fp32(x s - h), m = fp16(r) -- and now it is one fused multiply-add that reads the fp16 h and rounds to fp16 (v_fma_mixlo_f16 /
v_fma_mixhi_f16: m = fp16(x s - h) with the exact product and difference).  Both give the same bits because the exact residual is an
fp32 already: it is a multiple of ulp(x s) and no larger than |x s|.  This is the NumPy model of both, on the host:

    exact   d = x s - h in float64 (x s: 24 significant bits times a power of two; h within half an fp16 ulp of it: d is exact)
    once    fp16(d)
    twice   fp16(fp32(d))                    -- the parent's contracted form, v_fma_f32 x, s, -h then v_cvt_pk_f16_f32
    parent  fp16(fp32(fp32(x s) - fp32(h)))  -- the parent's source as written, v_pk_mul_f32 then the subtraction

over every scale exponent the kernels can choose (kScaleClamp: -60 .. 60), on
  * random fp32 bit patterns of every exponent (so that m is an fp16 subnormal or zero in a large share of them),
  * every fp16 binade boundary of x s, 2^-24 (the smallest subnormal) .. 2^15 and 65504 / 65520, a few fp32 ulps to either side,
  * the rounding boundaries of m itself: x s = h + (an fp16 midpoint of the residual's binade), a few fp32 ulps to either side,
  * x s at and beyond 65520, where h overflows to Inf (m = -Inf for a finite x s, NaN for an infinite one),
  * fp32 subnormal x (s large: the product is exact and may become normal; s small: the product is an fp32 subnormal or zero),
  * both zeros, both infinities, NaN.
Bit patterns are compared (NaN only as NaN: its payload is the hardware's).  The one boundary where the forms DO differ is outside what
the kernels feed them and is pinned by a test of its own: a FINITE x whose product x s overflows fp32.  There h is Inf either way, the
two-step forms give Inf - Inf = NaN and the single rounding gives -/+Inf.  A scale is chosen from its row's maximum so that |x s| < 2^15,
or is the fixed exponent of a bounded operand, or is clamped to 2^+-60 (then |x| < 2^-45 resp. the product only shrinks): no product comes
near 2^128."""
import numpy as np

SCALES = list(range(-60, 61))
F16_MAX_BITS = 0x7C00


def _f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def _models(x, e):
    """bit patterns of h and of m by the three forms, for fp32 x and the scale 2^e"""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        s32 = np.float32(2.0) ** np.float32(e)
        xs32 = (x * s32).astype(np.float32)                       # v_pk_mul_f32: rounds only when the product is an fp32 subnormal / overflows
        h = xs32.astype(np.float16)                               # v_cvt_pk_f16_f32, round to nearest even
        d = x.astype(np.float64) * np.float64(2.0) ** e - h.astype(np.float64)      # exact
        once = d.astype(np.float16)
        twice = d.astype(np.float32).astype(np.float16)
        parent = (xs32 - h.astype(np.float32)).astype(np.float32).astype(np.float16)
    return h, d, once, twice, parent


def _same_bits(a, b):
    an, bn = np.isnan(a), np.isnan(b)
    return (an & bn) | (~an & ~bn & (a.view(np.uint16) == b.view(np.uint16)))


def _product_is_fp32(x, e):
    """the domain: x s is a finite fp32 (or x itself is not finite)"""
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.abs(x.astype(np.float64)) * np.float64(2.0) ** e
    return ~np.isfinite(x) | (p <= np.float64(np.finfo(np.float32).max))


def _check(x, e, what):
    x = x[_product_is_fp32(x, e)]
    assert x.size, (what, e)
    h, d, once, twice, parent = _models(x, e)
    # The source as written and its compiled form part in ONE respect, the sign of a zero: a nonzero x whose product underflows fp32
    # altogether (|x s| < 2^-150) has fp32(x s) = h = -0 for x < 0, and (-0) - (-0) is +0 where the fma's exact x s - (-0) < 0 rounds
    # to -0.  The kernels never ran the unfused subtraction (the compiler contracts it: `v_fma_f32 r, x, s, -h` in the parent's
    # assembly, profiles/gemm_diet_asm.txt), so there `parent` is held to the value only; everywhere else to the bits.
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        flushed = (x != 0) & ((x * np.float32(2.0) ** np.float32(e)).astype(np.float32) == 0)
    assert np.all(parent[flushed] == 0) and np.all(once[flushed] == 0)
    bad = ~_same_bits(once, twice) | (~_same_bits(once, parent) & ~flushed)
    assert not bad.any(), (what, e, int(bad.sum()), x[bad][:4].view(np.uint32), once[bad][:4], twice[bad][:4], parent[bad][:4])
    return h, d, once


def _around(center_bits, span=4):
    """fp32 bit patterns within `span` ulps of each centre, both signs"""
    c = np.asarray(center_bits, dtype=np.int64)[:, None] + np.arange(-span, span + 1, dtype=np.int64)[None, :]
    c = np.clip(c.ravel(), 0, 0x7F7FFFFF).astype(np.uint32)
    return np.concatenate([c, c | np.uint32(0x80000000)])


def _scaled_back(xs_bits, e):
    """x such that x 2^e is the given fp32 (where that x is an fp32 itself: elsewhere the nearest one, which is as good a test value)"""
    with np.errstate(over="ignore", under="ignore"):
        return (_f32(xs_bits).astype(np.float64) * np.float64(2.0) ** -e).astype(np.float32)


def test_random_bit_patterns_under_every_scale():
    rng = np.random.default_rng(20240611)
    n_sub = 0
    for e in SCALES:
        bits = rng.integers(0, 1 << 32, size=60000, dtype=np.uint64).astype(np.uint32)
        # half of them moved to where the product lands in fp16's range and below it (m normal, subnormal and zero)
        want = rng.integers(127 - 40, 127 + 17, size=30000) - e
        ok = (want > 0) & (want < 255)
        half = bits[:30000]
        half[ok] = (half[ok] & np.uint32(0x807FFFFF)) | (want[ok].astype(np.uint32) << np.uint32(23))
        _, _, once = _check(_f32(bits), e, "random")
        mb = once.view(np.uint16) & np.uint16(0x7FFF)
        n_sub += int(((mb > 0) & (mb < 0x0400)).sum())
    assert n_sub > 200000, n_sub          # second pieces that are fp16 subnormals were really among them


def test_fp16_binade_boundaries_of_the_product():
    edges = [np.float32(2.0) ** np.float32(k) for k in range(-26, 17)] + [np.float32(65504.0), np.float32(65520.0), np.float32(65536.0)]
    centers = np.array(edges, dtype=np.float32).view(np.uint32)
    for e in SCALES:
        _check(_scaled_back(_around(centers), e), e, "binade boundaries")


def test_rounding_boundaries_of_the_second_piece():
    # x s = h + t with t on and around the midpoints between neighbouring fp16 values of the residual's range: where a value rounded to
    # fp32 first could land on a midpoint and then go the other way
    rng = np.random.default_rng(7)
    hs = np.concatenate([np.arange(0x0001, F16_MAX_BITS, 37, dtype=np.uint16), np.array([0x0001, 0x03FF, 0x0400, 0x7BFF], dtype=np.uint16)])
    h = hs.view(np.float16).astype(np.float64)
    def ulp16(v):       # spacing of fp16 at v (the top binade's included, where np.spacing overflows)
        return 2.0 ** np.maximum(np.floor(np.log2(np.maximum(np.abs(v.astype(np.float64)), 2.0 ** -24))) - 10, -24)
    ulp_h = ulp16(hs.view(np.float16))
    xs = []
    for frac in (0.5, 0.25, 0.125, 2.0 ** -11, 2.0 ** -12, 3 * 2.0 ** -13):
        t = ulp_h * frac
        # midpoints of m's own grid below t
        t16 = t.astype(np.float16)
        tm = t16.astype(np.float64) + 0.5 * ulp16(t16)
        xs += [h + t, h - t, h + tm, h - tm]
    centers = np.concatenate(xs).astype(np.float32).view(np.uint32)
    centers = centers[rng.permutation(centers.size)[:6000]]
    for e in SCALES:
        _check(_scaled_back(_around(centers, 3), e), e, "midpoints of the second piece")


def test_first_piece_overflowing_to_inf():
    big = np.array([65519.996, 65520.0, 65536.0, 1e5, 2.0 ** 20, 2.0 ** 67, 2.0 ** 100, 3e38], dtype=np.float32).view(np.uint32)
    for e in SCALES:
        x = _scaled_back(_around(big), e)
        h, d, once = _check(x, e, "h overflows")
        # (where the product stayed an fp32: h = +-Inf makes m the opposite infinity, in one rounding as in two)
        x_in = x[_product_is_fp32(x, e)]
        sel = np.isinf(h) & np.isfinite(x_in)
        assert np.all(np.isinf(once[sel]) & (np.signbit(once[sel]) != np.signbit(h[sel])))


def test_fp32_subnormal_inputs_zeros_and_non_finite_values():
    sub = np.concatenate([np.arange(1, 4096, dtype=np.uint32), np.arange(0x007FF000, 0x00800010, dtype=np.uint32),
                          np.random.default_rng(3).integers(1, 0x00800000, size=20000, dtype=np.uint64).astype(np.uint32)])
    special = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001], dtype=np.uint32)
    x = _f32(np.concatenate([sub, sub | np.uint32(0x80000000), special]))
    for e in SCALES:
        h, d, once = _check(x, e, "subnormal inputs")
        zero = x[_product_is_fp32(x, e)] == 0
        # x = +-0: h keeps the sign and m is +0 (x s - h = (+-0) - (+-0))
        assert np.all(once[zero].view(np.uint16) == 0) and np.all(np.signbit(h[zero]) == np.signbit(x[_product_is_fp32(x, e)][zero]))


def test_the_residual_is_an_fp32_wherever_the_product_is_a_normal_one():
    # the reason the two forms agree, checked on its own: fp32(d) == d
    rng = np.random.default_rng(11)
    for e in (-60, -17, 0, 14, 60):
        x = _f32(rng.integers(0, 1 << 32, size=200000, dtype=np.uint64).astype(np.uint32))
        with np.errstate(over="ignore", invalid="ignore"):
            p = np.abs(x.astype(np.float64)) * 2.0 ** e
        x = x[np.isfinite(x) & (p >= np.finfo(np.float32).tiny) & (p < 65520.0)]
        h, d, _, _, _ = _models(x, e)
        assert np.all(d.astype(np.float32).astype(np.float64) == d)
        assert np.all(np.abs(d) <= np.abs(x.astype(np.float64) * 2.0 ** e))


def test_the_one_place_the_forms_differ_a_finite_value_whose_product_overflows_fp32():
    x = np.array([2.0 ** 100, -(2.0 ** 100), 3e38], dtype=np.float32)
    e = 60
    assert not _product_is_fp32(x, e).any()
    h, d, once, twice, parent = _models(x, e)
    assert np.all(np.isinf(h))
    assert np.all(np.isinf(once) & (np.signbit(once) != np.signbit(h)))       # exact product - Inf
    assert np.all(np.isnan(parent))                                            # Inf - Inf

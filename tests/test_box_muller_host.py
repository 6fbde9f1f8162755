"""Box-Muller, host side (no GPU): the float64 definition of tests/box_muller_cases.py against the fp32 NumPy twin, the moments of the
ideal transform on the device's own 2^24 x 2^24 grid inside the caps the device is held to (so that a failure of
tests/test_gpu_box_muller.py is the device's), the closed form of the largest radius, and the argument checks of the entry point and its
binding that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from montecarlopredictivecoding_amd import _lib
from oracle import philox
from tests import box_muller_cases as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_fp64_definition_agrees_with_the_fp32_twin():
    rng = np.random.default_rng(20)
    a = rng.integers(0, 1 << 32, size=1 << 20, dtype=np.uint64).astype(np.uint32)
    b = rng.integers(0, 1 << 32, size=1 << 20, dtype=np.uint64).astype(np.uint32)
    a[:4] = (0, 0xFF, 0xFFFFFFFF, 0xFFFFFF00)                    # the largest radius (twice) and u1 = 1 (twice)
    b[:4] = (0, 0x40000000, 0x80000000, 0xC0000000)              # the quarter turns
    z0, z1 = bm.box_muller(a, b)
    t0, t1 = philox.box_muller(a, b)
    assert z0.dtype == np.float64 and np.isfinite(z0).all() and np.isfinite(z1).all()
    np.testing.assert_allclose(t0, z0, rtol=0, atol=bm.Z_ATOL)
    np.testing.assert_allclose(t1, z1, rtol=0, atol=bm.Z_ATOL)
    # the fields alone matter: the low 8 bits of either word are shifted out
    y0, y1 = bm.box_muller(a | np.uint32(0xFF), b & np.uint32(0xFFFFFF00))
    assert np.array_equal(y0, z0) and np.array_equal(y1, z1)
    assert np.array_equal(bm.u1_of(a).astype(np.float32), philox.u32_to_unit_open0(a))
    assert np.array_equal(bm.u2_of(b).astype(np.float32), philox.u32_to_unit_half_open(b))


def test_the_largest_radius_and_the_zero():
    assert bm.R_MAX == pytest.approx(5.768108, abs=1e-6)
    assert bm.radius(np.uint32([0, 0xFF]))[0] == bm.radius(np.uint32([0, 0xFF]))[1] == pytest.approx(np.sqrt(48.0 * np.log(2.0)), rel=1e-15)
    assert bm.radius(np.uint32([0xFFFFFF00, 0xFFFFFFFF])).tolist() == [0.0, 0.0]
    # next to u1 = 1: -2 ln(1 - 2^-24) = 2^-23 (1 + 2^-25 + ...)
    assert bm.radius(np.uint32([0xFFFFFE00]))[0] == pytest.approx(np.sqrt(2.0 ** -23 * (1 + 2.0 ** -25)), rel=1e-14)
    R = bm.ideal_tables()[0]
    assert R.max() == R[0] and R.min() == R[-1] == 0.0 and np.all(np.diff(R) < 0)
    # the derived bound: 2^-22 and a second-order allowance; the constant is closer to -2 ln 2 than the derivation assumes
    assert 2.0 ** -22 < bm.RADIUS_RTOL < 2.0 ** -22 * 1.00001 and bm.C_REL_ERR < bm.EPS
    assert bm.R_MAX * (1 + bm.RADIUS_RTOL) < 5.76812


def test_the_ideal_transform_on_the_grid_is_inside_the_caps():
    R, Cc, S = bm.ideal_tables()
    m = bm.grid_moments(R, Cc, S)
    print("[box-muller] ideal fp64 transform on the 2^24 x 2^24 grid: " + "  ".join(f"{k} = {v:.10g}" for k, v in m.items()))
    assert bm.cap_violations(m) == {}
    for k, want in bm.IDEAL.items():
        assert abs(m[k] - want) <= 1e-8, (k, m[k], want)
    assert abs(m["E sin^2"] - 0.5) <= 1e-8 and abs(m["E sin^4"] - 0.375) <= 1e-8
    assert max(abs(m["E cos"]), abs(m["E sin"]), abs(m["E cos sin"])) <= 1e-12
    # E r^2 = -(2 / N) ln(N! / N^N) = 2 - ln(2 pi N) / N - 1 / (6 N^2) + ... (Stirling)
    assert m["E r^2"] == pytest.approx(2.0 - np.log(2.0 * np.pi * bm.N) / bm.N, abs=1e-12)
    # the caps have teeth: a cosine table 2e-5 too large, leaning 2e-5 towards the sine, or offset by 1e-6; a radius table 1e-5 too long
    assert "E z0^2" in bm.cap_violations(bm.grid_moments(R, Cc * (1 + 2e-5), S))
    assert "E z0 z1" in bm.cap_violations(bm.grid_moments(R, Cc + 2e-5 * S, S))
    assert "E z0" in bm.cap_violations(bm.grid_moments(R, Cc + 1e-6, S))
    assert {"E z0^2", "E z1^2"} <= set(bm.cap_violations(bm.grid_moments(R * (1 + 1e-5), Cc, S)))
    assert {"E z0^4", "E z1^4"} <= set(bm.cap_violations(bm.grid_moments(R * (1 + 1e-5), Cc, S)))


def test_entry_point_is_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "mcpc.h")) as f:
        hdr = f.read()
    decl = re.search(r"int mcpc_box_muller\(([^;]*)\);", hdr).group(1)
    res, args = _lib.SYMBOLS["mcpc_box_muller"]
    assert res is C.c_int and len(args) == len(decl.split(",")) == 7
    assert "#define MCPC_ABI_VERSION 4" in hdr or re.search(r"MCPC_ABI_VERSION\s+4\b", hdr)
    lib = _lib.load()
    assert lib.mcpc_abi_version() == 4 and hasattr(lib, "mcpc_box_muller")


def test_argument_errors_are_refused_before_any_device_work():
    """Every MCPC_EINVAL case returns -1 with a message and touches no device: the pointers are never dereferenced."""
    lib = _lib.load()
    p = [C.c_void_p(0x1000 * (i + 1)) for i in range(4)]         # never dereferenced: every call below is refused or empty

    def call(a=p[0], b=p[1], n=8, z0=p[2], z1=p[3]):
        rc = lib.mcpc_box_muller(0, a, b, n, z0, z1, None)
        return rc, lib.mcpc_last_error().decode()

    for kw, word in [(dict(a=None), "null"), (dict(b=None), "null"), (dict(z0=None), "null"), (dict(z1=None), "null"),
                     (dict(n=-1), "n=-1"), (dict(n=-(1 << 40)), "n=-")]:
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("box_muller:") and word in msg, (kw, rc, msg)
    assert call(n=0)[0] == 0                                       # nothing to transform: no launch, no device


def test_the_binding_checks_its_tensors_before_any_device_work():
    from montecarlopredictivecoding_amd.engine import box_muller
    i32 = torch.zeros(8, dtype=torch.int32)
    with pytest.raises(TypeError, match=r"a: expected a torch.Tensor \[n\]"):
        box_muller(np.zeros(8, np.int32), i32)
    with pytest.raises(TypeError, match=r"b: expected a torch.Tensor \[n\]"):
        box_muller(i32, i32.reshape(2, 4))
    with pytest.raises(TypeError, match="a: expected torch.int32 or torch.uint32, got torch.float32"):
        box_muller(i32.float(), i32)
    with pytest.raises(TypeError, match="b: expected torch.int32 or torch.uint32, got torch.int64"):
        box_muller(i32, i32.long())
    with pytest.raises(ValueError, match="a: expected a tensor on a HIP device, got cpu"):
        box_muller(i32, i32)

"""The record entry points' shared argument checks, host side (no GPU): each of the six accumulate entries is called with one argument
of its record window wrong at a time, and the two evaluators with a null engine.  Every call is refused with MCPC_EINVAL before any
device work -- the pointers are fake and never dereferenced -- and `mcpc_last_error()` is compared as a whole string.  The strings
were recorded from the library as it was before the entries shared their checks (commit 2230ea4): they are the interface, whichever
helper formats them."""
import ctypes as C

import numpy as np
import pytest

from montecarlopredictivecoding_amd import _lib

EINVAL = -1
REC, P1, P2, P3, P4 = (C.c_void_p(0x1000 * i) for i in range(1, 6))        # never dereferenced: every call below is refused
EDGES = np.linspace(-1, 1, 5).astype(np.float32)


def _moments(lib, rec=REC, first=0, stride=1, n=4, transform=0):
    return lib.mcpc_moments_accumulate(0, rec, 15, first, stride, n, transform, P1, P2, 1, None)


def _cov(lib, rec=REC, B=3, first=0, stride=1, n=4, transform=0):
    recs = None if rec is None else (C.c_void_p * 2)(0x1000, 0x2000)
    widths, xf = (C.c_int32 * 2)(5, 7), (C.c_int32 * 2)(0, transform)
    return lib.mcpc_cov_accumulate(0, recs, widths, xf, 2, B, first, stride, n, 0, P1, 1, None, 0, None)


def _hist(lib, rec=REC, B=3, width=5, first=0, stride=1, n=4, transform=0):
    return lib.mcpc_hist_accumulate(0, rec, B, width, first, stride, n, transform, EDGES.ctypes.data_as(C.POINTER(C.c_float)), 4, 0, P1, 1, None)


def _acov(lib, rec=REC, B=3, width=5, first=0, stride=1, n=4, transform=0):
    return lib.mcpc_acov_accumulate(0, rec, B, width, first, stride, n, transform, 3, 0, P1, P2, P3, P4, None)


def _roll(lib, rec=REC, B=3, width=5, first=0, stride=1, n=4, transform=0):
    return lib.mcpc_roll_accumulate(0, rec, B, width, first, stride, n, transform, 4, 1, 0, P1, P2, P3, P4, None, None, None)


def _probe(lib, rec=REC, B=3, width=5, first=0, stride=1, n=4):
    return lib.mcpc_probe_accumulate(0, rec, B, width, first, stride, n, P1, None, 3, 0, P2, None, P3, P4, 1, None)


ENTRIES = {"moments": _moments, "cov": _cov, "hist": _hist, "acov": _acov, "roll": _roll, "probe": _probe}

# (entry, the one wrong argument, the whole message)
TABLE = [(name, kw, f"{name}: {text}")
         for name in ENTRIES
         for kw, text in [(dict(first=-1), "first=-1, must not be negative"),
                          (dict(stride=0), "stride=0, must be at least 1"),
                          (dict(n=-1), "n=-1, must not be negative"),
                          (dict(rec=None), "rec is null with n=4")]]
TABLE += [(name, dict(transform=xf), f"{name}: unknown transform {xf}") for name in ("moments", "hist", "acov", "roll") for xf in (2, -1)]
TABLE += [("cov", dict(transform=xf), f"cov: unknown transform {xf} of block 1") for xf in (2, -1)]          # (its own wording: per block)
TABLE += [(name, dict(B=0), f"{name}: B=0, must be at least 1") for name in ("cov", "hist", "acov", "roll", "probe")]
TABLE += [(name, dict(width=0), f"{name}: width=0, must be at least 1") for name in ("hist", "acov", "roll", "probe")]


@pytest.mark.parametrize("name, kw, message", TABLE, ids=[f"{n}-{k}={v}" for n, kw, _ in TABLE for k, v in kw.items()])
def test_one_wrong_window_argument_is_refused_with_the_recorded_message(name, kw, message):
    lib = _lib.load()
    rc = ENTRIES[name](lib, **kw)
    got = lib.mcpc_last_error().decode()
    assert rc == EINVAL and got == message and got.startswith(name + ":"), (name, kw, rc, got)


def test_the_table_covers_every_entry_and_every_shared_argument():
    have = {(name, key) for name, kw, _ in TABLE for key in kw}
    for name in ENTRIES:
        want = {"first", "stride", "n", "rec"} | ({"transform"} if name != "probe" else set()) | ({"B"} if name != "moments" else set())
        want |= {"width"} if name not in ("moments", "cov") else set()
        assert {key for n, key in have if n == name} == want, name
    assert len(TABLE) == 6 * 4 + 5 * 2 + 5 + 4


def test_a_good_window_with_nothing_to_add_is_accepted_without_a_device():
    lib = _lib.load()
    for name, fn in ENTRIES.items():
        if name in ("acov", "roll"):
            continue                                     # (their streams start empty with n = 0 and n_seen = 0: that zeroes outputs on the device)
        assert fn(lib, rec=None, n=0) == 0, name


def test_the_evaluators_refuse_a_null_engine():
    lib = _lib.load()
    x_rec = (C.c_void_p * 6)(*[0x1000] * 6)
    assert lib.mcpc_chain_energies(None, REC, x_rec, 2, 0, 1.0, 0, P1, 0, None) == EINVAL
    assert lib.mcpc_last_error().decode() == "chain energies: null engine"
    assert lib.mcpc_prediction_errors(None, REC, x_rec, 2, 0, 1.0, 0, x_rec, x_rec, None, None, 0, None) == EINVAL
    assert lib.mcpc_last_error().decode() == "prediction errors: null engine"

"""The three entry points of the Hamiltonian transition on the device (include/mcpc.h: mcpc_hmc_begin, mcpc_hmc_leap, mcpc_hmc_accept;
csrc/mcpc_hmc.h) against the restatements of tests/hmc_cases.py: the first and the interior leapfrog step bitwise on the device's own
normals, K0 and log_alpha at their roundoff bound 2^-41, the uniform exactly, every decision, the in-place overwrite of accepted
chains and of those alone, and what the header promises about isolation: a chain's result does not depend on the other chains, a
non-finite chain rejects and stays alone, nothing is written beyond rows x n_l, a refused call launches nothing."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import hmc_cases as H
from tests import parity_log
from tests.test_gpu_mala_kernels import DEV, GUARD, SENTINEL, _arr, dev, guarded, guards_intact, ibits, same

pytestmark = pytest.mark.gpu
CASES = sorted(H.KERNEL_CASES)
R = H.KERNEL_RUN
assert GUARD > 0 and SENTINEL < 0


def normals(widths, rows, step, base=None):
    from montecarlopredictivecoding_amd.engine import philox_normals
    base = R["chain_base"] if base is None else base
    return [philox_normals(R["seed"], step, l, base, rows, n, torch.device(DEV)) for l, n in enumerate(widths)]


def f32bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def blank(ts):
    """Guarded outputs shaped like ``ts``, filled with the sentinel: (wholes, views)."""
    pairs = [guarded(np.full(t.shape, SENTINEL, dtype=np.float32)) for t in ts]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def begin(name, rows=None):
    """One hmc_begin on (a slice of) a case, outputs guarded.  Returns a dict of the tensors after the call."""
    from montecarlopredictivecoding_amd.engine import hmc_begin
    xs, gs = H.kernel_inputs(name)[:2]
    sel = slice(None) if rows is None else rows
    xs, gs = [np.array(t[sel]) for t in xs], [np.array(t[sel]) for t in gs]
    base = R["chain_base"] + (0 if rows is None else rows.start)
    out = dict(n=xs[0].shape[0], base=base, inputs=(xs, gs), x=[dev(t) for t in xs], g=[dev(t) for t in gs])
    out["q_whole"], out["q"] = blank(xs)
    out["xt_whole"], out["xt"] = blank(xs)
    out["K0_whole"], out["K0"] = guarded(np.full(out["n"], SENTINEL), torch.float64)
    got = hmc_begin(out["x"], out["g"], R["lr"], R["seed"], R["step"], base, q_out=out["q"], x_out=out["xt"], K0=out["K0"])
    torch.cuda.synchronize()
    assert got[0] is out["q"] and got[1] is out["xt"] and got[2] is out["K0"]
    return out


def leap(name, rows=None):
    """One hmc_leap on (a slice of) a case's (x_t, q, g_t), the in-place tensors guarded."""
    from montecarlopredictivecoding_amd.engine import hmc_leap
    _, _, _, xts, gts, _, qs, _ = H.kernel_inputs(name)
    sel = slice(None) if rows is None else rows
    xts, gts, qs = ([np.array(t[sel]) for t in ts] for ts in (xts, gts, qs))
    out = dict(inputs=(xts, gts, qs), gt=[dev(t) for t in gts])
    for key, ts in (("xt", xts), ("q", qs)):
        pairs = [guarded(t) for t in ts]
        out[key + "_whole"], out[key] = [p[0] for p in pairs], [p[1] for p in pairs]
    hmc_leap(out["xt"], out["q"], out["gt"], R["lr"])
    torch.cuda.synchronize()
    return out


def accept(name, *, rows=None, plant=None, n_accepted_start=5, optional=True):
    """One hmc_accept on (a slice of) a case, everything written guarded.  ``plant``: (which of "q" / "gt" / "xt" / "Et" / "K0", row,
    value).  Returns a dict of the tensors after the call."""
    from montecarlopredictivecoding_amd.engine import hmc_accept
    xs, gs, E, xts, gts, Et, qs, K0 = H.kernel_inputs(name)
    sel = slice(None) if rows is None else rows
    cut = lambda ts: [np.array(t[sel]) for t in ts]                     # noqa: E731
    xs, gs, xts, gts, qs = cut(xs), cut(gs), cut(xts), cut(gts), cut(qs)
    E, Et, K0 = np.array(E[sel]), np.array(Et[sel]), np.array(K0[sel])
    n = E.shape[0]
    if plant is not None:
        what, row, value = plant
        if what in ("Et", "K0"):
            ({"Et": Et, "K0": K0}[what])[row] = value
        else:
            ({"q": qs, "gt": gts, "xt": xts}[what])[-1][row, -1] = value
    base = R["chain_base"] + (0 if rows is None else rows.start)
    out = dict(n=n)
    for key, ts in (("x", xs), ("g", gs)):
        pairs = [guarded(t) for t in ts]
        out[key + "_whole"], out[key] = [p[0] for p in pairs], [p[1] for p in pairs]
    out["xt"], out["gt"], out["q"] = [dev(t) for t in xts], [dev(t) for t in gts], [dev(t) for t in qs]
    out["E_whole"], out["E"] = guarded(E, torch.float64)
    out["Et"], out["K0"] = dev(Et, torch.float64), dev(K0, torch.float64)
    out["diag_whole"], out["diag"] = guarded(np.full((n, 3), SENTINEL), torch.float64)
    out["nacc_whole"], out["nacc"] = guarded(np.full(n, n_accepted_start, dtype=np.int32), torch.int32)
    out["inputs"] = (xs, gs, E, xts, gts, Et, qs, K0)
    hmc_accept(out["x"], out["g"], out["E"], out["xt"], out["gt"], out["Et"], out["q"], out["K0"], R["lr"], R["seed"], R["step"], base,
               diag=out["diag"] if optional else None, n_accepted=out["nacc"] if optional else None)
    torch.cuda.synchronize()
    return out


def reference(inputs, base):
    """(log_alpha, M, u, accepted) of the restatement on the inputs of an ``accept`` call."""
    _, _, E, _, gts, Et, qs, K0 = inputs
    la, Mr = H.log_alpha(E, Et, K0, [H.end_momentum(q, gt, R["lr"]) for q, gt in zip(qs, gts)])
    u = H.uniform(R["seed"], R["step"], base, E.shape[0])
    return la, Mr, u, H.decide(la, u)


# ---- begin --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_the_first_step_is_bitwise_the_fp32_restatement_on_the_devices_normals_and_k0_meets_its_bound(name):
    c = H.KERNEL_CASES[name]
    got = begin(name)
    xs, gs = got["inputs"]
    z = [t.cpu().numpy() for t in normals(c["widths"], c["rows"], R["step"])]
    for l, (x, g) in enumerate(zip(xs, gs)):
        q, x1 = H.begin(x, g, z[l], R["lr"])
        assert np.array_equal(f32bits(got["q"][l].cpu().numpy()), f32bits(q)), f"q, layer {l}"
        assert np.array_equal(f32bits(got["xt"][l].cpu().numpy()), f32bits(x1)), f"x_out, layer {l}"
    K0 = H.kinetic(z)
    err = np.abs(got["K0"].cpu().numpy() - K0)
    print(f"{name}: max |K0 err| {err.max():.3g}, largest fraction of the bound {float((err / (H.BOUND * K0)).max()):.3g}")
    parity_log.close("hmc_begin", f"{name} K0 err over 2^-41 K0", err / K0, np.zeros_like(err), atol=H.BOUND)
    assert (err <= H.BOUND * K0).all()
    assert guards_intact(got["q_whole"] + got["xt_whole"] + [got["K0_whole"]])
    for a, b in zip(got["x"] + got["g"], list(xs) + list(gs)):            # the state and its gradient are read only
        assert same(a, dev(b))
    # fresh outputs are the same bits; another step draws another momentum
    from montecarlopredictivecoding_amd.engine import hmc_begin
    q2, x2, k2 = hmc_begin(got["x"], got["g"], R["lr"], R["seed"], R["step"], R["chain_base"])
    assert all(same(a, b) for a, b in zip(q2 + x2 + [k2], got["q"] + got["xt"] + [got["K0"]]))
    q3, _, _ = hmc_begin(got["x"], got["g"], R["lr"], R["seed"], R["step"] + 1, R["chain_base"])
    assert not same(q3[-1], got["q"][-1])


def test_one_leapfrog_step_ends_at_the_mala_proposal():
    """x_out of hmc_begin against mala_propose at noise_var = 2 from the same (x, g, seed, step): the same normals, another order of
    the fp32 operations.  Either path rounds four times and holds two rounded constants (lr, s; eps, h -- eps enters twice), each a
    relative 2^-24 of a quantity no larger than S = |x| + lr |g| + sqrt(2 lr) |xi|: at most 13 of them between the two, 16 x 2^-24 S."""
    from montecarlopredictivecoding_amd.engine import mala_propose
    got = begin("six_layers")
    want = mala_propose(got["x"], got["g"], R["lr"], 2.0, R["seed"], R["step"], R["chain_base"])
    z = normals(H.KERNEL_CASES["six_layers"]["widths"], H.KERNEL_CASES["six_layers"]["rows"], R["step"])
    torch.cuda.synchronize()
    for a, b, x, g, xi in zip(got["xt"], want, got["x"], got["g"], z):
        scale = x.abs() + R["lr"] * g.abs() + math.sqrt(2.0 * R["lr"]) * xi.abs()
        assert bool(((a - b).abs() <= 16 * 2.0 ** -24 * scale).all())


# ---- leap ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_the_interior_step_is_bitwise_the_fp32_restatement_in_place(name):
    got = leap(name)
    xts, gts, qs = got["inputs"]
    for l in range(len(xts)):
        q, x2 = H.leap(xts[l], qs[l], gts[l], R["lr"])
        assert np.array_equal(f32bits(got["q"][l].cpu().numpy()), f32bits(q)), f"q, layer {l}"
        assert np.array_equal(f32bits(got["xt"][l].cpu().numpy()), f32bits(x2)), f"x_t, layer {l}"
        assert same(got["gt"][l], dev(gts[l]))                             # the gradient is read only
    assert guards_intact(got["q_whole"] + got["xt_whole"])


# ---- accept -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_log_alpha_the_uniform_and_every_decision(name):
    la, Mr, u, acc = H.kernel_reference(name)
    got = accept(name)
    diag = got["diag"].cpu().numpy()
    err = np.abs(diag[:, 0] - la)
    print(f"{name}: max |log_alpha err| {err.max():.3g}, largest fraction of the bound {float((err / (H.BOUND * Mr)).max()):.3g}, "
          f"accepted {int(diag[:, 2].sum())} of {acc.size}")
    parity_log.close("hmc_accept", f"{name} log_alpha err over 2^-41 M", err / Mr, np.zeros_like(err), atol=H.BOUND)
    assert (err <= H.BOUND * Mr).all()
    np.testing.assert_array_equal(diag[:, 1], u)
    np.testing.assert_array_equal(diag[:, 2], (np.log(diag[:, 1]) < diag[:, 0]).astype(np.float64))      # on the kernel's own numbers
    np.testing.assert_array_equal(diag[:, 2], acc.astype(np.float64))                                     # every decision, no exception


@pytest.mark.parametrize("name", CASES)
def test_accepted_chains_take_the_end_points_bits_and_rejected_ones_keep_theirs(name):
    _, _, _, acc = H.kernel_reference(name)
    got = accept(name)
    xs, gs, E, xts, gts, Et, qs, K0 = got["inputs"]
    pick = lambda new, old: np.where(acc.reshape(-1, *[1] * (new.ndim - 1)), new, old)       # noqa: E731
    for l in range(len(xs)):
        assert np.array_equal(f32bits(got["x"][l].cpu().numpy()), f32bits(pick(xts[l], xs[l]))), f"x[{l}]"
        assert np.array_equal(f32bits(got["g"][l].cpu().numpy()), f32bits(pick(gts[l], gs[l]))), f"g[{l}]"
    assert np.array_equal(got["E"].cpu().numpy().view(np.int64), pick(Et, E).view(np.int64))
    np.testing.assert_array_equal(got["nacc"].cpu().numpy(), 5 + acc.astype(np.int32))                    # incremented, not overwritten
    assert guards_intact(got["x_whole"] + got["g_whole"] + [got["E_whole"], got["diag_whole"], got["nacc_whole"]])
    for a, b in zip(got["xt"] + got["gt"] + got["q"] + [got["Et"], got["K0"]], list(xts) + list(gts) + list(qs) + [Et, K0]):
        assert same(a, dev(b, a.dtype)), "x_t, g_t, q, E_t or K0 was written"
    # without the optional outputs: the same state
    bare = accept(name, optional=False)
    assert all(same(a, b) for a, b in zip(bare["x"] + bare["g"] + [bare["E"]], got["x"] + got["g"] + [got["E"]]))
    assert bool((bare["diag"] == SENTINEL).all()) and bool((bare["nacc"] == 5).all())


@pytest.mark.parametrize("name", ["three_layers", "six_layers"])
def test_a_chains_result_does_not_depend_on_the_other_chains(name):
    rows = H.KERNEL_CASES[name]["rows"]
    for call, keys, scalars in ((begin, ("q", "xt"), ("K0",)), (leap, ("q", "xt"), ()), (accept, ("x", "g"), ("E", "diag", "nacc"))):
        flat = lambda o, s=slice(None): [ibits(t[s]) for k in keys for t in o[k]] + [ibits(o[k][s]) for k in scalars]  # noqa: E731,B023
        full, again = call(name), call(name)
        assert all(np.array_equal(a, b) for a, b in zip(flat(full), flat(again))), f"{call.__name__}: two runs of one call differ"
        for r in (0, 7, rows - 1):                                       # alone, a chain sits in wave 0 of workgroup 0
            alone = call(name, rows=slice(r, r + 1))
            assert all(np.array_equal(a, b) for a, b in zip(flat(alone), flat(full, slice(r, r + 1)))), f"{call.__name__}: row {r} alone differs"
        cut = 7                                                          # no multiple of 4: the chains change their wave
        lo, hi = call(name, rows=slice(0, cut)), call(name, rows=slice(cut, rows))
        for a, b, c in zip(flat(lo), flat(hi), flat(full)):
            assert np.array_equal(np.concatenate([a, b]), c), f"{call.__name__}: the rows split over two calls differ from one call"


@pytest.mark.parametrize("bad", [math.nan, math.inf])
@pytest.mark.parametrize("what", ["q", "gt", "Et", "K0"])
def test_a_non_finite_trajectory_rejects_and_stays_alone(what, bad):
    """One chain's q, g_t, E_t or K0 holds a NaN or +Inf (q, g_t: in the last unit of the last layer).  A NaN makes log_alpha a NaN; an
    Inf in q or g_t makes K1 = +Inf and log_alpha = -Inf; E_t = +Inf makes it -Inf.  All reject.  K0 = +Inf alone makes log_alpha
    +Inf: that chain ACCEPTS, as the arithmetic says (the restatement agrees); it still touches no other chain."""
    name, r = "three_layers", 6
    clean = accept(name)
    got = accept(name, plant=(what, r, bad))
    la, _, u, acc = reference(got["inputs"], R["chain_base"])
    expect = bool(what == "K0" and bad == math.inf)
    assert bool(acc[r]) == expect
    diag = got["diag"].cpu().numpy()
    assert diag[r, 2] == float(expect) and int(got["nacc"][r]) == 5 + int(expect)
    assert (np.isnan(diag[r, 0]) and np.isnan(la[r])) or diag[r, 0] == la[r]
    xs, gs, E = got["inputs"][:3]
    if not expect:
        for l in range(len(xs)):                                         # the chain keeps its bits
            assert np.array_equal(f32bits(got["x"][l][r].cpu().numpy()), f32bits(xs[l][r]))
            assert np.array_equal(f32bits(got["g"][l][r].cpu().numpy()), f32bits(gs[l][r]))
        assert float(got["E"][r]) == E[r]
    keep = np.arange(got["n"]) != r
    for key in ("x", "g"):
        for a, b in zip(got[key], clean[key]):
            assert np.array_equal(ibits(a)[keep], ibits(b)[keep]), key
    for key in ("E", "diag", "nacc"):
        assert np.array_equal(ibits(got[key])[keep], ibits(clean[key])[keep]), key
    assert guards_intact(got["x_whole"] + got["g_whole"] + [got["E_whole"], got["diag_whole"], got["nacc_whole"]])


def test_a_nan_in_the_state_stays_in_its_chain_through_begin_and_leap():
    from montecarlopredictivecoding_amd.engine import hmc_begin, hmc_leap
    name, r = "three_layers", 6
    clean_b, clean_l = begin(name), leap(name)
    xs, gs = H.kernel_inputs(name)[:2]
    gs = [np.array(g) for g in gs]
    gs[-1][r, -1] = math.nan
    q, xt, K0 = hmc_begin([dev(x) for x in xs], [dev(g) for g in gs], R["lr"], R["seed"], R["step"], R["chain_base"])
    _, _, _, xts, gts, _, qs, _ = H.kernel_inputs(name)
    gts = [np.array(g) for g in gts]
    gts[-1][r, -1] = math.nan
    xt2, q2 = [dev(t) for t in xts], [dev(t) for t in qs]
    hmc_leap(xt2, q2, [dev(g) for g in gts], R["lr"])
    torch.cuda.synchronize()
    keep = np.arange(xs[0].shape[0]) != r
    assert math.isnan(float(q[-1][r, -1])) and math.isnan(float(xt[-1][r, -1])) and math.isnan(float(q2[-1][r, -1]))
    assert math.isfinite(float(K0[r]))                                    # K0 is that of the momentum alone
    for a, b in zip(q + xt + [K0] + q2 + xt2, clean_b["q"] + clean_b["xt"] + [clean_b["K0"]] + clean_l["q"] + clean_l["xt"]):
        assert np.array_equal(ibits(a)[keep], ibits(b)[keep])
    for a, b in zip(q[:-1] + xt[:-1], clean_b["q"][:-1] + clean_b["xt"][:-1]):      # and, in its chain, in its unit
        assert same(a, b)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def _stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _w(widths):
    return None if widths is None else (C.c_int32 * len(widths))(*widths)


def raw_begin(x, g, widths, n_layers, rows, lr, q, out, K0):
    from montecarlopredictivecoding_amd import _lib as L
    return L.load().mcpc_hmc_begin(0, _arr(x), _arr(g), _w(widths), n_layers, rows, lr, 1, 2, 3, _arr(q), _arr(out), _p(K0), _stream())


def raw_leap(xt, q, gt, widths, n_layers, rows, lr):
    from montecarlopredictivecoding_amd import _lib as L
    return L.load().mcpc_hmc_leap(0, _arr(xt), _arr(q), _arr(gt), _w(widths), n_layers, rows, lr, _stream())


def raw_accept(x, g, E, xt, gt, Et, q, K0, widths, n_layers, rows, lr, diag=None, nacc=None):
    from montecarlopredictivecoding_amd import _lib as L
    return L.load().mcpc_hmc_accept(0, _arr(x), _arr(g), _p(E), _arr(xt), _arr(gt), _p(Et), _arr(q), _p(K0), _w(widths), n_layers, rows, lr,
                                    1, 2, 3, _p(diag), _p(nacc), _stream())


def test_refused_calls_launch_nothing_and_no_row_launches_nothing():
    from montecarlopredictivecoding_amd import _lib as L
    rows, widths = 9, [3, 6]
    mk = lambda: [torch.full((rows, n), 0.5, device=DEV) for n in widths]      # noqa: E731
    x, g, xt, gt, q, out = mk(), mk(), mk(), mk(), mk(), mk()
    E, Et = torch.zeros(rows, dtype=torch.float64, device=DEV), torch.full((rows,), -50.0, dtype=torch.float64, device=DEV)
    K0, K0b = torch.full((rows,), 7.0, dtype=torch.float64, device=DEV), torch.full((rows,), SENTINEL, dtype=torch.float64, device=DEV)
    written = x + g + xt + q + out + [E, K0b]
    snap = [t.clone() for t in written]
    good_b = dict(x=x, g=g, widths=widths, n_layers=2, rows=rows, lr=0.1, q=q, out=out, K0=K0b)
    good_l = dict(xt=xt, q=q, gt=gt, widths=widths, n_layers=2, rows=rows, lr=0.1)
    good_a = dict(x=x, g=g, E=E, xt=xt, gt=gt, Et=Et, q=q, K0=K0, widths=widths, n_layers=2, rows=rows, lr=0.1)
    shared = [dict(n_layers=0), dict(n_layers=L.MAX_LATENT + 1), dict(rows=-1), dict(rows=1 << 31), dict(lr=0.0), dict(lr=-0.1),
              dict(lr=math.nan), dict(lr=math.inf), dict(widths=None), dict(widths=[3, 0])]
    for change in shared + [dict(x=None), dict(g=None), dict(x=[x[0], None]), dict(g=[None, g[1]]), dict(q=None), dict(out=[out[0], None]),
                            dict(K0=None)]:
        assert raw_begin(**dict(good_b, **change)) == -1, change
        assert L.load().mcpc_last_error().decode().startswith("hmc_begin:"), change
    for change in shared + [dict(xt=None), dict(q=[q[0], None]), dict(gt=None), dict(gt=[None, gt[1]])]:
        assert raw_leap(**dict(good_l, **change)) == -1, change
        assert L.load().mcpc_last_error().decode().startswith("hmc_leap:"), change
    for change in shared + [dict(x=None), dict(g=[None, g[1]]), dict(E=None), dict(Et=None), dict(K0=None), dict(xt=None),
                            dict(gt=[gt[0], None]), dict(q=None)]:
        assert raw_accept(**dict(good_a, **change)) == -1, change
        assert L.load().mcpc_last_error().decode().startswith("hmc_accept:"), change
    assert raw_begin(**dict(good_b, rows=0)) == 0 and raw_begin(**dict(good_b, rows=0, x=None, g=None, q=None, out=None, K0=None)) == 0
    assert raw_leap(**dict(good_l, rows=0)) == 0 and raw_leap(**dict(good_l, rows=0, xt=None, q=None, gt=None)) == 0
    assert raw_accept(**dict(good_a, rows=0)) == 0
    assert raw_accept(**dict(good_a, rows=0, x=None, g=None, E=None, xt=None, gt=None, Et=None, q=None, K0=None)) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(written, snap)), "a refused call (or a call without rows) wrote"
    # and the good calls work: E_t = E - 50 accepts every chain whatever the uniform, without any optional output
    assert raw_accept(**good_a) == 0 and raw_leap(**good_l) == 0 and raw_begin(**good_b) == 0
    torch.cuda.synchronize()
    assert bool((E == -50.0).all()) and not torch.equal(q[1], snap[7]) and bool((K0b > 0).all())


def test_the_binding_checks_its_arguments():
    from montecarlopredictivecoding_amd.engine import hmc_accept, hmc_begin, hmc_leap
    mk = lambda: [torch.zeros(4, 3, device=DEV), torch.zeros(4, 5, device=DEV)]      # noqa: E731
    x, g, xt, gt, q = mk(), mk(), mk(), mk(), mk()
    E, Et, K0 = (torch.zeros(4, dtype=torch.float64, device=DEV) for _ in range(3))
    hmc_begin(x, g, 0.1, 0, 0)
    hmc_leap(xt, q, gt, 0.1)
    hmc_accept(x, g, E, xt, gt, Et, q, K0, 0.1, 0, 0)
    empty = [t[:0] for t in x]
    assert hmc_begin(empty, empty, 0.1, 0, 0)[2].shape == (0,) and hmc_leap(empty, empty, empty, 0.1) is None
    for args, kw, exc in (((x, g[:1], 0.1, 0, 0), {}, ValueError), (([t.cpu() for t in x], g, 0.1, 0, 0), {}, ValueError),
                          ((x, [t.double() for t in g], 0.1, 0, 0), {}, TypeError), ((x, g, 0.0, 0, 0), {}, ValueError),
                          ((x, g, math.inf, 0, 0), {}, ValueError), (([], [], 0.1, 0, 0), {}, ValueError),
                          ((x, g, 0.1, 0, 0), dict(K0=K0.float()), TypeError), ((x, g, 0.1, 0, 0), dict(q_out=q[:1]), ValueError),
                          ((x, g, 0.1, 0, 0), dict(x_out=[t[:3] for t in xt]), ValueError)):
        with pytest.raises(exc):
            hmc_begin(*args, **kw)
    for args, exc in (((xt, q[:1], gt, 0.1), ValueError), ((xt, q, gt, -1.0), ValueError), ((xt, q, [t.half() for t in gt], 0.1), TypeError)):
        with pytest.raises(exc):
            hmc_leap(*args)
    for kw, exc in ((dict(E=E.float()), TypeError), (dict(Et=Et[:3]), ValueError), (dict(K0=K0[:3]), ValueError), (dict(qs=q[:1]), ValueError),
                    (dict(diag=torch.zeros(4, 2, dtype=torch.float64, device=DEV)), ValueError),
                    (dict(n_accepted=torch.zeros(4, dtype=torch.int64, device=DEV)), TypeError), (dict(lr=math.nan), ValueError)):
        a = dict(xs=x, gs=g, E=E, xts=xt, gts=gt, Et=Et, qs=q, K0=K0, lr=0.1, seed=0, step=0)
        a.update(kw)
        with pytest.raises(exc):
            hmc_accept(**a)

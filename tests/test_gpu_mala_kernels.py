"""The two entry points of the Metropolis-adjusted Langevin step on the device (include/mcpc.h: mcpc_mala_propose, mcpc_mala_accept;
csrc/mcpc_mala.h) against the restatements of tests/mala_cases.py: the proposal bitwise, log_alpha at its roundoff bound 2^-41 M_r,
the uniform exactly, every decision, the in-place overwrite of accepted chains and of those alone, x_next, and what the header promises
about isolation: a chain's result does not depend on the other chains, a non-finite chain rejects and stays alone, nothing is written
beyond rows x n_l, a refused call launches nothing."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import ais_cases as A
from tests import mala_cases as M
from tests import parity_log

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = sorted(M.KERNEL_CASES)
GUARD = 3                                  # sentinel rows behind every output
SENTINEL = -777
R = M.KERNEL_RUN


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a)).to(device=DEV, dtype=dtype).contiguous()


def guarded(a, dtype=torch.float32):
    """(whole, view): a device copy of ``a`` with GUARD sentinel rows behind it, and the contiguous view of the rows of ``a``."""
    a = np.asarray(a)
    whole = torch.full((a.shape[0] + GUARD, *a.shape[1:]), SENTINEL, dtype=dtype, device=DEV)
    whole[:a.shape[0]] = torch.tensor(a).to(device=DEV, dtype=dtype)
    return whole, whole[:a.shape[0]]


def ibits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32).numpy()


def same(a, b):
    return np.array_equal(ibits(a), ibits(b))


def guards_intact(wholes):
    return all(bool((w[-GUARD:] == SENTINEL).all()) for w in wholes)


def normals(widths, rows, step):
    from montecarlopredictivecoding_amd.engine import philox_normals
    return [philox_normals(R["seed"], step, l, R["chain_base"], rows, n, torch.device(DEV)) for l, n in enumerate(widths)]


def accept(name, *, rows=None, plant=None, x_next=False, n_accepted_start=5):
    """One mala_accept on (a slice of) a case, everything guarded.  ``plant``: (which of "xp" / "gp" / "Ep", row, value).
    Returns a dict of the tensors after the call."""
    from montecarlopredictivecoding_amd.engine import mala_accept
    xs, gs, E, xps, gps, Ep = M.kernel_inputs(name)
    sel = slice(None) if rows is None else rows
    cut = lambda ts: [np.array(t[sel]) for t in ts]                     # noqa: E731
    xs, gs, xps, gps, E, Ep = cut(xs), cut(gs), cut(xps), cut(gps), np.array(E[sel]), np.array(Ep[sel])
    n = E.shape[0]
    if plant is not None:
        what, row, value = plant
        Ep[row] = E[row] + 40.0                                          # (see test_a_non_finite_proposal_rejects_and_stays_alone)
        if what == "Ep":
            Ep[row] = value
        else:
            ({"xp": xps, "gp": gps}[what])[-1][row, -1] = value
    base = R["chain_base"] + (0 if rows is None else rows.start)
    out = dict(n=n)
    for key, ts in (("x", xs), ("g", gs)):
        pairs = [guarded(t) for t in ts]
        out[key + "_whole"], out[key] = [p[0] for p in pairs], [p[1] for p in pairs]
    out["xp"], out["gp"] = [dev(t) for t in xps], [dev(t) for t in gps]
    out["E_whole"], out["E"] = guarded(E, torch.float64)
    out["Ep"] = dev(Ep, torch.float64)
    out["diag_whole"], out["diag"] = guarded(np.full((n, 3), SENTINEL), torch.float64)
    out["nacc_whole"], out["nacc"] = guarded(np.full(n, n_accepted_start, dtype=np.int32), torch.int32)
    if x_next:
        pairs = [guarded(np.full(t.shape, SENTINEL, dtype=np.float32)) for t in xs]
        out["next_whole"], out["next"] = [p[0] for p in pairs], [p[1] for p in pairs]
    out["inputs"] = (xs, gs, E, xps, gps, Ep)
    mala_accept(out["x"], out["g"], out["E"], out["xp"], out["gp"], out["Ep"], R["lr"], R["noise_var"], R["seed"], R["step"], base,
                diag=out["diag"], n_accepted=out["nacc"], x_next=out["next"] if x_next else None)
    torch.cuda.synchronize()
    return out


# ---- propose ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_the_proposal_is_bitwise_the_fp32_restatement_on_the_devices_normals(name):
    from montecarlopredictivecoding_amd.engine import mala_propose
    c = M.KERNEL_CASES[name]
    xs, gs = M.kernel_inputs(name)[:2]
    z = normals(c["widths"], c["rows"], R["step"])
    pairs = [guarded(np.full(x.shape, SENTINEL, dtype=np.float32)) for x in xs]
    out = mala_propose([dev(x) for x in xs], [dev(g) for g in gs], R["lr"], R["noise_var"], R["seed"], R["step"], R["chain_base"],
                       out=[p[1] for p in pairs])
    torch.cuda.synchronize()
    for l, (x, g) in enumerate(zip(xs, gs)):
        want = M.propose(x, g, z[l].cpu().numpy(), R["lr"], R["noise_var"])
        assert np.array_equal(out[l].cpu().numpy().view(np.int32), want.view(np.int32)), f"layer {l}"
    assert guards_intact([p[0] for p in pairs])
    fresh = mala_propose([dev(x) for x in xs], [dev(g) for g in gs], R["lr"], R["noise_var"], R["seed"], R["step"], R["chain_base"])
    assert all(same(a, b) for a, b in zip(fresh, out))
    # another step, another chain base: other normals
    other = mala_propose([dev(x) for x in xs], [dev(g) for g in gs], R["lr"], R["noise_var"], R["seed"], R["step"] + 1, R["chain_base"])
    assert not same(other[-1], out[-1])


def test_the_proposal_is_the_fused_langevin_step_of_the_same_seed_and_step():
    """Engine.run(1, noise_mode=PHILOX) from a state against mala_propose from the same state and the engine's own gradient: the
    project's state contract, 1e-5 absolute.  Whether it is in fact bitwise is printed (DESIGN.md section 4 records the answer)."""
    from montecarlopredictivecoding_amd import _lib as L
    from montecarlopredictivecoding_amd.engine import Engine, mala_propose
    c = A.ESTIMATOR_CASES["bern_relu"]
    W, b, data = A.estimator_params("bern_relu")
    rows, lr, seed, step, base = 19, 0.1, 4321, (1 << 32) + 3, 1000
    eng = Engine(list(c["sizes"]), [L.ACT_RELU] * 2, c["n_in"], c["n_out"], rows, device=torch.device(DEV))
    eng.bind_params([dev(w) for w in W], [dev(v) for v in b])
    eng.bind_inputs(None)
    eng.bind_target(dev(np.resize(data, (rows, c["n_out"]))))
    rng = np.random.default_rng(41)
    xs = [dev(rng.standard_normal((rows, n)).astype(np.float32)) for n in c["sizes"]]
    kw = dict(loss_kind=L.LOSS_BERNOULLI, mask_start=c["mask_start"], xopt=L.XOPT_SGD, lr=lr)
    eng.load_state(xs)
    g = eng.run(1, update_x=False, step_base=0, **kw).xgrad
    want = mala_propose(xs, g, lr, 2.0, seed, step, base)
    eng.load_state(xs)
    eng.run(1, noise_mode=L.NOISE_PHILOX, noise_var=2.0, seed=seed, step_base=step, chain_base=base, **kw)
    got = [torch.empty_like(x) for x in xs]
    eng.store_state(got)
    eng.sync_check()
    worst = max(float((a - b).abs().max()) for a, b in zip(got, want))
    bitwise = all(same(a, b) for a, b in zip(got, want))
    print(f"fused step ({eng.last_step_kernel().split('(')[0]}) against mala_propose: max |diff| = {worst:.3g}, bitwise: {bitwise}")
    for l, (a, w) in enumerate(zip(got, want)):
        parity_log.close("mala_propose", f"fused Langevin step, layer {l}", a.cpu().numpy(), w.cpu().numpy(), rtol=0, atol=1e-5)
    eng.close()


# ---- accept -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_log_alpha_the_uniform_and_every_decision(name):
    la, Mr, u, acc = M.kernel_reference(name)
    got = accept(name)
    diag = got["diag"].cpu().numpy()
    err = np.abs(diag[:, 0] - la)
    print(f"{name}: max |log_alpha err| {err.max():.3g}, largest fraction of the bound {float((err / (M.BOUND * Mr)).max()):.3g}, "
          f"accepted {int(diag[:, 2].sum())} of {acc.size}")
    parity_log.close("mala_accept", f"{name} log_alpha err over 2^-41 M", err / Mr, np.zeros_like(err), atol=M.BOUND)
    assert (err <= M.BOUND * Mr).all()
    np.testing.assert_array_equal(diag[:, 1], u)
    np.testing.assert_array_equal(diag[:, 2], (np.log(diag[:, 1]) < diag[:, 0]).astype(np.float64))      # on the kernel's own numbers
    np.testing.assert_array_equal(diag[:, 2], acc.astype(np.float64))                                     # every decision, no exception


@pytest.mark.parametrize("name", CASES)
def test_accepted_chains_take_the_proposals_bits_and_rejected_ones_keep_theirs(name):
    _, _, _, acc = M.kernel_reference(name)
    got = accept(name)
    xs, gs, E, xps, gps, Ep = got["inputs"]
    pick = lambda new, old: np.where(acc.reshape(-1, *[1] * (new.ndim - 1)), new, old)       # noqa: E731
    for l in range(len(xs)):
        assert np.array_equal(got["x"][l].cpu().numpy().view(np.int32), pick(xps[l], xs[l]).view(np.int32)), f"x[{l}]"
        assert np.array_equal(got["g"][l].cpu().numpy().view(np.int32), pick(gps[l], gs[l]).view(np.int32)), f"g[{l}]"
    assert np.array_equal(got["E"].cpu().numpy().view(np.int64), pick(Ep, E).view(np.int64))
    np.testing.assert_array_equal(got["nacc"].cpu().numpy(), 5 + acc.astype(np.int32))                    # incremented, not overwritten
    assert guards_intact(got["x_whole"] + got["g_whole"] + [got["E_whole"], got["diag_whole"], got["nacc_whole"]])
    for a, b in zip(got["xp"] + got["gp"] + [got["Ep"]], list(xps) + list(gps) + [Ep]):                   # the proposal is read only
        assert same(a, dev(b, a.dtype))


@pytest.mark.parametrize("name", CASES)
def test_x_next_is_bitwise_a_separate_proposal_and_changes_nothing_else(name):
    from montecarlopredictivecoding_amd.engine import mala_propose
    plain = accept(name)
    got = accept(name, x_next=True)
    for key in ("x", "g"):
        assert all(same(a, b) for a, b in zip(got[key], plain[key]))
    assert same(got["E"], plain["E"]) and same(got["diag"], plain["diag"]) and same(got["nacc"], plain["nacc"])
    want = mala_propose(got["x"], got["g"], R["lr"], R["noise_var"], R["seed"], R["step"] + 1, R["chain_base"])
    torch.cuda.synchronize()
    assert all(same(a, b) for a, b in zip(got["next"], want))
    assert guards_intact(got["next_whole"])


@pytest.mark.parametrize("name", ["three_layers", "six_layers"])
def test_a_chains_result_does_not_depend_on_the_other_chains(name):
    rows = M.KERNEL_CASES[name]["rows"]
    full = accept(name, x_next=True)
    again = accept(name, x_next=True)
    keys = ("x", "g", "next")
    flat = lambda o, s=slice(None): [ibits(t[s]) for k in keys for t in o[k]] + [ibits(o[k][s]) for k in ("E", "diag", "nacc")]  # noqa: E731
    assert all(np.array_equal(a, b) for a, b in zip(flat(full), flat(again))), "two runs of one call differ"
    for r in (0, 7, rows - 1):                                           # alone, a chain sits in wave 0 of workgroup 0
        alone = accept(name, rows=slice(r, r + 1), x_next=True)
        assert all(np.array_equal(a, b) for a, b in zip(flat(alone), flat(full, slice(r, r + 1)))), f"row {r} alone differs"
    cut = 7                                                              # no multiple of 4: the chains change their wave
    lo, hi = accept(name, rows=slice(0, cut), x_next=True), accept(name, rows=slice(cut, rows), x_next=True)
    for a, b, c in zip(flat(lo), flat(hi), flat(full)):
        assert np.array_equal(np.concatenate([a, b]), c), "the rows split over two calls differ from one call"


@pytest.mark.parametrize("bad", [math.nan, math.inf, 3.4e38])
@pytest.mark.parametrize("what", ["xp", "gp", "Ep"])
def test_a_non_finite_proposal_rejects_and_stays_alone(what, bad):
    """One chain's x', g' or E' holds a NaN, +Inf or 3.4e38 (in the last unit of the last layer).  A NaN makes log_alpha a NaN, an Inf
    in x' makes the two squared norms Inf and their difference a NaN, an Inf or 3.4e38 in g' or E' makes log_alpha -Inf or about -1e75:
    all reject.  3.4e38 in x' is the one case arithmetic alone does not decide: x - x' absorbs lr g' and lr g in fp64, the two squared
    norms are EQUAL bit for bit and log_alpha = E - E', as it is in the restatement.  So in this test the planted chain's E' is E + 40
    in the clean run and the planted one alike: log_alpha <= -40 < log u for every u (log u >= -16.7), a rejection by arithmetic."""
    name, r = "three_layers", 6
    clean = accept(name, x_next=True, plant=("Ep", r, float(M.kernel_inputs(name)[2][r]) + 40.0))
    got = accept(name, x_next=True, plant=(what, r, bad))
    xs, gs, E, xps, gps, Ep = got["inputs"]
    la, _ = M.log_alpha(xs, gs, E, xps, gps, Ep, R["lr"], R["noise_var"])
    assert not (np.log(M.uniform(R["seed"], R["step"], R["chain_base"], got["n"])[r]) < la[r])           # the restatement rejects it
    diag = got["diag"].cpu().numpy()
    assert diag[r, 2] == 0.0 and int(got["nacc"][r]) == 5
    for l in range(len(xs)):                                             # the chain keeps its bits
        assert np.array_equal(got["x"][l][r].cpu().numpy().view(np.int32), xs[l][r].view(np.int32))
        assert np.array_equal(got["g"][l][r].cpu().numpy().view(np.int32), gs[l][r].view(np.int32))
    assert float(got["E"][r]) == E[r]
    keep = np.arange(got["n"]) != r
    for key in ("x", "g", "next"):
        for a, b in zip(got[key], clean[key]):
            assert np.array_equal(ibits(a)[keep], ibits(b)[keep]), key
    for key in ("E", "diag", "nacc"):
        assert np.array_equal(ibits(got[key])[keep], ibits(clean[key])[keep]), key
    assert guards_intact(got["x_whole"] + got["g_whole"] + got["next_whole"] + [got["E_whole"], got["diag_whole"], got["nacc_whole"]])


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def _arr(ts):
    if ts is None:
        return None
    a = (C.c_void_p * len(ts))()
    for i, t in enumerate(ts):
        a[i] = None if t is None else t.data_ptr()
    return a


def raw_propose(x, g, widths, n_layers, rows, lr, noise_var, out):
    from montecarlopredictivecoding_amd import _lib as L
    w = None if widths is None else (C.c_int32 * len(widths))(*widths)
    return L.load().mcpc_mala_propose(0, _arr(x), _arr(g), w, n_layers, rows, lr, noise_var, 1, 2, 3, _arr(out),
                                      C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream))


def raw_accept(x, g, E, xp, gp, Ep, widths, n_layers, rows, lr, noise_var, diag=None, nacc=None, nxt=None):
    from montecarlopredictivecoding_amd import _lib as L
    w = None if widths is None else (C.c_int32 * len(widths))(*widths)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    return L.load().mcpc_mala_accept(0, _arr(x), _arr(g), p(E), _arr(xp), _arr(gp), p(Ep), w, n_layers, rows, lr, noise_var, 1, 2, 3,
                                     p(diag), p(nacc), _arr(nxt), C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream))


def test_refused_calls_launch_nothing_and_no_row_launches_nothing():
    from montecarlopredictivecoding_amd import _lib as L
    rows, widths = 9, [3, 6]
    mk = lambda: [torch.full((rows, n), 0.5, device=DEV) for n in widths]      # noqa: E731
    x, g, xp, gp, out = mk(), mk(), mk(), mk(), mk()
    E, Ep = torch.zeros(rows, dtype=torch.float64, device=DEV), torch.full((rows,), -50.0, dtype=torch.float64, device=DEV)
    snap = [t.clone() for t in x + g + out + [E]]
    good_p = dict(x=x, g=g, widths=widths, n_layers=2, rows=rows, lr=0.1, noise_var=2.0, out=out)
    good_a = dict(x=x, g=g, E=E, xp=xp, gp=gp, Ep=Ep, widths=widths, n_layers=2, rows=rows, lr=0.1, noise_var=2.0)
    shared = [dict(n_layers=0), dict(n_layers=L.MAX_LATENT + 1), dict(rows=-1), dict(lr=0.0), dict(lr=-0.1), dict(lr=math.nan),
              dict(lr=math.inf), dict(noise_var=0.0), dict(noise_var=-2.0), dict(noise_var=math.nan), dict(noise_var=math.inf),
              dict(widths=None), dict(widths=[3, 0]), dict(x=None), dict(g=None), dict(x=[x[0], None]), dict(g=[None, g[1]])]
    for change in shared + [dict(out=None), dict(out=[out[0], None])]:
        assert raw_propose(**dict(good_p, **change)) == -1, change
        assert L.load().mcpc_last_error().decode().startswith("mala_propose:"), change
    for change in shared + [dict(E=None), dict(Ep=None), dict(xp=None), dict(gp=[gp[0], None]), dict(nxt=[out[0], None])]:
        assert raw_accept(**dict(good_a, **change)) == -1, change
        assert L.load().mcpc_last_error().decode().startswith("mala_accept:"), change
    assert raw_propose(**dict(good_p, rows=0)) == 0 and raw_propose(**dict(good_p, rows=0, x=None, g=None, out=None)) == 0
    assert raw_accept(**dict(good_a, rows=0)) == 0 and raw_accept(**dict(good_a, rows=0, x=None, g=None, E=None, xp=None, gp=None, Ep=None)) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(x + g + out + [E], snap)), "a refused call (or a call without rows) wrote"
    # and the good calls work: E' = E - 50 accepts every chain whatever the uniform, without any optional output
    assert raw_propose(**good_p) == 0 and raw_accept(**good_a) == 0
    torch.cuda.synchronize()
    assert bool((E == -50.0).all()) and not torch.equal(out[1], snap[5])


def test_the_binding_checks_its_arguments():
    from montecarlopredictivecoding_amd.engine import mala_accept, mala_propose
    mk = lambda: [torch.zeros(4, 3, device=DEV), torch.zeros(4, 5, device=DEV)]      # noqa: E731
    x, g, xp, gp = mk(), mk(), mk(), mk()
    E, Ep = torch.zeros(4, dtype=torch.float64, device=DEV), torch.zeros(4, dtype=torch.float64, device=DEV)
    mala_propose(x, g, 0.1, 2.0, 0, 0)
    mala_accept(x, g, E, xp, gp, Ep, 0.1, 2.0, 0, 0)
    for args, exc in (((x, g[:1], 0.1, 2.0, 0, 0), ValueError), ((x, [g[0], g[1][:, :4].contiguous()], 0.1, 2.0, 0, 0), ValueError),
                      (([t.cpu() for t in x], g, 0.1, 2.0, 0, 0), ValueError), ((x, [t.double() for t in g], 0.1, 2.0, 0, 0), TypeError),
                      ((x, g, 0.0, 2.0, 0, 0), ValueError), ((x, g, 0.1, math.nan, 0, 0), ValueError), (([], [], 0.1, 2.0, 0, 0), ValueError),
                      ((x * 4, g * 4, 0.1, 2.0, 0, 0), ValueError)):
        with pytest.raises(exc):
            mala_propose(*args)
    for kw, exc in ((dict(E=E.float()), TypeError), (dict(Ep=Ep[:3]), ValueError), (dict(diag=torch.zeros(4, 2, dtype=torch.float64, device=DEV)), ValueError),
                    (dict(n_accepted=torch.zeros(4, dtype=torch.int64, device=DEV)), TypeError), (dict(x_next=x[:1]), ValueError)):
        a = dict(xs=x, gs=g, E=E, xps=xp, gps=gp, Ep=Ep, lr=0.1, noise_var=2.0, seed=0, step=0)
        a.update(kw)
        with pytest.raises(exc):
            mala_accept(**a)

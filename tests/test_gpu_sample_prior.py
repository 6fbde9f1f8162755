"""Ancestral samples drawn on the device (include/mcpc.h: mcpc_sample_prior; csrc/mcpc_ancestral.h).

Networks (n_in - latents - n_out): 5-19-33-130-37 relu, 3-16-20-40 tanh, 2-7-0 identity (ends in a PCLayer), and the first one with
ecoef = (1, 0.25, 4); rows n in {1, 63, 64, 65, 200}.  Widths short of, equal to and over a 16-unit tile and the 128-unit job, a width
that is no multiple of 4, a row tile that is empty, full and ragged.

1. Composition, bitwise: with the returned latents as records, mcpc_prediction_errors on an engine of batch n gives pred_l, and
   x_l == fl(pred_l + fl(s_l z_l)) with z_l from mcpc_philox_normals; HIDDEN == pred_out; MEAN == the sigmoid of mcpc_moments_accumulate;
   the draws from the raw stream / the normals of layer L.
2. Against fp64, per layer: x_l - s_l z_l within the project's prediction bound 1e-6 S_u (tests/test_gpu_pred_err.py) of the NumPy
   fp64 mu_l of the device's own x_{l-1}.  x_l carries two more fp32 roundings than a prediction (of s z and of the sum: at most
   2^-24 (|x| + |s z|) <= 6e-8 (S_u + 2 * 2 * 5.77) with s <= 2 and |z| <= 5.77); the biases of the cases are drawn with 3 <= |b| <= 4,
   so S_u >= 3 and that is under half of the bound, which stays as it is.  The Philox words are compared bitwise with oracle/philox.py.
3. Invariance, bitwise: splits over calls, max_rows, engine forms, what is asked for; guards around every destination; LDS poison.
4. Independence of step, seed and layer.   5. Every refusal launches nothing.   6. The Python fronts.
7. Mean and variance of the read-out of an identity 2-3-4-5 net over 65 536 samples against the analytic N(m, W W^T sums), 6 sigma.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import philox
from tests import loglik_cases as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, STEP, BASE = 0x1234_5678_9ABC, 7, 1000
ACT = {"identity": 0, "relu": 1, "tanh": 2}
NETS = {
    "relu": dict(n_in=5, sizes=(19, 33, 130), n_out=37, act="relu", ecoef=None),
    "tanh": dict(n_in=3, sizes=(16, 20), n_out=40, act="tanh", ecoef=None),
    "nohead": dict(n_in=2, sizes=(7,), n_out=0, act="identity", ecoef=None),
    "ecoef": dict(n_in=5, sizes=(19, 33, 130), n_out=37, act="relu", ecoef=(1.0, 0.25, 4.0)),
}
ROWS = (1, 63, 64, 65, 200)
NMAX = 200
NAN_BITS = 0x7FC0BEEF             # a quiet NaN with a payload


@functools.lru_cache(maxsize=None)
def params(name):
    """Seeded weights, biases (3 <= |b| <= 4, module docstring) and NMAX input rows of a case; never modified."""
    c = NETS[name]
    rng = np.random.default_rng([11, sorted(NETS).index(name)])
    dims = [c["n_in"], *c["sizes"]] + ([c["n_out"]] if c["n_out"] else [])
    W = [(rng.standard_normal((o, i)) * 1.5 / np.sqrt(i)).astype(np.float32) for i, o in zip(dims[:-1], dims[1:])]
    b = [(rng.uniform(3.0, 4.0, o) * rng.choice([-1.0, 1.0], o)).astype(np.float32) for o in dims[1:]]
    inputs = rng.standard_normal((NMAX, c["n_in"])).astype(np.float32)
    for a in (*W, *b, inputs):
        a.setflags(write=False)
    return W, b, inputs


def make_engine(name, batch=64, tuning=None, bind=True):
    from montecarlopredictivecoding_amd.engine import Engine
    c = NETS[name]
    eng = Engine(list(c["sizes"]), [ACT[c["act"]]] * len(c["sizes"]), c["n_in"], c["n_out"], batch, device=torch.device(DEV),
                 ecoef=c["ecoef"], tuning=tuning)
    if bind:
        W, b, _ = params(name)
        eng.bind_params([torch.tensor(w).to(DEV) for w in W], [torch.tensor(v).to(DEV) for v in b])
    return eng


def inputs_of(name, n, first=0):
    return torch.tensor(params(name)[2][first:first + n]).to(DEV).contiguous()


def scales(name):
    c = NETS[name]
    co = c["ecoef"] or (1.0,) * len(c["sizes"])
    return [np.float32(1.0 / np.sqrt(np.float64(np.float32(v)))) for v in co]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def same(a, b, what):
    assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), what


@functools.lru_cache(maxsize=None)
def drawn(name, n=NMAX):
    """(hidden read-out or None, latents) of rows BASE .. BASE + n of a case, from one call on an engine of batch 64; never modified."""
    eng = make_engine(name)
    out, xs = eng.sample_prior(n, SEED, step=STEP, sample_base=BASE, inputs=inputs_of(name, n), latents=True)
    eng.sync_check()
    eng.close()
    return out, xs


def raw_call(eng, n, x_ptrs=None, out=None, *, inputs=None, seed=SEED, step=STEP, base=BASE, loss=0, var=1.0, readout=0, max_rows=0,
             handle="own"):
    arr = None
    if x_ptrs is not None:
        arr = (C.c_void_p * eng.L)()
        for l, t in enumerate(x_ptrs):
            if t is not None:
                arr[l] = t.data_ptr()
    return eng._lib.mcpc_sample_prior(eng._h if handle == "own" else handle, None if inputs is None else C.c_void_p(inputs.data_ptr()), n,
                                      seed, step, base, loss, var, readout, arr, None if out is None else C.c_void_p(out.data_ptr()),
                                      max_rows, eng._stream())


# ---- 1. composition, bitwise ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("name", sorted(NETS))
def test_a_sample_is_the_prediction_plus_the_engines_normals(name, n):
    from montecarlopredictivecoding_amd.engine import moments_accumulate, philox_normals
    c = NETS[name]
    L = len(c["sizes"])
    eng = make_engine(name, batch=n)
    inp = inputs_of(name, n)
    out, xs = eng.sample_prior(n, SEED, step=STEP, sample_base=BASE, inputs=inp, latents=True)
    assert (out is None) == (c["n_out"] == 0) and len(xs) == L
    pe = eng.prediction_errors(inp, xs, quantity="prediction", outputs="prediction" if c["n_out"] else None)
    for l, s in enumerate(scales(name)):
        z = philox_normals(SEED, STEP, l, BASE, n, c["sizes"][l], DEV)
        t = z * torch.tensor(s, device=DEV)
        same(xs[l], pe[f"mu{l}"][0] + t, f"x_{l} = pred + s z")
    if c["n_out"]:
        same(out, pe["out"][0], "HIDDEN is pred_out")
        want = torch.empty(n, c["n_out"], dtype=torch.float64, device=DEV)
        moments_accumulate(out.unsqueeze(0), 0, 1, 1, want, transform="sigmoid", accumulate=False)
        mean = want.to(torch.float32)
        assert torch.equal(mean.double(), want)
        same(eng.sample_prior(n, SEED, step=STEP, sample_base=BASE, inputs=inp, loss="bernoulli", readout="mean")[0], mean, "MEAN, Bernoulli")
        same(eng.sample_prior(n, SEED, step=STEP, sample_base=BASE, inputs=inp, loss="gaussian", readout="mean")[0], out, "MEAN, Gaussian")
        raw = philox_normals(SEED, STEP, L, BASE, n, c["n_out"], DEV, raw=True)
        u = ((raw.to(torch.int64) & 0xFFFFFFFF) >> 8).to(torch.float32) * 2.0 ** -24
        draw = eng.sample_prior(n, SEED, step=STEP, sample_base=BASE, inputs=inp, loss="bernoulli", readout="draw")[0]
        same(draw, (u < mean).to(torch.float32), "DRAW, Bernoulli")
        assert n < 64 or 0.0 < float(draw.mean()) < 1.0
        sd = torch.tensor(np.float32(np.sqrt(0.3)), device=DEV)
        zl = philox_normals(SEED, STEP, L, BASE, n, c["n_out"], DEV)
        same(eng.sample_prior(n, SEED, step=STEP, sample_base=BASE, inputs=inp, loss="gaussian", var=0.3, readout="draw")[0], out + sd * zl,
             "DRAW, Gaussian")
    eng.sync_check()
    eng.close()


# ---- 2. against fp64, per layer -------------------------------------------------------------------------------------------------
def _f(name, a):
    return {"identity": a, "relu": np.maximum(a, 0.0), "tanh": np.tanh(a)}[NETS[name]["act"]]


@pytest.mark.parametrize("name", sorted(NETS))
def test_every_layer_against_fp64_of_the_devices_own_layer_below(name):
    from montecarlopredictivecoding_amd.engine import philox_normals
    c = NETS[name]
    W, b, inputs = (([a.astype(np.float64) for a in p] if isinstance(p, list) else p.astype(np.float64)) for p in params(name))
    out, xs = drawn(name)
    below = inputs
    for l, s in enumerate(scales(name)):
        n_l = c["sizes"][l]
        raw = philox_normals(SEED, STEP, l, BASE, NMAX, n_l, DEV, raw=True).cpu().numpy().view(np.uint32)
        assert np.array_equal(raw, philox.layer_u32(SEED, STEP, l, BASE, NMAX, n_l)), f"the Philox words of layer {l}"
        z = philox_normals(SEED, STEP, l, BASE, NMAX, n_l, DEV).cpu().numpy()
        np.testing.assert_allclose(z, philox.layer_normals(SEED, STEP, l, BASE, NMAX, n_l), rtol=0, atol=2e-5)
        mu = below @ W[l].T + b[l]
        S = np.abs(below) @ np.abs(W[l]).T + np.abs(b[l])
        x = xs[l].cpu().numpy().astype(np.float64)
        frac = np.abs(x - np.float64(s) * z.astype(np.float64) - mu) / (1e-6 * S)
        print(f"{name}: layer {l}: achieved {frac.max():.3f} of the bound (S_u >= {S.min():.2f})")
        assert np.isfinite(x).all() and frac.max() <= 1.0
        below = _f(name, x)
    if c["n_out"]:
        L = len(c["sizes"])
        mu = below @ W[L].T + b[L]
        S = np.abs(below) @ np.abs(W[L]).T + np.abs(b[L])
        frac = np.abs(out.cpu().numpy().astype(np.float64) - mu) / (1e-6 * S)
        print(f"{name}: read-out: achieved {frac.max():.3f} of the bound")
        assert frac.max() <= 1.0


# ---- 3. invariance, bitwise -----------------------------------------------------------------------------------------------------
def _everything(eng, name, n, first=0, **kw):
    out, xs = eng.sample_prior(n, SEED, step=STEP, sample_base=BASE + first, inputs=inputs_of(name, n, first), latents=True, **kw)
    return ([out] if out is not None else []) + xs


@pytest.mark.parametrize("name", ["relu", "tanh", "nohead"])
def test_samples_do_not_depend_on_how_the_rows_are_split(name):
    whole = ([drawn(name)[0]] if NETS[name]["n_out"] else []) + drawn(name)[1]
    eng = make_engine(name, batch=16)
    parts, first = [], 0
    for n in (1, 63, 64, 72):
        parts.append(_everything(eng, name, n, first))
        first += n
    for k, w in enumerate(whole):
        same(torch.cat([p[k] for p in parts]), w, f"1 + 63 + 64 + 72 rows, tensor {k}")
    for k, (w, g) in enumerate(zip(whole, _everything(eng, name, NMAX, max_rows=64))):
        same(g, w, f"max_rows=64, tensor {k}")
    for k, (w, g) in enumerate(zip(whole, _everything(eng, name, NMAX, max_rows=1))):
        same(g, w, f"max_rows=1 (one tile per chunk), tensor {k}")
    eng.sync_check()
    eng.close()


@pytest.mark.parametrize("tuning", ["ws=0", "ws=3", "ws=4"])
def test_samples_do_not_depend_on_the_engines_form(tuning):
    from montecarlopredictivecoding_amd import _lib
    name = "relu"
    try:
        eng = make_engine(name, batch=48, tuning=tuning)
    except _lib.MCPCError as exc:
        assert tuning == "ws=3", exc         # (the one form whose LDS plan may not hold the network)
        print(f"{tuning}: no plan for this network ({exc})")
        return
    print(tuning, eng._lib.mcpc_step_kernel_name(eng._h).decode())
    whole = [drawn(name)[0]] + drawn(name)[1]
    for k, (w, g) in enumerate(zip(whole, _everything(eng, name, NMAX))):
        same(g, w, f"{tuning}, tensor {k}")
    eng.sync_check()
    eng.close()


def test_samples_do_not_depend_on_what_is_asked_for_or_on_foreign_lds_content():
    from montecarlopredictivecoding_amd.engine import debug_poison_lds
    name = "relu"
    out, xs = drawn(name)
    eng = make_engine(name)
    inp = inputs_of(name, NMAX)
    kw = dict(step=STEP, sample_base=BASE, inputs=inp)
    o, x = eng.sample_prior(NMAX, SEED, **kw)
    assert x == [None] * 3
    same(o, out, "the read-out alone")
    o, x = eng.sample_prior(NMAX, SEED, readout=None, latents=(1,), **kw)
    assert o is None and x[0] is None and x[2] is None
    same(x[1], xs[1], "layer 1 alone")
    torch.cuda.synchronize()
    debug_poison_lds(DEV, 0x7FA00000)
    for k, (w, g) in enumerate(zip([out] + xs, _everything(eng, name, NMAX))):
        same(g, w, f"after the LDS was poisoned, tensor {k}")
    eng.sync_check()
    eng.close()


@pytest.mark.parametrize("name,guard", [("relu", 3), ("tanh", 8), ("tanh", 5)], ids=["odd-widths", "vector-stores", "unaligned"])
def test_nothing_is_written_beyond_the_destinations(name, guard):
    c = NETS[name]
    n = 65
    eng = make_engine(name)
    widths = list(c["sizes"]) + [c["n_out"]]
    bufs = [torch.full((2 * guard + n * w,), float("nan"), device=DEV).view(torch.int32).fill_(NAN_BITS).view(torch.float32) for w in widths]
    views = [b[guard:guard + n * w].view(n, w) for b, w in zip(bufs, widths)]
    assert all(v.is_contiguous() for v in views)
    rc = raw_call(eng, n, views[:-1], views[-1], inputs=inputs_of(name, n))
    assert rc == 0, eng._lib.mcpc_last_error()
    eng.sync_check()
    out, xs = drawn(name)
    for k, (v, w, b) in enumerate(zip(views, xs + [out], bufs)):
        same(v, w[:n], f"destination {k}")
        g = bits(b)
        assert (g[:guard] == NAN_BITS).all() and (g[-guard:] == NAN_BITS).all(), f"the guards of destination {k}"
    eng.close()


# ---- 4. independence ------------------------------------------------------------------------------------------------------------
def test_step_seed_and_layer_give_other_normals():
    name = "tanh"
    eng = make_engine(name)
    inp = inputs_of(name, NMAX)
    out, xs = drawn(name)
    for what, kw in (("step", dict(step=STEP + 1)), ("seed", dict(seed=SEED + 1))):
        o, x = eng.sample_prior(NMAX, kw.get("seed", SEED), step=kw.get("step", STEP), sample_base=BASE, inputs=inp, latents=True)
        for k, (a, b) in enumerate(zip([out] + xs, [o] + x)):
            assert bool((a != b).any(dim=1).all()), f"another {what} changes every row of tensor {k}"
    pe = eng.prediction_errors(inputs_of(name, 64), [x[:64].contiguous() for x in xs], quantity="error")
    z0, z1 = pe["e0"][0][:, :16], pe["e1"][0][:, :16]
    assert bool((z0 != z1).all()), "two layers never share normals"
    eng.sync_check()
    eng.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
def test_every_refusal_returns_its_code_and_launches_nothing():
    from montecarlopredictivecoding_amd import _lib
    from montecarlopredictivecoding_amd.engine import Engine
    name = "relu"
    c = NETS[name]
    n = 8
    eng, bare, nohead = make_engine(name), make_engine(name, bind=False), make_engine("nohead")
    xs = [torch.full((n, w), -7.25, device=DEV) for w in c["sizes"]]
    out = torch.full((n, c["n_out"]), -7.25, device=DEV)
    x7 = [torch.full((n, 7), -7.25, device=DEV)]
    EINVAL, ESTATE = -1, -4
    cases = [
        ("null engine", EINVAL, dict(eng=eng, handle=None, x=xs, out=out)),
        ("n < 0", EINVAL, dict(eng=eng, n=-1, x=xs, out=out)),
        ("sample_base + n > 2^32", EINVAL, dict(eng=eng, x=xs, out=out, base=(1 << 32) - n + 1)),
        ("sample_base > 2^32", EINVAL, dict(eng=eng, x=xs, out=out, base=(1 << 63))),
        ("max_rows < 0", EINVAL, dict(eng=eng, x=xs, out=out, max_rows=-1)),
        ("unknown readout", EINVAL, dict(eng=eng, x=xs, out=out, readout=3)),
        ("unknown loss_kind", EINVAL, dict(eng=eng, x=xs, out=out, loss=7)),
        ("out without a read-out", EINVAL, dict(eng=nohead, x=x7, out=out)),
        ("nothing wanted (x_out null)", EINVAL, dict(eng=eng, x=None, out=None)),
        ("nothing wanted (every entry null)", EINVAL, dict(eng=eng, x=[None] * 3, out=None)),
        ("MEAN without a loss", EINVAL, dict(eng=eng, x=xs, out=out, readout=_lib.SAMPLE_MEAN)),
        ("DRAW without a loss", EINVAL, dict(eng=eng, x=xs, out=out, readout=_lib.SAMPLE_DRAW)),
        ("Gaussian DRAW, var = 0", EINVAL, dict(eng=eng, x=xs, out=out, readout=_lib.SAMPLE_DRAW, loss=_lib.LOSS_GAUSSIAN, var=0.0)),
        ("Gaussian DRAW, var < 0", EINVAL, dict(eng=eng, x=xs, out=out, readout=_lib.SAMPLE_DRAW, loss=_lib.LOSS_GAUSSIAN, var=-1.0)),
        ("Gaussian DRAW, var NaN", EINVAL, dict(eng=eng, x=xs, out=out, readout=_lib.SAMPLE_DRAW, loss=_lib.LOSS_GAUSSIAN, var=float("nan"))),
        ("parameters not bound", ESTATE, dict(eng=bare, x=xs, out=out)),
    ]
    for what, code, kw in cases:
        e = kw.pop("eng")
        rc = raw_call(e, kw.pop("n", n), kw.pop("x"), kw.pop("out"), **kw)
        assert rc == code and e._lib.mcpc_last_error(), (what, rc, e._lib.mcpc_last_error())
    # an ecoef <= 0 never reaches the call: mcpc_create refuses the engine
    with pytest.raises(_lib.MCPCError, match="ecoef"):
        Engine([7], [0], 2, 0, 64, device=torch.device(DEV), ecoef=[0.0])
    assert raw_call(eng, 0, xs, out) == 0                      # n = 0 launches nothing either
    torch.cuda.synchronize()
    for t in (*xs, out, *x7):
        assert bool((t == -7.25).all())
    for e in (eng, bare, nohead):
        e.close()


# ---- 6. the Python fronts -------------------------------------------------------------------------------------------------------
def test_sample_pc_device_on_a_cpu_built_and_a_gpu_built_model():
    from montecarlopredictivecoding_amd.utils import training_evaluation as te
    from tests.test_evaluators_golden import load_eval_fixture
    for loss in ("bernoulli", "gaussian"):
        _, _, cfg, on_gpu, _ = load_eval_fixture(loss, device=DEV)
        _, _, _, on_cpu, _ = load_eval_fixture(loss)
        got = {}
        for where, model in (("gpu", on_gpu), ("cpu", on_cpu)):
            h, xs = te.sample_pc_device(100, model, cfg, is_return_hidden=True, seed=5, step=2, sample_base=40, return_latents=True)
            d = te.sample_pc_device(100, model, cfg, seed=5, step=2, sample_base=40)
            want_dev = next(model.parameters()).device
            assert all(t.device == want_dev and t.dtype == torch.float32 for t in (h, d, *xs))
            got[where] = (h, d, *xs)
        for k, (a, b) in enumerate(zip(got["gpu"], got["cpu"])):
            same(a, b, f"{loss}: CPU-built against GPU-built, tensor {k}")
        h, d = got["gpu"][:2]
        if loss == "bernoulli":
            assert set(np.unique(d.cpu().numpy())) == {0.0, 1.0}
        else:
            assert not torch.equal(h, d) and float((d - h).std()) == pytest.approx(cfg["input_var"] ** 0.5, rel=0.05)
        # the same ids through another split
        same(torch.cat([te.sample_pc_device(n, on_gpu, cfg, is_return_hidden=True, seed=5, step=2, sample_base=40 + s) for s, n in ((0, 33), (33, 67))]),
             h, f"{loss}: 33 + 67 samples")


def test_marginal_likelihood_with_the_device_sampler():
    from montecarlopredictivecoding_amd.likelihood import log_likelihood
    from montecarlopredictivecoding_amd.utils import training_evaluation as te
    from tests.test_evaluators_golden import load_eval_fixture
    z, meta, cfg, model, loader = load_eval_fixture("bernoulli", device=DEV)
    S = 120
    data = torch.from_numpy(z["data"]).to(DEV).to(torch.float32).reshape(z["data"].shape[0], -1)
    hidden = te.sample_pc_device(S, model, cfg, is_return_hidden=True, seed=3)
    one = te.get_marginal_likelihood_per_datum(model, cfg, loader, True, n_samples=S, sampler="device", seed=3)
    assert torch.equal(one.state, log_likelihood(data, hidden, loss="bernoulli").state)
    y, o = data.cpu().numpy(), hidden.cpu().numpy()
    want, tol = R.ref_state(y, o, "bernoulli", None, 20.0), R.tol(y, o, "bernoulli", None, 20.0)
    R.assert_state_close(one.state.cpu().numpy(), want, tol, "the device sampler, one chunk")
    for chunk in (1, 17):
        got = te.get_marginal_likelihood_per_datum(model, cfg, loader, True, n_samples=S, sample_chunk=chunk, sampler="device", seed=3)
        R.assert_state_close(got.state.cpu().numpy(), want, tol, f"the device sampler, sample_chunk={chunk}")
    # the default sampler is the torch stream it always was: the loop of the evaluator before it had a choice
    torch.manual_seed(meta["torch_seed"])
    default = te.get_marginal_likelihood_per_datum(model, cfg, loader, True, n_samples=S, sample_chunk=50)
    torch.manual_seed(meta["torch_seed"])
    state = None
    for s0 in range(0, S, 50):
        outputs = te.sample_pc(min(50, S - s0), model, cfg, use_cuda=True, is_return_hidden=True)
        if s0 == 0:
            rows = torch.cat([d.to(DEV).to(torch.float32).reshape(d.shape[0], -1) for d, _ in loader])
        state = log_likelihood(rows, outputs, loss="bernoulli", var=None, clamp=20.0, state=state)
    assert torch.equal(default.state, state.state)
    assert not torch.equal(default.state, one.state)


# ---- 7. the distribution ----------------------------------------------------------------------------------------------------------
DIST_SEED, DIST_N = 20261020, 65536


def dist_params():
    rng = np.random.default_rng(5)
    dims = [2, 3, 4, 5]
    W = [rng.standard_normal((o, i)).astype(np.float32) for i, o in zip(dims[:-1], dims[1:])]
    b = [rng.standard_normal(o).astype(np.float32) for o in dims[1:]]
    return W, b


def dist_analytic():
    """Mean and per-unit variance of the read-out of the identity 2-3-4-5 net with zero input: x_0 = b_0 + z_0, x_1 = W_1 x_0 + b_1 + z_1,
    o = W_2 x_1 + b_2, so o ~ N(W_2 (W_1 b_0 + b_1) + b_2, W_2 (W_1 W_1^T + I) W_2^T)."""
    W, b = ([a.astype(np.float64) for a in p] for p in dist_params())
    mean = W[2] @ (W[1] @ b[0] + b[1]) + b[2]
    cov = W[2] @ (W[1] @ W[1].T + np.eye(4)) @ W[2].T
    return mean, np.diag(cov)


def dist_check(o, slack_mean=0.0, slack_var=0.0):
    mean, var = dist_analytic()
    n = o.shape[0]
    o = np.asarray(o, np.float64)
    dm, dv = np.abs(o.mean(0) - mean), np.abs(o.var(0) - var)
    bm, bv = 6.0 * np.sqrt(var / n) + slack_mean, 6.0 * var * np.sqrt(2.0 / n) + slack_var
    print("mean: %.3f of the bound; variance: %.3f of the bound" % ((dm / bm).max(), (dv / bv).max()))
    assert (dm <= bm).all() and (dv <= bv).all()


def test_the_read_out_has_the_analytic_mean_and_variance():
    from montecarlopredictivecoding_amd.engine import Engine
    W, b = dist_params()
    eng = Engine([3, 4], [0, 0], 2, 5, 64, device=torch.device(DEV))
    eng.bind_params([torch.tensor(w).to(DEV) for w in W], [torch.tensor(v).to(DEV) for v in b])
    out, xs = eng.sample_prior(DIST_N, DIST_SEED, latents=(1,))
    eng.sync_check()
    # the fp32 prediction bound of the read-out, 1e-6 S_u, moves a sample by that much: the mean by its average, the variance by 2 sigma of it
    S = (np.abs(xs[1].cpu().numpy().astype(np.float64)) @ np.abs(W[2].astype(np.float64)).T + np.abs(b[2])).mean(0)
    dist_check(out.cpu().numpy(), 1e-6 * S, 2.0 * np.sqrt(dist_analytic()[1]) * 1e-6 * S)
    eng.close()

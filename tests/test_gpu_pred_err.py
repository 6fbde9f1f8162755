"""Prediction errors and predictions per unit through the C ABI (include/mcpc.h: mcpc_prediction_errors): against the fp64 oracle one
chain at a time, bitwise invariance under everything that regroups rows or requests, no store outside what was asked for, consistency
with mcpc_chain_energies and mcpc_run's rec_out, and the argument checks.

The bounds follow from the project's stated GEMM bound (tests/test_gpu_accuracy.py, restated in tests/chain_energy_cases.py): a
prediction mu_u = sum_k a_k W_uk + b_u is off by at most 1e-6 * S_u, S_u = sum_k |a_k W_uk| + |b_u|.  Hence
    |pred - want| <= 1e-6 * S_u,      |err - want| <= 1e-6 * (S_u + |d_u|)      (the subtraction's own rounding: half an ulp of d),
    |err_out - want| <= 1e-6 * (g * S_u + |e_u|),  g = |de / do| <= 1 / var (Gaussian) or 1 / 4 (Bernoulli: sigmoid' <= 1 / 4),
and err_out is exactly 0 under the mask."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import mcpc_oracle as mo
from tests import chain_energy_cases as cc
from tests import parity_log

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = -7.25                       # what the destinations hold before a call


def _engine(name, chains=None, ecoef=None):
    from montecarlopredictivecoding_amd.engine import Engine
    c, d = cc.NETS[name], cc.data(name)
    B = c["B"] if chains is None else chains
    L = len(c["sizes"])
    eng = Engine(list(c["sizes"]), [c["act"]] * L, c["n_in"], c["n_out"], B, device=torch.device(DEV), ecoef=ecoef)
    eng.bind_params([torch.tensor(w).to(DEV) for w in d["W"]], [torch.tensor(v).to(DEV) for v in d["b"]])
    if d["target"] is not None:
        eng.bind_target(torch.tensor(d["target"][:B]).to(DEV).contiguous())
    inputs = torch.tensor(d["inputs"][:B]).to(DEV).contiguous() if c["inputs"] else None
    xs = [torch.tensor(x[:, :B]).to(DEV).contiguous() for x in d["xs"]]
    return eng, inputs, xs


def _kw(name):
    c = cc.NETS[name]
    both = "both" if c["n_out"] else None
    return dict(quantity="both", outputs=both if c["loss"] != mo.LOSS_NONE else ("prediction" if c["n_out"] else None),
                loss_kind=c["loss"], loss_var=c["var"], mask_start=c["mask_start"])


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _same(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), f"{what}: {k}"


@functools.lru_cache(maxsize=None)
def reference(name):
    """fp64, one chain at a time: {block name: (want, bound)} of the case's recorded states, each [N_REC, B, n]; never modified."""
    c, d = cc.NETS[name], cc.data(name)
    L = len(c["sizes"])
    f64 = lambda a: None if a is None else np.asarray(a, np.float64)
    W, b = [f64(w) for w in d["W"]], [f64(v) for v in d["b"]]
    net = mo.NetSpec(sizes=list(c["sizes"]), acts=[c["act"]] * L, W=W, b=b, ecoef=[1.0] * L, has_head=c["n_out"] > 0)
    inputs, target, xs = f64(d["inputs"]), f64(d["target"]), [f64(x) for x in d["xs"]]
    n, B = cc.N_REC, c["B"]
    out = {}
    for l in range(L):
        for q in ("e", "mu"):
            out[f"{q}{l}"] = (np.zeros((n, B, c["sizes"][l])), np.zeros((n, B, c["sizes"][l])))
    if c["n_out"]:
        out["out"] = (np.zeros((n, B, c["n_out"])), np.zeros((n, B, c["n_out"])))
        if c["loss"] != mo.LOSS_NONE:
            out["eout"] = (np.zeros((n, B, c["n_out"])), np.zeros((n, B, c["n_out"])))
    g = 1.0 / c["var"] if c["loss"] == mo.LOSS_GAUSSIAN else 0.25
    for k in range(n):
        for ch in range(B):
            loss = mo.LossSpec(c["loss"], None if target is None else target[ch:ch + 1], c["var"], c["mask_start"])
            fw = mo.forward(net, inputs[ch:ch + 1], [x[k, ch:ch + 1] for x in xs], loss)
            for l in range(L):
                S = (np.abs(fw["acts_in"][l]) @ np.abs(W[l]).T + np.abs(b[l]))[0]
                dd = fw["errs"][l][0]                                   # ecoef = 1: the error is d itself
                out[f"e{l}"][0][k, ch], out[f"e{l}"][1][k, ch] = dd, 1e-6 * (S + np.abs(dd))
                out[f"mu{l}"][0][k, ch], out[f"mu{l}"][1][k, ch] = xs[l][k, ch] - dd, 1e-6 * S
            if c["n_out"]:
                S = (np.abs(fw["acts_in"][L]) @ np.abs(W[L]).T + np.abs(b[L]))[0]
                out["out"][0][k, ch], out["out"][1][k, ch] = fw["out"][0], 1e-6 * S
                if "eout" in out:
                    e = fw["e_out"][0]
                    out["eout"][0][k, ch], out["eout"][1][k, ch] = e, 1e-6 * (g * S + np.abs(e))
    for w_, b_ in out.values():
        w_.setflags(write=False)
        b_.setflags(write=False)
    return out


def _against_bound(group, got, ref):
    for name in sorted(ref):
        want, bound = ref[name]
        v = got[name].cpu().numpy().astype(np.float64)
        assert v.shape == want.shape and np.isfinite(v).all(), name
        bnd = np.maximum(bound, 1e-300)
        frac = float(np.max(np.abs(v - want) / bnd))
        print(f"{group}: {name}: achieved {frac:.3f} of the bound")
        parity_log.close(group, name + " / bound", v / bnd, want / bnd, rtol=0.0, atol=1.0)


# ---- 1. against the oracle, per chain --------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cc.NETS))
def test_values_match_the_oracle_chain_by_chain(name):
    c = cc.NETS[name]
    eng, inputs, xs = _engine(name)
    got = eng.prediction_errors(inputs, xs, **_kw(name))
    eng.sync_check()
    ref = reference(name)
    assert sorted(got) == sorted(ref)
    _against_bound(f"mcpc_prediction_errors vs oracle per chain ({name})", got, ref)
    if "eout" in got and c["mask_start"] > 0:
        assert (_bits(got["eout"][..., :c["mask_start"]]) == 0).all(), "the read-out error under the mask is exactly +0"
        assert (got["eout"][..., c["mask_start"]:] != 0).any()
    eng.close()


def test_err_is_not_scaled_by_ecoef():
    """ecoef = (0.5, 2, 0.25): err stays x - mu and pred stays mu (against the same oracle values as with ecoef = 1), bit for bit the
    ecoef = 1 engine's; the chain energies of the same engine carry the coefficient."""
    name = "relu_bern_mask"
    co = (0.5, 2.0, 0.25)
    eng, inputs, xs = _engine(name, ecoef=co)
    got = eng.prediction_errors(inputs, xs, **_kw(name))
    table = eng.chain_energies(inputs, xs, loss_kind=cc.NETS[name]["loss"], mask_start=cc.NETS[name]["mask_start"]).cpu().numpy()
    eng.sync_check()
    _against_bound(f"mcpc_prediction_errors vs oracle per chain ({name}, ecoef={co})", got, reference(name))
    one, inputs1, xs1 = _engine(name)
    _same(got, one.prediction_errors(inputs1, xs1, **_kw(name)), "ecoef != 1 against ecoef = 1")
    for l, c_ in enumerate(co):
        e = got[f"e{l}"].cpu().numpy().astype(np.float64)
        n_l = cc.NETS[name]["sizes"][l]
        np.testing.assert_allclose(0.5 * c_ * (e * e).sum(axis=-1), table[..., 1 + l], rtol=(16 * -(-n_l // 16) + 4) * 2.0 ** -24, atol=0.0)
    one.close()
    eng.close()


# ---- 2. bitwise -------------------------------------------------------------------------------------------------
def test_values_do_not_depend_on_how_they_are_grouped_or_asked_for():
    name = "relu_bern_mask"
    eng, inputs, xs = _engine(name)
    kw = _kw(name)
    one = eng.prediction_errors(inputs, xs, **kw)
    _same(one, eng.prediction_errors(inputs, xs, **kw), "a repeated call")
    _same(one, eng.prediction_errors(inputs, xs, max_rows=64, **kw), "max_rows=64 against the default")     # 210 rows: four chunks
    _same(one, eng.prediction_errors(inputs, xs, max_rows=1 << 20, **kw), "max_rows larger than the call")
    parts = [eng.prediction_errors(inputs, [x[k] for x in xs], **kw) for k in range(cc.N_REC)]
    _same(one, {k: torch.cat([p[k] for p in parts]) for k in one}, "n_rec = 3 in one call against three calls")
    eng16, inputs16, xs16 = _engine(name, chains=16)
    few = eng16.prediction_errors(inputs16, xs16, **kw)
    _same({k: v[:, :16] for k, v in one.items()}, few, "the first 16 chains alone")
    eng16.close()
    # one layer asked alone (its own job table; only the records it reads are passed) against all asked together
    for l in range(3):
        recs = [x if j in (l, l - 1) else None for j, x in enumerate(xs)]
        for q, key in (("error", f"e{l}"), ("prediction", f"mu{l}")):
            alone = eng.prediction_errors(inputs, recs, layers=(l,), quantity=q)
            _same({key: one[key]}, alone, f"layer {l} {q} alone")
    head = eng.prediction_errors(None, [None, None, xs[2]], layers=(), outputs="prediction")
    _same({"out": one["out"]}, head, "the read-out prediction alone")
    head = eng.prediction_errors(None, [None, None, xs[2]], layers=(), outputs="error", **{k: kw[k] for k in ("loss_kind", "loss_var", "mask_start")})
    _same({"eout": one["eout"]}, head, "the read-out error alone")
    eng.close()


def test_a_destination_that_is_only_4_byte_aligned_gets_the_same_bits():
    """n_l % 4 == 0 with a base off the 16-byte grid takes the per-element stores (tanh_gauss: widths 16, 16, 24)."""
    name = "tanh_gauss"
    c = cc.NETS[name]
    eng, inputs, xs = _engine(name)
    kw = _kw(name)
    one = eng.prediction_errors(inputs, xs, **kw)
    out, flats = {}, {}
    for k, v in one.items():
        flats[k] = torch.full((v.numel() + 2,), FILL, dtype=torch.float32, device=DEV)
        out[k] = flats[k][1:1 + v.numel()].view(v.shape)
        assert out[k].data_ptr() % 16 == 4
    off = eng.prediction_errors(inputs, xs, out=out, **kw)
    eng.sync_check()
    _same(one, off, "a 4-byte aligned destination")
    for k, f in flats.items():
        assert f[0].item() == FILL and f[-1].item() == FILL, k
    assert c["sizes"][1] % 4 == 0
    eng.close()


# ---- 3. no stray stores ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["relu_bern_mask", "mu1_only"])
def test_no_store_lands_outside_what_was_asked_for(name):
    c = cc.NETS[name]
    eng, inputs, xs = _engine(name)
    kw = _kw(name)
    L = len(c["sizes"])
    widths = {f"{q}{l}": c["sizes"][l] for l in range(L) for q in ("e", "mu")}
    if c["n_out"]:
        widths.update(eout=c["n_out"], out=c["n_out"])
    # a guard record before and after every destination, and two records more than the call fills
    big = {k: torch.full((cc.N_REC + 2, c["B"], w), FILL, dtype=torch.float32, device=DEV) for k, w in widths.items()}
    asked = ["e0"] if L == 1 else ["e1", "mu2", "eout"]
    layers_e = [int(k[1:]) for k in asked if k[0] == "e" and k != "eout"]
    layers_mu = [int(k[2:]) for k in asked if k.startswith("mu")]
    n_fill = cc.N_REC - 1                                               # records 1 .. n_fill of `big` are the destination
    recs = [x[:n_fill] for x in xs]
    # through the C ABI with every pointer in place: layers not asked for are NULL in err / pred
    lib = eng._lib
    err, pred = (C.c_void_p * L)(), (C.c_void_p * L)()
    for l in layers_e:
        err[l] = big[f"e{l}"][1:].data_ptr()
    for l in layers_mu:
        pred[l] = big[f"mu{l}"][1:].data_ptr()
    eout = big["eout"][1:].data_ptr() if "eout" in asked else None
    arr = (C.c_void_p * L)(*[r.data_ptr() for r in recs])
    stream = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    code = lib.mcpc_prediction_errors(eng._h, C.c_void_p(inputs.data_ptr()) if inputs is not None else None, arr, n_fill, kw["loss_kind"],
                                      kw["loss_var"], kw["mask_start"], err, pred, eout, None, 64, stream)
    assert code == 0, lib.mcpc_last_error().decode()
    eng.sync_check()
    fill_bits = np.float32(FILL).view(np.int32)
    want = eng.prediction_errors(inputs, recs, **kw)
    for k, t in big.items():
        bits = _bits(t)
        if k in asked:
            assert (bits[0] == fill_bits).all(), f"{k}: the guard record before"
            assert (bits[1 + n_fill:] == fill_bits).all(), f"{k}: the records beyond n_rec"
            assert np.array_equal(bits[1:1 + n_fill], _bits(want[k])), k
        else:
            assert (bits == fill_bits).all(), f"{k} was not asked for"
    eng.close()


# ---- 4. consistency with what exists --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cc.NETS))
def test_squared_errors_sum_to_the_chain_energies(name):
    """0.5 c sum_u err^2 in fp64 against the E_l column of mcpc_chain_energies on the same rows: the same d values, summed there in
    fp32 over npad_l units (at most npad_l + 4 roundings of relative size 2^-24, all terms non-negative)."""
    c = cc.NETS[name]
    eng, inputs, xs = _engine(name)
    got = eng.prediction_errors(inputs, xs, quantity="error")
    table = eng.chain_energies(inputs, xs).cpu().numpy()
    eng.sync_check()
    for l, n_l in enumerate(c["sizes"]):
        e = got[f"e{l}"].cpu().numpy().astype(np.float64)
        mine = 0.5 * (e * e).sum(axis=-1)
        npad = 16 * -(-n_l // 16)
        parity_log.close(f"sum of squared mcpc_prediction_errors vs mcpc_chain_energies ({name})", f"E_{l + 1}", mine, table[..., 1 + l],
                         rtol=(npad + 4) * 2.0 ** -24, atol=0.0)
    eng.close()


def test_read_out_prediction_of_recorded_states_against_rec_out():
    """The read-out prediction of the states mcpc_run recorded against that run's rec_out for the same records, within the bound of
    (1).  Whether it also holds bit for bit is reported (and recorded in DESIGN.md), not asserted."""
    from montecarlopredictivecoding_amd import _lib as L_
    name, T = "relu_bern_mask", 5
    c, d = cc.NETS[name], cc.data(name)
    eng, inputs, xs = _engine(name)
    eng.bind_inputs(inputs)
    eng.load_state([x[0].contiguous() for x in xs])
    res = eng.run(T, loss_kind=c["loss"], mask_start=c["mask_start"], xopt=L_.XOPT_SGD, lr=0.02, noise_mode=L_.NOISE_PHILOX, noise_var=2.0,
                  seed=9, step_base=0, energy_mode=L_.ENERGY_NONE, rec_count=T, rec_x=True, rec_out=True)
    got = eng.prediction_errors(None, [None, None, res.rec_x[2]], layers=(), outputs="prediction")["out"]
    eng.sync_check()
    a = torch.relu(res.rec_x[2].double()).cpu().numpy()
    W, b = np.asarray(d["W"][3], np.float64), np.asarray(d["b"][3], np.float64)
    S = np.abs(a) @ np.abs(W).T + np.abs(b)
    rec_out = res.rec_out.cpu().numpy().astype(np.float64)
    same = np.array_equal(_bits(got), _bits(res.rec_out))
    print(f"read-out prediction of recorded states vs rec_out: bitwise equal = {same}")
    parity_log.close("mcpc_prediction_errors pred_out vs mcpc_run rec_out", "out / bound", got.cpu().numpy() / (1e-6 * S), rec_out / (1e-6 * S),
                     rtol=0.0, atol=1.0)
    eng.close()


# ---- 5. bad arguments ----------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch():
    from montecarlopredictivecoding_amd import _lib as L_
    from montecarlopredictivecoding_amd.engine import Engine
    lib = L_.load()
    name = "relu_bern_mask"
    c, d = cc.NETS[name], cc.data(name)
    eng, inputs, xs = _engine(name)
    dst = [torch.full((cc.N_REC, c["B"], n), FILL, dtype=torch.float32, device=DEV) for n in c["sizes"]]
    dst_o = torch.full((cc.N_REC, c["B"], c["n_out"]), FILL, dtype=torch.float32, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    arr = (C.c_void_p * 3)(*[x.data_ptr() for x in xs])
    hole = (C.c_void_p * 3)(xs[0].data_ptr(), None, xs[2].data_ptr())
    err = (C.c_void_p * 3)(*[t.data_ptr() for t in dst])
    none = (C.c_void_p * 3)()
    base = dict(e=eng._h, inputs=C.c_void_p(inputs.data_ptr()), x=arr, n_rec=cc.N_REC, kind=c["loss"], var=1.0, mask=c["mask_start"],
                err=err, pred=None, eo=C.c_void_p(dst_o.data_ptr()), po=None, max_rows=0)

    def call(**kw):
        a = dict(base, **kw)
        code = lib.mcpc_prediction_errors(a["e"], a["inputs"], a["x"], a["n_rec"], a["kind"], a["var"], a["mask"], a["err"], a["pred"],
                                          a["eo"], a["po"], a["max_rows"], stream)
        return code, lib.mcpc_last_error().decode()

    EINVAL, ESTATE = -1, -4
    for kw, code, word in ((dict(e=None), EINVAL, "null engine"), (dict(x=None), EINVAL, "x_rec is null"), (dict(x=hole), EINVAL, "x_rec[1] is null"),
                           (dict(n_rec=-1), EINVAL, "n_rec=-1"), (dict(max_rows=-1), EINVAL, "max_rows=-1"),
                           (dict(err=None, eo=None), EINVAL, "nothing is asked for"), (dict(err=none, pred=none, eo=None), EINVAL, "nothing is asked for"),
                           (dict(kind=3), EINVAL, "loss_kind=3"), (dict(kind=L_.LOSS_NONE), EINVAL, "err_out needs a loss"),
                           (dict(mask=-1), EINVAL, "mask_start=-1"), (dict(mask=40), EINVAL, "mask_start=40"),
                           (dict(kind=L_.LOSS_GAUSSIAN, var=0.0), EINVAL, "loss_var must be positive")):
        got, msg = call(**kw)
        assert got == code and word in msg, (kw, got, msg)
    bare = Engine(list(c["sizes"]), [c["act"]] * 3, c["n_in"], c["n_out"], c["B"], device=torch.device(DEV))
    got, msg = call(e=bare._h)
    assert got == ESTATE and "no bound parameters" in msg, (got, msg)
    bare.bind_params([torch.tensor(w).to(DEV) for w in d["W"]], [torch.tensor(v).to(DEV) for v in d["b"]])
    got, msg = call(e=bare._h)
    assert got == ESTATE and "no target bound" in msg, (got, msg)
    headless, _, hx = _engine("mu1_only")
    for kw in (dict(eo=C.c_void_p(dst_o.data_ptr())), dict(eo=None, po=C.c_void_p(dst_o.data_ptr()))):
        got, msg = call(e=headless._h, x=(C.c_void_p * 1)(hx[0].data_ptr()), err=None, **kw)
        assert got == EINVAL and "need a read-out" in msg, (got, msg)
    torch.cuda.synchronize()
    assert all((t == FILL).all() for t in dst + [dst_o]), "a refused call wrote into a destination"
    assert call(n_rec=0)[0] == 0                                       # n_rec = 0 is a call that does nothing
    torch.cuda.synchronize()
    assert all((t == FILL).all() for t in dst + [dst_o])
    for e_ in (eng, bare, headless):
        e_.close()

"""Gradients and energies of handed-over states through the C ABI (include/mcpc.h: mcpc_state_gradients): bit for bit against the
layer-wise step kernels and mcpc_chain_energies, against the fp64 oracle one chain at a time, bitwise invariance under everything that
regroups rows, guard rows around every destination, special values, poisoned LDS, an untouched engine, a side stream, refusals."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import parity_log
from tests import state_grad_cases as sg
from tests import stream_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = sorted(sg.NETS)


def _engine(name, tuning=None, data=None):
    """An engine for the case with parameters and target bound, the inputs to pass and the states."""
    from montecarlopredictivecoding_amd import _lib
    from montecarlopredictivecoding_amd.engine import Engine
    c, d = sg.NETS[name], sg.data(name) if data is None else data
    L = len(c["sizes"])
    make = lambda t: Engine(list(c["sizes"]), [c["act"]] * L, c["n_in"], c["n_out"], c["B"], device=torch.device(DEV), ecoef=sg.ecoef(name), tuning=t)
    try:
        eng = make(tuning)
    except _lib.MCPCError as exc:                              # no LDS plan holds the net (wide_under_small): the layer-wise
        if tuning is not None or exc.code != -3:               # kernels are its default form, as for PCTrainer
            raise
        eng = make("wide=1")
    eng.bind_params([torch.tensor(w).to(DEV) for w in d["W"]], [torch.tensor(v).to(DEV) for v in d["b"]])
    if d["target"] is not None:
        eng.bind_target(torch.tensor(d["target"]).to(DEV).contiguous())
    inputs = torch.tensor(d["inputs"]).to(DEV).contiguous() if c["inputs"] else None
    xs = [torch.tensor(x).to(DEV).contiguous() for x in d["xs"]]
    return eng, inputs, xs


def _kw(name):
    c = sg.NETS[name]
    return dict(loss_kind=c["loss"], loss_var=c["var"], mask_start=c["mask_start"])


def _bits(t):
    a = t.detach().cpu().numpy()
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def _same(a, b):
    return all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(a, b))


def _step_xgrad(name, tuning):
    """xgrad of run(1, update_x=False) after load_state, per state: lists over the layers of [N_REC, B, n_l] (host), the kernel's name"""
    eng, inputs, xs = _engine(name, tuning)
    eng.bind_inputs(inputs)
    per = []
    for k in range(sg.N_REC):
        eng.load_state([x[k].contiguous() for x in xs])
        per.append([g.cpu().numpy() for g in eng.run(1, update_x=False, **_kw(name)).xgrad])
    kernel = eng.last_step_kernel()
    eng.sync_check()
    eng.close()
    return [np.stack([per[k][l] for k in range(sg.N_REC)]) for l in range(len(xs))], kernel


@functools.lru_cache(maxsize=None)
def _got(name):
    """One call of the case on a default engine, energies asked for: (grads, table) on the host, computed once and never modified"""
    eng, inputs, xs = _engine(name)
    grads, table = eng.state_gradients(inputs, xs, energies=True, **_kw(name))
    energies = eng.chain_energies(inputs, xs, **_kw(name))
    eng.sync_check()
    out = [g.cpu().numpy() for g in grads], table.cpu().numpy(), energies.cpu().numpy()
    eng.close()
    return out


# ---- 1. the layer-wise step kernels and mcpc_chain_energies, bit for bit -------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_gradients_are_the_layerwise_step_kernels_and_energies_the_chain_energies(name):
    want, kernel = _step_xgrad(name, "ws=4")
    assert "lw" in kernel, kernel
    grads, table, energies = _got(name)
    c = sg.NETS[name]
    for l, (g, w) in enumerate(zip(grads, want)):
        assert g.shape == (sg.N_REC, c["B"], c["sizes"][l]) and g.dtype == np.float32
        assert np.isfinite(g).all() and np.abs(g).max() > 0
        assert np.array_equal(g.view(np.int32), w.view(np.int32)), f"grad[{l}] against xgrad of {kernel}"
    assert table.shape == (sg.N_REC, c["B"], 8) and np.array_equal(table.view(np.int64), energies.view(np.int64))
    assert (table[..., -1] > 0).all()


# ---- 2. fp64, one chain at a time -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_gradients_meet_the_bound_against_fp64(name):
    want, bound = sg.reference(name)
    sg.log_against_bound(parity_log, f"mcpc_state_gradients vs oracle per chain ({name})", _got(name)[0], want, bound)


# ---- 3. the default step kernel of the case's engine -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_gradients_against_the_default_step_kernel(name):
    step, kernel = _step_xgrad(name, None)
    grads = _got(name)[0]
    bitwise = all(np.array_equal(g.view(np.int32), s.view(np.int32)) for g, s in zip(grads, step))
    print(f"{name}: default step kernel {kernel}: bitwise equal to mcpc_state_gradients: {bitwise}")
    if sg.NETS[name]["n_out"] == 0:
        assert bitwise, kernel
    else:
        want, bound = sg.reference(name)
        sg.log_against_bound(parity_log, f"xgrad of the default step kernel vs oracle per chain ({name}, {kernel})", step, want, bound)


# ---- 4. invariance, bitwise ---------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_grouping_or_on_what_else_is_asked():
    name = "relu_bern_mask"
    eng, inputs, xs = _engine(name)
    kw = _kw(name)
    one, table = eng.state_gradients(inputs, xs, energies=True, **kw)
    for rows in (64, 128):                                     # 210 rows: four and two chunks, none but the first starting at chain 0
        g, t = eng.state_gradients(inputs, xs, energies=True, max_rows=rows, **kw)
        assert _same(one, g) and _same([table], [t]), f"max_rows={rows} against the default"
    parts = [eng.state_gradients(inputs, [x[k] for x in xs], energies=True, **kw) for k in range(sg.N_REC)]
    assert _same(one, [torch.cat([p[0][l] for p in parts]) for l in range(len(xs))]), "three states in one call against one call each"
    assert _same([table], [torch.cat([p[1] for p in parts])])
    bare, none = eng.state_gradients(inputs, xs, **kw)
    assert none is None and _same(one, bare), "energies asked for against not asked for"
    # chain 7 of every state among other neighbours
    rs = np.random.RandomState(5)
    other = [torch.tensor(rs.randn(*x.shape).astype(np.float32)).to(DEV) for x in xs]
    for o, x in zip(other, xs):
        o[:, 7] = x[:, 7]
    g, t = eng.state_gradients(inputs, other, energies=True, **kw)
    assert _same([a[:, 7] for a in one], [a[:, 7] for a in g]) and _same([table[:, 7]], [t[:, 7]]), "a row among other rows"
    assert not _same([a[:, 8] for a in one], [a[:, 8] for a in g])
    eng.sync_check()
    eng.close()


# ---- 5. guard rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,offset", [("relu_bern_mask", 0), ("relu_bern_mask", 1), ("mu1_only", 0), ("wide_under_small", 0),
                                         ("wide_under_small", 1), ("ident_nohead", 0)])
def test_nothing_is_stored_outside_the_destination(name, offset):
    """Widths 200 / 784 / 40 / 24 / 12 take the 16-byte path at offset 0 and the per-element path 4 bytes further on; 33, 17 and 37 always
    take the per-element path."""
    MARGIN, MARK = 1024, -7.25
    eng, inputs, xs = _engine(name)
    want = _got(name)[0]
    c = sg.NETS[name]
    bufs, outs = [], []
    for n in c["sizes"]:
        size = sg.N_REC * c["B"] * n
        buf = torch.full((MARGIN + offset + size + MARGIN,), MARK, dtype=torch.float32, device=DEV)
        assert buf.data_ptr() % 16 == 0
        bufs.append(buf)
        outs.append(buf[MARGIN + offset:MARGIN + offset + size].view(sg.N_REC, c["B"], n))
    table = torch.full((sg.N_REC + 2, c["B"], 8), MARK, dtype=torch.float64, device=DEV)
    eng.state_gradients(inputs, xs, out=outs, energies_out=table[1:-1], max_rows=64, **_kw(name))
    eng.sync_check()
    for l, (buf, o) in enumerate(zip(bufs, outs)):
        assert np.array_equal(_bits(o), want[l].view(np.int32)), f"grad[{l}]"
        assert (buf[:MARGIN + offset] == MARK).all() and (buf[MARGIN + offset + o.numel():] == MARK).all(), f"around grad[{l}]"
    assert (table[0] == MARK).all() and (table[-1] == MARK).all()
    assert np.array_equal(_bits(table[1:-1]), _got(name)[1].view(np.int64))
    eng.close()


# ---- 6. special values stay in their row ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["relu_bern_mask", "six_tanh"])
def test_special_values_stay_in_their_chain(name):
    eng, inputs, xs = _engine(name)
    CH = 21                                                    # inside a chain tile, not its first row
    special = [x.clone() for x in xs]
    for l, x in enumerate(special):
        x[0, CH, 0] = float("nan")
        x[1, CH, l % x.shape[2]] = float("inf")
        x[2, CH, -1] = 3.4e38
    g, t = eng.state_gradients(inputs, special, energies=True, **_kw(name))
    eng.sync_check()
    want, table = _got(name)[0], _got(name)[1]
    keep = np.arange(sg.NETS[name]["B"]) != CH
    for l in range(len(xs)):
        assert np.array_equal(_bits(g[l])[:, keep], want[l].view(np.int32)[:, keep]), f"grad[{l}] of the other chains"
        assert not np.isfinite(g[l][0, CH].cpu().numpy()).all()
    assert np.array_equal(_bits(t)[:, keep], table.view(np.int64)[:, keep])
    eng.close()


# ---- 7. LDS content does not matter -----------------------------------------------------------------------------------------------------
def test_poisoned_lds_changes_nothing():
    from montecarlopredictivecoding_amd.engine import debug_poison_lds
    name = "relu_bern_wide"
    eng, inputs, xs = _engine(name)
    eng.state_gradients(inputs, xs, energies=True, **_kw(name))                  # (the scratch exists: nothing else runs in between)
    debug_poison_lds(DEV)
    g, t = eng.state_gradients(inputs, xs, energies=True, **_kw(name))
    eng.sync_check()
    assert all(np.array_equal(_bits(a), w.view(np.int32)) for a, w in zip(g, _got(name)[0]))
    assert np.array_equal(_bits(t), _got(name)[1].view(np.int64))
    eng.close()


# ---- 8. nothing of the engine moves -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tuning", [None, "ws=4"])
def test_the_engine_is_left_as_it_was(tuning):
    from montecarlopredictivecoding_amd import _lib as L_
    name = "relu_bern_mask"
    c = sg.NETS[name]

    def sequence(interleave):
        eng, inputs, xs = _engine(name, tuning)
        eng.bind_inputs(inputs)
        eng.load_state([x[0].contiguous() for x in xs])
        loss = dict(loss_kind=c["loss"], mask_start=c["mask_start"], lr=0.02)
        eng.run(3, xopt=L_.XOPT_ADAM, **loss)                   # (Adam moments worth keeping; the kick below is SGD's)
        run = dict(loss, xopt=L_.XOPT_SGD, noise_mode=L_.NOISE_PHILOX, noise_var=2.0, seed=9)
        eng.run(2, **run)                                      # (the Philox position has moved)
        if interleave:
            eng.state_gradients(None, [x[1:].contiguous() for x in xs], energies=True, **_kw(name))
        state = [torch.empty(c["B"], n, device=DEV) for n in c["sizes"]]
        ms, vs = [torch.empty_like(s) for s in state], [torch.empty_like(s) for s in state]
        eng.store_state(state)
        eng.store_adam_state(ms, vs)
        res = eng.run(3, energy_mode=L_.ENERGY_ALL, rec_count=3, rec_x=True, **run)
        after = [torch.empty_like(s) for s in state]
        eng.store_state(after)
        eng.sync_check()
        out = state + ms + vs + list(res.rec_x) + after
        counter = eng.step_counter
        eng.close()
        return out, res.energies, counter
    a, ea, ca = sequence(False)
    b, eb, cb = sequence(True)
    assert _same(a, b) and _same([ea], [eb]) and ca == cb == 8


# ---- 9. a side stream with pending inputs -------------------------------------------------------------------------------------------------
class StateGradientsCase(sc.Case):
    """state_gradients with energies on net relu_bern_mask, max_rows = 128 so that two chunks run (210 rows).  The warm-up call
    allocates the engine's scratch."""
    NET, MAX_ROWS = "relu_bern_mask", 128
    name = "state_gradients"
    entries = ("mcpc_state_gradients",)
    pending = ("inputs", "x0", "x1", "x2")

    @functools.lru_cache(maxsize=None)
    def inputs(self):
        d = sg.data(self.NET)
        out = {f"W{j}": d["W"][j] for j in range(4)}
        out.update({f"b{j}": d["b"][j] for j in range(4)})
        out.update({f"x{l}": d["xs"][l] for l in range(3)})
        out.update(inputs=d["inputs"], y=d["target"])
        return {k: np.array(v) for k, v in out.items()}

    def outputs(self, src):
        B = src["inputs"].shape[0]
        out = {f"grad{l}": sc.nan(src[f"x{l}"].shape) for l in range(3)}
        out["table"] = sc.nan((3, B, 8), sc.F64)
        return out

    def evaluate(self, st, d, out):
        grads = None if out is None else [out[f"grad{l}"] for l in range(3)]
        st.eng.state_gradients(d["inputs"], [d[f"x{l}"] for l in range(3)], out=grads, energies=True,
                               energies_out=None if out is None else out["table"], max_rows=self.MAX_ROWS, **_kw(self.NET))

    def before(self, dev, src):
        from montecarlopredictivecoding_amd.engine import Engine
        c = sg.NETS[self.NET]
        eng = Engine(list(c["sizes"]), [c["act"]] * 3, c["n_in"], c["n_out"], c["B"], device=dev)
        eng.bind_params([src[f"W{j}"] for j in range(4)], [src[f"b{j}"] for j in range(4)])
        eng.bind_inputs(None)
        eng.bind_target(src["y"])
        st = sc._State(eng=eng)
        self.evaluate(st, src, None)
        return st

    def call(self, st, buf, out):
        self.evaluate(st, buf, out)
        return {}


def test_on_a_side_stream_with_pending_inputs():
    sc.run_scenario(StateGradientsCase()).check()


# ---- 10. refusals -------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_device_work():
    from montecarlopredictivecoding_amd import _lib as L_
    from montecarlopredictivecoding_amd.engine import Engine
    lib = L_.load()
    name = "relu_bern_mask"
    c, d = sg.NETS[name], sg.data(name)
    eng, inputs, xs = _engine(name)
    MARK = -7.0
    grads = [torch.full_like(x, MARK) for x in xs]
    table = torch.full((sg.N_REC, c["B"], 8), MARK, dtype=torch.float64, device=DEV)
    arr = lambda ts: (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])
    base = dict(e=eng._h, desc=True, x=arr(xs), grad=arr(grads), n_rec=sg.N_REC, kind=c["loss"], var=1.0, mask=c["mask_start"], max_rows=0)

    def call(**kw):
        a = dict(base, **kw)
        g = L_.GradientDesc()
        g.inputs = inputs.data_ptr()
        g.x, g.grad = a["x"], a["grad"]
        g.n_rec, g.loss_kind, g.loss_var, g.mask_start, g.max_rows = a["n_rec"], a["kind"], a["var"], a["mask"], a["max_rows"]
        g.energies = table.data_ptr()
        g.stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
        code = lib.mcpc_state_gradients(a["e"], C.byref(g) if a["desc"] else None)
        return code, lib.mcpc_last_error().decode()

    EINVAL, ESTATE = -1, -4
    for kw, code, word in ((dict(e=None), EINVAL, "null engine"), (dict(desc=False), EINVAL, "null descriptor"), (dict(x=None), EINVAL, "x is null"),
                           (dict(grad=None), EINVAL, "grad is null"), (dict(x=arr([xs[0], None, xs[2]])), EINVAL, "x[1] is null"),
                           (dict(grad=arr([grads[0], grads[1], None])), EINVAL, "grad[2] is null"), (dict(n_rec=-1), EINVAL, "n_rec=-1"),
                           (dict(max_rows=-1), EINVAL, "max_rows=-1"), (dict(kind=3), EINVAL, "loss_kind=3"), (dict(mask=-1), EINVAL, "mask_start=-1"),
                           (dict(mask=40), EINVAL, "mask_start=40"), (dict(kind=L_.LOSS_GAUSSIAN, var=0.0), EINVAL, "loss_var must be positive")):
        got, msg = call(**kw)
        assert got == code and msg.startswith("state gradients: ") and word in msg, (kw, got, msg)
    bare = Engine(list(c["sizes"]), [c["act"]] * 3, c["n_in"], c["n_out"], c["B"], device=torch.device(DEV))
    got, msg = call(e=bare._h)
    assert got == ESTATE and "no bound parameters" in msg, (got, msg)
    bare.bind_params([torch.tensor(w).to(DEV) for w in d["W"]], [torch.tensor(v).to(DEV) for v in d["b"]])
    got, msg = call(e=bare._h)
    assert got == ESTATE and "no target bound" in msg, (got, msg)
    headless, _, hx = _engine("mu1_only")
    got, msg = call(e=headless._h, x=arr(hx), grad=arr([grads[0]]))
    assert got == EINVAL and "needs a read-out" in msg, (got, msg)
    assert call(n_rec=0)[0] == 0                              # a call that does nothing
    torch.cuda.synchronize()
    assert all((g == MARK).all() for g in grads) and (table == MARK).all(), "a refused call wrote into a destination"
    for e_ in (eng, bare, headless):
        e_.close()

"""Per-chain energies through the C ABI (include/mcpc.h: mcpc_chain_energies): against the fp64 oracle one chain at a time, bitwise
invariance under everything that regroups rows, against the step kernels' own energy table, and the argument checks."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import chain_energy_cases as cc
from tests import parity_log

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _engine(name, tuning=None, chains=None):
    """An engine for the case (its first `chains` chains), parameters, inputs-to-pass and target bound."""
    from montecarlopredictivecoding_amd.engine import Engine
    c, d = cc.NETS[name], cc.data(name)
    B = c["B"] if chains is None else chains
    L = len(c["sizes"])
    eng = Engine(list(c["sizes"]), [c["act"]] * L, c["n_in"], c["n_out"], B, device=torch.device(DEV), tuning=tuning)
    eng.bind_params([torch.tensor(w).to(DEV) for w in d["W"]], [torch.tensor(v).to(DEV) for v in d["b"]])
    if d["target"] is not None:
        eng.bind_target(torch.tensor(d["target"][:B]).to(DEV).contiguous())
    inputs = torch.tensor(d["inputs"][:B]).to(DEV).contiguous() if c["inputs"] else None
    xs = [torch.tensor(x[:, :B]).to(DEV).contiguous() for x in d["xs"]]
    return eng, inputs, xs


def _kw(name):
    c = cc.NETS[name]
    return dict(loss_kind=c["loss"], loss_var=c["var"], mask_start=c["mask_start"])


def _bits(t):
    return t.detach().cpu().numpy().view(np.int64)


# ---- 1. against the oracle, per chain --------------------------------------------------------------------------
@pytest.mark.parametrize("tuning", [None, "wide=1"])
@pytest.mark.parametrize("name", sorted(cc.NETS))
def test_rows_match_the_oracle_chain_by_chain(name, tuning):
    eng, inputs, xs = _engine(name, tuning)
    got = eng.chain_energies(inputs, xs, **_kw(name))
    eng.sync_check()
    L = len(cc.NETS[name]["sizes"])
    assert got.shape == (cc.N_REC, cc.NETS[name]["B"], 8) and got.dtype == torch.float64
    got = cc.columns(got.cpu().numpy(), L)
    want, bound = cc.reference(name)
    assert np.isfinite(got).all() and (want[..., -1] > 0).all()
    cc.log_against_bound(parity_log, f"mcpc_chain_energies vs oracle per chain ({name}, {tuning or 'default'})", got, want, bound,
                         ["loss"] + [f"E_{l + 1}" for l in range(L)] + ["overall"])
    eng.close()


# ---- 2. bitwise -------------------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_how_they_are_grouped():
    name = "relu_bern_mask"
    eng, inputs, xs = _engine(name)
    kw = _kw(name)
    one = eng.chain_energies(inputs, xs, **kw)
    again = eng.chain_energies(inputs, xs, **kw)
    assert np.array_equal(_bits(one), _bits(again)), "a repeated call"
    small = eng.chain_energies(inputs, xs, max_rows=64, **kw)                    # 210 rows: four chunks, none starting at a chain 0
    assert np.array_equal(_bits(one), _bits(small)), "max_rows=64 against the default"
    big = eng.chain_energies(inputs, xs, max_rows=1 << 20, **kw)
    assert np.array_equal(_bits(one), _bits(big)), "max_rows larger than the call"
    parts = torch.stack([eng.chain_energies(inputs, [x[k] for x in xs], **kw)[0] for k in range(cc.N_REC)])
    assert np.array_equal(_bits(one), _bits(parts)), "n_rec = 3 in one call against three calls"
    # the first 16 chains alone, on an engine of their own: other neighbours in the tile, another number of rows
    eng16, inputs16, xs16 = _engine(name, chains=16)
    few = eng16.chain_energies(inputs16, xs16, **kw)
    assert np.array_equal(_bits(one[:, :16].contiguous()), _bits(few)), "the first 16 chains alone"
    eng16.close()
    eng.close()


# ---- 3. against the step kernels --------------------------------------------------------------------------------
@pytest.mark.parametrize("tuning", [None, "ws=0", "ws=4"])
def test_chain_sums_are_the_step_kernels_energy_table(tuning):
    from montecarlopredictivecoding_amd import _lib as L_
    name, T = "relu_bern_mask", 5
    c = cc.NETS[name]
    eng, inputs, xs = _engine(name, tuning)
    eng.bind_inputs(inputs)
    eng.load_state([x[0].contiguous() for x in xs])
    res = eng.run(T, loss_kind=c["loss"], mask_start=c["mask_start"], xopt=L_.XOPT_SGD, lr=0.02, noise_mode=L_.NOISE_PHILOX, noise_var=2.0,
                  seed=9, step_base=0, energy_mode=L_.ENERGY_ALL, rec_count=T, rec_x=True)
    got = eng.chain_energies(inputs, res.rec_x, **_kw(name))
    eng.sync_check()
    table = res.energies.cpu().numpy()                                           # [T, 8]
    sums = got.cpu().numpy().sum(axis=1)                                         # fp64 over the chains
    assert (table[:, 0] > 0).all() and (table[:, 1:4] > 0).all()
    group = f"mcpc_chain_energies summed over chains vs mcpc_run energies ({tuning or 'default'}: {eng.last_step_kernel()})"
    for col, q in ((0, "loss"), (1, "E_1"), (2, "E_2"), (3, "E_3"), (7, "overall")):
        parity_log.close(group, q, sums[:, col], table[:, col], rtol=1e-6, atol=0.0)
    assert (sums[:, 4:7] == 0).all() and (table[:, 4:7] == 0).all()
    eng.close()


# ---- 4. bad arguments ----------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch():
    from montecarlopredictivecoding_amd import _lib as L_
    from montecarlopredictivecoding_amd.engine import Engine
    lib = L_.load()
    name = "relu_bern_mask"
    c, d = cc.NETS[name], cc.data(name)
    eng, inputs, xs = _engine(name)
    out = torch.full((cc.N_REC, c["B"], 8), -7.0, dtype=torch.float64, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    arr = (C.c_void_p * 3)(*[x.data_ptr() for x in xs])
    hole = (C.c_void_p * 3)(xs[0].data_ptr(), None, xs[2].data_ptr())
    base = dict(e=eng._h, inputs=C.c_void_p(inputs.data_ptr()), x=arr, n_rec=cc.N_REC, kind=c["loss"], var=1.0, mask=c["mask_start"],
                out=C.c_void_p(out.data_ptr()), max_rows=0)

    def call(**kw):
        a = dict(base, **kw)
        code = lib.mcpc_chain_energies(a["e"], a["inputs"], a["x"], a["n_rec"], a["kind"], a["var"], a["mask"], a["out"], a["max_rows"], stream)
        return code, lib.mcpc_last_error().decode()

    EINVAL, ESTATE = -1, -4
    for kw, code, word in ((dict(e=None), EINVAL, "null engine"), (dict(x=None), EINVAL, "x_rec is null"), (dict(x=hole), EINVAL, "x_rec[1] is null"),
                           (dict(out=None), EINVAL, "out is null"), (dict(n_rec=-1), EINVAL, "n_rec=-1"), (dict(max_rows=-1), EINVAL, "max_rows=-1"),
                           (dict(kind=3), EINVAL, "loss_kind=3"), (dict(mask=-1), EINVAL, "mask_start=-1"), (dict(mask=40), EINVAL, "mask_start=40"),
                           (dict(kind=L_.LOSS_GAUSSIAN, var=0.0), EINVAL, "loss_var must be positive")):
        got, msg = call(**kw)
        assert got == code and word in msg, (kw, got, msg)
    # a loss without a bound target; a loss on a network without a read-out
    bare = Engine(list(c["sizes"]), [c["act"]] * 3, c["n_in"], c["n_out"], c["B"], device=torch.device(DEV))
    got, msg = call(e=bare._h)
    assert got == ESTATE and "no bound parameters" in msg, (got, msg)
    bare.bind_params([torch.tensor(w).to(DEV) for w in d["W"]], [torch.tensor(v).to(DEV) for v in d["b"]])
    got, msg = call(e=bare._h)
    assert got == ESTATE and "no target bound" in msg, (got, msg)
    headless, _, hx = _engine("mu1_only")
    got, msg = call(e=headless._h, x=(C.c_void_p * 1)(hx[0].data_ptr()))
    assert got == EINVAL and "needs a read-out" in msg, (got, msg)
    torch.cuda.synchronize()
    assert (out == -7.0).all(), "a refused call wrote into out"
    # n_rec = 0 is a call that does nothing
    assert call(n_rec=0)[0] == 0
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    for e_ in (eng, bare, headless):
        e_.close()

"""mcpc_sample_prior without a GPU: the header and the binding agree on the entry point and its constants, a null engine is refused with a
message before any device work, and the Python fronts (engine.check_sample_prior behind Engine.sample_prior, sample_pc_device,
get_marginal_likelihood_per_datum(sampler=...)) refuse bad arguments before they need a device."""
import ctypes as C
import os
import re

import pytest
import torch

from montecarlopredictivecoding_amd import _lib
from montecarlopredictivecoding_amd import predictive_coding as pc
from montecarlopredictivecoding_amd.engine import check_sample_prior
from montecarlopredictivecoding_amd.utils import model as um
from montecarlopredictivecoding_amd.utils import training_evaluation as te

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mcpc.h")).read()
CTYPE = {"mcpc_engine*": C.c_void_p, "const float*": C.c_void_p, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "int32_t": C.c_int32,
         "double": C.c_double, "float* const*": C.POINTER(C.c_void_p), "float*": C.c_void_p, "void*": C.c_void_p}


def test_header_declares_the_entry_point_and_its_constants():
    for name, value in (("MCPC_SAMPLE_HIDDEN", 0), ("MCPC_SAMPLE_MEAN", 1), ("MCPC_SAMPLE_DRAW", 2)):
        m = re.search(r"#define\s+%s\s+(\d+)" % name, HEADER)
        assert m and int(m.group(1)) == value, name
    assert (_lib.SAMPLE_HIDDEN, _lib.SAMPLE_MEAN, _lib.SAMPLE_DRAW) == (0, 1, 2)
    assert re.search(r"#define\s+MCPC_ABI_VERSION\s+4\b", HEADER) and _lib.ABI_VERSION == 4


def test_binding_argument_types_match_the_declaration():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    m = re.search(r"\bint\s+mcpc_sample_prior\s*\((.*?)\)\s*;", code, flags=re.S)
    assert m, "include/mcpc.h does not declare mcpc_sample_prior"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    names = [p.rsplit(" ", 1)[1] for p in params]
    assert names == ["e", "inputs", "n", "seed", "step", "sample_base", "loss_kind", "loss_var", "readout", "x_out", "out", "max_rows", "stream"]
    want = [CTYPE[p.rsplit(" ", 1)[0]] for p in params]
    res, args = _lib.SYMBOLS["mcpc_sample_prior"]
    assert res is C.c_int and args == want


def test_null_engine_is_einval_with_a_message():
    lib = _lib.load()
    rc = lib.mcpc_sample_prior(None, None, 4, 1, 0, 0, _lib.LOSS_NONE, 1.0, _lib.SAMPLE_HIDDEN, None, None, 0, None)
    assert rc == -1 and b"sample prior: null engine" in lib.mcpc_last_error()
    with pytest.raises(_lib.MCPCError, match="null engine"):
        _lib.check(rc)


def test_argument_checks_of_engine_sample_prior():
    L, n_out = 3, 10
    n, kind, var, code, layers, want_out = check_sample_prior(L, n_out, 7)
    assert (n, kind, var, code, layers, want_out) == (7, _lib.LOSS_NONE, 1.0, _lib.SAMPLE_HIDDEN, (), True)
    assert check_sample_prior(L, n_out, 7, loss="bernoulli", readout="draw", latents=True)[1:] == (
        _lib.LOSS_BERNOULLI, 1.0, _lib.SAMPLE_DRAW, (0, 1, 2), True)
    assert check_sample_prior(L, n_out, 7, loss="gaussian", var=0.25, readout="draw", latents=(2, 0, 2))[1:] == (
        _lib.LOSS_GAUSSIAN, 0.25, _lib.SAMPLE_DRAW, (0, 2), True)
    assert check_sample_prior(L, n_out, 0, loss="gaussian", readout="mean")[3] == _lib.SAMPLE_MEAN          # (the mean needs no variance)
    assert check_sample_prior(L, 0, 5, latents=(1,))[4:] == ((1,), False)                                     # no read-out: latents alone
    assert check_sample_prior(L, n_out, 5, readout=None, latents=True)[5] is False
    assert check_sample_prior(L, n_out, 1, sample_base=(1 << 32) - 1)[0] == 1                                  # the last id there is
    for kw, msg in ((dict(n=-1), "must not be negative"),
                    (dict(n=2, sample_base=(1 << 32) - 1), "32 bits"),
                    (dict(n=1, sample_base=-1), "32 bits"),
                    (dict(n=1, max_rows=-64), "max_rows"),
                    (dict(n=1, readout="logits"), "readout"),
                    (dict(n=1, loss="poisson"), "loss"),
                    (dict(n=1, latents=(3,)), "out of range"),
                    (dict(n=1, latents=(-1,)), "out of range"),
                    (dict(n=1, readout=None), "nothing is asked for"),
                    (dict(n=1, readout="mean"), "needs a loss"),
                    (dict(n=1, readout="draw"), "needs a loss"),
                    (dict(n=1, readout="draw", loss="gaussian"), "positive variance"),
                    (dict(n=1, readout="draw", loss="gaussian", var=0.0), "positive variance")):
        with pytest.raises(ValueError, match=msg):
            check_sample_prior(L, n_out, **kw)
    with pytest.raises(ValueError, match="nothing is asked for"):
        check_sample_prior(L, 0, 1)


def _model(n_out=6):
    mods = [torch.nn.Linear(2, 5), pc.PCLayer(), torch.nn.ReLU(), torch.nn.Linear(5, 4), pc.PCLayer(), torch.nn.ReLU()]
    if n_out:
        mods.append(torch.nn.Linear(4, n_out))
    else:
        mods.pop()
    return torch.nn.Sequential(*mods)


def test_argument_checks_of_sample_pc_device_need_no_device():
    cfg = dict(input_size=2, loss_fn=um.bernoulli_fn, input_var=0.3)
    model = _model()
    with pytest.raises(ValueError, match="must not be negative"):
        te.sample_pc_device(-1, model, cfg)
    with pytest.raises(ValueError, match="32 bits"):
        te.sample_pc_device(2, model, cfg, sample_base=(1 << 32) - 1)
    with pytest.raises(ValueError, match="input_size"):
        te.sample_pc_device(2, model, dict(cfg, input_size=3))
    with pytest.raises(ValueError, match="positive variance"):
        te.sample_pc_device(2, model, dict(cfg, loss_fn=um.fe_fn, input_var=0.0))
    with pytest.raises(NotImplementedError, match="ends in a PCLayer"):
        te.sample_pc_device(2, _model(0), cfg)
    with pytest.raises(NotImplementedError, match="outside what the HIP engine expresses"):
        te.sample_pc_device(2, torch.nn.Sequential(torch.nn.Linear(2, 3), torch.nn.Sigmoid(), torch.nn.Linear(3, 2)), cfg)
    with pytest.raises(NotImplementedError, match="outside what the HIP engine expresses"):
        pc.PCTrainer(torch.nn.Sequential(torch.nn.Linear(2, 3)), update_p_at="never", plot_progress_at=[]).mcpc_sample_prior(2)


def test_marginal_likelihood_rejects_an_unknown_sampler():
    cfg = dict(input_size=2, loss_fn=um.bernoulli_fn, input_var=0.3)
    with pytest.raises(ValueError, match="sampler='numpy'"):
        te.get_marginal_likelihood_per_datum(_model(), cfg, [], False, n_samples=4, sampler="numpy")


def test_without_a_device_the_sampler_raises():
    if torch.cuda.is_available():
        pytest.skip("a HIP device is visible")
    cfg = dict(input_size=2, loss_fn=um.bernoulli_fn, input_var=0.3)
    with pytest.raises(_lib.MCPCLibraryError, match="no HIP device is visible"):
        te.sample_pc_device(3, _model(), cfg, is_return_hidden=True)

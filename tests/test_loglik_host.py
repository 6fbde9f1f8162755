"""The per-datum marginal likelihood, the host side: the binding, the C entry point's argument checks, the arithmetic of
``LogLikelihood`` against numpy, and the yardstick itself (tests/loglik_cases.py) against the reference's recorded value.  No GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from montecarlopredictivecoding_amd import _lib
from montecarlopredictivecoding_amd import likelihood as K
from tests import loglik_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g10_eval_bernoulli.npz")
INF = math.inf


def test_header_declares_the_entry_points_and_the_binding_binds_them():
    header = open(os.path.join(ROOT, "include", "mcpc.h")).read()
    assert re.search(r"\bint\s+mcpc_loglik_accumulate\s*\(", header) and re.search(r"\bint64_t\s+mcpc_loglik_workspace_bytes\s*\(", header)
    assert re.search(r"#define\s+MCPC_ABI_VERSION\s+4\b", header) and _lib.ABI_VERSION == 4
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, n_args, res in (("mcpc_loglik_accumulate", 14, C.c_int), ("mcpc_loglik_workspace_bytes", 3, C.c_int64)):
        decl = re.search(name + r"\s*\(([^)]*)\)", code).group(1)
        assert len(_lib.SYMBOLS[name][1]) == len(decl.split(",")) == n_args and _lib.SYMBOLS[name][0] is res
    args = _lib.SYMBOLS["mcpc_loglik_accumulate"][1]
    assert args[2] is C.c_int64 and args[4] is C.c_int64 and args[7] is C.c_double and args[8] is C.c_double and args[12] is C.c_int64
    from montecarlopredictivecoding_amd import engine
    assert callable(engine.loglik_accumulate) and callable(engine.loglik_workspace_bytes)
    lib = _lib.load()
    assert lib.mcpc_abi_version() == 4 and hasattr(lib, "mcpc_loglik_accumulate") and hasattr(lib, "mcpc_loglik_workspace_bytes")
    doc = header[header.index("The importance-sampled log marginal likelihood"):header.index("int mcpc_loglik_accumulate")]
    for word in ("merge rule", "What is bitwise", "within a bound", "softplus", "empty"):
        assert word in doc, word


@pytest.mark.parametrize("n_data, n_samp", [(1, 1), (16, 16), (17, 600), (48, 600), (17, 33), (1000, 5000), (10000, 5000), (20000, 7),
                                            (1, 1 << 20), ((1 << 31) - 1, 1), (1, (1 << 31) - 1)])
def test_the_python_plan_is_the_librarys(n_data, n_samp):
    """likelihood.plan mirrors the library's grouping: the workspace the library asks for is the one the plan implies, whatever the
    width, and the groups cover the sample tiles."""
    lib = _lib.load()
    p = K.plan(n_data, n_samp, 5)
    assert lib.mcpc_loglik_workspace_bytes(n_data, n_samp, 5) == lib.mcpc_loglik_workspace_bytes(n_data, n_samp, 784) == p["workspace_bytes"]
    assert (p["groups"] - 1) * p["tiles_per_group"] < p["n_stiles"] <= p["groups"] * p["tiles_per_group"]
    assert p["groups"] * p["n_dtiles"] <= 8192 + p["n_dtiles"]                        # the jobs aimed at, never more than a datum tile's worth over


def test_the_plan_of_nothing():
    lib = _lib.load()
    assert lib.mcpc_loglik_workspace_bytes(0, 600, 5) == 0 == K.plan(0, 600, 5)["workspace_bytes"]
    assert lib.mcpc_loglik_workspace_bytes(48, 0, 5) == 0 == K.plan(48, 0, 5)["workspace_bytes"]
    assert K.plan(17, 33, 5)["groups"] == 3 and K.plan(17, 600, 5)["groups"] == 38


def test_argument_errors_are_refused_before_any_device_work():
    """Every MCPC_EINVAL case returns -1 with a message and touches no device: the pointers are never dereferenced (this machine need
    not have a GPU)."""
    lib = _lib.load()
    p = [C.c_void_p(0x1000 * (i + 1)) for i in range(4)]             # never dereferenced: every call below is refused
    need = lib.mcpc_loglik_workspace_bytes(48, 600, 5)
    assert need > 0 and need % 8 == 0

    def call(y=p[0], n_data=48, out=p[1], n_samp=600, width=5, loss=_lib.LOSS_BERNOULLI, var=1.0, clamp=20.0, state=p[2], accumulate=0,
             ws=p[3], ws_bytes=need):
        rc = lib.mcpc_loglik_accumulate(0, y, n_data, out, n_samp, width, loss, var, clamp, state, accumulate, ws, ws_bytes, None)
        return rc, lib.mcpc_last_error().decode()

    for kw, word in [(dict(width=0), "width=0"), (dict(width=-3), "width=-3"),
                     (dict(n_data=-1), "n_data=-1 outside"), (dict(n_samp=-1), "n_samp=-1 outside"),
                     (dict(n_data=1 << 31), "n_data=2147483648 outside"), (dict(n_samp=1 << 31), "n_samp=2147483648 outside"),
                     (dict(loss=_lib.LOSS_NONE), "loss_kind=0"), (dict(loss=3), "loss_kind=3"), (dict(loss=-1), "loss_kind=-1"),
                     (dict(loss=_lib.LOSS_GAUSSIAN, var=0.0), "loss_var=0"), (dict(loss=_lib.LOSS_GAUSSIAN, var=-1.0), "loss_var=-1"),
                     (dict(loss=_lib.LOSS_GAUSSIAN, var=math.nan), "loss_var=nan"),
                     (dict(clamp=0.0), "clamp=0"), (dict(clamp=-20.0), "clamp=-20"), (dict(clamp=math.nan), "clamp=nan"),
                     (dict(y=None), "y is null with n_data=48"), (dict(state=None), "state is null with n_data=48"),
                     (dict(out=None), "out is null with n_samp=600"), (dict(ws=None), "workspace is null"),
                     (dict(ws_bytes=need - 1), "workspace of %d bytes is too small, %d needed" % (need - 1, need))]:
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("loglik:") and word in msg, (kw, rc, msg)
        args = {"n_data": 48, "n_samp": 600, "width": 5}
        if set(kw) & set(args):
            args.update(kw)
            assert lib.mcpc_loglik_workspace_bytes(args["n_data"], args["n_samp"], args["width"]) == -1
    # nothing to do: accepted without a device, and nothing is read
    assert call(n_data=0, y=None, state=None, ws=None, ws_bytes=0)[0] == 0
    assert call(n_samp=0, out=None, accumulate=1, ws=None, ws_bytes=0)[0] == 0
    assert call(n_data=0, y=None, state=None, loss=_lib.LOSS_GAUSSIAN, var=0.5, clamp=INF, ws=None, ws_bytes=0)[0] == 0


def _fixture():
    g = np.load(GOLDEN)
    return g["data"].astype(np.float32), g["ml_logits"].astype(np.float32), float(g["ml"])


def test_the_yardstick_reproduces_the_references_recorded_value():
    """ref_state on the reference's own prior samples and data against the scalar the reference recorded in fp32, at the tolerance
    tests/test_evaluators_golden.py gives that value; and what the scalar hides."""
    y, o, ml = _fixture()
    assert y.shape[0] == 48 and o.shape[0] == 600 and y.shape[1] == o.shape[1]
    st = R.ref_state(y, o, "bernoulli", None, 20.0)
    got = float(R.log_p(st).mean())
    print("reference ml %.12g, fp64 %.12g, relative difference %.3g" % (ml, got, abs(got - ml) / abs(ml)))
    assert got == pytest.approx(ml, rel=2e-6)
    es = R.ess(st)
    print("ESS of the importance weights per datum: %.1f .. %.1f of %d; max delta %.3g" % (es.min(), es.max(), o.shape[0],
                                                                                            R.delta(y, o, "bernoulli").max()))
    assert (st[:, 3] == 600).all() and (es >= 1).all() and (es <= 600).all() and es.min() < 100     # degenerate for some data


@pytest.mark.parametrize("loss", R.LOSSES)
def test_merge_and_cat_agree_with_numpy(loss):
    y, o, var = R.make_case(19, 211, 13, loss, seed=4)
    nll = R.nll_matrix(y, o, loss, var)
    a, b = R.state_from_nll(nll[:, :100]), R.state_from_nll(nll[:, 100:])
    A, B = K.LogLikelihood(torch.from_numpy(a)), K.LogLikelihood(torch.from_numpy(b))
    M = A.merge(B)
    assert M.state.dtype == torch.float64 and tuple(M.state.shape) == (19, 4) and len(M) == 19
    np.testing.assert_allclose(M.state.numpy(), R.merge(a, b), rtol=4 * 2.0 ** -52, atol=0)
    np.testing.assert_array_equal(M.n_samples.numpy(), np.full(19, 211.0))
    # the two halves against the whole, within the tolerance
    whole = R.ref_state(y, o, loss, var)
    t = R.tol(y, o, loss, var)
    R.assert_state_close(M.state.numpy(), whole, t, f"merge of two halves ({loss})")
    assert (np.abs(M.log_p.numpy() - R.log_p(whole)) <= t).all()                      # the properties, on the same footing
    assert (np.abs(M.ess.numpy() - R.ess(whole)) <= t * R.ess(whole)).all()
    assert M.mean() == pytest.approx(float(R.log_p(whole).mean()), abs=float(t.max()))
    # merge is symmetric up to rounding, and the operands are not modified
    np.testing.assert_allclose(B.merge(A).state.numpy(), M.state.numpy(), rtol=4 * 2.0 ** -52, atol=0)
    np.testing.assert_array_equal(A.state.numpy(), a)
    # cat: more data, in the order given
    top, bottom = K.LogLikelihood(torch.from_numpy(whole[:7].copy())), K.LogLikelihood(torch.from_numpy(whole[7:].copy()))
    both = K.LogLikelihood.cat([top, bottom])
    np.testing.assert_array_equal(both.state.numpy(), whole)
    np.testing.assert_array_equal(both.cpu().state.numpy(), whole)
    with pytest.raises(ValueError, match="19 data against 7"):
        M.merge(top)


def test_a_chain_of_merges_over_ragged_chunks():
    y, o, var = R.make_case(5, 97, 6, "bernoulli", seed=9)
    nll = R.nll_matrix(y, o, "bernoulli", None)
    acc = K.LogLikelihood(K.empty_state(5))
    for s0 in range(0, 97, 17):
        acc = acc.merge(K.LogLikelihood(torch.from_numpy(R.state_from_nll(nll[:, s0:s0 + 17]))))
    R.assert_state_close(acc.state.numpy(), R.ref_state(y, o, "bernoulli"), R.tol(y, o, "bernoulli"), "six chunks of 17")


def test_empty_states_and_data_without_samples():
    e = K.empty_state(3)
    assert e.dtype == torch.float64 and e.tolist() == [[INF, 0.0, 0.0, 0.0]] * 3
    E = K.LogLikelihood(e)
    assert torch.isnan(E.log_p).all() and torch.isnan(E.ess).all() and E.n_samples.tolist() == [0.0] * 3
    assert E.merge(E).state.tolist() == e.tolist()                                     # inf - inf is never formed
    st = torch.tensor([[2.5, 1.75, 1.3, 4.0], [INF, 0.0, 0.0, 0.0], [-3.0, 1.0, 1.0, 1.0]], dtype=torch.float64)
    S = K.LogLikelihood(st)
    assert S.merge(E).state.tolist() == st.tolist() and E.merge(S).state.tolist() == st.tolist()      # the empty state is neutral, exactly
    lp, es = S.log_p, S.ess
    assert float(lp[0]) == pytest.approx(math.log(1.75 / 4.0) - 2.5, abs=1e-15) and math.isnan(float(lp[1])) and float(lp[2]) == 3.0
    assert float(es[0]) == pytest.approx(1.75 ** 2 / 1.3, rel=1e-15) and math.isnan(float(es[1])) and float(es[2]) == 1.0
    assert math.isnan(S.mean())                                                        # a datum without samples has no estimate
    # the reference leaves the same: a row of the nll matrix without a finite entry
    nll = np.array([[1.0, np.nan, 2.0], [np.nan, np.inf, -np.inf], [5.0, 5.0, 5.0]])
    want = R.state_from_nll(nll)
    assert want[1].tolist() == [INF, 0.0, 0.0, 0.0] and want[0, 3] == 2 and want[2].tolist() == [5.0, 3.0, 3.0, 3.0]
    # more than 745 nats apart: the smaller side underflows to nothing, without a NaN
    far = K.LogLikelihood(torch.tensor([[0.0, 1.0, 1.0, 1.0]], dtype=torch.float64)).merge(
        K.LogLikelihood(torch.tensor([[900.0, 3.0, 2.0, 5.0]], dtype=torch.float64)))
    assert far.state.tolist() == [[0.0, 1.0, 1.0, 6.0]] and float(far.ess[0]) == 1.0 and float(far.log_p[0]) == -math.log(6.0)


def test_without_a_device_the_evaluator_raises():
    if torch.cuda.is_available():
        pytest.skip("a HIP device is visible")
    y = np.zeros((4, 3), dtype=np.float32)
    with pytest.raises(_lib.MCPCLibraryError, match="no HIP device is visible"):
        K.log_likelihood(y, y)
    with pytest.raises(_lib.MCPCLibraryError, match="no HIP device is visible"):
        K.log_likelihood(torch.zeros(4, 3), y, loss="gaussian", var=1.0)
    from montecarlopredictivecoding_amd.utils import training_evaluation as te
    assert callable(te.get_marginal_likelihood_per_datum)

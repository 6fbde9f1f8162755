"""The Metropolis-adjusted Langevin step and annealed importance sampling with it, as far as no device is needed: properties of the
restatement of tests/mala_cases.py, the Philox block of the accept step's uniform, what `adjust` refuses, the two entry points in the
header and the binding, and every figure tests/mala_cases.py records, recomputed."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from montecarlopredictivecoding_amd import _lib as L
from montecarlopredictivecoding_amd import ais
from montecarlopredictivecoding_amd import predictive_coding as pc
from montecarlopredictivecoding_amd.utils import model as um
from oracle import philox
from tests import ais_cases as A
from tests import mala_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(M.KERNEL_CASES))
def test_log_alpha_is_antisymmetric_under_exchanging_the_state_and_the_proposal(name):
    xs, gs, E, xps, gps, Ep = M.kernel_inputs(name)
    r = M.KERNEL_RUN
    fwd, m_fwd = M.log_alpha(xs, gs, E, xps, gps, Ep, r["lr"], r["noise_var"])
    bwd, m_bwd = M.log_alpha(xps, gps, Ep, xs, gs, E, r["lr"], r["noise_var"])
    # x - x' and x' - x, E - E' and E' - E, sa - sb and sb - sa are negations of each other bit for bit
    np.testing.assert_array_equal(fwd, -bwd)
    np.testing.assert_array_equal(m_fwd, m_bwd)
    assert np.isfinite(fwd).all() and (m_fwd > 0).all()


def test_the_fp32_proposal_rounds_four_times():
    rng = np.random.default_rng(3)
    x, g, z = (rng.standard_normal((7, 13)).astype(np.float32) for _ in range(3))
    lr, nv = 0.1, 2.0
    got = M.propose(x, g, z, lr, nv)
    f = np.float32
    want = np.empty_like(x)
    for i in np.ndindex(x.shape):                                          # element by element, a rounding after every operation
        p = f(f(lr) * g[i])
        a = f(x[i] - p)
        n = f(f(np.sqrt(nv * lr)) * z[i])
        want[i] = f(a + n)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))
    exact = x.astype(np.float64) - lr * g.astype(np.float64) + np.sqrt(nv * lr) * z.astype(np.float64)
    assert np.abs(got - exact).max() < 4 * 2.0 ** -24 * np.abs(exact).max() + 1e-7
    assert np.abs(M.propose(x, g, z, lr, nv, np.float64) - exact).max() < 1e-15


def test_a_nan_log_alpha_rejects():
    la = np.array([np.nan, -np.inf, np.inf, 0.0, -1e-300])
    u = np.array([0.5, 0.5, 0.5, 1.0, 1.0])
    assert M.decide(la, u).tolist() == [False, False, True, False, False]   # log 1 = 0 is not below 0


# ---- the uniform's Philox block --------------------------------------------------------------------------------------------------------
def test_the_uniform_is_word_0_of_the_block_of_layer_255():
    r = M.KERNEL_RUN
    seed, step, base = r["seed"], r["step"], r["chain_base"]
    w = philox.philox4x32_10(np.arange(base, base + 19, dtype=np.uint32), np.uint32(0xFF << 24), np.uint32(step & 0xFFFFFFFF),
                             np.uint32(step >> 32), np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32))[0]
    u = M.uniform(seed, step, base, 19)
    np.testing.assert_array_equal(u, ((w >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24)
    assert u.dtype == np.float64 and (u > 0).all() and (u <= 1).all()
    np.testing.assert_array_equal(M.uniform(seed, step, base + 5, 14), u[5:])            # a chain's uniform is its own


def _blocks(what, g0, sb, n, sizes, n_out, steps_per_stage):
    """Every Philox counter block (chain, word 1, step) an engine call of ais.engine_calls consumes for its normals: the prior draws
    the latent layers and, at most, the read-out under layer index n_latent; a run draws the latent layers at each of its steps."""
    widths = list(sizes) + ([n_out] if what == "prior" else [])
    steps = [sb] if what == "prior" else range(sb, sb + steps_per_stage)
    return {(c, (l << 24) | grp, t) for c in range(g0, g0 + n) for l, w in enumerate(widths) for grp in range((w + 3) // 4) for t in steps}


def test_the_uniforms_block_is_no_block_of_the_normals_or_the_prior():
    kw = dict(n_data=5, replicas=16, n_rungs=8, steps_per_stage=4, step_base=100, chain_base=40)
    sizes, n_out = (33, 17), 40
    normals = set()
    for max_chains in (80, 32):
        for call in ais.engine_calls(max_chains=max_chains, **kw):
            normals |= _blocks(*call, sizes, n_out, 4)
    uniforms = {(c, M.UNIFORM_LAYER << 24, 101 + s) for c in range(40, 120) for s in range(7 * 4)}
    assert len(uniforms) == 80 * 28 and len(normals) == 80 * (1 + 28) * (9 + 5) + 80 * 10
    assert not (uniforms & normals)
    # whatever the widths: a layer index is at most MAX_LATENT (the prior's read-out draw), a group index stays below 2^24
    assert M.UNIFORM_LAYER > L.MAX_LATENT and M.MAX_LATENT == L.MAX_LATENT
    assert all(w1 >> 24 <= L.MAX_LATENT for _, w1, _ in normals)
    # and the steps of a call's uniforms are those of its transitions: step_base + 1 onwards, never the prior's step
    assert min(t for _, _, t in uniforms) == kw["step_base"] + 1


# ---- what the call refuses ----------------------------------------------------------------------------------------------------------------
def _trainer():
    model = nn.Sequential(nn.Linear(6, 16), pc.PCLayer(), nn.Tanh(), nn.Linear(16, 24))
    model.train()
    return pc.PCTrainer(model, T=4, optimizer_x_fn=torch.optim.SGD, optimizer_x_kwargs={"lr": 0.03}, update_p_at="never", plot_progress_at=[])


@pytest.mark.parametrize("adjust", ["MALA", "mh", "", 1, True, 0.5, ("mala",), b"mala"])
def test_a_bad_adjust_is_a_value_error_before_any_device_is_asked_for(adjust):
    tr = _trainer()
    with pytest.raises(ValueError, match="adjust"):
        tr.mcpc_ais(torch.zeros(3, 24), um.fe_fn, {"_var": 0.7}, adjust=adjust)
    with pytest.raises(ValueError, match="adjust"):
        ais.check_adjust(adjust)
    assert tr.mcpc_last_ais_acceptance is None


def test_good_adjust_values_pass_the_check_and_reach_the_device():
    assert ais.check_adjust(None) is None and ais.check_adjust("mala") == "mala"
    assert _trainer().mcpc_last_ais_acceptance is None
    if torch.cuda.is_available():
        return                                                   # (tests/test_gpu_mala_ais.py runs them)
    with pytest.raises(L.MCPCLibraryError):
        _trainer().mcpc_ais(torch.zeros(3, 24), um.fe_fn, {"_var": 0.7}, replicas=4, stages=3, adjust="mala")


# ---- the entry points -----------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_both_entry_points_and_the_binding_binds_them():
    header = open(os.path.join(ROOT, "include", "mcpc.h")).read()
    for name in ("mcpc_mala_propose", "mcpc_mala_accept"):
        assert re.search(r"^int " + name + r"\(int device,", header, re.M), name
        assert name in L.SYMBOLS and L.SYMBOLS[name][0] is L.C.c_int
    # the argument counts of the declarations and of the binding agree
    for name in ("mcpc_mala_propose", "mcpc_mala_accept"):
        decl = re.search(r"^int " + name + r"\((.*?)\);", header, re.M | re.S).group(1)
        assert len(decl.split(",")) == len(L.SYMBOLS[name][1]), name
    assert re.search(r"#define MCPC_ABI_VERSION 4\b", header) and L.ABI_VERSION == 4
    assert "#define MCPC_MALA_MAX_ROWS" in header
    from montecarlopredictivecoding_amd import engine
    assert callable(engine.mala_propose) and callable(engine.mala_accept)


# ---- the recorded figures --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(M.KERNEL_CASES))
def test_the_kernel_cases_decide_far_from_roundoff_and_accept_about_half(name):
    c = M.KERNEL_CASES[name]
    assert 1 <= len(c["widths"]) <= M.MAX_LATENT and sum(c["widths"]) <= M.MAX_UNITS
    la, Mr, u, acc = M.kernel_reference(name)
    dist = np.abs(np.log(u) - la)
    need = M.margin_needed(Mr, u)
    print(f"{name}: accepted {int(acc.sum())} of {acc.size}, smallest |log u - log_alpha| = {dist.min():.3g}, needed {need.max():.3g}")
    assert (dist > need).all()
    if name in M.SHARE_CASES:
        assert 0.25 <= acc.mean() <= 0.75, acc.mean()
    elif name == "one_row_accepts":
        assert acc.all() and (la > 0).all()
    else:
        assert not acc.any() and (la < 24 * np.log(0.5)).all()


def test_the_cases_cover_the_shapes_the_kernel_treats_differently():
    shapes = {(c["widths"], c["rows"]) for c in M.KERNEL_CASES.values()}
    assert ((5, 33, 17), 19) in shapes and ((5, 33, 17), 1) in shapes and ((1,), 19) in shapes
    six = M.KERNEL_CASES["six_layers"]["widths"]
    assert len(six) == L.MAX_LATENT and all(w % 4 for w in six) and max(six) > 256        # a lane walks two groups of the widest layer


@pytest.mark.parametrize("name", sorted(A.ESTIMATOR_CASES))
def test_the_mala_restatement_stays_where_it_was_measured(name):
    l32, s32, a32, m32 = M.estimator_reference(name, "float32")
    l64, _, a64, m64 = M.estimator_reference(name, "float64")
    flipped = (a32 != a64).any(0)
    diff = float(np.abs(l32 - l64)[~flipped].max())
    share = a32.mean() / M.ESTIMATOR_RUN["steps_per_stage"]
    print(f"{name}: accepted {share:.3f}, {int(flipped.sum())} of {flipped.size} chains decide differently in fp32 and fp64, "
          f"max |logw32 - logw64| = {diff:.6g} (recorded {M.FP32_VS_FP64[name]:.6g}), smallest margin {m32:.3g} / {m64:.3g}")
    assert int(flipped.sum()) == M.FP32_VS_FP64_FLIPS[name] == 0
    assert abs(diff - M.FP32_VS_FP64[name]) <= 1e-3 * M.FP32_VS_FP64[name]
    assert np.isfinite(l32).all() and (s32[:, 3] == M.ESTIMATOR_RUN["replicas"]).all()
    assert a32.shape == (M.ESTIMATOR_RUN["stages"] - 1, A.N_DATA * M.ESTIMATOR_RUN["replicas"])
    assert 0.6 < share < 0.95                                              # both branches are taken, often
    assert M.ESTIMATOR_RUN["lr"] == 0.1 and M.estimator_tolerance(name) == 10.0 * M.FP32_VS_FP64[name]


def test_the_unadjusted_restatement_is_ais_cases_own():
    got = M.estimator_reference("gauss_tanh", lr=A.ESTIMATOR_RUN["lr"], adjust=None)
    want = A.estimator_reference("gauss_tanh")
    assert len(got) == 2 and np.array_equal(got[0].view(np.int64), want[0].view(np.int64))


def test_a_vanishing_step_size_accepts_every_proposal():
    _, _, acc, _ = M.estimator_reference("bern_relu", lr=1e-8)
    assert (acc == M.ESTIMATOR_RUN["steps_per_stage"]).all()


@pytest.mark.parametrize("lr", M.KAT_LRS)
def test_the_kat_errors_of_the_mala_restatement_are_the_recorded_ones(lr):
    errs, signed, share = M.kat_errors(lr)
    print(f"KAT, MALA restatement, lr {lr}: max |err| per seed", np.round(errs, 6), f"mean signed {signed:.4f}, acceptance {share:.3f}")
    np.testing.assert_allclose(errs, M.KAT_ERRORS[lr], rtol=0, atol=1e-4)
    assert M.KAT_TOL[lr] == 2.0 * max(M.KAT_ERRORS[lr]) and len(M.KAT_ERRORS[lr]) == 8
    assert abs(signed) < 0.05                                              # no bias to speak of: the unadjusted -0.19 and -0.82 are gone
    for seed in range(8):
        assert (np.abs(A.log_p(M.kat_run(seed, lr)[1]) - A.kat_exact()) <= M.KAT_TOL[lr]).all()


def test_the_kat_at_a_large_step_cannot_be_met_without_the_adjustment():
    errs, signed, _ = M.kat_errors(0.15, None)
    print("KAT, unadjusted restatement, lr 0.15: max |err| per seed", np.round(errs, 6), f"mean signed {signed:.4f}")
    np.testing.assert_allclose(errs, M.KAT_UNADJUSTED_ERRORS[0.15], rtol=0, atol=1e-4)
    assert M.KAT_TOL[0.15] < min(M.KAT_UNADJUSTED_ERRORS[0.15]), "the case does not tell an adjusted run from an unadjusted one"
    assert signed < -0.5
    # at the KAT's own step size the unadjusted restatement is ais_cases': the recorded bias
    np.testing.assert_allclose(M.kat_errors(0.05, None, seeds=range(2))[0], A.KAT_ERRORS[:2], rtol=0, atol=1e-4)

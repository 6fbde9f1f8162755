"""The Hamiltonian transition of L leapfrog steps and annealed importance sampling with it, as far as no device is needed: properties of
the restatement of tests/hmc_cases.py, the Philox block of the decision's uniform, what `leapfrog` refuses, the three entry points in
the header, the binding and csrc, and every figure tests/hmc_cases.py records, recomputed."""
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
from tests import hmc_cases as H
from tests import mala_cases as M
from tests import smc_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mcpc_hmc_begin", "mcpc_hmc_leap", "mcpc_hmc_accept")


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def test_the_fp32_elements_round_operation_by_operation():
    rng = np.random.default_rng(5)
    x, g, z, gt = (rng.standard_normal((7, 13)).astype(np.float32) for _ in range(4))
    lr, f = 0.1, np.float32
    eps = f(np.sqrt(2.0 * lr))
    h = f(f(0.5) * eps)
    assert float(h) * 2.0 == float(eps)                                    # h is exact
    q, x1 = H.begin(x, g, z, lr)
    q2, x2 = H.leap(x1, q, gt, lr)
    p_end = H.end_momentum(q2, gt, lr)
    for i in np.ndindex(x.shape):                                          # element by element, a rounding after every operation
        qi = f(z[i] - f(h * g[i]))
        xi = f(x[i] + f(eps * qi))
        assert qi == q[i] and xi == x1[i]
        qj = f(qi - f(eps * gt[i]))
        xj = f(xi + f(eps * qj))
        assert qj == q2[i] and xj == x2[i]
        assert f(qj - f(h * gt[i])) == p_end[i]
    assert all(t.dtype == np.float32 for t in (q, x1, q2, x2, p_end))
    # one leapfrog step ends at the MALA proposal at noise_var = 2, but for roundoff
    assert np.abs(x1 - M.propose(x, g, z, lr, 2.0)).max() < 4 * 2.0 ** -24 * np.abs(x1).max()
    q64, x64 = H.begin(x, g, z, lr, np.float64)
    exact = x.astype(np.float64) - lr * g.astype(np.float64) + np.sqrt(2.0 * lr) * z.astype(np.float64)
    assert np.abs(x64 - exact).max() < 1e-15 and q64.dtype == np.float64


def test_a_trajectory_run_backwards_returns_to_its_start():
    """Leapfrog is reversible: from (x_L, -p') the same steps end at (x, -p) -- in fp64 to roundoff.  The gradient of a quadratic."""
    rng = np.random.default_rng(6)
    A_ = rng.standard_normal((9, 9))
    A_ = A_ @ A_.T / 9.0 + np.eye(9)
    grad = lambda x: x @ A_                                                 # noqa: E731
    x0, p0 = rng.standard_normal((4, 9)), rng.standard_normal((4, 9))
    def trajectory(x, p, lr=0.02, Ls=5):
        q, xt = H.begin(x, grad(x), p, lr, np.float64)
        for _ in range(Ls - 1):
            q, xt = H.leap(xt, q, grad(xt), lr, np.float64)
        return xt, H.end_momentum(q, grad(xt), lr, np.float64)
    xL, pL = trajectory(x0, p0)
    xb, pb = trajectory(xL, -pL)
    assert np.abs(xb - x0).max() < 1e-13 and np.abs(pb + p0).max() < 1e-13
    # and the scheme is of second order: the same time in steps of half the size (a quarter of lr) errs four times less in H
    Hs = lambda x, p: 0.5 * np.einsum("ri,ij,rj->r", x, A_, x) + 0.5 * (p * p).sum(1)     # noqa: E731
    coarse = np.abs(Hs(x0, p0) - Hs(xL, pL))
    fine = np.abs(Hs(x0, p0) - Hs(*trajectory(x0, p0, 0.005, 10)))
    assert (fine < 0.3 * coarse).all() and (fine > 0.2 * coarse).all()


def test_a_nan_log_alpha_rejects_and_log_alpha_is_three_roundings():
    E, Et, K0 = np.array([3.0, np.nan, 1.0]), np.array([2.5, 1.0, 1.0]), np.array([7.0, 1.0, np.inf])
    ps = [np.array([[1.0, 2.0], [1.0, 1.0], [np.inf, 0.0]], dtype=np.float32)]
    la, Mr = H.log_alpha(E, Et, K0, ps)
    assert la[0] == (3.0 - 2.5) + (7.0 - 2.5) and Mr[0] == 3.0 + 2.5 + 7.0 + 2.5
    assert np.isnan(la[1]) and np.isnan(la[2])                              # Inf - Inf
    assert H.decide(la, np.array([0.5, 0.5, 0.5])).tolist() == [True, False, False]


# ---- the uniform's Philox block --------------------------------------------------------------------------------------------------------
def test_the_uniform_is_word_0_of_the_block_of_layer_0xfd():
    r = H.KERNEL_RUN
    seed, step, base = r["seed"], r["step"], r["chain_base"]
    w = philox.philox4x32_10(np.arange(base, base + 19, dtype=np.uint32), np.uint32(0xFD << 24), np.uint32(step & 0xFFFFFFFF),
                             np.uint32(step >> 32), np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32))[0]
    u = H.uniform(seed, step, base, 19)
    np.testing.assert_array_equal(u, ((w >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24)
    assert u.dtype == np.float64 and (u > 0).all() and (u <= 1).all()
    np.testing.assert_array_equal(H.uniform(seed, step, base + 5, 14), u[5:])            # a chain's uniform is its own
    assert not np.array_equal(u, M.uniform(seed, step, base, 19))                        # and not MALA's


def test_layer_0xfd_is_used_by_nothing_else():
    assert H.UNIFORM_LAYER == 0xFD and len({H.UNIFORM_LAYER, S.UNIFORM_LAYER, M.UNIFORM_LAYER}) == 3
    assert H.UNIFORM_LAYER > L.MAX_LATENT and H.MAX_LATENT == L.MAX_LATENT
    csrc = os.path.join(ROOT, "montecarlopredictivecoding_amd", "csrc")
    assert re.search(r"kHmcLayer = 0xFDu", open(os.path.join(csrc, "mcpc_hmc.h")).read())
    for name in ("mcpc_hmc.h", "mcpc_mala.h", "mcpc_smc.h"):                             # each header says who takes which layer
        text = open(os.path.join(csrc, name)).read()
        assert "0xFD" in text and "0xFE" in text and "0xFF" in text, name


# ---- what the call refuses ----------------------------------------------------------------------------------------------------------------
def _trainer():
    model = nn.Sequential(nn.Linear(6, 16), pc.PCLayer(), nn.Tanh(), nn.Linear(16, 24))
    model.train()
    return pc.PCTrainer(model, T=4, optimizer_x_fn=torch.optim.SGD, optimizer_x_kwargs={"lr": 0.03}, update_p_at="never", plot_progress_at=[])


BAD = [dict(leapfrog=0, adjust="mala"), dict(leapfrog=-3, adjust="mala"), dict(leapfrog=2.0, adjust="mala"), dict(leapfrog=True, adjust="mala"),
       dict(leapfrog="5", adjust="mala"), dict(leapfrog=None, adjust="mala"), dict(leapfrog=0), dict(leapfrog=2), dict(leapfrog=2, adjust=None),
       dict(leapfrog=2, adjust="mala", noise_var=1.0), dict(leapfrog=5, adjust="mala", noise_var=2.5)]


@pytest.mark.parametrize("kw", BAD, ids=[repr(sorted(k.items())) for k in BAD])
def test_a_bad_leapfrog_is_a_value_error_before_any_device_is_asked_for(kw):
    tr = _trainer()
    with pytest.raises(ValueError, match="leapfrog"):
        tr.mcpc_ais(torch.zeros(3, 24), um.fe_fn, {"_var": 0.7}, **kw)
    with pytest.raises(ValueError, match="leapfrog"):
        ais.check_leapfrog(kw["leapfrog"], kw.get("adjust"), kw.get("noise_var", 2.0))
    assert tr.mcpc_last_ais_acceptance is None


def test_good_leapfrog_values_pass_the_check_and_reach_the_device():
    assert ais.check_leapfrog(1) == 1 and ais.check_leapfrog(1, None, 0.5) == 1 and ais.check_leapfrog(1, "mala", 0.5) == 1
    assert ais.check_leapfrog(2, "mala") == 2 and ais.check_leapfrog(7, "mala", 2) == 7
    if torch.cuda.is_available():
        return                                                   # (tests/test_gpu_hmc_ais.py runs them)
    with pytest.raises(L.MCPCLibraryError):
        _trainer().mcpc_ais(torch.zeros(3, 24), um.fe_fn, {"_var": 0.7}, replicas=4, stages=3, adjust="mala", leapfrog=3)


def test_a_trajectory_takes_one_philox_step_whatever_its_length():
    """ais.engine_calls accounts for the Philox steps of a call; `leapfrog` does not enter it, and the restatement walks the same steps:
    the uniforms of rung k's transitions are those of steps step_base + 1 + (k - 1) steps_per_stage + t."""
    kw = dict(n_data=5, replicas=16, max_chains=80, n_rungs=8, steps_per_stage=4, step_base=100, chain_base=40)
    calls = ais.engine_calls(**kw)
    assert [c[2] for c in calls] == [100] + [101 + 4 * k for k in range(7)]
    uniforms = {(c, H.UNIFORM_LAYER << 24, 101 + s) for c in range(40, 120) for s in range(7 * 4)}
    mala = {(c, M.UNIFORM_LAYER << 24, t) for c, _, t in uniforms}
    smc = {(c, S.UNIFORM_LAYER << 24, t) for c, _, t in uniforms}
    assert not (uniforms & mala) and not (uniforms & smc) and len(uniforms) == 80 * 28


# ---- the entry points -----------------------------------------------------------------------------------------------------------------------
def _c_types(decl):
    """The argument list of a C declaration as the ctypes the binding should hold."""
    out = []
    for arg in decl.split(","):
        arg = " ".join(arg.split())
        if "* const*" in arg:
            out.append(L.C.POINTER(L.C.c_void_p))
        elif arg.startswith("const int32_t*") and "widths" in arg:
            out.append(L.C.POINTER(L.C.c_int32))
        elif "*" in arg:
            out.append(L.C.c_void_p)
        else:
            out.append({"int": L.C.c_int, "int32_t": L.C.c_int32, "int64_t": L.C.c_int64, "uint64_t": L.C.c_uint64,
                        "double": L.C.c_double}[arg.split()[0]])
    return out


def test_the_header_the_binding_and_csrc_agree_on_the_three_signatures():
    header = open(os.path.join(ROOT, "include", "mcpc.h")).read()
    source = open(os.path.join(ROOT, "montecarlopredictivecoding_amd", "csrc", "mcpc_records.hip")).read()
    norm = lambda s: " ".join(s.replace("stream_", "stream").split())      # noqa: E731
    for name in ENTRIES:
        decl = re.search(r"^int " + name + r"\((.*?)\);", header, re.M | re.S).group(1)
        defn = re.search(r"^int " + name + r"\((.*?)\) \{", source, re.M | re.S).group(1)
        assert decl.startswith("int device,") and norm(decl) == norm(defn), name
        assert name in L.SYMBOLS and L.SYMBOLS[name][0] is L.C.c_int
        assert L.SYMBOLS[name][1] == _c_types(decl), name
    assert re.search(r"#define MCPC_ABI_VERSION 4\b", header) and L.ABI_VERSION == 4
    assert "#define MCPC_HMC_MAX_ROWS 2147483647LL" in header
    assert '#include "mcpc_hmc.h"' in source
    from montecarlopredictivecoding_amd import engine
    assert callable(engine.hmc_begin) and callable(engine.hmc_leap) and callable(engine.hmc_accept)


# ---- the recorded figures --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(H.KERNEL_CASES))
def test_the_kernel_cases_decide_far_from_roundoff_and_accept_about_half(name):
    c = H.KERNEL_CASES[name]
    assert c == M.KERNEL_CASES[name] and H.KERNEL_RUN["step"] == (1 << 32) + 7 and H.KERNEL_RUN["chain_base"] == 1000
    assert 1 <= len(c["widths"]) <= H.MAX_LATENT and sum(c["widths"]) + 10 <= 2 ** 11 and sum(c["widths"]) <= H.MAX_UNITS
    la, Mr, u, acc = H.kernel_reference(name)
    dist = np.abs(np.log(u) - la)
    need = H.margin_needed(Mr, u)
    print(f"{name}: accepted {int(acc.sum())} of {acc.size}, smallest |log u - log_alpha| = {dist.min():.3g}, needed {need.max():.3g}")
    assert (dist > need).all()
    if name in H.SHARE_CASES:
        assert 0.25 <= acc.mean() <= 0.75, acc.mean()
    elif name == "one_row_accepts":
        assert acc.all() and (la > 0).all()
    else:
        assert not acc.any() and (la < 24 * np.log(0.5)).all()
    # the inputs are a trajectory's: (q, x_t) is BEGIN from (x, g) with the momentum whose kinetic energy is K0
    xs, gs, _, xts, _, _, qs, K0 = H.kernel_inputs(name)
    p0 = [(q.astype(np.float64) + 0.5 * float(H.step_sizes(H.KERNEL_RUN["lr"])[0]) * g) for q, g in zip(qs, gs)]
    assert np.abs(H.kinetic(p0) - K0).max() <= 1e-5 * K0.max()


@pytest.mark.parametrize("name", sorted(A.ESTIMATOR_CASES))
def test_the_leapfrog_restatement_stays_where_it_was_measured(name):
    l32, s32, a32, m32 = H.estimator_reference(name, "float32")
    l64, _, a64, m64 = H.estimator_reference(name, "float64")
    flipped = (a32 != a64).any(0)
    diff = float(np.abs(l32 - l64)[~flipped].max())
    share = a32.mean() / H.ESTIMATOR_RUN["steps_per_stage"]
    print(f"{name}: accepted {share:.3f}, {int(flipped.sum())} of {flipped.size} chains decide differently in fp32 and fp64, "
          f"max |logw32 - logw64| = {diff:.6g} (recorded {H.FP32_VS_FP64[name]:.6g}), smallest margin {m32:.3g} / {m64:.3g}")
    assert int(flipped.sum()) == H.FP32_VS_FP64_FLIPS[name] <= H.MAX_FLIPPED == 4 and flipped.size == 80
    assert abs(diff - H.FP32_VS_FP64[name]) <= 1e-3 * H.FP32_VS_FP64[name]
    assert np.isfinite(l32).all() and (s32[:, 3] == H.ESTIMATOR_RUN["replicas"]).all()
    assert a32.shape == (H.ESTIMATOR_RUN["stages"] - 1, A.N_DATA * H.ESTIMATOR_RUN["replicas"])
    assert abs(share - H.ACCEPTANCE[name]) < 1e-3 and 0.6 < share < 0.95    # both branches are taken, often
    assert (a32 < H.ESTIMATOR_RUN["steps_per_stage"]).any() and (a32 > 0).any()
    assert H.ESTIMATOR_RUN == dict(M.ESTIMATOR_RUN, leapfrog=3) and H.estimator_tolerance(name) == 10.0 * H.FP32_VS_FP64[name]


@pytest.mark.parametrize("name", sorted(A.ESTIMATOR_CASES))
def test_one_leapfrog_step_is_the_mala_step(name):
    """estimator(leapfrog=1) IS the MALA restatement; and the leapfrog ladder itself, at one step in fp64 with MALA's uniform, takes the
    MALA restatement's decisions with log-weights within 1e-12: a strict generalisation."""
    want = M.estimator_reference(name, "float64")
    same = H.estimator_reference(name, "float64", leapfrog=1)
    assert np.array_equal(same[0].view(np.int64), want[0].view(np.int64)) and np.array_equal(same[2], want[2])
    c = A.ESTIMATOR_CASES[name]
    W, b, data = A.estimator_params(name)
    r = dict(M.ESTIMATOR_RUN)
    stages = r.pop("stages")
    got = H.leapfrog_ladder(W, b, c["sizes"], [c["act"]] * len(c["sizes"]), c["n_in"], data, c["loss"], c["var"], c["mask_start"],
                            betas=A.schedule(stages), dtype=np.float64, leapfrog=1, uniform_of=M.uniform, **r)
    print(f"{name}: max |logw(one leapfrog step) - logw(MALA)| = {np.abs(got[0] - want[0]).max():.3g}")
    np.testing.assert_array_equal(got[2], want[2])
    assert np.abs(got[0] - want[0]).max() <= 1e-12
    # three steps move the chains elsewhere
    assert not np.array_equal(H.estimator_reference(name, "float64")[2], want[2])


def test_a_vanishing_step_size_accepts_every_trajectory():
    _, _, acc, _ = H.estimator_reference("bern_relu", lr=1e-8)
    assert (acc == H.ESTIMATOR_RUN["steps_per_stage"]).all()


def test_the_kat_errors_of_the_leapfrog_restatement_are_the_recorded_ones():
    errs, signed, share = H.kat_errors()
    print("KAT, leapfrog restatement", H.KAT_RUN, ": max |err| per seed", np.round(errs, 6), f"mean signed {signed:.4f}, acceptance {share:.3f}")
    np.testing.assert_allclose(errs, H.KAT_ERRORS, rtol=0, atol=1e-4)
    assert H.KAT_TOL == 2.0 * max(H.KAT_ERRORS) and len(H.KAT_ERRORS) == 8
    assert H.KAT_RUN == dict(lr=0.15, leapfrog=5, steps_per_stage=2)
    assert H.KAT_RUN["leapfrog"] * H.KAT_RUN["steps_per_stage"] == A.KAT["steps_per_stage"]      # ten gradient evaluations per rung
    assert H.KAT_TOL < min(M.KAT_UNADJUSTED_ERRORS[0.15]), "the case does not tell an adjusted run from an unadjusted one"
    assert abs(signed) < 0.05 and 0.5 < share <= 1.0
    for seed in range(8):
        assert (np.abs(A.log_p(H.kat_run(seed)[1]) - A.kat_exact()) <= H.KAT_TOL).all()


def test_the_closed_form_figures_are_the_recorded_ones_and_mala_misses_the_bound():
    e_h, ess_h, acc_h = H.cf_errors("hmc")
    e_m, ess_m, acc_m = H.cf_errors("mala")
    rms_h, rms_m = float(np.sqrt((e_h ** 2).mean())), float(np.sqrt((e_m ** 2).mean()))
    print(f"closed form: 5 MALA steps rms {rms_m:.6f} max {np.abs(e_m).max():.4f} ESS {ess_m.min():.1f} .. {ess_m.max():.1f} acceptance "
          f"{acc_m:.3f}; 1 x 5 leapfrog steps rms {rms_h:.6f} max {np.abs(e_h).max():.4f} ESS {ess_h.min():.1f} .. {ess_h.max():.1f} "
          f"acceptance {acc_h:.3f}; bound {H.cf_rms_bound():.4f}, tolerance {H.cf_tol():.4f}")
    assert abs(rms_h - H.CF_RMS["hmc"]) <= 1e-4 and abs(rms_m - H.CF_RMS["mala"]) <= 1e-4
    np.testing.assert_allclose(np.abs(e_h).max(1), H.CF_ERRORS, rtol=0, atol=1e-4)
    assert H.cf_tol() == 2.0 * max(H.CF_ERRORS) and H.cf_rms_bound() == (H.CF_RMS["hmc"] * H.CF_RMS["mala"]) ** 0.5
    assert H.CF_RUNS == {"hmc": dict(leapfrog=5, steps_per_stage=1), "mala": dict(leapfrog=1, steps_per_stage=5)} and H.CF is S.CF
    # the bound separates the two: the trajectory meets it, five MALA steps miss it, and so does a single leapfrog step per rung
    assert rms_h < H.cf_rms_bound() < rms_m
    W, b, data = S.cf_params()
    one = [H.estimator(W, b, (S.CF["n_latent"],), ["identity"], 1, data, "gaussian", S.CF["var"], 0, replicas=S.CF["replicas"],
                       betas=A.schedule(S.CF["stages"], S.CF["power"]), lr=S.CF["lr"], seed=seed, leapfrog=1, steps_per_stage=1)
           for seed in S.CF_SEEDS]
    e_1 = np.stack([A.log_p(r[1]) - S.cf_exact() for r in one])
    assert float(np.sqrt((e_1 ** 2).mean())) > H.cf_rms_bound()

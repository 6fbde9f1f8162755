"""Resampling in annealed importance sampling, everything that needs no device: the properties of the restatement of
tests/smc_cases.py itself, the Philox block of the resampling uniform, what `ais.run` refuses before a device is asked for, the two
entry points in the header and the binding, and every figure tests/smc_cases.py records, recomputed."""
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
from tests import smc_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = S.KERNEL_RUN
SHAPES = [(R, n) for R in S.KERNEL_REPLICAS for n in S.KERNEL_DATA]


# ---- the restatement's own properties -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,n", SHAPES)
def test_offspring_counts_are_floor_or_ceil_sum_to_r_and_ancestors_are_sorted(R, n):
    r = S.resample(S.kernel_logw(R, n), R, 1.0, **K)
    a = r.ancestors.reshape(n, R) - (np.arange(n) * R)[:, None]
    assert (a >= 0).all() and (a < R).all() and (np.diff(a, axis=1) >= 0).all()
    for i in range(n):
        if r.diag[i, 1]:
            counts, low, high = S.offspring_bounds(r.e[i], r.S[i], a[i])
            assert counts.sum() == R and (counts >= low).all() and (counts <= high).all()
        else:
            assert R == 1 and np.array_equal(a[i], np.arange(R))          # equal weights: ess = R is not below R


def test_zero_weight_replicas_are_never_chosen_and_a_datum_without_weights_is_untouched():
    R, n = 16, 5
    logw = np.asarray(S.kernel_logw(R, n)).copy()
    bad = [5, R - 1, 2 * R, 4 * R + 7]
    logw[bad] = [np.nan, np.inf, -np.inf, np.nan]
    logw[R:2 * R] = np.nan                                              # datum 1: cnt = 0
    logw[3 * R:3 * R + 4] = -2000.0                                     # finite, but exp underflows to 0: counted, never chosen
    r = S.resample(logw, R, 1.0, **K)
    assert not np.isin(r.ancestors, bad).any() and not np.isin(r.ancestors, np.arange(3 * R, 3 * R + 4)).any()
    rows = slice(R, 2 * R)
    assert np.array_equal(r.ancestors[rows], np.arange(R, 2 * R)) and np.isnan(r.logw[rows]).all()
    assert np.isnan(r.diag[1, 0]) and r.diag[1, 1] == 0.0 and np.isnan(r.diag[1, 3]) and 0.0 < r.diag[1, 2] < 1.0
    assert (r.diag[[0, 2, 3, 4], 1] == 1.0).all() and np.isfinite(np.delete(r.logw, np.arange(R, 2 * R))).all()
    # the log of the mean over the FINITE replicas, the ones ais.fold counts: 16 in datum 3, 14 in datum 0
    for i, cnt in ((3, 16), (0, 14)):
        w = logw[i * R:(i + 1) * R]
        w = w[np.isfinite(w)]
        assert w.size == cnt and abs(r.logw[i * R] - (w.max() + np.log(np.exp(w - w.max()).sum() / cnt))) < 1e-12


def test_a_last_position_at_the_total_is_clamped_to_the_last_positive_weight():
    # u just below 1 and trailing zero weights: p_{R-1} rounds to S or beyond no replica; the clamp keeps the ancestor alive
    logw = np.array([0.0, 0.0, -np.inf, np.nan])
    for step in range(200):
        r = S.resample(logw, 4, 1.0, 7, step, 0)
        assert set(r.ancestors) <= {0, 1} and np.bincount(r.ancestors, minlength=2).tolist() == [2, 2]


def test_threshold_zero_never_resamples_and_the_uniform_is_the_block_of_layer_0xfe():
    for R, n in SHAPES:
        r = S.resample(S.kernel_logw(R, n), R, 0.0, **K)
        assert not r.diag[:, 1].any() and np.array_equal(r.ancestors, np.arange(n * R))
        assert np.array_equal(r.logw.view(np.int64), np.asarray(S.kernel_logw(R, n)).view(np.int64))
    # the uniform: word 0 of the block (chain, (0xFE << 24) | 0, step lo, step hi; seed), on a 24-bit grid shifted by half a cell
    seed, step, chain = K["seed"], K["step"], K["chain_base"] + 65
    w = philox.philox4x32_10(np.uint32(chain), np.uint32(0xFE << 24), np.uint32(step & 0xFFFFFFFF), np.uint32(step >> 32),
                             np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32))[0]
    u = S.uniform(seed, step, chain)
    assert u == (int(w) >> 8) * 2.0 ** -24 + 2.0 ** -25 and 0.0 < u < 1.0
    assert S.UNIFORM_LAYER == 0xFE != M.UNIFORM_LAYER and S.UNIFORM_LAYER > L.MAX_LATENT          # no normal, no prior draw, no MALA uniform
    header = open(os.path.join(ROOT, "montecarlopredictivecoding_amd", "csrc", "mcpc_smc.h")).read()
    assert "kSmcLayer = 0xFEu" in header and "0xFF" in header


def test_the_estimator_without_resampling_is_the_one_it_is_built_on():
    for name in sorted(A.ESTIMATOR_CASES):
        l, st, _ = S.estimator_reference(name, None, None)
        l0, st0 = A.estimator_reference(name)
        assert np.array_equal(l.view(np.int64), l0.view(np.int64)) and np.array_equal(st, st0)
    c = A.ESTIMATOR_CASES["gauss_tanh"]
    W, b, data = A.estimator_params("gauss_tanh")
    r = dict(S.ESTIMATOR_RUN)
    kw = dict(betas=A.schedule(r.pop("stages")), **r)
    args = (W, b, c["sizes"], [c["act"]] * 2, c["n_in"], data, c["loss"], c["var"], c["mask_start"])
    l, _, tr = S.estimator(*args, adjust="mala", **kw)
    l0, _, acc0, _ = M.estimator(*args, adjust="mala", **kw)
    assert np.array_equal(l.view(np.int64), l0.view(np.int64)) and np.array_equal(tr.accepted, acc0)


# ---- what the call refuses ------------------------------------------------------------------------------------------------------------------
def _trainer():
    model = nn.Sequential(nn.Linear(6, 16), pc.PCLayer(), nn.Tanh(), nn.Linear(16, 24))
    model.train()
    return pc.PCTrainer(model, T=4, optimizer_x_fn=torch.optim.SGD, optimizer_x_kwargs={"lr": 0.03}, update_p_at="never", plot_progress_at=[])


@pytest.mark.parametrize("kw,match", [
    (dict(resample="multinomial"), "resample"), (dict(resample="Systematic"), "resample"), (dict(resample=True), "resample"),
    (dict(resample=1), "resample"), (dict(resample=b"systematic"), "resample"),
    (dict(resample="systematic", ess_threshold=-0.01), "ess_threshold"), (dict(resample="systematic", ess_threshold=1.01), "ess_threshold"),
    (dict(ess_threshold=2.0), "ess_threshold"), (dict(resample="systematic", ess_threshold=float("nan")), "ess_threshold"),
    (dict(resample="systematic", ess_threshold="0.5"), "ess_threshold"), (dict(resample="systematic", ess_threshold=True), "ess_threshold"),
    (dict(resample="systematic", replicas=4097), "replicas"),
])
def test_a_bad_resampling_keyword_is_a_value_error_before_any_device_is_asked_for(kw, match, monkeypatch):
    tr = _trainer()
    monkeypatch.setattr(tr, "_plan_or_raise", lambda *a, **k: pytest.fail("a device was asked for"))
    tr.mcpc_last_ais_resampling = "stale"
    with pytest.raises(ValueError, match=match):
        tr.mcpc_ais(torch.zeros(3, 24), um.fe_fn, {"_var": 0.7}, **kw)
    assert tr.mcpc_last_ais_resampling is None
    with pytest.raises(ValueError, match=match):
        ais.check_resample(kw.get("resample"), kw.get("ess_threshold", 0.5), kw.get("replicas", 64))


def test_good_resampling_keywords_pass_the_check_and_reach_the_device():
    assert ais.check_resample(None, 0.5, 64) == (None, 0.5) and ais.check_resample("systematic", 1, 4096) == ("systematic", 1.0)
    assert ais.check_resample(None, 0.0, 5000) == (None, 0.0)            # the cap holds only when resampling
    assert _trainer().mcpc_last_ais_resampling is None
    if torch.cuda.is_available():
        return                                                          # (tests/test_gpu_smc_ais.py runs them)
    with pytest.raises(L.MCPCLibraryError):
        _trainer().mcpc_ais(torch.zeros(3, 24), um.fe_fn, {"_var": 0.7}, replicas=4, stages=3, resample="systematic", ess_threshold=1.0)


# ---- the entry points -----------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_both_entry_points_and_the_binding_binds_them():
    header = open(os.path.join(ROOT, "include", "mcpc.h")).read()
    for name in ("mcpc_smc_ancestors", "mcpc_smc_gather"):
        assert re.search(r"^int " + name + r"\(int device,", header, re.M), name
        assert name in L.SYMBOLS and L.SYMBOLS[name][0] is L.C.c_int
        decl = re.search(r"^int " + name + r"\((.*?)\);", header, re.M | re.S).group(1)
        assert len(decl.split(",")) == len(L.SYMBOLS[name][1]), name
    assert re.search(r"#define MCPC_SMC_MAX_REPLICAS %d\b" % L.SMC_MAX_REPLICAS, header) and L.SMC_MAX_REPLICAS == S.MAX_REPLICAS == 4096
    assert "#define MCPC_SMC_MAX_ROWS" in header
    from montecarlopredictivecoding_amd import engine
    assert callable(engine.smc_ancestors) and callable(engine.smc_gather)


# ---- the recorded figures -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threshold", S.KERNEL_THRESHOLDS)
@pytest.mark.parametrize("R,n", SHAPES)
def test_the_kernel_cases_leave_no_slot_and_no_decision_out(R, n, threshold):
    r = S.kernel_reference(R, n, threshold)
    assert (r.slot_margin > S.SLOT_MARGIN).all()
    assert (r.ess_margin > S.ESS_MARGIN).all() or R == 1                # R = 1: ess = 1 exactly, whatever exp is
    if n == 5 and R > 1 and threshold == 0.5:
        assert 0 < r.diag[:, 1].sum() < n                               # both branches
    if threshold == 1.0 and R > 1:
        assert r.diag[:, 1].all()


@pytest.mark.parametrize("key", sorted(S.ESTIMATOR_FIGURES, key=repr))
def test_the_estimator_figures_are_the_recorded_ones(key):
    pairs, dmax, differ, ess_margin, slot_margin = S.estimator_figures(*key)
    want = S.ESTIMATOR_FIGURES[key]
    print(key, pairs, dmax, differ, ess_margin, slot_margin)
    assert (pairs, differ) == (want[0], want[2]) and differ == 0        # fp32 and fp64 take the same decisions everywhere
    assert abs(dmax - want[1]) <= 1e-5 * want[1]
    assert abs(ess_margin - want[3]) <= 0.01 * want[3] and abs(slot_margin - want[4]) <= 0.01 * want[4]
    assert ess_margin > 2.0 ** -20 and slot_margin > 2.0 ** -22         # far above roundoff: no datum is expected to be left out


def test_both_branches_are_taken_at_threshold_one_half_and_every_pair_resamples_at_one():
    n = (S.ESTIMATOR_RUN["stages"] - 1) * A.N_DATA
    assert 0 < S.ESTIMATOR_FIGURES[("gauss_tanh", 0.5, None)][0] < n
    assert all(S.ESTIMATOR_FIGURES[(name, 1.0, adj)][0] == n for name in A.ESTIMATOR_CASES for adj in S.ADJUSTS)
    _, st, _ = S.estimator_reference("gauss_tanh", 0.5)
    _, st0 = A.estimator_reference("gauss_tanh")
    assert A.ess(st).min() > A.ess(st0).max()                           # 6.5 .. 13.1 against 1.9 .. 3.3


def test_the_closed_form_figures_are_the_recorded_ones_and_plain_ais_misses_the_bound():
    exact = S.cf_exact()
    # the exact value against a Monte Carlo free check: the quadratic form through the Woodbury identity
    W, _, data = S.cf_params()
    Wd, yd, v = W[1].astype(np.float64), data.astype(np.float64), S.CF["var"]
    A_ = np.eye(S.CF["n_latent"]) + Wd.T @ Wd / v
    quad = (yd * yd).sum(1) / v - ((yd @ Wd / v) * np.linalg.solve(A_, (yd @ Wd / v).T).T).sum(1)
    logdet = np.linalg.slogdet(A_)[1] + S.CF["n_out"] * np.log(v)
    np.testing.assert_allclose(exact, -0.5 * (quad + logdet + S.CF["n_out"] * np.log(2 * np.pi)), rtol=0, atol=1e-10)
    plain, ess0 = S.cf_errors(None)
    res, ess1 = S.cf_errors(S.CF["threshold"])
    rms0, rms1 = np.sqrt((plain ** 2).mean()), np.sqrt((res ** 2).mean())
    print("plain", rms0, "resampled", rms1, "errors", np.abs(res).max(1))
    np.testing.assert_allclose(np.abs(res).max(1), S.CF_ERRORS, rtol=0, atol=2e-6)
    np.testing.assert_allclose([rms0, rms1], [S.CF_RMS["plain"], S.CF_RMS["resampled"]], rtol=0, atol=2e-6)
    assert rms0 / rms1 >= 1.5 and rms1 < S.cf_rms_bound() < rms0        # the plain estimator misses the bound
    assert ess1.min() > ess0.max()                                      # 23.3 .. 58.8 against 1.0 .. 6.9
    assert S.CF["n_data"] * S.CF["replicas"] <= 256 and (S.CF["stages"] - 1) * S.CF["steps_per_stage"] <= 75

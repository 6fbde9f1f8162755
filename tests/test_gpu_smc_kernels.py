"""The two resampling entry points on the device (include/mcpc.h: mcpc_smc_ancestors, mcpc_smc_gather; csrc/mcpc_smc.h) against the
restatement of tests/smc_cases.py: ancestors and decisions exactly wherever the restatement is far from a tie, the new log-weight at
its roundoff bound, the four columns of diag, the properties that do not depend on exp (offspring bounds, identity above the
threshold, threshold 0), special values, independence of the other data and of the run, the gather bitwise with its out-of-range
counter and canaries, and every refusal the header lists."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import smc_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 7                                  # sentinel elements behind every output
SENTINEL = -777
K = S.KERNEL_RUN
SHAPES = [(R, n) for R in S.KERNEL_REPLICAS for n in S.KERNEL_DATA]


def guarded(a, dtype):
    """(whole, view): a device copy of ``a`` (any shape, flattened rows first) with GUARD sentinels behind it, and the view of ``a``."""
    a = np.asarray(a)
    whole = torch.full((a.size + GUARD,), SENTINEL, dtype=dtype, device=DEV)
    whole[:a.size] = torch.tensor(a.reshape(-1)).to(device=DEV, dtype=dtype)
    return whole, whole[:a.size].view(a.shape)


def guards_intact(*wholes):
    return all(bool((w[-GUARD:] == SENTINEL).all()) for w in wholes)


def bits64(t):
    return t.detach().cpu().contiguous().view(torch.int64).numpy()


def ancestors(logw, R, threshold, chain_base=K["chain_base"]):
    """One smc_ancestors on host log-weights, everything guarded: (ancestors int64, logw fp64, diag [n, 4]) as NumPy arrays."""
    from montecarlopredictivecoding_amd.engine import smc_ancestors
    logw = np.asarray(logw, dtype=np.float64)
    n = logw.shape[0] // R
    lw_whole, lw = guarded(logw, torch.float64)
    an_whole, an = guarded(np.full(n * R, SENTINEL, dtype=np.int32), torch.int32)
    dg_whole, dg = guarded(np.full((n, 4), SENTINEL, dtype=np.float64), torch.float64)
    got = smc_ancestors(lw, R, threshold, K["seed"], K["step"], chain_base, ancestors=an, diag=dg)
    torch.cuda.synchronize()
    assert got is an and guards_intact(lw_whole, an_whole, dg_whole)
    return an.cpu().numpy().astype(np.int64), lw.cpu().numpy(), dg.cpu().numpy()


# ---- against the restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threshold", S.KERNEL_THRESHOLDS)
@pytest.mark.parametrize("R,n", SHAPES)
def test_ancestors_decisions_log_weights_and_diag_follow_the_restatement(R, n, threshold):
    logw = S.kernel_logw(R, n)
    want = S.resample(logw, R, threshold, **K)
    anc, lw, dg = ancestors(logw, R, threshold)
    # decisions: exact wherever the restatement's ESS is far from the threshold (R = 1: ess is exactly 1 on both sides)
    sure = (want.ess_margin > S.ESS_MARGIN) | (R == 1)
    assert sure.all(), "the seeded case leaves a decision out"
    np.testing.assert_array_equal(dg[sure, 1], want.diag[sure, 1])
    # slots: exact wherever the position is far from a cumulative weight; at most 1 % may be left out (here: none)
    keep = (want.slot_margin > S.SLOT_MARGIN) & sure[:, None]
    assert (~keep).sum() <= 0.01 * keep.size
    np.testing.assert_array_equal(anc.reshape(n, R)[keep], want.ancestors.reshape(n, R)[keep])
    print(f"R {R} n {n} threshold {threshold}: resampled {int(dg[:, 1].sum())} of {n}, slots left out {int((~keep).sum())}, "
          f"max |logw - restatement| = {np.abs(lw - want.logw).max():.3g}, max |ess - restatement| = {np.abs(dg[:, 0] - want.diag[:, 0]).max():.3g}")
    # the new log-weight (and the untouched ones, which must be the old bits)
    took = want.diag[:, 1] != 0.0
    rows = np.repeat(took, R)
    assert (np.abs(lw - want.logw)[rows] <= S.logw_tolerance(want.logw, R)[rows]).all()
    assert np.array_equal(lw[~rows].view(np.int64), np.asarray(logw)[~rows].view(np.int64))
    # diag: ess and the log of the mean weight at the same roundoff scale, the uniform exactly
    assert (np.abs(dg[:, 0] - want.diag[:, 0]) <= 2.0 ** -53 * 4 * (R + 16) * want.diag[:, 0]).all()
    np.testing.assert_array_equal(dg[:, 2], want.diag[:, 2])
    assert (np.abs(dg[:, 3] - want.diag[:, 3]) <= S.logw_tolerance(want.diag[:, 3], R)).all()
    assert np.array_equal(lw[rows], np.repeat(dg[:, 3], R)[rows])         # the log-weight written is the one reported


# ---- properties that do not depend on exp ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,n", SHAPES)
def test_offspring_counts_are_floor_or_ceil_and_ancestors_are_sorted(R, n):
    logw = np.asarray(S.kernel_logw(R, n))
    anc, lw, dg = ancestors(logw, R, 1.0)
    a = anc.reshape(n, R) - (np.arange(n) * R)[:, None]
    assert (a >= 0).all() and (a < R).all(), "an ancestor outside its datum"
    assert (np.diff(a, axis=1) >= 0).all()
    own = S.resample(logw, R, 1.0, **K)                                   # (e and S of the inputs; the device's differ by ulps)
    for i in np.nonzero(dg[:, 1] != 0.0)[0]:
        counts, low, high = S.offspring_bounds(own.e[i], own.S[i], a[i])
        assert counts.sum() == R and (counts >= low).all() and (counts <= high).all(), (i, counts, low, high)


@pytest.mark.parametrize("R,n", SHAPES)
def test_a_datum_above_the_threshold_keeps_identity_ancestors_and_its_log_weights(R, n):
    logw = np.asarray(S.kernel_logw(R, n))
    for threshold in (0.0, 0.5):
        anc, lw, dg = ancestors(logw, R, threshold)
        stay = np.repeat(dg[:, 1] == 0.0, R)
        assert (dg[:, 1] == 0.0).all() if threshold == 0.0 else True, "threshold 0 resampled"
        np.testing.assert_array_equal(anc[stay], np.arange(n * R)[stay])
        assert np.array_equal(lw[stay].view(np.int64), logw[stay].view(np.int64))
        assert ((dg[:, 0] >= threshold * R) == (dg[:, 1] == 0.0)).all()
    if n == 5 and R > 1:
        assert 0 < (dg[:, 1] != 0.0).sum() < n, "one of the two branches is never taken"


# ---- special values -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_a_non_finite_log_weight_stays_in_its_datum_and_is_never_an_ancestor(value):
    R, n = 16, 5
    clean = np.asarray(S.kernel_logw(R, n))
    logw = clean.copy()
    bad = [2 * R + 5, 2 * R + R - 1, 4 * R]                               # in data 2 (its last replica too) and 4
    logw[bad] = value
    anc, lw, dg = ancestors(logw, R, 1.0)
    want = S.resample(logw, R, 1.0, **K)
    assert not np.isin(anc, bad).any()
    assert np.isfinite(lw).all() and (dg[:, 1] == 1.0).all()              # every slot of a resampled datum holds the mean weight
    keep = (want.slot_margin > S.SLOT_MARGIN).reshape(-1)
    assert keep.all() and (want.ess_margin > S.ESS_MARGIN).all(), "the planted case sits on a tie"
    np.testing.assert_array_equal(anc[keep], want.ancestors[keep])
    assert (np.abs(lw - want.logw) <= S.logw_tolerance(want.logw, R)).all()
    c_anc, c_lw, c_dg = ancestors(clean, R, 1.0)
    for i in (0, 1, 3):                                                  # the other data: bit for bit what they are without it
        rows = slice(i * R, (i + 1) * R)
        assert np.array_equal(anc[rows], c_anc[rows]) and np.array_equal(lw[rows].view(np.int64), c_lw[rows].view(np.int64))
        assert np.array_equal(dg[i].view(np.int64), c_dg[i].view(np.int64))


def test_a_datum_without_a_finite_log_weight_is_untouched():
    R, n = 16, 5
    logw = np.asarray(S.kernel_logw(R, n)).copy()
    logw[R:2 * R] = np.nan
    logw[3 * R:4 * R] = [np.nan, np.inf, -np.inf, np.nan] * 4
    anc, lw, dg = ancestors(logw, R, 1.0)
    for i in (1, 3):
        rows = slice(i * R, (i + 1) * R)
        np.testing.assert_array_equal(anc[rows], np.arange(n * R)[rows])
        assert np.array_equal(lw[rows].view(np.int64), logw[rows].view(np.int64))
        assert np.isnan(dg[i, 0]) and dg[i, 1] == 0.0 and np.isnan(dg[i, 3]) and dg[i, 2] == S.uniform(K["seed"], K["step"], K["chain_base"] + i * R)
    assert (dg[[0, 2, 4], 1] == 1.0).all()


# ---- independence -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", S.KERNEL_REPLICAS)
def test_a_datum_does_not_depend_on_the_other_data_or_on_the_run(R):
    logw = np.asarray(S.kernel_logw(R, 5))
    for threshold in S.KERNEL_THRESHOLDS:
        anc, lw, dg = ancestors(logw, R, threshold)
        again = ancestors(logw, R, threshold)
        assert np.array_equal(anc, again[0]) and np.array_equal(lw.view(np.int64), again[1].view(np.int64))
        assert np.array_equal(dg.view(np.int64), again[2].view(np.int64))
        for i in (0, 3):                                                 # datum i alone, under its own chain ids
            a1, l1, d1 = ancestors(logw[i * R:(i + 1) * R], R, threshold, chain_base=K["chain_base"] + i * R)
            rows = slice(i * R, (i + 1) * R)
            assert np.array_equal(a1 + i * R, anc[rows]) and np.array_equal(l1.view(np.int64), lw[rows].view(np.int64))
            assert np.array_equal(d1[0].view(np.int64), dg[i].view(np.int64))


# ---- gather -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("widths", [(w,) for w in S.GATHER_WIDTHS] + [(2, 257, 17), (33, 1, 2)])
def test_gather_is_bitwise_counts_bad_indices_and_writes_nothing_beyond_its_rows(widths):
    from montecarlopredictivecoding_amd.engine import smc_gather
    rows = 23                                                            # four rows per workgroup: five full ones and 3 / 4 of a sixth
    rng = np.random.default_rng([37, *widths])
    xs = [rng.standard_normal((rows, w)).astype(np.float32) for w in widths]
    xs[0][1, 0], xs[-1][5, -1] = np.nan, np.inf                          # bits, not values
    anc = rng.integers(0, rows, rows).astype(np.int32)
    bad = {3: -1, 8: rows, 20: 2 ** 31 - 1, 22: -2 ** 31}
    for r, v in bad.items():
        anc[r] = v
    src = [torch.tensor(x).to(DEV) for x in xs]
    pairs = [guarded(np.full((rows, w), SENTINEL, dtype=np.float32), torch.float32) for w in widths]
    nb_whole, nb = guarded(np.array([5], dtype=np.int32), torch.int32)
    out = smc_gather(src, torch.tensor(anc).to(DEV), out=[p[1] for p in pairs], n_bad=nb)
    torch.cuda.synchronize()
    take = anc.astype(np.int64)
    for r in bad:
        take[r] = r
    for x, o in zip(xs, out):
        assert np.array_equal(o.cpu().numpy().view(np.int32), x[take].view(np.int32))
    assert int(nb[0]) == 5 + len(bad)
    assert guards_intact(nb_whole, *[p[0] for p in pairs])
    for s, x in zip(src, xs):                                            # out of place: the source keeps its bits
        assert np.array_equal(s.cpu().numpy().view(np.int32), x.view(np.int32))
    fresh = smc_gather(src, torch.tensor(np.arange(rows, dtype=np.int32)).to(DEV))         # no out, no counter: the identity
    for s, o in zip(src, fresh):
        assert np.array_equal(bits32(o), bits32(s))


def bits32(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def _stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _arr(ts):
    if ts is None:
        return None
    a = (C.c_void_p * len(ts))()
    for i, t in enumerate(ts):
        a[i] = None if t is None else t.data_ptr()
    return a


def test_refused_calls_launch_nothing_and_no_row_launches_nothing():
    from montecarlopredictivecoding_amd import _lib as L
    lib = L.load()
    R, n = 16, 3
    logw = torch.full((n * R,), -3.0, dtype=torch.float64, device=DEV)
    anc = torch.full((n * R,), SENTINEL, dtype=torch.int32, device=DEV)

    def raw_ancestors(logw=logw, n_data=n, replicas=R, threshold=0.5, anc=anc):
        return lib.mcpc_smc_ancestors(0, _p(logw), n_data, replicas, threshold, 1, 2, 3, _p(anc), None, _stream())

    for change in (dict(replicas=0), dict(replicas=-1), dict(replicas=L.SMC_MAX_REPLICAS + 1), dict(n_data=-1),
                   dict(n_data=(2 ** 31 - 1) // R + 1), dict(threshold=-0.01), dict(threshold=1.01), dict(threshold=float("nan")),
                   dict(logw=None), dict(anc=None)):
        assert raw_ancestors(**change) == -1, change
        assert lib.mcpc_last_error().decode().startswith("smc_ancestors:"), change
    assert raw_ancestors(n_data=0) == 0 and raw_ancestors(n_data=0, logw=None, anc=None) == 0

    rows, widths = 9, [3, 6]
    x = [torch.full((rows, w), 0.5, device=DEV) for w in widths]
    out = [torch.full((rows, w), float(SENTINEL), device=DEV) for w in widths]
    idx = torch.zeros(rows, dtype=torch.int32, device=DEV)

    def raw_gather(x=x, widths=widths, n_layers=2, rows=rows, idx=idx, out=out):
        w = None if widths is None else (C.c_int32 * len(widths))(*widths)
        return lib.mcpc_smc_gather(0, _arr(x), w, n_layers, rows, _p(idx), _arr(out), None, _stream())

    for change in (dict(n_layers=0), dict(n_layers=L.MAX_LATENT + 1), dict(rows=-1), dict(rows=2 ** 31), dict(widths=None),
                   dict(widths=[3, 0]), dict(x=None), dict(x=[x[0], None]), dict(out=None), dict(out=[None, out[1]]), dict(idx=None)):
        assert raw_gather(**change) == -1, change
        assert lib.mcpc_last_error().decode().startswith("smc_gather:"), change
    assert raw_gather(rows=0) == 0 and raw_gather(rows=0, x=None, out=None, idx=None) == 0
    torch.cuda.synchronize()
    assert (anc == SENTINEL).all() and (logw == -3.0).all() and all(bool((o == SENTINEL).all()) for o in out)


def test_the_python_front_refuses_what_the_library_would():
    from montecarlopredictivecoding_amd.engine import smc_ancestors, smc_gather
    logw = torch.zeros(32, dtype=torch.float64, device=DEV)
    for kw in (dict(replicas=0), dict(replicas=5), dict(replicas=4097), dict(threshold=1.5), dict(threshold=-0.1)):
        with pytest.raises(ValueError):
            smc_ancestors(logw, **dict(dict(replicas=16, threshold=0.5, seed=0, step=0), **kw))
    with pytest.raises(TypeError):
        smc_ancestors(logw.float(), 16, 0.5, 0, 0)
    with pytest.raises(TypeError):
        smc_gather([torch.zeros(4, 3, device=DEV)], torch.zeros(4, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        smc_gather([torch.zeros(4, 3, device=DEV)], torch.zeros(5, dtype=torch.int32, device=DEV))

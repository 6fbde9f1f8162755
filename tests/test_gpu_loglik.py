"""The per-datum importance-sampling state of the log marginal likelihood on the device (include/mcpc.h: mcpc_loglik_accumulate;
csrc/mcpc_loglik.h) against the fp64 numpy reference of tests/loglik_cases.py, within the tolerance derived there, for both read-outs.

Shapes: n_data and n_samp of one row, one short of a 16-row tile, a whole tile, one over, several tiles; widths of one column, short
of a k-step of 4, a whole one, one over, whole 16-column chunks and a ragged one -- widths that are multiples of 4 take the 16-byte
loads, the others the element-wise ones; plans of one group and of many, with one, two (a whole pair) and three (a pair and a half)
sample tiles per group."""
import math

import numpy as np
import pytest
import torch

from tests import loglik_cases as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
#        n_data, n_samp, width
CASES = [(1, 1, 1), (15, 15, 3), (16, 16, 4), (17, 17, 5), (48, 600, 64), (17, 600, 67), (15, 17, 67), (16, 1, 64), (1, 600, 5),
         (8000, 600, 5), (4800, 600, 4)]
NAN_BITS = np.float64(np.nan).view(np.int64)


def _run(y, o, loss, var, clamp=20.0, state=None, accumulate=False):
    """state [n_data, 4] as numpy; ``state`` (a device tensor) is updated in place when given, else one pre-filled with NaN is made."""
    from montecarlopredictivecoding_amd.engine import loglik_accumulate
    yd = y if isinstance(y, torch.Tensor) else torch.tensor(y, device=DEV)
    od = o if isinstance(o, torch.Tensor) else torch.tensor(o, device=DEV)
    if state is None:
        state = torch.full((yd.shape[0], 4), math.nan, dtype=torch.float64, device=DEV)
    loglik_accumulate(yd, od, loss, var, clamp, state, accumulate=accumulate)
    return state.cpu().numpy()


_REF = {}


def _reference(n_data, n_samp, width, loss):
    """(y, o, var, fp64 state, tolerance) of a shape; computed once, shared, never modified."""
    key = (n_data, n_samp, width, loss)
    if key not in _REF:
        y, o, var = R.make_case(n_data, n_samp, width, loss)
        want, t = R.ref_state(y, o, loss, var), R.tol(y, o, loss, var)
        for a in (y, o, want, t):
            a.setflags(write=False)
        _REF[key] = (y, o, var, want, t)
    return _REF[key]


@pytest.mark.parametrize("loss", R.LOSSES)
@pytest.mark.parametrize("n_data, n_samp, width", CASES)
def test_against_the_fp64_reference(n_data, n_samp, width, loss):
    from montecarlopredictivecoding_amd import likelihood as K
    from montecarlopredictivecoding_amd.engine import loglik_workspace_bytes
    y, o, var, want, t = _reference(n_data, n_samp, width, loss)
    p = K.plan(n_data, n_samp, width)
    assert loglik_workspace_bytes(n_data, n_samp, width) == p["workspace_bytes"]
    if (n_data, n_samp) == (17, 600):
        assert p["groups"] >= 3 and p["tiles_per_group"] == 1                          # many sample groups to merge
    if (n_data, n_samp) == (8000, 600):
        assert p["groups"] >= 3 and p["tiles_per_group"] == 3                          # a pair of sample tiles and a half
    if (n_data, n_samp) == (4800, 600):
        assert p["groups"] >= 3 and p["tiles_per_group"] == 2
    got = _run(y, o, loss, var)
    assert (want[:, 3] == n_samp).all()
    R.assert_state_close(got, want, t, f"{n_data} x {n_samp} x {width} {loss}")


@pytest.mark.parametrize("loss", R.LOSSES)
def test_two_runs_are_bitwise_equal(loss):
    y, o, var, want, t = _reference(48, 600, 64, loss)
    a, b = _run(y, o, loss, var), _run(y, o, loss, var)
    assert a.tobytes() == b.tobytes()
    y, o, var, want, t = _reference(8000, 600, 5, loss)
    assert _run(y, o, loss, var).tobytes() == _run(y, o, loss, var).tobytes()


@pytest.mark.parametrize("loss", R.LOSSES)
def test_chunked_and_permuted_samples_agree_within_the_tolerance(loss):
    y, o, var, want, t = _reference(17, 600, 67, loss)
    once = _run(y, o, loss, var)
    yd, od = torch.tensor(y, device=DEV), torch.tensor(o, device=DEV)
    for chunk in (1, 17, 217):
        state = torch.full((17, 4), math.nan, dtype=torch.float64, device=DEV)
        for s0 in range(0, 600, chunk):
            _run(yd, od[s0:s0 + chunk], loss, var, state=state, accumulate=s0 > 0)
        got = state.cpu().numpy()
        R.assert_state_close(got, want, t, f"chunks of {chunk} ({loss}) against fp64")
        R.assert_state_close(got, once, t, f"chunks of {chunk} ({loss}) against the one-shot call")
    perm = np.random.default_rng(5).permutation(600)
    got = _run(y, o[perm], loss, var)
    R.assert_state_close(got, want, t, f"permuted samples ({loss}) against fp64")
    R.assert_state_close(got, once, t, f"permuted samples ({loss}) against the given order")


@pytest.mark.parametrize("loss", R.LOSSES)
def test_the_clamp(loss):
    y, o, var, _, _ = _reference(17, 17, 5, loss)
    y, o = y.copy(), o.copy()
    o[:, 0], o[:, 1] = 50.0, -50.0                          # every sample holds read-outs beyond the clamp, on both sides ...
    y[0, 0], y[1, 1] = 0.0, 1.0                             # ... and for these data every sample pays for them
    clamped, free = R.ref_state(y, o, loss, var, 20.0), R.ref_state(y, o, loss, var, math.inf)
    assert np.abs(R.log_p(clamped) - R.log_p(free)).max() > 1.0                        # the clamp matters on these inputs
    R.assert_state_close(_run(y, o, loss, var, clamp=20.0), clamped, R.tol(y, o, loss, var, 20.0), f"clamp 20 ({loss})")
    R.assert_state_close(_run(y, o, loss, var, clamp=math.inf), free, R.tol(y, o, loss, var, math.inf), f"no clamp ({loss})")


@pytest.mark.parametrize("loss", R.LOSSES)
def test_one_sample_that_beats_all_others_by_more_than_exp_can_hold(loss):
    n_data, S, width, best = 17, 600, 64, 300
    y = np.ones((n_data, width), dtype=np.float32)
    if loss == "bernoulli":
        o, var = np.full((S, width), -20.0, dtype=np.float32), None
        o[best] = 20.0
    else:
        o, var = np.full((S, width), 6.0, dtype=np.float32), 0.3
        o[best] = 1.0
    nll = R.nll_matrix(y, o, loss, var)
    assert (np.delete(nll, best, axis=1).min(1) - nll[:, best] > 800).all()
    got = _run(y, o, loss, var)
    want = R.ref_state(y, o, loss, var)
    assert (got[:, 1] == 1.0).all() and (got[:, 2] == 1.0).all() and (got[:, 3] == S).all()
    assert (R.ess(got) == 1.0).all()
    np.testing.assert_allclose(R.log_p(got), -got[:, 0] - math.log(S), rtol=2.0 ** -50, atol=0)
    R.assert_state_close(got, want, R.tol(y, o, loss, var), f"underflow ({loss})")


@pytest.mark.parametrize("loss", R.LOSSES)
def test_stale_state_is_overwritten_and_nothing_is_the_empty_state(loss):
    y, o, var, want, t = _reference(17, 17, 5, loss)
    clean = _run(y, o, loss, var, state=torch.zeros(17, 4, dtype=torch.float64, device=DEV))
    stale = _run(y, o, loss, var, state=torch.full((17, 4), math.nan, dtype=torch.float64, device=DEV))
    assert clean.tobytes() == stale.tobytes()
    # no samples: the empty state with accumulate = 0, nothing with accumulate = 1
    none = _run(y, o[:0], loss, var)
    assert none.tolist() == [[math.inf, 0.0, 0.0, 0.0]] * 17
    state = torch.tensor(clean, device=DEV)
    assert _run(y, o[:0], loss, var, state=state, accumulate=True).tobytes() == clean.tobytes()
    # accumulating into empty states is the plain call
    state = torch.tensor(none, device=DEV)
    R.assert_state_close(_run(y, o, loss, var, state=state, accumulate=True), want, t, f"into empty states ({loss})")
    assert _run(y[:0], o, loss, var).shape == (0, 4)


@pytest.mark.parametrize("width", [5, 64])
@pytest.mark.parametrize("loss", R.LOSSES)
def test_interior_slices_of_nan_buffers(loss, width):
    """y, o and state are interior slices of larger buffers whose other rows are NaN: a read past a ragged edge would poison a result,
    a write past it would change the surrounding state rows."""
    n_data, n_samp = 17, 17
    y, o, var = R.make_case(n_data, n_samp, width, loss, seed=2)
    alone = _run(y, o, loss, var)
    big_y = torch.full((n_data + 7, width), math.nan, dtype=torch.float32, device=DEV)
    big_o = torch.full((n_samp + 7, width), math.nan, dtype=torch.float32, device=DEV)
    big_s = torch.full((n_data + 7, 4), math.nan, dtype=torch.float64, device=DEV)
    big_y[3:3 + n_data] = torch.tensor(y, device=DEV)
    big_o[4:4 + n_samp] = torch.tensor(o, device=DEV)
    got = _run(big_y[3:3 + n_data], big_o[4:4 + n_samp], loss, var, state=big_s[2:2 + n_data])
    assert got.tobytes() == alone.tobytes()
    R.assert_state_close(got, R.ref_state(y, o, loss, var), R.tol(y, o, loss, var), f"interior slices ({loss}, width {width})")
    around = big_s.cpu().numpy().view(np.int64)
    assert (around[:2] == NAN_BITS).all() and (around[2 + n_data:] == NAN_BITS).all()


@pytest.mark.parametrize("loss", R.LOSSES)
def test_special_values_stay_in_their_row(loss):
    y, o, var, want, t = _reference(48, 600, 64, loss)
    clean = _run(y, o, loss, var)
    # a NaN in one sample row: that sample is not taken, by any datum
    o2 = o.copy()
    o2[77, 13] = np.nan
    got = _run(y, o2, loss, var)
    assert (got[:, 3] == 599).all()
    R.assert_state_close(got, R.ref_state(y, o2, loss, var), R.tol(y, o2, loss, var), f"a NaN sample ({loss})")
    less = np.delete(o, 77, axis=0)
    R.assert_state_close(got, R.ref_state(y, less, loss, var), R.tol(y, less, loss, var), f"a NaN sample is a sample less ({loss})")
    # a NaN in one datum row: that datum takes nothing, every other datum is untouched
    y2 = y.copy()
    y2[21, 40] = np.nan
    got = _run(y2, o, loss, var)
    assert got[21].tolist() == [math.inf, 0.0, 0.0, 0.0]
    assert np.delete(got, 21, axis=0).tobytes() == np.delete(clean, 21, axis=0).tobytes()
    # an infinite logit without a clamp: the sample's own pairs only
    o3 = o.copy()
    o3[5, 0] = np.inf
    got = _run(y, o3, loss, var, clamp=math.inf)
    R.assert_state_close(got, R.ref_state(y, o3, loss, var, math.inf), R.tol(y, o3, loss, var, math.inf), f"an infinite read-out ({loss})")


def test_log_likelihood_streams_and_continues():
    from montecarlopredictivecoding_amd import likelihood as K
    y, o, var, want, t = _reference(48, 600, 64, "bernoulli")
    whole = K.log_likelihood(y, o)
    assert whole.state.device.type == "cuda" and whole.state.dtype == torch.float64 and tuple(whole.state.shape) == (48, 4)
    R.assert_state_close(whole.state.cpu().numpy(), want, t, "log_likelihood")
    chunked = K.log_likelihood(torch.tensor(y), o, chunk_bytes=100 * 64 * 4)                   # six chunks of 100 samples
    R.assert_state_close(chunked.state.cpu().numpy(), want, t, "log_likelihood in six chunks")
    first = K.log_likelihood(y, o[:250])
    kept = first.state.clone()
    both = K.log_likelihood(y, o[250:], state=first)
    assert torch.equal(first.state, kept)                                                      # the earlier state is not modified
    R.assert_state_close(both.state.cpu().numpy(), want, t, "log_likelihood continued")
    R.assert_state_close(first.merge(K.log_likelihood(y, o[250:])).state.cpu().numpy(), want, t, "LogLikelihood.merge on the device")
    assert abs(whole.mean() - float(R.log_p(want).mean())) <= float(t.max())
    assert bool((whole.ess >= 1).all()) and bool((whole.ess <= 600).all())
    with pytest.raises(ValueError, match="64 columns, outputs has 5"):
        K.log_likelihood(y, o[:, :5])


def test_the_evaluator_on_the_references_fixture():
    from montecarlopredictivecoding_amd.utils.training_evaluation import get_marginal_likelihood, get_marginal_likelihood_per_datum
    from tests.test_evaluators_golden import load_eval_fixture
    z, meta, cfg, model, loader = load_eval_fixture("bernoulli", device=DEV)
    n = int(z["data"].shape[0])
    torch.manual_seed(meta["torch_seed"])
    ll = get_marginal_likelihood_per_datum(model, cfg, loader, True, n_samples=600)
    torch.manual_seed(meta["torch_seed"])
    scalar = get_marginal_likelihood(model, cfg, loader, True, n_samples=600)
    print("per datum, mean %.12g; fp32 evaluator %.12g; the reference's %.12g; ESS %.1f .. %.1f" % (
        ll.mean(), scalar, float(z["ml"]), float(ll.ess.min()), float(ll.ess.max())))
    assert len(ll) == n and bool((ll.n_samples == 600).all())
    assert ll.mean() == pytest.approx(float(z["ml"]), rel=2e-6)
    assert ll.mean() == pytest.approx(scalar, rel=2e-6)
    assert bool((ll.ess >= 1).all()) and bool((ll.ess <= 600).all())
    torch.manual_seed(meta["torch_seed"])
    chunked = get_marginal_likelihood_per_datum(model, cfg, loader, True, n_samples=600, sample_chunk=100)
    assert bool((chunked.n_samples == 600).all()) and bool(torch.isfinite(chunked.log_p).all())


def test_the_evaluator_on_the_gaussian_fixture():
    from montecarlopredictivecoding_amd.utils.training_evaluation import get_marginal_likelihood_per_datum, sample_pc
    from tests.test_evaluators_golden import load_eval_fixture
    z, meta, cfg, model, loader = load_eval_fixture("gaussian", device=DEV)
    torch.manual_seed(meta["torch_seed"])
    ll = get_marginal_likelihood_per_datum(model, cfg, loader, True, n_samples=600)
    torch.manual_seed(meta["torch_seed"])
    means = sample_pc(600, model, cfg, use_cuda=True, is_return_hidden=True).cpu().numpy()
    y, var = z["data"].astype(np.float32), float(meta["input_var"])
    R.assert_state_close(ll.state.cpu().numpy(), R.ref_state(y, means, "gaussian", var, 20.0), R.tol(y, means, "gaussian", var, 20.0),
                         "the Gaussian fixture")

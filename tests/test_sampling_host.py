"""The one definition of "which steps are samples" (sampling.py): `SampleWindow.chunk` against a brute-force list, the nine request
classes against the base, the shared parsers' messages, and `slice_bounds` against worked examples of the trainer's slicing loop."""
import itertools
import re

import pytest
import torch

from montecarlopredictivecoding_amd import (autocovariance, chain_energies, cloud, covariance, errors, histogram, moments, probe,
                                            rolling, sampling)
from montecarlopredictivecoding_amd.sampling import SampleWindow, sample_steps, slice_bounds

SIZES, N_OUT, B, BIG = (5, 12, 9), 14, 4, 1 << 40


def _specs(begin, stride, T):
    """The nine validated requests of one window, by request name."""
    w = dict(begin=begin, stride=stride)
    nl = len(SIZES)
    return {
        "mcpc_moments": moments.validate_spec(dict(w, layers=(0,)), T, nl, N_OUT),
        "mcpc_chain_energies": chain_energies.validate_spec(dict(w), T),
        "mcpc_covariance": covariance.validate_spec(dict(w), T, nl, N_OUT, SIZES, B, BIG),
        "mcpc_histogram": histogram.validate_spec(dict(w, layers=(1,), bins=4, range=(-1.0, 1.0)), T, nl, N_OUT, SIZES, B, BIG),
        "mcpc_autocovariance": autocovariance.validate_spec(dict(w, layers=(1,), max_lag=2), T, nl, N_OUT, SIZES, B, BIG),
        "mcpc_probe": probe.validate_spec(dict(w, layer=1, weight=torch.zeros(3, 12)), T, nl, SIZES, B),
        "mcpc_cloud": cloud.validate_spec(dict(w, layer=0), T, nl, SIZES, B, BIG),
        "mcpc_rolling": rolling.validate_spec(dict(w, layers=(2,), window=2), T, nl, N_OUT, SIZES, B, BIG),
        "mcpc_errors": errors.validate_spec(dict(w, layers=(1,)), T, nl, N_OUT, SIZES, B, True, BIG),
    }


def test_chunk_is_the_brute_force_list_of_sample_steps():
    cases = 0
    for T in range(1, 13):
        for begin, stride in itertools.product(range(T), range(1, 6)):
            w = SampleWindow(begin=begin, stride=stride, T=T)
            steps = [t for t in range(T) if t >= begin and (t - begin) % stride == 0]
            assert w.steps == steps == list(sample_steps(begin, T, stride)) and w.n == len(steps)
            for t0 in range(T):
                for n_steps in range(1, T - t0 + 3):                 # also chunks that run past the call's end
                    inside = [t for t in steps if t0 <= t < t0 + n_steps]
                    first, count = w.chunk(t0, n_steps)
                    assert count == len(inside), (T, begin, stride, t0, n_steps)
                    assert [t0 + first + k * stride for k in range(count)] == inside, (T, begin, stride, t0, n_steps)
                    cases += 1
    assert cases > 3000


@pytest.mark.parametrize("begin,stride,T", [(0, 1, 60), (7, 5, 60), (59, 3, 60), (13, 3, 61), (20, 64, 60)])
def test_every_request_class_is_the_base_window(begin, stride, T):
    base = SampleWindow(begin=begin, stride=stride, T=T)
    specs = _specs(begin, stride, T)
    assert len(specs) == 9
    for name, spec in specs.items():
        assert isinstance(spec, SampleWindow) and (spec.begin, spec.stride, spec.T) == (begin, stride, T), name
        assert spec.n == base.n, name
        for t0, n_steps in ((0, T), (0, 1), (5, 7), (begin, 1), (T - 1, 1), (33, 27), (7, 7)):
            assert spec.chunk(t0, n_steps) == base.chunk(t0, n_steps), (name, t0, n_steps)
    assert specs["mcpc_chain_energies"].steps == base.steps
    assert specs["mcpc_rolling"].steps == base.steps[1:]             # its own: the newest sample of every full window of 2


def test_a_shared_parser_error_carries_the_requests_own_name():
    nl = len(SIZES)
    calls = {
        "mcpc_moments": lambda s: moments.validate_spec(s, 60, nl, N_OUT),
        "mcpc_chain_energies": lambda s: chain_energies.validate_spec(s, 60),
        "mcpc_covariance": lambda s: covariance.validate_spec(s, 60, nl, N_OUT, SIZES, B, BIG),
        "mcpc_histogram": lambda s: histogram.validate_spec(s, 60, nl, N_OUT, SIZES, B, BIG),
        "mcpc_autocovariance": lambda s: autocovariance.validate_spec(s, 60, nl, N_OUT, SIZES, B, BIG),
        "mcpc_probe": lambda s: probe.validate_spec(s, 60, nl, SIZES, B),
        "mcpc_cloud": lambda s: cloud.validate_spec(s, 60, nl, SIZES, B, BIG),
        "mcpc_rolling": lambda s: rolling.validate_spec(s, 60, nl, N_OUT, SIZES, B, BIG),
        "mcpc_errors": lambda s: errors.validate_spec(s, 60, nl, N_OUT, SIZES, B, True, BIG),
    }
    assert len(calls) == 9
    for name, validate in calls.items():
        with pytest.raises(ValueError, match=re.escape(f"{name}: expected a dict or None, got list")):
            validate([])
        with pytest.raises(ValueError, match=re.escape(f"{name}: unknown keys ['when']; known: ['begin', 'stride'")):
            validate(dict(when=3))
        with pytest.raises(ValueError, match=re.escape(f"{name}: begin=60 outside [0, T=60)")):
            validate(dict(begin=60))
        with pytest.raises(ValueError, match=re.escape(f"{name}: stride must be an int, got 2.0")):
            validate(dict(stride=2.0))
        with pytest.raises(ValueError, match=re.escape(f"{name}: stride=0, must be at least 1")):
            validate(dict(stride=0))
    for name in ("mcpc_moments", "mcpc_covariance", "mcpc_histogram", "mcpc_autocovariance", "mcpc_rolling", "mcpc_errors"):
        with pytest.raises(ValueError, match=re.escape(f"{name}: layer index 3 out of range, the model has 3 PC layers (0..2)")):
            calls[name](dict(layers=(0, 3)))
        with pytest.raises(ValueError, match=re.escape(f"{name}: outputs='softmax', expected None, ")):
            calls[name](dict(layers=(0,), outputs="softmax"))
    for name in ("mcpc_probe", "mcpc_cloud"):
        with pytest.raises(ValueError, match=re.escape(f"{name}: layer index 3 out of range, the model has 3 PC layers (0..2)")):
            calls[name](dict(layer=3))
        with pytest.raises(ValueError, match=re.escape(f"{name}: layer is required: the PC layer ")):
            calls[name](dict())


def test_what_layers_none_means_stays_each_requests_own():
    """The differences the nine copies had, kept as arguments of the shared parser: `layers=None` is every layer for the covariance,
    no layer for the histogram, the autocovariance and the rolling variability, and no sequence for the moments and the errors."""
    nl = len(SIZES)
    assert covariance.validate_spec(dict(), 60, nl, N_OUT, SIZES, B, BIG).layers == (0, 1, 2)
    assert covariance.validate_spec(dict(layers=None), 60, nl, N_OUT, SIZES, B, BIG).layers == (0, 1, 2)
    assert moments.validate_spec(dict(), 60, nl, N_OUT).layers == ()
    assert histogram.validate_spec(dict(layers=None, outputs="identity", bins=[0.0, 1.0]), 60, nl, N_OUT, SIZES, B, BIG).layers == ()
    assert autocovariance.validate_spec(dict(layers=None, outputs="identity", max_lag=1), 60, nl, N_OUT, SIZES, B, BIG).layers == ()
    assert rolling.validate_spec(dict(layers=None, outputs="identity", window=3), 60, nl, N_OUT, SIZES, B, BIG).layers == ()
    with pytest.raises(ValueError, match="mcpc_moments: layers must be a sequence of layer indices, got None"):
        moments.validate_spec(dict(layers=None), 60, nl, N_OUT)
    with pytest.raises(ValueError, match="mcpc_errors: layers must be a sequence of layer indices, got None"):
        errors.validate_spec(dict(layers=None), 60, nl, N_OUT, SIZES, B, True, BIG)
    assert sampling.parse_layers("r", dict(layers=2), 3) == (2,) and sampling.parse_layers("r", dict(layers=[2, 0, 2]), 3) == (0, 2)


def _keeps():
    for T in range(1, 13):
        for S in range(1, T + 2):
            yield T, S, None
            for a in range(T):
                for b in range(a + 1, T + 1):
                    yield T, S, (a, b)


def test_slice_bounds_tile_the_call_and_spare_the_kept_window():
    for T, S, keep in _keeps():
        bounds = slice_bounds(T, S, keep)
        assert bounds[0][0] == 0 and sum(n for _, n in bounds) == T, (T, S, keep)
        assert all(n >= 1 for _, n in bounds)
        assert all(a + n == b for (a, n), (b, _) in zip(bounds, bounds[1:])), (T, S, keep)          # in order, no gap
        if keep is None:
            assert all(n <= S for _, n in bounds)
            continue
        assert not any(keep[0] < t0 < keep[1] for t0, _ in bounds), (T, S, keep)                   # no boundary inside it
        holds = [(t0, n) for t0, n in bounds if t0 <= keep[0] and keep[1] <= t0 + n]
        assert len(holds) == 1, (T, S, keep)
        assert all(n <= S for t0, n in bounds if (t0, n) != holds[0]), (T, S, keep)


def test_slice_bounds_worked_examples():
    """Each traced by hand through the loop `_run_fused_sliced` held before: n = min(S, T - t0); if keep[0] < t0 + n < keep[1] the slice
    would end inside the window and becomes keep[0] - t0 (it starts before the window) or keep[1] - t0 (it starts in it)."""
    # no window: full slices and a remainder
    assert slice_bounds(10, 4, None) == [(0, 4), (4, 4), (8, 2)]
    # the window starts mid-slice: (6, 6) would end at 12, inside 8..14, and is cut at 8; (8, 6) ends at 14, which is not inside
    assert slice_bounds(20, 6, (8, 14)) == [(0, 6), (6, 2), (8, 6), (14, 6)]
    # the window is longer than S: (4, 4) would end at 8 and is cut at 5; (5, 4) would end at 9 and runs to 17 in one slice of 12
    assert slice_bounds(20, 4, (5, 17)) == [(0, 4), (4, 1), (5, 12), (17, 3)]
    # the facade tests' learning call: T = 60, gradients accumulated over 40..59, 7 steps per slice
    assert slice_bounds(60, 7, (40, 60)) == [(0, 7), (7, 7), (14, 7), (21, 7), (28, 7), (35, 5), (40, 20)]
    # S above T, and a window that is the whole call
    assert slice_bounds(5, 9, None) == [(0, 5)] and slice_bounds(6, 2, (0, 6)) == [(0, 6)]


def test_names_stay_importable_from_where_they_were():
    assert covariance.sample_steps is moments.sample_steps is chain_energies.sample_steps is errors.sample_steps is sample_steps
    assert covariance.human_bytes is sampling.human_bytes and covariance.human_bytes(3 << 20) == "3.0 MiB"

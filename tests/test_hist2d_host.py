"""Joint histograms and the probe as a derived record, host side (no GPU): the header and the binding, the MCPC_EINVAL cases of
`mcpc_hist2d_accumulate` and `mcpc_probe_records` (fake pointers, never dereferenced), the validation of `PCTrainer.mcpc_histogram2d`,
the numpy reference the GPU tests compare against, and the arithmetic of `Histogram2D` on hand-made counts."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from montecarlopredictivecoding_amd import _lib
from tests import hist2d_cases as hc
from tests.hist_cases import table as hist_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
REC, REC2, P1, P2 = (C.c_void_p(0x1000 * i) for i in range(1, 5))           # never dereferenced: every call below is refused
FP = C.POINTER(C.c_float)


def _H():
    import montecarlopredictivecoding_amd.histogram2d as H
    return H


# ---- the C interface ---------------------------------------------------------------------------------------------------------------
def _declared_args(header, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_header_declares_the_entry_points_and_the_binding_binds_them():
    header = open(os.path.join(ROOT, "include", "mcpc.h")).read()
    for macro, val in (("MCPC_HIST2D_MAX_BINS", 128), ("MCPC_HIST2D_MAX_CELLS", 12288), ("MCPC_HIST2D_MAX_PAIRS", 128)):
        assert re.search(r"#define\s+" + macro + r"\s+" + str(val) + r"\b", header), macro
    assert (_lib.HIST2D_MAX_BINS, _lib.HIST2D_MAX_CELLS, _lib.HIST2D_MAX_PAIRS) == (128, 12288, 128)
    # the signatures the header declares: 21 arguments, and 13 (device, rec, B, width, first, stride, n, W, bias, n_classes, link, out,
    # stream)
    for name, n_args in (("mcpc_hist2d_accumulate", 21), ("mcpc_probe_records", 13)):
        assert _declared_args(header, name) == n_args == len(_lib.SYMBOLS[name][1]), name
        assert _lib.SYMBOLS[name][0] is C.c_int
        assert hasattr(_lib.load(), name)
    assert re.search(r"#define\s+MCPC_ABI_VERSION\s+4\b", header) and _lib.ABI_VERSION == 4
    from montecarlopredictivecoding_amd import engine
    assert callable(engine.hist2d_accumulate) and callable(engine.probe_records)


EX = np.linspace(-1, 1, 5).astype(np.float32)
EY = np.linspace(-2, 2, 4).astype(np.float32)


def _hist2d(lib, rec_x=REC, wx=5, rec_y=REC2, wy=7, B=3, first=0, stride=1, n=4, tx=0, ty=0, pairs=((0, 0), (4, 6)), n_pairs=None,
            ex=EX, nx=None, ey=EY, ny=None, pool=0, counts=P1, accumulate=1):
    flat = None if pairs is None else (C.c_int32 * (2 * len(pairs)))(*[v for p in pairs for v in p])
    n_pairs = (0 if pairs is None else len(pairs)) if n_pairs is None else n_pairs
    px = None if ex is None else np.ascontiguousarray(ex, dtype=np.float32).ctypes.data_as(FP)
    py = None if ey is None else np.ascontiguousarray(ey, dtype=np.float32).ctypes.data_as(FP)
    nx = (len(ex) - 1 if ex is not None else 1) if nx is None else nx
    ny = (len(ey) - 1 if ey is not None else 1) if ny is None else ny
    return lib.mcpc_hist2d_accumulate(0, rec_x, wx, rec_y, wy, B, first, stride, n, tx, ty, flat, n_pairs, px, nx, py, ny, pool, counts,
                                      accumulate, None)


def _records(lib, rec=REC, B=3, width=5, first=0, stride=1, n=4, W=P1, n_classes=3, link=0, out=P2):
    return lib.mcpc_probe_records(0, rec, B, width, first, stride, n, W, None, n_classes, link, out, None)


WINDOW = [(dict(first=-1), "first=-1, must not be negative"), (dict(stride=0), "stride=0, must be at least 1"),
          (dict(n=-1), "n=-1, must not be negative")]
BIG = np.linspace(0, 1, 130).astype(np.float32)                             # 129 bins
HIST2D_CASES = [(kw, "hist2d: " + text, True) for kw, text in WINDOW] + [
    (dict(rec_x=None), "hist2d: rec is null with n=4", True),
    (dict(rec_y=None), "hist2d: rec_y is null with n=4", True),
    (dict(tx=2), "hist2d: unknown transform 2", True), (dict(ty=-1), "hist2d: unknown transform -1", True),
    (dict(B=0), "hist2d: B=0", False), (dict(wx=0), "hist2d: width_x=0", False), (dict(wy=-2), "hist2d: width_y=-2", False),
    (dict(pairs=None, n_pairs=1), "hist2d: pairs is null", False),
    (dict(n_pairs=0), "hist2d: n_pairs=0", False),
    (dict(pairs=((0, 0),) * 129), "hist2d: n_pairs=129", False),
    (dict(pairs=((0, 0), (5, 0))), "hist2d: pair 1: x column 5", False),
    (dict(pairs=((0, 0), (1, 1), (0, 7))), "hist2d: pair 2: y column 7", False),
    (dict(pairs=((-1, 0),)), "hist2d: pair 0: x column -1", False),
    (dict(nx=0), "hist2d: nx=0", False), (dict(ex=BIG), "hist2d: nx=129", False), (dict(ey=BIG), "hist2d: ny=129", False),
    (dict(ex=BIG[:129], ey=BIG[:100]), "hist2d: (nx + 3) * (ny + 3) = 13362 cells", False),
    (dict(ex=None), "hist2d: edges_x is null", False), (dict(ey=None), "hist2d: edges_y is null", False),
    (dict(ex=np.array([0, np.inf, 2], dtype=np.float32)), "hist2d: edges_x[1] is not finite", False),
    (dict(ey=np.array([0, 1, np.nan], dtype=np.float32)), "hist2d: edges_y[2] is not finite", False),
    (dict(ex=np.array([0, 1, 1], dtype=np.float32)), "hist2d: edges_x are not strictly ascending at 2", False),
    (dict(ey=np.array([0, -1], dtype=np.float32)), "hist2d: edges_y are not strictly ascending at 1", False),
    (dict(pool=2), "hist2d: pool=2", False),
    (dict(counts=None), "hist2d: counts is null", False),
]
RECORDS_CASES = [(kw, "probe records: " + text, True) for kw, text in WINDOW] + [
    (dict(rec=None), "probe records: rec is null with n=4", True),
    (dict(W=None), "probe records: W is null", False), (dict(out=None), "probe records: out is null", False),
    (dict(B=0), "probe records: B=0, must be at least 1", True), (dict(width=0), "probe records: width=0, must be at least 1", True),
    (dict(n_classes=0), "probe records: n_classes=0 outside 1..64", True),
    (dict(n_classes=65), "probe records: n_classes=65 outside 1..64", True),
    (dict(link=3), "probe records: unknown link 3", True), (dict(link=-1), "probe records: unknown link -1", True),
]


@pytest.mark.parametrize("fn, kw, message, whole",
                         [(_hist2d,) + c for c in HIST2D_CASES] + [(_records,) + c for c in RECORDS_CASES],
                         ids=[f"hist2d-{i}" for i in range(len(HIST2D_CASES))] + [f"records-{i}" for i in range(len(RECORDS_CASES))])
def test_argument_errors_are_refused_before_any_device_work(fn, kw, message, whole):
    """Every MCPC_EINVAL case returns -1 with a message that opens with the entry's name and holds the offending value; the window's
    four have the wording of `check_window`, whole.  No device is touched: the pointers are never dereferenced."""
    lib = _lib.load()
    rc = fn(lib, **kw)
    got = lib.mcpc_last_error().decode()
    assert rc == EINVAL and (got == message if whole else got.startswith(message)), (kw, rc, got)


def test_nothing_to_add_is_accepted_without_a_device():
    lib = _lib.load()
    assert _hist2d(lib, rec_x=None, rec_y=None, n=0, accumulate=1) == 0
    assert _records(lib, rec=None, n=0) == 0


# ---- the request ---------------------------------------------------------------------------------------------------------------------
KW = dict(T=60, n_layers=3, n_out=24, sizes=(6, 16, 16), B=37, max_bytes=2 << 30)
W0 = torch.zeros(5, 6)
UNITS = dict(x=(0, (3, 3, 5)), y=(2, (5, 11, 2)), bins=10, range=(-1, 1))
PROBE = dict(probe=dict(layer=0, weight=W0), bins=10, range=(-1, 1))


def test_defaults():
    H = _H()
    s = H.validate_spec(dict(UNITS), **KW)
    assert (s.begin, s.stride, s.T, s.n, s.pooled, s.probe, s.project) == (0, 1, 60, 60, False, None, None)
    assert (s.layers, s.x_layer, s.y_layer, s.pairs) == ((0, 2), 0, 2, ((3, 5), (3, 11), (5, 2)))
    assert s.edges_x.dtype == np.float32 and np.array_equal(s.edges_x, np.linspace(-1, 1, 11).astype(np.float32))
    assert np.array_equal(s.edges_y, s.edges_x)
    s = H.validate_spec(dict(x=(1, 4), y=(1, 4), bins=(3, 5), range=((0, 1), (-2, 2)), pool="chains", begin=7, stride=2), **KW)
    assert (s.layers, s.pairs, s.pooled, s.n) == ((1,), ((4, 4),), True, len(range(7, 60, 2)))
    assert np.array_equal(s.edges_x, np.linspace(0, 1, 4).astype(np.float32)) and np.array_equal(s.edges_y, np.linspace(-2, 2, 6).astype(np.float32))
    s = H.validate_spec(dict(x=(0, [1]), y=(1, [2]), bins=([0.0, 0.5, 2.0], [-1.0, 1.0])), **KW)
    assert s.edges_x.tolist() == [0.0, 0.5, 2.0] and s.edges_y.tolist() == [-1.0, 1.0]
    s = H.validate_spec(dict(PROBE), **KW)
    assert s.probe.layer == 0 and s.probe.link == "softmax" and s.probe.C == 5 and s.layers == (0,) and s.pairs == ((0, 1),)
    assert s.project.shape == (2, 5) and s.project.dtype == np.float32 and np.array_equal(s.project, H.polygon(5))
    lin = torch.nn.Linear(16, 3)
    s = H.validate_spec(dict(probe=dict(layer=1, linear=lin, link="sigmoid"), project=[[1, 0, 0], [0, 1, 0]], bins=4, range=(0, 1)), **KW)
    assert s.probe.C == 3 and s.probe.link == "sigmoid" and s.project.tolist() == [[1, 0, 0], [0, 1, 0]]


@pytest.mark.parametrize("C", [2, 3, 10])
def test_the_default_plane_is_the_class_polygon(C):
    P = _H().polygon(C)
    assert P.shape == (2, C) and P.dtype == np.float32
    for i in range(C):
        assert P[0, i] == np.float32(np.cos(2 * np.pi * i / C)) and P[1, i] == np.float32(np.sin(2 * np.pi * i / C))


@pytest.mark.parametrize("spec, word", [
    ([1, 2], "expected a dict"),
    (dict(UNITS, layers=(0,)), "unknown keys"),
    (dict(UNITS, begin=60), "begin=60"), (dict(UNITS, begin=-1), "begin=-1"), (dict(UNITS, stride=0), "stride=0"),
    (dict(UNITS, begin=1.5), "begin must be an int"),
    (dict(UNITS, probe=dict(layer=0, weight=W0)), "both forms"),
    (dict(bins=10, range=(-1, 1)), "neither form"), (dict(x=(0, (1,)), bins=10, range=(-1, 1)), "neither form"),
    (dict(UNITS, y=(2, (5, 11))), "equal length"), (dict(UNITS, x=(0, ()), y=(0, ())), "equal length"),
    (dict(UNITS, x=(0, (3, 3, 6))), "unit 6 of x out of range"), (dict(UNITS, y=(2, (5, -1, 2))), "unit -1 of y out of range"),
    (dict(UNITS, x=(3, (3, 3, 5))), "layer index 3"), (dict(UNITS, y=(-1, (3, 3, 5))), "layer index -1"),
    (dict(UNITS, x=5), r"x must be \(layer"),
    (dict(UNITS, project=np.zeros((2, 5))), "project belongs to the probe form"),
    (dict(PROBE, project=np.zeros((2, 4))), r"project has shape \(2, 4\)"), (dict(PROBE, project=np.zeros((5, 2))), "project has shape"),
    (dict(PROBE, project=np.full((2, 5), np.inf)), "project is not finite"),
    (dict(PROBE, probe=dict(layer=0, weight=W0, begin=3)), "unknown keys"),
    (dict(PROBE, probe=dict(layer=5, weight=W0)), "layer index 5"),
    (dict(PROBE, probe=dict(layer=0, weight=W0, link="tanh")), "link='tanh'"),
    (dict(PROBE, probe=dict(layer=1, weight=W0)), "weight is"),
    (dict(x=(0, (1,)), y=(0, (2,))), "bins is required"),
    (dict(UNITS, range=None), "needs range"), (dict(UNITS, bins=0), "bins=0"), (dict(UNITS, bins=129), "bins=129"),
    (dict(UNITS, bins=True), "bins"), (dict(UNITS, bins=(3, 4, 5)), "bins must be an int"),
    (dict(UNITS, range=(1, 1)), "lo < hi"), (dict(UNITS, range=((0, 1), (2, np.inf))), "finite"),
    (dict(UNITS, bins=([0, 1, 1], [0, 1])), "not strictly ascending"), (dict(UNITS, bins=([0, 1], [0, np.nan])), "not finite"),
    (dict(UNITS, bins=([0, 1], [[0, 1]])), "1-D"),
    (dict(UNITS, bins=(128, 100)), "13493 cells"),
    (dict(UNITS, pool="all"), "pool='all'"),
])
def test_invalid_requests_are_value_errors(spec, word):
    with pytest.raises(ValueError, match="mcpc_histogram2d: .*" + word):
        _H().validate_spec(spec, **KW)


@pytest.mark.parametrize("begin, stride, T", [(0, 1, 10), (3, 1, 10), (20, 3, 60), (5, 7, 33), (9, 4, 10)])
def test_sample_count_and_chunks(begin, stride, T):
    s = _H().validate_spec(dict(UNITS, begin=begin, stride=stride), **dict(KW, T=T))
    steps = list(range(begin, T, stride))
    assert s.n == len(steps) and s.steps == steps
    for S in (1, 4, 7, T):
        got, most = [], 0
        for t0 in range(0, T, S):
            first, cnt = s.chunk(t0, min(S, T - t0))
            got += [t0 + first + k * stride for k in range(cnt)]
            most = max(most, cnt)
        assert got == steps and most <= s.max_samples(S)


def test_the_size_guard():
    H = _H()
    need = 8 * 37 * 3 * 13 * 13
    assert H.result_bytes(3, 10, 10, 37, False) == need and H.result_bytes(3, 10, 10, 37, True) == need // 37
    H.validate_spec(dict(UNITS), **dict(KW, max_bytes=need))
    with pytest.raises(ValueError, match=r"mcpc_histogram2d_max_bytes.*fewer pairs or fewer bins or pool='chains'"):
        H.validate_spec(dict(UNITS), **dict(KW, max_bytes=need - 1))
    H.validate_spec(dict(UNITS, pool="chains"), **dict(KW, max_bytes=need // 37))
    with pytest.raises(ValueError, match=r"3 pairs x 13 x 13 int64 counters\) takes 4.0 KiB.*fewer pairs or fewer bins$"):
        H.validate_spec(dict(UNITS, pool="chains"), **dict(KW, max_bytes=need // 37 - 1))


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def test_reference_bins_equal_numpy_histogram2d_on_data_in_range():
    rng = np.random.default_rng(3)
    x = rng.uniform(-1.0, 1.0, size=(500, 4)).astype(np.float32)
    y = rng.normal(0.0, 0.5, size=(500, 4)).astype(np.float32).clip(-1.5, 1.5)
    ex, ey = np.linspace(-1, 1, 8).astype(np.float32), np.array([-1.5, -0.3, 0.0, 0.1, 1.5], dtype=np.float32)
    x[0, 0], y[1, 0], x[2, 1], y[2, 1] = ex[0], ey[-1], ex[-1], ey[2]                 # values on the edges, the closed last bin among them
    full = hc.ref_hist2d(x, y, ex, ey)
    assert full.shape == (4, 10, 7) and full.dtype == np.int64
    for j in range(4):
        want, _, _ = np.histogram2d(x[:, j].astype(np.float64), y[:, j].astype(np.float64), bins=[ex.astype(np.float64), ey.astype(np.float64)])
        assert np.array_equal(full[j, :7, :4], want.astype(np.int64)) and full[j].sum() == 500 == full[j, :7, :4].sum()


def test_reference_side_cells_on_the_directed_vector():
    assert np.array_equal(hc.classes(hc.SPECIAL, hc.EDGES_SPECIAL), hc.SPECIAL_CLASS)
    x, y = hc.special_pairs()
    full = hc.ref_hist2d(x, y, hc.EDGES_SPECIAL, hc.EDGES_SPECIAL)
    assert full.shape == (8, 8)
    per = np.bincount(hc.SPECIAL_CLASS, minlength=8)                                   # by hand: samples per class of one axis
    assert per.tolist() == [2, 2, 3, 3, 2, 2, 2, 1]
    assert np.array_equal(full, np.outer(per, per))                                    # every value meets every value once
    assert full[7, 7] == 1 and full[7, :7].sum() == 16 and full[:7, 7].sum() == 16     # NaN in both, in x only, in y only
    assert full[5, 6] == 4 and full[:5, :5].sum() == 12 * 12


# ---- the result ------------------------------------------------------------------------------------------------------------------------
def _result(seed=0, B=2, pairs=((0, 1), (2, 2), (1, 0))):
    H = _H()
    rng = np.random.default_rng(seed)
    n = 50
    v = rng.normal(0, 1, size=(n, B, 3)).astype(np.float32)
    v[3, 0, 0], v[4, 1, 1], v[5, 1, 2] = np.nan, np.inf, -np.inf
    ex, ey = np.linspace(-1.5, 1.5, 7).astype(np.float32), np.array([-2, -0.5, 0.5, 1.0], dtype=np.float32)
    full = hc.ref_pairs(v, v, list(pairs), ex, ey)
    return H.Histogram2D(n=n, B=B, pooled=False, pairs=list(pairs), edges_x=torch.from_numpy(ex), edges_y=torch.from_numpy(ey),
                         full=torch.from_numpy(full)), v


def test_histogram2d_arithmetic_on_hand_made_counts():
    h, v = _result()
    assert tuple(h.full.shape) == (2, 3, 9, 6) and tuple(h.counts.shape) == (2, 3, 6, 3) and h.counts.dtype == torch.int64
    assert h.N == 50 and bool((h.total() == 50).all())                                # the invariant
    assert bool((h.counts.sum((-2, -1)) + h.outside + h.nan == 50).all())
    assert h.nan[0].tolist() == [1, 0, 1] and h.nan[1].tolist() == [0, 0, 0]
    ex, ey = h.edges_x.numpy().astype(np.float64), h.edges_y.numpy().astype(np.float64)
    d = h.density()
    assert d.dtype == torch.float64
    for c in range(2):
        for k, (px, py) in enumerate(h.pairs):
            x, y = v[:, c, px].astype(np.float64), v[:, c, py].astype(np.float64)
            ok = ~(np.isnan(x) | np.isnan(y))
            want, _, _ = np.histogram2d(x[ok], y[ok], bins=[ex, ey], density=True)
            np.testing.assert_allclose(d[c, k].numpy(), want, rtol=1e-12, atol=0)
            # a marginal with its side columns is the 1-D histogram of that unit
            assert np.array_equal(h.marginal("x", sides=True)[c, k].numpy(), hist_table(v[:, c, px], h.edges_x.numpy()))
            assert np.array_equal(h.marginal("y", sides=True)[c, k].numpy(), hist_table(v[:, c, py], h.edges_y.numpy()))
    assert tuple(h.marginal("x").shape) == (2, 3, 6) and tuple(h.marginal("y").shape) == (2, 3, 3)
    assert torch.equal(h.marginal("x"), h.marginal("x", sides=True)[..., :6])
    with pytest.raises(ValueError, match="axis"):
        h.marginal("z")
    p = h.pool()
    assert p.pooled and p.N == 100 and torch.equal(p.full, h.full.sum(0)) and bool((p.total() == 100).all()) and p.pool() is p
    assert torch.equal(p.full, torch.from_numpy(hc.ref_pairs(v, v, h.pairs, h.edges_x.numpy(), h.edges_y.numpy(), pool=True)))
    assert h.cpu().full.device.type == "cpu"


def test_merge_and_cat():
    H = _H()
    a, va = _result(0)
    b, vb = _result(1)
    m = a.merge(b)
    both = np.concatenate([va, vb])
    assert m.n == 100 and torch.equal(m.full, torch.from_numpy(hc.ref_pairs(both, both, a.pairs, a.edges_x.numpy(), a.edges_y.numpy())))
    c = H.Histogram2D.cat([a, b])
    assert (c.n, c.B) == (50, 4) and torch.equal(c.full, torch.cat([a.full, b.full]))
    other, _ = _result(0, pairs=((0, 1), (2, 2), (1, 1)))
    with pytest.raises(ValueError, match="different requests"):
        a.merge(other)
    with pytest.raises(ValueError, match="different requests"):
        H.Histogram2D.cat([a, other])
    with pytest.raises(ValueError, match="pooled ones merge"):
        H.Histogram2D.cat([a.pool(), b.pool()])


def test_the_trainer_has_the_opt_in_attributes_and_they_are_off():
    import montecarlopredictivecoding_amd.predictive_coding as pc
    from montecarlopredictivecoding_amd.predictive_coding import ring
    model = torch.nn.Sequential(torch.nn.Linear(2, 2), pc.PCLayer(), torch.nn.Linear(2, 3))
    tr = pc.PCTrainer(model, T=4, plot_progress_at=[])
    assert tr.mcpc_histogram2d is None and tr.mcpc_last_histogram2d is None and tr.mcpc_histogram2d_max_bytes == 2 << 30
    import montecarlopredictivecoding_amd.utils.model as um
    assert callable(um.get_posterior_class_density)
    row = ring.REQUESTS[-1]                                                           # at the end: the order of the others is unchanged
    assert (row.attr, row.only) == ("mcpc_histogram2d", "joint histograms are counted by the fused HIP loop only")
    assert row.reducer.attr == "mcpc_last_histogram2d" and len(ring.REQUESTS) == 10

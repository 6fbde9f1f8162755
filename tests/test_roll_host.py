"""Rolling-window variability, host side (no GPU): the `mcpc_rolling` request, which samples emit a row however the call is sliced, the
fp64 arithmetic from the pooled sums to the mean and spread, joining results, `carry=`, and the C entry points' declaration, binding and
argument checks; and the sequential loop the kernel is held to against a two-pass variance of every window."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from montecarlopredictivecoding_amd import _lib
from montecarlopredictivecoding_amd import rolling as R
from tests.roll_cases import noise, onset, pooled, ref_roll, two_pass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (6, 16, 16)
KW = dict(T=60, n_layers=3, n_out=24, sizes=SIZES, B=37, max_bytes=2 << 30)


def test_defaults():
    spec = R.validate_spec(dict(layers=(0,), window=8), **KW)
    assert (spec.begin, spec.stride, spec.layers, spec.outputs, spec.window, spec.every, spec.pool, spec.carry, spec.T, spec.n) == \
        (0, 1, (0,), None, 8, 1, "all", None, 60, 60)
    assert spec.columns == (("x0", 6),) and spec.n_seen == 0 and spec.rows == 53 and spec.steps == list(range(7, 60))
    spec = R.validate_spec(dict(outputs="sigmoid", window=2, pool=None), **KW)          # layers defaults to (): the read-out alone
    assert spec.layers == () and spec.columns == (("out", 24),) and spec.pool is None and spec.rows == 59
    spec = R.validate_spec(dict(begin=13, stride=3, layers=(2, 0, 2), outputs="identity", window=5, every=4), **KW)
    assert spec.layers == (0, 2) and spec.n == len(range(13, 60, 3)) == 16 and spec.columns == (("x0", 6), ("x2", 16), ("out", 24))
    assert spec.rows == 3 and spec.steps == [13 + 3 * 4, 13 + 3 * 8, 13 + 3 * 12]          # samples 4, 8, 12 end a window
    assert R.validate_spec(dict(layers=1, window=3), **KW).columns == (("x1", 16),)
    assert R.validate_spec(dict(layers=(0,), window=100), **KW).rows == 0                    # a stream shorter than the window


@pytest.mark.parametrize("spec, word", [
    (dict(layers=(0,), window=8, strid=2), "unknown keys"),
    (dict(layers=(0,), window=8, begin=-1), "begin"),
    (dict(layers=(0,), window=8, begin=60), "begin"),
    (dict(layers=(0,), window=8, begin=1.0), "begin must be an int"),
    (dict(layers=(0,), window=8, begin=True), "begin must be an int"),
    (dict(layers=(0,), window=8, stride=0), "stride"),
    (dict(layers=(0,), window=8, stride="2"), "stride must be an int"),
    (dict(layers=(0,), window=8, every=0), "every=0"),
    (dict(layers=(0,), window=8, every=2.0), "every must be an int"),
    (dict(layers=(0, 3), window=8), "layer index"),
    (dict(layers=(-1,), window=8), "layer index"),
    (dict(layers=(True,), window=8), "layer index"),
    (dict(layers=1.5, window=8), "sequence of layer indices"),
    (dict(window=8), "no columns"),
    (dict(layers=(), window=8), "no columns"),
    (dict(outputs="softmax", window=8), "outputs"),
    ([("begin", 0)], "expected a dict"),
    (dict(layers=(0,)), "window is required"),
    (dict(layers=(0,), window=None), "window is required"),
    (dict(layers=(0,), window=1), "window=1"),
    (dict(layers=(0,), window=-3), "window=-3"),
    (dict(layers=(0,), window=8.0), "window must be an int"),
    (dict(layers=(0,), window=True), "window must be an int"),
    (dict(layers=(0,), window=8, pool="chains"), "pool='chains'"),
    (dict(layers=(0,), window=8, carry="yes"), "carry must be the Rolling"),
    (dict(layers=(0,), window=8, max_lag=3), "unknown keys"),
])
def test_invalid_requests_are_value_errors(spec, word):
    with pytest.raises(ValueError, match=word):
        R.validate_spec(spec, **KW)


def test_outputs_need_a_read_out():
    with pytest.raises(ValueError, match="read-out"):
        R.validate_spec(dict(outputs="identity", window=4), **dict(KW, n_layers=2, n_out=0))
    assert R.validate_spec(dict(layers=(1,), window=4), **dict(KW, n_layers=2, n_out=0)).layers == (1,)


def test_the_size_guard_names_the_size_and_the_ways_out():
    spec = dict(layers=(0, 1, 2), window=8)
    E = 37 * 38
    rows = 53
    state = E * (8 + 8 + 4 * 8)                                        # s1, s2 in fp64, 8 samples in fp32
    workspace = -(-37 * 16 // 256) * 60 * 32                           # the widest block's workgroups x the call's samples x 4 doubles
    need = state + workspace + 3 * rows * 32
    ok = R.validate_spec(spec, **dict(KW, max_bytes=need))
    assert R.request_bytes(ok.columns, 37, 8, 60, rows, "all") == need
    with pytest.raises(ValueError, match=r"37 chains x 38 units x a window of 8 samples.*53 rows\) take .*KiB.*mcpc_rolling_max_bytes"
                                         r".*a shorter window, fewer layers or a larger every"):
        R.validate_spec(spec, **dict(KW, max_bytes=need - 1))
    assert R.validate_spec(dict(spec, window=7), **dict(KW, max_bytes=need - 1)).window == 7
    # every element's variance is kept with pool=None: 8 B per row and element more
    assert R.request_bytes(ok.columns, 37, 8, 60, rows, None) == need + rows * E * 8
    with pytest.raises(ValueError, match="of every element in fp64"):
        R.validate_spec(dict(spec, pool=None), **dict(KW, max_bytes=need))
    # the figure's request fits the default; the same with every element kept does not
    fig = dict(T=8000, n_layers=3, n_out=784, sizes=(20, 128, 128), B=256, max_bytes=2 << 30)
    assert R.validate_spec(dict(layers=(0, 1, 2), window=1000), **fig).rows == 7001
    with pytest.raises(ValueError, match="GiB"):
        R.validate_spec(dict(layers=(0, 1, 2), window=1000, pool=None), **fig)


@pytest.mark.parametrize("begin, stride, T", [(0, 1, 1), (13, 3, 60), (59, 7, 60), (200, 1, 1000), (3, 4, 5), (0, 60, 60)])
def test_sample_count_and_chunks(begin, stride, T):
    spec = R.validate_spec(dict(layers=(0,), window=4, begin=begin, stride=stride), **dict(KW, T=T))
    steps = list(range(begin, T, stride))
    assert spec.n == len(steps)
    for S in (1, 5, 7, T):                               # however the call is sliced, the chunks name exactly the sample steps, in order
        got = []
        for t0 in range(0, T, S):
            n = min(S, T - t0)
            first, cnt = spec.chunk(t0, n)
            assert cnt == 0 or (0 <= first and first + (cnt - 1) * stride < n)
            got += [t0 + first + k * stride for k in range(cnt)]
        assert got == steps


@pytest.mark.parametrize("W", [2, 5, 16])
@pytest.mark.parametrize("every", [1, 3, 4, 7])
def test_emitted_rows_across_chunk_boundaries(W, every):
    """Chunks whose lengths are no multiple of `every`: the rows of the chunks add up to the stream's, and each chunk emits exactly the
    samples j >= W - 1 with (j - (W - 1)) % every == 0 that lie in it."""
    spec = R.validate_spec(dict(layers=(0,), window=W, every=every), **dict(KW, T=150))
    assert spec.rows == len([j for j in range(150) if j >= W - 1 and (j - (W - 1)) % every == 0])
    for chunks in ([150], [1, 3, W - 1, W, W + 1], [5] * 30, [0, 2, 0, 11]):
        chunks = chunks + [150 - sum(chunks)]
        seen, total = 0, 0
        for c in chunks:
            want = len([j for j in range(seen, seen + c) if j >= W - 1 and (j - (W - 1)) % every == 0])
            assert spec.chunk_rows(seen, c) == R.emitted_rows(seen, c, W, every) == want, (seen, c)
            seen, total = seen + c, total + want
        assert total == spec.rows
    # a carried stream: the second call's first row covers W - 1 samples of the first
    first = _result(noise(40, 6, seed=1), W, every, B=2)
    second = R.validate_spec(dict(layers=(0,), window=W, every=every, carry=first), **dict(KW, T=30, B=2, sizes=(3, 16, 16)))
    assert second.n_seen == 40 and second.rows == len([j for j in range(40, 70) if (j - (W - 1)) % every == 0])
    assert second.steps == [j - 40 for j in range(40, 70) if (j - (W - 1)) % every == 0]
    if every == 1:
        assert second.steps[0] == 0


def _result(g, W, every=1, B=1, keep_var=False, name="x0", layers=(0,), T=None):
    """g: fp32 [n, B * w] -> Rolling of one block from the tables of the host loop."""
    n, E = g.shape
    w = E // B
    v, s1, s2, samples = ref_roll(g, W, every)
    state = [dict(s1=torch.from_numpy(s1).reshape(B, w), s2=torch.from_numpy(s2).reshape(B, w),
                  hist=torch.zeros(W, B, w), n_seen=n)]
    return R.Rolling(B=B, window=W, every=every, stride=1, layers=layers, outputs=None, columns=((name, w),), T=n if T is None else T,
                     n_seen=n, steps=torch.tensor(samples, dtype=torch.int64), names=[name],
                     sums={name: torch.from_numpy(pooled(v))}, var={name: torch.from_numpy(v).reshape(-1, B, w)} if keep_var else {},
                     state=state)


def test_the_statistics_are_those_of_the_rolling_standard_deviations():
    g = onset(120, 12, seed=3, at=70)
    r = _result(g, 16, keep_var=True, B=3)
    sd = np.sqrt(two_pass(g, 16))                                                      # [105, 12]
    assert r.rows == 105 and tuple(r.var["x0"].shape) == (105, 3, 4) and r.steps.tolist() == list(range(15, 120))
    np.testing.assert_allclose(r.mean_std("x0").numpy(), sd.mean(1), rtol=1e-12)
    np.testing.assert_allclose(r.std_std("x0").numpy(), sd.std(1, ddof=1), rtol=1e-9)
    np.testing.assert_allclose(r.sem("x0").numpy(), sd.std(1, ddof=1) / np.sqrt(12), rtol=1e-9)
    np.testing.assert_allclose(r.mean_var("x0").numpy(), (sd * sd).mean(1), rtol=1e-12)
    assert bool((r.count("x0") == 12).all()) and r.mean_std("x0").dtype == torch.float64
    # the quench shows: the windows wholly after the onset are a quarter as spread as those wholly before it
    m = r.mean_std("x0").numpy()
    assert m[:50].min() > 3 * m[-30:].max()
    with pytest.raises(KeyError, match="x1"):
        r.mean_std("x1")


def test_a_non_finite_element_is_a_missing_count():
    g = noise(30, 8, seed=5)
    g[10, 3] = np.inf
    r = _result(g, 4)
    c = r.count("x0").numpy()
    assert (c[:7] == 8).all() and (c[7:] == 7).all()                                   # from the window that holds sample 10 on, for ever
    assert bool(torch.isfinite(r.mean_std("x0")).all()) and bool(torch.isfinite(r.std_std("x0")).all())


def test_all_pools_the_blocks_and_cat_joins():
    g = noise(50, 20, seed=7)
    a, b = _result(np.ascontiguousarray(g[:, :8]), 5, B=2, keep_var=True), _result(np.ascontiguousarray(g[:, 8:]), 5, B=2, name="x1",
                                                                                   keep_var=True)
    both = R.Rolling(B=2, window=5, every=1, stride=1, layers=(0, 1), outputs=None, columns=(("x0", 4), ("x1", 6)), T=50, n_seen=50,
                     steps=a.steps, names=["x0", "x1"], sums={"x0": a.sums["x0"], "x1": b.sums["x1"]})
    allb = both.all()
    sd = np.sqrt(two_pass(g, 5))
    assert allb.names == ["all"] and allb.columns == (("all", 10),) and allb.rows == 46
    np.testing.assert_allclose(allb.mean_std("all").numpy(), sd.mean(1), rtol=1e-12)
    np.testing.assert_allclose(allb.sem("all").numpy(), sd.std(1, ddof=1) / np.sqrt(20), rtol=1e-9)
    # along the chains: the sums add, the variances are joined
    whole = _result(np.ascontiguousarray(g[:, :12]), 5, B=3, keep_var=True)
    parts = [_result(np.ascontiguousarray(g[:, :8]), 5, B=2, keep_var=True), _result(np.ascontiguousarray(g[:, 8:12]), 5, B=1, keep_var=True)]
    cat = R.Rolling.cat(parts, dim="chains")
    assert cat.B == 3 and torch.equal(cat.var["x0"], whole.var["x0"]) and torch.equal(cat.steps, whole.steps)
    np.testing.assert_allclose(cat.sums["x0"].numpy(), whole.sums["x0"].numpy(), rtol=1e-14)
    # in time: the rows follow one another, and the later call's steps count on from the earlier call's T
    first, second = _result(g[:30], 5, B=2, T=30), _result(g[30:], 5, B=2, T=20)
    t = R.Rolling.cat([first, second])
    assert t.rows == first.rows + second.rows and t.T == 50 and t.n_seen == second.n_seen and t.state is second.state
    assert t.steps.tolist() == first.steps.tolist() + [30 + s for s in second.steps.tolist()]
    assert torch.equal(t.sums["x0"], torch.cat([first.sums["x0"], second.sums["x0"]]))
    with pytest.raises(ValueError, match="different requests"):
        R.Rolling.cat([first, _result(g[30:], 6, B=2)])
    with pytest.raises(ValueError, match="different requests"):
        R.Rolling.cat([parts[0], _result(g[:40, :4], 5, B=1, keep_var=True)], dim="chains")
    with pytest.raises(ValueError, match="dim="):
        R.Rolling.cat([first, second], dim="units")


def test_a_carry_of_another_request_is_refused():
    kw = dict(KW, B=2, sizes=(3, 16, 16))
    first = _result(noise(40, 6, seed=1), 8, every=2, B=2)
    ok = R.validate_spec(dict(layers=(0,), window=8, every=2, carry=first), **kw)
    assert ok.carry is first and ok.n_seen == 40
    for change, word in [(dict(window=9), "window=8 there, 9 here"), (dict(every=1), "every=2 there, 1 here"),
                         (dict(stride=2), "stride=1 there, 2 here"), (dict(layers=(0, 1)), r"layers=\(0,\) there, \(0, 1\) here"),
                         (dict(outputs="identity"), "outputs=None there, 'identity' here")]:
        with pytest.raises(ValueError, match="carry is the result of a different request: .*" + word):
            R.validate_spec(dict(dict(layers=(0,), window=8, every=2, carry=first), **change), **kw)
    with pytest.raises(ValueError, match="B=2 there, 37 here"):
        R.validate_spec(dict(layers=(0,), window=8, every=2, carry=first), **KW)
    with pytest.raises(ValueError, match="carry must be the Rolling"):
        R.validate_spec(dict(layers=(0,), window=8, every=2, carry=first.all()), **kw)             # a pooled view keeps no state


def test_the_trainer_has_the_opt_in_attributes_and_they_are_off():
    import montecarlopredictivecoding_amd.predictive_coding as pc
    model = torch.nn.Sequential(torch.nn.Linear(2, 2), pc.PCLayer(), torch.nn.Linear(2, 3))
    tr = pc.PCTrainer(model, T=4, plot_progress_at=[])
    assert tr.mcpc_rolling is None and tr.mcpc_last_rolling is None and tr.mcpc_rolling_max_bytes == 2 << 30
    import montecarlopredictivecoding_amd.utils.model as um
    assert callable(um.get_variability_time_course)


def _args(text, name):
    """The parameter list of `name` in C text, comments removed: [(type, identifier)]."""
    code = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1)
    out = []
    for a in decl.split(","):
        a = " ".join(a.split())
        m = re.match(r"(.*?)(\w+)$", a)
        out.append((m.group(1).replace(" ", ""), m.group(2).rstrip("_")))
    return out


def test_header_source_and_binding_agree_on_both_signatures():
    header = open(os.path.join(ROOT, "include", "mcpc.h")).read()
    source = open(os.path.join(ROOT, "montecarlopredictivecoding_amd", "csrc", "mcpc_records.hip")).read()       # the unit of the stateless reducers
    assert re.search(r"#define\s+MCPC_ABI_VERSION\s+4\b", header) and _lib.ABI_VERSION == 4
    ctype = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64}
    for name, count, res in (("mcpc_roll_accumulate", 18, C.c_int), ("mcpc_roll_workspace_bytes", 3, C.c_int64)):
        h, s = _args(header, name), _args(source, name)
        assert h == s and len(h) == count, name
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is res and len(argtypes) == count
        for (t, ident), a in zip(h, argtypes):
            assert a is (C.c_void_p if t.endswith("*") else ctype[t]), (name, ident, t)
    names = [i for _, i in _args(header, "mcpc_roll_accumulate")]
    assert names == ["device", "rec", "B", "width", "first", "stride", "n", "transform", "window", "every", "n_seen", "s1", "s2", "hist",
                     "out_elem", "out_pool", "workspace", "stream"]
    assert _lib.SYMBOLS["mcpc_roll_accumulate"][1][10] is C.c_int64                       # n_seen is 64-bit
    from montecarlopredictivecoding_amd import engine
    assert callable(engine.roll_accumulate) and callable(engine.roll_workspace_bytes)
    lib = _lib.load()
    assert lib.mcpc_abi_version() == 4 and hasattr(lib, "mcpc_roll_accumulate") and hasattr(lib, "mcpc_roll_workspace_bytes")
    # the workspace: 4 doubles per workgroup of 256 elements and sample
    assert lib.mcpc_roll_workspace_bytes(37, 3, 150) == 1 * 150 * 32 and lib.mcpc_roll_workspace_bytes(300, 5, 7) == 6 * 7 * 32
    assert lib.mcpc_roll_workspace_bytes(0, 5, 7) == -1 and "B=0" in lib.mcpc_last_error().decode()
    for W, every, seen, n in [(2, 1, 0, 150), (5, 4, 3, 9), (16, 4, 40, 1), (64, 1, 10, 50), (5, 3, 0, 4)]:
        assert engine.roll_rows(seen, n, W, every) == R.emitted_rows(seen, n, W, every)


def test_argument_errors_are_refused_before_any_device_work():
    """Every MCPC_EINVAL case returns -1 with a message and touches no device: the pointers are never dereferenced (this machine need
    not have a GPU)."""
    lib = _lib.load()
    p = [C.c_void_p(0x1000 * (i + 1)) for i in range(7)]             # never dereferenced: every call below is refused

    def call(rec=p[0], B=3, width=5, first=0, stride=1, n=4, transform=0, window=3, every=1, n_seen=0, s1=p[1], s2=p[2], hist=p[3],
             out_elem=p[4], out_pool=p[5], workspace=p[6]):
        rc = lib.mcpc_roll_accumulate(0, rec, B, width, first, stride, n, transform, window, every, n_seen, s1, s2, hist, out_elem,
                                      out_pool, workspace, None)
        return rc, lib.mcpc_last_error().decode()

    for kw, word in [(dict(s1=None), "s1 is null"), (dict(s2=None), "s2 is null"), (dict(hist=None), "hist is null"),
                     (dict(out_elem=None, out_pool=None), "both null"), (dict(rec=None), "rec is null with n=4"), (dict(B=0), "B=0"),
                     (dict(width=0), "width=0"), (dict(stride=0), "stride=0"), (dict(first=-1), "first=-1"), (dict(n=-1), "n=-1"),
                     (dict(n_seen=-1), "n_seen=-1"), (dict(window=1), "window=1"), (dict(window=0), "window=0"),
                     (dict(every=0), "every=0"), (dict(transform=2), "unknown transform 2"), (dict(transform=-1), "unknown transform -1"),
                     (dict(workspace=None), "workspace is null")]:
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("roll:") and word in msg, (kw, rc, msg)
    # nothing to add in the middle of a stream: accepted without a device, and nothing is read
    assert call(n=0, n_seen=7, rec=None)[0] == 0
    assert call(n=0, n_seen=7, rec=None, out_pool=None, workspace=None)[0] == 0


SERIES = [("white", lambda: noise(400, 5, seed=11)), ("offset", lambda: noise(400, 5, seed=12, mean=8.0, scale=0.5)),
          ("onset", lambda: onset(400, 5, seed=13, at=250))]


@pytest.mark.parametrize("W, every", [(2, 1), (5, 1), (16, 4), (64, 1), (100, 7)])
@pytest.mark.parametrize("name, make", SERIES)
def test_the_loop_is_a_two_pass_variance_within_its_rounding_bound(name, make, W, every):
    """Each sample adds at most 4 roundings to sums bounded by W D^2, D = max |g| of the element: |v - two-pass| <= 16 j 2^-53 D^2 at
    stream index j, the bound computed here from the data, per element and row."""
    g = make()
    v, _, _, samples = ref_roll(g, W, every)
    want = two_pass(g, W, every)
    assert v.shape == want.shape and v.shape[0] == len(samples) > 0
    D = np.abs(g.astype(np.float64)).max(0)
    bound = 16 * (np.asarray(samples, dtype=np.float64)[:, None] + 1) * 2.0 ** -53 * D[None, :] ** 2
    err = np.abs(v - want)
    print("%s W=%d: max error %.3g, the bound there %.3g" % (name, W, err.max(), bound.reshape(-1)[err.argmax()]))
    assert (err <= bound).all()

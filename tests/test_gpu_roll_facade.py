"""Rolling-window variability on the device, the trainer: `PCTrainer.mcpc_rolling` against the recorded trajectory of the same call put
through the sequential host loop (tests/roll_cases.py): the variances bitwise, the pooled sums within 4 E 2^-53, however the call is
sliced, and across two calls with `carry=`."""
import warnings

import numpy as np
import pytest
import torch

from tests.roll_cases import pooled, ref_roll

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES, N_OUT, B, T = (5, 12, 9), 14, 37, 60
W = 8
SPEC = dict(begin=0, stride=1, layers=(0, 2), outputs="identity", window=W, every=1, pool=None)
NAMES = ["x0", "x2", "out"]
WIDTH = dict(x0=5, x2=9, out=14)
OTHERS = dict(mcpc_moments=dict(begin=20, stride=1, layers=(0, 2), outputs="identity"),
              mcpc_chain_energies=dict(begin=7, stride=5),
              mcpc_covariance=dict(begin=13, stride=3, layers=(0, 2), outputs="identity"),
              mcpc_histogram=dict(begin=20, stride=3, layers=(0, 2), outputs="identity", bins=19, range=(-3.0, 3.0)),
              mcpc_autocovariance=dict(begin=20, stride=1, layers=(0, 2), outputs="identity", max_lag=8),
              mcpc_probe=dict(begin=10, stride=2, layer=1, weight=torch.linspace(-1, 1, 36).reshape(3, 12), bias=None, link="softmax"),
              mcpc_cloud=dict(begin=5, stride=4, layer=2, units=(0, 3, 8)),
              mcpc_errors=dict(begin=11, stride=3, layers=(1, 2), quantity="error", outputs="error", covariance="chain"))


def _net(device):
    """5-12-9 -> 14, ReLU, Bernoulli loss; the same weights, data and x0 on whichever device."""
    import montecarlopredictivecoding_amd.utils.model as um
    torch.manual_seed(3)
    cfg = dict(input_size=SIZES[0], hidden_size=SIZES[1], hidden2_size=SIZES[2], output_size=N_OUT, activation_fn="relu")
    model = um.get_model(cfg, False)
    g = torch.Generator().manual_seed(8)
    x0 = [torch.randn(B, n, generator=g) for n in SIZES]
    for layer, x in zip([m for m in model if hasattr(m, "get_x")], x0):
        layer._sample_x_fn = lambda inp, _x=x: _x.clone().to(inp["mu"].device)
    data = (torch.rand(B, N_OUT, generator=g) < 0.3).float()
    model.to(device)
    return um, model, data.to(device), torch.zeros(B, SIZES[0], device=device)


def _trainer(model, update_p_at="never"):
    import montecarlopredictivecoding_amd.predictive_coding as pc
    tr = pc.PCTrainer(model, T=T, optimizer_x_fn=torch.optim.SGD, optimizer_x_kwargs={"lr": 0.05}, update_p_at=update_p_at,
                      accumulate_p_at=list(range(40, T)) if update_p_at == "last" else "never",
                      optimizer_p_fn=torch.optim.Adam, optimizer_p_kwargs={"lr": 0.01}, plot_progress_at=[])
    tr.mcpc_seed = 5
    return tr


def _run(tr, um, data, inputs, every_t=True, xs=True, outputs=True, sample=True):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return tr.train_on_batch(inputs=inputs, callback_after_t=um.random_step, callback_after_t_kwargs={"_pc_trainer": tr},
                                 is_log_progress=False, is_return_results_every_t=every_t, is_return_xs=xs, is_return_outputs=outputs,
                                 is_sample_x_at_batch_start=sample, loss_fn=um.bernoulli_fn, loss_fn_kwargs={"_target": data, "_var": None})


def _call(um, model, data, inputs, roll, chunk=None, max_bytes=None, update_p_at="never", others=None, **kw):
    import montecarlopredictivecoding_amd.predictive_coding.pc_trainer as pt
    tr = _trainer(model, update_p_at)
    tr.mcpc_rolling = roll
    for k, v in (others or {}).items():
        setattr(tr, k, v)
    if chunk is not None:
        tr.mcpc_moments_chunk_bytes = chunk
    if max_bytes is not None:
        tr.mcpc_rolling_max_bytes = max_bytes
    base = pt._PHILOX_STEPS[0]
    res = _run(tr, um, data, inputs, **kw)
    pt._PHILOX_STEPS[0] = base                               # the next run replays the same noise
    return tr, res


def _trajectory(res, steps):
    """Per block of SPEC: fp32 [n, B, w] from the records of the sample steps."""
    out = {f"x{l}": np.stack([res["xs"][t][l].detach().cpu().numpy() for t in steps]) for l in (0, 2)}
    out["out"] = torch.stack([res["outputs"][t].detach() for t in steps]).cpu().numpy()
    return out


def _same(a, b):
    assert (a.B, a.window, a.every, a.names, a.n_seen) == (b.B, b.window, b.every, b.names, b.n_seen) and torch.equal(a.steps, b.steps)
    for nm in a.names:
        assert torch.equal(a.sums[nm], b.sums[nm]) and torch.equal(a.var[nm], b.var[nm]), nm
    for s, t in zip(a.state, b.state):
        assert s["n_seen"] == t["n_seen"] and all(torch.equal(s[k], t[k]) for k in ("s1", "s2", "hist"))


def _against_the_host_loop(r, traj, every=1, first_row=0, steps=None):
    """`traj[name]` the samples of the whole stream; rows first_row .. of its host loop are what `r` holds."""
    assert r.names == NAMES and r.B == B and r.window == W
    for nm in NAMES:
        g = traj[nm]
        n, E = g.shape[0], B * WIDTH[nm]
        v, s1, s2, samples = ref_roll(g.reshape(n, -1), W, every)
        v = v[first_row:]
        assert r.rows == v.shape[0] and r.var[nm].dtype == r.sums[nm].dtype == torch.float64 and r.var[nm].device.type == "cuda"
        assert tuple(r.var[nm].shape) == (r.rows, B, WIDTH[nm]) and tuple(r.sums[nm].shape) == (r.rows, 4)
        assert np.array_equal(r.var[nm].cpu().numpy().reshape(r.rows, -1), v), nm                 # bitwise
        want, got = pooled(v), r.sums[nm].cpu().numpy()
        assert np.array_equal(got[:, 3], want[:, 3]) and (got[:, 3] == E).all()
        assert (np.abs(got[:, :3] - want[:, :3]) <= 4 * E * 2.0 ** -53 * np.abs(want[:, :3])).all(), nm
        sd = np.sqrt(v)
        np.testing.assert_allclose(r.mean_std(nm).cpu().numpy(), sd.mean(1), rtol=1e-12)
        np.testing.assert_allclose(r.sem(nm).cpu().numpy(), sd.std(1, ddof=1) / np.sqrt(E), rtol=1e-9)
        st = r.state[NAMES.index(nm)]
        assert st["n_seen"] == n and st["s1"].device.type == "cuda"
        assert np.array_equal(st["s1"].cpu().numpy().reshape(-1), s1) and np.array_equal(st["s2"].cpu().numpy().reshape(-1), s2)
    if steps is not None:
        assert r.steps.tolist() == steps


@pytest.fixture(scope="module")
def reference_call():
    """The call of SPEC: its result and the trajectory the same call returned.  Shared, never modified."""
    um, model, data, inputs = _net(DEV)
    tr, res = _call(um, model, data, inputs, dict(SPEC))
    assert tr.last_call_mode == "fused" and tr.last_record_slices == 1
    return tr.mcpc_last_rolling, _trajectory(res, range(T))


def test_the_result_is_the_host_loop_on_the_recorded_trajectory(reference_call):
    r, traj = reference_call
    _against_the_host_loop(r, traj, steps=list(range(W - 1, T)))
    assert r.rows == T - W + 1 and r.T == T and r.n_seen == T
    pooled_all = r.all()
    sd = np.sqrt(np.concatenate([r.var[nm].cpu().numpy().reshape(r.rows, -1) for nm in NAMES], axis=1))
    np.testing.assert_allclose(pooled_all.mean_std("all").cpu().numpy(), sd.mean(1), rtol=1e-12)
    np.testing.assert_allclose(pooled_all.std_std("all").cpu().numpy(), sd.std(1, ddof=1), rtol=1e-9)


def test_begin_stride_every_and_the_pooled_form():
    um, model, data, inputs = _net(DEV)
    tr, res = _call(um, model, data, inputs, dict(SPEC, begin=7, stride=2, every=3))
    steps = list(range(7, T, 2))
    _against_the_host_loop(tr.mcpc_last_rolling, _trajectory(res, steps), every=3, steps=[steps[j] for j in range(W - 1, len(steps), 3)])
    pooled_only, _ = _call(um, model, data, inputs, dict(SPEC, begin=7, stride=2, every=3, pool="all"), xs=False, outputs=False)
    p = pooled_only.mcpc_last_rolling
    assert p.var == {} and all(torch.equal(p.sums[nm], tr.mcpc_last_rolling.sums[nm]) for nm in NAMES)


@pytest.mark.parametrize("per_slice", [1, 5, 7])
def test_a_sliced_call_gives_the_same_bits(reference_call, per_slice):
    """Slices of fewer than W = 8 steps: every window crosses slice boundaries through the kernel's history."""
    um, model, data, inputs = _net(DEV)
    step_bytes = 4 * B * (SIZES[0] + SIZES[2] + N_OUT)
    cut, _ = _call(um, model, data, inputs, dict(SPEC), chunk=per_slice * step_bytes, xs=False, outputs=False)
    assert cut.last_record_slices == -(-T // per_slice) > 2
    _same(cut.mcpc_last_rolling, reference_call[0])


def test_two_calls_with_carry_are_one_stream():
    """The second call continues the first one's stream: its first row covers W - 1 samples of the first call."""
    import montecarlopredictivecoding_amd.predictive_coding.pc_trainer as pt
    from montecarlopredictivecoding_amd.rolling import Rolling
    um, model, data, inputs = _net(DEV)
    tr = _trainer(model)
    base = pt._PHILOX_STEPS[0]
    tr.mcpc_rolling = dict(SPEC)
    res1 = _run(tr, um, torch.zeros_like(data), inputs)
    first = tr.mcpc_last_rolling
    kept = {k: v.clone() for k, v in first.state[0].items() if k != "n_seen"}
    tr.mcpc_rolling = dict(SPEC, carry=first)
    tr.mcpc_moments_chunk_bytes = 5 * 4 * B * (SIZES[0] + SIZES[2] + N_OUT)              # and the second call in slices of a few steps
    res2 = _run(tr, um, data, inputs, sample=False)
    second = tr.mcpc_last_rolling
    pt._PHILOX_STEPS[0] = base
    assert tr.last_record_slices > 12 and second.rows == T and second.steps.tolist() == list(range(T)) and second.n_seen == 2 * T
    t1, t2 = _trajectory(res1, range(T)), _trajectory(res2, range(T))
    whole = {nm: np.concatenate([t1[nm], t2[nm]]) for nm in NAMES}
    _against_the_host_loop(second, whole, first_row=T - W + 1)
    both = Rolling.cat([first, second])
    _against_the_host_loop(both, whole, steps=list(range(W - 1, 2 * T)))
    assert all(torch.equal(kept[k], first.state[0][k]) for k in kept)                    # the first result keeps its own state
    with pytest.raises(ValueError, match="carry is the result of a different request: window=8 there, 9 here"):
        tr.mcpc_rolling = dict(SPEC, window=9, carry=first)
        _run(tr, um, data, inputs, sample=False)


def test_all_nine_features_compose_in_a_learning_call():
    um, model, data, inputs = _net(DEV)
    w0 = {k: v.clone() for k, v in model.state_dict().items() if "_x" not in k}
    runs = []
    for roll in (None, dict(SPEC)):
        model.load_state_dict(w0, strict=False)
        for p in model.parameters():
            p.grad = None
        tr, res = _call(um, model, data, inputs, roll, update_p_at="last", xs=False, outputs=False, every_t=False,
                        others={k: (dict(v)) for k, v in OTHERS.items()})
        assert tr.last_call_mode == "fused"
        lin = [p for m in model if isinstance(m, torch.nn.Linear) for p in m.parameters()]
        runs.append((tr, [p.grad.clone() for p in lin], [p.detach().clone() for p in lin],
                     [x.detach().clone() for x in tr.get_model_xs()], {k: res[k] for k in ("loss", "energy", "overall")}))
    (t0, g0, p0, x0, e0), (t1, g1, p1, x1, e1) = runs
    assert t0.mcpc_last_rolling is None and t1.mcpc_last_rolling.rows == T - W + 1
    assert e0 == e1
    for a, b in zip(g0 + p0 + x0, g1 + p1 + x1):
        assert torch.equal(a, b)                                                     # param.grad, the parameters, x: bitwise
    m, k = t0.mcpc_last_moments, t1.mcpc_last_moments
    for p, q in ((m.out_sum, k.out_sum), (m.out_sumsq, k.out_sumsq), (m.x_sum[0], k.x_sum[0]), (m.x_sumsq[2], k.x_sumsq[2])):
        assert torch.equal(p, q)
    e, f = t0.mcpc_last_chain_energies, t1.mcpc_last_chain_energies
    assert e.steps == f.steps and torch.equal(e.loss, f.loss) and torch.equal(e.energy, f.energy) and torch.equal(e.overall, f.overall)
    a, b = t0.mcpc_last_covariance, t1.mcpc_last_covariance
    assert torch.equal(a.sum, b.sum) and torch.equal(a.outer, b.outer) and a.columns == b.columns
    h, i = t0.mcpc_last_histogram, t1.mcpc_last_histogram
    for nm in h.names:
        for fld in ("counts", "under", "over", "nan"):
            assert torch.equal(getattr(h, fld)[nm], getattr(i, fld)[nm])
    a, b = t0.mcpc_last_autocovariance, t1.mcpc_last_autocovariance
    for nm in a.names:
        for fld in ("lagged", "sum", "head", "tail"):
            assert torch.equal(getattr(a, fld)[nm], getattr(b, fld)[nm])
    a, b = t0.mcpc_last_probe, t1.mcpc_last_probe
    assert torch.equal(a.psum, b.psum) and torch.equal(a.psumsq, b.psumsq) and torch.equal(a.votes, b.votes) and torch.equal(a.entsum, b.entsum)
    assert torch.equal(t0.mcpc_last_cloud.points, t1.mcpc_last_cloud.points)
    a, b = t0.mcpc_last_errors, t1.mcpc_last_errors
    assert a.names == b.names == ["e1", "e2", "eout"] and a.n == b.n == len(range(11, T, 3))
    for nm in a.names:
        assert torch.equal(a.sum[nm], b.sum[nm]) and torch.equal(a.sumsq[nm], b.sumsq[nm]), nm
    assert a.covariance.columns == b.covariance.columns and torch.equal(a.covariance.sum, b.covariance.sum)
    assert torch.equal(a.covariance.outer, b.covariance.outer)


def test_the_side_stream_reduces_the_same_bits_beside_other_reducers():
    """The driver's side-stream branch with more than one reducer: moments on the side stream while the histogram and the
    autocovariance stay on the call's own, in slices of 7 steps, against the same call with everything on the call's own stream."""
    import montecarlopredictivecoding_amd.predictive_coding.pc_trainer as pt
    um, model, data, inputs = _net(DEV)
    asked = {k: OTHERS[k] for k in ("mcpc_moments", "mcpc_histogram", "mcpc_autocovariance")}
    runs = []
    for side in (True, False):
        tr = _trainer(model)
        for k, v in asked.items():
            setattr(tr, k, dict(v))
        tr.mcpc_moments_side_stream = side
        tr.mcpc_moments_chunk_bytes = 7 * 4 * B * (SIZES[0] + SIZES[2] + N_OUT)
        base = pt._PHILOX_STEPS[0]
        _run(tr, um, data, inputs, xs=False, outputs=False)
        pt._PHILOX_STEPS[0] = base
        assert tr.last_call_mode == "fused" and tr.last_record_slices == -(-T // 7)
        runs.append(tr)
    t0, t1 = runs
    m, k = t0.mcpc_last_moments, t1.mcpc_last_moments
    assert m.n == k.n == T - 20
    for p, q in zip([m.out_sum, m.out_sumsq, m.x_sum[0], m.x_sumsq[0], m.x_sum[2], m.x_sumsq[2]],
                    [k.out_sum, k.out_sumsq, k.x_sum[0], k.x_sumsq[0], k.x_sum[2], k.x_sumsq[2]]):
        assert torch.equal(p, q)
    h, i = t0.mcpc_last_histogram, t1.mcpc_last_histogram
    assert h.names == i.names == NAMES
    for nm in h.names:
        for fld in ("counts", "under", "over", "nan"):
            assert torch.equal(getattr(h, fld)[nm], getattr(i, fld)[nm])
        assert bool((h.total(nm) == h.n).all())
    a, b = t0.mcpc_last_autocovariance, t1.mcpc_last_autocovariance
    assert a.names == b.names == NAMES
    for nm in a.names:
        for fld in ("lagged", "sum", "head", "tail"):
            assert torch.equal(getattr(a, fld)[nm], getattr(b, fld)[nm])


def test_calls_that_are_not_fused_are_rejected():
    import montecarlopredictivecoding_amd.predictive_coding as pc
    um, model, data, inputs = _net(DEV)
    with pytest.raises(NotImplementedError, match="mcpc_rolling is set.*step by step.*update_p_at"):
        _call(um, model, data, inputs, dict(layers=(0,), window=4), update_p_at="all")
    assert all(m.get_x() is None for m in model if hasattr(m, "get_x"))              # before any work
    masked = torch.nn.Sequential(torch.nn.Linear(3, 3), pc.PCLayer(M=torch.ones(3, device=DEV)), torch.nn.Linear(3, 2)).to(DEV)
    masked.train()
    tr = pc.PCTrainer(masked, T=3, update_p_at="never", plot_progress_at=[])
    tr.mcpc_rolling = dict(layers=(0,), window=2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(NotImplementedError, match="mcpc_rolling is set.*generic torch loop.*S/M masks"):
            tr.train_on_batch(inputs=torch.zeros(2, 3, device=DEV), is_log_progress=False, is_return_results_every_t=False)
    # a bad request on a call that would be fused: ValueError, before any work
    with pytest.raises(ValueError, match="layer index"):
        _call(um, model, data, inputs, dict(layers=(3,), window=4))
    with pytest.raises(ValueError, match="window is required"):
        _call(um, model, data, inputs, dict(layers=(0,)))
    from montecarlopredictivecoding_amd.rolling import request_bytes
    need = request_bytes((("x0", 5), ("x2", 9), ("out", 14)), B, W, T, T - W + 1, None)
    with pytest.raises(ValueError, match=r"mcpc_rolling_max_bytes.*a shorter window, fewer layers or a larger every"):
        _call(um, model, data, inputs, dict(SPEC), max_bytes=need - 1)
    assert all(m.get_x() is None for m in model if hasattr(m, "get_x"))
    tr, _ = _call(um, model, data, inputs, dict(SPEC), max_bytes=need, xs=False, outputs=False)
    assert tr.mcpc_last_rolling.rows == T - W + 1


def test_cpu_built_model(reference_call):
    um, model, data, inputs = _net("cpu")
    cpu = _call(um, model, data, inputs, dict(SPEC), xs=False, outputs=False)[0].mcpc_last_rolling
    dev = reference_call[0]
    assert all(cpu.sums[nm].device.type == "cpu" and cpu.var[nm].device.type == "cpu" for nm in NAMES)
    assert cpu.state[0]["hist"].device.type == "cuda"                                    # the state stays on the engine's device
    for nm in NAMES:
        assert torch.equal(cpu.sums[nm], dev.sums[nm].cpu()) and torch.equal(cpu.var[nm], dev.var[nm].cpu())


def _figure_setup():
    import montecarlopredictivecoding_amd.utils.model as um
    from montecarlopredictivecoding_amd.utils.training_evaluation import get_mcpc_trainer, get_pc_trainer
    torch.manual_seed(5)
    cfg = dict(input_size=SIZES[0], hidden_size=SIZES[1], hidden2_size=SIZES[2], output_size=N_OUT, activation_fn="relu",
               loss_fn=um.bernoulli_fn, input_var=0.3, T_pc=40, optimizer_x_fn_pc=torch.optim.Adam, optimizer_x_kwargs_pc={"lr": 0.1},
               mixing=0, sampling=40, optimizer_x_kwargs_mcpc={"lr": 0.03},
               optimizer_p_fn_mcpc=torch.optim.Adam, optimizer_p_kwargs_mcpc={"lr": 0.01})
    model = um.get_model(cfg, True, sample_x_fn=um.sample_x_fn_normal)
    g = torch.Generator().manual_seed(2)
    data = (torch.rand(16, N_OUT, generator=g) < 0.3).float()
    trainers = [get_pc_trainer(model, cfg, is_mcpc=True, training=False), get_mcpc_trainer(model, cfg, training=False)]
    return um, cfg, model, data, trainers


def test_get_variability_time_course_is_the_four_calls_made_by_hand():
    import montecarlopredictivecoding_amd.predictive_coding.pc_trainer as pt
    from montecarlopredictivecoding_amd.rolling import Rolling
    um, cfg, model, data, trainers = _figure_setup()
    base = pt._PHILOX_STEPS[0]
    trainers[1].mcpc_rolling = "kept"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(7)
        r = um.get_variability_time_course(model, cfg, trainers, data, window=W, every=2, layers=(0, 2))
    assert trainers[1].mcpc_rolling == "kept"                                            # the previous setting is back
    n = 40                                                                               # T of the MCPC trainer: config["sampling"]
    assert trainers[1].get_T() == n
    assert r.names == ["x0", "x2"] and r.B == 16 and r.T == 2 * n and r.n_seen == 2 * n and r.var == {}
    assert r.steps.tolist() == list(range(W - 1, 2 * n, 2)) and bool((r.count("x0") == 16 * 5).all())
    a = r.all()
    assert a.names == ["all"] and bool((a.count("all") == 16 * 14).all())
    assert bool(torch.isfinite(a.mean_std("all")).all()) and bool((a.mean_std("all") > 0).all()) and bool((a.sem("all") > 0).all())
    # by hand, replaying the same noise and the same initial x
    pt._PHILOX_STEPS[0] = base
    pc_tr, mc_tr = trainers
    dev = next(model.parameters()).device
    zeros = torch.zeros(16, SIZES[0], device=dev)
    quiet = dict(is_log_progress=False, is_return_results_every_t=False, is_checking_after_callback_after_t=False)
    mc = dict(callback_after_t=um.random_step, callback_after_t_kwargs={"_pc_trainer": mc_tr}, is_sample_x_at_batch_start=False)
    request = dict(begin=0, stride=1, layers=(0, 2), outputs=None, window=W, every=2, pool="all")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(7)
        mc_tr.mcpc_rolling = None
        pc_tr.train_on_batch(inputs=zeros, **quiet)
        mc_tr.train_on_batch(inputs=zeros, **mc, **quiet)
        mc_tr.mcpc_rolling = dict(request)
        mc_tr.train_on_batch(inputs=zeros, loss_fn=um.zero_fn, loss_fn_kwargs={}, **mc, **quiet)
        before = mc_tr.mcpc_last_rolling
        mc_tr.mcpc_rolling = dict(request, carry=before)
        mc_tr.train_on_batch(inputs=zeros, loss_fn=cfg["loss_fn"], loss_fn_kwargs={"_target": data.to(dev), "_var": cfg["input_var"]},
                             **mc, **quiet)
        after = mc_tr.mcpc_last_rolling
    mc_tr.mcpc_rolling = None
    pt._PHILOX_STEPS[0] = base
    hand = Rolling.cat([before, after])
    assert torch.equal(hand.steps, r.steps) and all(torch.equal(hand.sums[nm], r.sums[nm]) for nm in r.names)
    assert before.rows == len(range(W - 1, n, 2)) and after.steps[0] == (1 if (n - (W - 1)) % 2 else 0)
